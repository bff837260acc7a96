"""TEST INFRASTRUCTURE ONLY - two references for contextual biasing (src/bias.py, csrc/ctx_bias.hip), sharing no code
with either:

* `Ref`: the semantics restated from their definition on tuples and dicts in float64 - a node IS its token prefix,
  fail is "the longest proper suffix that is a trie path", goto is "the longest suffix of history + token that is a
  trie path", full / psi / phi / credit / arrive by their recursions; `delta` is the one float32 subtraction of the
  two float32-rounded values.
* `emulate_*`: the kernels' steps (binary search in the node's merged list, else the root tables; fill, overwrite)
  restated in numpy float32 on the flat image - what the device must reproduce bit for bit.
"""
import numpy as np


class Ref:
    def __init__(self, phrases, vocab_size, weight, scale=1.0):
        self.V = int(vocab_size)
        self.nodes, self.end, mult = {()}, set(), {}
        for p, m in phrases:
            p = tuple(int(t) for t in p)
            self.end.add(p)
            for k in range(1, len(p) + 1):
                self.nodes.add(p[:k])
                mult[p[:k]] = max(mult.get(p[:k], 0.0), float(m))
        self.e = {n: float(weight) * m * float(scale) for n, m in mult.items()}
        self._memo = {}

    def fail(self, n):
        for k in range(1, len(n) + 1):
            if n[k:] in self.nodes:
                return n[k:]
        return ()

    def goto(self, n, v):
        if not 0 <= int(v) < self.V:
            return ()
        h = tuple(n) + (int(v),)
        while h not in self.nodes:
            h = h[1:]
        return h

    def full(self, n):
        return 0.0 if not n else self.full(n[:-1]) + self.e[n]

    def psi(self, n):
        return 0.0 if not n else self.phi(n[:-1]) + self.e[n]

    def phi(self, n):
        return 0.0 if (not n or n in self.end) else self.psi(n)

    def credit(self, n):
        if not n or n in self.end:
            return 0.0
        f = self.fail(n)
        while f and f not in self.end:
            f = self.fail(f)
        return self.full(f) if f else 0.0

    def arrive(self, n):
        return 0.0 if not n else self.psi(n) + self.credit(n)

    def delta(self, n, v):
        """float32: one subtraction of the two stored (float32-rounded) values"""
        return np.float32(np.float32(self.arrive(self.goto(n, v))) - np.float32(self.phi(n)))

    def row(self, n):
        """float32 [V]: delta(n, v) for every v"""
        n = tuple(n)
        if n not in self._memo:
            self._memo[n] = np.array([self.delta(n, v) for v in range(self.V)], np.float32)
        return self._memo[n]

    def state(self, seq):
        n = ()
        for v in seq:
            n = self.goto(n, v)
        return n

    def walk(self, seq):
        """-> (final node, total, residual): total the float32 sum of the deltas in token order"""
        n, tot = (), np.float32(0.0)
        for v in seq:
            tot = np.float32(tot + self.delta(n, v))
            n = self.goto(n, v)
        return n, tot, np.float32(self.phi(n))

    def ids(self):
        """node -> id: breadth first, children in ascending token order"""
        return {n: i for i, n in enumerate(sorted(self.nodes, key=lambda n: (len(n), n)))}


def brute_goto(nodes, history, v):
    """the longest suffix of history + (v,) that is a trie path, by trying every suffix"""
    h = tuple(history) + (int(v),)
    for k in range(len(h) + 1):
        if h[k:] in nodes:
            return h[k:]
    raise AssertionError("the empty path is always a trie path")


# ---- the kernels' arithmetic in numpy float32 ---------------------------------------------------------------------
def emulate_goto(image, s, token):
    """-> (next state, arrive of it as float32)"""
    V, N = int(image['vocab_size']), len(image['phi'])
    if not 0 <= token < V:
        return 0, np.float32(0.0)
    if not 0 <= s < N:
        s = 0
    if s != 0:
        lo, hi = int(image['ext_off'][s]), int(image['ext_off'][s + 1])
        j = lo + int(np.searchsorted(image['ext_word'][lo:hi], token))
        if j < hi and image['ext_word'][j] == token:
            return int(image['ext_next'][j]), image['ext_arrive'][j]
    return int(image['root_next'][token]), image['root_arrive'][token]


def emulate_row(image, s):
    """float32 [V]: the row of state s - fill from the root tables, then the node's merged entries"""
    phi = image['phi'][s]
    out = (image['root_arrive'] - phi).astype(np.float32)
    assert image['root_arrive'].dtype == np.float32 and phi.dtype == np.float32
    if s != 0:
        lo, hi = int(image['ext_off'][s]), int(image['ext_off'][s + 1])
        out[image['ext_word'][lo:hi]] = image['ext_arrive'][lo:hi] - phi
    return out


def emulate_step(image, s, token):
    """-> (new state, row [V] float32) of asrk_bias_step_f32"""
    ns, _ = emulate_goto(image, int(s), int(token))
    return ns, emulate_row(image, ns)


def emulate_walk(image, seq):
    s, tot = 0, np.float32(0.0)
    for v in seq:
        ns, a = emulate_goto(image, s, int(v))
        tot = np.float32(tot + np.float32(a - image['phi'][s]))
        s = ns
    return s, tot, image['phi'][s]


def emulate_fused(ngram_reference, ng_image, b_image, sn, sb, token):
    """-> ((n-gram state, bias state), row): the n-gram's emulate_f32 row plus ONE float32 add of the bias row"""
    nn, lrow = ngram_reference.emulate_f32(ng_image, int(sn), int(token))
    nb, brow = emulate_step(b_image, int(sb), int(token))
    assert lrow.dtype == np.float32 and brow.dtype == np.float32
    return (nn, nb), (lrow + brow).astype(np.float32)


def image_nodes(image):
    """node id -> token prefix of a flat image, by walking it from the root (a child entry is the one whose target
    is one token deeper than the node)"""
    V = int(image['vocab_size'])
    path = {0: ()}
    frontier = []
    for v in range(V):
        c = int(image['root_next'][v])
        if c != 0:
            path[c] = (v,)
            frontier.append(c)
    while frontier:
        nxt = []
        for s in frontier:
            for e in range(int(image['ext_off'][s]), int(image['ext_off'][s + 1])):
                c = int(image['ext_next'][e])
                if c > s and c not in path:                 # breadth-first ids: a child is numbered after its parent
                    cand = path[s] + (int(image['ext_word'][e]),)
                    path[c] = cand
                    nxt.append(c)
        frontier = nxt
    return path
