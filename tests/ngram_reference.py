"""TEST INFRASTRUCTURE ONLY - two references for the back-off n-gram LM (src/ngram.py, csrc/ngram.hip), sharing no
code with either:

* a float64, dict-based scorer and state function written from the definition: p(w | h) is the explicit entry of
  h.w if the model has one, else bo(h) + p(w | h without its oldest token), bo = 0 for a context the model does not
  hold; at the unigram level a word without a unigram has the constant ln(10) * -99 (back-off weights collected on
  the way down add to it as to any other unigram value - the kernel's step 3 does the same for every v).  The
  state after a history is its longest suffix of at most n - 1 tokens that the model holds as an n-gram of order
  < n; a token without a unigram, fed as context, leads to the empty context.
* `emulate_f32`: the kernel's four steps (advance, chain, fill, overwrite) restated in numpy float32 on the flat
  image - what the device must reproduce bit for bit.
"""
import gzip
import math

import numpy as np

LN10 = math.log(10.0)
UNSEEN = LN10 * -99.0
_SPECIAL = {'<s>': 0, '</s>': 1, '<unk>': 2}


class Model:
    def __init__(self, order, vocab_size, prob, bo):
        self.order, self.V, self.prob, self.bo = order, vocab_size, prob, bo
        self._rows = {}


def read_arpa(path, vocab_size):
    """a reader for well-formed files only (the product's parser is the one under test for everything else)"""
    prob, bo, k = {}, {}, 0
    opener = gzip.open if str(path).endswith('.gz') else open
    with opener(path, 'rt') as f:
        for line in f:
            line = line.strip()
            if line.endswith('-grams:'):
                k = int(line[1:].split('-')[0])
            elif line == '\\end\\':
                break
            elif k and line:
                fs = line.split()
                g = tuple(_SPECIAL[w] if w in _SPECIAL else int(w) for w in fs[1:k + 1])
                prob[g] = float(fs[0]) * LN10
                if len(fs) > k + 1:
                    bo[g] = float(fs[k + 1]) * LN10
    return Model(max(len(g) for g in prob), vocab_size, prob, bo)


def from_tables(order, grams, vocab_size):
    """a Model from per-order {tuple: (ln p, ln bo)} tables in float64"""
    prob = {g: v[0] for t in grams for g, v in t.items()}
    bo = {g: v[1] for t in grams for g, v in t.items()}
    return Model(order, vocab_size, prob, bo)


def image_contexts(image):
    """node id -> context tuple of a flat image, by walking it from the unigram level"""
    order, V = int(image['order']), int(image['vocab_size'])
    ctx = {0: ()}
    frontier = []
    for w in range(V):
        s = int(image['uni_next'][w])
        if s != 0:
            ctx[s] = (w,)
            frontier.append(s)
    for length in range(1, order - 1):
        nxt = []
        for s in frontier:
            for e in range(int(image['child_off'][s]), int(image['child_off'][s + 1])):
                t = int(image['next'][e])
                ctx[t] = ctx[s] + (int(image['word'][e]),)
                nxt.append(t)
        frontier = nxt
    return ctx


def from_image(image):
    """the n-grams a flat image holds, as a Model (float32 values widened to float64)"""
    order, V = int(image['order']), int(image['vocab_size'])
    ctx = image_contexts(image)
    prob, bo = {}, {}
    unseen32 = np.float32(UNSEEN)
    for w in range(V):
        if int(image['uni_next'][w]) != 0 or image['uni_logp'][w] != unseen32:
            prob[(w,)] = float(image['uni_logp'][w])
    for s, h in ctx.items():
        if s == 0:
            continue
        bo[h] = float(image['bo'][s])
        for e in range(int(image['child_off'][s]), int(image['child_off'][s + 1])):
            prob[h + (int(image['word'][e]),)] = float(image['logp'][e])
    return Model(order, V, prob, bo)


def terms(m, h, w):
    """the float64 terms whose sum is ln p(w | h): back-off weights from the longest context down, then the entry"""
    h = tuple(h)[-(m.order - 1):] if m.order > 1 else ()
    g = h + (int(w),)
    out = []
    while True:
        if g in m.prob:
            out.append(m.prob[g])
            return out
        if len(g) == 1:
            out.append(UNSEEN)
            return out
        out.append(m.bo.get(g[:-1], 0.0))
        g = g[1:]


def logp(m, h, w):
    acc = 0.0
    for t in terms(m, h, w):
        acc += t
    return acc


def state(m, h):
    h = tuple(h)[-(m.order - 1):] if m.order > 1 else ()
    while h and h not in m.prob:
        h = h[1:]
    return h


def advance(m, st, token):
    if (int(token),) not in m.prob:
        return ()
    return state(m, tuple(st) + (int(token),))


def row(m, h):
    h = state(m, h)
    if h not in m._rows:
        m._rows[h] = np.array([logp(m, h, w) for w in range(m.V)], np.float64)
    return m._rows[h]


def f64_lm_step(m):
    """lm_step(token, hidden) for the search oracles: hidden is the state as a tuple of tokens"""
    def step(token, hidden):
        st = advance(m, () if hidden is None else hidden, token)
        return row(m, st), st
    return step


# ---- the kernel's arithmetic in numpy float32 ---------------------------------------------------------------------
def emulate_advance(image, s, token):
    V = int(image['vocab_size'])
    if not 0 <= token < V:
        return 0
    off, word = image['child_off'], image['word']
    while s != 0:
        lo, hi = int(off[s]), int(off[s + 1])
        j = lo + int(np.searchsorted(word[lo:hi], token))
        if j < hi and word[j] == token:
            return int(image['next'][j])
        s = int(image['fail'][s])
    return int(image['uni_next'][token])


def emulate_chain(image, s):
    c, B = [s], [np.float32(0.0)]
    while c[-1] != 0:
        B.append(np.float32(B[-1] + image['bo'][c[-1]]))
        c.append(int(image['fail'][c[-1]]))
    return c, B


def emulate_f32(image, s, token):
    """-> (new state, row [V] float32): steps 1-4 of the kernel"""
    ns = emulate_advance(image, int(s), int(token))
    c, B = emulate_chain(image, ns)
    d = len(c) - 1
    out = (B[d] + image['uni_logp']).astype(np.float32)
    assert image['uni_logp'].dtype == np.float32 and out.dtype == np.float32
    off = image['child_off']
    for k in range(d - 1, -1, -1):
        lo, hi = int(off[c[k]]), int(off[c[k] + 1])
        out[image['word'][lo:hi]] = B[k] + image['logp'][lo:hi]
    return ns, out


def f32_lm_step(image):
    """lm_step(token, hidden) made from emulate_f32: hidden is the int state"""
    cache = {}

    def step(token, hidden):
        key = (0 if hidden is None else int(hidden), int(token))
        if key not in cache:
            cache[key] = emulate_f32(image, *key)
        ns, r = cache[key]
        return r, ns
    return step
