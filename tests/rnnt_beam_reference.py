"""TEST INFRASTRUCTURE ONLY - float64 reference of the transducer beam search (alignment-length synchronous, Saon et al.
2020) as TransducerHead.beam_search defines it, one utterance at a time, on rnnt_reference.HeadRef:

 * lae            the float64 logaddexp of csrc/rnnt_beam.inc restated operation for operation (+, -, *, / only), so that
                  the host build, the kernel and this file agree to the bit
 * select_step    one iteration on a [W, K+1] table: candidates (slot ascending, blank first, labels by rank), merge of
                  equal sequences, cut to W, finished list; plain python on tuples and dicts, sharing no code with the .inc
 * beam_search    the search with the decision margins of every iteration and what the case conditions ask about
 * random_tables  the tables and beams the host build and the kernel are run on (planted merges, ties, -inf, dead and
                  capped slots)
"""
import math

import numpy as np
import torch

NEG = float("-inf")


def lae(a, b):
    m = a if a > b else b
    if m == NEG:
        return m
    t = a - b if a > b else b - a
    if not t < 40.0:
        return m
    nf = math.floor(t * 1.4426950408889634 + 0.5)
    x = -((t - nf * 0.693147180369123816490) - nf * 1.90821492927058770002e-10)
    p = 1.0
    for j in range(14, 0, -1):
        p = 1.0 + (x / float(j)) * p
    sc, hf, n = 1.0, 0.5, int(nf)
    while n > 0:
        if n & 1:
            sc = sc * hf
        hf = hf * hf
        n >>= 1
    u = p * sc
    s = u / (2.0 + u)
    s2 = s * s
    q = 0.0
    for j in range(19, -1, -1):
        q = 1.0 / float(2 * j + 1) + s2 * q
    return m + (2.0 * s) * q


class Hyp:
    __slots__ = ("tok", "t", "n_sym", "s", "parent", "emit", "last")

    def __init__(self, tok=(), t=0, n_sym=0, s=0.0, parent=0, emit=0, last=0):
        self.tok, self.t, self.n_sym, self.s, self.parent, self.emit, self.last = tuple(tok), t, n_sym, s, parent, emit, last

    def key(self):
        return (self.tok, self.t, self.n_sym, self.s, self.parent, self.emit, self.last)


def select_step(beam, lpb, val, lab, W, K, Tb, max_symbols, max_len, fin, combine=lae):
    """beam: the live Hyps in slot order; lpb [n], val / lab [n][K] python numbers; fin: [(tok, s)] sorted.
    -> (next beam in slot order, next finished list, info)"""
    cands = {}                                   # token tuple -> [position, score, Hyp fields of the better constituent]
    n_merge = 0
    unmerged = []
    for h, hyp in enumerate(beam):
        ext = [(h * (K + 1), Hyp(hyp.tok, hyp.t + 1, 0, hyp.s + lpb[h], h, 0, 0))]
        if hyp.n_sym < max_symbols and len(hyp.tok) < max_len:
            for c in range(K):
                if lab[h][c] >= 0:
                    ext.append((h * (K + 1) + 1 + c,
                                Hyp(hyp.tok + (int(lab[h][c]),), hyp.t, hyp.n_sym + 1, hyp.s + val[h][c], h, 1,
                                    int(lab[h][c]))))
        for pos, c in ext:
            unmerged.append((pos, c))
            if c.tok in cands:
                first = cands[c.tok]
                a, b = first[1], c.s
                first[1] = combine(a, b)
                if not a >= b:
                    first[2] = c
                n_merge += 1
            else:
                cands[c.tok] = [pos, c.s, c]
    merged = sorted(cands.values(), key=lambda e: e[0])
    ranked = sorted(merged, key=lambda e: -e[1] if e[1] == e[1] else NEG)      # stable: ties in candidate order
    kept = ranked[:W]
    # would the cut differ if equal sequences kept the better score instead of the sum?
    best = {}
    for pos, c in unmerged:
        if c.tok not in best:
            best[c.tok] = [pos, c.s]
        elif c.s > best[c.tok][1]:
            best[c.tok][1] = c.s
    alt = sorted(sorted(best.items(), key=lambda kv: kv[1][0]), key=lambda kv: -kv[1][1])[:W]
    info = dict(n_merge=n_merge, merge_changed_cut={e[2].tok for e in kept} != {k for k, _ in alt},
                cut_gap=(ranked[W - 1][1] - ranked[W][1]) if len(ranked) > W else None,
                capped=any(h.n_sym >= max_symbols and len(h.tok) < max_len for h in beam))
    nxt, finishers = [], []
    for e in kept:
        c = e[2]
        hyp = Hyp(_tok_of(e, beam, lab, K), c.t, c.n_sym, e[1], c.parent, c.emit, c.last)
        (finishers if hyp.t >= Tb else nxt).append(hyp)
    union = list(fin) + [(h.tok, h.s) for h in finishers]
    union = sorted(union, key=lambda f: -f[1])                                   # stable: the earlier entry first
    info["fin_overflow"] = len(union) > W
    return nxt, union[:W], info


def _tok_of(entry, beam, lab, K):
    """the token sequence of the candidate at entry's POSITION (equal to the sequence of its better constituent)"""
    pos = entry[0]
    h, c = divmod(pos, K + 1)
    return beam[h].tok + ((int(lab[h][c - 1]),) if c else ())


def fin_gaps(fin):
    return [fin[i][1] - fin[i + 1][1] for i in range(len(fin) - 1)]


@torch.no_grad()
def beam_search(ref, enc, W, max_symbols, max_len, lm_row=None, lm_weight=0.0, blank=0, dump=None, lp_fn=None):
    """one utterance enc [T, D] float64 on HeadRef `ref`; lm_row(tokens) -> float64 [V] LM log-probabilities after
    <sos> + tokens, or None.  -> (finished list [(tokens, score)], trace): trace holds per iteration the info of
    select_step plus row_gap (the smallest gap between the K-th and (K+1)-th label of a row), and `done_at`, the
    iteration after which no hypothesis is live.  dump: {iteration: list} receives (tok, t, n_sym, s) of the live beam
    AFTER that iteration.  lp_fn(tokens, t) -> float64 [V] replaces the head's own log-probabilities (the tests'
    "existing device path": the same search on log-probabilities computed elsewhere)."""
    assert blank == 0
    T = enc.shape[0]
    V = ref.lin_out.out_features
    K = min(W, V - 1)
    fe = ref.lin_enc(enc)
    cache = {}

    def pred(tok):
        if tok not in cache:
            if not tok:
                out, st = ref.rnn(ref.emb(torch.tensor([[0]])), None)
            else:
                _, st0 = pred(tok[:-1])
                out, st = ref.rnn(ref.emb(torch.tensor([[tok[-1]]])), st0)
            cache[tok] = (ref.lin_pred(out[0, 0]), st)
        return cache[tok]

    beam, fin, trace, done_at, max_lp = [Hyp()], [], [], None, 0.0
    for i in range(T + max_len):
        if not beam:
            continue
        lpb, val, lab, row_gap = [], [], [], None
        for hyp in beam:
            assert hyp.t + len(hyp.tok) == i
            if lp_fn is None:
                z = ref.lin_out(torch.tanh(fe[hyp.t] + pred(hyp.tok)[0]))
                lp = z - torch.logsumexp(z, dim=0)
            else:
                lp = lp_fn(hyp.tok, hyp.t)
            max_lp = max(max_lp, float(lp[blank].abs()))
            r = lp.clone()
            if lm_row is not None:
                r = r + lm_weight * torch.as_tensor(lm_row(hyp.tok), dtype=torch.float64)
            r[blank] = NEG
            order = sorted(range(V), key=lambda k: (-float(r[k]), k))
            order = [k for k in order if k != blank]
            lpb.append(float(lp[blank]))
            lab.append(order[:K])
            val.append([float(r[k]) for k in order[:K]])
            max_lp = max([max_lp] + [abs(float(lp[k])) for k in order[:K]])
            if len(order) > K and hyp.n_sym < max_symbols and len(hyp.tok) < max_len:
                g = float(r[order[K - 1]] - r[order[K]])
                row_gap = g if row_gap is None else min(row_gap, g)
        beam, fin, info = select_step(beam, lpb, val, lab, W, K, T, max_symbols, max_len, fin)
        info["row_gap"] = row_gap
        info["iteration"] = i
        trace.append(info)
        if dump is not None and i in dump:
            dump[i] = [(h.tok, h.t, h.n_sym, h.s) for h in beam]
        if not beam and done_at is None:
            done_at = i
    assert not beam and fin
    return fin, dict(steps=trace, done_at=done_at, fin_gaps=fin_gaps(fin), max_lp=max_lp)


def min_margin(trace):
    """the smallest decision margin of a search: cut gaps, row gaps and the gaps inside the finished list"""
    gaps = [s["cut_gap"] for s in trace["steps"] if s["cut_gap"] is not None]
    gaps += [s["row_gap"] for s in trace["steps"] if s["row_gap"] is not None]
    gaps += trace["fin_gaps"]
    return min(gaps) if gaps else float("inf")


# ---- tables for the select step of the host build and of the kernel ------------------------------------------------------
def random_tables(W, seed, B=6, V=40, T=7, max_len=5, max_symbols=2):
    """a batch of B utterances for ONE select step: numpy arrays in the layout of asrk_rnnt_beam_select (state arrays
    [2, B, ...], buffer 0 current) with, spread over the utterances: a planted merge whose sum changes the cut where W
    allows one, exact score ties, -inf values, missing labels, dead slots, slots at the max_symbols / max_len cap,
    slots whose blank finishes, and a finished list that is partly or completely full (so that it overflows)."""
    rng = np.random.RandomState(seed)
    K = min(W, V - 1)
    Lc = max(max_len, 1)
    n_live = np.zeros((2, B), np.int32)
    t_ptr = np.zeros((2, B, W), np.int32)
    n_sym = np.zeros((2, B, W), np.int32)
    n_tok = np.zeros((2, B, W), np.int32)
    score = np.zeros((2, B, W), np.float64)
    tokens = np.zeros((2, B, W, Lc), np.int32)
    fin_n = np.zeros((2, B), np.int32)
    fin_len = np.zeros((2, B, W), np.int32)
    fin_score = np.zeros((2, B, W), np.float64)
    fin_tok = np.zeros((2, B, W, Lc), np.int32)
    lpb = np.zeros((B, W), np.float32)
    val = np.full((B, W, K), -np.inf, np.float32)
    lab = np.full((B, W, K), -1, np.int32)
    enc_len = np.zeros((B,), np.int64)
    for b in range(B):
        Tb = int(rng.randint(1, T + 1))
        enc_len[b] = Tb
        i = int(rng.randint(0, Tb + max_len)) if b else 0           # the iteration: t + len = i for every live row
        nl = 1 if (b == 0 or i == 0) else int(rng.randint(0 if b == 1 else 1, W + 1))
        seen = set()
        rows = []
        for _ in range(nl * 8):
            if len(rows) == nl:
                break
            ln = int(rng.randint(max(0, i - Tb + 1), min(max_len, i) + 1)) if i - Tb + 1 <= min(max_len, i) else None
            if ln is None:
                break
            tok = tuple(int(x) for x in rng.randint(1, 5, size=ln))   # few symbols: prefixes of each other are common
            if tok in seen:
                continue
            seen.add(tok)
            rows.append(tok)
        rows.sort(key=lambda tk: (rng.rand(), tk))
        nl = len(rows)
        n_live[0, b] = nl
        for h, tok in enumerate(rows):
            n_tok[0, b, h] = len(tok)
            tokens[0, b, h, :len(tok)] = tok
            t_ptr[0, b, h] = i - len(tok)
            n_sym[0, b, h] = int(rng.randint(0, max_symbols + 1))       # == max_symbols: capped
            score[0, b, h] = -float(rng.randint(0, 40)) * 0.25            # a coarse grid: exact ties occur
            lpb[b, h] = np.float32(-float(rng.randint(0, 12)) * 0.25)
            if rng.rand() < 0.1:
                lpb[b, h] = -np.inf
            nk = K if rng.rand() < 0.7 else int(rng.randint(0, K + 1))   # missing labels at the end
            labels = rng.permutation(np.arange(1, V))[:nk]
            vals = np.sort(-rng.randint(0, 16, size=nk).astype(np.float32) * 0.25)[::-1].copy()
            if nk and rng.rand() < 0.1:
                vals[-1] = -np.inf
            lab[b, h, :nk] = labels
            val[b, h, :nk] = vals
        # planted merges: where row h spells row g plus one token, make that token a label of g
        for h in range(nl):
            for g in range(nl):
                if len(rows[h]) == len(rows[g]) + 1 and rows[h][:-1] == rows[g] and rng.rand() < 0.8:
                    k = rows[h][-1]
                    if k not in lab[b, g] and lab[b, g, 0] >= 0:
                        c = int(rng.randint(0, int((lab[b, g] >= 0).sum())))
                        lab[b, g, c] = k
        if b == 2 and W >= 2:
            # the planted case: rows (1) and (1, 2); blank of the second and label 2 of the first both score -1.0 and
            # sum to -0.307, ahead of the first row's other W - 1 labels (-0.5, exact ties) and of (1, 2, 5) at -0.5, which
            # the cut drops on the tie in candidate order - without the sum, (1, 2) at -1.0 would be dropped instead
            enc_len[b] = 5
            n_live[0, b] = 2
            n_tok[0, b, :2] = (1, 2)
            tokens[0, b, 0, :1] = (1,)
            tokens[0, b, 1, :2] = (1, 2)
            t_ptr[0, b, :2] = (2, 1)
            n_sym[0, b, :2] = 0
            score[0, b, :2] = (0.0, -0.75)
            lpb[b, :2] = (-4.0, -0.25)
            lab[b, 0] = list(range(3, 3 + K - 1)) + [2]
            val[b, 0] = [-0.5] * (K - 1) + [-1.0]
            lab[b, 1] = [5] + list(range(6, 6 + K - 1))
            val[b, 1] = [0.25] + [-3.0] * (K - 1)
        nf = int(rng.randint(0, W + 1)) if b % 2 else W
        fin_n[0, b] = nf
        fs = np.sort(-rng.randint(0, 40, size=nf).astype(np.float64) * 0.25)[::-1]
        for j in range(nf):
            ln = int(rng.randint(0, max_len + 1))
            fin_len[0, b, j] = ln
            fin_tok[0, b, j, :ln] = rng.randint(1, V, size=ln)
            fin_score[0, b, j] = fs[j]
    return dict(B=B, T=T, W=W, K=K, V=V, max_len=max_len, max_symbols=max_symbols, enc_len=enc_len, lpb=lpb, val=val,
                lab=lab, n_live=n_live, t_ptr=t_ptr, n_sym=n_sym, n_tok=n_tok, score=score, tokens=tokens, fin_n=fin_n,
                fin_len=fin_len, fin_score=fin_score, fin_tok=fin_tok,
                parent=np.zeros((B * W,), np.int64), last_tok=np.zeros((B * W,), np.int64),
                emit=np.zeros((B * W,), np.int32), sel=np.zeros((B * W,), np.int64), lm_sel=np.zeros((B * W,), np.int64))


def select_tables_reference(tb):
    """select_step on every utterance of random_tables' batch -> per utterance a dict of what the kernel must write
    into buffer 1 and into the gather outputs, plus the info of the step"""
    out = []
    B, W, K = tb["B"], tb["W"], tb["K"]
    for b in range(B):
        nl = int(tb["n_live"][0, b])
        beam = [Hyp(tb["tokens"][0, b, h, :tb["n_tok"][0, b, h]].tolist(), int(tb["t_ptr"][0, b, h]),
                    int(tb["n_sym"][0, b, h]), float(tb["score"][0, b, h])) for h in range(nl)]
        fin = [(tuple(tb["fin_tok"][0, b, j, :tb["fin_len"][0, b, j]].tolist()), float(tb["fin_score"][0, b, j]))
               for j in range(int(tb["fin_n"][0, b]))]
        Tb = min(max(int(tb["enc_len"][b]), 1), tb["T"])
        nxt, fin2, info = select_step(beam, [float(x) for x in tb["lpb"][b]], tb["val"][b].astype(np.float64).tolist(),
                                      tb["lab"][b].tolist(), W, K, Tb, tb["max_symbols"], tb["max_len"], fin)
        out.append(dict(beam=nxt, fin=fin2, info=info))
    return out


def check_select_output(tb, ref):
    """asserts that buffer 1 and the gather outputs of `tb` (after the host build or the kernel ran on it with cur = 0)
    equal the reference's select step exactly"""
    B, W = tb["B"], tb["W"]
    rows = B * W
    for b in range(B):
        nxt, fin = ref[b]["beam"], ref[b]["fin"]
        assert int(tb["n_live"][1, b]) == len(nxt), (b, int(tb["n_live"][1, b]), len(nxt))
        for r in range(W):
            g = b * W + r
            if r < len(nxt):
                h = nxt[r]
                got = (tuple(tb["tokens"][1, b, r, :tb["n_tok"][1, b, r]].tolist()), int(tb["t_ptr"][1, b, r]),
                       int(tb["n_sym"][1, b, r]), float(tb["score"][1, b, r]), int(tb["parent"][g]) - b * W,
                       int(tb["emit"][g]), int(tb["last_tok"][g]))
                assert got == h.key(), (b, r, got, h.key())
                assert int(tb["sel"][g]) == g + h.emit * rows
                assert int(tb["lm_sel"][g]) == (rows + g if h.emit else b * W + h.parent)
            else:
                assert (int(tb["parent"][g]), int(tb["emit"][g]), int(tb["last_tok"][g]), int(tb["sel"][g]),
                        int(tb["lm_sel"][g]), int(tb["n_tok"][1, b, r])) == (g, 0, 0, g, g, 0), (b, r)
        assert int(tb["fin_n"][1, b]) == len(fin), (b, int(tb["fin_n"][1, b]), len(fin))
        for j, (tok, s) in enumerate(fin):
            got = (tuple(tb["fin_tok"][1, b, j, :tb["fin_len"][1, b, j]].tolist()), float(tb["fin_score"][1, b, j]))
            assert got == (tok, s), (b, j, got, (tok, s))


# ---- the cases of the search comparison --------------------------------------------------------------------------------------
BEAM_WIDTHS = (2, 4)
BEAM_LM_WEIGHT = 0.3
MIN_MARGIN = 1e-3
# (prediction network, layers, seed, blank bias) of rnnt_reference.greedy_case: seeds for which the float64 reference
# alone meets check_beam_cases (chosen on the CPU, tests/test_rnnt_beam_cpu.py)
BEAM_CASES = [("LSTM", 1, 6, 0.5), ("GRU", 2, 0, 0.5)]


def planted_lm(V, seed):
    """a small bigram model over the V tokens: -> (order, grams) with grams[k-1] = {k-tuple: (ln p, ln back-off)} in
    float64, every token with a unigram, some forty bigrams (contexts <s> = 0 among them)"""
    rng = np.random.RandomState(seed)
    uni = rng.randn(V) * 1.5
    uni = uni - np.log(np.exp(uni).sum())
    g1 = {(w,): (float(uni[w]), float(-0.5 * rng.rand())) for w in range(V)}
    g2 = {}
    for _ in range(40):
        a, b = int(rng.randint(0, V)), int(rng.randint(1, V))
        g2[(a, b)] = (float(-3.0 * rng.rand()), 0.0)
    return 2, [g1, g2]


def planted_lm_model(ngram_module, ngram_reference, V, seed):
    """-> (image for NGramLM, lm_row(tokens) -> float64 [V] after <sos> + tokens) of planted_lm; the rows hold the image's
    float32 values, the inputs the device sees"""
    order, grams = planted_lm(V, seed)
    image = ngram_module.build_image(order, grams, V)
    m = ngram_reference.from_image(image)
    return image, (lambda tok: ngram_reference.row(m, (0,) + tuple(tok)))


def run_case(ref, enc, lens, W, max_symbols, max_len, lm_row=None, lm_weight=0.0, dump=None, lp_fn=None):
    """beam_search on every utterance of a case -> [(finished list, trace)]; lp_fn(b) -> the lp_fn of utterance b"""
    return [beam_search(ref, enc[b, :int(lens[b])].double(), W, max_symbols, max_len, lm_row, lm_weight,
                        dump=None if dump is None else dump[b], lp_fn=None if lp_fn is None else lp_fn(b))
            for b in range(enc.shape[0])]


def case_facts(runs):
    """what check_beam_cases asks of the searches of one setting"""
    steps = [s for _, tr in runs for s in tr["steps"]]
    return dict(margin=min(min_margin(tr) for _, tr in runs), merges=sum(s["n_merge"] for s in steps),
                merge_changed_cut=any(s["merge_changed_cut"] for s in steps), capped=any(s["capped"] for s in steps),
                fin_overflow=any(s["fin_overflow"] for s in steps), done_at=[tr["done_at"] for _, tr in runs],
                best=[fin[0][0] for fin, _ in runs])
