"""TEST INFRASTRUCTURE ONLY - fixtures shared by the contextual-biasing tests (CPU and GPU): the worked examples of
DESIGN.md 3.27, seeded random phrase sets, and the phrase set that holds every shape the kernels can go wrong on."""
import importlib

import numpy as np

from conftest import PKG_NAME


def bias_mod():
    return importlib.import_module(PKG_NAME + ".src.bias")


# ---- the worked examples: every edge 1.0; sequence -> (total, residual) --------------------------------------------
WORKED_PHRASES = [((5, 6), 1.0), ((4, 5, 6, 7), 1.0), ((5, 6, 8, 9), 1.0), ((3,), 1.0)]
WORKED = [((4, 5, 6), 5, 3), ((4, 5, 6, 7), 6, 0), ((4, 5, 6, 1), 2, 0), ((4, 5, 6, 8), 3, 1), ((4, 5, 6, 8, 9), 4, 0),
          ((5, 6), 2, 0), ((5, 1), 0, 0), ((3, 3), 2, 0), ((4, 5, 1), 0, 0), ((4, 5, 5, 6), 2, 0)]


def random_phrases(seed, V=12, n=8, max_len=5):
    """n phrases over the ids 3 .. V - 1 from a small alphabet (so that prefixes, suffixes and whole phrases nest),
    a third of them with a multiplier of their own"""
    rng = np.random.RandomState(seed)
    alpha = np.arange(3, min(V, 3 + 4 + seed % 3))
    out = []
    for _ in range(n):
        p = tuple(int(t) for t in rng.choice(alpha, size=int(rng.randint(1, max_len + 1))))
        out.append((p, float(rng.choice([1.0, 1.0, 0.5, 2.5]))))
    return out


# ---- the kernels' fixture -------------------------------------------------------------------------------------------
BIG_NODE = (3,)                        # the node with min(300, V - 8) children: more entries than a workgroup has lanes
LONG = tuple(range(10, 22))            # a 12-token phrase: states at every depth up to 12
KERNEL_WEIGHT = 1.5


def kernel_phrases(V):
    """a node with up to 300 merged entries, a 12-token phrase, phrases nested in it (shorter phrases completing
    inside a longer partial match, entries inherited along fail chains of several hops), multipliers that differ on
    shared edges, a one-token phrase"""
    assert V >= 37
    big = [w for w in range(4, V)][:min(300, V - 8)]
    ph = [(BIG_NODE + (w,), 1.0 + 0.25 * (w % 3)) for w in big]
    ph += [(LONG, 1.0), (LONG[3:7], 2.0), (LONG[4:6], 0.5), (LONG[5:9] + (30,), 1.25), (LONG[8:10] + (31, 32), 1.0),
           (LONG[:2] + (33,), 3.0), ((LONG[1], 34), 0.75), ((35,), 1.0), (BIG_NODE + (LONG[0], LONG[1], 36), 0.3)]
    return ph


def kernel_rows(image, paths, n, seed=0):
    """n (state, token) pairs: first every node as the NEW state (every depth is reached; capped at n // 2, deepest
    first), then tokens outside [0, V), specials and breaking tokens from deep states, then random pairs"""
    rng = np.random.RandomState(seed)
    V, N = int(image['vocab_size']), len(image['phi'])
    node_of = {p: s for s, p in paths.items()}
    by_depth = {}
    for s, p in sorted(paths.items()):
        if s != 0:
            by_depth.setdefault(len(p), []).append((node_of[p[:-1]], p[-1]))
    rows, k = [], 0
    while len(rows) < max(1, n // 2) and any(k < len(v) for v in by_depth.values()):
        rows += [v[k] for _, v in sorted(by_depth.items(), reverse=True) if k < len(v)]
        k += 1
    rows = rows[:max(1, n // 2)]
    deep = node_of[LONG[:8]]
    rows += [(deep, -1), (deep, V), (deep, V + 5), (deep, -(2 ** 40)), (deep, 2 ** 40), (deep, 1), (deep, 0), (0, 0),
             (deep, 30), (deep, LONG[8]), (deep, 35), (node_of[BIG_NODE], 9), (node_of[BIG_NODE], 2)]
    while len(rows) < n:
        rows.append((int(rng.randint(N)), int(rng.randint(V))))
    rows = rows[:n]
    return np.array([r[0] for r in rows], np.int32), np.array([r[1] for r in rows], np.int64)


def walk_sequences(V, seed=0):
    """token rows for asrk_bias_walk: lengths 0, 1 and 40 among them, phrases embedded in noise"""
    rng = np.random.RandomState(seed)
    L = 40
    seqs = [[], [35], [5], list(LONG), list(LONG[:7]), list(LONG[3:7]) + [1] + list(LONG[:2]) + [33]]
    long40 = list(rng.randint(3, V, size=L))
    long40[5:17] = LONG
    long40[20:22] = [3, 7]
    long40[30:34] = LONG[3:7]
    seqs.append([int(t) for t in long40])
    seqs.append([int(t) for t in rng.randint(3, V, size=L)])
    seqs.append([3, 4, -1, 3, V, 3, 5])
    for _ in range(8):
        seqs.append([int(t) for t in rng.choice(list(LONG) + [3, 30, 33, 35], size=int(rng.randint(2, L)))])
    tok = np.zeros((len(seqs), L), np.int64)
    for i, s in enumerate(seqs):
        tok[i, :len(s)] = s
    tok[0, :] = LONG[0]                                     # beyond n_tok: never read
    return tok, np.array([len(s) for s in seqs], np.int32)


# ---- the searches ---------------------------------------------------------------------------------------------------
def f32_step(bias_reference, image):
    """lm_step(token, hidden) for the CTC search oracle from the image's float32 restatement: hidden is the node"""
    def step(token, hidden):
        ns, row = bias_reference.emulate_step(image, 0 if hidden is None else int(hidden), int(token))
        return row, ns
    return step


def search_phrases(V, seed=5, n=14):
    """phrases over 3 .. V - 3 for the CTC search cases (ngram_cases.search_posteriors spikes on these ids): one to three
    tokens, some sharing prefixes, two with a multiplier"""
    rng = np.random.RandomState(seed)
    out = []
    for i in range(n):
        p = tuple(int(t) for t in rng.randint(3, V - 2, size=int(rng.randint(1, 4))))
        out.append((p, 2.0 if i % 5 == 0 else 1.0))
    out += [(out[1][0] + (7,), 1.0), (out[2][0][:1] + (9, 11), 1.0)]
    return out


PLANTED_PHRASE = (8, 5, 9, 6)


def planted_ctc(V, T=12):
    """[T, V] float32 log-probabilities: every third frame emits, token a_i best and PLANTED_PHRASE[i] the runner-up
    0.4 below it; every other frame is blank.  -> (posteriors, the unbiased search's output)"""
    best = (4, 10, 3, 7)
    x = np.full((T, V), -4.0, np.float32)
    x[:, 0] = 6.0
    for i, (a, p) in enumerate(zip(best, PLANTED_PHRASE)):
        t = 1 + 3 * i
        x[t, 0], x[t, a], x[t, p] = -2.0, 6.0, 5.6
    x = x - np.log(np.exp(x.astype(np.float64)).sum(1, keepdims=True)).astype(np.float32)
    return x, list(best)


def planted_rnnt_head(head_cls, V=11, enc_dim=16):
    """a transducer head whose output depends on the encoder frame alone (lin_pred is zero, lin_enc the identity):
    frame i makes label a_i the best and PLANTED_PHRASE[i] the runner-up 0.4 below it, blank far below; with
    max_symbols = 1 every frame emits once.  -> (head, enc [1, 4, enc_dim], lens, the unbiased output)"""
    import torch
    best = (4, 10, 3, 7)
    head = head_cls(V, enc_dim, dict(module='LSTM', dim=12, layer=1, emb_dim=8, dropout=0), enc_dim)
    with torch.no_grad():
        for lin in (head.lin_pred, head.lin_enc, head.lin_out):
            lin.weight.zero_()
            lin.bias.zero_()
        head.lin_enc.weight.copy_(torch.eye(enc_dim))
        for i, (a, p) in enumerate(zip(best, PLANTED_PHRASE)):
            head.lin_out.weight[a, i], head.lin_out.weight[p, i] = 8.0, 7.6
    enc = torch.zeros((1, 4, enc_dim))
    for i in range(4):
        enc[0, i, i] = 4.0                                  # tanh(4) = 0.9993: the logits are 8 and 7.6 times that
    return head, enc, torch.tensor([4]), list(best)


# transducer search cases on the seeded heads of rnnt_beam_reference / rnnt_stateless_reference (V = 11): chosen on the
# CPU so that the float64 reference alone has every decision margin (the corrected finished lists included) above
# rnnt_beam_reference.MIN_MARGIN in all eight settings (tests/test_bias_cpu.py asserts at least three of every four),
# finished hypotheses stop inside a phrase and the correction changes the order of finished lists
RNNT_PHRASES = [((5, 8, 3), 1.0), ((4, 7), 1.0), ((9, 9, 8), 1.0), ((10, 9), 2.0), ((7, 7, 4, 6), 1.0),
                ((5, 5, 9, 8, 10), 1.0), ((3,), 1.0)]
RNNT_WEIGHT = 0.5
RNNT_SETTINGS = [(head, W, with_ngram) for head in ("LSTM", "stateless") for W in (1, 4) for with_ngram in (False, True)]


def rnnt_scorer_rows(bias_reference, ngram_row, V, lm_weight):
    """-> (lm_row(tokens) float64 [V], residual(tokens) float, the weight the search multiplies rows by): bias alone
    (ngram_row None: weight 1) or the n-gram's float64 row plus the bias row of the image scaled by 1 / lm_weight"""
    if ngram_row is None:
        ref = bias_reference.Ref(RNNT_PHRASES, V, RNNT_WEIGHT)
        return (lambda tok: ref.row(ref.state(tok)).astype(np.float64)), \
            (lambda tok: float(np.float32(ref.phi(ref.state(tok))))), 1.0
    ref = bias_reference.Ref(RNNT_PHRASES, V, RNNT_WEIGHT, 1.0 / lm_weight)
    return (lambda tok: ngram_row(tok) + ref.row(ref.state(tok)).astype(np.float64)), \
        (lambda tok: float(np.float32(ref.phi(ref.state(tok))))), lm_weight


def bank(fin, residual, weight):
    """the finished list [(tokens, score)] with every pending bonus taken back, re-sorted (stable)"""
    return sorted([(t, s - weight * residual(t)) for t, s in fin], key=lambda f: -f[1])


def rnnt_setting(head_name, W, with_ngram):
    """one transducer search setting -> dict(head on the host, ref (float64 mirror), enc, lens, ngram_image or None,
    lm_row, residual, weight, want): `want` = rnnt_beam_reference.run_case's result with the scorer's rows,
    `margin` the smallest decision margin, the gaps of the corrected finished lists included"""
    import ngram_reference as NR
    import rnnt_beam_reference as BR
    import rnnt_reference as RR
    import rnnt_stateless_reference as SR
    tr = importlib.import_module(PKG_NAME + ".src.transducer")
    ng = importlib.import_module(PKG_NAME + ".src.ngram")
    if head_name == "LSTM":
        case = BR.BEAM_CASES[0]
        head, enc, lens = RR.greedy_case(tr.TransducerHead, *case)
        ref, seed = RR.HeadRef.of(head, RR.GREEDY_ENC_DIM), case[2]
    else:
        case = SR.BEAM_CASES[0]
        head, enc, lens = SR.head_case(tr.TransducerHead, *case)
        ref, seed = SR.StatelessHeadRef.of(head, RR.GREEDY_ENC_DIM), case[1]
    import bias_reference
    image, ng_row = BR.planted_lm_model(ng, NR, RR.GREEDY_V, seed) if with_ngram else (None, None)
    lm_row, residual, weight = rnnt_scorer_rows(bias_reference, ng_row, RR.GREEDY_V, BR.BEAM_LM_WEIGHT)
    want = BR.run_case(ref, enc, lens, W, RR.GREEDY_MAX_SYMBOLS, RR.GREEDY_MAX_LEN, lm_row, weight)
    banked = [bank(fin, residual, weight) for fin, _ in want]
    gaps = [c[i][1] - c[i + 1][1] for c in banked for i in range(len(c) - 1)]
    margin = min([BR.min_margin(t) for _, t in want] + gaps)
    return dict(head=head, ref=ref, enc=enc, lens=lens, ngram_image=image, lm_row=lm_row, residual=residual,
                weight=weight, want=want, banked=banked, margin=margin)
