"""TEST INFRASTRUCTURE ONLY - fixtures shared by the n-gram LM tests (CPU and GPU): seeded corpora, estimated ARPA
files, the hand-built model that holds every shape the step kernel can go wrong on, and the six search cases."""
import importlib
import os

import numpy as np
import torch

from conftest import PKG_NAME, ROOT  # noqa: F401  (ROOT on sys.path: `tools` is importable)
from tools import ngram_lm as NT

LN10 = float(np.log(10.0))


def ngram_mod():
    return importlib.import_module(PKG_NAME + ".src.ngram")


def corpus(seed, V=12, lines=300, unseen=1):
    """sentences over the ids 3 .. V - 1 - unseen with second-order structure (so that higher orders matter); the
    last `unseen` ids never occur: tokens without a unigram"""
    rng = np.random.RandomState(seed)
    n = V - 3 - unseen
    out = []
    for _ in range(lines):
        L = int(rng.randint(1, 9))
        s = [int(rng.randint(n))]
        for i in range(1, L):
            prev2 = s[i - 2] if i > 1 else 0
            if rng.rand() < 0.7:
                s.append((2 * s[i - 1] + prev2 + int(rng.randint(2))) % n)
            else:
                s.append(int(rng.randint(n)))
        out.append([3 + t for t in s])
    return out


def estimated_arpa(path, sentences, order):
    NT.write_arpa(NT.witten_bell(sentences, order), str(path))
    return str(path)


# ---- the step kernel's fixture -----------------------------------------------------------------------------------
NO_UNIGRAM = (5,)                      # + V - 1: ids that appear in no n-gram
EVERY_LEVEL = 7                        # the word with an entry at every level of the chain (9, 10, 11) -> (11) -> ()
BIG_NODE = (3,)                        # the context with min(300, V - 8) children
CHAIN = (9, 10, 11)


def kernel_fixture(V, order, seed=0):
    """per-order {tuple: (ln p, ln bo)} tables for build_image: random values (positive back-off weights among them),
    a context with up to 300 children, contexts without children, one word at every level of one chain, contexts of
    every length, two ids without a unigram.  Suffixes / prefixes that the random draw leaves out are the builder's
    to complete."""
    rng = np.random.RandomState(1000 * order + V + seed)
    val = lambda: (float(rng.uniform(-8.0, -0.1)), float(rng.uniform(-1.5, 0.7)))
    skip = set(NO_UNIGRAM) | {V - 1}
    words = [w for w in range(V) if w not in skip]
    grams = [dict() for _ in range(order)]
    for w in words:
        grams[0][(w,)] = val()
    grams[0][(0,)] = (-99.0 * LN10, float(rng.uniform(-1.0, 0.0)))
    if order >= 2:
        for w in words[:min(300, V - 8)]:
            grams[1][BIG_NODE + (w,)] = val()
        for k in range(2, order + 1):                      # the chain and EVERY_LEVEL under each of its suffixes
            ctx = CHAIN[-(k - 1):]
            if len(ctx) == k - 1:
                grams[k - 1][ctx + (EVERY_LEVEL,)] = val()
                if k - 1 >= 2 and k - 1 < order:
                    grams[k - 2].setdefault(ctx, val())
        for k in range(2, order + 1):                      # random entries under random existing contexts
            ctxs = sorted(grams[k - 2])
            for _ in range(40):
                h = ctxs[int(rng.randint(len(ctxs)))]
                if h[-1] == 1 or h == BIG_NODE:
                    continue
                for w in rng.choice(words, size=int(rng.randint(1, 6)), replace=False):
                    if int(w) != 0:
                        grams[k - 1].setdefault(h + (int(w),), val())
    return grams


def kernel_rows(image, contexts, n, seed=0):
    """n (state, token) pairs: first every node as the NEW state (so every depth is reached), then the special tokens
    from deep states, then random pairs"""
    rng = np.random.RandomState(seed)
    V, N = int(image['vocab_size']), len(image['bo'])
    node_of = {h: s for s, h in contexts.items()}
    by_depth = {}
    for s, h in sorted(contexts.items()):
        if s != 0:
            by_depth.setdefault(len(h), []).append((node_of[h[:-1]], h[-1]))
    rows, k = [], 0
    while len(rows) < max(1, n // 2) and any(k < len(v) for v in by_depth.values()):
        rows += [v[k] for _, v in sorted(by_depth.items(), reverse=True) if k < len(v)]     # deepest first, all depths
        k += 1
    deep = max(contexts, key=lambda s: len(contexts[s]))
    rows = rows[:max(1, n // 2)]
    rows += [(deep, NO_UNIGRAM[0]), (deep, V - 1), (deep, 1), (deep, EVERY_LEVEL), (0, 0), (deep, 0)]
    while len(rows) < n:
        rows.append((int(rng.randint(N)), int(rng.randint(V))))
    rows = rows[:n]
    return np.array([r[0] for r in rows], np.int32), np.array([r[1] for r in rows], np.int64)


# ---- the search cases ---------------------------------------------------------------------------------------------
SEARCH_V, SEARCH_T, SEARCH_BEAM, SEARCH_CAND = 40, 30, 5, 8
# (seed, lm_w): chosen on the CPU so that in the ORACLE's run the fused score changes the best hypothesis against
# lm_w = 0 in at least four of the six (tests/test_ngram_cpu.py asserts it)
SEARCH_CASES = [(0, 0.3), (1, 1.0), (2, 0.3), (3, 1.0), (4, 0.3), (5, 1.0)]
SEARCH_LM_SEED, SEARCH_LM_ORDER = 11, 3


def search_lm_arpa(path):
    return estimated_arpa(path, corpus(SEARCH_LM_SEED, V=SEARCH_V, lines=400, unseen=2), SEARCH_LM_ORDER)


def search_posteriors(seed, T=SEARCH_T, V=SEARCH_V):
    """[T, V] float32 log-probabilities: blank-dominated frames with emitting spikes whose two or three best tokens
    are close - the situation in which a language model decides"""
    rng = np.random.RandomState(100 + seed)
    logits = rng.randn(T, V).astype(np.float32)
    logits[:, 0] += 4.0
    for t in rng.choice(T, size=T // 3, replace=False):
        logits[t, 0] -= 5.0
        a, b, c = rng.choice(np.arange(3, V - 2), size=3, replace=False)
        logits[t, a] += 3.0
        logits[t, b] += 3.0 - 0.6 * rng.rand()
        logits[t, c] += 2.0
    if seed % 2:
        logits[rng.randint(T // 2, T), 1] += 4.0           # an <eos> candidate
    return torch.log_softmax(torch.from_numpy(logits), dim=-1).numpy()


# ---- the joint CTC-attention search on the las_hybrid_loc golden model (V = 13) ---------------------------------------
# corpus seed of the 3-gram, chosen on the CPU with oracle/beam_oracle.py (beam 3, ctc 0.4, lm 0.3, utterance 0): the
# mean scores of the oracle's three hypotheses are 2.8e-2 or more apart and the best one differs from lm_weight = 0
# (tests/test_ngram_decode_gpu.py asserts both before it compares)
JOINT_LM_SEED, JOINT_LM_ORDER = 21, 3
JOINT_KW = dict(beam_size=3, ctc_weight=0.4, lm_weight=0.3)


def joint_lm_arpa(path, V):
    return estimated_arpa(path, corpus(JOINT_LM_SEED, V=V, lines=300, unseen=1), JOINT_LM_ORDER)


def vocab_range(V):
    return [1] + list(range(3, V))
