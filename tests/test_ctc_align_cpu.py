"""CPU: the host reference of CTC forced alignment (tests/ctc_align_reference.py) against brute-force enumeration,
the tie rule of the contract, and the argument validation of asrk_ctc_align_f32 / asrk_ctc_align_ws_bytes, which
happens before any device call."""
import ctypes
import importlib

import numpy as np
import pytest

from conftest import PKG_NAME
import ctc_align_reference as R


def _log_softmax(x):
    x = x - x.max(-1, keepdims=True)
    return (x - np.log(np.exp(x).sum(-1, keepdims=True))).astype(np.float32)


def test_reference_viterbi_equals_brute_force_over_every_path():
    rng = np.random.default_rng(20240)
    V, n_infeasible, n_repeat = 4, 0, 0
    for case in range(300):
        T = int(rng.integers(1, 7))
        L = int(rng.integers(0, 3))
        target = [int(v) for v in rng.integers(1, V, L)]
        n_repeat += L == 2 and target[0] == target[1]
        lp = _log_softmax(rng.standard_normal((T, V)))
        states, tokens, spans, score = R.viterbi(lp, target)
        best, count = R.brute_force(lp, target)
        assert (count > 0) == R.feasible(T, target), (case, T, target)
        if count == 0:
            n_infeasible += 1
            assert states is None and tokens is None and spans is None
            assert score == -np.inf and best == -np.inf
            continue
        assert abs(float(score) - best) <= 1e-5, (case, T, target, score, best)
        # the path the reference returns is admissible and is the one its score belongs to
        ext = R.ext_labels(target)
        assert states[0] <= 1 and states[-1] >= len(ext) - 2
        d = np.diff(states)
        assert ((d >= 0) & (d <= 2)).all()
        for t in np.nonzero(d == 2)[0]:
            assert states[t + 1] & 1 and ext[states[t + 1]] != ext[states[t + 1] - 2]
        assert abs(float(sum(np.float64(lp[t, ext[states[t]]]) for t in range(T))) - best) <= 1e-5
        assert (tokens == ext[states]).all()
        for l in range(L):
            assert (np.nonzero(states == 2 * l + 1)[0] == np.arange(spans[l, 0], spans[l, 1])).all()
    assert n_infeasible >= 5 and n_repeat >= 5, (n_infeasible, n_repeat)


def test_tie_rule_on_constant_log_probs():
    lp = np.full((9, 5), np.log(0.2), dtype=np.float32)
    score = np.float32(0)
    for _ in range(9):                                   # 9 * log 0.2 accumulated in f32, frame by frame
        score = np.float32(score + lp[0, 0])
    states, tokens, spans, sc = R.viterbi(lp, [3, 3, 4])
    assert states.tolist() == [1, 2, 3, 5, 6, 6, 6, 6, 6]
    assert tokens.tolist() == [3, 0, 3, 4, 0, 0, 0, 0, 0]
    assert spans.tolist() == [[0, 1], [2, 3], [3, 4]]
    assert sc.tobytes() == score.tobytes()
    states, tokens, spans, sc = R.viterbi(lp, [])
    assert states.tolist() == [0] * 9 and tokens.tolist() == [0] * 9 and spans.shape == (0, 2)
    assert sc.tobytes() == score.tobytes()


def test_reference_batch_contract():
    rng = np.random.default_rng(3)
    lp = _log_softmax(rng.standard_normal((6, 4, 5)))
    targets = np.array([[1, 2, 0], [3, 3, 3], [0, 0, 0], [1, 9, 0]])
    states, tokens, spans, score = R.align_batch(lp, targets, [6, 4, 5, 6], [2, 3, 0, 2])
    assert (states[0] >= 0).all() and spans[0, 2].tolist() == [-1, -1]
    assert score[1] == -np.inf and (states[1] == -1).all() and (spans[1] == -1).all()      # 3 + 2 repeats > 4 frames
    assert states[2].tolist() == [0, 0, 0, 0, 0, -1] and tokens[2].tolist() == [0, 0, 0, 0, 0, -1]
    assert np.isnan(score[3]) and (states[3] == -1).all() and (tokens[3] == -1).all()


@pytest.fixture(scope="module")
def lib():
    importlib.import_module(PKG_NAME + ".build").build(verbose=False)
    return importlib.import_module(PKG_NAME + "._lib").load()


AUTO, LDS, GLOBAL = 0, 1, 2           # ASRK_ALIGN_BP_* (include/asrk.h)


def test_workspace_size(lib):
    ws = lib.asrk_ctc_align_ws_bytes
    S = 2 * 64 + 1
    # LDS route: the gathered log-probs only; global route: plus 4 * ceil(S / 64) words per frame and utterance
    assert ws(32, 400, 64, LDS) == 32 * 400 * S * 4 == ws(32, 400, 64, AUTO)
    assert ws(32, 400, 64, GLOBAL) == 32 * 400 * S * 4 + 32 * 400 * 3 * 16
    assert ws(32, 1600, 256, LDS) == 0                     # over the LDS budget: the call returns ASRK_ESHAPE
    assert ws(32, 1600, 256, AUTO) == ws(32, 1600, 256, GLOBAL) > 0
    for bad in ((0, 10, 4, AUTO), (-1, 10, 4, AUTO), (2, 0, 4, AUTO), (2, -5, 4, AUTO), (2, 10, -1, AUTO),
                (2, 10, 1024, AUTO), (2, 10, 4, 3), (2, 10, 4, -1)):
        assert ws(*bad) == 0, bad
    for flags in (AUTO, GLOBAL):                           # monotone in every extent, multiples of 16 bytes
        prev = 0
        for n in (1, 2, 7, 64, 500, 3000):
            cur = ws(n, 50, 8, flags)
            assert cur > prev and cur % 16 == 0
            prev = cur
        sizes = [ws(3, T, 40, flags) for T in (1, 9, 100, 1000, 2000, 4000, 9000)]
        assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
        sizes = [ws(3, 700, Lm, flags) for Lm in (0, 1, 31, 32, 100, 500, 1023)]
        assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)


def test_argument_errors_need_no_gpu(lib):
    z, fake = ctypes.c_void_p(0), ctypes.c_void_p(4096)
    T, B, V, Lmax = 10, 2, 7, 3

    def call(**kw):
        a = dict(lp=fake, st=B * V, sb=V, T=T, B=B, V=V, targets=fake, ts=Lmax, Lmax=Lmax, il=fake, tl=fake,
                 blank=0, flags=AUTO, states=fake, tokens=fake, spans=fake, score=fake, stamps=z, ws=fake,
                 ws_bytes=lib.asrk_ctc_align_ws_bytes(B, T, Lmax, kw.get('flags', AUTO)))
        a.update(kw)
        return lib.asrk_ctc_align_f32(a['lp'], a['st'], a['sb'], a['T'], a['B'], a['V'], a['targets'], a['ts'],
                                      a['Lmax'], a['il'], a['tl'], a['blank'], a['flags'], a['states'], a['tokens'],
                                      a['spans'], a['score'], a['stamps'], a['ws'], a['ws_bytes'], z)

    for name in ('lp', 'targets', 'il', 'tl', 'states', 'tokens', 'spans', 'score', 'ws'):
        assert call(**{name: z}) == -1, name
    for kw in (dict(T=-1), dict(B=-1), dict(V=0), dict(Lmax=-1), dict(blank=-1), dict(blank=V), dict(flags=3),
               dict(flags=-1), dict(ws=ctypes.c_void_p(4100))):
        assert call(**kw) == -1, kw
    assert call(B=0) == 0                                                    # empty batch: nothing to do
    assert call(ws_bytes=lib.asrk_ctc_align_ws_bytes(B, T, Lmax, AUTO) - 1) == -3
    assert call(flags=GLOBAL, ws_bytes=lib.asrk_ctc_align_ws_bytes(B, T, Lmax, AUTO)) == -3
    assert call(ws_bytes=0) == -3
    assert call(Lmax=1024, ts=1024) == -2                                    # 2 * Lmax + 1 > 2048 states
    assert call(T=1600, Lmax=256, ts=256, flags=LDS) == -2                   # forced LDS route over its budget
