"""GPU: ops.ctc_align (asrk_ctc_align_f32: Viterbi lattice + backtrace in one launch) against the numpy reference
tests/ctc_align_reference.py.  states / tokens / spans must be EQUAL and the f32 score equal bit for bit (the kernel's
arithmetic is float32 compares and one add, in the reference's order), on both backpointer routes and for both
memory layouts of the log-probs (contiguous [T,B,V]; the transposed view of a [B,T,V] tensor)."""
import importlib

import numpy as np
import pytest
import torch

from conftest import PKG_NAME
import ctc_align_reference as R

pytestmark = pytest.mark.gpu

AUTO, LDS, GLOBAL = 0, 1, 2           # ASRK_ALIGN_BP_* (include/asrk.h)


def _log_probs(T, B, V, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.log_softmax(torch.randn((T, B, V), generator=g), dim=-1).numpy()


def _targets(rng, B, Lmax, V, lens, repeats=True):
    t = np.zeros((B, max(Lmax, 0)), dtype=np.int64)
    for b, L in enumerate(lens):
        row = rng.integers(1, V, L)
        if not repeats:
            for i in range(1, L):
                while row[i] == row[i - 1]:
                    row[i] = rng.integers(1, V)
        t[b, :L] = row
    return t


def _device(ops, lp, targets, il, tl, flags, layout):
    if layout == 'tbv':
        x = torch.from_numpy(lp).cuda()
    else:                                   # the solver's layout: a [T,B,V] view of a [B,T,V] tensor
        x = torch.from_numpy(np.ascontiguousarray(lp.transpose(1, 0, 2))).cuda().transpose(0, 1)
    out = ops.ctc_align(x, torch.from_numpy(targets), torch.tensor(il), torch.tensor(tl), blank=0, flags=flags)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def _same(got, ref, what):
    states, tokens, spans, score = got
    r_states, r_tokens, r_spans, r_score = ref
    assert states.dtype == np.int32 and tokens.dtype == np.int32 and spans.dtype == np.int32
    assert score.dtype == np.float32
    assert np.array_equal(states, r_states), what
    assert np.array_equal(tokens, r_tokens), what
    assert np.array_equal(spans, r_spans), what
    nan = np.isnan(r_score)
    assert np.array_equal(np.isnan(score), nan), what
    assert np.array_equal(score[~nan].view(np.int32), r_score[~nan].view(np.int32)), (what, score, r_score)


def _check(ops, lp, targets, il, tl, routes=(LDS, GLOBAL)):
    ref = R.align_batch(lp, targets, il, tl)
    for flags in routes:
        for layout in ('tbv', 'btv_view'):
            _same(_device(ops, lp, targets, il, tl, flags, layout), ref, (flags, layout))
    return ref


def _plain_case(ops, T, L, V):
    rng = np.random.default_rng(1000 * T + L)
    lens = [L, max(L - 1, 0)]
    targets = _targets(rng, 2, L, V, lens, repeats=False)
    states, _, _, score = _check(ops, _log_probs(T, 2, V, seed=T * 31 + L), targets, [T, T], lens)
    assert np.isfinite(score).all() and (states >= 0).all()


# (T, L): one frame; below, at, just past and well past the 8-frame register ring; S = 63 / 65 around one state per
# lane; several states per lane (L = 100: the <4> build, L = 130: the <16> build of the kernel)
@pytest.mark.parametrize("T,L", [(1, 0), (1, 1), (5, 2), (8, 3), (9, 3), (17, 5), (40, 31), (40, 32), (130, 100),
                                 (170, 130)])
def test_equals_reference(ops, T, L):
    _plain_case(ops, T, L, V=7)


@pytest.mark.parametrize("T,L", [(1, 1), (9, 3), (17, 12)])
def test_equals_reference_large_vocabulary(ops, T, L):
    _plain_case(ops, T, L, V=5000)          # the vocabulary only changes the gather: small lattices suffice


def test_long_padded_targets_use_the_widest_build(ops):
    """Lmax = 512 -> 17 states per lane (the <32> build) while the utterances' own targets still fit the LDS route"""
    rng = np.random.default_rng(5)
    T, B, V, Lmax = 300, 2, 11, 512
    lens = [100, 30]
    targets = _targets(rng, B, Lmax, V, lens)
    _, _, _, score = _check(ops, _log_probs(T, B, V, seed=9), targets, [300, 211], lens)
    assert np.isfinite(score).all()


def test_auto_takes_the_workspace_route_past_the_lds_budget(ops):
    L_ = importlib.import_module(PKG_NAME + "._lib").load()
    T, B, V, L = 2100, 1, 7, 100            # 2100 frames x 4 states per lane x 16 B > 128 KiB
    assert L_.asrk_ctc_align_ws_bytes(B, T, L, AUTO) == L_.asrk_ctc_align_ws_bytes(B, T, L, GLOBAL)
    assert L_.asrk_ctc_align_ws_bytes(B, T, L, LDS) == 0
    rng = np.random.default_rng(6)
    targets = _targets(rng, B, L, V, [L])
    _, _, _, score = _check(ops, _log_probs(T, B, V, seed=10), targets, [T], [L], routes=(AUTO,))
    assert np.isfinite(score).all()


def test_forced_lds_over_budget_is_a_shape_error(ops):
    lib = importlib.import_module(PKG_NAME + "._lib")
    lp = torch.zeros((1600, 1, 7), device='cuda')
    with pytest.raises(lib.AsrkError, match="rc=-2"):
        ops.ctc_align(lp, torch.ones((1, 256), dtype=torch.int64), [1600], [256], flags=LDS)


def test_adjacent_repeats_at_and_below_the_minimal_length(ops):
    targets = np.array([[3, 3, 5, 5, 5, 2]], dtype=np.int64)          # 6 labels + 3 repeats -> 9 frames at least
    lp = _log_probs(9, 1, 7, seed=3)
    assert R.feasible(9, targets[0].tolist()) and not R.feasible(8, targets[0].tolist())
    states, _, spans, score = _check(ops, lp, targets, [9], [6])
    assert states[0].tolist() == [1, 2, 3, 5, 6, 7, 8, 9, 11] and np.isfinite(score[0])     # the only admissible path
    assert spans[0].tolist() == [[0, 1], [2, 3], [3, 4], [5, 6], [7, 8], [8, 9]]
    states, tokens, spans, score = _check(ops, lp, targets, [8], [6])
    assert score[0] == -np.inf and (states == -1).all() and (tokens == -1).all() and (spans == -1).all()


def test_ragged_batch(ops):
    rng = np.random.default_rng(8)
    T, B, V, Lmax = 12, 5, 7, 4
    il, tl = [12, 7, 3, 9, 12], [3, 0, 4, 2, 4]     # full, all blank, infeasible (3 frames, 4 labels), short, full
    targets = _targets(rng, B, Lmax, V, tl)
    states, tokens, spans, score = _check(ops, _log_probs(T, B, V, seed=4), targets, il, tl)
    assert score[2] == -np.inf and (states[2] == -1).all() and (spans[2] == -1).all()
    assert (states[1, :7] == 0).all() and (states[1, 7:] == -1).all() and (spans[1] == -1).all()
    assert (states[3, :9] >= 0).all() and (states[3, 9:] == -1).all() and (tokens[3, 9:] == -1).all()
    assert (spans[3, :2] >= 0).all() and (spans[3, 2:] == -1).all()
    for b in (0, 1, 3, 4):
        assert np.isfinite(score[b])


def test_out_of_range_label(ops):
    rng = np.random.default_rng(9)
    T, B, V = 10, 3, 7
    targets = _targets(rng, B, 3, V, [3, 3, 3])
    lp = _log_probs(T, B, V, seed=5)
    clean = R.align_batch(lp, targets, [T] * B, [3] * B)
    for bad in (V, -1, 1 << 40):
        t2 = targets.copy()
        t2[1, 1] = bad
        states, tokens, spans, score = _check(ops, lp, t2, [T] * B, [3] * B)
        assert np.isnan(score[1]) and (states[1] == -1).all() and (tokens[1] == -1).all() and (spans[1] == -1).all()
        for b in (0, 2):                            # the neighbours are untouched
            assert np.array_equal(states[b], clean[0][b]) and score[b] == clean[3][b]


def test_tie_rule_on_the_device(ops):
    lp = np.full((9, 2, 5), np.log(0.2), dtype=np.float32)
    targets = np.array([[3, 3, 4], [0, 0, 0]], dtype=np.int64)
    states, tokens, spans, score = _check(ops, lp, targets, [9, 9], [3, 0])
    assert states[0].tolist() == [1, 2, 3, 5, 6, 6, 6, 6, 6] and states[1].tolist() == [0] * 9
    want = np.float32(0)
    for _ in range(9):
        want = np.float32(want + np.float32(np.log(0.2)))
    assert score[0].tobytes() == want.tobytes() and score[1].tobytes() == want.tobytes()


def test_properties_of_an_alignment(ops):
    rng = np.random.default_rng(11)
    T, B, V, L = 60, 4, 30, 12
    tl = [12, 9, 12, 1]
    il = [60, 60, 41, 60]
    targets = _targets(rng, B, L, V, tl)
    lp = _log_probs(T, B, V, seed=6)
    states, tokens, spans, score = _check(ops, lp, targets, il, tl)
    for b in range(B):
        tok = tokens[b, :il[b]].tolist()
        merged = [c for i, c in enumerate(tok) if i == 0 or c != tok[i - 1]]
        st = states[b, :il[b]]
        # collapsing the tokens (drop repeats, then blanks) gives the target back
        assert [c for c in merged if c != 0] == targets[b, :tl[b]].tolist()
        sp = spans[b, :tl[b]]
        assert (sp[:, 0] < sp[:, 1]).all() and (sp[1:, 0] >= sp[:-1, 1]).all()          # ordered and disjoint
        assert sp[0, 0] >= 0 and sp[-1, 1] <= il[b]
        for l in range(tl[b]):
            assert np.array_equal(np.nonzero(st == 2 * l + 1)[0], np.arange(sp[l, 0], sp[l, 1]))
    nll = ops.CTCLoss(blank=0, reduction='none')(torch.from_numpy(lp).cuda(), torch.from_numpy(targets).cuda(),
                                                 torch.tensor(il), torch.tensor(tl)).cpu().numpy()
    # the best path is one of the many paths the loss sums over
    assert (score <= -nll).all(), (score, -nll)


def test_phase_stamps_are_monotone(ops):
    """the optional [B,4] stamps (start, lattice done, backtrace done, end of every utterance's wave) on both routes;
    the outputs do not depend on asking for them"""
    rng = np.random.default_rng(12)
    T, B, V, L = 50, 3, 9, 6
    tl, il = [6, 0, 4], [50, 33, 3]                 # aligned, all blank, infeasible: every wave stamps all four
    targets = _targets(rng, B, L, V, tl)
    lp = _log_probs(T, B, V, seed=7)
    ref = R.align_batch(lp, targets, il, tl)
    for flags in (LDS, GLOBAL):
        stamps = torch.zeros((B, 4), dtype=torch.int64, device='cuda')
        out = ops.ctc_align(torch.from_numpy(lp).cuda(), torch.from_numpy(targets), il, tl, flags=flags,
                            stamps=stamps)
        _same([o.cpu().numpy() for o in out], ref, flags)
        s = stamps.cpu().numpy()
        assert (s[:, 0] > 0).all() and (np.diff(s, axis=1) >= 0).all(), s
