"""GPU: ops.rnnt_align (csrc/rnnt_align.hip) against the numpy f32 reference of the same recurrence
(tests/rnnt_align_reference.py), bit for bit, on both backpointer routes.

Bounds, from the operation counts and never from what the kernel gives:
 * the kernel's path, scored in float64 on the f32 inputs, against the float64 optimum: the f32 walk adds T + U rounded
   terms along any path, each rounding at most 2^-24 of a partial sum bounded by A = the largest |delta| of the float64
   Viterbi: (T + U) * 2^-24 * max(1, A);
 * tok_post against float64 exp of the same three-term sum of the device's own alpha, beta and nll: three rounded adds
   on magnitudes up to A' plus expf: relative error at most 3 * 2^-24 * max(1, A') + 2^-21."""
import importlib

import numpy as np
import pytest
import torch

import rnnt_align_reference as AR
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu
DEV = "cuda"
SMALL = [(1, 0), (1, 1), (1, 5), (5, 0), (2, 1), (7, 3), (3, 7)]
LATTICES = SMALL + [(64, 63), (65, 64), (9, 300), (130, 100)]
AUTO, LDS, GLOBAL = 0, 1, 2


def _mod(name):
    return importlib.import_module(PKG_NAME + "." + name)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _align(ops, lpb, lpl, el, tl, flags=AUTO, lattice=False):
    """numpy in, numpy out"""
    lpb_d, lpl_d = _dev(lpb), _dev(lpl)
    lat = ops.rnnt_lattice(lpb_d, lpl_d, torch.tensor(el), torch.tensor(tl)) if lattice else None
    r = ops.rnnt_align(lpb_d, lpl_d, torch.tensor(el), torch.tensor(tl), flags=flags, lattice=lat)
    torch.cuda.synchronize()
    out = dict(frames=r.frames.cpu().numpy(), labels_done=r.labels_done.cpu().numpy(),
               tok_logp=r.tok_logp.cpu().numpy(), score=r.score.cpu().numpy(),
               tok_post=None if r.tok_post is None else r.tok_post.cpu().numpy())
    if lattice:
        out["lattice"] = tuple(x.cpu().numpy() for x in lat)
    return out


def _same(got, ref, b=0):
    assert np.array_equal(got["frames"][b], ref["frames"]) and np.array_equal(got["labels_done"][b], ref["labels_done"])
    assert got["tok_logp"][b].tobytes() == ref["tok_logp"].tobytes()
    assert got["score"][b:b + 1].tobytes() == np.float32(ref["score"]).tobytes()      # NaN positions and bits included


@pytest.mark.parametrize("flags", [LDS, GLOBAL])
@pytest.mark.parametrize("T,U", LATTICES)
def test_equals_reference_exactly_and_path_is_optimal(ops, T, U, flags):
    lpb, lpl = AR.random_lattice(T, U, 31 * T + U)
    ref = AR.align_f32(lpb, lpl, T, U)
    got = _align(ops, lpb[None], lpl[None], [T], [U], flags)
    _same(got, ref)
    assert got["tok_post"] is None
    auto = _align(ops, lpb[None], lpl[None], [T], [U], AUTO)           # AUTO: the LDS route here, the same bits
    _same(auto, ref)
    assert _mod("_lib").load().asrk_rnnt_align_ws_bytes(1, T, U + 1, AUTO) == 0
    # the path against the float64 optimum
    _, s64, A = AR.viterbi64(lpb, lpl, T, U)
    mine = AR.path_score64(lpb, lpl, list(got["frames"][0][:U]), T, U)
    gap, bound = s64 - mine, (T + U) * 2.0 ** -24 * max(1.0, A)
    print("T %d U %d: float64 optimum %.9g, the kernel's path %.9g, gap %.3g, bound %.3g" % (T, U, s64, mine, gap, bound))
    assert abs(gap) <= bound


def test_edge_cases_on_both_routes(ops):
    T, U = 6, 4
    ties = np.full((1, T, U + 1), -1.0, np.float32)
    lpb, lpl = AR.random_lattice(T, U, 9)
    nan, inf, one = lpl.copy(), lpl.copy(), lpl.copy()
    nan[:, 1] = np.nan
    inf[:, 2] = -np.inf
    one[3, 0] = np.nan
    for flags in (LDS, GLOBAL):
        got = _align(ops, ties, ties, [T], [U], flags)
        assert list(got["frames"][0]) == [0] * U and list(got["labels_done"][0]) == [U] * T
        assert got["score"][0] == -float(T + U)
        for x in (nan, inf, one):
            got = _align(ops, lpb[None], x[None], [T], [U], flags, lattice=True)
            _same(got, AR.align_f32(lpb, x, T, U))
            assert (got["frames"] == -1).all() and (got["labels_done"] == -1).all()
            assert (got["tok_logp"] == 0).all() and (got["tok_post"] == 0).all()
        assert np.isnan(_align(ops, lpb[None], nan[None], [T], [U], flags)["score"][0])
        assert _align(ops, lpb[None], inf[None], [T], [U], flags)["score"][0] == -np.inf


def test_forced_lds_route_that_does_not_fit(ops):
    """U1 = 65: two words per diagonal; T = 8129 is the first length whose (T + 64) * 16 bytes pass 128 KiB"""
    lib = _mod("_lib")
    T, U1 = 8129, 65
    lpb = torch.zeros((1, T, U1), dtype=torch.float32, device=DEV)
    with pytest.raises(lib.AsrkError, match="shape"):
        ops.rnnt_align(lpb, lpb, torch.tensor([T]), torch.tensor([U1 - 1]), flags=LDS)
    assert lib.load().asrk_rnnt_align_ws_bytes(1, T, U1, AUTO) > 0     # AUTO goes through the workspace


@pytest.mark.parametrize("flags", [LDS, GLOBAL])
def test_ragged_batch_equals_every_utterance_alone(ops, flags):
    """B = 3, mixed (T_b, U_b), one U_b = 0, lpb / lpl padded in T and U1 beyond the longest utterance (U1 = 70: two
    ballot slots), NaN in every cell outside a lattice: reading one of them would show in the score"""
    T, U1 = 80, 70
    sizes = [(70, 66), (33, 0), (75, 9)]
    lpb = np.full((3, T, U1), np.nan, np.float32)
    lpl = np.full((3, T, U1), np.nan, np.float32)
    for b, (Tb, Ub) in enumerate(sizes):
        a, c = AR.random_lattice(Tb, Ub, 40 + b)
        lpb[b, :Tb, :Ub + 1] = a
        lpl[b, :Tb, :Ub] = c[:, :Ub]
    el, tl = [s[0] for s in sizes], [s[1] for s in sizes]
    got = _align(ops, lpb, lpl, el, tl, flags, lattice=True)
    assert np.isfinite(got["score"]).all() and np.isfinite(got["tok_post"]).all()
    for b, (Tb, Ub) in enumerate(sizes):
        _same(got, AR.align_f32(lpb[b], lpl[b], Tb, Ub), b)
        alone = _align(ops, np.ascontiguousarray(lpb[b:b + 1, :Tb, :Ub + 1]),
                       np.ascontiguousarray(lpl[b:b + 1, :Tb, :Ub + 1]), [Tb], [Ub], flags, lattice=True)
        assert np.array_equal(alone["frames"][0], got["frames"][b, :Ub])
        assert np.array_equal(alone["labels_done"][0], got["labels_done"][b, :Tb])
        assert alone["tok_logp"][0].tobytes() == got["tok_logp"][b, :Ub].tobytes()
        assert alone["tok_post"][0].tobytes() == got["tok_post"][b, :Ub].tobytes()
        assert alone["score"].tobytes() == got["score"][b:b + 1].tobytes()
        assert (got["frames"][b, Ub:] == -1).all() and (got["labels_done"][b, Tb:] == -1).all()
        assert (got["tok_logp"][b, Ub:] == 0).all() and (got["tok_post"][b, Ub:] == 0).all()


@pytest.mark.parametrize("T,U", LATTICES)
def test_tok_post_against_float64(ops, T, U):
    lpb, lpl = AR.random_lattice(T, U, 31 * T + U)
    got = _align(ops, lpb[None], lpl[None], [T], [U], AUTO, lattice=True)
    alpha, beta, nll = (x.astype(np.float64) for x in got["lattice"])
    assert got["tok_post"].shape == (1, U)
    for u in range(U):
        t = int(got["frames"][0, u])
        terms = (alpha[0, t, u], float(lpl[t, u]), beta[0, t, u + 1], nll[0])
        want = np.exp(((terms[0] + terms[1]) + terms[2]) + terms[3])
        bound = 3 * 2.0 ** -24 * max(1.0, max(abs(x) for x in terms)) + 2.0 ** -21
        have = float(got["tok_post"][0, u])
        assert abs(have - want) <= bound * want, (u, have, want, bound)


def test_two_runs_are_bit_equal(ops):
    T, U = 130, 100
    lpb, lpl = AR.random_lattice(T, U, 3)
    B = 4
    lpb, lpl = np.repeat(lpb[None], B, 0), np.repeat(lpl[None], B, 0)
    el, tl = [T, T - 7, 50, 1], [U, 60, U, 0]
    for flags in (LDS, GLOBAL):
        a = _align(ops, lpb, lpl, el, tl, flags, lattice=True)
        b = _align(ops, lpb, lpl, el, tl, flags, lattice=True)
        for k in ("frames", "labels_done", "tok_logp", "tok_post", "score"):
            assert a[k].tobytes() == b[k].tobytes(), k


def test_argument_checks_of_the_wrapper(ops):
    lib = _mod("_lib")
    f = torch.zeros((2, 3, 4), dtype=torch.float32, device=DEV)
    el, tl = torch.tensor([3, 3]), torch.tensor([3, 3])
    with pytest.raises(lib.AsrkError):
        ops.rnnt_align(f.cpu(), f.cpu(), el, tl)
    with pytest.raises(lib.AsrkError):
        ops.rnnt_align(f, f[:, :, :3], el, tl)
    with pytest.raises(lib.AsrkError):
        ops.rnnt_align(f.double(), f.double(), el, tl)
    with pytest.raises(lib.AsrkError):
        ops.rnnt_align(f, f, el[:1], tl)
    with pytest.raises(lib.AsrkError):
        ops.rnnt_align(f, f, el, tl, lattice=(f, f, torch.zeros(3, device=DEV)))
    with pytest.raises(lib.AsrkError):
        ops.rnnt_align(f, f, el, tl, flags=7)
    with pytest.raises(lib.AsrkError):
        ops.rnnt_align(f, f, el, tl, stamps=torch.zeros((2, 3), dtype=torch.int64, device=DEV))
