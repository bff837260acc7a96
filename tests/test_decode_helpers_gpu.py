"""GPU: the helpers of one beam-search position (decoder_ops.py), each against a plain reference of the same
operation instead of through whole beam searches:

  gather_rows_multi   against torch indexing, compared as int32 bit patterns (NaN, +-inf, -0 count), destinations inside
                      sentinel-guarded allocations;
  joint_score         against a float64 evaluation of the formula in its docstring with the three scalars rounded to
                      float32 first (as the kernel's comment says the original does).  LOG_ZERO = -1e8 sits in every row,
                      so a per-tensor relative error would see nothing: every ELEMENT has to be within
                      4 * 2**-24 * (the sum of the magnitudes of its terms) - one rounding per float32 operation of
                      the expression, at most four of them on a term;
  linear_infer, lstm_cell_infer
                      against float64 on both sides of every branch condition (rows 127 | 128, widths 32 | 40, 64 | 65,
                      32 | 36), the branch that ran counted through ops.gemm_panels.  Criterion: helpers.rel_err < 1e-3
                      and rel_err <= max(F * e32, 4 * 2**-24), e32 = the float32 CPU run of the same formula;
  the weight-panel cache  follows a version bump, and a write through an alias that bumps no version once
                      drop_weight_panels() has run (the situation the comment above decoder_ops._weight_panels describes).

Every figure is printed before it is asserted (pytest -s, lines starting DECODEHELP).  F: the smallest power of two at
least twice the largest device / e32 seen on the MI355X:

    linear_infer y       1.14 (B=130 K=40 N=257, bias)    F = 4
    lstm_cell_infer h    1.33 (B=127 In=65 H=32)          F = 4
    lstm_cell_infer c    1.16 (B=128 In=64 H=36)          F = 4

joint_score: the largest element error seen is 0.39 of its bound.
"""
import ctypes
import importlib
import itertools

import pytest
import torch

from conftest import PKG_NAME
from helpers import rel_err
import speller_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = dict(linear=4, h=4, c=4)
HARD, FLOOR, EPS = 1e-3, 4 * 2.0 ** -24, 2.0 ** -24
GUARD = 64                       # floats on either side of a destination: keeps its 16-byte alignment
PATTERN = 0x7FA12345             # a NaN payload nothing computes


@pytest.fixture()
def dops(ops):
    m = importlib.import_module(PKG_NAME + ".decoder_ops")
    m.drop_weight_panels()       # as every beam search starts
    return m


def _bound(e32, f):
    return min(max(f * e32, FLOOR), HARD)


def _report(name, kind, e32, bound, err):
    print("DECODEHELP %s | %s | e32 %.3e | bound %.3e | device %.3e | device/e32 %.2f"
          % (name, kind, e32, bound, err, err / e32 if e32 else 0.0))


# ---------------------------------------------------------------------------------------------- gather_rows_multi
def _source(g, rows, rf, offset=0):
    """contiguous [rows, rf] with NaN, +-inf and -0 sprinkled in; offset: floats past the allocation's start"""
    buf = torch.randn(offset + rows * rf, generator=g)
    flat = buf[offset:]
    for k, v in enumerate((float('nan'), float('inf'), -float('inf'), -0.0)):
        flat[k::11] = v
    buf = buf.to(DEV)
    return buf[offset:].view(rows, rf)


def _dest(n, rf, offset=0):
    big = torch.full((n * rf + 2 * GUARD,), PATTERN, dtype=torch.int32, device=DEV).view(torch.float32)
    return big, big[GUARD + offset:GUARD + offset + n * rf].view(n, rf)


def _gather_and_check(dops, ops, specs, parent, col, rows):
    """specs: (row_floats, mul, use_col, source offset, destination offset)"""
    g = torch.Generator().manual_seed(3)
    n = len(parent)
    parent_d, col_d = torch.tensor(parent, device=DEV), torch.tensor(col, device=DEV)
    segs, bigs = [], []
    for rf, mul, uc, so, do in specs:
        src = _source(g, rows * mul, rf, so)
        big, dst = _dest(n, rf, do)
        assert (src.data_ptr() % 16 != 0) == (so % 4 != 0) and (dst.data_ptr() % 16 != 0) == (do % 4 != 0)
        segs.append((src, dst, rf, mul, uc))
        bigs.append(big)
    dops.gather_rows_multi(segs, parent_d, col_d)
    ops.check_errors()
    torch.cuda.synchronize()
    for (src, dst, rf, mul, uc), big, spec in zip(segs, bigs, specs):
        want = src[parent_d * mul + (col_d if uc else 0)]
        assert torch.equal(dst.view(torch.int32), want.view(torch.int32)), spec
        do = spec[4]
        outside = torch.cat([big[:GUARD + do], big[GUARD + do + n * rf:]]).view(torch.int32)
        assert bool((outside == PATTERN).all()), spec


TE, C = 21, 4
EIGHT = [(1, 1, 0, 0, 0), (3, 1, 0, 0, 0), (20, 1, 0, 0, 0),
         (1028, 1, 0, 0, 0),                     # 257 float4 per row: past one 256-thread sweep
         (2 * TE, C, 1, 0, 0),                   # the CTC prefix-state form r_new[parent, col]
         (8, 1, 0, 1, 0),                        # source 4 bytes past a 16-byte boundary, rf % 4 == 0: scalar path
         (1030, 1, 0, 0, 0),                     # rf % 4 != 0, more than one scalar sweep
         (4, 1, 0, 0, 2)]                        # destination 8 bytes past a boundary


def test_gather_rows_multi_eight_segments(ops, dops):
    """8 segments in one call, parents with repeats and out of order"""
    _gather_and_check(dops, ops, EIGHT, parent=[3, 0, 3, 1, 2], col=[2, 0, 1, 3, 0], rows=4)


def test_gather_rows_multi_one_row(ops, dops):
    _gather_and_check(dops, ops, EIGHT[2:6], parent=[2], col=[3], rows=3)


def test_gather_rows_multi_refuses_nine_segments(ops, dops):
    lib = importlib.import_module(PKG_NAME + "._lib")
    parent = torch.tensor([1, 0], device=DEV)
    segs, bigs = [], []
    for _ in range(9):
        big, dst = _dest(2, 4)
        segs.append((torch.ones(2, 4, device=DEV), dst, 4, 1, 0))
        bigs.append(big)
    with pytest.raises(lib.AsrkError):
        dops.gather_rows_multi(segs, parent)
    torch.cuda.synchronize()
    assert all(bool((b.view(torch.int32) == PATTERN).all()) for b in bigs)       # nothing was copied


# ---------------------------------------------------------------------------------------------------- joint_score
LOGZERO = -1e8
f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))


def _candidates(g, n, V, C):
    """[n,C] int64: distinct labels of a row, among them 0 (<sos>) and -1 (a missing pick of ops.topk)"""
    rows = []
    for _ in range(n):
        labels = (torch.randperm(V - 1, generator=g)[:max(min(C - 2, V - 1), 0)] + 1).tolist()
        row = [0] + labels + [-1] * (C - 1 - len(labels))
        rows.append([row[i] for i in torch.randperm(C, generator=g).tolist()])
    return torch.tensor(rows, dtype=torch.int64)


def _joint_reference(att, cand, psi, prev, lm, ctc_w, lm_w):
    """-> (out, magnitude of the terms of every element) in float64"""
    wa, wc, wl, lz = f32(1.0 - ctc_w), f32(ctc_w), f32(lm_w), f32(LOGZERO)
    out, mag = att.double().clone(), att.double().abs()
    if cand is not None:
        hack = torch.full_like(out, lz)
        hmag = torch.full_like(out, abs(lz))
        for r in range(cand.shape[0]):
            for c in range(cand.shape[1]):
                v = int(cand[r, c])
                if v >= 0:
                    hack[r, v] = psi[r, c].double() - prev[r].double()
                    hmag[r, v] = psi[r, c].double().abs() + prev[r].double().abs()
        out, mag = wa * out + wc * hack, abs(wa) * mag + abs(wc) * hmag
        out[:, 0], mag[:, 0] = lz, abs(lz)                               # <sos> (the LM term is still added)
    if lm is not None:
        out, mag = out + wl * lm.double(), mag + abs(wl) * lm.double().abs()
    return out, mag


@pytest.mark.parametrize("V", [7, 257, 1031])
@pytest.mark.parametrize("C", [None, 4, 24])
def test_joint_score_vs_float64(ops, dops, V, C):
    g = torch.Generator().manual_seed(V * 31 + (C or 0))
    worst = 0.0
    for n, with_lm in itertools.product((1, 5), (False, True)):
        att = torch.log_softmax(torch.randn(n, V, generator=g) * 3, dim=-1)
        lm = torch.log_softmax(torch.randn(n, V, generator=g) * 2, dim=-1) if with_lm else None
        cand = psi = prev = None
        if C is not None:
            cand = _candidates(g, n, V, C)
            psi, prev = -torch.rand(n, C, generator=g) * 40, -torch.rand(n, generator=g) * 30
            assert bool((cand == 0).any(1).all()) and bool((cand == -1).any(1).all())
        ctc_w, lm_w = (0.3 if C is not None else 0.0), (0.45 if with_lm else 0.0)
        dv = lambda x: None if x is None else x.to(DEV)
        got = dops.joint_score(dv(att), dv(cand), dv(psi), dv(prev), dv(lm), ctc_w, lm_w, LOGZERO)
        ops.check_errors()
        want, mag = _joint_reference(att, cand, psi, prev, lm, ctc_w, lm_w)
        got = got.double().cpu()
        assert got.shape == (n, V) and bool(torch.isfinite(got).all())
        ratio = float(((got - want).abs() / (4 * EPS * mag).clamp(min=1e-300)).max())
        worst = max(worst, ratio)
        print("DECODEHELP joint_score n=%d V=%d C=%s lm=%d | max error / (4 * 2**-24 * magnitude) %.3f"
              % (n, V, C, with_lm, ratio))
        if C is not None:
            assert with_lm or bool((got[:, 0] == f32(LOGZERO)).all())            # <sos> stays exactly LOG_ZERO
            hit = torch.zeros(n, V, dtype=torch.bool)
            for r in range(n):
                hit[r, cand[r][cand[r] > 0]] = True
            assert bool((got[hit] > -1e3).all()) and bool((got[~hit] < -1e6).all())   # candidates and only they
    assert worst <= 1.0


def test_joint_score_refuses_in_place(ops):
    L = importlib.import_module(PKG_NAME + "._lib").load()
    att = torch.zeros(2, 7, device=DEV)
    p = ctypes.c_void_p(att.data_ptr())
    z = ctypes.c_void_p(0)
    assert L.asrk_joint_score_f32(p, z, z, z, z, p, 2, 7, 0, 0.0, 0.0, LOGZERO, ops._stream()) == -1
    torch.cuda.synchronize()
    assert float(att.abs().sum()) == 0.0


# ------------------------------------------------------------------------------- linear_infer / lstm_cell_infer
@pytest.fixture()
def panel_calls(ops, monkeypatch):
    """counts the calls of ops.gemm_panels (the many-row branch of both helpers and nothing else in them)"""
    calls, real = [], ops.gemm_panels

    def counting(*a, **k):
        calls.append(a[:3])
        return real(*a, **k)
    monkeypatch.setattr(ops, "gemm_panels", counting)
    return calls


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("N", [31, 257])
@pytest.mark.parametrize("K", [32, 40])
@pytest.mark.parametrize("B", [127, 128, 130])
def test_linear_infer_vs_float64(ops, dops, panel_calls, B, K, N, bias):
    g = torch.Generator().manual_seed(B * 1000 + K * 10 + N)
    x, w = torch.randn(B, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g) * 0.1 if bias else None
    ref = lambda dt: x.to(dt) @ w.to(dt).t() + (b.to(dt) if bias else 0)
    want = ref(torch.float64)
    e32 = rel_err(ref(torch.float32), want)
    with torch.no_grad():
        y = dops.linear_infer(x.to(DEV), w.to(DEV), b.to(DEV) if bias else None)
    ops.check_errors()
    err, bound = rel_err(y.cpu(), want), _bound(e32, F['linear'])
    _report("linear_infer B=%d K=%d N=%d bias=%d" % (B, K, N, bias), "y", e32, bound, err)
    assert y.shape == (B, N)
    assert len(panel_calls) == (1 if B >= 128 and K % 32 == 0 else 0)
    assert err < HARD and err <= bound


@pytest.mark.parametrize("with_out", [False, True], ids=["fresh", "out"])
@pytest.mark.parametrize("H", [32, 36])
@pytest.mark.parametrize("In", [64, 65])
@pytest.mark.parametrize("B", [127, 128])
def test_lstm_cell_infer_vs_float64(ops, dops, panel_calls, B, In, H, with_out):
    g = torch.Generator().manual_seed(B * 1000 + In * 10 + H)
    rn = lambda *s: torch.randn(*s, generator=g)
    t = [rn(B, In), torch.tanh(rn(B, H)), rn(B, H), rn(4 * H, In) / In ** 0.5, rn(4 * H, H) / H ** 0.5,
         rn(4 * H) * 0.1, rn(4 * H) * 0.1]
    want = R.lstm_cell_reference(*[a.double() for a in t])
    r32 = R.lstm_cell_reference(*t)
    out = None
    if with_out:
        out = (torch.full((B, H), 9.0, device=DEV), torch.full((B, H), 9.0, device=DEV))
    with torch.no_grad():
        got = dops.lstm_cell_infer(*[a.to(DEV) for a in t], out=out)
    ops.check_errors()
    if with_out:
        assert got[0].data_ptr() == out[0].data_ptr() and got[1].data_ptr() == out[1].data_ptr()
    assert len(panel_calls) == (2 if B >= 128 and In % 32 == 0 and H % 32 == 0 else 0)
    bad = []
    for kind, dev, w64, w32 in zip(("h", "c"), got, want, r32):
        e32 = rel_err(w32, w64)
        err, bound = rel_err(dev.cpu(), w64), _bound(e32, F[kind])
        _report("lstm_cell_infer B=%d In=%d H=%d out=%d" % (B, In, H, with_out), kind, e32, bound, err)
        assert dev.shape == (B, H)
        if not (err < HARD and err <= bound):
            bad.append((kind, err, bound))
    assert not bad, bad


def test_weight_panel_cache_follows_the_weights(ops, dops, panel_calls):
    """three many-row calls on one weight tensor: the first; after weight.mul_(2) (a version bump); after a write
    through an alias that shares the storage but bumps no version, followed by drop_weight_panels()"""
    g = torch.Generator().manual_seed(17)
    B, K, N = 128, 32, 31
    x, w0 = torch.randn(B, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5
    xd, w = x.to(DEV), w0.to(DEV)
    want = x.double() @ w0.double().t()

    def call(scale, label):
        with torch.no_grad():
            y = dops.linear_infer(xd, w)
        ops.check_errors()
        err = rel_err(y.cpu(), scale * want)
        print("DECODEHELP panel cache | %s | device %.3e" % (label, err))
        return err
    assert call(1, "first call") < 1e-5
    v = w._version
    w.mul_(2)
    assert w._version > v
    assert call(2, "after weight.mul_(2)") < 1e-5
    v = w._version
    w.data.mul_(3)                               # as the fused optimiser writes parameters: no version bump
    assert w._version == v
    dops.drop_weight_panels()
    assert call(6, "after an unversioned write and drop_weight_panels()") < 1e-5
    assert len(panel_calls) == 3
