"""GPU: every kernel variant of the convolutional prenet (csrc/conv3x3.hip, csrc/conv.hip through conv_ops.conv /
conv_ops.conv_len and the autograd of ConvFn) against the float64 reference and on the case table of
tests/conv_reference.py; tests/test_conv_plan_cpu.py holds every row to the tile geometry it names, and every row asserts
its route on the device before it runs (Geom.direct3x3_ok / first3x3_ok / channels_last_ok and asrk_conv3x3_plan_info at
the live arguments), so a shape that falls back to another route fails instead of passing on that route's arithmetic.

Criterion, per tensor: helpers.rel_err < 1e-4 (outputs) / 1e-3 (gradients), the hard limits of tests/test_conv_gpu.py,
AND rel_err <= max(F * e32, 4 * 2**-24), e32 = rel_err of the float32 CPU run of the same reference against its float64
run on the row's inputs.  Every test prints e32, the bound, the device error and device / e32 (pytest -s, lines starting
CONVVAR).  Exact where the code promises it (torch.equal): zeros beyond hlen, zeros of dx at inputs no window reads, dW /
db over two runs, pooling ties, hlen = H + 3 against H and hlen = -2 against 0.

F is set per tensor kind to the largest device / e32 seen on the MI355X over every row below, times 4 (a tile-and-slab
summation order against the CPU library's own: both are f32 sums of the same exact f32 products), rounded up to a power
of two:

    tensor   largest device / e32   where                                      F
    y        5.56                   w_thmax_ragged (5.12 d_w20_128x128)        32
    dx       5.72                   w_s4_even2 (5.32 w_s2_walk)                32
    dw       1.77                   f_c3_64_w65_btcf_ld (GEMM route, K = 28)   8
    db       1.64                   g_cnn_odd (1.15 d_h1)                      8

(167 figures over 70 tests; e32 4e-8 ... 1.4e-6, device 4e-8 ... 1.5e-6.  The largest y / dx ratios all belong to rows
with 128 channels in the contraction: two channel passes of 9 x 64 products each, summed in MFMA order, against a CPU
library that blocks the same 1152 products differently.  The slab-summed dw / db of the walk rows - 40 000 positions
per sum - are at 0.13 ... 0.23 of e32: the CPU's float32 run loses more there than tiles and slabs do.)

The gradients' ReLU gate is discontinuous, so the table's dy is 0 where a pre-activation is within 1e-4 of 0
(conv_reference.near_zero_preactivations): no bound derived from rounding holds across a flipped gate, and large rows
have such elements more often than not.
"""
import ctypes
import importlib

import pytest
import torch
import torch.nn.functional as Fn

from conftest import PKG_NAME
from helpers import rel_err
import conv_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = dict(y=32, dx=32, dw=8, db=8)
KNOBS = ("ASRK_CONV_DIRECT", "ASRK_CONV_CL")
_cache = {}


@pytest.fixture(scope="module")
def C(pkg):
    return importlib.import_module(pkg.__name__ + ".conv_ops")


def _base(c):
    """inputs, full float64 reference and its float32 CPU run: computed once, shared by every test, never modified"""
    if c.name not in _cache:
        t = R.make_inputs(c)
        full = None if c.mode == 'len' else 'xwb'
        _cache[c.name] = (t, R.reference_of(c, t, grads=full), R.reference_of(c, t, dtype=torch.float32, grads=full))
    return _cache[c.name]


def _knobs(monkeypatch, c):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in c.env:
        monkeypatch.setenv(k, v)


def _device_inputs(C, c, t, grads=''):
    idx = R.layout_index(c)
    flat = torch.empty(idx.numel())
    flat[idx.flatten()] = t['x'].flatten()
    xd = flat.to(DEV).requires_grad_('x' in grads)
    wd = t['w'].to(DEV).requires_grad_('w' in grads)
    bd = t['b'].to(DEV).requires_grad_('b' in grads)
    geom = C.Geom(c.B, c.H, c.W, c.C, c.k[0], c.k[1], c.s[0], c.s[1], c.p[0], c.p[1], *R.strides(c))
    assert (geom.Ho, geom.Wo) == R.out_hw(c)
    return xd, wd, bd, geom, idx


def _assert_route(c, geom, xd, wd):
    """the route ConvFn.forward / conv_len will take, by their own predicates in their own order, and the live plan"""
    route = ('direct' if geom.direct3x3_ok(c.Cout, xd, wd) else 'first' if geom.first3x3_ok(c.Cout, wd)
             else 'im2col_cl' if geom.channels_last_ok(xd) else 'im2col_ld')
    assert route == c.route, "%s takes the %s route, the row is there for %s" % (c.name, route, c.route)
    L = importlib.import_module(PKG_NAME + "._lib").load()
    out = (ctypes.c_int * R.PLAN_LEN)()
    for fam, q in R.plan_queries(c).items():
        assert L.asrk_conv3x3_plan_info(*q, out, R.PLAN_LEN) == 0
        got = dict(zip(R.PLAN_FIELDS, out))
        assert got['supported'] == 1 or route.startswith('im2col')
        for field, v in c.plan.get(fam, {}).items():
            assert got[field] == v, (c.name, fam, field, got[field], v)


def _nchw(c, y):
    Ho, Wo = R.out_hw(c)
    return y.detach().cpu().view(c.B, Ho, Wo, c.Cout).permute(0, 3, 1, 2)


def _judge(label, got, ref, r32):
    bad = []
    for k, v in got.items():
        e32 = rel_err(r32[k], ref[k])
        err = rel_err(v.double(), ref[k])
        b = R.bound(e32, F[k], k)
        print("CONVVAR %s | %s | e32 %.3e | bound %.3e | device %.3e | device/e32 %.2f" % (label, k, e32, b, err, err / e32))
        if not (err < R.HARD[k] and err <= b):
            bad.append((k, err, b))
    assert not bad, (label, bad)


def _train(C, c, t, grads):
    """one forward and backward -> dict of CPU tensors in the reference's layouts"""
    xd, wd, bd, geom, idx = _device_inputs(C, c, t, grads)
    _assert_route(c, geom, xd, wd)
    y = C.conv(xd, wd, bd, geom, relu=c.relu)
    assert y.shape == (geom.M, c.Cout)
    y.backward(t['dy'].permute(0, 2, 3, 1).reshape(-1, c.Cout).contiguous().to(DEV))
    got = dict(y=_nchw(c, y))
    for k, v in (('x', xd), ('w', wd), ('b', bd)):
        if k in grads:
            got['d' + k] = v.grad.cpu().flatten()[idx] if k == 'x' else v.grad.cpu()
        else:
            assert v.grad is None, k
    return got


@pytest.mark.parametrize("case", R.TRAIN_CASES, ids=lambda c: c.name)
def test_training_row(ops, C, monkeypatch, case):
    c = case
    _knobs(monkeypatch, c)
    t, ref, r32 = _base(c)
    got = _train(C, c, t, c.grads)
    if c in R.REPEAT:
        again = _train(C, c, t, c.grads)
        assert torch.equal(again['dw'], got['dw']) and torch.equal(again['db'], got['db'])      # fixed-order slab sums
    ops.check_errors()
    if c.name in R.UNCOVERED:
        unc = R.uncovered_inputs(c)
        assert torch.equal(got['dx'][:, :, unc], torch.zeros_like(got['dx'][:, :, unc]))        # as in the reference
        assert float(ref['dx'][:, :, unc].abs().max()) == 0.0
    _judge(c.name, got, ref, r32)


@pytest.mark.parametrize("only", R.PARTIAL_GRADS)
@pytest.mark.parametrize("base", R.PARTIAL_BASES)
def test_partial_gradient_request(ops, C, monkeypatch, base, only):
    """requires_grad on one of weight / bias / input: that gradient against the same float64 gradient, the others stay
    None (ConvFn.backward passes dw == NULL or db == NULL to the weight-gradient entries)"""
    c = R.BY_NAME[base]
    _knobs(monkeypatch, c)
    t, ref, r32 = _base(c)
    got = _train(C, c, t, only)
    ops.check_errors()
    assert set(got) == {'y', 'd' + only}
    _judge("%s[%s only]" % (c.name, only), got, ref, r32)


def _len_run(C, c, t, hlen):
    xd, wd, bd, geom, _ = _device_inputs(C, c, t)
    _assert_route(c, geom, xd, wd)
    hd = torch.tensor(hlen, dtype=torch.int64, device=DEV)
    oh = R.out_hlen_of(c, hlen)
    with torch.no_grad():
        y = C.conv_len(xd, wd, bd, geom, hd, relu=c.relu,
                       out_hlen=None if oh is None else torch.tensor(oh, dtype=torch.int64, device=DEV))
    assert y.shape == (geom.M, c.Cout)
    return _nchw(c, y)


@pytest.mark.parametrize("case", R.LEN_CASES, ids=lambda c: c.name)
def test_length_row(ops, C, monkeypatch, case):
    c = case
    _knobs(monkeypatch, c)
    t, ref, r32 = _base(c)
    y = _len_run(C, c, t, c.hlen)
    above = _len_run(C, c, t, tuple(h + 3 if h == c.H else h for h in c.hlen))
    below = _len_run(C, c, t, tuple(-2 if h == 0 else h for h in c.hlen))
    ops.check_errors()
    oh = R.out_hlen_of(c) or tuple(max(0, min(h, c.H)) for h in c.hlen)
    for i, n in enumerate(oh):
        tail = y[i, :, n:]
        assert torch.equal(tail, torch.zeros_like(tail)), (c.name, i)                # exactly 0 beyond the valid height
        assert n == 0 or float(y[i, :, :n].abs().max()) > 0.0
    assert torch.equal(above, y) and torch.equal(below, y)                           # hlen is clamped to [0, H]
    _judge(c.name, dict(y=y), ref, r32)


def test_maxpool_ties_follow_the_first_maximum(ops, C):
    """an input that went through ReLU ties at 0 in many windows: values and dx equal F.max_pool2d's, which sends a tied
    window's gradient to its first maximum in (dh, dw) row-major order"""
    x, dy = R.pool_ties_input()
    B, Ch, H, W = x.shape
    xr = x.clone().requires_grad_(True)
    yr = Fn.max_pool2d(xr, 2, stride=2)
    yr.backward(dy)
    Ho, Wo = H // 2, W // 2
    xd = x.permute(0, 2, 3, 1).contiguous().to(DEV).requires_grad_(True)
    y = C.maxpool2x2(xd, (B, H, W, Ch), (B, Ho, Wo, Ch), (Ho * Wo * Ch, Wo * Ch, Ch, 1))
    y.backward(dy.permute(0, 2, 3, 1).contiguous().to(DEV))
    ops.check_errors()
    assert torch.equal(y.detach().cpu().permute(0, 3, 1, 2), yr.detach())
    assert torch.equal(xd.grad.cpu().permute(0, 3, 1, 2), xr.grad)


def test_relu_bwd_stops_at_exact_zeros(ops):
    y, dy = R.relu_zero_input()
    L = ops._L()
    yd, dyd = y.to(DEV), dy.to(DEV)
    dx = torch.full_like(dyd, 7.0)
    lib = importlib.import_module(PKG_NAME + "._lib")
    lib.check(L.asrk_relu_bwd_f32(ops._p(yd), ops._p(dyd), ops._p(dx), y.numel(), ops._stream()), "relu_bwd")
    ops.check_errors()
    assert torch.equal(dx.cpu(), torch.where(y > 0, dy, torch.zeros_like(dy)))
