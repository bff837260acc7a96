"""GPU: every kernel variant of the streaming helpers against the float64 references and on the case tables of
tests/rowops_reference.py - csrc/rowops.hip: the six copy3d instantiations and the three colsum kernels; csrc/norm.hip: the
three LayerNorm kernels and both dropout instantiations; csrc/optim.hip: the three single-tensor step kernels, the two
multi-tensor ones, the two stages of the gradient norm and the fill kernel (22 instantiations).  Through the C ABI wherever
ops.py cannot reach a variant.  tests/test_rowops_plan_cpu.py holds every row to the kernel it names, and every row asserts
that plan again at its live pointers before it runs (asrk_rowops_plan_info), so a shape that drifts onto another kernel
fails instead of passing on that kernel's arithmetic.

Every output lies inside an allocation pre-filled with NaN (fill: with a sentinel), with slack around it and, where the
layout has them, gaps inside it; nothing outside the addressed elements may change.

Exact (bit for bit): copy3d on the whole destination allocation; colsum, db of LayerNorm with integer dy and the gradient
norm on inputs k/8 whose sums are exact in any order; dropout against the numpy Philox oracle, the whole tensor at the
grid-stride sizes too (the oracle takes a second for 8.4 M elements); the single-tensor optimiser steps against the
multi-tensor form; fill.

Two copy3d branches need more than 1 GiB of destination and are held by the plan test on the CPU only: rows per workgroup
= ceil(rows / 65535), and the fallback to the generic kernel from 2^30 rows on.

Criterion for LayerNorm and the optimiser steps, per tensor: rel_err (tests/helpers.py) inside the hard limit the suite
already holds the op to - LayerNorm 1e-4 forward, 1e-3 gradients; optimiser 2e-6 against torch's float32 run - AND
rel_err <= max(F * e32, 4 * 2**-24) against the float64 reference, e32 = rel_err of torch's float32 CPU run of the op
(native_layer_norm and its autograd; torch.optim) against float64 on the row's inputs.  Every test prints
    ROWVAR name | kind | e32 | bound | device | device/e32
(pytest -s).  F is set per tensor kind to the largest device / e32 seen on the MI355X over every row below, times 4, rounded
up to a power of two:

    tensor            largest device / e32   where (next)                                               F
    ln_y              1.83                   d65_r3 (1.77 d64_r5)                                       8
    ln_mean           1.94                   d64_r5 (1.52 const_row)                                    8
    ln_rstd           2.36                   d65_r1 (1.52 d129_r65)                                     16
    ln_dx             1.56                   eps0 (1.53 d65_r4)                                         8
    ln_dw             2.15                   d65_r1, the same through ops.py and deterministic          16
    ln_db             3.00                   d2_r5 (1.94 d63_r5)                                        16
    adadelta_param    1.00                   vec_loop, vec without a coefficient and most other rows    4
    adadelta_state0   1.38                   vec_loop (1.31 table gap_at_edge26)                        8
    adadelta_state1   1.03                   odd without a coefficient, odd with one above 1            8
    adam_param        1.00                   vec_loop, vec without a coefficient and most other rows    4
    adam_state0       1.49                   table n24 (1.31 misaligned, coefficient below 1)           8
    adam_state1       1.54                   vec without a coefficient, vec with one above 1            8

(306 figures over 242 tests; e32 9.2e-09 ... 6.0e-05, device 0 ... 3.3e-05.)  What the figures say:
  - Nothing is decided by F: every ratio is between 0 and 3, the device lands where torch's float32 CPU run lands.  The
    LayerNorm kernels sum a row over 64 lanes and a shuffle tree where torch sums vector lanes, the parameter gradient adds
    its row chunks in whatever order the atomics arrive (d65_r257 dw gave 0.99 and 0.82 in two sessions); both are a few
    roundings of the largest element.  The parameters after six optimiser steps are the float32 CPU run's to three digits
    of the ratio, and the single-tensor kernels are the multi-tensor kernel bit for bit (asserted).
  - The rows where e32 is 0 or the reference is 0 (D = 1: y = bias, dx = dw = 0; eps = 0 at D = 2: dx = 0; the constant
    row) are met exactly by the device as well and are not in the table.
  - D = 2 with a variance far above eps has NO float32 answer for dx (it is eps / (var + eps) of the terms it is the
    difference of: torch's CPU run is off by 2e-2 there, the kernel by 1e-2); the D = 2 row therefore has a spread
    comparable with sqrt(eps), see tests/rowops_reference.py.
"""
import ctypes
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import PKG_NAME
import rowops_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
NAN = float('nan')
EINVAL, EWORKSPACE = -1, -3
F = dict(ln_y=8, ln_mean=8, ln_rstd=16, ln_dx=8, ln_dw=16, ln_db=16,
         adadelta_param=4, adadelta_state0=8, adadelta_state1=8, adam_param=4, adam_state0=8, adam_state1=8)


def _lib():
    return importlib.import_module(PKG_NAME + "._lib")


class Judge:
    """collects every tensor of a test, prints its line, and fails at the end with all of them"""

    def __init__(self, name):
        self.name, self.bad = name, []

    def add(self, kind, e32, err, hard_err, hard):
        b = R.bound(e32, F[kind])
        print("ROWVAR %s | %s | e32 %.3e | bound %.3e | device %.3e | device/e32 %.2f" % (
            self.name, kind, e32, b, err, err / e32 if e32 > 0 else float('nan')))
        if not hard_err < hard or not err <= b:
            self.bad.append((kind, err, b, hard_err))

    def done(self):
        assert not self.bad, (self.name, self.bad)


def bits(t):
    """a float32 tensor or array as int32 numpy"""
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().contiguous().numpy()
    return np.ascontiguousarray(t, np.float32).view(np.int32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


class Guarded:
    """a float32 device view of n elements `off` floats into an allocation filled with `fill`, `tail` floats of slack behind"""

    def __init__(self, n, off=4, tail=5, fill=NAN, data=None):
        self.n, self.off = n, off
        self.buf = torch.full((off + n + tail,), fill, device=DEV)
        assert self.buf.data_ptr() % 16 == 0
        self.view = self.buf[off:off + n]
        self.fill = np.float32(fill)
        if data is not None:
            self.view.copy_(torch.as_tensor(np.asarray(data, np.float32).reshape(-1)))

    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + 4 * self.off)

    def get(self):
        return self.view.cpu().numpy()

    def slack_untouched(self):
        b = bits(self.buf)
        want = np.full((1,), self.fill, np.float32).view(np.int32)[0]
        return bool((b[:self.off] == want).all() and (b[self.off + self.n:] == want).all())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ====================================================================================================== copy3d
@pytest.mark.parametrize("acc", [0, 1], ids=["copy", "acc"])
@pytest.mark.parametrize("case", R.COPY3D_CASES, ids=lambda c: c.name)
def test_copy3d_row(ops, case, acc):
    """the whole destination allocation, bit for bit: the addressed elements, the gaps between rows and planes and the slack
    around them (NaN before the call, NaN after)"""
    c = case
    src, dst0, _, _ = R.copy3d_buffers(c.name)
    sd = dev(src)
    dd = dev(dst0) if acc else torch.full((dst0.size,), NAN, device=DEV)
    sp, dp = sd.data_ptr() + 4 * c.soff, dd.data_ptr() + 4 * c.doff
    assert sd.data_ptr() % 16 == 0 and dd.data_ptr() % 16 == 0
    got = R.plan(ops._L(), R.OP_COPY3D, [sp, dp], [c.n0, c.n1, c.n2, c.ss0, c.ss1, c.ds0, c.ds1, acc])
    assert got['variant'] == c.variant + acc, (c.name, R.COPY3D_VARIANTS[got['variant']])
    for field, v in c.plan.items():
        assert got[field] == v, (c.name, field, got[field], v)
    _lib().check(ops._L().asrk_copy3d_f32(ctypes.c_void_p(sp), ctypes.c_void_p(dp), c.n0, c.n1, c.n2, c.ss0, c.ss1, c.ds0,
                                          c.ds1, acc, ops._stream()), "copy3d")
    ops.check_errors()
    want = R.copy3d_expected(c.name, acc)
    g = bits(dd)
    if not np.array_equal(g, bits(want)):
        bad = np.flatnonzero(g != bits(want))
        raise AssertionError("%s: %d of %d floats differ, the first at %d" % (c.name, bad.size, g.size, bad[0]))
    assert same_bits(sd, src)                                        # the source is read-only


def test_copy3d_empty_and_invalid(ops):
    L, st = ops._L(), ops._stream()
    d = Guarded(64)
    s = dev(R.exact_ints((64,), 1))
    for dims in ((0, 4, 16), (4, 0, 16), (4, 4, 0)):
        assert L.asrk_copy3d_f32(ops._p(s), d.ptr(), *dims, 16, 4, 16, 4, 0, st) == 0
    assert L.asrk_copy3d_f32(ops._p(s), d.ptr(), -1, 4, 4, 16, 4, 16, 4, 0, st) == EINVAL
    assert L.asrk_copy3d_f32(None, d.ptr(), 1, 4, 4, 16, 4, 16, 4, 0, st) == EINVAL
    ops.check_errors()
    assert np.isnan(d.buf.cpu().numpy()).all()


# ====================================================================================================== colsum
def _colsum(ops, c, acc, out_off=3):
    buf, out0 = R.colsum_inputs(c.name)
    xd = dev(buf)
    assert xd.data_ptr() % 16 == 0
    xp = xd.data_ptr() + 4 * c.off
    out = Guarded(c.N, off=out_off, data=out0 if acc else None)
    got = R.plan(ops._L(), R.OP_COLSUM, [xp, out.ptr().value], [c.M, c.N, c.ldx, acc])
    _lib().check(ops._L().asrk_colsum_f32(ctypes.c_void_p(xp), c.M, c.N, c.ldx, out.ptr(), acc, ops._stream()), "colsum")
    ops.check_errors()
    return got, out


@pytest.mark.parametrize("case", R.COLSUM_CASES, ids=lambda c: c.name)
def test_colsum_row(ops, case):
    """accumulate = 0 on top of NaN and accumulate = 1 on top of a known out: the float64 sums bit for bit (exact inputs), in
    their own columns (every column has its own signature), nothing beside out touched"""
    c = case
    for acc in (0, 1):
        got, out = _colsum(ops, c, acc)
        assert got['variant'] == c.variant, (c.name, R.COLSUM_VARIANTS[got['variant']])
        for field, v in c.plan.items():
            assert got[field] == v, (c.name, field, got[field], v)
        want = R.colsum_expected(c.name, acc)
        g = out.get()
        assert same_bits(g, want), (c.name, acc, np.flatnonzero(g != want)[:8], g[g != want][:8], want[g != want][:8])
        assert out.slack_untouched()


def test_colsum_degenerate_sizes(ops):
    L, st = ops._L(), ops._stream()
    x = dev(R.exact_ints((64,), 2))
    out = Guarded(8)
    assert L.asrk_colsum_f32(ops._p(x), 0, 8, 8, out.ptr(), 1, st) == 0           # M = 0, accumulate: out left alone
    assert L.asrk_colsum_f32(ops._p(x), 5, 0, 8, out.ptr(), 0, st) == 0           # N = 0: nothing
    ops.check_errors()
    assert np.isnan(out.buf.cpu().numpy()).all()
    assert L.asrk_colsum_f32(None, 0, 8, 8, out.ptr(), 0, st) == 0                # M = 0: out zeroed, X not needed
    ops.check_errors()
    assert same_bits(out.get(), np.zeros(8, np.float32)) and out.slack_untouched()
    assert L.asrk_colsum_f32(ops._p(x), 5, 8, 7, out.ptr(), 0, st) == EINVAL
    assert L.asrk_colsum_f32(ops._p(x), -1, 8, 8, out.ptr(), 0, st) == EINVAL
    assert L.asrk_colsum_f32(None, 5, 8, 8, out.ptr(), 0, st) == EINVAL
    ops.check_errors()
    assert same_bits(out.get(), np.zeros(8, np.float32))


# ====================================================================================================== LayerNorm
def _ln_abi(ops, c, want_dx=True, want_dw=True):
    """forward and backward through the C ABI, every output guarded -> dict of Guarded"""
    L, st = ops._L(), ops._stream()
    x, w, b, dy = (dev(t.numpy()) for t in R.ln_inputs(c.name))
    n = c.rows * c.D
    o = dict(y=Guarded(n, off=3), mean=Guarded(c.rows, off=1), rstd=Guarded(c.rows, off=2), dx=Guarded(n, off=5),
             dw=Guarded(c.D, off=1), db=Guarded(c.D, off=3))
    _lib().check(L.asrk_layer_norm_fwd_f32(ops._p(x), ops._p(w), ops._p(b), o['y'].ptr(), o['mean'].ptr(), o['rstd'].ptr(),
                                           c.rows, c.D, c.eps, st), "layer_norm_fwd")
    _lib().check(L.asrk_layer_norm_bwd_f32(ops._p(x), ops._p(w), ops._p(dy), o['mean'].ptr(), o['rstd'].ptr(),
                                           o['dx'].ptr() if want_dx else None, o['dw'].ptr() if want_dw else None,
                                           o['db'].ptr() if want_dw else None, c.rows, c.D, st), "layer_norm_bwd")
    ops.check_errors()
    return o


def _ln_judge(label, c, got, kinds=R.LN_KINDS):
    ref, e32 = R.ln_expected(c.name), R.ln_e32(c.name)
    j = Judge(label)
    for k in kinds:
        g = got[k].reshape(ref[k].shape)
        assert np.isfinite(g).all(), (label, k)
        err = R.rel_err(g, ref[k])
        j.add('ln_' + k, e32[k], err, err, R.LN_HARD[k])
    j.done()


@pytest.mark.parametrize("case", R.LN_CASES, ids=lambda c: c.name)
def test_layer_norm_row(ops, case):
    c = case
    got = R.plan(ops._L(), R.OP_LN_PARAM, [], [c.rows, c.D])
    for field, v in c.plan.items():
        assert got[field] == v, (c.name, field, got[field], v)
    o = _ln_abi(ops, c)
    assert all(g.slack_untouched() for g in o.values()), c.name
    res = {k: g.get() for k, g in o.items()}
    _ln_judge(c.name, c, res)
    if c.kind == 'int_dy':                                           # sums of k/8: exact in any order
        assert same_bits(res['db'], R.ln_expected(c.name)['db'].astype(np.float32)), c.name
    if c.kind == 'const_row':                                        # variance exactly 0: rstd = 1 / sqrt(eps), y = bias
        eps = np.float32(c.eps)
        assert res['rstd'][R.CONST_ROW] == np.float32(1.0) / np.sqrt(eps)
        assert same_bits(res['y'].reshape(c.rows, c.D)[R.CONST_ROW], R.ln_inputs(c.name)[2].numpy())
    # the autograd path of ops.py is the same two calls
    x, w, b, dy = (t.to(DEV) for t in R.ln_inputs(c.name))
    x.requires_grad_(True); w.requires_grad_(True); b.requires_grad_(True)
    y = ops.layer_norm(x, w, b, c.eps)
    dx, dw, db = torch.autograd.grad(y, (x, w, b), dy)
    ops.check_errors()
    assert same_bits(y, res['y'].reshape(c.rows, c.D)) and same_bits(dx, res['dx'].reshape(c.rows, c.D))
    _ln_judge(c.name + "[ops]", c, dict(dw=dw.cpu().numpy(), db=db.cpu().numpy()), kinds=('dw', 'db'))


@pytest.mark.parametrize("name", ['d65_r65', 'd129_r65'])
def test_layer_norm_optional_outputs(ops, name):
    """dx NULL with dw / db set, dw = db = NULL with dx set: the present outputs as in the full call, the absent ones not
    written; exactly one of dw / db NULL is refused; rows = 0 zeroes dw / db"""
    c = R.LN_BY_NAME[name]
    L, st = ops._L(), ops._stream()
    full = _ln_abi(ops, c)
    no_dx = _ln_abi(ops, c, want_dx=False)
    assert np.isnan(no_dx['dx'].buf.cpu().numpy()).all()
    _ln_judge(name + "[dx NULL]", c, {k: no_dx[k].get() for k in ('dw', 'db')}, kinds=('dw', 'db'))
    no_dw = _ln_abi(ops, c, want_dw=False)
    assert np.isnan(no_dw['dw'].buf.cpu().numpy()).all() and np.isnan(no_dw['db'].buf.cpu().numpy()).all()
    assert same_bits(no_dw['dx'].get(), full['dx'].get()) and no_dw['dx'].slack_untouched()
    x, w, b, dy = (dev(t.numpy()) for t in R.ln_inputs(c.name))
    dw, db, dx = Guarded(c.D), Guarded(c.D), Guarded(c.rows * c.D)
    head = (ops._p(x), ops._p(w), ops._p(dy), full['mean'].ptr(), full['rstd'].ptr())
    assert L.asrk_layer_norm_bwd_f32(*head, dx.ptr(), dw.ptr(), None, c.rows, c.D, st) == EINVAL
    assert L.asrk_layer_norm_bwd_f32(*head, dx.ptr(), None, db.ptr(), c.rows, c.D, st) == EINVAL
    ops.check_errors()
    assert all(np.isnan(g.buf.cpu().numpy()).all() for g in (dw, db, dx))
    assert L.asrk_layer_norm_bwd_f32(None, None, None, None, None, None, dw.ptr(), db.ptr(), 0, c.D, st) == 0
    ops.check_errors()
    for g in (dw, db):
        assert same_bits(g.get(), np.zeros(c.D, np.float32)) and g.slack_untouched()


# ====================================================================================================== dropout
def _dropout(ops, x, p, seed, offset, x_off=4, y_off=4, expect=0):
    """asrk_dropout_f32 on views x_off / y_off floats into aligned allocations -> (plan, Guarded y)"""
    xg = Guarded(x.size, off=x_off, data=x)
    y = Guarded(x.size, off=y_off)
    got = R.plan(ops._L(), R.OP_DROPOUT, [xg.ptr().value, y.ptr().value], [x.size])
    rc = ops._L().asrk_dropout_f32(xg.ptr(), y.ptr(), x.size, p, ctypes.c_uint64(seed), ctypes.c_uint64(offset),
                                   ops._stream())
    assert rc == expect, rc
    ops.check_errors()
    return got, y


@pytest.mark.parametrize("name,n,variant", R.DROP_SIZES)
def test_dropout_sizes(ops, name, n, variant):
    """both instantiations below and beyond the 8192-workgroup cap (the grid-stride loop's second pass), the whole tensor
    against the numpy Philox oracle"""
    x = R.dropout_input(n)
    seed, offset = 0x9E3779B97F4A7C15, 3
    got, y = _dropout(ops, x, 0.5, seed, offset)
    assert got['variant'] == variant and got['gx'] == min(8192, -(-got['items'] // 256)), got
    assert ('loop' in name) == (got['items'] > 8192 * 256)
    want = R.dropout_expected(x, 0.5, seed, offset)
    g = y.get()
    assert same_bits(g, want), (name, np.flatnonzero(g != want)[:8])
    assert y.slack_untouched()


@pytest.mark.parametrize("offset", R.DROP_OFFSETS)
def test_dropout_offset_word(ops, offset):
    """the offset words of the Philox counter, the high one included, on both instantiations"""
    for n, variant in ((4100, 1), (4099, 0)):
        x = R.dropout_input(n, seed=n)
        got, y = _dropout(ops, x, 0.3, 0x0123456789ABCDEF, offset)
        assert got['variant'] == variant
        assert same_bits(y.get(), R.dropout_expected(x, 0.3, 0x0123456789ABCDEF, offset)), (offset, n)
        assert y.slack_untouched()
    if offset:
        assert not same_bits(y.get(), R.dropout_expected(x, 0.3, 0x0123456789ABCDEF, 0))


@pytest.mark.parametrize("name,p", R.DROP_P)
def test_dropout_thresholds(ops, name, p):
    x = R.dropout_input(70001, seed=9)[:70000]
    got, y = _dropout(ops, x, p, 42, 0)
    want = R.dropout_expected(x, p, 42, 0)
    assert same_bits(y.get(), want) and y.slack_untouched()
    if name == 'thresh0':
        assert same_bits(y.get(), x)                                 # threshold 0 keeps everything, scale is 1
    if name == 'almost_one':                                         # one word in 2^24 survives, scaled by 2^24
        kept = y.get() != 0
        assert kept.sum() <= 2 and np.array_equal(y.get()[kept], x[kept] * np.float32(2.0 ** 24))


def test_dropout_refuses_p_outside_the_half_open_interval(ops):
    x = R.dropout_input(64)
    for p in (1.0, NAN, -0.25, 1.5):
        _, y = _dropout(ops, x, p, 1, 0, expect=EINVAL)
        assert np.isnan(y.buf.cpu().numpy()).all()


def test_dropout_backward_rederives_the_mask_on_a_misaligned_gradient(ops):
    """forward on aligned x (16-byte kernel), backward = the same call on a dy one float off alignment (scalar kernel): the
    same elements survive"""
    n, seed, offset = 8200, 77, 2 ** 32 + 1
    x, dy = R.dropout_input(n, seed=1), R.dropout_input(n, seed=2)
    fwd, y = _dropout(ops, x, 0.5, seed, offset)
    bwd, dx = _dropout(ops, dy, 0.5, seed, offset, x_off=1, y_off=4)
    assert (fwd['variant'], bwd['variant']) == (1, 0)
    assert np.array_equal(y.get() != 0, dx.get() != 0)
    assert same_bits(dx.get(), R.dropout_expected(dy, 0.5, seed, offset)) and dx.slack_untouched()


# ====================================================================================================== optimiser steps
def _coef_tensor(coef):
    return None if coef is None else torch.tensor([coef], dtype=torch.float32, device=DEV)


def _ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def _single_step(ops, kind, views, g, n, step, coef_t):
    L, st, p = ops._L(), ops._stream(), ops._p
    a = [ctypes.c_void_p(v.data_ptr()) for v in views]
    if kind == 'adadelta':
        hp = R.ADADELTA_HP
        rc = L.asrk_adadelta_step_f32(a[0], p(g), a[1], a[2], n, hp['lr'], hp['rho'], hp['eps'], p(coef_t), st)
    else:
        hp = R.ADAM_HP
        rc = L.asrk_adam_step_f32(a[0], p(g), a[1], a[2], n, hp['lr'], hp['beta1'], hp['beta2'], hp['eps'], step, p(coef_t), st)
    _lib().check(rc, kind + "_step")


def _multi_step(ops, kind, params, grads, s0, s1, sizes, step, coef_t):
    """-> rc; lists of tensors (None for an empty entry: a NULL pointer)"""
    L, st = ops._L(), ops._stream()
    n = (ctypes.c_int64 * len(sizes))(*sizes)
    arrs = [_ptr_array(t) for t in (params, grads, s0, s1)]
    if kind == 'adadelta':
        hp = R.ADADELTA_HP
        return L.asrk_adadelta_multi_f32(len(sizes), *arrs, n, hp['lr'], hp['rho'], hp['eps'], ops._p(coef_t), st)
    hp = R.ADAM_HP
    return L.asrk_adam_multi_f32(len(sizes), *arrs, n, hp['lr'], hp['beta1'], hp['beta2'], hp['eps'], step, ops._p(coef_t), st)


def _reference(kind, p0, grads, coef, dtype=np.float64):
    if kind == 'adadelta':
        return R.adadelta_reference(p0, grads, coef, dtype=dtype, **R.ADADELTA_HP)
    return R.adam_reference(p0, grads, coef, dtype=dtype, **R.ADAM_HP)


def _opt_judge(label, kind, runs, p0, grads, coef, e32):
    """runs: per step (p, s0, s1) numpy from the device"""
    ref = _reference(kind, p0, grads, coef)
    skip, _ = R.clip_of(coef)
    if skip:                                                         # the NaN rule: bit-identical to before
        for p, s0, s1 in runs:
            assert same_bits(p, p0) and not s0.any() and not s1.any(), label
        return
    t32 = R.torch_optim_run(kind, p0, grads, coef, torch.float32)
    j = Judge(label)
    for i, k in enumerate(R.OPT_KINDS):
        err = max(R.rel_err(r[i], f[i]) for r, f in zip(runs, ref))
        hard = max(R.rel_err(r[i], t[i]) for r, t in zip(runs, t32))
        j.add('%s_%s' % (kind, k), e32[i], err, hard, R.OPT_HARD)
    j.done()


def _single_against_multi(ops, kind, n, mis, coef, steps, seed):
    p0, grads = R.opt_inputs(n, seed, steps)
    coef_t = _coef_tensor(coef)
    # single: the state one float off alignment where the row says so; multi: copies of the same tensors
    single = [Guarded(n, off=4, data=p0), Guarded(n, off=4 + mis, data=np.zeros(n)), Guarded(n, off=4, data=np.zeros(n))]
    multi = [Guarded(n, off=4, data=p0), Guarded(n, off=4 + mis, data=np.zeros(n)), Guarded(n, off=4, data=np.zeros(n))]
    if kind == 'adadelta':
        got = R.plan(ops._L(), R.OP_ADADELTA, [single[0].ptr().value, 0x1000, single[1].ptr().value, single[2].ptr().value], [n])
        assert got['variant'] == int(n % 4 == 0 and not mis), got
        assert (got['items'] > 4096 * 256) == (n > R.OPT_LOOP)
    runs = []
    for step in range(1, steps + 1):
        g = dev(grads[step - 1])
        assert g.data_ptr() % 16 == 0
        _single_step(ops, kind, [s.view for s in single], g, n, step, coef_t)
        rc = _multi_step(ops, kind, [multi[0].view], [g], [multi[1].view], [multi[2].view], [n], step, coef_t)
        _lib().check(rc, kind + "_multi")
        ops.check_errors()
        for a, b, k in zip(single, multi, R.OPT_KINDS):              # the source's claim: element-identical arithmetic
            assert torch.equal(a.buf.view(torch.int32), b.buf.view(torch.int32)), (kind, n, mis, coef, step, k)
        runs.append(tuple(s.get() for s in single))
    assert all(s.slack_untouched() for s in single + multi)
    return p0, grads, runs


@pytest.mark.parametrize("coef_name,coef", R.OPT_COEFS)
@pytest.mark.parametrize("name,n,mis", [r for r in R.OPT_SINGLE if 'loop' not in r[0]])
@pytest.mark.parametrize("kind", ['adadelta', 'adam'])
def test_single_tensor_steps(ops, kind, name, n, mis, coef_name, coef):
    """six steps of the single-tensor entry (16-byte, scalar by n % 4, scalar by alignment) bit for bit against the
    multi-tensor entry, and both against the float64 recurrence"""
    p0, grads, runs = _single_against_multi(ops, kind, n, mis, coef, R.OPT_STEPS, seed=n + mis)
    e32 = None if R.clip_of(coef)[0] else R.opt_e32(kind, n, n + mis, coef)
    _opt_judge("%s[%s %s]" % (kind, name, coef_name), kind, runs, p0, grads, coef, e32)


@pytest.mark.parametrize("name,n,mis", [r for r in R.OPT_SINGLE if 'loop' in r[0]])
@pytest.mark.parametrize("kind", ['adadelta', 'adam'])
def test_single_tensor_steps_beyond_the_grid_cap(ops, kind, name, n, mis):
    """n above 4096 x 256 x 4: the grid-stride loop of every single-tensor kernel runs a second pass (two steps)"""
    p0, grads, runs = _single_against_multi(ops, kind, n, mis, 0.37, 2, seed=5)
    _opt_judge("%s[%s]" % (kind, name), kind, runs, p0, grads, 0.37, R.opt_e32(kind, n, 5, 0.37, 2))


class Table:
    """the tensors of a table laid end to end in one guarded allocation per role, 3 floats of NaN between them (so every
    alignment occurs); empty entries are None (NULL pointers)"""

    def __init__(self, sizes, roles, data=None):
        self.sizes = sizes
        self.starts = np.cumsum([0] + [n + 3 for n in sizes])[:-1]
        self.total = int(sum(n + 3 for n in sizes))
        self.g = {r: Guarded(self.total, off=4) for r in roles}
        for r, d in (data or {}).items():
            for s, n, t in zip(self.starts, sizes, d):
                self.g[r].view[s:s + n] = torch.from_numpy(np.asarray(t, np.float32)).to(DEV)

    def tensors(self, role):
        return [None if n == 0 else self.g[role].view[s:s + n] for s, n in zip(self.starts, self.sizes)]

    def payload(self, role):
        a = self.g[role].get()
        return np.concatenate([a[s:s + n] for s, n in zip(self.starts, self.sizes)])

    def gaps_untouched(self, role):
        a = self.g[role].get()
        return all(np.isnan(a[s + n:s + n + 3]).all() for s, n in zip(self.starts, self.sizes)) and self.g[role].slack_untouched()


def _split(flat, sizes):
    return np.split(flat, np.cumsum(sizes)[:-1])


@pytest.mark.parametrize("table", list(R.TABLES))
@pytest.mark.parametrize("kind", ['adadelta', 'adam'])
def test_multi_tensor_table_boundaries(ops, kind, table):
    """23 / 24 / 25 / 49 table entries, empty ones (NULL pointers) at the edges of the 24-slot launches, a tensor of one
    element and one beyond the 2048-workgroup cap: two steps against the float64 recurrence, gaps untouched"""
    sizes = R.TABLES[table]
    total = sum(sizes)
    p0, grads = R.opt_inputs(total, len(sizes), 2)
    tb = Table(sizes, ('p', 's0', 's1'), dict(p=_split(p0, sizes), s0=_split(np.zeros(total), sizes),
                                              s1=_split(np.zeros(total), sizes)))
    coef_t = _coef_tensor(0.37)
    runs = []
    for step in (1, 2):
        gt = Table(sizes, ('g',), dict(g=_split(grads[step - 1], sizes)))
        rc = _multi_step(ops, kind, tb.tensors('p'), gt.tensors('g'), tb.tensors('s0'), tb.tensors('s1'), sizes, step, coef_t)
        _lib().check(rc, kind + "_multi")
        ops.check_errors()
        assert same_bits(gt.payload('g'), grads[step - 1])           # gradients are read-only
        runs.append(tuple(tb.payload(r) for r in ('p', 's0', 's1')))
    assert all(tb.gaps_untouched(r) for r in ('p', 's0', 's1'))
    _opt_judge("%s[table %s]" % (kind, table), kind, runs, p0, grads, 0.37, R.opt_e32(kind, total, len(sizes), 0.37, 2))


@pytest.mark.parametrize("bad", ['numel', 'param', 'grad', 'state'])
@pytest.mark.parametrize("kind", ['adadelta', 'adam'])
def test_multi_tensor_invalid_entry_leaves_every_tensor_alone(ops, kind, bad):
    """30 entries, entry 27 invalid (numel = -1 or a NULL pointer): ASRK_EINVAL and all 30 parameters and states
    bit-identical to before - the first 24 are not stepped before the error is found"""
    sizes = [40 + 3 * t for t in range(30)]
    total = sum(sizes)
    p0, grads = R.opt_inputs(total, 30, 1)
    s0 = np.abs(R.opt_inputs(total, 31, 1)[0])
    data = dict(p=_split(p0, sizes), s0=_split(s0, sizes), s1=_split(s0 * 0.5, sizes), g=_split(grads[0], sizes))
    tb = Table(sizes, ('p', 's0', 's1', 'g'), data)
    before = {r: bits(tb.g[r].buf).copy() for r in ('p', 's0', 's1', 'g')}
    lists = {r: tb.tensors(r) for r in ('p', 'g', 's0', 's1')}
    n = list(sizes)
    if bad == 'numel':
        n[27] = -1
    else:
        lists[dict(param='p', grad='g', state='s1')[bad]][27] = None
    assert _multi_step(ops, kind, lists['p'], lists['g'], lists['s0'], lists['s1'], n, 1, None) == EINVAL
    ops.check_errors()
    for r in before:
        assert np.array_equal(bits(tb.g[r].buf), before[r]), (kind, bad, r)
    # the valid table steps all 30
    _lib().check(_multi_step(ops, kind, tb.tensors('p'), tb.tensors('g'), tb.tensors('s0'), tb.tensors('s1'), sizes, 1, None),
                 kind + "_multi")
    ops.check_errors()
    moved = _split(bits(tb.payload('p')) != bits(p0), sizes)
    assert all(m.any() for m in moved)


# ====================================================================================================== gradient norm
def _grad_norm(ops, tensors, sizes, max_norm, want_norm=True, want_coef=True, ws_short=0, ws_off=0, ws=None):
    """-> (rc, Guarded out [norm, coef], Guarded ws)"""
    L, st = ops._L(), ops._stream()
    n = (ctypes.c_int64 * len(sizes))(*sizes)
    need = L.asrk_grad_norm_ws_bytes(len(sizes), n)
    assert need % 8 == 0 and need == 8 * (sum(R.norm_blocks_of(s) for s in sizes if s > 0) + 1)
    ws = ws or Guarded(need // 4, off=4 + ws_off)
    out = Guarded(2, off=3)
    norm_p = ctypes.c_void_p(out.ptr().value) if want_norm else None
    coef_p = ctypes.c_void_p(out.ptr().value + 4) if want_coef else None
    rc = L.asrk_grad_norm_multi_f32(len(sizes), _ptr_array(tensors), n, max_norm, norm_p, coef_p, ws.ptr(), need - ws_short, st)
    ops.check_errors()
    return rc, out, ws


@pytest.mark.parametrize("table", list(R.TABLES))
def test_grad_norm_exact(ops, table):
    """gradients k/8: every float32 per-thread sum and every double beyond is exact, so norm is float(sqrt(exact sum)) and
    coef is max_norm / (norm + 1e-6f) in float32, bit for bit; twice"""
    sizes = R.TABLES[table]
    grads = R.grad_norm_inputs(sizes, 5)
    tb = Table(sizes, ('g',), dict(g=grads))
    for max_norm in (5.0, 1e-3):
        norm, coef = R.grad_norm_expected(grads, max_norm)
        for _ in range(2):
            rc, out, ws = _grad_norm(ops, tb.tensors('g'), sizes, max_norm)
            assert rc == 0
            got = out.get()
            assert same_bits(got, np.array([norm, coef], np.float32)), (table, got, norm, coef)
            assert out.slack_untouched() and ws.slack_untouched()
    assert same_bits(tb.payload('g'), np.concatenate(grads)) and tb.gaps_untouched('g')


def test_grad_norm_inexact_inputs_against_float64(ops):
    sizes = R.TABLES['e49']
    g = np.random.RandomState(3)
    grads = [(g.standard_normal(n) * 10.0 ** g.uniform(-3, 1)).astype(np.float32) for n in sizes]
    tb = Table(sizes, ('g',), dict(g=grads))
    want = R.grad_norm_float64(grads)
    res = []
    for _ in range(2):
        rc, out, _ = _grad_norm(ops, tb.tensors('g'), sizes, 5.0)
        assert rc == 0
        res.append(out.get())
    assert same_bits(res[0], res[1])                                 # two fixed-order stages: bit-reproducible
    # float32 per thread over at most 9 squares, double beyond: a few roundings of the norm
    print("ROWVAR grad_norm[e49 randn] | rel err %.3e" % (abs(float(res[0][0]) - want) / want))
    assert abs(float(res[0][0]) - want) <= 4 * 2.0 ** -24 * want
    assert res[0][1] == np.float32(5.0) / (res[0][0] + np.float32(1e-6))


def test_grad_norm_nonfinite_null_outputs_and_workspace(ops):
    sizes = R.TABLES['n25']
    grads = R.grad_norm_inputs(sizes, 5)
    norm, coef = R.grad_norm_expected(grads, 5.0)
    tb = Table(sizes, ('g',), dict(g=grads))
    t = tb.tensors('g')
    # one of the two outputs NULL: the other one is written, its neighbour is not
    rc, out, _ = _grad_norm(ops, t, sizes, 5.0, want_coef=False)
    assert rc == 0 and same_bits(out.get()[:1], np.array([norm])) and np.isnan(out.get()[1]) and out.slack_untouched()
    rc, out, _ = _grad_norm(ops, t, sizes, 5.0, want_norm=False)
    assert rc == 0 and same_bits(out.get()[1:], np.array([coef])) and np.isnan(out.get()[0]) and out.slack_untouched()
    rc, out, _ = _grad_norm(ops, t, sizes, 5.0, want_norm=False, want_coef=False)
    assert rc == EINVAL
    # a short or misaligned workspace
    for kw in (dict(ws_short=1), dict(ws_short=8), dict(ws_off=1)):
        rc, out, ws = _grad_norm(ops, t, sizes, 5.0, **kw)
        assert rc == EWORKSPACE, kw
        assert np.isnan(out.buf.cpu().numpy()).all() and np.isnan(ws.buf.cpu().numpy()).all()
    # NaN and +inf gradients (in the tensor beyond the block cap, past its first pass)
    big = sizes.index(R.BIG)
    for value, want in ((NAN, (NAN, NAN)), (float('inf'), (float('inf'), 0.0))):
        t[big][R.BIG - 7] = value
        rc, out, _ = _grad_norm(ops, t, sizes, 5.0)
        assert rc == 0 and same_bits(out.get(), np.array(want, np.float32)), (value, out.get())
    # count = 0: norm 0, coef max_norm / 1e-6f
    rc, out, _ = _grad_norm(ops, [], [], 5.0)
    assert rc == 0 and same_bits(out.get(), np.array([0.0, np.float32(5.0) / np.float32(1e-6)], np.float32))


@pytest.mark.parametrize("bad", ['numel', 'grad'])
def test_grad_norm_invalid_entry_launches_nothing(ops, bad):
    """30 entries, entry 27 invalid: ASRK_EINVAL with the outputs and the workspace untouched"""
    sizes = [40 + 3 * t for t in range(30)]
    tb = Table(sizes, ('g',), dict(g=R.grad_norm_inputs(sizes, 9)))
    t, n = tb.tensors('g'), list(sizes)
    ws = Guarded(2 * 31, off=4)
    if bad == 'numel':
        n[27] = -1
    else:
        t[27] = None
    L, st = ops._L(), ops._stream()
    out = Guarded(2, off=3)
    rc = L.asrk_grad_norm_multi_f32(30, _ptr_array(t), (ctypes.c_int64 * 30)(*n), 5.0, out.ptr(),
                                    ctypes.c_void_p(out.ptr().value + 4), ws.ptr(), 8 * 31, st)
    ops.check_errors()
    assert rc == EINVAL
    assert np.isnan(out.buf.cpu().numpy()).all() and np.isnan(ws.buf.cpu().numpy()).all()


# ====================================================================================================== fill
@pytest.mark.parametrize("n", R.FILL_SIZES)
def test_fill(ops, n):
    sent = 12345.5
    for value in R.FILL_VALUES:
        for off in (4, 1):
            g = Guarded(n, off=off, fill=sent)
            _lib().check(ops._L().asrk_fill_f32(g.ptr(), n, value, ops._stream()), "fill")
            ops.check_errors()
            assert same_bits(g.get(), np.full((n,), value, np.float32)), (n, value)       # -0.0 keeps its sign, NaN is NaN
            assert g.slack_untouched()
    g = Guarded(4, fill=sent)
    assert ops._L().asrk_fill_f32(g.ptr(), 0, 1.0, ops._stream()) == 0
    assert ops._L().asrk_fill_f32(g.ptr(), -1, 1.0, ops._stream()) == EINVAL
    ops.check_errors()
    assert same_bits(g.buf, np.full((13,), sent, np.float32))


# ====================================================================================================== ASRK_DETERMINISTIC
@pytest.fixture(scope="module")
def det_runs(tmp_path_factory):
    """one fresh process with ASRK_DETERMINISTIC=1 (the library reads it once)"""
    out = str(tmp_path_factory.mktemp("rowdet") / "det.npz")
    r = subprocess.run([sys.executable, os.path.join(HERE, "rowops_variants_worker.py"), out], capture_output=True, text=True,
                       env=dict(os.environ, ASRK_DETERMINISTIC="1"), timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    z = np.load(out)
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", R.COLSUM_DET_ROWS)
def test_colsum_deterministic(ops, det_runs, name):
    """one chunk / one block per column (asserted from the plan inside the worker): still exact, on all three kernels"""
    c = R.COLSUM_BY_NAME[name]
    assert int(det_runs['cs_variant_' + name]) == c.variant and int(det_runs['cs_chunks_' + name]) == 1
    for acc in (0, 1):
        assert same_bits(det_runs['cs_%d_%s' % (acc, name)], R.colsum_expected(name, acc)), (name, acc)


def test_colsum_deterministic_rows_cover_all_three_kernels():
    assert {R.COLSUM_BY_NAME[n].variant for n in R.COLSUM_DET_ROWS} == {0, 1, 2}


@pytest.mark.parametrize("name", R.LN_DET_ROWS)
def test_layer_norm_param_gradient_deterministic(ops, det_runs, name):
    c = R.LN_BY_NAME[name]
    assert int(det_runs['ln_chunks_' + name]) == 1 and bool(det_runs['ln_same_' + name])
    _ln_judge(name + "[det]", c, dict(dw=det_runs['ln_dw_' + name], db=det_runs['ln_db_' + name]), kinds=('dw', 'db'))
    if c.kind == 'int_dy':
        assert same_bits(det_runs['ln_db_' + name], R.ln_expected(name)['db'].astype(np.float32))
