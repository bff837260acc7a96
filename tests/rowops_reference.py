"""Case tables and float64 references of the streaming helpers: csrc/rowops.hip (copy3d, colsum), csrc/norm.hip (LayerNorm,
dropout) and csrc/optim.hip (Adadelta / Adam steps, gradient norm, fill).  Plain numpy / torch float64, no device.

Every row NAMES the kernel variant it is there for (`variant`, the code asrk_rowops_plan_info reports) and the parts of the
launch plan that make it interesting (`plan`): tests/test_rowops_plan_cpu.py asks the library for each row's plan without a
GPU, tests/test_rowops_variants_gpu.py asserts it again at the live pointers before it runs the row.
tests/test_rowops_reference_cpu.py holds the references to torch's own float64 ops and the rows to the conditions their
exact checks rest on.

Exact inputs: integers k / 8.  A sum of M of them with |k| <= KMAX is a multiple of 1/8 below M * KMAX / 8; as long as
M * KMAX < 2^24 every partial sum in ANY order is a float32, so the float32 result of any summation order is the float64 sum
bit for bit (`exactly_summable`)."""
import collections
import ctypes
import functools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import regularizer_oracle as PH          # noqa: E402  (the numpy Philox dropout)

FLOOR = 4 * 2.0 ** -24
KMAX = 64


def bound(e32, factor, floor=FLOOR):
    """`factor` times what torch's float32 CPU run of the operation is off by on the same inputs, never less than a few
    float32 roundings of the largest element (tests/loss_reference.py)"""
    return max(factor * e32, floor)


def rel_err(a, b):
    """tests/helpers.rel_err: max|a - b| / max|b|"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.size == 0:
        return 0.0
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-12))


def exact_ints(shape, seed, kmax=KMAX):
    """float32 k / 8 with integer |k| <= kmax"""
    g = np.random.RandomState(seed)
    return (g.randint(-kmax, kmax + 1, size=shape).astype(np.float64) / 8.0).astype(np.float32)


def exactly_summable(x, count, kmax=KMAX):
    """the condition of the module docstring for sums of `count` elements of x"""
    k = np.asarray(x, np.float64) * 8.0
    return bool(np.array_equal(k, np.rint(k)) and (np.abs(k).max() if k.size else 0) <= kmax and count * kmax < 2 ** 24)


# ====================================================================================================== launch plans
PLAN_LEN = 8
PLAN_FIELDS = ('variant', 'launches', 'gx', 'gy', 'per', 'chunks', 'items', 'zeroed')
OP_COPY3D, OP_COLSUM, OP_DROPOUT, OP_ADADELTA, OP_LN_PARAM = range(5)
COPY3D_VARIANTS = {0: 'copy3d_kernel<scalar,copy>', 1: 'copy3d_kernel<scalar,acc>', 2: 'copy3d_kernel<vec,copy>',
                   3: 'copy3d_kernel<vec,acc>', 4: 'copy3d_rows_kernel<copy>', 5: 'copy3d_rows_kernel<acc>'}
COLSUM_VARIANTS = {0: 'colsum_kernel', 1: 'colsum_vec_kernel', 2: 'colsum_narrow_kernel'}
SCALAR, VEC, NARROW = 0, 1, 2
G_SCALAR, G_VEC, ROWS = 0, 2, 4                       # copy3d, + 1 for accumulate
A16 = 0x7f0000001000                                  # a 16-byte aligned address that is never read


def plan_info(L, op, ptrs, args):
    """asrk_rowops_plan_info -> (rc, dict); ptrs are integers (addresses), args integers"""
    p = (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs)
    a = (ctypes.c_int64 * max(len(args), 1))(*args)
    out = (ctypes.c_int64 * PLAN_LEN)()
    rc = L.asrk_rowops_plan_info(op, p, a, out, PLAN_LEN)
    return rc, dict(zip(PLAN_FIELDS, out))


def plan(L, op, ptrs, args):
    rc, d = plan_info(L, op, ptrs, args)
    assert rc == 0, (op, ptrs, args, rc)
    return d


# ====================================================================================================== copy3d
# strides in floats; soff / doff: the view starts that many floats into a 16-byte aligned allocation
C3 = collections.namedtuple('C3', 'name n0 n1 n2 ss0 ss1 ds0 ds1 soff doff variant plan')


def _c3(name, n0, n1, n2, variant, src='gap', dst='gap', soff=0, doff=0, plan=None, bump=None):
    def strides(kind, g1, g0):
        if kind == 'gap':                             # positive wraps, gaps between rows and between planes; % 4 == 0
            s1 = (n2 + 3) // 4 * 4 + g1
            return n1 * s1 + g0, s1
        if kind == 'tight':
            return n1 * n2, n2
        if kind == 'transposed':                      # the [n1][n0][n2] layout: wrap s0 - n1 * s1 < 0
            return n2, n0 * n2
        raise ValueError(kind)
    ss0, ss1 = strides(src, 4, 8)
    ds0, ds1 = strides(dst, 8, 4)
    s = dict(ss0=ss0, ss1=ss1, ds0=ds0, ds1=ds1)
    if bump:
        s[bump] += 1
    return C3(name, n0, n1, n2, s['ss0'], s['ss1'], s['ds0'], s['ds1'], soff, doff, variant, plan or {})


VEC_BASE = dict(n0=3, n1=5, n2=256)                   # rows-kernel eligible; every broken condition lands on scalar
COPY3D_CASES = [
    # generic kernel: rows narrower than 64 float4
    _c3('g_vec_24', 5, 7, 24, G_VEC),
    _c3('g_scalar_23', 5, 7, 23, G_SCALAR),
    _c3('g_vec_transposed', 6, 5, 24, G_VEC, src='transposed', dst='tight'),
    # ... beyond the 4096-workgroup cap: the grid-stride loop's second pass
    _c3('g_scalar_loop', 41, 257, 100, G_SCALAR, src='tight', dst='gap', doff=1, plan=dict(gx=4096, items=41 * 257 * 100)),
    _c3('g_vec_loop', 165, 257, 100, G_VEC, src='tight', dst='gap', plan=dict(gx=4096, items=165 * 257 * 25)),
    # rows kernel: per_row 64 / 65 / 256 / 257, rpb 4 with row counts 15 (4+4+4+3), 6 (4+2), 9 (4+4+1)
    _c3('r_pr64_rows15', 3, 5, 256, ROWS, plan=dict(per=4, gx=1, gy=4)),
    _c3('r_pr65_rows15', 3, 5, 260, ROWS, plan=dict(per=4, gx=1, gy=4)),
    _c3('r_pr256_rows6', 2, 3, 1024, ROWS, plan=dict(per=4, gx=1, gy=2)),
    _c3('r_pr257_rows9', 3, 3, 1028, ROWS, plan=dict(per=4, gx=2, gy=3)),
    _c3('r_n1_is_1', 7, 1, 260, ROWS, plan=dict(per=4, gx=1, gy=2)),
    _c3('r_rows1', 1, 1, 256, ROWS, plan=dict(per=4, gx=1, gy=1)),
    # rpb 8: 16381 = 2047 * 8 + 5 rows (n1 = 1: the wrap is taken on every row); rpb 16: 32761 = 2047 * 16 + 9 rows
    _c3('r_rpb8', 16381, 1, 256, ROWS, src='tight', dst='gap', plan=dict(per=8, gx=1, gy=2048)),
    _c3('r_rpb16', 181, 181, 256, ROWS, src='gap', dst='tight', plan=dict(per=16, gx=1, gy=2048)),
    # the batch <-> time transpose at a wide feature axis: negative wrap on the source side, on the destination side
    _c3('r_src_transposed', 7, 5, 260, ROWS, src='transposed', dst='tight', plan=dict(per=4)),
    _c3('r_dst_transposed', 7, 5, 260, ROWS, src='tight', dst='transposed', plan=dict(per=4)),
    _c3('r_both_transposed_gap', 6, 3, 1028, ROWS, src='transposed', dst='gap', plan=dict(per=4, gx=2)),
    # the vec predicate, one condition broken at a time
    _c3('p_base', variant=ROWS, **VEC_BASE),
    _c3('p_src_plus4', variant=G_SCALAR, soff=1, **VEC_BASE),
    _c3('p_dst_plus4', variant=G_SCALAR, doff=1, **VEC_BASE),
    _c3('p_n2_255', 3, 5, 255, G_SCALAR),
    _c3('p_ss0', variant=G_SCALAR, bump='ss0', **VEC_BASE),
    _c3('p_ss1', variant=G_SCALAR, bump='ss1', **VEC_BASE),
    _c3('p_ds0', variant=G_SCALAR, bump='ds0', **VEC_BASE),
    _c3('p_ds1', variant=G_SCALAR, bump='ds1', **VEC_BASE),
]
COPY3D_BY_NAME = {c.name: c for c in COPY3D_CASES}
PREDICATE_ROWS = [c.name for c in COPY3D_CASES if c.name.startswith('p_') and c.name != 'p_base']
# plan only (more than 1 GiB of destination): rows / rpb would pass 65535 workgroups; 2^30 rows fall back to the generic kernel
COPY3D_PLAN_ONLY = [
    _c3('huge_rpb33', 2048, 1024, 256, ROWS, src='tight', dst='tight', plan=dict(per=33, gx=1, gy=63551)),
    _c3('huge_rows_2p30', 32768, 32768, 256, G_VEC, src='tight', dst='tight', plan=dict(gx=4096, gy=1)),
]
SLACK = 7


def copy3d_index(c):
    """-> (src index [n0,n1,n2], dst index, src floats, dst floats) into the allocations (offsets included)"""
    i0 = np.arange(c.n0, dtype=np.int64)[:, None, None]
    i1 = np.arange(c.n1, dtype=np.int64)[None, :, None]
    e = np.arange(c.n2, dtype=np.int64)[None, None, :]
    si = c.soff + i0 * c.ss0 + i1 * c.ss1 + e
    di = c.doff + i0 * c.ds0 + i1 * c.ds1 + e
    return si, di, int(si.max()) + 1 + SLACK, int(di.max()) + 1 + SLACK


@functools.lru_cache(maxsize=2)
def copy3d_buffers(name):
    """-> (src allocation, dst allocation before an accumulate call, si, di); float32.  src is exact k/8 everywhere (the
    gaps too: reading one would show in the sums), dst is NaN outside the addressed elements"""
    c = COPY3D_BY_NAME[name]
    si, di, ns, nd = copy3d_index(c)
    seed = sum(map(ord, name))
    src = exact_ints((ns,), seed)
    dst = np.full((nd,), np.nan, np.float32)
    dst[di.reshape(-1)] = exact_ints((di.size,), seed + 1)
    return src, dst, si, di


def copy3d_expected(name, accumulate):
    """the whole destination allocation after the call, float64 arithmetic rounded once to float32 (the kernel starts from
    all-NaN for a copy, from copy3d_buffers' dst for an accumulate)"""
    src, dst0, si, di = copy3d_buffers(name)
    out = dst0.astype(np.float64) if accumulate else np.full(dst0.shape, np.nan, np.float64)
    v = src.astype(np.float64)[si.reshape(-1)]
    out[di.reshape(-1)] = v + out[di.reshape(-1)] if accumulate else v
    return out.astype(np.float32)


# ====================================================================================================== colsum
# X is the [M, N] block at float offset `off` of a 16-byte aligned allocation with row pitch ldx
CS = collections.namedtuple('CS', 'name M N ldx off variant plan')
VEC_N, VEC_M = (4, 252, 256, 260), (1, 3, 4, 5, 31, 32, 33, 100, 4097)
NARROW_N, NARROW_M = (4, 8, 16, 32, 64, 128), (4096, 4099, 8191)
COLSUM_CASES = (
    [CS('s_n1', 33, 1, 1, 0, SCALAR, dict(gx=1, chunks=2)),
     CS('s_n63', 100, 63, 64, 0, SCALAR, dict(gx=1, chunks=4)),
     CS('s_n65', 37, 65, 65, 0, SCALAR, dict(gx=2, chunks=2)),
     CS('s_n517', 257, 517, 520, 0, SCALAR, dict(gx=9, chunks=9)),
     CS('s_misaligned', 33, 64, 64, 1, SCALAR, dict(gx=1)),
     CS('s_ldx66', 33, 64, 66, 0, SCALAR, dict(gx=1)),
     CS('s_tall', 4100, 64, 64, 3, SCALAR, dict(chunks=129))]
    + [CS('v_n%d_m%d' % (n, m), m, n, n + 8, 0, VEC, dict(gx=-(-n // 256))) for n in VEC_N for m in VEC_M]
    + [CS('n_n%d_m%d' % (n, m), m, n, n, 0, NARROW, dict(per=2048, gy=1)) for n in NARROW_N for m in NARROW_M]
    + [CS('v_m4095_n64', 4095, 64, 64, 0, VEC, {}),           # one row short of the narrow kernel
       CS('v_ldx_n_plus_4', 4096, 64, 68, 0, VEC, {}),        # not contiguous
       CS('v_n12', 4096, 12, 12, 0, VEC, {}),                 # 256 % 3 != 0
       CS('s_narrow_misaligned', 4096, 64, 64, 1, SCALAR, {})]
)
COLSUM_BY_NAME = {c.name: c for c in COLSUM_CASES}
COLSUM_DET_ROWS = ['s_n517', 's_tall', 'v_n260_m4097', 'v_n4_m100', 'n_n4_m8191', 'n_n128_m4099', 'n_n64_m4096']


@functools.lru_cache(maxsize=None)
def colsum_inputs(name):
    """-> (allocation [off + M * ldx + SLACK], out0 [N]) float32, exact k/8.  Column c carries the signature (c % 25) - 12
    on top of the noise, so two columns' sums differ by about M * (their signatures' difference) / 8: a sum that lands in
    another column shows.  The gaps of the allocation hold 1e30 (one of them in a sum shows)."""
    c = COLSUM_BY_NAME[name]
    g = np.random.RandomState(sum(map(ord, name)))
    k = g.randint(-40, 41, size=(c.M, c.N)) + (np.arange(c.N)[None, :] % 25 - 12)
    buf = np.full((c.off + c.M * c.ldx + SLACK,), 1e30, np.float32)
    view = buf[c.off:c.off + c.M * c.ldx].reshape(c.M, c.ldx)
    view[:, :c.N] = (k / 8.0).astype(np.float32)
    return buf, exact_ints((c.N,), 7 + c.N)


def colsum_matrix(name):
    c = COLSUM_BY_NAME[name]
    buf, _ = colsum_inputs(name)
    return buf[c.off:c.off + c.M * c.ldx].reshape(c.M, c.ldx)[:, :c.N]


def colsum_expected(name, accumulate):
    """float64 column sums (+ out0) as float32: exact, see exactly_summable"""
    s = colsum_matrix(name).astype(np.float64).sum(axis=0)
    if accumulate:
        s = s + colsum_inputs(name)[1].astype(np.float64)
    return s.astype(np.float32)


# ====================================================================================================== LayerNorm
LN = collections.namedtuple('LN', 'name rows D kind eps plan')
LN_D, LN_ROWS = (1, 2, 63, 64, 65, 129, 2050), (1, 3, 4, 5, 64, 65, 257)
LN_CASES = (
    # D = 1: dw and db are one-element tensors, so rel_err has no larger element to be measured against and a sum of five
    # normal deviates that cancels would be held to a fraction of its own ulp in whatever order; with integer dy the sum is
    # exact in every order and the row asserts equality instead
    # D = 2: xhat is +-sqrt(var / (var + eps)), and dx = rstd * (gw0 - gw1) / 2 * eps / (var + eps): with a variance of 9 that
    # is 1e-6 of the terms it is the difference of, and no float32 evaluation has three digits of it (torch's CPU run: 2e-2).
    # The row has a gradient to measure where the variance is comparable with eps: x = 0.5 + 0.004 * randn ('tight')
    [LN('d%d_r5' % d, 5, d, {1: 'int_dy', 2: 'tight'}.get(d, 'randn'), 1e-5, dict(chunks=1, per=8)) for d in LN_D]
    + [LN('d65_r%d' % r, r, 65, 'randn', 1e-5, {}) for r in LN_ROWS if r != 5]
    + [LN('d2050_r257', 257, 2050, 'randn', 1e-5, dict(chunks=5, per=52)),       # 4 chunks of 52 rows and one of 49
       LN('d129_r65', 65, 129, 'randn', 1e-5, dict(chunks=2, per=36)),           # 36 + 29 rows
       LN('mean1000', 65, 129, 'mean1000', 1e-5, {}),
       LN('const_row', 9, 65, 'const_row', 1e-5, {}),
       LN('eps0', 65, 64, 'randn', 0.0, {}),
       LN('eps0_d2', 5, 2, 'randn', 0.0, {}),
       LN('int_dy', 257, 65, 'int_dy', 1e-5, dict(chunks=5)),
       LN('int_dy_d2050', 5, 2050, 'int_dy', 1e-5, {})]
)
LN_BY_NAME = {c.name: c for c in LN_CASES}
LN_DET_ROWS = ['d2050_r257', 'd129_r65', 'int_dy', 'd65_r1']
LN_KINDS = ('y', 'mean', 'rstd', 'dx', 'dw', 'db')
LN_HARD = dict(y=1e-4, mean=1e-4, rstd=1e-4, dx=1e-3, dw=1e-3, db=1e-3)
CONST_ROW, CONST_VALUE = 4, 0.5


@functools.lru_cache(maxsize=None)
def ln_inputs(name):
    """-> x [rows,D], w [D], b [D], dy [rows,D] float32 torch"""
    c = LN_BY_NAME[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    x = torch.randn(c.rows, c.D, generator=g) * 3 + 0.5
    if c.kind == 'mean1000':
        x = torch.randn(c.rows, c.D, generator=g) + 1000.0
    if c.kind == 'tight':
        x = torch.randn(c.rows, c.D, generator=g) * 0.004 + 0.5
    if c.kind == 'const_row':
        x[CONST_ROW] = CONST_VALUE                    # D * 0.5 and its mean are exact: variance exactly 0
    w = torch.randn(c.D, generator=g) * 0.5 + 1.0
    b = torch.randn(c.D, generator=g)
    dy = torch.randn(c.rows, c.D, generator=g)
    if c.kind == 'int_dy':
        dy = torch.from_numpy(exact_ints((c.rows, c.D), c.rows + c.D))
    return x, w, b, dy


def ln_eps(c):
    return float(np.float32(c.eps))                   # the ABI takes a float


def layer_norm_reference(x, w, b, dy, eps):
    """the definition, written out in float64 (numpy in, dict of numpy out)"""
    x, w, b, dy = (np.asarray(a, np.float64) for a in (x, w, b, dy))
    D = x.shape[1]
    mean = x.sum(axis=1) / D
    xc = x - mean[:, None]
    var = (xc * xc).sum(axis=1) / D                    # biased
    rstd = 1.0 / np.sqrt(var + eps)
    xh = xc * rstd[:, None]
    y = xh * w[None, :] + b[None, :]
    gw = dy * w[None, :]
    s1 = gw.sum(axis=1) / D
    s2 = (gw * xh).sum(axis=1) / D
    dx = rstd[:, None] * (gw - s1[:, None] - xh * s2[:, None])
    return dict(y=y, mean=mean, rstd=rstd, dx=dx, dw=(dy * xh).sum(axis=0), db=dy.sum(axis=0))


@functools.lru_cache(maxsize=None)
def ln_expected(name):
    c = LN_BY_NAME[name]
    x, w, b, dy = ln_inputs(name)
    return layer_norm_reference(x.numpy(), w.numpy(), b.numpy(), dy.numpy(), ln_eps(c))


def ln_torch(name, dtype):
    """torch's own CPU layer_norm (native_layer_norm: y, mean, rstd) and its autograd, in `dtype` -> dict of numpy"""
    c = LN_BY_NAME[name]
    x, w, b, dy = (t.clone().to(dtype) for t in ln_inputs(name))
    x.requires_grad_(True); w.requires_grad_(True); b.requires_grad_(True)
    y, mean, rstd = torch.native_layer_norm(x, [c.D], w, b, ln_eps(c))
    dx, dw, db = torch.autograd.grad(y, (x, w, b), dy)
    return {k: v.detach().reshape(-1 if k in ('mean', 'rstd') else v.shape).numpy()
            for k, v in dict(y=y, mean=mean, rstd=rstd, dx=dx, dw=dw, db=db).items()}


@functools.lru_cache(maxsize=None)
def ln_e32(name):
    ref, t32 = ln_expected(name), ln_torch(name, torch.float32)
    return {k: rel_err(t32[k], ref[k]) for k in LN_KINDS}


# ====================================================================================================== dropout
DROP_LOOP = 4 * 8192 * 256                            # elements one pass of the capped grid covers
DROP_SIZES = [('vec_loop', DROP_LOOP + 1200, 1), ('scalar_loop', DROP_LOOP + 1203, 0), ('vec_small', 260, 1),
              ('scalar_small', 259, 0), ('one', 1, 0)]
DROP_P = [('thresh0', 1e-9), ('half', 0.5), ('almost_one', 1.0 - 2.0 ** -24), ('p03', 0.3)]
DROP_OFFSETS = [0, 1, 12345, 2 ** 32, 2 ** 32 + 5, 2 ** 63 + 11]


def dropout_input(n, seed=3):
    """exact k/8 without zeros: a dropped element differs from every kept one"""
    x = exact_ints((n,), seed)
    x[x == 0] = 0.125
    return x


def dropout_expected(x, p, seed, offset=0):
    return PH.dropout(x, p, seed, offset)


# ====================================================================================================== optimisers
ADADELTA_HP = dict(lr=1.0, rho=0.95, eps=1e-8)
ADAM_HP = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
OPT_STEPS = 6
OPT_COEFS = [('below', 0.37), ('above', 2.5), ('none', None), ('nan', float('nan'))]
OPT_LOOP = 4096 * 256 * 4                             # one pass of the 16-byte Adadelta kernel's capped grid
# (name, n, state misaligned by one float): vector / scalar by n % 4 / scalar by alignment, and the grid-stride loops
OPT_SINGLE = [('vec', 1028, 0), ('odd', 1027, 0), ('misaligned', 1028, 1), ('vec_loop', OPT_LOOP + 2052, 0),
              ('odd_loop', OPT_LOOP + 2053, 0)]


def opt_inputs(n, seed, steps=OPT_STEPS):
    """-> p0 [n], grads [steps, n] float32 numpy"""
    g = np.random.RandomState(seed)
    p0 = g.standard_normal(n).astype(np.float32)
    grads = (g.standard_normal((steps, n)) * np.exp(g.uniform(-3, 1, size=(steps, 1)))).astype(np.float32)
    return p0, grads


def clip_of(coef):
    """-> (skip, c): the NaN rule and min(coef, 1) of csrc/optim.hip; coef a float32 value or None"""
    if coef is None:
        return False, 1.0
    coef = float(np.float32(coef))
    if coef != coef:
        return True, 1.0
    return False, min(coef, 1.0)


def adadelta_reference(p0, grads, coef, lr, rho, eps, dtype=np.float64):
    """-> list over steps of (p, square_avg, acc_delta); hyper-parameters as the ABI rounds them when dtype is float32"""
    f = dtype
    p, sq, acc = np.asarray(p0, f).copy(), np.zeros(len(p0), f), np.zeros(len(p0), f)
    skip, c = clip_of(coef)
    lr_, rho_, omr, eps_, c = f(lr), f(rho), f(1.0 - rho), f(eps), f(c)
    out = []
    for g in grads:
        if not skip:
            gr = np.asarray(g, f) * c
            sq = sq * rho_ + omr * gr * gr
            delta = np.sqrt(acc + eps_) / np.sqrt(sq + eps_) * gr
            acc = acc * rho_ + omr * delta * delta
            p = p - lr_ * delta
        out.append((p.copy(), sq.copy(), acc.copy()))
    return out


def adam_reference(p0, grads, coef, lr, beta1, beta2, eps, dtype=np.float64):
    """-> list over steps of (p, exp_avg, exp_avg_sq); the step count advances on a skipped step too (the caller of the
    ABI passes it)"""
    f = dtype
    p, m, v = np.asarray(p0, f).copy(), np.zeros(len(p0), f), np.zeros(len(p0), f)
    skip, c = clip_of(coef)
    c = f(c)
    out = []
    for t, g in enumerate(grads, 1):
        if not skip:
            bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
            gr = np.asarray(g, f) * c
            m = m + (gr - m) * f(1.0 - beta1)
            v = v * f(beta2) + f(1.0 - beta2) * gr * gr
            p = p - f(lr / bc1) * (m / (np.sqrt(v) / f(np.sqrt(bc2)) + f(eps)))
        out.append((p.copy(), m.copy(), v.copy()))
    return out


def torch_optim_run(kind, p0, grads, coef, dtype):
    """torch.optim.Adadelta / Adam on the CPU in `dtype`, the gradient scaled by min(coef, 1) first and the step skipped
    for a NaN coefficient (clip_grad_norm_ and the guard of the training loop) -> list of (p, state0, state1) numpy"""
    p = torch.nn.Parameter(torch.from_numpy(np.asarray(p0)).to(dtype).clone())
    if kind == 'adadelta':
        opt = torch.optim.Adadelta([p], **ADADELTA_HP)
        keys = ('square_avg', 'acc_delta')
    else:
        opt = torch.optim.Adam([p], lr=ADAM_HP['lr'], betas=(ADAM_HP['beta1'], ADAM_HP['beta2']), eps=ADAM_HP['eps'])
        keys = ('exp_avg', 'exp_avg_sq')
    skip, c = clip_of(coef)
    assert not skip
    out = []
    for g in grads:
        p.grad = torch.from_numpy(np.asarray(g)).to(dtype) * c
        opt.step()
        st = opt.state[p]
        out.append((p.detach().numpy().copy(), st[keys[0]].numpy().copy(), st[keys[1]].numpy().copy()))
    return out


OPT_KINDS = ('param', 'state0', 'state1')
OPT_HARD = 2e-6                                        # tests/test_kernels_gpu.py, against torch float32


@functools.lru_cache(maxsize=None)
def opt_e32(kind, n, seed, coef, steps=OPT_STEPS):
    """per tensor kind: the largest rel_err over the steps of torch.optim's float32 CPU run against its float64 run"""
    p0, grads = opt_inputs(n, seed, steps)
    r32, r64 = torch_optim_run(kind, p0, grads, coef, torch.float32), torch_optim_run(kind, p0, grads, coef, torch.float64)
    return tuple(max(rel_err(a[i], b[i]) for a, b in zip(r32, r64)) for i in range(3))


# ---- tables of the multi-tensor form and of the gradient norm: 24 slots per launch, empty tensors take none
MT_MAX = 24
STEP_CAP, NORM_CAP = 2048 * 1024, 2048 * 1024          # elements at which a tensor reaches its block cap (2048 / 1024 blocks)
BIG = STEP_CAP + 1500                                  # one tensor beyond both caps


def table_sizes(count, empties=(), big=None):
    """element counts of `count` tensors: odd sizes, one of 1 element, empty at `empties`, tensor `big` beyond the caps"""
    n = [1 + (37 * t) % 301 + (1024 if t % 7 == 3 else 0) for t in range(count)]
    n[1] = 1
    for t in empties:
        n[t] = 0
    if big is not None:
        n[big] = BIG
    return n


# 23 / 24 / 25 / 49 tensors without and with empty ones (at 0, 23, 24 and last where they exist); gap_at_edge26: the 24 slots are
# full at entry 23 and entry 24, the first of the next launch, is empty; tail_empty26: only empty entries follow a full launch
TABLES = collections.OrderedDict(
    [('n%d' % c, table_sizes(c, big=12 if c == 25 else None)) for c in (23, 24, 25, 49)]
    + [('e%d' % c, table_sizes(c, [t for t in (0, 23, 24, c - 1) if t < c], big=30 if c == 49 else None))
       for c in (23, 24, 25, 49)]
    + [('gap_at_edge26', table_sizes(26, [24])), ('tail_empty26', table_sizes(26, [24, 25]))])


def norm_blocks_of(n):
    return max(1, min(-(-n // 2048), 1024))


def norm_thread_elems(n):
    """the most elements one thread of sqnorm_partial_kernel adds in float32"""
    return -(-n // (norm_blocks_of(n) * 256))


def grad_norm_inputs(sizes, seed):
    return [exact_ints((n,), seed + t) for t, n in enumerate(sizes)]


def grad_norm_exact(grads):
    """-> (sum of squares as an exact python int in units of 1/64, float64 sum)"""
    units = sum(int((np.rint(g.astype(np.float64) * 8.0).astype(np.int64) ** 2).sum()) for g in grads)
    return units, units / 64.0


def grad_norm_expected(grads, max_norm):
    """-> (norm, coef) float32: float(sqrt(exact sum)) and max_norm / (norm + 1e-6f) in float32"""
    _, s = grad_norm_exact(grads)
    norm = np.float32(np.sqrt(np.float64(s)))
    with np.errstate(divide='ignore', invalid='ignore'):
        coef = np.float32(max_norm) / (norm + np.float32(1e-6))
    return norm, np.float32(coef)


def grad_norm_float64(grads):
    return float(np.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in grads)))


FILL_SIZES = (1, 255, 256, 257, 4096 * 256 + 259)
FILL_VALUES = (0.0, -0.0, float('nan'), 1.5)
