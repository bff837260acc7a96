"""The case table, the inputs and the references of the exact-f32 GEMM dispatch (csrc/gemm.hip: asrk_gemm_f32).

A row names one launch (layout, extents, leading dimensions, pointer misalignment, alpha / beta, biases, splitk, flags,
knobs) and the plan record asrk_gemm_plan_info gives for it on a 256-CU device.  tests/test_gemm_plan_cpu.py holds every
row to its record and the table to the whole set of kernel variants; tests/test_gemm_variants_gpu.py runs every row.  A
re-tune that moves a row to another kernel fails the plan test: then move the SHAPE, not the assertion.

Two data sets per row, same launch arguments:
  exact : A, B integers in [-8, 8], C0 and the biases integers in [-64, 64], alpha in {1, 0.5, -2}, beta in {0, 1, 0.5, -2}:
          every product, partial sum and result is a multiple of 0.5 below 2^24 (K <= 2048: |sum| <= 131072), so the result
          does not depend on the summation order (atomics included) and must equal the int64 reference BIT FOR BIT;
  gauss : randn operands against float64, |C - ref| <= 2e-6 * (|alpha| |A| |B| + |beta C0| + |b1| + |b2| + 1) elementwise
          (the criterion of test_kernels_gpu.py::test_gemm_matches_fp64 extended to the whole epilogue).
Each operand is a view inside a larger NaN-filled buffer (leading-dimension padding, a row before and after, >= 64 floats
of margin on both sides): no clamped or zero-selected load may let an out-of-range value reach a stored element.  C sits
in a buffer filled with a known pattern (beta * C is read), with ldc >= N + 3, a guard row on both sides and 64 floats
of margin."""
import collections
import zlib

import numpy as np
import torch

NCU = 256
SK_NT, SK_NN, SPLIT, FAST, GENERIC = 0, 1, 2, 3, 4
PATH_NAMES = ("skinny_nt", "skinny_nn", "split", "fast", "generic")
PRE_NONE, PRE_MEMSET, PRE_SCALE = 0, 1, 2
ST_OVER, ST_RMW, ST_ADD, ST_ATOMIC = 0, 1, 2, 3
SPLIT_ALWAYS = 2
TRANS = {"NT": (0, 1), "NN": (0, 0), "TN": (1, 0)}
BOUND = 2e-6            # the elementwise criterion, relative to the scale above
SEQ32_BOUND = 1e-6      # sequential float32 accumulation on the CPU must stay below half of it on every row
MARGIN = 64


def lds_hint(kib):
    return (kib & 0xff) << 8


Plan = collections.namedtuple("Plan", "path a_kc b_kc vec splitk kps pre store")
Row = collections.namedtuple("Row", "name mode M N K lda ldb ldc offa offb alpha beta b1 b2 splitk flags knobs plan "
                                    "run twin lds")

ROWS = []


def _nat(mode, M, N, K):
    """natural (contiguous) leading dimensions of A and B as stored; at least 4 so that K = 0 keeps a valid, aligned ld"""
    lda = K if mode in ("NT", "NN") else M
    ldb = K if mode == "NT" else N
    return max(lda, 4) if lda == 0 else lda, max(ldb, 4) if ldb == 0 else ldb


def row(name, mode, M, N, K, plan, lda=None, ldb=None, ldc=None, offa=0, offb=0, alpha=1.0, beta=0.0, b1=False, b2=False,
        splitk=0, flags=0, knobs=(), run=True, twin=None, lds=None):
    la, lb = _nat(mode, M, N, K)
    if plan[0] in (FAST, GENERIC):          # the tiled kernels' pre-pass and store form follow from the row's beta
        plan = _tiled(mode, plan[0], plan[3], K, plan[4], plan[5], beta)
    r = Row(name, mode, M, N, K, la if lda is None else lda, lb if ldb is None else ldb, N + 3 if ldc is None else ldc,
            offa, offb, float(alpha), float(beta), b1, b2, splitk, flags, tuple(knobs), Plan(*plan), run, twin, lds)
    assert r.ldc >= N + 3 and r.offa in (0, 1) and r.offb in (0, 1)
    assert r.alpha in (1.0, 0.5, -2.0) and r.beta in (0.0, 1.0, 0.5, -2.0) and K <= 2048
    ROWS.append(r)
    return r


def _kc(mode):
    return (mode != "TN", mode == "NT")


def _tiled(mode, path, vec, K, splitk=1, kps=None, beta=0.0):
    """plan record of a tiled-kernel row: kps defaults to the whole K rounded up to k-tiles"""
    a, b = _kc(mode)
    kps = max(32, -(-K // 32) * 32) if kps is None else kps
    if splitk > 1:
        pre = PRE_MEMSET if beta == 0 else PRE_NONE if beta == 1 else PRE_SCALE
        return (path, a, b, vec, splitk, kps, pre, ST_ATOMIC)
    return (path, a, b, vec, 1, kps, PRE_NONE, ST_RMW if beta != 0 else ST_OVER)


NOFAST = (("ASRK_GEMM_NOFAST", "1"),)
NOSKINNY = (("ASRK_GEMM_NOSKINNY", "1"),)
NOSKINNY_NOFAST = (("ASRK_GEMM_NOFAST", "1"), ("ASRK_GEMM_NOSKINNY", "1"))
SK3 = (("ASRK_SKINNY_SK", "3"),)
DETERMINISTIC = (("ASRK_DETERMINISTIC", "1"),)
KNOB_SETS = [NOFAST, NOSKINNY, NOSKINNY_NOFAST, SK3, DETERMINISTIC]

# ---------------------------------------------------------------------------------------------- skinny NT
# (path, a_kc, b_kc, vec, K ranges, k per range, pre-pass, store form)
S = {}
S[1] = row("S1", "NT", 1, 1, 32, (SK_NT, 1, 1, 1, 1, 128, PRE_NONE, ST_OVER))
# two slabs, the second with one column; wave 0 has 32 k, wave 1 has 4, waves 2 and 3 are empty
S[2] = row("S2", "NT", 5, 33, 36, (SK_NT, 1, 1, 1, 1, 128, PRE_NONE, ST_OVER), lda=40, ldb=44, alpha=0.5, b1=True, b2=True)
S[3] = row("S3", "NT", 32, 31, 516, (SK_NT, 1, 1, 1, 2, 384, PRE_MEMSET, ST_ATOMIC), b1=True)      # ranges 384 + 132
S[4] = row("S4", "NT", 17, 64, 2048, (SK_NT, 1, 1, 1, 8, 256, PRE_SCALE, ST_ATOMIC), alpha=-2.0, beta=0.5, b2=True)
S[5] = row("S5", "NT", 32, 40, 160, (SK_NT, 1, 1, 1, 1, 256, PRE_NONE, ST_ADD), beta=1.0, b1=True, ldc=48)
S[6] = row("S6", "NT", 9, 32, 96, (SK_NT, 1, 1, 1, 1, 128, PRE_SCALE, ST_ADD), alpha=0.5, beta=-2.0)
# ---------------------------------------------------------------------------------------------- skinny NN
NN_ = {}
NN_[1] = row("N1", "NN", 1, 4, 32, (SK_NN, 1, 0, 1, 1, 64, PRE_NONE, ST_OVER))          # every lane clamped to column 0
# the second slab has 4 columns; the waves get 16 / 16 / 4 / 0 k
NN_[2] = row("N2", "NN", 7, 132, 36, (SK_NN, 1, 0, 1, 1, 64, PRE_NONE, ST_OVER), ldb=136, alpha=-2.0, b1=True, b2=True)
NN_[3] = row("N3", "NN", 32, 128, 260, (SK_NN, 1, 0, 1, 2, 192, PRE_MEMSET, ST_ATOMIC), b2=True)   # ranges 192 + 68
NN_[4] = row("N4", "NN", 20, 256, 1024, (SK_NN, 1, 0, 1, 8, 128, PRE_SCALE, ST_ATOMIC), alpha=0.5, beta=0.5, b1=True)
NN_[5] = row("N5", "NN", 12, 8, 64, (SK_NN, 1, 0, 1, 1, 64, PRE_NONE, ST_ADD), beta=1.0, lda=68, ldc=16)
NN_[6] = row("N6", "NN", 3, 36, 48, (SK_NN, 1, 0, 1, 1, 64, PRE_SCALE, ST_ADD), beta=-2.0, b1=True)
# --------------------------------------------------------------------------- routed away from the skinny kernels
row("R1", "NT", 33, 64, 64, _tiled("NT", FAST, 1, 64))                           # M = 33
row("R2", "NT", 8, 64, 28, _tiled("NT", FAST, 1, 28))                            # K < 32
row("R3", "NT", 8, 64, 34, _tiled("NT", GENERIC, 0, 34))                         # K % 4 != 0
row("R4", "NT", 8, 64, 64, _tiled("NT", GENERIC, 0, 64), lda=66)                 # lda % 4 != 0
row("R5", "NT", 8, 64, 64, _tiled("NT", GENERIC, 0, 64), offa=1)                 # A one float off 16-byte alignment
row("R6", "NT", 8, 64, 64, _tiled("NT", GENERIC, 0, 64), offb=1)
row("R7", "NN", 8, 6, 64, _tiled("NN", GENERIC, 0, 64))                          # NN with N % 4 != 0
row("R8", "TN", 8, 64, 64, _tiled("TN", FAST, 1, 64))                            # TN has no skinny kernel
row("R9", "NT", 8, 64, 64, _tiled("NT", FAST, 1, 64, 2, 32), splitk=2)           # the caller's split-K: tiled + atomics
row("R10", "NT", 8, 64, 64, (SK_NT, 1, 1, 1, 1, 128, PRE_NONE, ST_OVER), flags=SPLIT_ALWAYS, run=False)   # stays skinny
row("R11", "NT", 8, 64, 34, (SPLIT, 1, 1, 0, 1, 34, PRE_NONE, ST_OVER), flags=SPLIT_ALWAYS, run=False)    # the split path
# ---------------------------------------------------------------------------------------------- fast tiled
# TN reads both operands M/N-contiguous: 16-byte loads need M % 4 == 0, so its second row tile has 4 rows, not 2
F1_SHAPE = {"NT": (130, 132), "NN": (130, 132), "TN": (132, 132)}
F1_K = (4, 32, 36, 64, 68, 100, 128)     # nk = 1 tail | 1 | 2 tail | 2 | 3 tail (n_plain 0) | 4 tail (n_plain 1) | 4 (n_plain 2)
F1 = {}
for _m in ("NT", "NN", "TN"):
    for _i, _k in enumerate(F1_K):
        F1[_m, _k] = row("F1-%s-%d" % (_m, _k), _m, *F1_SHAPE[_m], _k, _tiled(_m, FAST, 1, _k),
                         alpha=(1.0, 0.5, -2.0)[_i % 3], beta=(0.0, 0.5, 1.0, -2.0)[_i % 4], b1=_i % 2 == 0, b2=_i % 3 == 0)
row("F2-TN-67", "TN", 132, 132, 67, _tiled("TN", FAST, 1, 67), b1=True)          # K % 4 != 0 on the fast kernel
row("F2-TN-33", "TN", 132, 132, 33, _tiled("TN", FAST, 1, 33), beta=0.5)
row("F3-TN", "TN", 4, 4, 4, _tiled("TN", FAST, 1, 4))                            # the smallest extents the fast kernel takes
row("F3-NN", "NN", 33, 4, 4, _tiled("NN", FAST, 1, 4), b1=True)
row("F3-NT", "NT", 33, 1, 4, _tiled("NT", FAST, 1, 4), beta=1.0)
F4_9 = {"NT": (258, 260), "NN": (258, 260), "TN": (260, 260)}
row("F4-NT-9", "NT", 258, 260, 32, _tiled("NT", FAST, 1, 32), ldc=269, b1=True)          # tile remap: 3 x 3 tiles
row("F4-NN-15", "NN", 260, 516, 36, _tiled("NN", FAST, 1, 36), ldc=523, beta=1.0)        # 3 x 5
row("F4-TN-17", "TN", 4, 2052, 36, _tiled("TN", FAST, 1, 36), ldc=2057, alpha=0.5)       # 1 x 17
row("F4-NT-1", "NT", 40, 44, 32, _tiled("NT", FAST, 1, 32), ldc=49)
row("F4-NN-8", "NN", 132, 500, 32, _tiled("NN", FAST, 1, 32), ldc=505, b2=True)          # 2 x 4
# split-K: the caller's (3 -> 64 + 36; 8 -> 4 ranges, the last with 4 k; 64 clamped to the 4 k-tiles) and the library's
F5_LIB = []
for _m in ("NT", "TN"):
    _mn = F1_SHAPE[_m]
    for _beta in (0.0, 1.0, 0.5):
        _t = "%s-b%g" % (_m, _beta)
        row("F5-%s-s3" % _t, _m, *_mn, 100, _tiled(_m, FAST, 1, 100, 2, 64, _beta), beta=_beta, splitk=3, b1=True)
        row("F5-%s-s8" % _t, _m, *_mn, 100, _tiled(_m, FAST, 1, 100, 4, 32, _beta), beta=_beta, splitk=8, alpha=0.5)
        row("F5-%s-s64" % _t, _m, *_mn, 100, _tiled(_m, FAST, 1, 100, 4, 32, _beta), beta=_beta, splitk=64, b2=True)
        F5_LIB.append(row("F5-%s-k512" % _t, _m, 128, 128, 512, _tiled(_m, FAST, 1, 512, 2, 256, _beta), beta=_beta,
                          alpha=-2.0))
        F5_LIB.append(row("F5-%s-k2048" % _t, _m, 128, 128, 2048, _tiled(_m, FAST, 1, 2048, 8, 256, _beta), beta=_beta,
                          b1=True))
# the launch hint: same kernel with more dynamic LDS; bit-identical to the hint-0 twin
for _m in ("NT", "NN", "TN"):
    _r = F1[_m, 100]
    for _kib, _lds in ((96, 96 * 1024), (200, 158 * 1024)):
        row("F6-%s-%d" % (_m, _kib), _m, _r.M, _r.N, 100, _r.plan, alpha=_r.alpha, beta=_r.beta, b1=_r.b1, b2=_r.b2,
            flags=lds_hint(_kib), twin=_r.name, lds=_lds)
# ---------------------------------------------------------------------------------------------- generic tiled
for _m in ("NT", "NN", "TN"):
    row("G1-%s-33" % _m, _m, 33, 17, 5, _tiled(_m, GENERIC, 0, 5), b1=True)
    _la, _lb = _nat(_m, 129, 130, 67)
    row("G1-%s-129" % _m, _m, 129, 130, 67, _tiled(_m, GENERIC, 0, 67, beta=0.5), lda=_la + 1 + _la % 2,
        ldb=_lb + 1 + _lb % 2, beta=0.5, alpha=-2.0, b2=True)                     # odd leading dimensions
    row("G1-%s-off" % _m, _m, 36, 40, 8, _tiled(_m, GENERIC, 0, 8), offa=int(_m != "TN"), offb=int(_m == "TN"))
    # split-K with a ragged last range on the generic kernel: 64 + 3
    row("G4-%s" % _m, _m, 129, 130, 67, _tiled(_m, GENERIC, 0, 67, 2, 64, 1.0), lda=_la + 1 + _la % 2,
        ldb=_lb + 1 + _lb % 2, beta=1.0, splitk=2, b1=True)
row("G2-TN-1", "TN", 132, 136, 1, _tiled("TN", GENERIC, 1, 1), b1=True)           # VEC = 1 by shape: TN with K < 4
row("G2-TN-3", "TN", 132, 136, 3, _tiled("TN", GENERIC, 1, 3), beta=-2.0)
# K = 0: C = beta * C0 + b1 + b2
row("G2-NT-0", "NT", 33, 36, 0, _tiled("NT", GENERIC, 1, 0, beta=0.5), beta=0.5, b1=True, b2=True)
row("G2-NN-0", "NN", 33, 36, 0, _tiled("NN", GENERIC, 1, 0), b1=True)
row("G2-TN-0", "TN", 36, 40, 0, _tiled("TN", GENERIC, 1, 0, beta=-2.0), beta=-2.0, b2=True)
# ---------------------------------------------------------------------------------------------- knob rows


def _variant(r, tag, knobs, plan):
    return row("%s@%s" % (r.name, tag), r.mode, r.M, r.N, r.K, plan, lda=r.lda, ldb=r.ldb, ldc=r.ldc, offa=r.offa,
               offb=r.offb, alpha=r.alpha, beta=r.beta, b1=r.b1, b2=r.b2, splitk=r.splitk, flags=r.flags, knobs=knobs)


for _m in ("NT", "NN", "TN"):      # generic VEC = 1 in all three layouts, with work to do
    for _k in (36, 100):
        _variant(F1[_m, _k], "nofast", NOFAST, _tiled(_m, GENERIC, 1, _k, beta=F1[_m, _k].beta))
    row("F4-%s-9@nofast" % _m, _m, *F4_9[_m], 32, _tiled(_m, GENERIC, 1, 32), ldc=269, b1=True, knobs=NOFAST)
for _r in (S[1], S[2], NN_[1], NN_[2]):     # the fast kernel at M = 1 and M = 5: rows clamped to M - 1
    _variant(_r, "noskinny", NOSKINNY, _tiled(_r.mode, FAST, 1, _r.K))
for _r in (S[2], NN_[2]):
    _variant(_r, "generic", NOSKINNY_NOFAST, _tiled(_r.mode, GENERIC, 1, _r.K))
# forced K split of the skinny kernels: the last range has 8 k (wave 0 takes them, the others none); beta = 1: atomics on
# top of C with no pre-pass
row("S7@sk3", "NT", 8, 64, 520, (SK_NT, 1, 1, 1, 3, 256, PRE_NONE, ST_ATOMIC), beta=1.0, b1=True, knobs=SK3)
row("N7@sk3", "NN", 8, 64, 392, (SK_NN, 1, 0, 1, 3, 192, PRE_NONE, ST_ATOMIC), beta=1.0, b2=True, knobs=SK3)
# one K range per output element, no atomics
_variant(S[3], "det", DETERMINISTIC, (SK_NT, 1, 1, 1, 1, 640, PRE_NONE, ST_OVER))
_variant(S[4], "det", DETERMINISTIC, (SK_NT, 1, 1, 1, 1, 2048, PRE_SCALE, ST_ADD))
_variant(NN_[3], "det", DETERMINISTIC, (SK_NN, 1, 0, 1, 1, 320, PRE_NONE, ST_OVER))
for _r in F5_LIB:
    _variant(_r, "det", DETERMINISTIC, _tiled(_r.mode, FAST, 1, _r.K, beta=_r.beta))

ROW_BY_NAME = {r.name: r for r in ROWS}
assert len(ROW_BY_NAME) == len(ROWS)
PLAIN_RUN_ROWS = [r for r in ROWS if r.run and not r.knobs]


def knob_rows(knobs):
    return [r for r in ROWS if r.knobs == tuple(knobs)]


def align_bits(r):
    return (1 if r.offa == 0 else 0) | (2 if r.offb == 0 else 0)


def k_ranges(r):
    """lengths of the K ranges of the row's plan"""
    p = r.plan
    return [min(r.K, (i + 1) * p.kps) - i * p.kps for i in range(p.splitk)]


def loop_form(n):
    """the form of the fast kernel's K loop over a range of n k's (gemm_f32_fast_kernel): nk tiles, a partial last one"""
    nk, tail = -(-n // 32), n % 32 != 0
    if nk <= 2:
        return "nk%d%s" % (nk, "+tail" if tail else "")
    if nk == 3 and tail:
        return "chk-first"                       # n_plain = 0: the CHK body runs first
    return "plain+chk" if tail else "plain"      # n_plain >= 1


LOOP_FORMS = {"nk1+tail", "nk1", "nk2+tail", "nk2", "chk-first", "plain+chk", "plain"}

# ------------------------------------------------------------------------------------------------- inputs


def _seed(r, kind):
    return zlib.crc32(("%s/%s" % (r.twin or r.name.split("@")[0], kind)).encode())


def _place(mat, ld, off):
    """mat [R, C] as a view with leading dimension ld inside a NaN-filled buffer -> (buffer, start): a row of ld floats
    before and after, >= 64 floats of margin; start is 16-byte aligned plus `off` floats"""
    R, C = mat.shape
    start = MARGIN + (-ld) % 4 + ld
    assert start % 4 == 0 and ld >= C
    buf = torch.full((start + (R + 1) * ld + MARGIN + 4,), float("nan"), dtype=torch.float32)
    start += off
    torch.as_strided(buf, (R, C), (ld, 1), start).copy_(mat)
    return buf, start


_inputs = {}


def make_inputs(r, kind):
    """-> dict: A [M, K], B [K, N], C0 [M, N], b1, b2 (float64, the logical operands), and the buffers the launch reads:
    Abuf / a_start, Bbuf / b_start (NaN around the operands), Cbuf / c_start (pattern everywhere).  Cached: treat as
    read-only."""
    key = (r.name, kind)
    if key in _inputs:
        return _inputs[key]
    g = torch.Generator().manual_seed(_seed(r, kind))
    M, N, K = r.M, r.N, r.K
    crows = M + 2
    if kind == "exact":
        A = torch.randint(-8, 9, (M, K), generator=g).double()
        B = torch.randint(-8, 9, (K, N), generator=g).double()
        Cfull = torch.randint(-64, 65, (MARGIN + crows * r.ldc + MARGIN,), generator=g).double()
        b1, b2 = (torch.randint(-64, 65, (N,), generator=g).double() for _ in range(2))
    else:
        assert kind == "gauss"
        A = torch.randn(M, K, generator=g).double()
        B = torch.randn(K, N, generator=g).double()
        Cfull = torch.randn(MARGIN + crows * r.ldc + MARGIN, generator=g).double()
        b1, b2 = (torch.randn(N, generator=g).double() for _ in range(2))
    A, B = A.float().double(), B.float().double()
    a_st = A.t() if r.mode == "TN" else A              # as stored
    b_st = B.t() if r.mode == "NT" else B
    Abuf, a_start = _place(a_st.float(), r.lda, r.offa)
    Bbuf, b_start = _place(b_st.float(), r.ldb, r.offb)
    Cbuf = Cfull.float()
    c_start = MARGIN + r.ldc
    C0 = torch.as_strided(Cbuf, (M, N), (r.ldc, 1), c_start).double()
    d = dict(A=A, B=B, C0=C0, b1=b1 if r.b1 else None, b2=b2 if r.b2 else None, Abuf=Abuf, a_start=a_start, Bbuf=Bbuf,
             b_start=b_start, Cbuf=Cbuf, c_start=c_start)
    _inputs[key] = d
    return d


# ------------------------------------------------------------------------------------------------- references
def _epilogue(r, d, prod):
    out = r.alpha * prod + r.beta * d["C0"]
    for b in (d["b1"], d["b2"]):
        if b is not None:
            out = out + b[None, :]
    return out


def reference(r, d):
    """float64: alpha * A B + beta * C0 + b1 + b2"""
    return _epilogue(r, d, d["A"] @ d["B"])


def reference_int64(r, d):
    """the exact data through int64 products; every term is a multiple of 0.5, exact in float64"""
    prod = (d["A"].long() @ d["B"].long()).double()
    return _epilogue(r, d, prod)


def scale(r, d):
    """|alpha| |A| |B| + |beta C0| + |b1| + |b2| + 1"""
    s = abs(r.alpha) * (d["A"].abs() @ d["B"].abs()) + (r.beta * d["C0"]).abs() + 1.0
    for b in (d["b1"], d["b2"]):
        if b is not None:
            s = s + b.abs()[None, :]
    return s


def reference_seq32(r, d):
    """the same result in float32 with SEQUENTIAL accumulation over k (the worst summation order a kernel could use)"""
    A, B = d["A"].float().numpy(), d["B"].float().numpy()
    acc = np.zeros((r.M, r.N), dtype=np.float32)
    for k in range(r.K):
        acc += A[:, k:k + 1] * B[k:k + 1, :]
    out = np.float32(r.alpha) * acc + np.float32(r.beta) * d["C0"].float().numpy()
    for b in (d["b1"], d["b2"]):
        if b is not None:
            out = out + b.float().numpy()[None, :]
    return torch.from_numpy(out.astype(np.float32))


def ratio(r, d, got, ref=None):
    """max over the elements of |got - ref| / (BOUND * scale): the criterion holds iff <= 1.  NaN -> inf"""
    ref = reference(r, d) if ref is None else ref
    q = ((got.double() - ref).abs() / (BOUND * scale(r, d)))
    if q.numel() == 0:
        return 0.0
    m = float(q.max())
    return m if m == m and not bool(torch.isnan(q).any()) else float("inf")


def to_f32_bits(x):
    """float64 reference -> the int32 bit patterns of its float32 value, -0 normalised to +0 (no kernel epilogue can give
    -0: every stored value is a sum with a +0 or non-zero addend)"""
    return (x.float() + 0.0).view(torch.int32)


def mutations(r, d):
    """wrong references a correct criterion must reject: one k dropped, one bias doubled, one column (row) shifted by one"""
    ref = reference(r, d)
    out = {}
    if r.K > 0:
        k = int(torch.argmax(d["A"].abs().sum(0) * d["B"].abs().sum(1)))
        out["drop_k"] = ref - r.alpha * d["A"][:, k:k + 1] * d["B"][k:k + 1, :]
    for name in ("b1", "b2"):
        if d[name] is not None:
            out["double_" + name] = ref + d[name][None, :]
    if r.N > 1:
        out["shift_col"] = torch.roll(ref, 1, dims=1)
    elif r.M > 1:
        out["shift_row"] = torch.roll(ref, 1, dims=0)
    return out
