"""CPU: every row of tests/rowops_reference.py gets the kernel variant it names - asked of the library itself through
asrk_rowops_plan_info, which reads the plan functions of csrc/rowops_plan.h that asrk_copy3d_f32, asrk_colsum_f32,
asrk_dropout_f32, asrk_adadelta_step_f32 and the LayerNorm parameter gradient launch from (host only) - and the tables as a
whole reach every instantiation and both sides of every threshold of the dispatch.  A change of the dispatch that takes a
row off its kernel fails here: then move the SHAPE, not the assertion.

The two copy3d branches that need more than 1 GiB of destination (rows per workgroup = ceil(rows / 65535), and the
fallback to the generic kernel from 2^30 rows on) are held here and nowhere else."""
import ctypes
import importlib
import os
import subprocess
import sys

import pytest

from conftest import PKG_NAME
import rowops_reference as R

MOVE = "the dispatch moved this row to another kernel: move the shape, not the assertion"
EINVAL = -1
A = R.A16
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def L():
    importlib.import_module(PKG_NAME + ".build").build(verbose=False)
    return importlib.import_module(PKG_NAME + "._lib").load()


def cdiv(a, b):
    return -(-a // b)


def copy3d_plan(L, c, acc, src=A, dst=A):
    return R.plan(L, R.OP_COPY3D, [src + 4 * c.soff, dst + 4 * c.doff],
                  [c.n0, c.n1, c.n2, c.ss0, c.ss1, c.ds0, c.ds1, acc])


def expected_copy3d(c, acc):
    """the dispatch as include/asrk.h and the comments of csrc/rowops_plan.h document it"""
    vec = c.soff % 4 == 0 and c.doff % 4 == 0 and all(v % 4 == 0 for v in (c.n2, c.ss0, c.ss1, c.ds0, c.ds1))
    rows = c.n0 * c.n1
    if vec and c.n2 // 4 >= 64 and rows < 2 ** 30:
        gx, rpb = cdiv(c.n2 // 4, 256), 16
        while rpb > 4 and gx * cdiv(rows, rpb) < 2048:
            rpb //= 2
        if cdiv(rows, rpb) > 65535:
            rpb = cdiv(rows, 65535)
        return dict(variant=4 + acc, launches=1, gx=gx, gy=cdiv(rows, rpb), per=rpb)
    total = rows * (c.n2 // 4 if vec else c.n2)
    return dict(variant=(2 if vec else 0) + acc, launches=1, gx=max(1, min(cdiv(total, 256), 4096)), gy=1, per=0, items=total)


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("case", R.COPY3D_CASES + R.COPY3D_PLAN_ONLY, ids=lambda c: c.name)
def test_copy3d_row_gets_the_kernel_it_names(L, case, acc):
    c = case
    got = copy3d_plan(L, c, acc)
    assert got['variant'] == c.variant + acc, "%s: %s, the row is there for %s - %s" % (
        c.name, R.COPY3D_VARIANTS[got['variant']], R.COPY3D_VARIANTS[c.variant + acc], MOVE)
    for field, v in c.plan.items():
        assert got[field] == v, "%s: %s is %d, the row is there for %d - %s" % (c.name, field, got[field], v, MOVE)
    for field, v in expected_copy3d(c, acc).items():
        assert got[field] == v, (c.name, field, got[field], v)
    if got['variant'] >= 4:                                          # the grid covers every row and every 16-byte piece
        rows, per_row = c.n0 * c.n1, c.n2 // 4
        assert got['gy'] <= 65535 and (got['gy'] - 1) * got['per'] < rows <= got['gy'] * got['per']
        assert (got['gx'] - 1) * 256 < per_row <= got['gx'] * 256


def test_copy3d_table_reaches_every_instantiation_and_threshold(L):
    by = R.COPY3D_BY_NAME
    assert {c.variant + a for c in R.COPY3D_CASES for a in (0, 1)} == set(range(6)), MOVE
    rows_cases = [c for c in R.COPY3D_CASES if c.variant == R.ROWS]
    assert {copy3d_plan(L, c, 0)['per'] for c in rows_cases} == {4, 8, 16}
    assert {c.n2 // 4 for c in rows_cases} >= {64, 65, 256, 257}
    assert by['g_vec_24'].n2 // 4 < 64 <= by['r_pr64_rows15'].n2 // 4              # the width threshold, both sides
    assert any(c.n1 == 1 for c in rows_cases)
    def last_group(c):                                               # rows in the last 4-row group of the last workgroup
        p = copy3d_plan(L, c, 0)
        return (c.n0 * c.n1 - (p['gy'] - 1) * p['per']) % 4
    assert {last_group(c) for c in rows_cases} >= {1, 2, 3}
    assert any(c.n0 * c.n1 % copy3d_plan(L, c, 0)['per'] for c in rows_cases if copy3d_plan(L, c, 0)['per'] > 4)
    wraps_s = {(c.ss0 - c.n1 * c.ss1 > 0) - (c.ss0 - c.n1 * c.ss1 < 0) for c in rows_cases}
    wraps_d = {(c.ds0 - c.n1 * c.ds1 > 0) - (c.ds0 - c.n1 * c.ds1 < 0) for c in rows_cases}
    assert wraps_s >= {-1, 1} and wraps_d >= {-1, 1}
    for name in ('g_scalar_loop', 'g_vec_loop'):                      # the grid-stride loop's second pass is short
        p = copy3d_plan(L, by[name], 0)
        assert p['gx'] == 4096 and 4096 * 256 < p['items'] < 4096 * 256 + 16384, (name, p)
    # the vec predicate: every row of PREDICATE_ROWS differs from p_base in exactly one of its seven conditions
    base = by['p_base']
    conds = lambda c: (c.soff % 4 == 0, c.doff % 4 == 0, c.n2 % 4 == 0, c.ss0 % 4 == 0, c.ss1 % 4 == 0, c.ds0 % 4 == 0,
                       c.ds1 % 4 == 0)
    assert all(conds(base))
    broken = [tuple(i for i, ok in enumerate(conds(by[n])) if not ok) for n in R.PREDICATE_ROWS]
    assert sorted(broken) == [(i,) for i in range(7)], broken
    # ... and the destination of the two plan-only rows is out of reach of a test: more than 1 GiB
    for c in R.COPY3D_PLAN_ONLY:
        assert c.n0 * c.n1 * c.n2 * 4 > 2 ** 30


def test_copy3d_plan_alignment_is_the_pointers_own(L):
    c = R.COPY3D_BY_NAME['p_base']
    for src, dst, variant in ((A, A, 4), (A + 4, A, 0), (A, A + 8, 0), (A + 12, A + 12, 0), (A + 16, A + 32, 4)):
        assert copy3d_plan(L, c, 0, src, dst)['variant'] == variant


def colsum_plan(L, c, acc=0, base=A):
    return R.plan(L, R.OP_COLSUM, [base + 4 * c.off, A], [c.M, c.N, c.ldx, acc])


def expected_colsum(M, N, ldx, off, det=False):
    vec = off % 4 == 0 and N % 4 == 0 and ldx % 4 == 0
    if vec and ldx == N and N <= 128 and 256 % (N // 4) == 0 and M >= 4096:
        total4 = M * (N // 4)
        per = cdiv(cdiv(total4, 1 if det else 512), 2048) * 2048
        return dict(variant=2, launches=1, gx=cdiv(total4, per), gy=1, per=per, chunks=cdiv(total4, per), items=total4)
    gx = cdiv(N, 256 if vec else 64)
    chunks = min(cdiv(2048 if vec else 1024, gx), cdiv(M, 32))
    if chunks < 1 or det:
        chunks = 1
    rpc = cdiv(M, chunks)
    return dict(variant=int(vec), launches=1, gx=gx, gy=cdiv(M, rpc), per=rpc, chunks=cdiv(M, rpc))


@pytest.mark.parametrize("case", R.COLSUM_CASES, ids=lambda c: c.name)
def test_colsum_row_gets_the_kernel_it_names(L, case):
    c = case
    for acc in (0, 1):
        got = colsum_plan(L, c, acc)
        assert got['variant'] == c.variant, "%s: %s, the row is there for %s - %s" % (
            c.name, R.COLSUM_VARIANTS[got['variant']], R.COLSUM_VARIANTS[c.variant], MOVE)
        for field, v in c.plan.items():
            assert got[field] == v, "%s: %s is %d, the row is there for %d - %s" % (c.name, field, got[field], v, MOVE)
        for field, v in expected_colsum(c.M, c.N, c.ldx, c.off).items():
            assert got[field] == v, (c.name, field, got[field], v)
        assert got['zeroed'] == 1 - acc
        assert (got['chunks'] - 1) * got['per'] < (got['items'] if c.variant == 2 else c.M) <= got['chunks'] * got['per']


def test_colsum_table_reaches_every_kernel_and_threshold(L):
    by = R.COLSUM_BY_NAME
    assert {c.variant for c in R.COLSUM_CASES} == {0, 1, 2}, MOVE
    narrow = [c for c in R.COLSUM_CASES if c.variant == R.NARROW]
    assert {c.N for c in narrow} == {4, 8, 16, 32, 64, 128} and min(c.M for c in narrow) == 4096
    # two or more blocks with a ragged last one, for every N; a last block shorter than one pass of 256 pieces
    for n in R.NARROW_N:
        ragged = [c for c in narrow if c.N == n and colsum_plan(L, c)['chunks'] >= 2
                  and colsum_plan(L, c)['items'] % colsum_plan(L, c)['per']]
        assert ragged, n
    assert by['v_m4095_n64'].M == 4095 and by['v_ldx_n_plus_4'].ldx == by['v_ldx_n_plus_4'].N + 4
    vec = [c for c in R.COLSUM_CASES if c.variant == R.VEC]
    # the 16-row unrolled loop (r + 12 < r1 for a wave's first row), its 4-row tail, one and several chunks
    per = {c.name: colsum_plan(L, c) for c in vec}
    assert any(p['chunks'] == 1 and p['per'] < 13 for p in per.values())          # tail only
    assert any(p['per'] >= 16 and p['per'] % 16 for p in per.values())            # unrolled loop, then the tail
    assert any(p['chunks'] > 1 and by[n].M % p['per'] for n, p in per.items())    # several chunks, the last one short
    scalar = [c for c in R.COLSUM_CASES if c.variant == R.SCALAR]
    assert {c.N for c in scalar} >= {1, 63, 65, 517}
    assert any(c.off % 4 and c.N % 4 == 0 and c.ldx % 4 == 0 for c in scalar)     # scalar by the base alone
    assert any(c.off == 0 and c.N % 4 == 0 and c.ldx % 4 for c in scalar)         # scalar by ldx alone
    assert all(c.M <= 8192 for c in R.COLSUM_CASES)


def test_colsum_plan_sweep_against_the_documented_arithmetic(L):
    for M in (1, 31, 32, 33, 100, 4095, 4096, 4097, 70000, 524288):
        for N, ldx in ((1, 1), (4, 4), (4, 8), (12, 12), (64, 64), (64, 68), (128, 128), (132, 132), (256, 256), (517, 520),
                       (2048, 2048), (100000, 100000)):
            for off in (0, 1):
                got = R.plan(L, R.OP_COLSUM, [A + 4 * off, A], [M, N, ldx, 0])
                for field, v in expected_colsum(M, N, ldx, off).items():
                    assert got[field] == v, (M, N, ldx, off, field, got[field], v)


def test_dropout_and_adadelta_plans(L):
    for name, n, variant in R.DROP_SIZES:
        got = R.plan(L, R.OP_DROPOUT, [A, A], [n])
        assert got['variant'] == variant and got['items'] == cdiv(n, 4), (name, got, MOVE)
        assert got['gx'] == min(8192, cdiv(cdiv(n, 4), 256))
        if 'loop' in name:                                           # the grid-stride loop's second pass, a short one
            assert got['gx'] == 8192 and 8192 * 256 < got['items'] < 8192 * 256 + 512
    assert R.plan(L, R.OP_DROPOUT, [A + 4, A], [260])['variant'] == 0
    assert R.plan(L, R.OP_DROPOUT, [A, A + 4], [260])['variant'] == 0
    for name, n, mis in R.OPT_SINGLE:
        got = R.plan(L, R.OP_ADADELTA, [A, A, A + 4 * mis, A], [n])
        vec = int(n % 4 == 0 and not mis)
        assert got['variant'] == vec and got['items'] == (n // 4 if vec else n), (name, got, MOVE)
        assert got['gx'] == max(1, min(cdiv(got['items'], 256), 4096))
        assert ('loop' in name) == (got['items'] > 4096 * 256), (name, got)
    assert {R.plan(L, R.OP_ADADELTA, [A, A, A + 4 * m, A], [n])['variant'] for _, n, m in R.OPT_SINGLE} == {0, 1}
    for k in range(4):                                               # each of the four pointers decides
        ptrs = [A] * 4
        ptrs[k] += 4
        assert R.plan(L, R.OP_ADADELTA, ptrs, [1028])['variant'] == 0


@pytest.mark.parametrize("case", R.LN_CASES, ids=lambda c: c.name)
def test_layer_norm_param_plan(L, case):
    c = case
    got = R.plan(L, R.OP_LN_PARAM, [], [c.rows, c.D])
    for field, v in c.plan.items():
        assert got[field] == v, "%s: %s is %d, the row is there for %d - %s" % (c.name, field, got[field], v, MOVE)
    chunks = max(1, min(cdiv(c.rows, 64), 256))
    rpc = cdiv(cdiv(c.rows, chunks), 4) * 4
    assert (got['gx'], got['gy'], got['per'], got['chunks']) == (cdiv(c.D, 64), cdiv(c.rows, rpc), rpc, cdiv(c.rows, rpc))


def test_layer_norm_table_reaches_the_chunk_edges(L):
    plans = {c.name: R.plan(L, R.OP_LN_PARAM, [], [c.rows, c.D]) for c in R.LN_CASES}
    assert any(p['chunks'] == 1 for p in plans.values()) and any(p['chunks'] > 2 for p in plans.values())
    assert any(p['chunks'] > 1 and R.LN_BY_NAME[n].rows % p['per'] for n, p in plans.items())     # a partial last chunk
    assert {c.D for c in R.LN_CASES} >= set(R.LN_D) and {c.rows for c in R.LN_CASES} >= set(R.LN_ROWS)


def test_deterministic_knob_plans_one_chunk():
    """ASRK_DETERMINISTIC is read once by the library, so a fresh process asks: every deterministic row of both tables gets
    ONE chunk (colsum: one row chunk or one block of the narrow stream; LayerNorm: one row chunk) on the kernel it names"""
    code = ("import sys, importlib; sys.path[:0] = [%r, %r]; import rowops_reference as R\n"
            "L = importlib.import_module(%r + '._lib').load()\n"
            "for n in R.COLSUM_DET_ROWS:\n"
            "    c = R.COLSUM_BY_NAME[n]; p = R.plan(L, R.OP_COLSUM, [R.A16 + 4 * c.off, R.A16], [c.M, c.N, c.ldx, 0])\n"
            "    assert p['variant'] == c.variant and p['chunks'] == 1 and p['gy'] == 1, (n, p)\n"
            "    assert c.variant != R.NARROW or (p['gx'] == 1 and p['per'] >= p['items'] and p['per'] %% 2048 == 0), (n, p)\n"
            "    assert c.variant == R.NARROW or p['per'] == c.M, (n, p)\n"
            "for n in R.LN_DET_ROWS:\n"
            "    c = R.LN_BY_NAME[n]; p = R.plan(L, R.OP_LN_PARAM, [], [c.rows, c.D])\n"
            "    assert p['chunks'] == 1 and p['gy'] == 1 and p['per'] >= c.rows and p['per'] %% 4 == 0, (n, p)\n"
            "print('DET PLANS OK')\n") % (os.path.dirname(HERE), HERE, PKG_NAME)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True,
                       env=dict(os.environ, ASRK_DETERMINISTIC="1"), timeout=120)
    assert r.returncode == 0 and 'DET PLANS OK' in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]
    assert any(R.LN_BY_NAME[n].rows > 64 for n in R.LN_DET_ROWS)     # rows that get several chunks without the knob
    assert {R.COLSUM_BY_NAME[n].variant for n in R.COLSUM_DET_ROWS} == {0, 1, 2}


def test_plan_info_argument_checks(L):
    n = R.PLAN_LEN
    out = (ctypes.c_int64 * (n + 2))(*([7] * (n + 2)))
    ptrs = (ctypes.c_void_p * 4)(A, A, A, A)
    args = (ctypes.c_int64 * 8)(3, 5, 256, 2000, 300, 2000, 300, 0)
    f = L.asrk_rowops_plan_info
    assert f(R.OP_COPY3D, ptrs, args, None, n) == EINVAL
    assert f(R.OP_COPY3D, ptrs, args, out, n - 1) == EINVAL and list(out) == [7] * (n + 2)
    assert f(99, ptrs, args, out, n) == EINVAL and list(out) == [0] * n + [7, 7]       # zeroed first, nothing beyond n
    assert f(R.OP_COPY3D, ptrs, None, out, n) == EINVAL and f(R.OP_COPY3D, None, args, out, n) == EINVAL
    assert f(R.OP_COPY3D, ptrs, args, out, n) == 0 and out[0] == 4
    # what the entries refuse, the query refuses; what they accept as empty launches nothing
    for op, p, a, rc in ((R.OP_COPY3D, [A, A], [-1, 5, 256, 0, 0, 0, 0, 0], EINVAL),
                         (R.OP_COPY3D, [0, A], [3, 5, 256, 2000, 300, 2000, 300, 0], EINVAL),
                         (R.OP_COPY3D, [0, 0], [0, 5, 256, 2000, 300, 2000, 300, 0], 0),
                         (R.OP_COLSUM, [A, A], [5, 8, 7, 0], EINVAL), (R.OP_COLSUM, [A, A], [-1, 8, 8, 0], EINVAL),
                         (R.OP_COLSUM, [A, 0], [5, 8, 8, 0], EINVAL), (R.OP_COLSUM, [0, 0], [5, 0, 8, 0], 0),
                         (R.OP_COLSUM, [0, A], [0, 8, 8, 0], 0),
                         (R.OP_DROPOUT, [A, A], [-1], EINVAL), (R.OP_DROPOUT, [A, 0], [4], EINVAL),
                         (R.OP_DROPOUT, [0, 0], [0], 0),
                         (R.OP_ADADELTA, [A, A, A, A], [-1], EINVAL), (R.OP_ADADELTA, [A, A, 0, A], [4], EINVAL),
                         (R.OP_ADADELTA, [0, 0, 0, 0], [0], 0),
                         (R.OP_LN_PARAM, [], [-1, 4], EINVAL), (R.OP_LN_PARAM, [], [4, 0], EINVAL),
                         (R.OP_LN_PARAM, [], [0, 4], 0)):
        got_rc, d = R.plan_info(L, op, p, a)
        assert got_rc == rc, (op, p, a, got_rc)
        assert d['launches'] == 0
    rc, d = R.plan_info(L, R.OP_COLSUM, [0, A], [0, 8, 8, 0])          # M == 0: no kernel, but out is zeroed
    assert rc == 0 and d['zeroed'] == 1 and d['launches'] == 0
    rc, d = R.plan_info(L, R.OP_COLSUM, [0, A], [0, 8, 8, 1])
    assert rc == 0 and d['zeroed'] == 0
