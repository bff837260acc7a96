"""CPU: every row of the GEMM case table (tests/gemm_reference.py) gets the kernel it names - asked of the library itself
through asrk_gemm_plan_info (host only, planned for a 256-CU device) - and the table reaches every kernel variant the
dispatch of asrk_gemm_f32 (csrc/gemm.hip) can launch.  A re-tune that moves a row to another kernel fails here instead of
silently taking a kernel out of the GPU tests' reach: then move the SHAPE, not the assertion.  Also the self-checks of the
references the GPU test judges by."""
import ctypes
import importlib
import json
import os
import subprocess
import sys

import pytest
import torch

from conftest import PKG_NAME
import gemm_reference as R
import gemm_worker as W

HERE = os.path.dirname(os.path.abspath(__file__))
KNOBS = ("ASRK_GEMM_NOFAST", "ASRK_GEMM_NOSKINNY", "ASRK_SKINNY_SK", "ASRK_DETERMINISTIC")


@pytest.fixture(scope="module")
def L():
    importlib.import_module(PKG_NAME + ".build").build(verbose=False)
    return W.load()


def _child_plans(knobs, names, ncu=R.NCU):
    env = {k: v for k, v in os.environ.items() if not k.startswith("ASRK_")}
    env.update(dict(knobs))
    r = subprocess.run([sys.executable, os.path.join(HERE, "gemm_worker.py"), "plan", str(ncu)] + names,
                       capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert [o["case"] for o in out] == names
    return out


@pytest.fixture(scope="module")
def plans(L):
    """row name -> plan record at 256 CUs: plain rows in-process (refused if the environment sets a knob), knob rows from
    one child process per knob set"""
    assert not [k for k in os.environ if k in KNOBS], "run the plan test without GEMM knobs in the environment"
    got = {}
    for r in R.ROWS:
        if not r.knobs:
            rc, d = W.plan_info(L, r, R.NCU)
            got[r.name] = dict(d, rc=rc)
    for knobs in R.KNOB_SETS:
        for o in _child_plans(knobs, [r.name for r in R.knob_rows(knobs)]):
            got[o["case"]] = o
    return got


@pytest.mark.parametrize("row", R.ROWS, ids=lambda r: r.name)
def test_row_gets_the_kernel_it_names(plans, row):
    p = plans[row.name]
    assert W.plan_matches(row, p["rc"], p), W.plan_message(row, p["rc"], p)
    assert p["ncu"] == R.NCU
    # the record is one plan: its parts add up
    assert p["a_kc"] == (row.mode != "TN") and p["b_kc"] == (row.mode == "NT")
    if p["path"] == R.SPLIT:
        assert p["launches"] == 3 and p["splitk"] == 1
        return
    assert p["launches"] == 1 + (p["pre"] != R.PRE_NONE)
    assert p["gy"] == p["splitk"] == len(R.k_ranges(row)) and all(n > 0 for n in R.k_ranges(row)) or row.K == 0
    assert (p["store"] == R.ST_ATOMIC) == (p["splitk"] > 1)
    assert (p["pre"] == R.PRE_MEMSET) == (row.beta == 0 and p["store"] in (R.ST_ATOMIC, R.ST_ADD))
    assert (p["pre"] == R.PRE_SCALE) == (row.beta not in (0, 1) and p["store"] in (R.ST_ATOMIC, R.ST_ADD))
    if p["path"] in (R.SK_NT, R.SK_NN):
        assert (p["gx"], p["gz"]) == (-(-row.N // (32 if p["path"] == R.SK_NT else 128)), -(-row.M // 32))
        assert p["lds"] == 0 and p["kps"] % (128 if p["path"] == R.SK_NT else 64) == 0
    else:
        assert (p["gx"], p["gz"]) == (-(-row.M // 128) * -(-row.N // 128), 1)
        assert p["kps"] % 32 == 0 and 73728 <= p["lds"] <= 158 * 1024
        assert p["lds"] == 73728 or (p["path"] == R.FAST and row.flags >> 8)


def test_table_reaches_every_variant(plans):
    rows = [r for r in R.ROWS if r.run]
    P = lambda r: plans[r.name]
    # both skinny kernels, times every way beta * C is established and stored
    forms = {(R.PRE_NONE, R.ST_OVER), (R.PRE_MEMSET, R.ST_ATOMIC), (R.PRE_SCALE, R.ST_ATOMIC), (R.PRE_NONE, R.ST_ATOMIC),
             (R.PRE_NONE, R.ST_ADD), (R.PRE_SCALE, R.ST_ADD)}
    for path in (R.SK_NT, R.SK_NN):
        assert {(P(r)["pre"], P(r)["store"]) for r in rows if P(r)["path"] == path} == forms
        ks = {P(r)["splitk"] for r in rows if P(r)["path"] == path}
        assert {1, 2, 3, 8} <= ks
        sk = [r for r in rows if P(r)["path"] == path]
        assert any(r.M == 1 for r in sk) and any(r.K % 32 for r in sk) and any(R.k_ranges(r)[-1] == 8 for r in sk)
        assert any(r.N % (32 if path == R.SK_NT else 128) for r in sk) and any(r.b1 and r.b2 for r in sk)
    # the 3 fast layouts, times the seven forms of the K loop; each also with split-K where only the last range is ragged
    for mode in ("NT", "NN", "TN"):
        fast = [r for r in rows if P(r)["path"] == R.FAST and r.mode == mode]
        assert {R.loop_form(n) for r in fast for n in R.k_ranges(r)} == R.LOOP_FORMS, mode
        assert {R.loop_form(R.k_ranges(r)[0]) for r in fast if P(r)["splitk"] == 1} == R.LOOP_FORMS, mode
    # the 6 generic instantiations <A_KC, B_KC, VEC>, each with k to multiply (K > 0)
    gen = {(P(r)["a_kc"], P(r)["b_kc"], P(r)["vec"]) for r in rows if P(r)["path"] == R.GENERIC and r.K > 0}
    assert gen == {(a, b, v) for (a, b) in ((1, 1), (1, 0), (0, 0)) for v in (0, 1)}
    assert {r.mode for r in rows if P(r)["path"] == R.GENERIC and r.K == 0} == {"NT", "NN", "TN"}
    for path in (R.FAST, R.GENERIC):
        mine = [r for r in rows if P(r)["path"] == path]
        # split-K with a ragged last range, and every pre-pass under the atomics
        assert any(P(r)["splitk"] > 1 and R.k_ranges(r)[-1] % 32 for r in mine), path
        # tile counts the XCD remap treats unevenly: r8 != 0 and q8 >= 1
        assert any(P(r)["gx"] >= 9 and P(r)["gx"] % 8 for r in mine), path
    fast = [r for r in rows if P(r)["path"] == R.FAST]
    assert {P(r)["pre"] for r in fast if P(r)["splitk"] > 1} == {R.PRE_NONE, R.PRE_MEMSET, R.PRE_SCALE}
    assert {P(r)["gx"] for r in fast} >= {1, 8, 9, 15, 17}
    assert {P(r)["lds"] for r in fast} == {73728, 96 * 1024, 158 * 1024}
    assert any(r.offa for r in rows) and any(r.offb for r in rows)
    assert {P(r)["path"] for r in R.ROWS} == {R.SK_NT, R.SK_NN, R.SPLIT, R.FAST, R.GENERIC}
    # deterministic rows: one K range, no atomics, on shapes that split K without the knob
    det = R.knob_rows(R.DETERMINISTIC)
    assert det and all(P(r)["splitk"] == 1 and P(r)["store"] != R.ST_ATOMIC for r in det)
    assert all(P(R.ROW_BY_NAME[r.name.split("@")[0]])["store"] == R.ST_ATOMIC for r in det)


def test_each_skinny_condition_routes_away(L):
    """one condition flipped at a time on a base shape that takes the skinny kernel"""
    info = (ctypes.c_int * 16)()

    def path(mode, M=8, N=64, K=64, lda=None, ldb=None, align=3, splitk=0, flags=0):
        ta, tb = R.TRANS[mode]
        la, lb = (K if ta == 0 else M), (K if tb else N)
        rc = L.asrk_gemm_plan_info(ta, tb, M, N, K, la if lda is None else lda, lb if ldb is None else ldb, N, align,
                                   0.0, splitk, flags, R.NCU, info)
        assert rc == 0
        return info[0]

    assert path("NT") == R.SK_NT and path("NN") == R.SK_NN
    assert path("NT", M=32) == R.SK_NT and path("NT", K=32) == R.SK_NT and path("NT", splitk=1) == R.SK_NT
    assert path("NT", flags=R.SPLIT_ALWAYS) == R.SK_NT             # the skinny kernels come before the split path
    for mode in ("NT", "NN"):
        tiled = (R.FAST, R.GENERIC)
        assert path(mode, M=33) in tiled
        assert path(mode, K=28) in tiled and path(mode, K=34) in tiled
        assert path(mode, lda=66) in tiled and path(mode, ldb=66) in tiled
        assert path(mode, align=2) in tiled and path(mode, align=1) in tiled
        assert path(mode, splitk=2) in tiled
    assert path("NN", N=6) in tiled and path("NN", N=2) in tiled
    assert path("TN") == R.FAST
    assert path("NT", K=34, flags=R.SPLIT_ALWAYS) == R.SPLIT


def test_plan_info_rejects_where_the_launch_does(L):
    info = (ctypes.c_int * 16)()
    EINVAL = -1
    q = lambda *a: L.asrk_gemm_plan_info(*a)
    z = ctypes.c_void_p(0)
    fake = ctypes.c_void_p(4096)

    def launch(ta, tb, M, N, K, lda, ldb, ldc, flags=0):
        return L.asrk_gemm_f32(ta, tb, M, N, K, 1.0, fake, lda, fake, ldb, 0.0, fake, ldc, z, z, 0, flags, z, 0, z)

    bad = [(1, 1, 8, 8, 8, 8, 8, 8, 0),              # TT
           (0, 1, -1, 8, 8, 8, 8, 8, 0), (0, 1, 8, -1, 8, 8, 8, 8, 0), (0, 1, 8, 8, -1, 8, 8, 8, 0),
           (0, 1, 8, 8, 8, 8, 8, 8, -1),             # negative flags
           (0, 1, 8, 8, 8, 7, 8, 8, 0), (1, 0, 8, 8, 4, 7, 8, 8, 0),      # lda below K / below M
           (0, 1, 8, 8, 8, 8, 7, 8, 0), (0, 0, 8, 8, 4, 4, 7, 8, 0),      # ldb below K / below N
           (0, 1, 8, 8, 8, 8, 8, 7, 0)]                                   # ldc below N
    for ta, tb, M, N, K, lda, ldb, ldc, flags in bad:
        assert q(ta, tb, M, N, K, lda, ldb, ldc, 3, 0.0, 0, flags, 256, info) == EINVAL
        assert launch(ta, tb, M, N, K, lda, ldb, ldc, flags) == EINVAL       # before it touches a pointer's target
        assert list(info) == [0] * 16
    assert q(0, 1, 8, 8, 8, 8, 8, 8, 3, 0.0, 0, 0, 256, None) == EINVAL
    assert q(0, 1, 8, 8, 8, 8, 8, 8, 3, 0.0, 0, 0, -1, info) == EINVAL
    for M, N in ((0, 8), (8, 0)):                     # nothing to do: OK, no launch - also for TT and a short ld
        assert q(0, 1, M, N, 8, 8, 8, 8, 3, 0.0, 0, 0, 256, info) == 0 and info[12] == 0
        assert q(1, 1, M, N, 8, 1, 1, 1, 3, 0.0, 0, 0, 256, info) == 0 and info[12] == 0
        assert launch(0, 1, M, N, 8, 8, 8, 8) == 0 and launch(1, 1, M, N, 8, 1, 1, 1) == 0
    assert q(0, 1, 8, 8, 8, 8, 8, 8, 3, 0.0, 0, 0, 256, info) == 0 and info[12] == 1 and info[13] == 256
    assert q(0, 1, 8, 8, 8, 8, 8, 8, 3, 0.0, 0, 0, 104, info) == 0 and info[13] == 104
    if not torch.cuda.is_available():                 # ncu == 0 without a device: 256, as the launch assumes
        assert q(0, 1, 8, 8, 8, 8, 8, 8, 3, 0.0, 0, 0, 0, info) == 0 and info[13] == 256


def test_plan_depends_on_the_cu_count_only_through_the_k_split(L):
    """the kernel instantiation never depends on the CU count; the K split does (the table is written for 256 CUs)"""
    for r in R.ROWS:
        if r.knobs:
            continue
        a, b = W.plan_info(L, r, 256)[1], W.plan_info(L, r, 64)[1]
        assert [a[k] for k in ("path", "a_kc", "b_kc", "vec", "gx", "gz")] == [b[k] for k in ("path", "a_kc", "b_kc", "vec",
                                                                                               "gx", "gz")]


# ------------------------------------------------------------------------------------------ the references themselves
RUN_ROWS = [r for r in R.ROWS if r.run and "@" not in r.name and r.twin is None]      # one per distinct data set


@pytest.mark.parametrize("row", RUN_ROWS, ids=lambda r: r.name)
def test_references_and_bounds(row):
    r = row
    # exact data: int64 and float64 agree, every value is a float32, and the wrong references differ
    d = R.make_inputs(r, "exact")
    ref = R.reference_int64(r, d)
    assert torch.equal(ref, R.reference(r, d)) and torch.equal(ref.float().double(), ref)
    assert float(ref.abs().max()) < 2 ** 24 and torch.equal(ref * 2, (ref * 2).round())
    assert torch.equal(R.reference_seq32(r, d).double(), ref)            # sequential f32 accumulation is exact too
    muts = R.mutations(r, d)
    assert muts or (r.K == 0 and not r.b1 and not r.b2 and r.M == r.N == 1)
    for name, m in muts.items():
        assert not torch.equal(R.to_f32_bits(m), R.to_f32_bits(ref)), name
    # gaussian data: sequential f32 stays below half the bound; the wrong references violate it
    d = R.make_inputs(r, "gauss")
    ref = R.reference(r, d)
    e32 = R.ratio(r, d, R.reference_seq32(r, d), ref) * R.BOUND
    assert e32 < R.SEQ32_BOUND, e32
    for name, m in R.mutations(r, d).items():
        assert R.ratio(r, d, m.float(), ref) > 1.0, name
    # the operands sit in NaN: everything around them, nothing in them
    for buf, start, ld, shape in ((d["Abuf"], d["a_start"], r.lda, d["A"].t().shape if r.mode == "TN" else d["A"].shape),
                                  (d["Bbuf"], d["b_start"], r.ldb, d["B"].t().shape if r.mode == "NT" else d["B"].shape)):
        inner = torch.as_strided(buf, tuple(shape), (ld, 1), start)
        assert not bool(torch.isnan(inner).any())
        assert int(torch.isnan(buf).sum()) == buf.numel() - inner.numel()
        assert start - ld >= R.MARGIN and buf.numel() - (start + shape[0] * ld) >= R.MARGIN
    assert not bool(torch.isnan(d["Cbuf"]).any()) and r.ldc >= r.N + 3


def test_table_rows_are_small_and_distinct():
    assert max(max(r.M * r.K, r.K * r.N, r.M * r.N) for r in R.ROWS) <= 2052 * 36 * 4
    assert len({r.name for r in R.ROWS}) == len(R.ROWS)
    a, b = R.make_inputs(R.ROWS[1], "gauss"), R.make_inputs(R.ROWS[1], "gauss")
    assert a is b
