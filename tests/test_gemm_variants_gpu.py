"""GPU: every kernel variant of the exact-f32 GEMM dispatch (csrc/gemm.hip: the two skinny kernels, the fast tiled kernel
in its 3 layouts and 7 K-loop forms, the 6 generic instantiations, every way beta * C is established), called through
asrk_gemm_f32 on the case table of tests/gemm_reference.py (tests/test_gemm_plan_cpu.py holds every row to its plan
record and the table to the whole set of variants).

Per row: asrk_gemm_plan_info(ncu = 0) gives the record the row names - on a device whose CU count plans otherwise the
row FAILS with a message naming both plans (the table is written for 256 CUs), it never skips; on the integer data
C[:M, :N] equals the int64 reference bit for bit; on the Gaussian data |C - ref| <= 2e-6 * (|alpha| |A| |B| + |beta C0|
+ |b1| + |b2| + 1) elementwise against float64 (the error-to-bound ratio is printed); the guard columns, guard rows and
margins of C are bit-unchanged and no NaN of the operands' surroundings reaches C; a second call on a fresh C is
bit-identical (rows with atomics: on the integer data, where the order cannot matter); check_errors is clean.

Rows whose kernel only a knob selects run in one child process per knob set (knobs are read once per process)."""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

import gemm_reference as R
import gemm_worker as W

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
OK, EINVAL, EWORKSPACE = 0, -1, -3


def _judge(r, out):
    assert "failed" not in out, out
    assert tuple(out["plan"]) == tuple(int(x) for x in r.plan), out
    print("%-22s %-9s grid %-14s K ranges %d x %-4d pre %d store %d  error / bound = %.3f" % (
        r.name, out["path"], out["grid"], out["plan"][4], out["plan"][5], out["plan"][6], out["plan"][7], out["ratio"]))
    assert out["exact_equal"], "%d elements differ from the int64 reference" % out["exact_mismatches"]
    assert out["exact_guards_ok"] and out["gauss_guards_ok"], "bytes around C[:M, :N] changed"
    assert out["exact_nan_free"] and out["gauss_nan_free"], "a NaN from outside the operands reached C"
    assert out["exact_repeat_equal"], "a second call on the integer data changed bits"
    if not out["atomic"]:
        assert out["gauss_repeat_equal"], "a second call without atomics changed bits"
    if r.twin is not None:
        assert out["twin_equal"], "the LDS hint changed the result"
    assert out["ratio"] <= 1.0, out["ratio"]


@pytest.mark.parametrize("row", R.PLAIN_RUN_ROWS, ids=lambda r: r.name)
def test_variant_exact_and_vs_float64(ops, row):
    L = W.load()
    rc, d = W.plan_info(L, row, 0)
    assert W.plan_matches(row, rc, d), "on this device: " + W.plan_message(row, rc, d)
    _judge(row, W.run_case(L, row, ops))


@pytest.mark.parametrize("knobs", R.KNOB_SETS, ids=lambda k: ",".join("%s=%s" % kv for kv in k))
def test_knob_selected_variants(ops, knobs):
    """one child process per knob set; it checks plan_info for every row before it launches it and stops at the first
    failure.  Not retried."""
    rows = R.knob_rows(knobs)
    env = {k: v for k, v in os.environ.items() if not k.startswith("ASRK_")}
    env.update(dict(knobs))
    r = subprocess.run([sys.executable, os.path.join(HERE, "gemm_worker.py"), "run"] + [x.name for x in rows],
                       capture_output=True, text=True, env=env, timeout=90)
    outs = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0, (outs[-1:] or r.stdout[-500:], r.stderr[-2000:])
    assert [o["case"] for o in outs] == [x.name for x in rows]
    for x, o in zip(rows, outs):
        _judge(x, o)


def test_abi_returns(ops):
    """the return codes of asrk_gemm_f32, called directly; a rejected call and an empty one do not touch C"""
    L = W.load()
    dev = "cuda"
    A = torch.ones(64 * 64, device=dev)
    B = torch.ones(64 * 64, device=dev)
    C = torch.full((64 * 64,), 7.0, device=dev)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(ta, tb, M, N, K, a=p(A), lda=64, ldb=64, ldc=64, flags=0, ws=None, nws=0):
        return L.asrk_gemm_f32(ta, tb, M, N, K, 1.0, a, lda, p(B), ldb, 0.0, p(C), ldc, None, None, 0, flags, ws, nws,
                               stream)

    assert call(1, 1, 8, 8, 8) == EINVAL                       # TT
    assert call(0, 1, -1, 8, 8) == EINVAL and call(0, 1, 8, -1, 8) == EINVAL and call(0, 1, 8, 8, -1) == EINVAL
    assert call(0, 1, 8, 8, 64, lda=63) == EINVAL              # lda below K
    assert call(1, 0, 64, 8, 8, lda=63) == EINVAL              # TN: lda below M
    assert call(0, 0, 8, 64, 8, ldb=63) == EINVAL and call(0, 1, 8, 64, 8, ldc=63) == EINVAL
    assert call(0, 1, 8, 8, 8, a=None) == EINVAL               # NULL A with M, N > 0
    assert call(0, 1, 0, 8, 8) == OK and call(0, 1, 8, 0, 8) == OK
    need = L.asrk_gemm_ws_bytes(64, 64, 64, R.SPLIT_ALWAYS)
    assert need > 0
    ws = torch.zeros(need + 16, dtype=torch.uint8, device=dev)
    assert call(0, 1, 64, 64, 64, flags=R.SPLIT_ALWAYS) == EWORKSPACE
    assert call(0, 1, 64, 64, 64, flags=R.SPLIT_ALWAYS, ws=p(ws), nws=need - 1) == EWORKSPACE
    assert call(0, 1, 64, 64, 64, flags=R.SPLIT_ALWAYS, ws=p(ws, 8), nws=need) == EINVAL     # misaligned by 8 bytes
    torch.cuda.synchronize()
    assert bool((C == 7.0).all())
    assert call(0, 1, 64, 64, 64, flags=R.SPLIT_ALWAYS, ws=p(ws), nws=need) == OK            # and the good call runs
    torch.cuda.synchronize()
    assert bool((C == 64.0).all())
    ops.check_errors()
