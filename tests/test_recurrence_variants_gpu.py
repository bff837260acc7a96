"""GPU: every kernel variant of the persistent LSTM / GRU recurrence (csrc/lstm_rec*.hip), called through the C entry
points of include/asrk.h, against the float64 reference of tests/recurrence_reference.py on the case table kept there
(tests/test_recurrence_plan_cpu.py holds every row to its variant and the table to the whole set of variants).

Forward: Y, C, the activated gates left in G, and Y2.  Backward: dG and the in-kernel db, computed ON the reference's
gates / cell states / outputs rounded to f32, so a forward error can neither cause nor hide a backward failure.  After
every launch: asrk_lstm_check_error == 0, the exchange buffer is all 0xFF again (ASRK_REC_REARM), and a second launch on
it with xchg_prefilled = 1 gives bit-identical Y / dG.

Tolerance per tensor: max(8 x e32, floor), never above the project's 1e-3, where e32 is the error of the
SAME reference run in float32 on the CPU and floor the largest e32 of that tensor kind over the table.

Each row first asserts that asrk_lstm_plan_info(ncu = 0) names the row's variant: on a device whose CU count gives
another plan the row FAILS with that message (the table is written for 256 CUs); it never skips.  Rows whose variant
only a tuning knob selects run in one child process per knob set (knobs are read once per process)."""
import json
import os
import subprocess
import sys

import pytest

import recurrence_reference as R
import recurrence_worker as W

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _judge(case, out):
    """assert one case's worker record against the bounds derived from the reference alone"""
    assert "failed" not in out, out
    assert tuple(out["variant"]) == case.row.variant and out["launches"] == case.row.launches, out
    e32 = R.e32(case)
    rows = {k: (out["errs"][k], e32[k], R.bound(case, k)) for k in e32}
    print(case.name, R.MODE_NAMES[case.mode], " ".join("%s err=%.2e e32=%.2e bound=%.2e" % ((k,) + v)
                                                       for k, v in rows.items()))
    assert set(out["errs"]) == set(e32)
    ck = out["checks"]
    assert ck["queries_agree"], "asrk_lstm_xchg_bytes / plan_workgroups / plan_is_bf disagree with plan_info"
    assert ck["rearmed"], "the exchange buffer did not come back all 0xFF"
    assert ck["replay_equal"], "a second launch on the re-armed buffer (xchg_prefilled = 1) changed bits"
    assert ck["untouched"], "the lens form wrote frames t >= lens[b] of C or G"
    bad = {k: v for k, v in rows.items() if not v[0] <= v[2]}
    assert not bad, bad
    assert all(v[2] <= R.CEILING for v in rows.values())


@pytest.mark.parametrize("case", R.PLAIN_CASES, ids=lambda c: c.name)
def test_variant_vs_float64(ops, case):
    L = W.load()
    rc, d = W.plan_info(L, case.row, 0)
    assert rc == 0 and tuple(d["variant"]) == case.row.variant and d["launches"] == case.row.launches, \
        "on this device (%d CUs) plan_info gives %s x %d launches (rc %d); the row names %s x %d" % (
            d["ncu"], d["variant"], d["launches"], rc, list(case.row.variant), case.row.launches)
    _judge(case, W.run_case(L, case))


@pytest.mark.parametrize("knobs", R.KNOB_SETS, ids=lambda k: ",".join("%s=%s" % kv for kv in k))
def test_knob_selected_variants_vs_float64(ops, knobs):
    """one child process per knob set; it checks plan_info for every row before it launches it and stops at the first
    failure.  Not retried."""
    cases = R.knob_cases(knobs)
    env = {k: v for k, v in os.environ.items() if not k.startswith("ASRK_")}
    env.update(dict(knobs))
    r = subprocess.run([sys.executable, os.path.join(HERE, "recurrence_worker.py"), "run"] + [c.name for c in cases],
                       capture_output=True, text=True, env=env, timeout=90)
    outs = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0, (outs[-1:] or r.stdout[-500:], r.stderr[-2000:])
    assert [o["case"] for o in outs] == [c.name for c in cases]
    for c, o in zip(cases, outs):
        _judge(c, o)
