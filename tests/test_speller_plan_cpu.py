"""CPU: every shape of the decoder-loop case table (tests/speller_reference.py) gets the kernel variant the table
names, and the table reaches every variant `make_plan` / `speller_step_fwd` can select for the training loop - asked
of the library itself through asrk_speller_plan_info (host only).  A re-tune of the plan thresholds that moves a case
to another variant fails here instead of silently taking a kernel out of the GPU tests' reach: then move the SHAPE
(tests/speller_reference.py) back onto the variant, not the assertion."""
import ctypes
import importlib

import pytest

from conftest import PKG_NAME
import speller_reference as R


@pytest.fixture(scope="module")
def plan_info():
    importlib.import_module(PKG_NAME + ".build").build(verbose=False)
    L = importlib.import_module(PKG_NAME + "._lib").load()
    sops = importlib.import_module(PKG_NAME + ".speller_ops")

    def info(c):
        d = sops.SpellerT(c.B, c.Te, c.A, c.Dv, c.K, (c.taps - 1) // 2 if c.K else 0, R.H, R.E, c.L, R.TEMPERATURE, 0)
        d.nlayer, d.att_mode, d.nhead = c.layers, (0 if c.K else 1), c.N
        out = (ctypes.c_int * 8)()
        rc = L.asrk_speller_plan_info(ctypes.byref(d), out)
        assert rc == 0, (c.name, rc)
        tc_f, tc_b = ctypes.c_int(0), ctypes.c_int(0)
        assert L.asrk_speller_plan(ctypes.byref(d), ctypes.byref(tc_f), ctypes.byref(tc_b)) == 0
        keys = ("ae2_na", "ae2_km", "eb3_na", "eb3_km", "tpb_f", "tpb_b", "KP", "ctx_vec")
        r = dict(zip(keys, list(out)))
        # the report and the plan the launches use are one: chunk counts follow from the reported frames per workgroup
        assert tc_f.value == -(-c.Te // r["tpb_f"]) and tc_b.value == -(-c.Te // r["tpb_b"]), (c.name, r)
        return r
    return info


def _variant(na, km):
    return R.STAGED if na == 0 else (na, km)


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_case_gets_the_variant_the_table_names(plan_info, case):
    r = plan_info(case)
    assert _variant(r["ae2_na"], r["ae2_km"]) == case.fwd, r
    assert _variant(r["eb3_na"], r["eb3_km"]) == case.bwd, r
    assert bool(r["ctx_vec"]) == case.ctx_vec
    assert r["KP"] == (case.K + 1 if case.K % 2 == 0 else case.K)
    if case.name in R.TPB:
        assert (r["tpb_f"], r["tpb_b"]) == R.TPB[case.name], r


@pytest.mark.parametrize("case", R.DOT_CASES, ids=lambda c: c.name)
def test_dot_cases_plan(plan_info, case):
    r = plan_info(case)
    assert (r["ae2_na"], r["eb3_na"]) == (0, 0) and bool(r["ctx_vec"]) == case.ctx_vec


def test_table_reaches_every_variant(plan_info):
    every = {R.STAGED, (2, 12), (2, 16), (5, 12), (5, 16)}
    got = [plan_info(c) for c in R.CASES]
    assert {_variant(r["ae2_na"], r["ae2_km"]) for r in got} == every
    assert {_variant(r["eb3_na"], r["eb3_km"]) for r in got} == every
    assert {r["ctx_vec"] for r in got} == {0, 1}
    assert {bool(plan_info(c)["ctx_vec"]) for c in R.DOT_CASES} == {False, True}


def test_plan_info_rejects_what_the_plan_rejects(plan_info):
    L = importlib.import_module(PKG_NAME + "._lib").load()
    sops = importlib.import_module(PKG_NAME + ".speller_ops")
    out = (ctypes.c_int * 8)()
    d = sops.SpellerT(2, 19, 24, 12, 3, 4, R.H, R.E, 3, R.TEMPERATURE, 0)
    assert L.asrk_speller_plan_info(ctypes.byref(d), None) == -1
    assert L.asrk_speller_plan_info(None, out) == -1
    d.nhead = 2                                  # several heads: dot-product attention only
    assert L.asrk_speller_plan_info(ctypes.byref(d), out) == -2
