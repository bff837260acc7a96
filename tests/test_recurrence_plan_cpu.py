"""CPU: every row of the recurrence case table (tests/recurrence_reference.py) gets the kernel variant it names - asked
of the library itself through asrk_lstm_plan_info (host only, planned for a 256-CU device) - and the table reaches every
variant the four dispatch functions (launch_fwd_plan, launch_fwd_bf_plan, launch_bwd_plan, launch_bwd_bf) can launch
and a plan can select at all.  A re-tune that moves a row to another variant fails here instead of silently taking a
kernel out of the GPU tests' reach: then move the SHAPE, not the assertion."""
import ctypes
import importlib
import json
import os
import subprocess
import sys

import pytest

from conftest import PKG_NAME
import recurrence_reference as R
import recurrence_worker as W

HERE = os.path.dirname(os.path.abspath(__file__))
F, BF = "f32", "bf"

# Every instantiation the dispatch functions name, minus the ones no plan reaches on any device (DESIGN §4 lists them
# with the reason): forward f32 <MT, NT, KGW, DB> ...
FWD_F32 = {
    (F, 1, 1, 4, 1), (F, 1, 1, 8, 1), (F, 1, 1, 16, 1),
    (F, 1, 2, 4, 1), (F, 1, 2, 8, 1), (F, 1, 2, 16, 1),
    (F, 2, 1, 4, 1), (F, 2, 1, 8, 1), (F, 2, 1, 16, 1),
    (F, 2, 2, 4, 1), (F, 2, 2, 8, 1), (F, 2, 2, 16, 0),
    (F, 1, 4, 4, 1), (F, 1, 4, 8, 1), (F, 1, 4, 16, 1),
    (F, 4, 1, 4, 1), (F, 4, 1, 8, 0),
}
# ... forward bf16x6 <MT, NT, DB, KSW> written as (MT, NT, KSW, DB) ...
FWD_BF = {(BF, 2, 1, 4, 1), (BF, 2, 2, 4, 1), (BF, 2, 1, 8, 1), (BF, 2, 2, 8, 0), (BF, 4, 1, 8, 0)}
# ... backward f32 (UB, NT, RK): <NT, RK> with the run-time UB; RK = 32 needs NT = 1 and a slice too long for LDS: UB = 16
# from H = 640, UB = 8 only past H = 1024 (no forward plan there, but the BPTT entry point takes it) ...
BWD_F32 = {(F, ub, nt, 0) for ub in (16, 8, 4) for nt in (1, 2, 4)} | {(F, 16, 1, 32), (F, 8, 1, 32)}
# ... backward bf16x6: <KS = 16> (H = 512) and <KS = 32> (H = 1024), told apart by the row's H
BWD_BF = {(BF, 16, 1, 0)}


@pytest.fixture(scope="module")
def L():
    importlib.import_module(PKG_NAME + ".build").build(verbose=False)
    return W.load()


def _child_plans(knobs, names, ncu=R.NCU):
    """plan_info of the named cases from a child process started with the knobs in its environment"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("ASRK_")}
    env.update(dict(knobs))
    r = subprocess.run([sys.executable, os.path.join(HERE, "recurrence_worker.py"), "plan", str(ncu)] + names,
                       capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert [o["case"] for o in out] == names
    return out


@pytest.fixture(scope="module")
def plans(L):
    """row name -> plan record at 256 CUs: plain rows in-process (refused if the environment sets a knob), knob rows
    from one child process per knob set"""
    assert not [k for k in os.environ if k.startswith("ASRK_FWD_") or k.startswith("ASRK_BWD_")
                or k == "ASRK_REC_BF_MT4"], "run the plan test without recurrence tuning knobs in the environment"
    got = {}
    for r in R.ROWS:
        if not r.knobs:
            rc, d = W.plan_info(L, r, R.NCU)
            got[r.name] = dict(d, rc=rc)
    for knobs in R.KNOB_SETS:
        names = [r.name for r in R.ROWS if r.knobs == knobs]
        for o in _child_plans(knobs, names):
            got[o["case"]] = o
    return got


@pytest.mark.parametrize("row", R.ROWS, ids=lambda r: r.name)
def test_row_gets_the_variant_it_names(plans, row):
    p = plans[row.name]
    assert p["rc"] == 0, p
    assert tuple(p["variant"]) == row.variant, p
    assert p["launches"] == row.launches, p
    # the record is one plan: its parts add up
    assert p["workgroups"] == p["ndir_l"] * p["nbg_l"] * p["nwg"] <= R.NCU
    assert p["launches"] == -(-row.ndir // p["ndir_l"]) * -(-p["nbg"] // p["nbg_l"])
    assert 0 < p["lds"] <= 160 * 1024 and p["xbytes"] > 0 and p["xbytes"] % 256 == 0 and p["ncu"] == R.NCU
    bg = 16 * p["nt"]
    assert p["nbg"] == -(-row.B // bg)
    units = p["a"] if row.bwd else 4 * p["a"]
    assert p["nwg"] == -(-row.H // units)


def test_table_reaches_every_selectable_variant(plans):
    def got(bwd, fam):
        return {tuple(plans[r.name]["variant"]) for r in R.ROWS if r.bwd == bwd and plans[r.name]["variant"][0] == fam}
    assert got(0, F) == FWD_F32
    assert got(0, BF) == FWD_BF
    assert got(1, F) == BWD_F32
    assert got(1, BF) == BWD_BF
    assert {r.H for r in R.ROWS if r.bwd and r.variant[0] == BF} == {512, 1024}      # both backward bf16x6 kernels
    # the several-launches fallback in both directions, one of them with a last launch of fewer batch groups
    multi = [plans[r.name] for r in R.ROWS if r.launches > 1]
    assert {r.bwd for r in R.ROWS if r.launches > 1} == {0, 1}
    assert any(p["nbg"] % p["nbg_l"] for p in multi) and any(p["nbg"] % p["nbg_l"] == 0 for p in multi)
    assert any(r.H % 16 for r in R.ROWS if not r.bwd) and any(r.H % 16 for r in R.ROWS if r.bwd)


def _classes(row):
    """the multi-tile properties of a row's variant"""
    v = row.variant
    if row.bwd:
        return {n for n, on in (("UB<16", v[1] < 16), ("NT>1", v[2] > 1), ("RK=32", v[3] == 32)) if on}
    return {n for n, on in (("MT>1", v[1] > 1), ("NT>1", v[2] > 1), ("DB=0", v[4] == 0)) if on}


def test_modes_gru_and_lens_cover_every_multi_tile_class():
    fams = {}
    for c in R.CASES:
        fams.setdefault((c.row.bwd, c.row.variant[0]), []).append(c)
    assert len(fams) == 4
    for (bwd, fam), cases in fams.items():
        classes = set().union(*[_classes(c.row) for c in cases])
        classes.discard("DB=0")                                   # asked of the GRU rows only
        for cl in classes:
            modes = {c.mode[0] for c in cases if cl in _classes(c.row)}
            assert {1, 2} <= modes, (bwd, fam, cl, modes)         # a 'concat' and a 'drop' each
        gru = set().union(*[_classes(c.row) for c in cases if c.kind == "gru"])
        want = {"UB<16", "NT>1"} | ({"RK=32"} if fam == F else set()) if bwd else {"MT>1", "NT>1", "DB=0"}
        assert want & set().union(*[_classes(c.row) for c in cases]) <= gru, (bwd, fam, gru)
    gru_bwd = {c.row.variant[1:3] for c in R.CASES if c.kind == "gru" and c.row.bwd and c.row.variant[0] == F}
    assert {(8, 2), (8, 4)} <= gru_bwd and {nt for _, nt in gru_bwd} >= {2, 4}
    assert any(c.kind == "gru" and c.row.H == 640 and c.row.variant == (F, 16, 1, 32) for c in R.CASES)
    assert {c.mode for c in R.CASES} == set(R.MODES)
    lens = {c.row.variant for c in R.CASES if c.kind == "lens"}
    assert (F, 4, 1, 8, 0) in lens and (BF, 4, 1, 8, 0) in lens and any(v[0] == F and v[2] == 2 for v in lens)
    for c in R.CASES:
        if c.kind == "lens":
            ln = R.case_lens(c).tolist()
            assert 1 in ln and R.T in ln
            bg = 16 * c.row.variant[2]
            for g0 in range(0, c.row.B, bg):
                tile = ln[g0:g0 + bg]
                assert len(tile) == 1 or len(set(tile)) > 1, (c.name, g0)


def test_every_case_uses_t7_and_fixed_seeds():
    assert R.T == 7
    assert len({c.name for c in R.CASES}) == len(R.CASES)
    a, b = R.make_inputs(R.CASES[0]), R.make_inputs(R.CASES[0])
    assert all(bool((x == y).all()) for x, y in zip([a[0], *a[1], a[2]], [b[0], *b[1], b[2]]))


def test_plan_info_rejects_where_the_launch_does(L):
    info = (ctypes.c_int * 16)()
    q = lambda *a: L.asrk_lstm_plan_info(*a)
    EINVAL, ESHAPE, EDEVICE = -1, -2, -4
    for bwd in (0, 1):
        assert q(7, 3, 20, 2, bwd, 0, 256, None) == EINVAL
        assert q(7, 3, 20, 2, bwd, -1, 256, info) == EINVAL
        assert q(7, 3, 20, 2, bwd, 0, -1, info) == EINVAL
        assert q(-1, 3, 20, 2, bwd, 0, 256, info) == EINVAL
        assert q(7, 0, 20, 2, bwd, 0, 256, info) == EINVAL
        assert q(7, 3, 0, 2, bwd, 0, 256, info) == EINVAL
        assert q(7, 3, 20, 3, bwd, 0, 256, info) == EINVAL and q(7, 3, 20, 0, bwd, 0, 256, info) == EINVAL
        assert q(7, 3, 22, 2, bwd, 0, 256, info) == ESHAPE                  # H % 4 != 0
        assert q(0, 3, 20, 2, bwd, 0, 256, info) == 0 and info[5] == 0      # T == 0: the launch returns OK, 0 launches
        assert q(7, 3, 20, 2, bwd, 0, 256, info) == 0 and info[5] == 1
    # no plan at all: a unit slice that fits no LDS / a layer with more slices than CUs
    assert q(7, 1, 1028, 1, 0, 0, 256, info) == ESHAPE                      # forward: more than 16 k-groups per wave
    assert q(7, 1, 4096, 1, 1, 0, 256, info) == ESHAPE                      # backward: H = 4096 fits no LDS slice
    assert q(7, 1, 512, 1, 0, 0, 2, info) == ESHAPE                         # 2 CUs: no tile covers 512 units
    # the launch itself answers the same, before it touches a pointer's target (no device needed for EINVAL)
    z = ctypes.c_void_p(0)
    assert L.asrk_lstm_rec_fwd_f32(z, z, z, z, z, 7, 3, 20, 2, z, 0, z, -1, z) == EINVAL
    assert L.asrk_lstm_rec_fwd_f32(z, z, z, z, z, 7, 3, 20, 3, z, 0, z, 0, z) == EINVAL
    import torch
    if not torch.cuda.is_available():
        assert q(7, 3, 20, 2, 0, 0, 0, info) == EDEVICE                     # ncu == 0 asks the device


def test_older_queries_are_views_of_plan_info(L):
    """asrk_lstm_plan_workgroups / _is_bf / asrk_lstm_xchg_bytes answer from plan_info at the device's CU count: equal
    to it where a device is present, 0 ('unsupported') exactly where plan_info(ncu = 0) fails"""
    info = (ctypes.c_int * 16)()
    shapes = [(r.B, r.H, r.ndir, r.bwd, r.flags) for r in R.ROWS if not r.knobs] + [(3, 22, 2, 0, 0), (1, 4096, 1, 1, 0)]
    for B, H, ndir, bwd, flags in shapes:
        rc = L.asrk_lstm_plan_info(R.T, B, H, ndir, bwd, flags, 0, info)
        a = (R.T, B, H, ndir, bwd, flags)
        if rc != 0:
            assert L.asrk_lstm_plan_workgroups(*a) == 0 and L.asrk_lstm_plan_is_bf(*a) == 0
            assert L.asrk_lstm_xchg_bytes(*a) == 0
        else:
            assert L.asrk_lstm_plan_workgroups(*a) == info[11] == info[6] * info[7] * info[8]
            assert L.asrk_lstm_plan_is_bf(*a) == info[0]
            assert L.asrk_lstm_xchg_bytes(*a) == (info[13] << 31) | info[12] > 0


def test_exchange_bytes_follow_from_the_reported_plan(plans):
    """the exchange size in the record is the documented layout of the kernel the record names: per (direction, batch
    group) of a launch and step, kgp k-groups x NT tiles x 1 KiB (x 4 gates backward, x 3 bf16 planes packed for the
    bf16x6 kernels) plus 4 canary words per producer padded to 256 B"""
    for r in R.ROWS:
        p = plans[r.name]
        canw = -(-4 * p["nwg"] // 64) * 64
        kg = -(-r.H // 16)
        if p["bf"]:
            frag = (r.H // 32) * p["nt"] * 3 * 256
        else:
            frag = kg * p["nt"] * 256
        if r.bwd:
            frag *= 4
        assert p["xbytes"] == 4 * p["ndir_l"] * p["nbg_l"] * R.T * (frag + canw), (r.name, p)
