"""CPU: the host-side plan of the LSTM layer backward (ops.lstm_bwd_plan) over a table of layer shapes - which panels the
BPTT kernel writes, whether it keeps the f32 dG and sums the biases, how dW_ih and dW_hh are multiplied and under which
stream schedule.  The plan is a pure function of its facts; the split-GEMM routing rule it asks is the library's own
(asrk_gemm_takes_split, host only, mode AUTO).  A re-tune that moves a row fails here, not in a step time."""
import importlib

import pytest

from conftest import PKG_NAME

AUTO = 0                                   # ASRK_GEMM_SPLIT_AUTO (include/asrk.h)
PANEL = object()                           # what the stand-in pool hands out


@pytest.fixture(scope="module")
def L():
    importlib.import_module(PKG_NAME + ".build").build(verbose=False)
    return importlib.import_module(PKG_NAME + "._lib").load()


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module(PKG_NAME + ".ops")


# the facts of a row unless it says otherwise
BASE = dict(T=12, B=32, Din=80, H=1024, ndir=2, has_bias=True, needs_dx=False, stacked=True, can_defer=True,
            to_scratch=True, beside_bptt=False, bf_bwd=True, share_env=True, skip_dg_switch=True)
NARROW = dict()                                                         # the bottom layer of the wide models
WIDE = dict(T=800, Din=4096, needs_dx=True)                             # a layer above it
# expected: (pG, pGT, db_in_kernel, skip_dg, rows_ih / H, dW_ih route, dW_hh through panels, schedule, release deferred)
NARROW_PLAN = (False, True, True, True, 8, "panels_splitk", True, "STREAM", False)
WIDE_PLAN = (True, True, True, True, 8, "panels", True, "STREAM", False)
ROWS = [
    # name, facts, panels available, expected
    ("bottom_narrow", NARROW, True, NARROW_PLAN),
    ("bottom_din36", dict(Din=36), True, NARROW_PLAN),
    ("bottom_full_length", dict(T=1600), True, NARROW_PLAN),                       # cfg3 layer 0
    ("bottom_first_sight", NARROW, False, (False, False, True, False, 4, "f32", False, "SIDE_REVERSE", False)),
    ("bottom_din38", dict(Din=38), True, (False, True, True, False, 4, "f32", True, "SIDE_REVERSE_SHARED", True)),
    ("upper_wide", WIDE, True, WIDE_PLAN),
    # dX fails the routing rule at 384 tokens and reads the f32 dG
    ("upper_wide_short", dict(T=12, Din=2048, needs_dx=True), True,
     (False, True, True, False, 8, "panels", True, "STREAM", False)),
    ("upper_wide_bucket", dict(WIDE, to_scratch=False), True, (True, True, True, True, 4, "panels", True, "STREAM", False)),
    ("not_deferrable", dict(can_defer=False), True, NARROW_PLAN),
    ("share_panels_off", dict(WIDE, share_env=False), True, (True, False, True, False, 8, "f32", False, "STREAM", False)),
    ("skip_dg_off", dict(skip_dg_switch=False), True, NARROW_PLAN[:3] + (False,) + NARROW_PLAN[4:]),
    ("three_batch_groups", dict(B=48), True, (False, True, False, False, 8, "panels_splitk", True, "STREAM", False)),
    # B % 16 != 0: no dG^T from the kernel, dW_hh multiplies panels split on the host; dW_ih = 8192 x 512 over 288 tokens
    # fails the routing rule (2MN / (M + N) = 964 < 1500) and stays one stacked f32 GEMM
    ("b24", dict(B=24, Din=512, needs_dx=True), True, (False, False, True, False, 8, "f32", True, "STREAM", False)),
    ("cfg2_bottom", dict(T=1000, H=512, stacked=False, beside_bptt=True), True,
     (False, False, True, False, 4, "f32", False, "SIDE_REVERSE", False)),
    ("cfg2_upper", dict(T=500, Din=2048, H=512, stacked=False, beside_bptt=True, needs_dx=True), True,
     (False, False, True, False, 4, "f32", False, "SIDE_ALL", False)),
    ("one_direction_bottom", dict(ndir=1, stacked=False), True,
     (False, True, True, True, 4, "panels_splitk", True, "SIDE_ALL", False)),
    # share0 needs T > 1: no shared panels, and the executor's dW_hh is the zero matrix
    ("t1", dict(T=1), True, (False, False, True, False, 4, "f32", False, "SIDE_REVERSE", False)),
    ("no_bias", dict(has_bias=False), True, NARROW_PLAN[:2] + (False,) + NARROW_PLAN[3:]),
]


def plan_of(ops, L, facts, available):
    f = dict(BASE, **facts)
    asked = []

    def take_panel(rows, K):
        asked.append((rows, K))
        return PANEL if available else None

    p = ops.lstm_bwd_plan(takes_split=lambda M, N, K: bool(L.asrk_gemm_takes_split(M, N, K, AUTO)),
                          take_panel=take_panel, **f)
    return f, p, asked


@pytest.mark.parametrize("name,facts,available,want", ROWS, ids=[r[0] for r in ROWS])
def test_row_gets_the_plan_it_names(ops, L, name, facts, available, want):
    f, p, asked = plan_of(ops, L, facts, available)
    H, M = f["H"], f["T"] * f["B"]
    got = (p.pG is not None, p.pGT is not None, p.db_in_kernel, p.skip_dg, p.rows_ih // H, p.dw_ih_route, p.dw_hh_panels,
           p.schedule, p.defer_release)
    assert got == want, p
    assert p.rows_ih in (4 * H, 8 * H) and all(x in (None, PANEL) for x in (p.pG, p.pGT))
    # the pool is asked in a fixed order, the dG panel before the dG^T panel, and only for what a row could use
    assert asked == [s for s in ((M, 8 * H), (f["ndir"] * 4 * H, M)) if s in asked]
    if available:
        assert asked == [(M, 8 * H)] * want[0] + [(f["ndir"] * 4 * H, M)] * want[1]
    # the record is one plan: its parts agree
    assert not p.skip_dg or p.pGT is not None
    assert p.dw_ih_route != "panels_splitk" or (p.pGT is not None and p.dw_hh_panels)
    assert p.dw_ih_route == "f32" or p.dw_hh_panels
    assert not p.defer_release or p.schedule == "SIDE_REVERSE_SHARED"
    assert (p.schedule == "SIDE_REVERSE_SHARED") <= (p.pGT is not None and not p.skip_dg)
    assert p.schedule != "SIDE_REVERSE" or (p.pGT is None and not p.dw_hh_panels and p.dw_ih_route == "f32")


def test_table_reaches_every_decision(ops, L):
    both = [plan_of(ops, L, facts, available)[:2] for _, facts, available, _ in ROWS]
    plans = [p for _, p in both]
    assert {p.schedule for p in plans} == {ops.STREAM, ops.SIDE_ALL, ops.SIDE_REVERSE_SHARED, ops.SIDE_REVERSE}
    assert {ops.STREAM, ops.SIDE_ALL, ops.SIDE_REVERSE_SHARED, ops.SIDE_REVERSE} == {"STREAM", "SIDE_ALL",
                                                                                     "SIDE_REVERSE_SHARED", "SIDE_REVERSE"}
    routes = {(p.dw_ih_route, p.rows_ih // f["H"]) for f, p in both}          # every route, stacked and per direction
    assert routes == {(r, n) for r in (ops.IH_PANELS, ops.IH_SPLITK, ops.IH_F32) for n in (4, 8)}
    assert (ops.IH_PANELS, ops.IH_SPLITK, ops.IH_F32) == ("panels", "panels_splitk", "f32")
    for field in ("skip_dg", "db_in_kernel", "defer_release", "dw_hh_panels"):
        assert {getattr(p, field) for p in plans} == {False, True}, field
    assert {(p.pG is not None, p.pGT is not None) for p in plans} == {(a, b) for a in (False, True) for b in (False, True)}


def test_plan_is_a_function_of_its_facts(ops, L):
    """no tensor, stream, device or environment behind it: the same facts, the same record - and it is immutable"""
    for _, facts, available, _ in ROWS:
        a, b = plan_of(ops, L, facts, available)[1], plan_of(ops, L, facts, available)[1]
        assert a == b
    with pytest.raises(AttributeError):
        a.schedule = ops.STREAM
