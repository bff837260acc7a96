"""CPU: every row of the convolution case table (tests/conv_reference.py) gets the plan it names - asked of the library
itself through asrk_conv3x3_plan_info, which reads fwd_plan / wgrad_plan / wgrad_groups / first_plan of
csrc/conv3x3.hip (host only) - and the table as a whole reaches every property the GPU test is there for.  A re-tune of
wgrad_lds, the 80-KB budget, the cost model or the tile size that takes a property out of the GPU tests' reach fails here:
then move the SHAPE, not the assertion."""
import ctypes
import importlib
import itertools

import pytest

from conftest import PKG_NAME
import conv_reference as R

MOVE = "a re-tune took this property out of the table's reach: move the shape, not the assertion"


@pytest.fixture(scope="module")
def L():
    importlib.import_module(PKG_NAME + ".build").build(verbose=False)
    return importlib.import_module(PKG_NAME + "._lib").load()


def plan(L, kind, B, H, W, C, Cout):
    out = (ctypes.c_int * R.PLAN_LEN)()
    assert L.asrk_conv3x3_plan_info(kind, B, H, W, C, Cout, out, R.PLAN_LEN) == 0
    return dict(zip(R.PLAN_FIELDS, out))


@pytest.fixture(scope="module")
def plans(L):
    """row name -> launch family -> record"""
    return {c.name: {fam: plan(L, *q) for fam, q in R.plan_queries(c).items()} for c in R.CASES}


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_row_gets_the_plan_it_names(L, plans, case):
    c, got = case, plans[case.name]
    assert set(c.plan) <= set(got), "the row names a launch family its geometry does not have"
    for fam, want in c.plan.items():
        for field, v in want.items():
            assert got[fam][field] == v, "%s %s: %s is %d, the row is there for %d - %s" % (
                c.name, fam, field, got[fam][field], v, MOVE)
    # the route the row names is the route its geometry and knobs lead to (the GPU test asks Geom on the device too)
    knobs = dict(c.env)
    direct_on = knobs.get('ASRK_CONV_DIRECT', '1') != '0'
    is3 = (c.k, c.s, c.p) == ((3, 3), (1, 1), (1, 1))
    direct = direct_on and is3 and c.layout == 'cl' and bool(L.asrk_conv3x3_supported(c.H, c.W, c.C, c.Cout))
    first = direct_on and is3 and bool(L.asrk_conv3x3_first_supported(c.H, c.W, c.C, c.Cout))
    sb, sh, sw, sc = R.strides(c)
    cl = knobs.get('ASRK_CONV_CL', '1') != '0' and sc == 1 and c.C % 4 == 0 and sb % 4 == sh % 4 == sw % 4 == 0
    route = 'direct' if direct else 'first' if first else 'im2col_cl' if cl else 'im2col_ld'
    assert route == c.route, MOVE
    for fam, p in got.items():
        # the record is one plan: its parts add up
        assert p['supported'] == 1 or c.route.startswith('im2col')
        if not p['supported']:
            assert all(v == 0 for v in p.values())
            continue
        assert p['ntiles'] == c.B * p['tiles_img'] and 0 < p['lds'] <= 158 * 1024
        assert p['fewest'] <= p['most'] and p['fewest'] * p['gx'] <= p['ntiles'] <= p['most'] * p['gx']
        if fam == 'wgrad':
            assert p['TH'] <= p['thmax'] and p['tiles_img'] == -(-c.H // p['TH']) and p['gx'] <= p['ntiles']
            assert p['most'] == -(-p['ntiles'] // p['gx']) and p['ws'] > 0
            assert p['gy'] == (c.Cout // 64 if c.C <= 3 else (c.C // 64) * (c.Cout // 64))
        else:
            assert p['gx'] == p['ntiles'] and p['most'] == p['fewest'] == 1 and p['ws'] == 0
            assert p['tiles_img'] == (-(-c.H // p['TH']) if c.C <= 3 else -(-c.H * c.W // 128))


def test_workspace_functions_equal_the_report(L, plans):
    n = 0
    for c in R.CASES:
        q = R.plan_queries(c)
        if 'wgrad' in q:
            fn = L.asrk_conv3x3_first_wgrad_ws_bytes if q['wgrad'][0] == 3 else L.asrk_conv3x3_wgrad_ws_bytes
            assert int(fn(*q['wgrad'][1:])) == plans[c.name]['wgrad']['ws'], c.name
            n += plans[c.name]['wgrad']['ws'] > 0
    assert n >= 20
    # B == 0 launches nothing and needs nothing
    assert L.asrk_conv3x3_wgrad_ws_bytes(0, 7, 40, 64, 64) == 0 == plan(L, 1, 0, 7, 40, 64, 64)['ws']
    assert L.asrk_conv3x3_first_wgrad_ws_bytes(0, 7, 40, 3, 64) == 0 == plan(L, 3, 0, 7, 40, 3, 64)['ws']
    assert plan(L, 1, 0, 7, 40, 64, 64)['supported'] == 1 and plan(L, 1, 0, 7, 40, 64, 64)['gx'] == 0


def test_report_refuses_what_supported_refuses(L):
    for H, W, C, Cout in itertools.product((1, 7, 400), (1, 40, 127, 128, 129, 200), (1, 3, 4, 32, 64, 128, 192, 256),
                                           (1, 32, 64, 128, 192, 256)):
        for kind in (0, 1):
            assert plan(L, kind, 2, H, W, C, Cout)['supported'] == L.asrk_conv3x3_supported(H, W, C, Cout), (H, W, C, Cout)
        for kind in (2, 3):
            assert plan(L, kind, 2, H, W, C, Cout)['supported'] == L.asrk_conv3x3_first_supported(H, W, C, Cout)
    assert L.asrk_conv3x3_supported(3, 128, 64, 64) == 1 and L.asrk_conv3x3_supported(3, 129, 64, 64) == 0
    assert L.asrk_conv3x3_first_supported(3, 128, 3, 64) == 1 and L.asrk_conv3x3_first_supported(3, 128, 4, 64) == 0


def test_table_reaches_every_property(plans):
    P = lambda c, fam: plans[c.name][fam]
    train = [c for c in R.TRAIN_CASES]
    direct = [c for c in train if c.route == 'direct']
    assert direct and all(c.B >= 2 for c in direct), MOVE
    ragged = lambda c: c.H * c.W > 128 and (c.H * c.W) % 128 != 0
    # ---- forward / data gradient tiles: 128 consecutive positions
    for W in (1, 2, 3, 6, 13, 20, 33, 40, 64, 65, 100, 127):
        assert any(c.W == W and ragged(c) and P(c, 'fwd')['tiles_img'] >= 2 for c in direct), (W, MOVE)
    assert any(c.W == 128 and P(c, 'fwd')['tiles_img'] >= 2 for c in direct), MOVE
    assert any(c.H * c.W < 128 for c in direct) and any(c.H == 1 for c in direct), MOVE
    assert any(c.H * c.W > 128 and (c.H * c.W) % 128 == 0 for c in direct), MOVE
    ths = {P(c, 'fwd')['TH'] for c in direct}
    assert {1, 2, 3} <= ths and len([t for t in ths if t >= 4]) >= 3, (ths, MOVE)
    for pair in ((64, 128), (128, 128), (128, 64)):
        assert any((c.C, c.Cout) == pair and c.relu and 13 <= c.W <= 40 and c.grads == 'xwb' for c in direct), (pair, MOVE)
    assert any(not c.relu for c in direct) and any(c.grads == 'b' for c in direct), MOVE
    assert all(P(c, 'dgrad')['TH'] == P(c, 'fwd')['TH'] for c in direct)
    over = [c for c in train if c.W == 129 and (c.k, c.s, c.p) == ((3, 3), (1, 1), (1, 1)) and c.C == 64]
    assert over and all(c.route == 'im2col_cl' and P(c, 'fwd')['supported'] == 0 for c in over), MOVE
    # ---- the weight gradient's tile walk
    for splits in (1, 2, 4):
        assert any(P(c, 'wgrad')['gy'] == splits and P(c, 'wgrad')['most'] >= 2
                   and P(c, 'wgrad')['fewest'] < P(c, 'wgrad')['most'] for c in direct), (splits, MOVE)
    wg = [P(c, 'wgrad') for c in direct]
    assert any(p['most'] == p['fewest'] == 2 for p in wg), MOVE
    assert any(c.H % P(c, 'wgrad')['TH'] and P(c, 'wgrad')['tiles_img'] >= 2 for c in direct), MOVE
    assert any(p['TH'] < p['thmax'] and p['most'] >= 2 for p in wg), MOVE
    assert any(c.H % P(c, 'wgrad')['TH'] and 1 < P(c, 'wgrad')['TH'] == P(c, 'wgrad')['thmax'] for c in direct), MOVE
    big = [c for c in direct if c.W == 128]
    assert big and all(P(c, 'wgrad')['TH'] == 1 for c in big), MOVE
    assert max(p['lds'] for p in wg) == max(P(c, 'wgrad')['lds'] for c in big) > 140000, MOVE
    assert any(c.W == 1 for c in direct), MOVE
    assert all(c in R.REPEAT for c in direct if P(c, 'wgrad')['most'] >= 2)
    # ---- the first layer
    first = [c for c in train if c.route == 'first']
    assert {(c.C, c.Cout, c.layout) for c in first} >= set(itertools.product((1, 2, 3), (64, 128), ('cl', 'btcf'))), MOVE
    assert {P(c, 'fwd')['gy'] for c in first} == {1, 2}
    for W, th in ((40, 3), (64, 2), (65, 1), (128, 1)):
        assert any(c.W == W and P(c, 'fwd')['TH'] == th == P(c, 'wgrad')['TH'] for c in first), (W, MOVE)
    assert any(c.W == 13 and c.H * c.W < 128 and P(c, 'fwd')['TH'] == c.H for c in first), MOVE
    assert any(c.H % P(c, 'fwd')['TH'] for c in first), MOVE
    assert any(P(c, 'wgrad')['most'] >= 2 and P(c, 'wgrad')['fewest'] < P(c, 'wgrad')['most'] for c in first), MOVE
    ld = {c.name: c for c in train if c.route == 'im2col_ld' and dict(c.env).get('ASRK_CONV_DIRECT') == '0'}
    for c in first:
        if c.name != 'f_walk':
            t = ld[c.name + '_ld']
            assert t._replace(name=c.name, route='first', env=(), plan=c.plan, why=c.why) == c
    assert {(9 * c.C, (9 * c.C + 3) // 4 * 4) for c in ld.values()} == {(9, 12), (18, 20), (27, 28)}
    # ---- the generic route
    gen = [c for c in train if (c.k, c.s, c.p) != ((3, 3), (1, 1), (1, 1))]
    assert any(c.k == (5, 5) and c.s == (3, 3) and c.p == (2, 2) for c in gen)
    unc = [c for c in gen if c.k == (2, 2) and c.s == (3, 3) and c.p == (0, 0)]
    assert {(c.route, dict(c.env).get('ASRK_CONV_CL')) for c in unc} == {('im2col_cl', None), ('im2col_ld', '0')}
    assert all(c.C % 4 == 0 and c.name in R.UNCOVERED for c in unc)
    assert any(R.out_hw(c) == (1, 1) and c.k == (c.H + 2 * c.p[0], c.W + 2 * c.p[1]) for c in gen)
    assert any(c.layout == 'cnn' and c.k == (4, 1) and c.s == (2, 1) and c.p == (1, 0) and c.H % 2 for c in gen)
    # ---- length-aware inference
    assert {c.route for c in R.LEN_CASES} == {'direct', 'first', 'im2col_cl', 'im2col_ld'}
    for c in R.LEN_CASES:
        assert c.B == 5 and c.hlen[0] == c.H and c.hlen[3] == 0 and c.hlen[4] == 1
        if c.W > 1:
            assert (c.hlen[1] * c.W) % 128 != 0 and (c.hlen[2] * c.W) % 128 == 0 and 0 < c.hlen[2] < c.H
    assert {c.route for c in R.LEN_CASES if R.out_hlen_of(c) is not None} == {'im2col_cl', 'im2col_ld'}
    assert {c.route for c in R.LEN_CASES if dict(c.env)} == {'im2col_cl', 'im2col_ld'}
    # ---- partial gradient requests: one direct and one first-layer row, strided
    assert [R.BY_NAME[n].route for n in R.PARTIAL_BASES] == ['direct', 'first']


def test_table_rows_are_small_and_distinct():
    assert len({c.name for c in R.CASES}) == len(R.CASES)
    for c in R.CASES:
        Ho, Wo = R.out_hw(c)
        assert max(c.B * c.H * c.W * c.C, c.B * Ho * Wo * c.Cout) * 4 <= 11e6, c.name
