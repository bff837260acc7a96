"""CPU: every CTC row of tests/loss_reference.py gets the launch plan it names - asked of the library itself through
asrk_ctc_loss_plan_info, which reads the ctc_plan() both launchers of csrc/ctc.hip read (host only) - and the table as a
whole reaches every lattice instantiation, both FAST values and the edges of the gradient kernel's time chunks.  A change
of the dispatch that takes a row off its route fails here: then move the SHAPE, not the assertion."""
import ctypes
import importlib

import pytest

from conftest import PKG_NAME
import loss_reference as R

MOVE = "the dispatch moved this row to another route: move the shape, not the assertion"
EINVAL, ESHAPE = -1, -2


@pytest.fixture(scope="module")
def L():
    importlib.import_module(PKG_NAME + ".build").build(verbose=False)
    return importlib.import_module(PKG_NAME + "._lib").load()


def plan(L, T, B, Lmax):
    out = (ctypes.c_int * R.PLAN_LEN)()
    assert L.asrk_ctc_loss_plan_info(T, B, Lmax, out, R.PLAN_LEN) == 0
    return dict(zip(R.PLAN_FIELDS, out))


def expected_plan(T, B, Lmax):
    """the dispatch as include/asrk.h documents it"""
    smax = 2 * Lmax + 1
    tmpl = 4 if smax <= 256 else 16 if smax <= 1024 else 32
    p = dict(tmpl=tmpl, fast=int(tmpl == 4 and T <= 512), spl=-(-smax // 64), gather_y=0, t_per_block=0, tchunks=0,
             dense_grid=0, smax=smax)
    if B > 0:
        p['gather_y'] = -(-T // 8)
    if B > 0 and T > 0:
        chunks = max(1, min(-(-512 // B), -(-T // 4)))
        p['t_per_block'] = -(-(-(-T // chunks)) // 4) * 4
        p['tchunks'] = -(-T // p['t_per_block'])
        p['dense_grid'] = -(-T * B // 4)
    return p


@pytest.mark.parametrize("case", R.ALL_CTC, ids=lambda c: c.name)
def test_row_gets_the_plan_it_names(L, case):
    c = case
    got = plan(L, c.T, c.B, c.Lmax)
    assert (got['tmpl'], bool(got['fast'])) == c.route, "%s: %r - %s" % (c.name, got, MOVE)
    for field, v in c.plan.items():
        assert got[field] == v, "%s: %s is %d, the row is there for %d - %s" % (c.name, field, got[field], v, MOVE)
    assert got == expected_plan(c.T, c.B, c.Lmax)
    # the record is one plan: its parts add up
    assert got['spl'] <= got['tmpl'] and (got['spl'] - 1) * 64 < got['smax'] <= got['spl'] * 64
    assert got['t_per_block'] % 4 == 0
    assert got['t_per_block'] * (got['tchunks'] - 1) < c.T <= got['t_per_block'] * got['tchunks']
    assert (got['gather_y'] - 1) * 8 < c.T <= got['gather_y'] * 8
    assert (got['dense_grid'] - 1) * 4 < c.T * c.B <= got['dense_grid'] * 4


def test_table_reaches_every_instantiation(L):
    routes = {c.route for c in R.CTC_CASES}
    assert routes == {(4, True), (4, False), (16, False), (32, False)}, MOVE
    by = R.CTC_BY_NAME
    # both sides of every boundary of the dispatch
    assert by['l127'].route == (4, True) and by['l128'].route == (16, False)
    assert by['l511'].route == (16, False) and by['l512'].route == (32, False)
    assert by['t512_l3'].route == (4, True) and by['t513_l3'].route == (4, False)
    assert plan(L, by['l127'].T, 3, 127)['spl'] + 1 == plan(L, by['l128'].T, 3, 128)['spl']
    assert plan(L, by['l511'].T, 3, 511)['spl'] + 1 == plan(L, by['l512'].T, 3, 512)['spl']
    # whole lanes without a state: an utterance of length 2 has 5 states, a lane holds spl of them
    for name in ('l127', 'l128', 'l511', 'l512'):
        c = by[name]
        spl = plan(L, c.T, c.B, c.Lmax)['spl']
        lanes = [-(-(2 * min(t, c.Lmax) + 1) // spl) for t in c.tg_len]
        assert min(lanes) <= 2 and max(lanes) >= 52, (name, lanes)      # 257 states at 5 per lane fill 52 lanes


def test_table_reaches_the_edges_of_the_time_chunks(L):
    by = R.CTC_BY_NAME
    c = by['chunk_b1_t9']                              # chunks 4 / 4 / 1, the utterance ends inside the second
    p = plan(L, c.T, c.B, c.Lmax)
    assert (p['t_per_block'], p['tchunks']) == (4, 3) and p['t_per_block'] < c.in_len[0] < 2 * p['t_per_block']
    c = by['b600_t6']                                  # B > 512: one chunk
    p = plan(L, c.T, c.B, c.Lmax)
    assert c.B > 512 and p['tchunks'] == 1 and p['t_per_block'] >= c.T
    c = by['b601_t5']
    assert (c.T * c.B) % 4 != 0
    c = by['ring_edges']                               # T_b before, inside and at the end of a chunk
    p = plan(L, c.T, c.B, c.Lmax)
    assert p['tchunks'] > 1 and any(t % p['t_per_block'] for t in c.in_len) and any(t < p['t_per_block'] for t in c.in_len)
    chunky = [c for c in R.CTC_CASES if plan(L, c.T, c.B, c.Lmax)['tchunks'] > 1
              and any(t <= c.T - plan(L, c.T, c.B, c.Lmax)['t_per_block'] for t in c.in_len)]
    assert len(chunky) >= 3                            # workgroups whose whole chunk lies beyond T_b


def test_plan_info_sweep_against_the_documented_arithmetic(L):
    for T in (0, 1, 3, 4, 5, 8, 9, 17, 511, 512, 513, 1600):
        for B in (0, 1, 2, 7, 128, 511, 512, 513, 600):
            for Lmax in (0, 1, 31, 32, 127, 128, 511, 512, 1023):
                assert plan(L, T, B, Lmax) == expected_plan(T, B, Lmax), (T, B, Lmax)


def test_plan_info_argument_checks(L):
    n = R.PLAN_LEN
    out = (ctypes.c_int * (n + 2))(*([7] * (n + 2)))
    assert L.asrk_ctc_loss_plan_info(10, 2, 3, None, n) == EINVAL
    assert L.asrk_ctc_loss_plan_info(10, 2, 3, out, n - 1) == EINVAL and list(out) == [7] * (n + 2)
    for bad in ((-1, 2, 3), (10, -1, 3), (10, 2, -1)):
        out[:] = [7] * (n + 2)
        assert L.asrk_ctc_loss_plan_info(*bad, out, n) == EINVAL
        assert list(out) == [0] * n + [7, 7]           # zeroed first, nothing beyond n touched
    out[:] = [7] * (n + 2)
    assert L.asrk_ctc_loss_plan_info(10, 2, 1024, out, n) == ESHAPE and list(out)[:n] == [0] * n
    assert L.asrk_ctc_loss_plan_info(10, 2, 1023, out, n) == 0 and out[0] == 32 and out[2] == 32
