"""CPU: every row of the attention energy case table (tests/attention_reference.py) has the launch geometry it names -
asked of the library itself through asrk_attn_energy_plan, the host function both energy launchers take their frames per
workgroup, grid and LDS size from - and the tables as a whole reach every branch the GPU test is there for.  A re-tune
of energy_tpb or of the LDS budget that takes a property out of the GPU test's reach fails here: then move the SHAPE,
not the assertion."""
import ctypes
import importlib

import pytest

from conftest import PKG_NAME
import attention_reference as R

MOVE = "a re-tune took this property out of the table's reach: move the shape, not the assertion"


@pytest.fixture(scope="module")
def L():
    importlib.import_module(PKG_NAME + ".build").build(verbose=False)
    return importlib.import_module(PKG_NAME + "._lib").load()


def plan(L, loc, bwd, BN, T, A, K):
    """-> (status, tpb, chunks, lds bytes)"""
    tpb, chunks, lds = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_int64(-7)
    rc = L.asrk_attn_energy_plan(loc, bwd, BN, T, A, K, ctypes.byref(tpb), ctypes.byref(chunks), ctypes.byref(lds))
    return rc, tpb.value, chunks.value, lds.value


@pytest.mark.parametrize("case", R.ENERGY_CASES, ids=lambda c: c.name)
def test_row_has_the_geometry_it_names(L, case):
    c = case
    BN = c.B * c.N
    rc, tpb, chunks, lds = plan(L, c.loc, 0, BN, c.T, c.A, c.K)
    assert (rc, (tpb, chunks)) == (0, c.fwd), "%s forward: %s, the row is there for %s - %s" % (c.name, (tpb, chunks), c.fwd, MOVE)
    assert lds == 4 * (2 * c.A + c.A * c.K + tpb * c.K if c.loc else c.A)
    assert chunks == -(-c.T // tpb) and 0 < lds <= 150 * 1024
    rc, btpb, bchunks, blds = plan(L, c.loc, 1, BN, c.T, c.A, c.K)
    if c.bwd is None:
        assert (rc, btpb, bchunks, blds) == (-2, 0, 0, 0), (c.name, MOVE)
    else:
        assert (rc, (btpb, bchunks)) == (0, c.bwd), "%s backward: %s, the row is there for %s - %s" % (
            c.name, (btpb, bchunks), c.bwd, MOVE)
        floats = 5 * c.A + (5 * c.A + 5 * c.A * c.K + btpb * c.K if c.loc else 0)
        assert blds == 4 * floats <= 150 * 1024 and bchunks == -(-c.T // btpb)
        if c.bwd != c.fwd:       # shrunk: the unshrunk size did not fit, and the halving went 20 -> 10
            assert 4 * (floats + (tpb - btpb) * c.K) > 150 * 1024 and btpb == (tpb + 1) // 2
    # the lengths the row promises
    assert len(c.lens) == c.B
    if c.B >= 5:
        for t in {tpb, btpb} - {0}:
            assert c.T in c.lens and 1 in c.lens and any(v > c.T for v in c.lens), c.name
            inside = [v for v in c.lens if 1 < v < c.T]
            if chunks > 1:
                assert any(v % t == 0 for v in inside) and any(v % t == 1 and v - 1 in c.lens for v in inside), (c.name, t)
    # size limit of the GPU test: no tensor above 64 MB
    assert BN * c.T * c.A * 4 <= 64e6


def test_shrink_row_is_shrunk_from_20_to_10(L):
    c = R.ENERGY_BY_NAME['l_shrink']
    assert (c.fwd, c.bwd) == ((20, 8), (10, 16))
    assert plan(L, 1, 0, c.B * c.N, c.T, c.A, c.K)[1] == 20 and plan(L, 1, 1, c.B * c.N, c.T, c.A, c.K)[1] == 10
    d = R.ENERGY_BY_NAME['d_a424_no_shrink']
    assert (d.B, d.N, d.T, d.A) == (c.B, c.N, c.T, c.A) and d.bwd == (20, 8)


@pytest.mark.parametrize("args,status,why", R.ENERGY_REFUSED, ids=[r[2] for r in R.ENERGY_REFUSED])
def test_refused_geometry(L, args, status, why):
    assert plan(L, *args) == (status, 0, 0, 0)


def test_argument_checks_and_empty_batch(L):
    i, j, k = ctypes.c_int(5), ctypes.c_int(5), ctypes.c_int64(5)
    assert L.asrk_attn_energy_plan(1, 0, 4, 8, 20, 3, None, ctypes.byref(j), ctypes.byref(k)) == -1
    assert (j.value, k.value) == (0, 0)
    assert L.asrk_attn_energy_plan(1, 0, 4, 8, 20, 3, ctypes.byref(i), None, ctypes.byref(k)) == -1
    assert L.asrk_attn_energy_plan(1, 0, 4, 8, 20, 3, ctypes.byref(i), ctypes.byref(j), None) == -1
    # BN == 0 launches nothing: OK before K is looked at, as in the launchers (B == 0)
    assert plan(L, 1, 1, 0, 8, 20, 17) == (0, 0, 0, 0) and plan(L, 1, 0, 0, 8, 20, 0) == (0, 0, 0, 0)
    # dot energies ignore K
    assert plan(L, 0, 1, 4, 8, 20, 99) == plan(L, 0, 1, 4, 8, 20, 0) == (0, 8, 1, 4 * 5 * 20)
    # K = 16 is the last width the loc backward takes; the forward takes 17
    assert plan(L, 1, 1, 5, 9, 20, 16)[0] == 0 and plan(L, 1, 1, 5, 9, 20, 17)[0] == -2 and plan(L, 1, 0, 5, 9, 20, 17)[0] == 0
    # the null-pointer and temperature checks of the launchers come before any device call
    z = ctypes.c_void_p(0)
    p = ctypes.c_void_p(4096)
    assert L.asrk_attn_energy_fwd_f32(0, p, p, z, z, z, z, p, p, p, 2, 1, 8, 20, 0, 0.0, z) == -1
    assert L.asrk_attn_energy_fwd_f32(0, z, p, z, z, z, z, p, p, p, 2, 1, 8, 20, 0, 1.0, z) == -1
    assert L.asrk_attn_energy_fwd_f32(1, p, p, p, p, p, p, p, p, p, 1, 4, 8, 2400, 16, 1.0, z) == -2
    assert L.asrk_attn_energy_bwd_f32(1, p, p, p, p, p, p, p, p, p, p, p, p, p, p, 5, 1, 9, 20, 17, 1.0, z) == -2
    assert L.asrk_attn_energy_bwd_f32(1, p, p, p, p, p, p, p, p, p, p, p, p, p, p, 4, 1, 8, 430, 16, 1.0, z) == -2
    assert L.asrk_attn_energy_bwd_f32(1, p, p, p, p, p, p, p, p, p, p, p, p, p, p, 0, 1, 8, 430, 16, 1.0, z) == 0


def test_tables_reach_every_branch(L):
    for loc in (1, 0):
        rows = [c for c in R.ENERGY_CASES if c.loc == loc]
        assert {1, 63, 64, 65, 257, 300} <= {c.A for c in rows}, MOVE
        assert {1, 2, 4} <= {c.N for c in rows} and {0.5, 1.0, 2.0} <= {c.temp for c in rows}
        assert {5, 7, 8, 20} <= {c.fwd[0] for c in rows}, MOVE
        assert any(c.B * c.N == 1 and c.T == 9 and c.fwd == (5, 2) for c in rows), MOVE
        assert any(c.T == 200 and c.fwd == (8, 25) for c in rows), MOVE
        assert any(c.B * c.N >= 1024 and c.fwd == (c.T, 1) for c in rows), MOVE
        assert any(c.T % c.fwd[0] for c in rows if c.fwd[1] > 1), MOVE
        assert sum(c.softmax for c in rows) == 1
        assert len(rows) <= 25
    loc = [c for c in R.ENERGY_CASES if c.loc]
    assert {1, 10, 16} <= {c.K for c in loc if c.bwd is not None}
    assert any(c.K == 17 and c.bwd is None for c in loc)
    assert any(c.bwd not in (None, c.fwd) for c in loc), MOVE
    assert any(c.A > 512 for c in R.ENERGY_CASES if not c.loc)
    assert len({c.name for c in R.ENERGY_CASES}) == len(R.ENERGY_CASES)
    # location convolution: 64-frame tiles, 4 waves over channels / heads, 256 threads over taps
    cv = R.CONV_CASES
    assert {1, 63, 64, 65, 130} <= {c.T for c in cv} and {0, 3, 100, 130} <= {c.ks for c in cv}
    assert {1, 3, 4, 5, 10, 16} <= {c.K for c in cv} and {1, 2, 4, 5} <= {c.N for c in cv} and {1, 3} <= {c.B for c in cv}
    assert any(c.ks > c.T for c in cv) and any(2 * c.ks + 1 > 256 for c in cv)
    assert {c.skip for c in cv} == {'', 'dprev', 'dWc'}
    for c in cv:
        assert c.N * (64 + 2 * c.ks) * 4 <= 60 * 1024 and ((64 + 2 * c.ks) * c.K + 4 * c.N * 64) * 4 <= 60 * 1024, c.name
    # context: 256-thread tiles over Dv
    cx = R.CTX_CASES
    assert {1, 255, 256, 257, 600} <= {c.Dv for c in cx} and {1, 3, 5, 257} <= {c.T for c in cx}
    assert {1, 6} <= {c.BN for c in cx} and {0, 24} <= {c.pad for c in cx}
    assert any(c.pad and c.Dv > 256 for c in cx) and all(c.T * 4 <= 60 * 1024 for c in cx)
    assert R.CELL_SHAPES == [(3, 5), (1, 256), (7, 37), (128, 64)]
    assert R.EMB_SHAPES == [(1, 1, 1), (7, 300, 31), (130, 10, 5), (513, 33, 1031)]
    assert [(c.loc, c.N) for c in R.CHAIN_CASES] == [(1, 1), (1, 2), (1, 4), (0, 1), (0, 4)]
    s = R.CHAIN
    assert (s['B'], s['T'], s['lens'], s['A'], s['Dv'], s['K'], s['ks'], s['temp']) == (3, 70, (70, 33, 1), 20, 40, 3, 4, 0.7)
