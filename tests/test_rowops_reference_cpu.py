"""CPU: the float64 references of tests/rowops_reference.py against torch's own float64 ops on every case row, and the
conditions the exact checks of tests/test_rowops_variants_gpu.py rest on: every summed input is an integer k/8 small enough
that any float32 summation order gives the float64 sum, destinations do not overlap, the dropout inputs have no zeros."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rowops_reference as R
from oracle import regularizer_oracle as PH


# ====================================================================================================== copy3d
@pytest.mark.parametrize("case", R.COPY3D_CASES, ids=lambda c: c.name)
def test_copy3d_reference_is_torch_as_strided(case):
    c = case
    src, dst0, si, di = R.copy3d_buffers(c.name)
    assert np.unique(di).size == di.size                              # no destination element is written twice
    assert si.min() >= 0 and di.min() >= 0
    assert R.exactly_summable(src, 2) and R.exactly_summable(dst0[di.reshape(-1)], 2)
    assert np.isnan(np.delete(dst0, di.reshape(-1))).all()
    sview = torch.from_numpy(src).double().as_strided((c.n0, c.n1, c.n2), (c.ss0, c.ss1, 1), c.soff)
    for acc in (0, 1):
        want = torch.from_numpy(dst0.copy() if acc else np.full_like(dst0, np.nan)).double()
        dview = want.as_strided((c.n0, c.n1, c.n2), (c.ds0, c.ds1, 1), c.doff)
        if acc:
            dview += sview
        else:
            dview.copy_(sview)
        got = R.copy3d_expected(c.name, acc)
        assert np.array_equal(got.view(np.int32), want.float().numpy().view(np.int32)), (c.name, acc)
        assert np.isnan(got).sum() == got.size - di.size              # NaN exactly outside the addressed elements


# ====================================================================================================== colsum
@pytest.mark.parametrize("case", R.COLSUM_CASES, ids=lambda c: c.name)
def test_colsum_reference_and_exact_summability(case):
    c = case
    X = R.colsum_matrix(c.name)
    out0 = R.colsum_inputs(c.name)[1]
    assert c.M <= 8192 and R.exactly_summable(X, c.M + 1) and R.exactly_summable(out0, c.M + 1)
    for acc in (0, 1):
        want = torch.from_numpy(X).double().sum(0) + (torch.from_numpy(out0).double() if acc else 0.0)
        got = R.colsum_expected(c.name, acc)
        assert np.array_equal(got.astype(np.float64), want.numpy())   # the float32 result IS the float64 sum
    # float32 sums in two very different orders give the same bits: what `exact` means
    assert np.array_equal(X.sum(0, dtype=np.float32), X[::-1].cumsum(0, dtype=np.float32)[-1])
    if c.N > 1:                                                       # distinct columns: a misplaced sum shows
        s = R.colsum_expected(c.name, 0)
        assert np.unique(s).size > min(c.N, 25) // 2
        assert (s[:-1] != s[1:]).mean() > 0.9                         # neighbours (a lane's other columns) differ


# ====================================================================================================== LayerNorm
@pytest.mark.parametrize("case", R.LN_CASES, ids=lambda c: c.name)
def test_layer_norm_reference_against_torch_float64(case):
    c = case
    x, w, b, dy = R.ln_inputs(c.name)
    ref = R.ln_expected(c.name)
    x64 = x.double().requires_grad_(True)
    w64, b64 = w.double().requires_grad_(True), b.double().requires_grad_(True)
    y = F.layer_norm(x64, (c.D,), w64, b64, R.ln_eps(c))
    dx, dw, db = torch.autograd.grad(y, (x64, w64, b64), dy.double())
    t64 = R.ln_torch(c.name, torch.float64)
    # relative to the tensor, or (where the tensor is 0 by cancellation: D = 1) to the terms that cancel
    scale = float(ref['rstd'].max() * dy.abs().max() * w.abs().max()) * c.rows
    for k, v in dict(y=y.detach(), dx=dx, dw=dw, db=db).items():
        err = float(np.abs(ref[k] - v.numpy()).max())
        assert err <= 1e-12 * max(float(np.abs(ref[k]).max()), scale), (c.name, k, err)
    for k in ('mean', 'rstd'):
        assert R.rel_err(ref[k], t64[k]) < 1e-12, (c.name, k)
    assert all(np.isfinite(v).all() for v in ref.values())
    if c.kind == 'const_row':
        assert ref['rstd'][R.CONST_ROW] == 1.0 / np.sqrt(R.ln_eps(c))  # variance exactly 0
        assert np.array_equal(ref['y'][R.CONST_ROW], b.double().numpy())
    if c.kind == 'mean1000':
        assert abs(ref['mean'].mean() - 1000) < 1 and 0.5 < ref['rstd'].mean() < 2
    if c.kind == 'int_dy':
        assert R.exactly_summable(dy.numpy(), c.rows)
        assert np.array_equal(ref['db'], ref['db'].astype(np.float32).astype(np.float64))
    if c.eps == 0:
        assert x.var(1, unbiased=False).min() > 1e-3                  # eps = 0 on non-constant rows only


# ====================================================================================================== dropout
def test_philox_known_answers_and_the_large_sizes():
    for ctr, key, want in PH.KAT:
        assert tuple(int(v) for v in PH.philox4x32_10(np.array([ctr], np.uint32), key)[0]) == want
    n = R.DROP_SIZES[0][1]
    x = R.dropout_input(n)
    assert (x != 0).all() and R.exactly_summable(x, 1)
    y = R.dropout_expected(x, 0.5, 0x1234567887654321, 2 ** 32 + 5)   # the oracle handles the grid-stride sizes whole
    assert 0.49 < (y == 0).mean() < 0.51 and np.array_equal(y[y != 0], x[y != 0] * 2)
    assert not np.array_equal(y[:4096], R.dropout_expected(x[:4096], 0.5, 0x1234567887654321, 5))    # offset's high word counts
    for name, p in R.DROP_P:
        thresh = int(np.rint(np.float32(p) * np.float32(16777216.0)))
        assert 0 <= thresh < 2 ** 24
        assert (name == 'thresh0') == (thresh == 0) and (name == 'almost_one') == (thresh == 2 ** 24 - 1)
    assert np.array_equal(R.dropout_expected(x[:1000], 1e-9, 7), x[:1000])                           # thresh 0: identity


# ====================================================================================================== optimisers
@pytest.mark.parametrize("coef", [c for _, c in R.OPT_COEFS], ids=[n for n, _ in R.OPT_COEFS])
@pytest.mark.parametrize("kind", ['adadelta', 'adam'])
def test_optimiser_recurrences_against_torch_optim_float64(kind, coef):
    p0, grads = R.opt_inputs(1027, 11)
    ref = (R.adadelta_reference(p0, grads, coef, **R.ADADELTA_HP) if kind == 'adadelta'
           else R.adam_reference(p0, grads, coef, **R.ADAM_HP))
    assert len(ref) == R.OPT_STEPS
    if coef is not None and coef != coef:                            # the NaN rule: nothing moves
        for p, s0, s1 in ref:
            assert np.array_equal(p, p0.astype(np.float64)) and not s0.any() and not s1.any()
        return
    want = R.torch_optim_run(kind, p0, grads, coef, torch.float64)
    for step, (a, b) in enumerate(zip(ref, want)):
        for i in range(3):
            assert R.rel_err(a[i], b[i]) < 1e-12, (kind, coef, step, R.OPT_KINDS[i])
    if coef is not None and coef > 1:                                # min(coef, 1): the same as no clipping
        none = (R.adadelta_reference(p0, grads, None, **R.ADADELTA_HP) if kind == 'adadelta'
                else R.adam_reference(p0, grads, None, **R.ADAM_HP))
        assert all(np.array_equal(a[i], b[i]) for a, b in zip(ref, none) for i in range(3))
    e32 = R.opt_e32(kind, 1027, 11, coef)
    assert all(0 < e < R.OPT_HARD for e in e32), e32                  # the float32 CPU run itself is inside the hard limit


def test_tables_and_gradient_norm_exactness():
    assert [len(v) for k, v in R.TABLES.items() if k[0] == 'n'] == [23, 24, 25, 49]
    for name, sizes in R.TABLES.items():
        live = [n for n in sizes if n > 0]
        assert 1 in sizes, name
        if name[0] == 'n':
            assert len(live) == len(sizes)                           # 23 / 24 / 25 / 49 table slots in use
        if name[0] == 'e':
            assert all(sizes[t] == 0 for t in (0, 23, 24, len(sizes) - 1) if t < len(sizes))
        grads = R.grad_norm_inputs(sizes, 5)
        # float32 per thread: at most norm_thread_elems squares of at most KMAX^2 / 64; double beyond
        for g, n in zip(grads, sizes):
            assert R.exactly_summable(g, 1) and (n == 0 or R.norm_thread_elems(n) * R.KMAX ** 2 < 2 ** 24)
        units, s = R.grad_norm_exact(grads)
        assert units < 2 ** 53 and s * 64 == units
        norm, coef = R.grad_norm_expected(grads, 5.0)
        assert abs(float(norm) - R.grad_norm_float64(grads)) <= 2.0 ** -24 * float(norm)
        t = torch.cat([torch.from_numpy(g).double() for g in grads])
        assert abs(float(t.norm()) - R.grad_norm_float64(grads)) < 1e-9 * float(norm)
        assert coef == np.float32(5.0) / (norm + np.float32(1e-6))
    sizes = R.TABLES['gap_at_edge26']
    assert all(n > 0 for n in sizes[:24]) and sizes[24] == 0 and sizes[25] > 0
    assert R.TABLES['tail_empty26'][24:] == [0, 0] and all(n > 0 for n in R.TABLES['tail_empty26'][:24])
    big = [max(v) for v in R.TABLES.values() if max(v) >= R.BIG]
    assert len(big) == 2 and R.BIG > R.STEP_CAP and R.norm_blocks_of(R.BIG) == 1024 and R.norm_thread_elems(R.BIG) == 9
    assert R.norm_blocks_of(1) == 1 and R.norm_blocks_of(2049) == 2
