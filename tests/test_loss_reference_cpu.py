"""CPU: the float64 references of tests/loss_reference.py against torch's CPU ops in float64 (1e-10) on every row torch
accepts, the documented semantics asserted directly on the rows it rejects, and the input condition of every row: the
float32 CPU run of torch's op is off by e32 against its float64 run, and 4 * e32 stays inside the hard limit the GPU test
holds the kernel to, so that the reference's own rounding never decides a test."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_reference as R

TOL = 1e-10


def _close(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, what
    assert R.same_nonfinite(a, b), what
    assert R.finite_rel_err(a, b) <= TOL, (what, R.finite_rel_err(a, b))


# ------------------------------------------------------------------------------------------------ CTC
@pytest.mark.parametrize("case", R.CTC_CASES, ids=lambda c: c.name)
def test_ctc_reference_is_torch_in_float64(case):
    c = case
    out, grad = R.ctc_torch(c, R.F64)
    exp = R.ctc_expected(c)
    _close(exp['out'], out, c.name + ' loss')
    lp, tg, il, tl = R.ctc_inputs(c)
    for b in range(c.B):
        if c.name in R.TORCH_LAST_FRAME:
            # the last label is the blank: torch drops one of the two end states from the blank column of the last frame
            # (see the table); everything else is torch's, and that element is held to the definition below
            Tb, want, mine = c.in_len[b], grad[:, b].copy(), exp['grad'][:, b]
            assert abs(want[Tb - 1, c.blank] - mine[Tb - 1, c.blank]) > 1e-3
            want[Tb - 1, c.blank] = mine[Tb - 1, c.blank]
            _close(mine, want, '%s grad of utterance %d' % (c.name, b))
        elif np.isfinite(exp['grad'][:, b]).all():
            _close(exp['grad'][:, b], grad[:, b], '%s grad of utterance %d' % (c.name, b))
        else:
            # nll = +inf without zero_infinity: torch makes every element of the utterance's frames NaN; the library
            # keeps exp(lp) * gscale outside the label columns (ops.CTCLossFn), and so does the reference
            assert not c.zero_inf and exp['nll'][b] == np.inf
            Tb = min(c.in_len[b], c.T)
            assert np.isnan(grad[:Tb, b]).all() and (grad[Tb:, b] == 0).all()
            used = np.zeros(c.V, bool)
            used[c.blank] = True
            used[tg[b, :min(c.tg_len[b], c.Lmax)].numpy()] = True
            assert np.isnan(exp['grad'][:Tb, b][:, used]).all() and (exp['grad'][Tb:, b] == 0).all()
            want = np.exp(lp[:Tb, b].double().numpy()) * exp['gscale'][b]
            assert np.array_equal(exp['grad'][:Tb, b][:, ~used], want[:, ~used])


@pytest.mark.parametrize("case", [c for c in R.CTC_CASES if c.name.startswith('inf_')], ids=lambda c: c.name)
def test_ctc_infeasible_rows_are_what_they_claim(case):
    c = case
    exp = R.ctc_expected(c)
    assert tuple(b for b in range(c.B) if exp['nll'][b] == np.inf) == R.INFEASIBLE
    assert exp['nll'][0] == 0.0 and np.isfinite(exp['nll'][[0, 2, 4]]).all()
    if c.zero_inf:
        assert np.isfinite(exp['out']).all() and np.isfinite(exp['grad']).all()
        assert not exp['grad'][:, list(R.INFEASIBLE)].any()
    else:
        assert np.isinf(exp['out']).any()


def test_ctc_rows_cover_what_they_are_there_for():
    by = R.CTC_BY_NAME
    assert list(by['ring_edges'].in_len) == [1, 2, 7, 8, 9, 10, 16, 17]
    assert {c.blank for c in R.CTC_CASES} >= {0, 2, 5} and by['blank_last'].blank == by['blank_last'].V - 1
    for name in ('label_is_blank', 'label_is_blank_mid', 'label_is_blank_last'):
        c = by[name]
        tg = R.ctc_targets(c)
        assert all((tg[b, :c.tg_len[b]] == c.blank).any() for b in range(c.B))
        assert all((tg[b, c.tg_len[b] - 1] == c.blank) == (name in R.TORCH_LAST_FRAME) for b in range(c.B))
    tg = R.ctc_targets(by['repeats'])
    assert set(np.unique(tg)) == {1, 2} and (tg[:, 1:] == tg[:, :-1]).sum() >= 6
    assert R.ctc_inputs(by['no_labels'])[1].shape == (3, 0)
    assert {c.layout for c in R.CTC_CASES} == {'tbv', 'btv', 'pad', 'off1'}
    assert by['lay_pad'].V % 4 == 0 and by['lay_off1'].V % 4 == 0 and by['lay_v7'].V % 4 != 0
    assert {(c.reduction, c.zero_inf) for c in R.CTC_CASES} >= {(r, z) for r in ('none', 'mean', 'sum') for z in (False, True)}
    lp = R.ctc_inputs(by['peaky'])[0]
    assert -80.0 < float(lp.min()) < -50.0
    for name in ('l511', 'l512'):                      # one full-length utterance, one of half length, one of length 2
        c = by[name]
        assert c.tg_len[0] == c.Lmax and c.tg_len[1] == c.Lmax // 2 and c.tg_len[2] == 2
    for c in R.CTC_CASES:                              # every row has a feasible utterance with something to compare
        exp = R.ctc_expected(c)
        assert np.isfinite(exp['nll']).any() and np.abs(np.nan_to_num(exp['grad'])).max() > 0, c.name


@pytest.mark.parametrize("name", ['label_is_blank', 'label_is_blank_last', 'repeats', 'blank_mid'])
def test_ctc_lattices_meet_in_the_middle(name):
    """sum_s alpha_t[s] * beta_t[s] / p(lp_t[ext[s]]) = p(target) at every frame - what ties alpha to beta - and so the
    state occupancies of a frame, the terms the gradient subtracts from exp(lp), add up to 1: sum_c grad[t,b,c] / gscale
    = sum_c exp(lp) - 1.  This holds the one element where the reference leaves torch (TORCH_LAST_FRAME) to the
    definition."""
    c = R.CTC_BY_NAME[name]
    lp, tg, il, tl = R.ctc_inputs(c)
    exp = R.ctc_expected(c)
    for b in range(c.B):
        al, be = exp['alpha'][b], exp['beta'][b]
        ext = np.full(2 * c.tg_len[b] + 1, c.blank)
        ext[1::2] = tg[b, :c.tg_len[b]].numpy()
        x = lp[:, b].double().numpy()
        for t in range(al.shape[0]):
            tot = np.logaddexp.reduce(al[t] + be[t] - x[t][ext])
            assert abs(tot + exp['nll'][b]) < 1e-9
            assert abs(exp['grad'][t, b].sum() / exp['gscale'][b] - (np.exp(x[t]).sum() - 1.0)) < 1e-9


def test_ctc_out_of_range_labels_have_the_documented_gradient():
    c = R.BAD_LABELS
    lp, tg, il, tl = R.ctc_inputs(c)
    exp = R.ctc_expected(c)
    good = list(R.GOOD_UTTS)
    assert sorted(good + list(R.BAD_UTTS)) == list(range(c.B))
    for b in R.BAD_UTTS:
        Tb = c.in_len[b]
        assert np.isnan(exp['nll'][b]) and np.isnan(exp['grad'][:Tb, b]).all() and not exp['grad'][Tb:, b].any()
    # the good utterances are what torch gives for them alone
    x = lp[:, good].double().requires_grad_(True)
    w = torch.as_tensor(R.ctc_weights(c)).double()[good]
    out = F.ctc_loss(x, tg[good], il[good], tl[good], blank=c.blank, reduction='none')
    (out * w).sum().backward()
    _close(exp['nll'][good], out.detach().numpy(), 'nll of the good utterances')
    _close(exp['grad'][:, good], x.grad.numpy(), 'gradient of the good utterances')


@pytest.mark.parametrize("case", R.LEN_BEYOND, ids=lambda c: c.name)
def test_ctc_lengths_beyond_the_tensor_are_clamped(case):
    c = case
    lp, tg, il, tl = R.ctc_inputs(c)
    assert (il > c.T).any() and (tl > c.Lmax).any()
    exp = R.ctc_expected(c)
    out, grad = R.ctc_torch(c, R.F64)                  # torch on the clamped lengths
    _close(exp['out'], out, 'loss')
    _close(exp['grad'], grad, 'grad')


@pytest.mark.parametrize("case", R.CTC_CASES + R.LEN_BEYOND + [R.BAD_LABELS], ids=lambda c: c.name)
def test_ctc_input_condition(case):
    e = R.ctc_e32(case, R.GOOD_UTTS if case is R.BAD_LABELS else None)
    print("LOSSCOND %s | ctc_loss e32 %.3e | ctc_grad e32 %.3e | max nll %.1f" % (
        case.name, e['ctc_loss'], e['ctc_grad'], np.nanmax(np.where(np.isfinite(R.ctc_expected(case)['nll']),
                                                                      R.ctc_expected(case)['nll'], np.nan))))
    for kind, v in e.items():
        assert 4 * v <= R.HARD[kind], (case.name, kind, v)


# ------------------------------------------------------------------------------------------------ cross entropy
@pytest.mark.parametrize("case", R.CE_CASES, ids=lambda c: c.name)
def test_ce_reference_is_torch_in_float64(case):
    c, x, t = R.ce_inputs(case)
    loss, dx = R.ce_expected(c)
    tl, tg = R.ce_torch(c, x, t, R.F64)
    _close(loss, tl, c.name + ' loss')
    _close(dx, tg, c.name + ' dx')
    live = ((t != c.ignore) & (t >= 0) & (t < c.V)).numpy()
    assert not dx[~live].any()
    if c.all_ignored:
        assert not live.any() and np.isnan(loss) and not dx.any()
    elif c.values == 'ninf_target':
        assert loss == np.inf and np.isfinite(dx).all()
    else:
        assert np.isfinite(loss) and live.any()
    if c.oob:
        assert ((t < 0) | (t >= c.V)).any()


def test_ce_rows_cover_what_they_are_there_for():
    assert {(c.V, c.R) for c in R.CE_CASES} >= {(V, r) for V in (1, 3, 63, 64, 65, 4100) for r in (1, 4, 5, 257)}
    for ign in (0, -100):
        assert sum(c.ignore == ign for c in R.CE_CASES) >= 4
    assert any(c.ignore not in (0, -100) and 0 < c.ignore < c.V - 1 for c in R.CE_CASES)
    seen = set()
    for c in R.CE_CASES:
        if c.oob:
            t = R.ce_inputs(c)[2]
            seen |= {int(v) - c.V if v >= c.V else int(v) for v in t[(t < 0) | (t >= c.V)]}
    assert seen >= {-1, 0, 7}                           # targets -1, V and V + 7
    x = R.ce_inputs('offset')[1]
    assert float(x.max()) > 80 and float(x.min()) < -80
    x = R.ce_inputs('constant')[1]
    assert float(x[0].min()) == float(x[0].max())
    assert {pad for _, pad in R.CE_LD_CASES} == {3, 4}


@pytest.mark.parametrize("name", [c.name for c in R.CE_CASES] + ['det_%d' % r for r in R.CE_DET_ROWS])
def test_ce_input_condition(name):
    e = R.ce_e32(name)
    print("LOSSCOND %s | ce_loss e32 %.3e | ce_grad e32 %.3e" % (name, e['ce_loss'], e['ce_grad']))
    for kind, v in e.items():
        assert 4 * v <= R.HARD[kind], (name, kind, v)


# ------------------------------------------------------------------------------------------------ log-softmax, tanh
@pytest.mark.parametrize("case", R.LSM_CASES, ids=lambda c: c.name)
def test_log_softmax_reference_is_torch_in_float64(case):
    y, dx = R.lsm_expected(case)
    ty, tdx = R.lsm_torch(case, R.F64)
    _close(y, ty, case.name + ' y')
    _close(dx, tdx, case.name + ' dx')
    e = R.lsm_e32(case)
    print("LOSSCOND %s | lsm_y e32 %.3e | lsm_dx e32 %.3e" % (case.name, e['lsm_y'], e['lsm_dx']))
    ref_max = np.abs(y[np.isfinite(y)]).max() if np.isfinite(y).any() else 0.0
    assert 4 * e['lsm_y'] * ref_max <= R.HARD['lsm_y'] and 4 * e['lsm_dx'] <= R.HARD['lsm_dx']
    if case.values == 'extremes':
        x = R.lsm_inputs(case)[0]
        assert float(x[0].max()) == 90.0 and float(x[1].max()) == -90.0
        assert np.isnan(y[3]).all() and np.isinf(y[2, ::3]).all() and np.isfinite(y[[0, 1, 4]]).all()


def test_log_softmax_abi_rows_reach_both_kernels():
    assert {k for *_, k in R.LSM_ABI} == {'vector', 'scalar'}
    for name, pad, off, kernel in R.LSM_ABI:
        c = R.LSM_BY_NAME[name]
        assert R.lsm_kernel(c.cols, c.cols + pad, off) == kernel, (name, pad, off)
    pads = {(pad, off) for _, pad, off, _ in R.LSM_ABI}
    assert pads >= {(0, 0), (4, 0), (1, 0), (0, 1)}
    assert {c.cols for c in R.LSM_CASES} >= set(R.LSM_COLS) and {c.rows for c in R.LSM_CASES} >= set(R.LSM_ROWS)


@pytest.mark.parametrize("n", R.TANH_SIZES[:4])
def test_tanh_reference_is_torch_in_float64(n):
    x, dy = R.tanh_inputs(n)
    x = torch.cat([x, R.tanh_special()])[:max(n, len(R.TANH_SPECIAL))]
    dy = torch.ones_like(x)
    y, dx = R.tanh_reference(x, dy)
    xr = x.double().requires_grad_(True)
    ty = torch.tanh(xr)
    _close(y.numpy(), ty.detach().numpy(), 'tanh')
    y32 = ty.detach().float().double()
    _close(dx.numpy(), (dy.double() * (1 - y32 * y32)).numpy(), 'tanh backward')


def test_ulp_distance():
    one = np.float32(1.0)
    up = np.nextafter(one, np.float32(2.0))
    assert R.ulp_distance([one, up, -one, np.float32(0.0)], [1.0, 1.0, float(np.nextafter(-one, np.float32(-2))), -0.0]
                          ).tolist() == [0, 1, 1, 0]
    assert R.ulp_distance([np.float32(1e-45)], [-1e-45]).tolist() == [2]
    assert R.ulp_distance([np.float32('nan'), one], [float('nan'), float('nan')]).tolist() == [0, 2 ** 31]
