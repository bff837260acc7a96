"""GPU: every kernel variant of the CTC loss (csrc/ctc.hip: gather, the four lattice instantiations, the dense and the sparse
gradient pass) and of the loss and row kernels of csrc/rowops.hip (plain cross entropy forward / fixed-order sum / backward,
log-softmax vector and scalar, tanh) against the float64 references and on the case tables of tests/loss_reference.py.
tests/test_loss_plan_cpu.py holds every CTC row to the launch plan it names, and every CTC row asserts that plan on the
device before it runs (asrk_ctc_loss_plan_info at the live arguments), so a shape that drifts onto another instantiation
fails instead of passing on that one's arithmetic.

Criterion, per tensor: helpers.rel_err (over the elements where the reference is finite) is inside the hard limit the
suite already holds the op to - CTC loss and lattices 1e-4, CTC gradient 1e-3, cross entropy 1e-4 / 1e-3
(tests/test_loss_options_gpu.py), log-softmax 2e-5 absolute forward and 1e-4 backward, tanh 4 ulp forward - AND
rel_err <= max(F * e32, 4 * 2**-24), e32 = rel_err of the float32 CPU run of torch's op against its float64 run on the
row's inputs (alpha / beta: of the reference's own float32 run).  Every test prints
    LOSSVAR name | kind | e32 | bound | device | device/e32
(pytest -s).  Exact where the code promises it: zeros of the CTC gradient at t >= T_b, of utterances zeroed under
zero_infinity and of ignored cross-entropy rows, untouched sentinels around and between rows, NaN and +-inf exactly where
the reference has them, bit-equal repeats under ASRK_DETERMINISTIC.

F is set per tensor kind to the largest device / e32 seen on the MI355X over every row below, times 4, rounded up to a
power of two:

    tensor        largest device / e32   where                                                  F
    ctc_loss      1.00                   t513_l3, t512_l3 and most other rows                   4
    ctc_lattice   1.00                   ring_edges beta, t513_l3 beta (0.54 l128 alpha)        4
    ctc_grad      1.33                   bad_labels, its two good utterances (1.16 repeats)     8
    ce_loss       36.62                  v64_r1_ign0 (21.37 v4100_r257_ignmid through the ABI)  256
    ce_grad       18.95                  offset (9.23 v4100_r5_ign-100)                         128
    lsm_y         2.93                   extremes_odd (1.77 c260_r5)                            16
    lsm_dx        24.20                  extremes_odd (7.78 c4_r1)                              128
    tanh_y        2.62                   n = 1048835 (2.25 n = 256); at most 1 ulp everywhere   16
    tanh_dx       1.00                   every row                                              4

(383 figures over 140 tests; e32 0 ... 1.0e-4, device 0 ... 1.0e-4.)  What the figures say:
  - The CTC kernels land on torch's float32 CPU run almost element for element (ratios of 1.00 to three digits on most
    rows, FAST or not): alpha, beta and nll are numbers around 100 stored in float32, the rounding of that store (4e-6)
    is far larger than anything exp / log contribute inside a step, and both implementations round the same true values.
    The gradient's 1e-4 on the long rows is that store's error walking through 560 frames, on the CPU as on the device.
  - ce_loss 36.62 is one row with one counted target whose CPU run happens to be right to 2e-9; the device's 7e-8 is
    half an ulp of the loss and under the 2.4e-7 floor.  The ratios that are decided by F are the sums: 257 rows of
    float atomics in whatever order they arrive (15.78 and 21.37 for the same row in one session).
  - ce_grad `offset` and lsm_dx `extremes_odd` are rows whose maximum is 80 ... 90: the kernels form lse = m + log(sum) in
    float32 and subtract it from x, so y = x - lse carries half an ulp of 90 (4e-6) into exp(y), where torch subtracts m
    first.  Inside every hard limit by a factor of fifty; from |m| = 512 on half an ulp of m is 3e-5 and the forward
    would pass its 2e-5.
"""
import ctypes
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import PKG_NAME
import loss_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
F = dict(ctc_loss=4, ctc_lattice=4, ctc_grad=8, ce_loss=256, ce_grad=128, lsm_y=16, lsm_dx=128, tanh_y=16, tanh_dx=4)
SENT = 12345.5                      # guard value: exact in float32, nothing a kernel computes


def _lib():
    return importlib.import_module(PKG_NAME + "._lib")


class Judge:
    """collects every tensor of a test, prints its line, and fails at the end with all of them"""

    def __init__(self, name):
        self.name, self.bad = name, []

    def add(self, kind, e32, err, hard_err=None):
        b = R.bound(e32, F[kind])
        print("LOSSVAR %s | %s | e32 %.3e | bound %.3e | device %.3e | device/e32 %.2f" % (
            self.name, kind, e32, b, err, err / e32 if e32 > 0 else float('nan')))
        hard = err if hard_err is None else hard_err
        if not (kind not in R.HARD or hard < R.HARD[kind]) or not err <= b:
            self.bad.append((kind, err, b, hard))

    def done(self):
        assert not self.bad, (self.name, self.bad)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ====================================================================================================== CTC
def _assert_plan(ops, c):
    out = (ctypes.c_int * R.PLAN_LEN)()
    assert ops._L().asrk_ctc_loss_plan_info(c.T, c.B, c.Lmax, out, R.PLAN_LEN) == 0
    got = dict(zip(R.PLAN_FIELDS, out))
    assert (got['tmpl'], bool(got['fast'])) == c.route, (c.name, got)
    for field, v in c.plan.items():
        assert got[field] == v, (c.name, field, got[field], v)


def _ctc_exact(c, grad, exp, out=None):
    """what the code promises exactly; grad [T,B,V] numpy"""
    ref = exp['grad']
    assert R.same_nonfinite(grad, ref), c.name                       # NaN exactly where the reference has it
    for b in range(c.B):
        Tb = max(min(c.in_len[b], c.T), 0)
        assert not grad[Tb:, b].any(), (c.name, b)                   # frames beyond the utterance: exactly 0
        if c.zero_inf and exp['nll'][b] == np.inf:
            assert not grad[:, b].any(), (c.name, b)                 # zeroed utterance: exactly 0, label columns too
    if out is not None:
        assert R.same_nonfinite(out, exp['out']), c.name
        assert np.array_equal(np.asarray(out) == 0, np.asarray(exp['out']) == 0)


def _ctc_ops(ops, c):
    """through ops.CTCLoss -> (returned loss, gradient as CTCLossFn.backward hands it over)"""
    lp, tg, il, tl = R.ctc_inputs(c)
    x = R.ctc_layout(c, lp, DEV).detach().requires_grad_(True)
    mod = ops.CTCLoss(blank=c.blank, reduction=c.reduction, zero_infinity=c.zero_inf)
    out = mod(x, tg.to(DEV), il.to(DEV), tl.to(DEV))
    w = torch.as_tensor(R.ctc_weights(c)).to(DEV)
    (grad,) = torch.autograd.grad((out * w).sum(), x)
    return mod, out.detach().cpu().numpy(), grad


@pytest.mark.parametrize("case", R.CTC_CASES, ids=lambda c: c.name)
def test_ctc_row(ops, case):
    c = case
    _assert_plan(ops, c)
    exp, e32 = R.ctc_expected(c), R.ctc_e32(c)
    mod, out, grad = _ctc_ops(ops, c)
    ops.check_errors()
    assert grad.shape == (c.T, c.B, c.V)
    if c.layout == 'btv':                                            # the layout CTCLossFn.backward documents
        assert grad.transpose(0, 1).is_contiguous() and (c.B == 1 or grad.stride(1) > grad.stride(0))
    else:
        assert grad.is_contiguous()
    g = grad.cpu().numpy()
    _ctc_exact(c, g, exp, out)
    if c.zero_inf:
        assert int(mod.n_infeasible) == int((exp['nll'] == np.inf).sum())
    j = Judge(c.name)
    j.add('ctc_loss', e32['ctc_loss'], R.finite_rel_err(out, exp['out']))
    j.add('ctc_grad', e32['ctc_grad'], R.ctc_grad_err(g, exp['grad']))
    j.done()


def _ctc_abi(ops, c, x, gscale, ex, flags=0, grad=None):
    """the C ABI directly, plain or _ex entry points -> dict of device tensors; alpha / beta / nll start as sentinels"""
    L, p = ops._L(), ops._p
    lp, tg, il, tl = R.ctc_inputs(c)
    S = 2 * c.Lmax + 1
    tgd, ild, tld = tg.to(DEV).contiguous(), il.to(DEV), tl.to(DEV)
    alpha = torch.full((c.B, c.T, S), SENT, device=DEV)
    beta = torch.full((c.B, c.T, S), SENT, device=DEV)
    lpg = torch.full((c.B, c.T, S), SENT, device=DEV)
    nll = torch.full((c.B,), SENT, device=DEV)
    loss = torch.full((c.B,), SENT, device=DEV) if ex else None
    cnt = torch.full((), -7, dtype=torch.int32, device=DEV) if ex else None
    gs = torch.as_tensor(np.asarray(gscale, np.float32)).to(DEV)
    if grad is None:
        grad = torch.full((c.T, c.B, c.V), SENT, device=DEV)
    head = (p(x), x.stride(0), x.stride(1), c.T, c.B, c.V, p(tgd if c.Lmax else None), c.Lmax, c.Lmax, p(ild), p(tld),
            c.blank)
    st = ops._stream()
    if ex:
        _lib().check(L.asrk_ctc_loss_fwd_ex_f32(*head, p(alpha), p(beta), p(lpg), p(nll), flags, p(loss), p(cnt), st),
                     "ctc_fwd_ex")
        _lib().check(L.asrk_ctc_loss_bwd_ex_f32(*head, p(alpha), p(beta), p(lpg), p(nll), p(gs), p(grad), grad.stride(0),
                                                grad.stride(1), flags, st), "ctc_bwd_ex")
    else:
        _lib().check(L.asrk_ctc_loss_fwd_f32(*head, p(alpha), p(beta), p(lpg), p(nll), st), "ctc_fwd")
        _lib().check(L.asrk_ctc_loss_bwd_f32(*head, p(alpha), p(beta), p(lpg), p(nll), p(gs), p(grad), grad.stride(0),
                                             grad.stride(1), st), "ctc_bwd")
    ops.check_errors()
    return dict(alpha=alpha, beta=beta, nll=nll, loss=loss, cnt=cnt, grad=grad)


def _lattices(c, dev, exp):
    """[B,T,S] device lattice -> per utterance [T_b,S_b] numpy, None where the reference has none"""
    a = dev.cpu().numpy()
    out = []
    for b in range(c.B):
        r = exp[b]
        out.append(None if r is None else a[b, :r.shape[0], :r.shape[1]])
    return out


@pytest.mark.parametrize("ex", [False, True], ids=["plain", "ex"])
@pytest.mark.parametrize("name", R.LATTICE_ROWS)
def test_ctc_lattices(ops, name, ex):
    """alpha and beta themselves, both entry points: one row per lattice instantiation, the prefetch-ring edges and a
    target with the blank's index in it"""
    c = R.CTC_BY_NAME[name]
    _assert_plan(ops, c)
    exp = R.ctc_expected(c)
    lp = R.ctc_inputs(c)[0]
    r = _ctc_abi(ops, c, R.ctc_layout(c, lp, DEV), exp['gscale'], ex)
    e32 = R.ctc_lattice_e32(c)
    j = Judge("%s[%s]" % (c.name, "ex" if ex else "plain"))
    j.add('ctc_lattice', e32, R.lattice_err(_lattices(c, r['alpha'], exp['alpha']), exp['alpha']))
    j.add('ctc_lattice', e32, R.lattice_err(_lattices(c, r['beta'], exp['beta']), exp['beta']))
    g = r['grad'].cpu().numpy()
    _ctc_exact(c, g, exp)
    t32 = R.ctc_e32(c)
    j.add('ctc_loss', t32['ctc_loss'], R.finite_rel_err(r['nll'].cpu().numpy(), exp['nll']))
    j.add('ctc_grad', t32['ctc_grad'], R.ctc_grad_err(g, exp['grad']))
    j.done()
    if ex:
        assert torch.equal(r['loss'], r['nll']) and int(r['cnt']) == 0


@pytest.mark.parametrize("name,off", [('lay_pad', 0), ('lay_btv', 1), ('lay_off1', 1)])
def test_ctc_gradient_into_a_strided_allocation(ops, name, off):
    """the C ABI with grad itself a [:, :, :V] view of a [T,B,V+1] allocation entered `off` floats in: the alignment of the
    gradient rows (and, for lay_pad, of the log-prob rows with them) changes from row to row, so ctc_grad_dense_kernel
    takes 16-byte and scalar rows in one launch (lay_off1: no log-prob row is aligned, all scalar); the gaps between the
    rows and the guards around them keep their sentinel"""
    c = R.CTC_BY_NAME[name]
    exp = R.ctc_expected(c)
    x = R.ctc_layout(c, R.ctc_inputs(c)[0], DEV)
    n = c.T * c.B * (c.V + 1)
    buf = torch.full((off + n + 3,), SENT, device=DEV)
    assert buf.data_ptr() % 16 == 0 and c.V % 4 == 0
    grad = buf[off:off + n].view(c.T, c.B, c.V + 1)[:, :, :c.V]
    rows = {(x[t, b].data_ptr() | grad[t, b].data_ptr()) % 16 == 0 for t in range(c.T) for b in range(c.B)}
    assert rows == ({False} if name == 'lay_off1' else {True, False}), rows          # both kinds of row in this launch
    r = _ctc_abi(ops, c, x, exp['gscale'], False, grad=grad)
    g = grad.cpu().numpy()
    _ctc_exact(c, g, exp)
    full = buf[off:off + n].view(c.T, c.B, c.V + 1)
    assert torch.equal(full[:, :, c.V], torch.full((c.T, c.B), SENT, device=DEV))
    assert torch.equal(buf[:off], torch.full((off,), SENT, device=DEV))
    assert torch.equal(buf[off + n:], torch.full((3,), SENT, device=DEV))
    j = Judge(c.name + "[strided grad]")
    e32 = R.ctc_e32(c)
    j.add('ctc_loss', e32['ctc_loss'], R.finite_rel_err(r['nll'].cpu().numpy(), exp['nll']))
    j.add('ctc_grad', e32['ctc_grad'], R.ctc_grad_err(g, exp['grad']))
    j.done()


@pytest.mark.parametrize("ex", [False, True], ids=["plain", "ex"])
def test_ctc_out_of_range_labels_write_nothing_outside_their_rows(ops, ex):
    """labels -3 and V + 100 inside three utterances: nll NaN, their frames NaN for t < T_b and 0 beyond, the other
    utterances as if they were alone, and the memory before and after the gradient untouched (as column indices the
    labels would reach both)"""
    c = R.BAD_LABELS
    exp = R.ctc_expected(c)
    x = R.ctc_layout(c, R.ctc_inputs(c)[0], DEV)
    n, g0, g1 = c.T * c.B * c.V, 37, 131
    buf = torch.full((g0 + n + g1,), SENT, device=DEV)
    grad = buf[g0:g0 + n].view(c.T, c.B, c.V)
    for flags in ((0, 1) if ex else (0,)):
        buf.fill_(SENT)
        r = _ctc_abi(ops, c, x, exp['gscale'], ex, flags=flags, grad=grad)
        assert torch.equal(buf[:g0], torch.full((g0,), SENT, device=DEV))
        assert torch.equal(buf[g0 + n:], torch.full((g1,), SENT, device=DEV))
        g, nll = grad.cpu().numpy(), r['nll'].cpu().numpy()
        assert tuple(b for b in range(c.B) if np.isnan(nll[b])) == R.BAD_UTTS
        _ctc_exact(c, g, exp)
        for b in R.BAD_UTTS:
            assert np.isnan(g[:c.in_len[b], b]).all() and not g[c.in_len[b]:, b].any()
        j = Judge("bad_labels[%s flags=%d]" % ("ex" if ex else "plain", flags))
        e32 = R.ctc_e32(c, R.GOOD_UTTS)                               # torch on the utterances it accepts
        j.add('ctc_loss', e32['ctc_loss'], R.finite_rel_err(nll, exp['nll']))
        j.add('ctc_grad', e32['ctc_grad'], R.ctc_grad_err(g, exp['grad']))
        j.done()
        if ex:
            assert int(r['cnt']) == 0 and _same_bits(r['loss'], r['nll'])


def test_ctc_out_of_range_labels_through_autograd(ops):
    """ops.CTCLoss(...).backward() on that batch: the leaf gradient is not finite (what the solver's guard tests), the
    good utterances' slices are right"""
    c = R.BAD_LABELS
    exp = R.ctc_expected(c)
    lp, tg, il, tl = R.ctc_inputs(c)
    x = lp.to(DEV).requires_grad_(True)
    out = ops.CTCLoss(blank=c.blank, reduction='none')(x, tg.to(DEV), il.to(DEV), tl.to(DEV))
    (out * torch.as_tensor(R.ctc_weights(c)).to(DEV)).sum().backward()
    ops.check_errors()
    g = x.grad.cpu().numpy()
    assert not np.isfinite(g).all() and not np.isfinite(np.linalg.norm(g))
    assert R.same_nonfinite(out.detach().cpu().numpy(), exp['out'])
    _ctc_exact(c, g, exp)
    good = list(R.GOOD_UTTS)
    e32 = R.ctc_e32(c, good)
    j = Judge("bad_labels[autograd]")
    j.add('ctc_grad', e32['ctc_grad'], R.finite_rel_err(g[:, good], exp['grad'][:, good]))
    j.done()
    mean = ops.CTCLoss(blank=c.blank, reduction='mean')(lp.to(DEV), tg.to(DEV), il.to(DEV), tl.to(DEV))
    assert torch.isnan(mean).item()


@pytest.mark.parametrize("case", R.LEN_BEYOND, ids=lambda c: c.name)
def test_ctc_lengths_beyond_the_tensor_are_clamped(ops, case):
    """input_length > T and target_length > Lmax give what the clamped lengths give, bit for bit, and that is the
    reference's (the 'mean' divisor included)"""
    c = case
    lp, tg, il, tl = R.ctc_inputs(c)
    exp, e32 = R.ctc_expected(c), R.ctc_e32(c)
    w = torch.as_tensor(R.ctc_weights(c)).to(DEV)
    res = []
    for i, t in ((il, tl), (il.clamp(max=c.T), tl.clamp(max=c.Lmax))):
        x = lp.to(DEV).requires_grad_(True)
        out = ops.CTCLoss(blank=c.blank, reduction=c.reduction)(x, tg.to(DEV), i.to(DEV), t.to(DEV))
        (out * w).sum().backward()
        res.append((out.detach().reshape(-1), x.grad))
    ops.check_errors()
    assert _same_bits(res[0][0], res[1][0]) and _same_bits(res[0][1], res[1][1])
    g = res[0][1].cpu().numpy()
    _ctc_exact(c, g, exp)
    j = Judge(c.name)
    j.add('ctc_loss', e32['ctc_loss'], R.finite_rel_err(res[0][0].cpu().numpy().reshape(exp['out'].shape), exp['out']))
    j.add('ctc_grad', e32['ctc_grad'], R.ctc_grad_err(g, exp['grad']))
    j.done()


# ====================================================================================================== cross entropy
def _ce_abi(ops, x, t, c, pad):
    """asrk_cross_entropy_{fwd,bwd}_f32 with ld = V + pad; the gaps of logits hold 1e30 (reading them would show), the
    gaps of dlogits a sentinel -> (loss, dx [R,V], the whole dlogits buffer)"""
    L, p = ops._L(), ops._p
    ld = c.V + pad
    xb = torch.full((c.R, ld), 1e30, device=DEV)
    xb[:, :c.V] = x.to(DEV)
    db = torch.full((c.R, ld), SENT, device=DEV)
    td = t.to(DEV)
    lse = torch.empty((c.R,), device=DEV)
    sums = torch.full((2,), SENT, device=DEV)
    st = ops._stream()
    _lib().check(L.asrk_cross_entropy_fwd_f32(p(xb), c.R, c.V, ld, p(td), c.ignore, p(lse), p(sums), st), "ce_fwd")
    gscale = (torch.tensor(R.CE_W, device=DEV) / sums[1]).reshape(1).contiguous()       # as CrossEntropyFn.backward
    _lib().check(L.asrk_cross_entropy_bwd_f32(p(xb), c.R, c.V, ld, p(td), c.ignore, p(lse), p(gscale), p(db), st), "ce_bwd")
    ops.check_errors()
    return (sums[0] / sums[1]).cpu().numpy(), db[:, :c.V].cpu().numpy(), db


def _ce_judge(label, c, t, loss, dx, kinds=('ce_loss', 'ce_grad')):
    ref_loss, ref_dx = R.ce_expected(c)
    e32 = R.ce_e32(c)
    assert R.same_nonfinite(loss, ref_loss) and R.same_nonfinite(dx, ref_dx), label
    live = ((t != c.ignore) & (t >= 0) & (t < c.V)).numpy()
    assert not dx[~live].any(), label                                # ignored rows: exactly 0
    j = Judge(label)
    if 'ce_loss' in kinds:
        j.add('ce_loss', e32['ce_loss'], R.finite_rel_err(loss, ref_loss))
    j.add('ce_grad', e32['ce_grad'], R.finite_rel_err(dx, ref_dx))
    j.done()


@pytest.mark.parametrize("case", R.CE_CASES, ids=lambda c: c.name)
def test_ce_row(ops, case):
    """the plain kernels through ops.CrossEntropyLoss and through the C ABI (ld == V)"""
    c, x, t = R.ce_inputs(case)
    xg = x.to(DEV).requires_grad_(True)
    loss = ops.CrossEntropyLoss(ignore_index=c.ignore)(xg, t.to(DEV))
    (loss * R.CE_W).backward()
    ops.check_errors()
    _ce_judge(c.name, c, t, loss.detach().cpu().numpy(), xg.grad.cpu().numpy())
    loss2, dx2, _ = _ce_abi(ops, x, t, c, 0)
    _ce_judge(c.name + "[abi]", c, t, loss2, dx2)
    assert np.array_equal(dx2, xg.grad.cpu().numpy(), equal_nan=True)        # the same kernel on the same numbers


@pytest.mark.parametrize("name,pad", R.CE_LD_CASES)
def test_ce_leading_dimension(ops, name, pad):
    c, x, t = R.ce_inputs(name)
    loss, dx, db = _ce_abi(ops, x, t, c, pad)
    assert torch.equal(db[:, c.V:], torch.full((c.R, pad), SENT, device=DEV))          # the gaps of dlogits are not written
    _ce_judge("%s[ld=V+%d]" % (c.name, pad), c, t, loss, dx)


@pytest.fixture(scope="module")
def det_runs(tmp_path_factory):
    """a fresh process with ASRK_DETERMINISTIC=1: ce_fwd_kernel without atomics + ce_sum_kernel"""
    out = str(tmp_path_factory.mktemp("lossdet") / "det.npz")
    r = subprocess.run([sys.executable, os.path.join(HERE, "loss_variants_worker.py"), out], capture_output=True, text=True,
                       env=dict(os.environ, ASRK_DETERMINISTIC="1"), timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    z = np.load(out)
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize("rows", R.CE_DET_ROWS)
def test_ce_fixed_order_sum(ops, det_runs, rows):
    """ce_sum_kernel against the reference, not against itself: 1 row, one short of / exactly / one past the 256
    threads of its workgroup, and a third pass (600)"""
    name = 'det_%d' % rows
    c, x, t = R.ce_inputs(name)
    assert bool(det_runs['same_%d' % rows])                          # two runs, the same bits
    _ce_judge(name, c, t, det_runs['loss_%d' % rows], det_runs['grad_%d' % rows])


# ====================================================================================================== log-softmax
def _lsm_judge(label, y, dx, ref_y, ref_dx, e32):
    assert R.same_nonfinite(y, ref_y) and R.same_nonfinite(dx, ref_dx), label
    m = np.isfinite(ref_y)
    j = Judge(label)
    j.add('lsm_y', e32['lsm_y'], R.finite_rel_err(y, ref_y),
          hard_err=float(np.abs(y[m].astype(np.float64) - ref_y[m]).max()) if m.any() else 0.0)
    j.add('lsm_dx', e32['lsm_dx'], R.finite_rel_err(dx, ref_dx))
    j.done()


@pytest.mark.parametrize("case", R.LSM_CASES, ids=lambda c: c.name)
def test_log_softmax_row(ops, case):
    c = case
    x, dy = R.lsm_inputs(c)
    ref_y, ref_dx = R.lsm_expected(c)
    xg = x.to(DEV).requires_grad_(True)
    y = ops.log_softmax(xg)
    y.backward(dy.to(DEV))
    with torch.no_grad():
        y2 = ops.log_softmax(x.to(DEV))                              # the inference entry: the same kernel call
    ops.check_errors()
    assert _same_bits(y2, y.detach())
    _lsm_judge(c.name, y.detach().cpu().numpy(), xg.grad.cpu().numpy(), ref_y, ref_dx, R.lsm_e32(c))


@pytest.mark.parametrize("name,pad,off,kernel", R.LSM_ABI)
def test_log_softmax_abi(ops, name, pad, off, kernel):
    """ld > cols and a base off alignment through the C ABI: the vector or the scalar kernel as the row claims, gap and
    guard sentinels untouched, forward and backward"""
    c = R.LSM_BY_NAME[name]
    x, dy = R.lsm_inputs(c)
    ref_y, ref_dx = R.lsm_expected(c)
    ld = c.cols + pad
    L, p, st = ops._L(), ops._p, ops._stream()

    def buffer(fill, data=None):
        buf = torch.full((off + c.rows * ld + 5,), fill, device=DEV)
        assert buf.data_ptr() % 16 == 0
        view = buf[off:off + c.rows * ld].view(c.rows, ld)
        if data is not None:
            view[:, :c.cols] = data.to(DEV)
        return buf, view
    _, xv = buffer(1e30, x)
    _, gv = buffer(1e30, dy)
    ybuf, yv = buffer(SENT)
    dbuf, dv = buffer(SENT)
    vec = all(v.data_ptr() % 16 == 0 for v in (xv, yv, gv, dv)) and c.cols % 4 == 0 and ld % 4 == 0
    assert ('vector' if vec else 'scalar') == kernel == R.lsm_kernel(c.cols, ld, off)
    _lib().check(L.asrk_log_softmax_fwd_f32(p(xv), p(yv), c.rows, c.cols, ld, st), "log_softmax")
    _lib().check(L.asrk_log_softmax_bwd_f32(p(yv), p(gv), p(dv), c.rows, c.cols, ld, st), "log_softmax_bwd")
    ops.check_errors()
    for buf, view in ((ybuf, yv), (dbuf, dv)):
        assert torch.equal(view[:, c.cols:], torch.full((c.rows, pad), SENT, device=DEV))
        assert torch.equal(buf[:off], torch.full((off,), SENT, device=DEV))
        assert torch.equal(buf[off + c.rows * ld:], torch.full((5,), SENT, device=DEV))
    _lsm_judge("%s[ld+%d off%d %s]" % (name, pad, off, kernel), yv[:, :c.cols].cpu().numpy(), dv[:, :c.cols].cpu().numpy(),
               ref_y, ref_dx, R.lsm_e32(c))


# ====================================================================================================== tanh
def _tanh_judge(label, x, dy, y, dx):
    """y against the float64 tanh (4 ulp and the e32 criterion); dx against dy * (1 - y^2) of the y the kernel read"""
    ref_y, _ = R.tanh_reference(x)
    ref_y = ref_y.numpy()
    ulp = R.ulp_distance(y, ref_y)
    print("LOSSVAR %s | tanh ulp | largest %d of %d allowed" % (label, int(ulp.max()), R.TANH_ULP))
    assert int(ulp.max()) <= R.TANH_ULP, (label, x.numpy()[ulp.argmax()], y[ulp.argmax()])
    assert R.same_nonfinite(y, ref_y)
    y32 = torch.tanh(x)
    ref_dx = (dy.double() * (1.0 - torch.from_numpy(y).double() ** 2)).numpy()
    dx32 = (dy * (1.0 - torch.from_numpy(y) * torch.from_numpy(y))).numpy()
    assert R.same_nonfinite(dx, ref_dx)
    j = Judge(label)
    j.add('tanh_y', R.finite_rel_err(y32.numpy(), ref_y), R.finite_rel_err(y, ref_y))
    j.add('tanh_dx', R.finite_rel_err(dx32, ref_dx), R.finite_rel_err(dx, ref_dx))
    j.done()


@pytest.mark.parametrize("n", R.TANH_SIZES)
def test_tanh_sizes(ops, n):
    """one thread, one short of / exactly / one past a workgroup, and 259 elements past the 4096 x 256 threads of the
    largest grid (the grid-stride loop's second pass); the special values ride along where they fit"""
    x, dy = R.tanh_inputs(n)
    if n >= len(R.TANH_SPECIAL):
        x = x.clone()
        x[-len(R.TANH_SPECIAL):] = R.tanh_special()
    xg = x.to(DEV).requires_grad_(True)
    y = ops.tanh(xg)
    y.backward(dy.to(DEV))
    inplace = ops.tanh_(x.to(DEV).clone())
    ops.check_errors()
    assert _same_bits(inplace, y.detach())                           # tanh_ in place is tanh
    _tanh_judge("tanh[n=%d]" % n, x, dy, y.detach().cpu().numpy(), xg.grad.cpu().numpy())


def test_tanh_special_values_and_saturated_backward(ops):
    """+-0, subnormals, +-9, +-100, +-inf and NaN through the C ABI inside guards; the backward with y exactly +-1"""
    L, p, st = ops._L(), ops._p, ops._stream()
    x = R.tanh_special()
    n = x.numel()
    dy = torch.linspace(-2.0, 3.0, n)
    ybuf = torch.full((n + 6,), SENT, device=DEV)
    dbuf = torch.full((n + 6,), SENT, device=DEV)
    xd, dyd = x.to(DEV), dy.to(DEV)
    _lib().check(L.asrk_tanh_fwd_f32(p(xd), p(ybuf[3:]), n, st), "tanh")
    _lib().check(L.asrk_tanh_bwd_f32(p(ybuf[3:]), p(dyd), p(dbuf[3:]), n, st), "tanh_bwd")
    ops.check_errors()
    for buf in (ybuf, dbuf):
        assert torch.equal(buf[:3], torch.full((3,), SENT, device=DEV)) and torch.equal(buf[3 + n:], buf[:3])
    y = ybuf[3:3 + n].cpu()
    assert torch.equal(y[x.abs() >= 19.0], torch.sign(x[x.abs() >= 19.0]))           # saturated: exactly +-1
    assert torch.equal(y[x == 0], x[x == 0]) and torch.equal(torch.signbit(y[x == 0]), torch.signbit(x[x == 0]))
    _tanh_judge("tanh[special]", x, dy, y.numpy(), dbuf[3:3 + n].cpu().numpy())
    ones = torch.tensor([1.0, -1.0] * 130, device=DEV)
    out = torch.full((260,), SENT, device=DEV)
    dy35 = torch.full((260,), 3.5, device=DEV)
    _lib().check(L.asrk_tanh_bwd_f32(p(ones), p(dy35), p(out), 260, st), "tanh_bwd")
    ops.check_errors()
    assert torch.equal(out, torch.zeros(260, device=DEV))
