"""GPU: the extended optimiser step of csrc/optim.hip (weight decay, L2 and decoupled, and the weight average inside the
update kernel), the average as a launch of its own, the swap, and the classes and wrapper keys above them, on the case
table of tests/optim_ext_reference.py: tensors of 1, 3, 255, 256, 257 and 1025 elements, one of 2100 x 1100 (over the
2048-workgroup cap) in a table of 53 with empty ones among them (three launches), laid end to end with 3 floats of NaN
between them so that every alignment occurs, and the whole layout once more one float further on.

Criterion for values, per tensor kind (parameter, state 0, state 1, average), that of tests/test_rowops_variants_gpu.py:
rel_err against the float64 reference <= max(F * e32, 4 * 2**-24), e32 the rel_err of torch's own float32 CPU run
(torch.optim.Adadelta / Adam(weight_decay=) / AdamW on gradients scaled by min(coef, 1); the average as e.lerp_(p, w))
against its float64 run on the same inputs; F = 4 / 8 / 8 and 4 for the average; parameters and states also within 2e-6 of
the float32 run.  Every test prints
    OPTEXT name | kind | e32 | bound | device | device/e32
(pytest -s); the largest ratios per kind are in DESIGN.md 3.28."""
import copy
import ctypes
import importlib

import numpy as np
import pytest
import torch

from conftest import PKG_NAME
import optim_ext_reference as X
import rowops_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float('nan')
EINVAL = -1
ROLES = ('p', 's0', 's1', 'e')


def _lib():
    return importlib.import_module(PKG_NAME + "._lib")


def bits(t):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().contiguous().numpy()
    return np.ascontiguousarray(t, np.float32).view(np.int32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


class Table:
    """the tensors of a table end to end in one allocation per role, filled with NaN: `off` floats of slack in front (4:
    the first tensor 16-byte aligned, 5: everything one float further), 3 floats between tensors, 5 behind; empty entries
    are None (NULL pointers)"""

    def __init__(self, sizes, roles, off=4, data=None):
        self.sizes, self.off = list(sizes), off
        self.starts = [int(s) for s in off + np.cumsum([0] + [n + 3 for n in sizes])[:-1]]
        self.total = off + int(sum(n + 3 for n in sizes)) + 5
        self.buf = {r: torch.full((self.total,), NAN, device=DEV) for r in roles}
        self.mask = np.zeros(self.total, bool)                        # True on payload
        for s, n in zip(self.starts, sizes):
            self.mask[s:s + n] = True
        for r, flat in (data or {}).items():
            self.put(r, flat)

    def put(self, role, flat):
        full = np.full(self.total, np.nan, np.float32)
        full[self.mask] = np.asarray(flat, np.float32)
        self.buf[role].copy_(torch.from_numpy(full))

    def tensors(self, role):
        return [None if n == 0 else self.buf[role][s:s + n] for s, n in zip(self.starts, self.sizes)]

    def payload(self, role):
        return self.buf[role].cpu().numpy()[self.mask]

    def gaps_untouched(self, role):
        return bool(np.isnan(self.buf[role].cpu().numpy()[~self.mask]).all())


def _ptrs(tensors):
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def _coef_tensor(coef):
    return None if coef is None else torch.tensor([coef], dtype=torch.float32, device=DEV)


def _plain_step(ops, kind, tb, g, step, coef_t):
    L, st = ops._L(), ops._stream()
    n = (ctypes.c_int64 * len(tb.sizes))(*tb.sizes)
    arrs = [_ptrs(tb.tensors('p')), _ptrs(g.tensors('g')), _ptrs(tb.tensors('s0')), _ptrs(tb.tensors('s1'))]
    if kind == 'adadelta':
        hp = R.ADADELTA_HP
        rc = L.asrk_adadelta_multi_f32(len(tb.sizes), *arrs, n, hp['lr'], hp['rho'], hp['eps'], ops._p(coef_t), st)
    else:
        hp = R.ADAM_HP
        rc = L.asrk_adam_multi_f32(len(tb.sizes), *arrs, n, hp['lr'], hp['beta1'], hp['beta2'], hp['eps'], step,
                                   ops._p(coef_t), st)
    _lib().check(rc, kind + "_multi")


def _ext_step(ops, kind, tb, g, step, coef_t, lam, decay_mode, averaged, weight):
    """lam: None (NULL), a scalar for every tensor, or a list per tensor"""
    L, st = ops._L(), ops._stream()
    count = len(tb.sizes)
    n = (ctypes.c_int64 * count)(*tb.sizes)
    arrs = [_ptrs(tb.tensors('p')), _ptrs(g.tensors('g')), _ptrs(tb.tensors('s0')), _ptrs(tb.tensors('s1'))]
    wd = None if lam is None else (ctypes.c_float * count)(*(lam if isinstance(lam, (list, tuple)) else [lam] * count))
    avg = _ptrs(tb.tensors('e')) if averaged else None
    if kind == 'adadelta':
        hp = R.ADADELTA_HP
        rc = L.asrk_adadelta_multi_ext_f32(count, *arrs, n, hp['lr'], hp['rho'], hp['eps'], ops._p(coef_t), wd, decay_mode,
                                           avg, weight, st)
    else:
        hp = R.ADAM_HP
        rc = L.asrk_adam_multi_ext_f32(count, *arrs, n, hp['lr'], hp['beta1'], hp['beta2'], hp['eps'], step, ops._p(coef_t),
                                       wd, decay_mode, avg, weight, st)
    _lib().check(rc, kind + "_multi_ext")


def _avg_step(ops, tb, weight, coef_t):
    n = (ctypes.c_int64 * len(tb.sizes))(*tb.sizes)
    _lib().check(ops._L().asrk_avg_multi_f32(len(tb.sizes), _ptrs(tb.tensors('e')), _ptrs(tb.tensors('p')), n, weight,
                                             ops._p(coef_t), ops._stream()), "avg_multi")


def _fresh(sizes, off, p0, roles=ROLES):
    zeros = np.zeros(len(p0), np.float32)
    return Table(sizes, roles, off, dict(p=p0, s0=zeros, s1=zeros, e=p0))


def _grad_tables(sizes, off, grads):
    return [Table(sizes, ('g',), off, dict(g=g)) for g in grads]


# ====================================================================================================== values
SEED = 53
VALUE_CASES = [(m, a, cn, c, 0) for m in X.MODES for a in X.AVERAGES for cn, c in X.COEFS] + \
              [(m, a, 'below', 0.7, 1) for m in X.MODES for a in X.AVERAGES]


@pytest.mark.parametrize("mode,avg,coef_name,coef,mis", VALUE_CASES,
                         ids=["%s-%s-%s-off%d" % (c[0], c[1], c[2], c[4]) for c in VALUE_CASES])
def test_values_against_float64(ops, mode, avg, coef_name, coef, mis):
    """six steps of every mode x average through the extended entry on the whole table; with a NaN coefficient nothing may
    change, the average included"""
    sizes, total = X.SIZES, sum(X.SIZES)
    kind = X.KIND_OF[mode]
    p0, grads = X.inputs(total, SEED)
    weights = X.average_weights(avg)
    tb = _fresh(sizes, 4 + mis, p0)
    coef_t = _coef_tensor(coef)
    runs = []
    for step, g in enumerate(_grad_tables(sizes, 4 + mis, grads), 1):
        _ext_step(ops, kind, tb, g, step, coef_t, X.LAMBDA, X.DECAY_MODE[mode], weights is not None,
                  weights[step - 1] if weights else 0.0)
        ops.check_errors()
        runs.append(tuple(tb.payload(r) for r in ROLES))
        assert same_bits(g.payload('g'), grads[step - 1])             # gradients are read-only
    assert all(tb.gaps_untouched(r) for r in ROLES)
    if R.clip_of(coef)[0]:
        for p, s0, s1, e in runs:
            assert same_bits(p, p0) and not s0.any() and not s1.any() and same_bits(e, p0)
        return
    if weights is None:
        assert all(same_bits(r[3], p0) for r in runs)                 # no average attached: e is not written
    ref, t32, e32 = X.expected(mode, total, SEED, coef, avg)
    bad = []
    for i, k in enumerate(X.KINDS[:len(e32)]):
        err = max(R.rel_err(r[i], f[i]) for r, f in zip(runs, ref))
        hard = max(R.rel_err(r[i], t[i]) for r, t in zip(runs, t32))
        b = R.bound(e32[i], X.F[k])
        print("OPTEXT %s[%s %s off%d] | %s | e32 %.3e | bound %.3e | device %.3e | device/e32 %.2f" % (
            mode, avg, coef_name, mis, k, e32[i], b, err, err / e32[i] if e32[i] > 0 else NAN))
        if not err <= b or (k != 'average' and not hard < R.OPT_HARD):
            bad.append((k, err, b, hard))
    assert not bad, bad


# ====================================================================================================== identities
@pytest.mark.parametrize("lam,decay_mode", [(None, 0), (0.0, 1), (0.01, 0)], ids=['null', 'zeros', 'mode0'])
@pytest.mark.parametrize("kind", ['adadelta', 'adam'])
def test_extended_entry_switched_off_is_the_plain_entry(ops, kind, lam, decay_mode):
    """lam = 0 everywhere (or decay_mode 0 whatever the table says), no average: parameters and state bit for bit"""
    sizes, total = X.SIZES, sum(X.SIZES)
    p0, grads = X.inputs(total, SEED)
    a, b = _fresh(sizes, 5, p0), _fresh(sizes, 5, p0)
    coef_t = _coef_tensor(0.7)
    for step, g in enumerate(_grad_tables(sizes, 5, grads[:2]), 1):
        _plain_step(ops, kind, a, g, step, coef_t)
        _ext_step(ops, kind, b, g, step, coef_t, lam, decay_mode, False, 0.0)
        ops.check_errors()
        for r in ROLES:
            assert torch.equal(a.buf[r].view(torch.int32), b.buf[r].view(torch.int32)), (kind, step, r)
    assert not same_bits(a.payload('p'), p0)


@pytest.mark.parametrize("coef", [None, 0.7])
@pytest.mark.parametrize("kind", ['adadelta', 'adam'])
def test_fused_average_is_the_separate_launch(ops, kind, coef):
    """the plain entry followed by asrk_avg_multi_f32 against one fused launch: p, state and e bit for bit"""
    sizes, total = X.SIZES, sum(X.SIZES)
    p0, grads = X.inputs(total, SEED)
    a, b = _fresh(sizes, 5, p0), _fresh(sizes, 5, p0)
    coef_t = _coef_tensor(coef)
    weights = X.average_weights('ema')
    for step, g in enumerate(_grad_tables(sizes, 5, grads[:3]), 1):
        _plain_step(ops, kind, a, g, step, coef_t)
        _avg_step(ops, a, weights[step - 1], coef_t)
        _ext_step(ops, kind, b, g, step, coef_t, None, 0, True, weights[step - 1])
        ops.check_errors()
        for r in ROLES:
            assert torch.equal(a.buf[r].view(torch.int32), b.buf[r].view(torch.int32)), (kind, step, r)
    assert not same_bits(a.payload('e'), p0) and not same_bits(a.payload('e'), a.payload('p'))


@pytest.mark.parametrize("mode", X.MODES)
def test_nan_coefficient_leaves_all_four_untouched(ops, mode):
    """after a clean step (so that the state is not zero): a NaN coefficient leaves p, both states and e bit-identical, in
    the fused launch and in the separate one; the next clean step moves all four"""
    sizes = [n for n in X.SIZES if n != X.BIG] + [4099]
    total = sum(sizes)
    kind = X.KIND_OF[mode]
    p0, grads = X.inputs(total, 7, 3)
    tb = _fresh(sizes, 5, p0)
    gts = _grad_tables(sizes, 5, grads)
    _ext_step(ops, kind, tb, gts[0], 1, _coef_tensor(0.7), X.LAMBDA, X.DECAY_MODE[mode], True, 0.25)
    before = {r: bits(tb.buf[r]).copy() for r in ROLES}
    nan_t = _coef_tensor(NAN)
    _ext_step(ops, kind, tb, gts[1], 2, nan_t, X.LAMBDA, X.DECAY_MODE[mode], True, 0.25)
    _avg_step(ops, tb, 0.25, nan_t)
    ops.check_errors()
    for r in ROLES:
        assert np.array_equal(bits(tb.buf[r]), before[r]), (mode, r)
    _ext_step(ops, kind, tb, gts[2], 3, _coef_tensor(0.7), X.LAMBDA, X.DECAY_MODE[mode], True, 0.25)
    ops.check_errors()
    for r in ROLES:
        moved = np.split(bits(tb.payload(r)) != before[r][tb.mask], np.cumsum(sizes)[:-1])
        assert all(m.any() for m, n in zip(moved, sizes) if n), (mode, r)
        assert tb.gaps_untouched(r)


@pytest.mark.parametrize("mis", [0, 1])
def test_swap_exchanges_exactly_and_twice_is_the_identity(ops, mis):
    sizes, total = X.SWAP_SIZES, sum(X.SWAP_SIZES)
    a0, b0 = R.opt_inputs(total, 21, 1)
    b0 = b0[0]
    a0[::97], b0[::89] = -0.0, np.float32(NAN)                        # bit patterns arithmetic would not keep
    tb = Table(sizes, ('a', 'b'), 4 + mis, dict(a=a0, b=b0))
    n = (ctypes.c_int64 * len(sizes))(*sizes)

    def swap():
        _lib().check(ops._L().asrk_swap_multi_f32(len(sizes), _ptrs(tb.tensors('a')), _ptrs(tb.tensors('b')), n,
                                                  ops._stream()), "swap_multi")
        ops.check_errors()
    swap()
    assert same_bits(tb.payload('a'), b0) and same_bits(tb.payload('b'), a0)
    assert tb.gaps_untouched('a') and tb.gaps_untouched('b')
    swap()
    assert same_bits(tb.payload('a'), a0) and same_bits(tb.payload('b'), b0)
    assert tb.gaps_untouched('a') and tb.gaps_untouched('b')


def test_invalid_entry_beyond_the_first_launch_leaves_everything_alone(ops):
    """entry 27 of 30 with a negative weight decay: ASRK_EINVAL, and the 24 tensors of the first launch are not stepped"""
    sizes = [40 + 3 * t for t in range(30)]
    p0, grads = X.inputs(sum(sizes), 30, 1)
    tb = _fresh(sizes, 5, p0)
    g = _grad_tables(sizes, 5, grads)[0]
    before = {r: bits(tb.buf[r]).copy() for r in ROLES}
    lam = [0.01] * 30
    lam[27] = -0.01
    with pytest.raises(_lib().AsrkError):
        _ext_step(ops, 'adam', tb, g, 1, None, lam, 1, True, 0.5)
    ops.check_errors()
    for r in ROLES:
        assert np.array_equal(bits(tb.buf[r]), before[r]), r


# ====================================================================================================== classes
def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    shapes = [(33, 5), (7,), (128, 64), (64,), (3, 4, 3, 3), (1,)]
    return [torch.randn(*s, generator=g) for s in shapes]


@pytest.mark.parametrize("name", ['Adadelta', 'Adam', 'AdamW'])
def test_decay_min_dim_exempts_the_one_dimensional_tensors(ops, pkg, name):
    """group key decay_min_dim = 2: the 1-D tensors take the weight_decay = 0 result bit for bit, the others the result of
    decaying everything, which is not the weight_decay = 0 one"""
    fo = importlib.import_module(pkg.__name__ + ".fused_optim")
    base = _params()
    runs = {}
    for label, lam, min_dim in (('exempt', 0.05, 2), ('none', 0.0, None), ('all', 0.05, None)):
        ps = [p.clone().to(DEV).requires_grad_(True) for p in base]
        opt = fo.FUSED[name](ps, lr=0.01, weight_decay=lam)
        if min_dim is not None:
            opt.param_groups[0]['decay_min_dim'] = min_dim
        g = torch.Generator().manual_seed(1)
        for _ in range(3):
            for p in ps:
                p.grad = torch.randn(*p.shape, generator=g).to(DEV)
            opt.clip_and_step(5.0)
        ops.check_errors()
        runs[label] = [p.detach().cpu() for p in ps]
    for i, p in enumerate(base):
        if p.dim() < 2:
            assert same_bits(runs['exempt'][i], runs['none'][i]), (name, i)
        else:
            assert same_bits(runs['exempt'][i], runs['all'][i]) and not same_bits(runs['exempt'][i], runs['none'][i]), (name, i)


@pytest.mark.parametrize("name,kw", [('Adadelta', dict(lr=1.0, weight_decay=0.02)), ('Adam', dict(lr=0.01, weight_decay=0.02)),
                                     ('AdamW', dict(lr=0.01, weight_decay=0.1)), ('AdamW', dict(lr=0.01))])
def test_fused_classes_with_decay_match_torch(ops, pkg, name, kw):
    """more tensors than one launch holds, some without a gradient on some steps (Adam: sub-launches per step count)"""
    fo = importlib.import_module(pkg.__name__ + ".fused_optim")
    g = torch.Generator().manual_seed(5)
    shapes = [((3 + i, 5) if i % 9 != 4 else (0, 5)) for i in range(30)]
    ps_ref = [torch.randn(*s, generator=g).requires_grad_(True) for s in shapes]
    ps_dev = [p.detach().clone().to(DEV).requires_grad_(True) for p in ps_ref]
    o_ref, o_dev = getattr(torch.optim, name)(ps_ref, foreach=False, **kw), fo.FUSED[name](ps_dev, **kw)
    for step in range(3):
        for i, (pr, pd) in enumerate(zip(ps_ref, ps_dev)):
            if i % 7 == 3 and step != 1:
                pr.grad, pd.grad = None, None
                continue
            gr = torch.randn(*pr.shape, generator=g)
            pr.grad, pd.grad = gr.clone(), gr.clone().to(DEV)
        o_ref.step()
        o_dev.step()
        for pr, pd in zip(ps_ref, ps_dev):
            if pr.numel():
                assert R.rel_err(pd.detach().cpu().numpy(), pr.detach().numpy()) < 2e-6
    assert o_ref.state_dict()['param_groups'][0].keys() == o_dev.state_dict()['param_groups'][0].keys()


def test_adamw_state_dict_round_trip_between_torch_and_fused(ops, pkg):
    fo = importlib.import_module(pkg.__name__ + ".fused_optim")
    g = torch.Generator().manual_seed(3)
    p_t = [torch.randn(16, 8, generator=g).to(DEV).requires_grad_(True)]
    p_f = [p_t[0].detach().clone().requires_grad_(True)]
    kw = dict(lr=0.01, eps=1e-8, weight_decay=0.1)
    o_t, o_f = torch.optim.AdamW(p_t, **kw), fo.FusedAdamW(p_f, **kw)
    assert isinstance(o_f, torch.optim.AdamW) and fo.FUSED['AdamW'] is fo.FusedAdamW
    for o, p in ((o_t, p_t), (o_f, p_f)):
        p[0].grad = torch.ones_like(p[0])
        o.step()
    assert o_t.state_dict()['param_groups'] == o_f.state_dict()['param_groups']
    # fused state -> torch optimiser and back: the next steps agree.  Copies: load_state_dict keeps a tensor that already
    # has the parameter's device and dtype, so without them both optimisers would step the same exp_avg and step count
    o_t.load_state_dict(copy.deepcopy(o_f.state_dict()))
    o_f.load_state_dict(copy.deepcopy(o_t.state_dict()))
    assert o_t.state[p_t[0]]['exp_avg'].data_ptr() != o_f.state[p_f[0]]['exp_avg'].data_ptr()
    for o, p in ((o_t, p_t), (o_f, p_f)):
        p[0].grad = torch.full_like(p[0], 0.3)
        o.step()
    assert R.rel_err(p_f[0].detach().cpu().numpy(), p_t[0].detach().cpu().numpy()) < 2e-6


# ====================================================================================================== wrapper
class _Recorder:
    """the loaded library with the names of the entry points fetched from it"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        if name.startswith('asrk_'):
            self.calls.append(name)
        return getattr(self._lib, name)


@pytest.fixture
def route(ops, pkg, monkeypatch):
    fo = importlib.import_module(pkg.__name__ + ".fused_optim")
    rec = _Recorder(ops._L())
    monkeypatch.setattr(fo, '_L', lambda: rec)
    monkeypatch.setattr(ops, '_L', lambda: rec)
    return rec


def _steps(o, ps, n, seed=2, clip=True):
    fo = importlib.import_module(PKG_NAME + ".fused_optim")
    g = torch.Generator().manual_seed(seed)
    its = [[p.detach().clone() for p in ps]]
    for step in range(n):
        o.pre_step(step)
        for p in ps:
            p.grad = torch.randn(*p.shape, generator=g).to(DEV)
        if clip and o.fused:
            norm, coef = fo.grad_norm_and_coef(ps, 5.0)
            o.step(norm, 5.0, coef=coef)
        else:
            o.step()
        its.append([p.detach().clone() for p in ps])
    return its


def test_wrapper_routes(ops, pkg, route):
    optim = importlib.import_module(pkg.__name__ + ".src.optim")
    fo = importlib.import_module(pkg.__name__ + ".fused_optim")
    new = lambda: [torch.nn.Parameter(t.to(DEV)) for t in _params()]
    step_calls = lambda: [c for c in route.calls if 'multi' in c and 'grad_norm' not in c]
    # without the keys: today's call, for the three classes
    for name, entry in (('Adadelta', 'asrk_adadelta_multi_f32'), ('Adam', 'asrk_adam_multi_f32')):
        ps = new()
        o = optim.Optimizer([{'params': iter(ps)}], name, 0.01, 1e-8, 'fixed')
        assert o.fused and o.average is None and 'decay_min_dim' not in o.opt.param_groups[0]
        route.calls.clear()
        _steps(o, ps, 2)
        assert step_calls() == [entry, entry]
    # AdamW with weight_decay is fused and decoupled, and exempts the 1-D tensors by default
    ps = new()
    o = optim.Optimizer([{'params': iter(ps)}], 'AdamW', 0.01, 1e-8, 'fixed', weight_decay=0.01)
    assert o.fused and isinstance(o.opt, fo.FusedAdamW) and o.opt.param_groups[0]['decay_min_dim'] == 2
    assert o.opt.param_groups[0]['weight_decay'] == 0.01 and not o.device_nan_skip
    route.calls.clear()
    _steps(o, ps, 2)
    assert step_calls() == ['asrk_adam_multi_ext_f32'] * 2
    # averaging on: the extended entry from the step the average starts at, the plain one before it
    ps = new()
    o = optim.Optimizer([{'params': iter(ps)}], 'Adadelta', 1.0, 1e-8, 'fixed',
                        average=dict(enable=True, mode='mean', start_step=1))
    route.calls.clear()
    its = _steps(o, ps, 4)
    assert step_calls() == ['asrk_adadelta_multi_f32'] + ['asrk_adadelta_multi_ext_f32'] * 3
    assert o.average.k == 3
    for i, e in enumerate(o.average.tensors[0]):                       # the mean of the iterates from step 1 on
        want = torch.stack([it[i].double() for it in its[1:]]).mean(0)
        assert R.rel_err(e.cpu().numpy(), want.cpu().numpy()) < 1e-6
    # not fused: torch's own step, the average by the launch of its own
    ps = new()
    o = optim.Optimizer([{'params': iter(ps)}], 'Adadelta', 1.0, 1e-8, 'fixed', fused_step=False,
                        average=dict(enable=True, mode='ema', decay=0.5, warmup=False))
    assert not o.fused
    route.calls.clear()
    its = _steps(o, ps, 3)
    assert step_calls() == ['asrk_avg_multi_f32'] * 3
    for i, e in enumerate(o.average.tensors[0]):
        want = its[0][i].double()
        for it in its[1:]:
            want = 0.5 * want + 0.5 * it[i].double()
        assert R.rel_err(e.cpu().numpy(), want.cpu().numpy()) < 1e-6


def test_weight_average_swap_applied_and_state_dict(ops, pkg):
    optim = importlib.import_module(pkg.__name__ + ".src.optim")
    ps = [torch.nn.Parameter(t.to(DEV)) for t in _params()]
    o = optim.Optimizer([{'params': iter(ps)}], 'Adam', 0.01, 1e-8, 'fixed', average=dict(enable=True, decay=0.9))
    _steps(o, ps, 3)
    avg = o.average
    live = [p.detach().clone() for p in ps]
    mean = [e.clone() for e in avg.tensors[0]]
    assert not any(torch.equal(a, b) for a, b in zip(live, mean))
    with avg.applied():
        assert avg.swapped and all(same_bits(p, m) for p, m in zip(ps, mean))
        assert all(same_bits(e, l) for e, l in zip(avg.tensors[0], live))
        with pytest.raises(RuntimeError):
            avg.state_dict()
    assert not avg.swapped and all(same_bits(p, l) for p, l in zip(ps, live))
    with pytest.raises(KeyError):
        with avg.applied():
            raise KeyError('body')
    assert not avg.swapped and all(same_bits(p, l) for p, l in zip(ps, live))
    assert all(same_bits(e, m) for e, m in zip(avg.tensors[0], mean))
    sd = avg.state_dict()
    assert sd['k'] == 3 and sd['mode'] == 'ema' and all(same_bits(a, b) for a, b in zip(sd['tensors'][0], mean))
