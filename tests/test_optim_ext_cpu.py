"""CPU: the float64 references of tests/optim_ext_reference.py against torch.optim, the weight-average schedules against an
explicit loop, the new `hparas` keys of src/optim.py (absent keys build today's objects), and the host-side argument checks
of the four new entry points (no GPU: every error is found before a device call)."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from conftest import PKG_NAME
import optim_ext_reference as X
import rowops_reference as R

EINVAL = -1
NAN, INF = float('nan'), float('inf')


@pytest.fixture(scope="module")
def lib():
    build = importlib.import_module(PKG_NAME + ".build")
    build.build(verbose=False)
    return importlib.import_module(PKG_NAME + "._lib")


@pytest.fixture(scope="module")
def optim():
    return importlib.import_module(PKG_NAME + ".src.optim")


# ====================================================================================================== references
def _torch_clipped_run(mode, p0, grads, max_norm, lam):
    """float64, clipping through clip_grad_norm_ itself -> (list over steps of (p, s0, s1), the gradients as clipped)"""
    p = torch.nn.Parameter(torch.from_numpy(p0).double())
    if mode == 'adadelta_l2':
        opt, keys = torch.optim.Adadelta([p], weight_decay=lam, **R.ADADELTA_HP), ('square_avg', 'acc_delta')
    else:
        hp = R.ADAM_HP
        cls = torch.optim.AdamW if mode == 'adamw' else torch.optim.Adam
        opt = cls([p], lr=hp['lr'], betas=(hp['beta1'], hp['beta2']), eps=hp['eps'], weight_decay=lam)
        keys = ('exp_avg', 'exp_avg_sq')
    out, clipped = [], []
    for g in grads:
        p.grad = torch.from_numpy(g).double()
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_([p], max_norm)
        clipped.append(p.grad.numpy().copy())
        opt.step()
        st = opt.state[p]
        out.append((p.detach().numpy().copy(), st[keys[0]].numpy().copy(), st[keys[1]].numpy().copy()))
    return out, clipped


@pytest.mark.parametrize("max_norm", [None, 3.0, 1e4])
@pytest.mark.parametrize("mode", X.MODES)
def test_references_against_torch_in_float64(mode, max_norm):
    """six steps against torch.optim.Adadelta(weight_decay=) / Adam(weight_decay=) / AdamW, the gradient clipped by
    clip_grad_norm_ first (a threshold that clips and one that does not).  The reference is given the gradients as
    clip_grad_norm_ left them (g' = c * g), so what is checked is that the decay comes after the clipping and is not
    scaled by it"""
    p0, grads = R.opt_inputs(517, 3)
    want, clipped = _torch_clipped_run(mode, p0, grads, max_norm, X.LAMBDA)
    scaled = [not np.array_equal(c, np.float64(g)) for c, g in zip(clipped, grads)]
    assert any(scaled) == (max_norm == 3.0)
    got = X.ext_reference(mode, p0, clipped, None, X.LAMBDA)
    for a, b in zip(got, want):
        for i in range(3):
            assert R.rel_err(a[i], b[i]) < 1e-12, (mode, i)
    # and the decay is there at all: without it the parameters differ
    plain = X.ext_reference(mode, p0, clipped, None, 0.0)
    assert R.rel_err(plain[-1][0], want[-1][0]) > 1e-6


@pytest.mark.parametrize("coef", [None, 0.7, 1.3])
@pytest.mark.parametrize("mode", X.MODES)
def test_reference_follows_torch_with_a_fixed_coefficient(mode, coef):
    """the form the GPU tests use (one coefficient for all six steps), with the average: float64 against torch's"""
    p0, grads = R.opt_inputs(300, 4)
    w = X.average_weights('ema')
    got = X.ext_reference(mode, p0, grads, coef, X.LAMBDA, w)
    want = X.torch_ext_run(mode, p0, grads, coef, X.LAMBDA, w, torch.float64)
    for a, b in zip(got, want):
        for i in range(4):
            assert R.rel_err(a[i], b[i]) < 1e-12, (mode, coef, i)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("coef", [None, 0.37, NAN])
def test_without_decay_and_average_the_reference_is_the_plain_one(coef, dtype):
    """lam = 0: the restatement here and the imported recurrences of tests/rowops_reference.py agree bit for bit"""
    p0, grads = R.opt_inputs(200, 6)
    for mode, plain, hp in (('adadelta_l2', X.adadelta_reference, R.ADADELTA_HP), ('adam_l2', X.adam_reference, R.ADAM_HP),
                            ('adamw', X.adam_reference, R.ADAM_HP)):
        got = X.ext_reference(mode, p0, grads, coef, 0.0, None, dtype)
        want = plain(p0, grads, coef, dtype=dtype, **hp)
        for a, b in zip(got, want):
            for i in range(3):
                assert np.array_equal(a[i], b[i]) and a[i].dtype == b[i].dtype, (mode, i)
            assert a[3] is None
    if coef == coef:
        for kind, mode in (('adadelta', 'adadelta_l2'), ('adam', 'adam_l2')):
            a = X.torch_ext_run(mode, p0, grads, coef, 0.0, None, torch.float64)
            b = X.torch_optim_run(kind, p0, grads, coef, torch.float64)
            assert all(np.array_equal(x[i], y[i]) for x, y in zip(a, b) for i in range(3))


def test_nan_coefficient_freezes_the_reference():
    p0, grads = R.opt_inputs(50, 8)
    for mode in X.MODES:
        for p, s0, s1, e in X.ext_reference(mode, p0, grads, NAN, X.LAMBDA, X.average_weights('mean')):
            assert np.array_equal(p, np.float64(p0)) and not s0.any() and not s1.any() and np.array_equal(e, np.float64(p0))


# ====================================================================================================== the average
def test_average_update_and_both_schedules_against_an_explicit_loop(optim):
    g = np.random.RandomState(0)
    iterates = g.standard_normal((9, 40))                             # p_0 (the copy, sample 1) and eight updates
    # mean: after n updates the float64 mean of the n + 1 iterates
    e = iterates[0].copy()
    for k in range(1, 9):
        w = optim.average_weight('mean', k)
        assert w == 1.0 / (k + 1)
        e = X.average_update(e, iterates[k], w)
        assert np.allclose(e, iterates[:k + 1].mean(0), rtol=1e-13, atol=1e-15)
    # ema with warm-up: d_k = min(decay, (1 + k) / (10 + k)), written out
    e, want = iterates[0].copy(), iterates[0].copy()
    for k in range(1, 9):
        d = min(0.9, (1.0 + k) / (10.0 + k))
        w = optim.average_weight('ema', k, decay=0.9, warmup=True)
        assert w == pytest.approx(1.0 - d, abs=1e-15)
        e = X.average_update(e, iterates[k], w)
        want = d * want + (1.0 - d) * iterates[k]
        assert np.allclose(e, want, rtol=1e-13, atol=1e-15)
    assert [optim.average_weight('ema', k, decay=0.9, warmup=True) for k in (1, 80, 81, 82)] == pytest.approx(
        [1 - 2 / 11, 1 - 81 / 90, 1 - 0.9, 1 - 0.9])                  # the warm-up meets decay = 0.9 at k = 80
    assert optim.average_weight('ema', 1, decay=0.75, warmup=False) == 0.25
    # the case table's schedule is the product's
    for avg in ('ema', 'mean'):
        assert X.average_weights(avg) == [optim.average_weight(avg, k, decay=X.EMA_DECAY) for k in range(1, X.STEPS + 1)]


def test_case_table():
    n = X.SIZES
    assert len(n) == 53 and all(s in n for s in X.SMALL) and X.BIG in n and X.BIG > R.STEP_CAP
    assert all(n[t] == 0 for t in X.EMPTY_AT) and len([s for s in n if s]) > 2 * R.MT_MAX
    assert X.BIG in X.SWAP_SIZES and 0 in X.SWAP_SIZES


# ====================================================================================================== config parsing
class Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(6, 3)
        self.norm = torch.nn.LayerNorm(3)
        self.emb = torch.nn.Embedding(5, 3)


BASE = dict(optimizer='Adadelta', lr=1.0, eps=1e-8, lr_scheduler='fixed')


def test_absent_keys_build_todays_objects(optim):
    net = Net()
    for name in ('Adadelta', 'Adam', 'AdamW'):
        o = optim.Optimizer(net.parameters(), **dict(BASE, optimizer=name), valid_step=10, max_step=20)
        ref = getattr(torch.optim, name)(net.parameters(), lr=1.0, eps=1e-8)
        assert type(o.opt) is type(ref) and not o.fused and o.average is None
        assert o.opt.param_groups[0].keys() == ref.param_groups[0].keys()
        assert {k: v for k, v in o.opt.param_groups[0].items() if k != 'params'} == \
               {k: v for k, v in ref.param_groups[0].items() if k != 'params'}
    assert optim.Optimizer(net.parameters(), **BASE, average={'enable': False, 'mode': 'nonsense'}).average is None


@pytest.mark.parametrize("kw,key", [
    (dict(average=dict(enable=True, decay=0.0)), 'average.decay'),
    (dict(average=dict(enable=True, decay=1.0)), 'average.decay'),
    (dict(average=dict(enable=True, decay=NAN)), 'average.decay'),
    (dict(average=dict(enable=True, mode='median')), 'average.mode'),
    (dict(average=dict(enable=True, start_step=-1)), 'average.start_step'),
    (dict(weight_decay=-0.01), 'weight_decay'),
    (dict(weight_decay=NAN), 'weight_decay'),
    (dict(weight_decay=INF), 'weight_decay'),
    (dict(weight_decay=0.01, weight_decay_min_dim=-1), 'weight_decay_min_dim'),
    (dict(weight_decay=0.01, weight_decay_min_dim=0, decoupled_weight_decay=True), 'decoupled_weight_decay'),
])
def test_invalid_values_raise_value_error_naming_the_key(optim, kw, key):
    with pytest.raises(ValueError, match=key.replace('.', r'\.')):
        optim.Optimizer(Net().parameters(), **BASE, **kw)


def test_weight_decay_reaches_the_optimiser_and_min_dim_picks_the_tensors(optim):
    fo = importlib.import_module(PKG_NAME + ".fused_optim")
    net = Net()
    # not fused (CPU parameters): torch's classes decay every tensor of a group, so an exemption is refused, not ignored
    with pytest.raises(ValueError, match='weight_decay_min_dim'):
        optim.Optimizer(net.parameters(), **dict(BASE, optimizer='AdamW'), weight_decay=0.05)
    o = optim.Optimizer(net.parameters(), **dict(BASE, optimizer='AdamW'), weight_decay=0.05, weight_decay_min_dim=0)
    g = o.opt.param_groups[0]
    assert type(o.opt) is torch.optim.AdamW and g['weight_decay'] == 0.05 and 'decay_min_dim' not in g
    assert optim.Optimizer(net.parameters(), **BASE, weight_decay=0.0, weight_decay_min_dim=0).opt.param_groups[0]['weight_decay'] == 0
    # the selection the fused step makes, on the group the wrapper would hand it
    names = dict((p, n) for n, p in net.named_parameters())
    for min_dim, want in ((2, {'lin.weight', 'emb.weight'}), (1, set(names.values())), (0, set(names.values())), (3, set())):
        group = dict(g, decay_min_dim=min_dim)
        assert {names[p] for p in g['params'] if fo.tensor_decay(group, p) == 0.05} == want
        assert all(fo.tensor_decay(group, p) in (0.0, 0.05) for p in g['params'])
    assert all(fo.tensor_decay(g, p) == 0.05 for p in g['params'])     # key absent: torch's behaviour
    # the fused classes take the keys torch's take (param_groups stay interchangeable)
    f = fo.FUSED['AdamW'](net.parameters(), lr=1e-3, weight_decay=0.05)
    t = torch.optim.AdamW(net.parameters(), lr=1e-3, weight_decay=0.05)
    assert f.param_groups[0].keys() == t.param_groups[0].keys() and f.state_dict()['param_groups'] == t.state_dict()['param_groups']


def test_weight_average_bookkeeping_without_a_device(optim):
    """start_step, the count of attempted updates and the state dict's mismatch check (no launch: the optimiser is never
    stepped here)"""
    net = Net()
    o = optim.Optimizer(net.parameters(), **BASE, average=dict(enable=True, mode='mean', start_step=2))
    a = o.average
    assert isinstance(a, optim.WeightAverage) and not a.started() and a.k == 0 and a.mode == 'mean'
    a.start()
    assert a.started() and [len(t) for t in a.tensors] == [len(list(net.parameters()))]
    assert all(torch.equal(e, p) and e.data_ptr() != p.data_ptr() for e, p in zip(a.tensors[0], net.parameters()))
    assert [a.next_weight() for _ in range(3)] == [1 / 2, 1 / 3, 1 / 4] and a.k == 3
    sd = a.state_dict()
    assert sd['mode'] == 'mean' and sd['k'] == 3 and len(sd['tensors'][0]) == len(a.tensors[0])
    b = optim.Optimizer(Net().parameters(), **BASE, average=dict(enable=True, mode='mean')).average
    b.load_state_dict(sd)
    assert b.k == 3 and all(torch.equal(x, y) for x, y in zip(b.tensors[0], a.tensors[0]))
    c = optim.Optimizer(Net().parameters(), **BASE, average=dict(enable=True, mode='ema')).average
    with pytest.raises(ValueError, match=r'average\.mode'):
        c.load_state_dict(sd)


# ====================================================================================================== argument errors
def _tables(count, n=8):
    fake = [4096 + 64 * t for t in range(count)]
    arr = lambda: (ctypes.c_void_p * count)(*fake)
    return arr, (ctypes.c_int64 * count)(*([n] * count)), (ctypes.c_float * count)(*([0.01] * count))


def _adadelta(L, count, p, g, s0, s1, n, wd, mode, avg, w):
    return L.asrk_adadelta_multi_ext_f32(count, p, g, s0, s1, n, 1.0, 0.95, 1e-8, None, wd, mode, avg, w, None)


def _adam(L, count, p, g, s0, s1, n, wd, mode, avg, w, step=1):
    return L.asrk_adam_multi_ext_f32(count, p, g, s0, s1, n, 1e-3, 0.9, 0.999, 1e-8, step, None, wd, mode, avg, w, None)


@pytest.mark.parametrize("entry", ['adadelta', 'adam'])
def test_step_entries_argument_errors_without_gpu(lib, entry):
    """every error case of the header, each ASRK_EINVAL before a device call (the pointers are not addresses of anything)"""
    L = lib.load()
    call = _adadelta if entry == 'adadelta' else _adam
    arr, n, wd = _tables(3)
    ok = [3, arr(), arr(), arr(), arr(), n, wd, 1, arr(), 0.5]
    assert call(L, 0, *ok[1:]) == 0                                  # empty table: nothing to do
    assert call(L, -1, *ok[1:]) == EINVAL
    for pos in (1, 2, 3, 4, 5):                                      # a NULL table
        a = list(ok)
        a[pos] = None
        assert call(L, *a) == EINVAL, pos
    a = list(ok)
    a[5] = (ctypes.c_int64 * 3)(8, -1, 8)                            # negative numel
    assert call(L, *a) == EINVAL
    for pos in (1, 2, 3, 4):                                         # a non-empty tensor with a NULL pointer
        a = list(ok)
        a[pos] = (ctypes.c_void_p * 3)(4096, None, 8192)
        assert call(L, *a) == EINVAL, pos
    for bad in (-0.01, NAN, INF, -INF):                              # lambda < 0 or not finite
        a = list(ok)
        a[6] = (ctypes.c_float * 3)(0.01, bad, 0.0)
        assert call(L, *a) == EINVAL, bad
    for bad in (-1e-9, 1.0 + 1e-9, NAN, INF):                        # avg_weight outside [0, 1] or not finite
        a = list(ok)
        a[9] = bad
        assert call(L, *a) == EINVAL, bad
        a[8] = None                                                  # also without an average
        assert call(L, *a) == EINVAL, bad
    for bad in (-1, 3):                                              # decay_mode outside 0..2
        a = list(ok)
        a[7] = bad
        assert call(L, *a) == EINVAL, bad
    a = list(ok)
    a[7] = 2
    if entry == 'adadelta':
        assert call(L, *a) == EINVAL                                 # decoupled decay is Adam's
        assert call(L, 0, *a[1:]) == EINVAL                          # ... whatever the table holds
    else:
        assert _adam(L, *ok, step=0) == EINVAL
    # all of these on an empty table of non-empty entries too: the scalars are checked first
    assert call(L, 0, *ok[1:9], 2.0) == EINVAL


def test_avg_and_swap_argument_errors_without_gpu(lib):
    L = lib.load()
    arr, n, _ = _tables(3)
    assert L.asrk_avg_multi_f32(0, arr(), arr(), n, 0.5, None, None) == 0
    assert L.asrk_swap_multi_f32(0, arr(), arr(), n, None) == 0
    assert L.asrk_avg_multi_f32(-1, arr(), arr(), n, 0.5, None, None) == EINVAL
    assert L.asrk_swap_multi_f32(-1, arr(), arr(), n, None) == EINVAL
    neg = (ctypes.c_int64 * 3)(8, 8, -2)
    hole = (ctypes.c_void_p * 3)(4096, 8192, None)
    for a, b, c in ((None, arr(), n), (arr(), None, n), (arr(), arr(), None), (arr(), arr(), neg), (hole, arr(), n),
                    (arr(), hole, n)):
        assert L.asrk_avg_multi_f32(3, a, b, c, 0.5, None, None) == EINVAL
        assert L.asrk_swap_multi_f32(3, a, b, c, None) == EINVAL
    for bad in (-1e-9, 1.0 + 1e-9, NAN, INF):
        assert L.asrk_avg_multi_f32(3, arr(), arr(), n, bad, None, None) == EINVAL
        assert L.asrk_avg_multi_f32(0, arr(), arr(), n, bad, None, None) == EINVAL
