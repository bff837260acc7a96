"""Float64 restatements and the case table of the extended optimiser step of csrc/optim.hip (asrk_*_multi_ext_f32,
asrk_avg_multi_f32, asrk_swap_multi_f32): the three decay forms and the weight average, in the style of
tests/rowops_reference.py, whose Adadelta / Adam recurrences (adadelta_reference, adam_reference) and torch runner
(torch_optim_run) are imported, not copied: with no decay and no average the functions here ARE those
(tests/test_optim_ext_cpu.py asserts it bit for bit).

Per element, c = min(coef, 1), g' = c * g:
    adadelta_l2   g' += lam * p, then Adadelta                       torch.optim.Adadelta(weight_decay=lam)
    adam_l2       g' += lam * p, then Adam                           torch.optim.Adam(weight_decay=lam)
    adamw         p *= 1 - lr * lam, then Adam on g'                 torch.optim.AdamW(weight_decay=lam)
    average       e += w * (p_new - e) after the update              e.lerp_(p, w)
A NaN coefficient leaves p, both states and e as they were (the schedule of w is the caller's and advances).
Plain numpy / torch on the CPU, no device."""
import functools

import numpy as np
import torch

import rowops_reference as R
from rowops_reference import adadelta_reference, adam_reference, torch_optim_run    # noqa: F401  (re-used, see above)

MODES = ('adadelta_l2', 'adam_l2', 'adamw')
KIND_OF = dict(adadelta_l2='adadelta', adam_l2='adam', adamw='adam')
DECAY_MODE = dict(adadelta_l2=1, adam_l2=1, adamw=2)                 # the ABI's decay_mode
LAMBDA = 0.01
STEPS = R.OPT_STEPS                                                  # six
COEFS = [('none', None), ('below', 0.7), ('above', 1.3), ('nan', float('nan'))]
AVERAGES = ('off', 'ema', 'mean')
EMA_DECAY = 0.9
KINDS = R.OPT_KINDS + ('average',)
F = dict(param=4, state0=8, state1=8, average=4)                     # tests/test_rowops_variants_gpu.py; 4 for the average

# the smallest shapes that reach every branch: one element, below / at / above one workgroup, more than one workgroup, one
# tensor over the 2048-workgroup cap (2100 x 1100 > 2048 x 1024), and a table of 53 tensors, more than two launches of 24
# slots, with empty ones among them (at the start, on both sides of a launch boundary, at the end)
SMALL = (1, 3, 255, 256, 257, 1025)
BIG = 2100 * 1100
EMPTY_AT = (0, 23, 24, 52)                                           # 49 non-empty tensors: three launches


def table_sizes():
    n = [1 + (37 * t) % 301 for t in range(53)]
    for t, s in zip((1, 2, 3, 5, 26, 50), SMALL):
        n[t] = s
    n[30] = BIG
    for t in EMPTY_AT:
        n[t] = 0
    return n


SIZES = table_sizes()
SWAP_SIZES = [n if n != BIG else 4099 for n in SIZES] + [BIG]        # the swap needs the cap once, not in the middle


def average_weights(avg, steps=STEPS, decay=EMA_DECAY, warmup=True):
    """w of update k = 1 .. steps: ema 1 - min(decay, (1 + k) / (10 + k)) (warm-up), mean 1 / (k + 1); None for 'off'"""
    if avg == 'off':
        return None
    if avg == 'mean':
        return [1.0 / (k + 1) for k in range(1, steps + 1)]
    return [1.0 - (min(decay, (1.0 + k) / (10.0 + k)) if warmup else decay) for k in range(1, steps + 1)]


def average_update(e, p, w, dtype=np.float64):
    f = dtype
    return e + f(w) * (np.asarray(p, f) - e)


def ext_reference(mode, p0, grads, coef, lam, weights=None, dtype=np.float64):
    """-> list over steps of (p, state0, state1, e); e starts as a copy of p0 (sample 1) and is None without weights.
    lam: a scalar or an array per element (a table whose tensors decay differently).  Hyper-parameters rounded as the ABI
    rounds them when dtype is float32."""
    f = dtype
    kind = KIND_OF[mode]
    hp = R.ADADELTA_HP if kind == 'adadelta' else R.ADAM_HP
    p = np.asarray(p0, f).copy()
    s0, s1 = np.zeros(len(p0), f), np.zeros(len(p0), f)
    e = p.copy() if weights is not None else None
    skip, c = R.clip_of(coef)
    c = f(c)
    lam = np.asarray(lam, np.float64)
    out = []
    for t, g in enumerate(grads, 1):
        if not skip:
            gr = np.asarray(g, f) * c
            if mode == 'adamw':
                p = p * (1.0 - hp['lr'] * lam).astype(f)             # the factor formed in double, as torch forms it
            elif f is np.float32:
                # the kernel's fused multiply-add (one rounding): the product of two float32 is exact in float64
                gr = (np.float64(gr) + np.float64(lam.astype(f)) * np.float64(p)).astype(f)
            else:
                gr = gr + lam * p
            if kind == 'adadelta':
                rho, omr, eps = f(hp['rho']), f(1.0 - hp['rho']), f(hp['eps'])
                s0 = s0 * rho + omr * gr * gr
                delta = np.sqrt(s1 + eps) / np.sqrt(s0 + eps) * gr
                s1 = s1 * rho + omr * delta * delta
                p = p - f(hp['lr']) * delta
            else:
                b1, b2 = hp['beta1'], hp['beta2']
                bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
                s0 = s0 + (gr - s0) * f(1.0 - b1)
                s1 = s1 * f(b2) + f(1.0 - b2) * gr * gr
                p = p - f(hp['lr'] / bc1) * (s0 / (np.sqrt(s1) / f(np.sqrt(bc2)) + f(hp['eps'])))
            if weights is not None:
                e = average_update(e, p, weights[t - 1], f)
        out.append((p.copy(), s0.copy(), s1.copy(), None if e is None else e.copy()))
    return out


def torch_ext_run(mode, p0, grads, coef, lam, weights, dtype):
    """torch.optim.Adadelta / Adam(weight_decay=lam) / AdamW(weight_decay=lam) on the CPU in `dtype`, the gradient scaled
    by min(coef, 1) first (clip_grad_norm_ followed by step()), the average as e.lerp_(p, w) -> as ext_reference"""
    p = torch.nn.Parameter(torch.from_numpy(np.asarray(p0)).to(dtype).clone())
    if mode == 'adadelta_l2':
        opt, keys = torch.optim.Adadelta([p], weight_decay=lam, **R.ADADELTA_HP), ('square_avg', 'acc_delta')
    else:
        cls = torch.optim.AdamW if mode == 'adamw' else torch.optim.Adam
        hp = R.ADAM_HP
        opt = cls([p], lr=hp['lr'], betas=(hp['beta1'], hp['beta2']), eps=hp['eps'], weight_decay=lam)
        keys = ('exp_avg', 'exp_avg_sq')
    skip, c = R.clip_of(coef)
    assert not skip
    e = p.detach().clone() if weights is not None else None
    out = []
    for t, g in enumerate(grads):
        p.grad = torch.from_numpy(np.asarray(g)).to(dtype) * c
        opt.step()
        if e is not None:
            e.lerp_(p.detach(), weights[t])
        st = opt.state[p]
        out.append((p.detach().numpy().copy(), st[keys[0]].numpy().copy(), st[keys[1]].numpy().copy(),
                    None if e is None else e.numpy().copy()))
    return out


@functools.lru_cache(maxsize=None)
def inputs(n, seed, steps=STEPS):
    return R.opt_inputs(n, seed, steps)


@functools.lru_cache(maxsize=1)
def expected(mode, n, seed, coef, avg, lam=LAMBDA, steps=STEPS):
    """(float64 reference, torch float32 run, e32 per tensor kind) of a case, computed once and shared by the tests that
    follow each other on it (one case of the full table is half a gigabyte: the cache holds the latest only); read-only"""
    p0, grads = inputs(n, seed, steps)
    w = average_weights(avg, steps)
    ref = ext_reference(mode, p0, grads, coef, lam, w)
    t32 = torch_ext_run(mode, p0, grads, coef, lam, w, torch.float32)
    t64 = torch_ext_run(mode, p0, grads, coef, lam, w, torch.float64)
    kinds = range(4 if w is not None else 3)
    e32 = tuple(max(R.rel_err(a[i], b[i]) for a, b in zip(t32, t64)) for i in kinds)
    return ref, t32, e32
