"""Fused optimiser steps over the gfx950 kernels of csrc/optim.hip.

`FusedAdadelta` / `FusedAdam` subclass the torch optimisers (same constructor, same `state` /
`state_dict()` layout, so checkpoints written by either side load in the other) and replace
`step()` by one streaming kernel launch per param_group (all its tensors in one call).  `clip_and_step()` folds
`torch.nn.utils.clip_grad_norm_` (src/solver.py:84) into that pass: the global norm is reduced once,
the clipping coefficient stays on the device and the gradients are never rewritten."""
import ctypes

import torch

from . import _lib
from .ops import _L, _p, _stream


def _ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _grads(params):
    return [p.grad for p in params if p.grad is not None]


def grad_norm_and_coef(params, max_norm):
    """(2-norm over all gradients, max_norm / (norm + 1e-6)) as device scalars: what clip_grad_norm_ computes
    (src/solver.py:84), by the two-stage deterministic reduction of csrc/optim.hip (asrk_grad_norm_multi_f32)"""
    gs = [g if g.is_contiguous() else g.contiguous() for g in _grads(params)]
    dev = gs[0].device if gs else (params[0].device if params else torch.device("cpu"))
    out = torch.empty((2,), dtype=torch.float32, device=dev)
    if not gs or not gs[0].is_cuda or any(g.dtype != torch.float32 for g in gs):
        raise _lib.AsrkError("gradient norm: f32 gradients on the GPU expected")
    L = _L()
    numel = (ctypes.c_int64 * len(gs))(*[g.numel() for g in gs])
    nws = int(L.asrk_grad_norm_ws_bytes(len(gs), numel))
    ws = torch.empty((nws,), dtype=torch.uint8, device=dev)
    _lib.check(L.asrk_grad_norm_multi_f32(len(gs), _ptr_array(gs), numel, float(max_norm), _p(out[0:1]), _p(out[1:2]),
                                          _p(ws), nws, _stream()), "grad_norm")
    return out[0], out[1:2]


def total_grad_norm(params):
    """2-norm over all gradients (what clip_grad_norm_ returns), as a device scalar"""
    if not _grads(params):
        return torch.zeros((), device=params[0].device if params else "cpu")
    return grad_norm_and_coef(params, 1.0)[0]


def tensor_decay(group, p):
    """lambda_t of parameter p in `group`: the group's weight_decay where p.dim() >= the group's `decay_min_dim` (a key
    only the wrapper of src/optim.py sets; absent = 0 = torch's behaviour, everything decays), else 0 - biases and
    LayerNorm gains are exempt without splitting the group the solver clips as one"""
    return float(group.get('weight_decay', 0)) if p.dim() >= int(group.get('decay_min_dim', 0)) else 0.0


class _FusedMixin:
    _state_keys = ()
    _decoupled = False          # group flag `decoupled_weight_decay` (torch.optim.AdamW); Adadelta has none

    def _launch_group(self, group, params, grads, st0, st1, numel, coef):
        raise NotImplementedError

    def _launch_group_ext(self, group, params, grads, st0, st1, numel, coef, wd, mode, avg, weight):
        raise NotImplementedError

    def attach_average(self, tensors_by_param):
        """{parameter: f32 tensor of its shape}: from the next step on the update kernel also moves each of these
        towards the new value of its parameter, e += w * (p_new - e), w as set by set_average_weight.  A parameter
        that is not in the mapping has no average; None or {} detaches."""
        avg = dict(tensors_by_param or {})
        for p, e in avg.items():
            if not (e.is_cuda and e.dtype == torch.float32 and e.is_contiguous() and e.shape == p.shape):
                raise _lib.AsrkError("weight average: a contiguous f32 GPU tensor of the parameter's shape expected")
        self._average = avg

    def set_average_weight(self, weight):
        weight = float(weight)
        if not 0.0 <= weight <= 1.0:
            raise ValueError("average weight %r outside [0, 1]" % weight)
        self._average_weight = weight

    @torch.no_grad()
    def step(self, closure=None, clip_coef=None, clip_groups=None):
        """clip_coef: optional device scalar max_norm / (total_norm + 1e-6).  All tensors of a
        param_group go to the device in ONE call (asrk_*_multi_f32).  clip_groups = k: only the first k param_groups
        are clipped (the reference clips the model's gradients, not a plug-in's: src/solver.py:84); the others take
        their gradients as they are, but still skip the update when the coefficient is NaN.
        A group takes the extended entry (asrk_*_multi_ext_f32) only when one of its tensors decays
        (weight_decay != 0, and p.dim() >= the group's `decay_min_dim` where the wrapper set that key), the decay is
        decoupled, or an average is attached; every other group makes the plain call."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        k0, k1 = self._state_keys
        average = getattr(self, '_average', None) or {}
        unclipped = None
        if clip_coef is not None and clip_groups is not None and clip_groups < len(self.param_groups):
            unclipped = clip_coef * 0 + 1        # 1, or NaN with the coefficient: the kernels' skip predicate
        for gi, group in enumerate(self.param_groups):
            if group.get('maximize', False) or group.get('amsgrad', False):
                raise NotImplementedError("fused step: maximize / amsgrad are not used by the reference configs")
            lam = float(group.get('weight_decay', 0))
            if lam < 0 or lam != lam or lam == float('inf'):
                raise ValueError("weight_decay %r" % lam)
            decoupled = bool(group.get('decoupled_weight_decay', False))
            if decoupled and not self._decoupled:
                raise NotImplementedError("fused step: decoupled weight decay is Adam's")
            params, grads, st0, st1, wd, avg = [], [], [], [], [], []
            for p in group['params']:
                if p.grad is None:
                    continue
                if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()
                        and p.grad.dtype == torch.float32):
                    raise _lib.AsrkError("fused optimiser needs contiguous f32 parameters on the GPU")
                st = self.state[p]
                if len(st) == 0:
                    st['step'] = torch.zeros((), dtype=torch.float32)
                    st[k0] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st[k1] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st['step'] += 1
                params.append(p)
                grads.append(p.grad if p.grad.is_contiguous() else p.grad.contiguous())
                st0.append(st[k0])
                st1.append(st[k1])
                wd.append(tensor_decay(group, p))
                avg.append(average.get(p))
            if not params:
                continue
            numel = (ctypes.c_int64 * len(params))(*[p.numel() for p in params])
            coef = clip_coef if (clip_groups is None or gi < clip_groups) else unclipped
            has_avg = any(e is not None for e in avg)
            if decoupled or has_avg or any(w != 0 for w in wd):
                self._launch_group_ext(group, params, _ptr_array(params), _ptr_array(grads), _ptr_array(st0),
                                       _ptr_array(st1), numel, coef, (ctypes.c_float * len(wd))(*wd),
                                       2 if decoupled else 1,
                                       (ctypes.c_void_p * len(avg))(*[None if e is None else e.data_ptr() for e in avg])
                                       if has_avg else None,
                                       getattr(self, '_average_weight', 0.0) if has_avg else 0.0)
            else:
                self._launch_group(group, params, _ptr_array(params), _ptr_array(grads), _ptr_array(st0),
                                   _ptr_array(st1), numel, coef)
        # the parameters changed through raw pointers (no version bump): split panels of them are stale from here on
        from . import decoder_ops
        decoder_ops.drop_weight_panels()
        return loss

    def clip_and_step(self, max_norm):
        """clip_grad_norm_(params, max_norm) + step() in one pass over the gradients; returns the
        total gradient norm (device scalar).  A NaN norm poisons nothing: the caller decides whether to
        call this at all (src/solver.py:85-89 checks the norm first)."""
        params = [p for g in self.param_groups for p in g['params']]
        if not _grads(params):
            return torch.zeros((), device=params[0].device if params else "cpu")
        norm, coef = grad_norm_and_coef(params, max_norm)
        self.step(clip_coef=coef)
        return norm


class FusedAdadelta(_FusedMixin, torch.optim.Adadelta):
    _state_keys = ('square_avg', 'acc_delta')

    def _launch_group(self, group, params, pp, gp, s0, s1, numel, coef):
        _lib.check(_L().asrk_adadelta_multi_f32(len(params), pp, gp, s0, s1, numel, float(group['lr']),
                                                float(group['rho']), float(group['eps']), _p(coef),
                                                _stream()), "adadelta_multi")

    def _launch_group_ext(self, group, params, pp, gp, s0, s1, numel, coef, wd, mode, avg, weight):
        _lib.check(_L().asrk_adadelta_multi_ext_f32(len(params), pp, gp, s0, s1, numel, float(group['lr']),
                                                    float(group['rho']), float(group['eps']), _p(coef), wd, mode, avg,
                                                    float(weight), _stream()), "adadelta_multi_ext")


class FusedAdam(_FusedMixin, torch.optim.Adam):
    _state_keys = ('exp_avg', 'exp_avg_sq')
    _decoupled = True

    def _by_step(self, params):
        # one bias correction per call: tensors that joined the optimiser later (different step
        # counts) go in separate calls
        by_step = {}
        for i, p in enumerate(params):
            by_step.setdefault(int(self.state[p]['step'].item()), []).append(i)
        return by_step

    def _launch_group(self, group, params, pp, gp, s0, s1, numel, coef):
        b1, b2 = group['betas']
        for step, idx in self._by_step(params).items():
            def sub(arr, ty=ctypes.c_void_p):
                return (ty * len(idx))(*[arr[i] for i in idx])
            _lib.check(_L().asrk_adam_multi_f32(len(idx), sub(pp), sub(gp), sub(s0), sub(s1),
                                                sub(numel, ctypes.c_int64), float(group['lr']), float(b1),
                                                float(b2), float(group['eps']), step, _p(coef), _stream()),
                       "adam_multi")

    def _launch_group_ext(self, group, params, pp, gp, s0, s1, numel, coef, wd, mode, avg, weight):
        b1, b2 = group['betas']
        for step, idx in self._by_step(params).items():
            def sub(arr, ty=ctypes.c_void_p):
                return (ty * len(idx))(*[arr[i] for i in idx])
            _lib.check(_L().asrk_adam_multi_ext_f32(len(idx), sub(pp), sub(gp), sub(s0), sub(s1),
                                                    sub(numel, ctypes.c_int64), float(group['lr']), float(b1),
                                                    float(b2), float(group['eps']), step, _p(coef),
                                                    sub(wd, ctypes.c_float), mode, None if avg is None else sub(avg),
                                                    float(weight), _stream()), "adam_multi_ext")


class FusedAdamW(_FusedMixin, torch.optim.AdamW):
    """torch.optim.AdamW is Adam with the group flag decoupled_weight_decay = True: same state, same state_dict()"""
    _state_keys = FusedAdam._state_keys
    _decoupled = True
    _by_step = FusedAdam._by_step
    _launch_group = FusedAdam._launch_group
    _launch_group_ext = FusedAdam._launch_group_ext


FUSED = {'Adadelta': FusedAdadelta, 'Adam': FusedAdam, 'AdamW': FusedAdamW}
