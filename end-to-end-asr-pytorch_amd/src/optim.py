"""Optimizer wrapper with learning-rate and teacher-forcing schedules — mirror of the reference's
src/optim.py:6-82 (same constructor kwargs as the `hparas` config block, same `pre_step` /
`step` / state-dict surface).  The update itself is torch.optim (elementwise HBM-bound work on
resident parameters); the schedules are host scalars.
"""
import contextlib
import ctypes
import math
from functools import partial

import torch


def warmup_scheduler(step, init_lr, warmup_step=4000.0):
    ''' "Noam" warm-up, scaled so that the peak equals init_lr (src/optim.py:20-25) '''
    s = step + 1
    return init_lr * warmup_step ** 0.5 * min(s * warmup_step ** -1.5, s ** -0.5)


def speech_aug_scheduler(step, s_r, s_i, s_f, peak_lr):
    ''' SpecAugment schedule: ramp to peak_lr over s_r steps, hold until s_i, base-10 exponential
        decay to 0.01*peak_lr at s_f (src/optim.py:65-82) '''
    final_lr_ratio = 0.01
    cur_step = step + 1
    if cur_step < s_r:
        return peak_lr * float(cur_step) / s_r
    if cur_step < s_i:
        return peak_lr
    if cur_step <= s_f:
        decay = -math.log10(final_lr_ratio) / (s_f - s_i)
        return peak_lr * 10.0 ** (-decay * (cur_step - s_i))
    return peak_lr * final_lr_ratio


AVERAGE_MODES = ('ema', 'mean')


def parse_average(spec):
    """the `hparas.average` block -> None (absent or enable: false) or a dict of checked values"""
    if not spec or not spec.get('enable', False):
        return None
    mode = spec.get('mode', 'ema')
    if mode not in AVERAGE_MODES:
        raise ValueError("average.mode: %r is none of %s" % (mode, '|'.join(AVERAGE_MODES)))
    decay = float(spec.get('decay', 0.9999))
    if mode == 'ema' and not 0.0 < decay < 1.0:
        raise ValueError("average.decay: %r is outside (0, 1)" % decay)
    start = int(spec.get('start_step', 0))
    if start < 0:
        raise ValueError("average.start_step: %r is negative" % start)
    return dict(mode=mode, decay=decay, warmup=bool(spec.get('warmup', True)), start_step=start)


def average_weight(mode, k, decay=0.9999, warmup=True):
    """w of update k = 1, 2, ... in e += w * (p - e).  ema: 1 - d_k with d_k = min(decay, (1 + k) / (10 + k)) under
    warm-up, else decay; mean: 1 / (k + 1), the copy the average started from being sample 1."""
    if mode == 'mean':
        return 1.0 / (k + 1)
    return 1.0 - (min(decay, (1.0 + k) / (10.0 + k)) if warmup else decay)


def _ptrs(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


class WeightAverage:
    """A running average of the weights: one f32 tensor per parameter of every group the optimiser owns (the model's
    and a plug-in's; buffers are not averaged).  It starts as a copy of the weights (sample 1); update k = 1, 2, ...
    is e += w_k * (p - e) with average_weight(mode, k).  With a fused optimiser the update happens inside the step
    kernel (the new p is in a register there: 8 B per element instead of the 12 of a launch of its own); with any other
    optimiser it is one asrk_avg_multi_f32 per group after the step.

    k counts ATTEMPTED updates, on the host.  A step the device skipped for a NaN gradient norm (fused Adadelta) is
    not visible here: it advances the schedule and leaves e as it was.
    Limit: a parameter without a gradient on some step is not in that step's launch, so its average does not move on
    that step (its weight did not either, unless decay is on)."""

    def __init__(self, opt, mode='ema', decay=0.9999, warmup=True, start_step=0):
        self.opt, self.mode, self.decay, self.warmup, self.start_step = opt, mode, decay, warmup, start_step
        self.k = 0
        self.tensors = None          # per param_group: list of tensors, in the order of group['params']
        self.swapped = False         # True while the averages sit in the live parameters (inside applied())

    def groups(self):
        return [list(g['params']) for g in self.opt.param_groups]

    def started(self):
        return self.tensors is not None

    @torch.no_grad()
    def start(self):
        """the average := a copy of the weights as they are now (sample 1)"""
        self.tensors = [[p.detach().clone(memory_format=torch.contiguous_format) for p in ps] for ps in self.groups()]
        self.k = 0
        if hasattr(self.opt, 'attach_average'):
            self.opt.attach_average({p: e for ps, es in zip(self.groups(), self.tensors) for p, e in zip(ps, es)})

    def next_weight(self):
        """advance the schedule by one attempted update -> its w"""
        self.k += 1
        return average_weight(self.mode, self.k, self.decay, self.warmup)

    @torch.no_grad()
    def update_unfused(self, weight, coef=None):
        """e += w * (p - e) as a launch of its own per group (an optimiser that is not fused)"""
        from .. import _lib
        from ..ops import _L, _p, _stream
        for ps, es in zip(self.groups(), self.tensors):
            if not ps:
                continue
            if not all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() for p in ps):
                raise _lib.AsrkError("weight average needs contiguous f32 parameters on the GPU")
            numel = (ctypes.c_int64 * len(ps))(*[p.numel() for p in ps])
            _lib.check(_L().asrk_avg_multi_f32(len(ps), _ptrs(es), _ptrs(ps), numel, float(weight), _p(coef), _stream()),
                       "avg_multi")

    @torch.no_grad()
    def swap(self):
        """exchange the averages with the live weights in place (one asrk_swap_multi_f32 per group) and drop every
        cache of derived weights: the bf16 split panels of decoder_ops are keyed by data_ptr and _version, and a raw
        write changes neither.  They are the only such cache: packed and stacked weight images are rebuilt per call."""
        from .. import _lib, decoder_ops
        from ..ops import _L, _stream
        if self.tensors is None:
            raise RuntimeError("weight average: nothing to swap before the first update")
        for ps, es in zip(self.groups(), self.tensors):
            if not ps:
                continue
            if not all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() for p in ps):
                raise _lib.AsrkError("weight average needs contiguous f32 parameters on the GPU")
            numel = (ctypes.c_int64 * len(ps))(*[p.numel() for p in ps])
            _lib.check(_L().asrk_swap_multi_f32(len(ps), _ptrs(ps), _ptrs(es), numel, _stream()), "swap_multi")
        self.swapped = not self.swapped
        decoder_ops.drop_weight_panels()

    @contextlib.contextmanager
    def applied(self):
        """context manager: the averaged weights in the live model inside, the live weights back (bit-identical)
        afterwards, also when the body raises"""
        self.swap()
        try:
            yield self
        finally:
            self.swap()

    def _module_state_dict(self, module, group, averaged):
        sd = module.state_dict()
        if self.tensors is None:
            raise RuntimeError("weight average: not started")
        if averaged == self.swapped:
            return sd                     # what was asked for is what the module holds right now
        by_ptr = {p.data_ptr(): e for p, e in zip(self.groups()[group], self.tensors[group]) if p.numel()}
        for name, p in module.named_parameters():
            e = by_ptr.get(p.data_ptr())
            if e is not None and name in sd:
                sd[name] = e
        return sd

    def averaged_state_dict(self, module, group=0):
        """module.state_dict() with the averaged value of every parameter of param_group `group` (buffers as they
        are), whichever way round the swap currently is; the tensors are references, not copies"""
        return self._module_state_dict(module, group, True)

    def live_state_dict(self, module, group=0):
        """module.state_dict() with the live (last-iterate) weights, also from inside applied()"""
        return self._module_state_dict(module, group, False)

    @torch.no_grad()
    def load_averaged_state_dict(self, module, sd, group=0):
        """the averages of param_group `group` from a state dict of `module` (a checkpoint's model_avg)"""
        if self.tensors is None:
            self.start()
        by_ptr = {p.data_ptr(): e for p, e in zip(self.groups()[group], self.tensors[group]) if p.numel()}
        for name, p in module.named_parameters():
            e = by_ptr.get(p.data_ptr())
            if e is not None:
                e.copy_(sd[name])

    def state_dict(self):
        if self.swapped:
            raise RuntimeError("weight average: state_dict() inside applied() would save the live weights as the average")
        return dict(mode=self.mode, k=self.k,
                    tensors=None if self.tensors is None else [[e.clone() for e in es] for es in self.tensors])

    @torch.no_grad()
    def load_state_dict(self, sd):
        if sd['mode'] != self.mode:
            raise ValueError("average.mode: the checkpoint holds a %r average, the config asks for %r"
                             % (sd['mode'], self.mode))
        if sd['tensors'] is None:
            self.tensors, self.k = None, 0
            return
        groups = self.groups()
        if [[tuple(e.shape) for e in es] for es in sd['tensors']] != [[tuple(p.shape) for p in ps] for ps in groups]:
            raise ValueError("weight average: the checkpoint's tensors do not match the optimiser's parameters")
        self.start()
        for es, src in zip(self.tensors, sd['tensors']):
            for e, t in zip(es, src):
                e.copy_(t)
        self.k = int(sd['k'])


class Optimizer():
    def __init__(self, parameters, optimizer, lr, eps, lr_scheduler, tf_start=1, tf_end=1, tf_step=1, **kwargs):
        # scheduled sampling: linear from tf_start to tf_end over tf_step steps
        self.tf_type = tf_end != 1
        self.tf_rate = lambda step: max(tf_end, tf_start - (tf_start - tf_end) * step / tf_step)
        self.opt_type = optimizer
        self.init_lr = lr
        self.sch_type = lr_scheduler
        opt = getattr(torch.optim, optimizer)
        # Adadelta / Adam / AdamW on GPU parameters: one fused streaming kernel per tensor (same state layout)
        self.fused = False
        # True: the fused update skips itself on a NaN clipping coefficient and keeps no host-side step counter that
        # a skipped step would corrupt (Adadelta); Adam's bias correction counts steps on the host -> host-side guard
        self.device_nan_skip = False
        # weight_decay: absent -> nothing is passed (the class's own default applies); given -> as torch defines it for
        # the class (L2 for Adadelta / Adam, decoupled for AdamW), on tensors of at least weight_decay_min_dim dimensions
        extra = {}
        wd = kwargs.get('weight_decay')
        if wd is not None:
            wd = float(wd)
            if not 0.0 <= wd < float('inf'):
                raise ValueError("weight_decay: %r is negative or not finite" % wd)
            extra['weight_decay'] = wd
        if kwargs.get('decoupled_weight_decay', False) and optimizer == 'Adadelta':
            raise ValueError("decoupled_weight_decay: Adadelta has no decoupled form (use optimizer: AdamW)")
        if kwargs.get('decoupled_weight_decay', False):
            extra['decoupled_weight_decay'] = True
        min_dim = kwargs.get('weight_decay_min_dim')
        if min_dim is None:
            min_dim = 2 if wd is not None else 0
        min_dim = int(min_dim)
        if min_dim < 0:
            raise ValueError("weight_decay_min_dim: %r is negative" % min_dim)
        avg_spec = parse_average(kwargs.get('average'))
        # materialise the (possibly generator-valued) parameter spec so it can be inspected
        parameters = [dict(g, params=list(g['params'])) if isinstance(g, dict) else g for g in parameters]
        tensors = [p for g in parameters for p in (g['params'] if isinstance(g, dict) else [g])]
        if tensors and all(p.is_cuda for p in tensors) and kwargs.get('fused_step', True):
            from ..fused_optim import FUSED
            if optimizer in FUSED:
                opt = FUSED[optimizer]
                self.fused = True
                self.device_nan_skip = optimizer == 'Adadelta'
        if wd is not None and min_dim > 0 and not self.fused:
            # torch.optim has no per-tensor exemption inside a group; the group stays whole for the solver's clipping
            raise ValueError("weight_decay_min_dim: %d needs the fused optimiser (Adadelta, Adam or AdamW on the GPU "
                             "with fused_step on); use 0 to decay every tensor" % min_dim)
        if lr_scheduler == 'warmup':
            self.lr_scheduler = partial(warmup_scheduler, init_lr=lr)
            self.opt = opt(parameters, lr=1.0, **extra)
        elif lr_scheduler == 'spec-aug-basic':
            self.lr_scheduler = partial(speech_aug_scheduler, s_r=500, s_i=20000, s_f=80000, peak_lr=lr)
            self.opt = opt(parameters, lr=lr, eps=eps, **extra)
        elif lr_scheduler == 'spec-aug-double':
            self.lr_scheduler = partial(speech_aug_scheduler, s_r=1000, s_i=40000, s_f=160000, peak_lr=lr)
            self.opt = opt(parameters, lr=lr, eps=eps, **extra)
        else:
            self.lr_scheduler = None
            self.opt = opt(parameters, lr=lr, eps=eps, **extra)
        if wd is not None and min_dim > 0:
            for g in self.opt.param_groups:
                g['decay_min_dim'] = min_dim
        self.average = None if avg_spec is None else WeightAverage(self.opt, **avg_spec)
        # the step index average.start_step refers to: the one pre_step was given, else the count of step() calls
        self._n_step = 0

    def get_opt_state_dict(self):
        return self.opt.state_dict()

    def load_opt_state_dict(self, state_dict):
        self.opt.load_state_dict(state_dict)

    def pre_step(self, step):
        ''' set this step's lr, clear gradients, return the teacher-forcing rate '''
        if self.lr_scheduler is not None:
            cur_lr = self.lr_scheduler(step)
            for param_group in self.opt.param_groups:
                param_group['lr'] = cur_lr
        self.opt.zero_grad()
        self._n_step = step
        return self.tf_rate(step)

    def step(self, grad_norm=None, max_norm=None, coef=None, clip_groups=None):
        """plain step, or (fused optimisers) step with gradient clipping folded in: pass the total
        gradient norm (device scalar) and the clip threshold, or the ready clipping coefficient
        max_norm / (norm + 1e-6) as a device tensor [1] (fused_optim.grad_norm_and_coef).  clip_groups = k limits
        the clipping to the first k parameter groups (the model's; a plug-in's group is stepped unclipped).
        With `average` on, the first call at or after average.start_step makes the average a copy of the weights
        (before that call's update); every later call is one update of it."""
        avg, weight = self.average, None
        if avg is not None:
            if not avg.started():
                if self._n_step >= avg.start_step:
                    avg.start()
            if avg.started():
                weight = avg.next_weight()
                if self.fused:
                    self.opt.set_average_weight(weight)
        self._n_step += 1
        if self.fused and (grad_norm is not None or coef is not None):
            if coef is None:
                coef = (max_norm / (grad_norm + 1e-6)).to(torch.float32).reshape(1)
            if clip_groups is None:
                self.opt.step(clip_coef=coef)
            else:
                self.opt.step(clip_coef=coef, clip_groups=clip_groups)
        else:
            self.opt.step()
        if weight is not None and not self.fused:
            avg.update_unfused(weight)

    def create_msg(self):
        return ['Optim.spec.| Algo. = {}\t| Lr = {}\t (Scheduler = {})| Scheduled sampling = {}'
                .format(self.opt_type, self.init_lr, self.sch_type, self.tf_type)]
