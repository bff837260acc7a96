"""Autograd Functions of the word-embedding plug-in (reference: src/plugin.py) over csrc/emb_fuse.hip: the fused
decoder / embedding distribution, the cosine embedding loss with in-kernel target gather, row L2 normalisation and an
out-of-place ReLU.  The GEMMs around them are ops.linear / decoder_ops.linear_infer."""
import torch
from torch.autograd import Function

from . import _lib
from . import ops as _ops
from .ops import _L, _p, _stream, _f32c, _require_gpu

NORM_EPS = 1e-12        # torch.nn.functional.normalize's default


def _rows_ld(x, V):
    """x [N,V] as (tensor, leading dimension): a row-strided view is passed as it is, anything else is compacted"""
    if x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1 and x.stride(0) >= V and x.shape[0] > 1:
        return x, x.stride(0)
    x = _f32c(x)
    return x, V


def _param(p, V, what):
    p = _f32c(p.detach()).reshape(-1)
    if p.numel() not in (1, V):
        raise RuntimeError("%s must hold 1 or %d values, got %d" % (what, V, p.numel()))
    return p


def _fuse_forward(dec_logit, emb_logit, temp, lam, lam_is_logit, eps):
    _require_gpu(dec_logit)
    _require_gpu(emb_logit)
    V = dec_logit.shape[-1]
    if emb_logit.shape[-1] != V or emb_logit.numel() // V != dec_logit.numel() // V:
        raise RuntimeError("fused distribution: decoder logits %s against embedding logits %s" % (
            tuple(dec_logit.shape), tuple(emb_logit.shape)))
    d, ld = _rows_ld(dec_logit.reshape(-1, V) if dec_logit.dim() != 2 else dec_logit, V)
    e = _f32c(emb_logit).reshape(-1, V)
    N = d.shape[0]
    tp, lm = _param(temp, V, "temp"), _param(lam, V, "fuse_lambda")
    y = torch.empty((N, V), dtype=torch.float32, device=d.device)
    stats = torch.empty((N, 4), dtype=torch.float32, device=d.device)
    _lib.check(_L().asrk_emb_fuse_fwd_f32(_p(d), ld, _p(e), _p(tp), tp.numel(), _p(lm), lm.numel(), int(lam_is_logit),
                                          float(eps), N, V, _p(y), _p(stats), _stream()), "emb_fuse")
    return y, (d, ld, e, tp, lm, stats)


class FuseFn(Function):
    """log((1 - s) softmax(dec_logit) + s softmax(relu(temp) * emb_logit) + eps), s = sigmoid(lam) or lam
    (src/plugin.py:103-123).  dec_logit / emb_logit [..., V]; temp, lam of 1 or V values."""

    @staticmethod
    def forward(ctx, dec_logit, emb_logit, temp, lam, lam_is_logit, eps):
        y, saved = _fuse_forward(dec_logit, emb_logit, temp, lam, lam_is_logit, eps)
        d, ld, e, tp, lm, stats = saved
        ctx.save_for_backward(d, e, tp, lm, stats)
        ctx.ld, ctx.is_logit, ctx.eps = ld, int(lam_is_logit), float(eps)
        ctx.shapes = (dec_logit.shape, emb_logit.shape, temp.shape, lam.shape)
        return y.reshape(dec_logit.shape)

    @staticmethod
    def backward(ctx, g):
        d, e, tp, lm, stats = ctx.saved_tensors
        N, V = e.shape
        gc = _f32c(g).reshape(N, V)
        dev = gc.device
        dd = torch.empty((N, V), dtype=torch.float32, device=dev)
        de = torch.empty((N, V), dtype=torch.float32, device=dev)
        dtemp = torch.empty_like(tp) if ctx.needs_input_grad[2] else None
        dlam = torch.empty_like(lm) if ctx.needs_input_grad[3] else None
        L = _L()
        nws = int(L.asrk_emb_fuse_bwd_ws_bytes(N, V, tp.numel(), lm.numel(), int(dtemp is not None),
                                               int(dlam is not None)))
        ws = torch.empty((max(nws, 4),), dtype=torch.uint8, device=dev)
        _lib.check(L.asrk_emb_fuse_bwd_f32(_p(gc), _p(d), ctx.ld, _p(e), _p(tp), tp.numel(), _p(lm), lm.numel(),
                                           ctx.is_logit, ctx.eps, _p(stats), N, V, _p(dd), _p(de), _p(dtemp), _p(dlam),
                                           _p(ws), ws.numel(), _stream()), "emb_fuse_bwd")
        s_d, s_e, s_t, s_l = ctx.shapes
        return (dd.reshape(s_d), de.reshape(s_e), dtemp.reshape(s_t) if dtemp is not None else None,
                dlam.reshape(s_l) if dlam is not None else None, None, None)


def fuse(dec_logit, emb_logit, temp, lam, lam_is_logit, eps):
    if not torch.is_grad_enabled():              # decode positions: the kernel call without an autograd node
        return _fuse_forward(dec_logit, emb_logit, temp, lam, lam_is_logit, eps)[0].reshape(dec_logit.shape)
    return FuseFn.apply(dec_logit, emb_logit, temp, lam, lam_is_logit, eps)


class CosEmbLossFn(Function):
    """mean_b(sum_t (1 - cos(x_bt, table[label_bt])) / #{t: label_bt != 0}) with pad rows (label 0) masked out
    (src/plugin.py:137-155).  x [B*L,E] (or [B,L,E]), table [V,E], label [B,L]."""

    @staticmethod
    def forward(ctx, x, table, label):
        _require_gpu(x)
        _require_gpu(table)
        tb = _f32c(table)
        E = tb.shape[1]
        if label.dim() != 2 or x.shape[-1] != E or x.numel() != label.numel() * E:
            raise RuntimeError("cosine embedding loss: x %s, table %s, label %s" % (
                tuple(x.shape), tuple(tb.shape), tuple(label.shape)))
        xc = _f32c(x).reshape(-1, E)
        B, L = label.shape
        lb = label.to(device=xc.device, dtype=torch.int64).contiguous()
        row_loss = torch.empty((B * L,), dtype=torch.float32, device=xc.device)
        count = torch.empty((B,), dtype=torch.float32, device=xc.device)
        loss = torch.empty((1,), dtype=torch.float32, device=xc.device)
        _lib.check(_L().asrk_cos_emb_loss_fwd_f32(_p(xc), _p(tb), tb.shape[0], _p(lb), B, L, E, _p(row_loss),
                                                  _p(count), _p(loss), _stream()), "cos_emb_loss")
        ctx.save_for_backward(xc, tb, lb, count)
        ctx.x_shape = x.shape
        return loss[0]

    @staticmethod
    def backward(ctx, gout):
        xc, tb, lb, count = ctx.saved_tensors
        B, L = lb.shape
        V, E = tb.shape
        go = gout.to(torch.float32).reshape(1).contiguous()
        dx = torch.empty_like(xc)
        dy = torch.empty_like(xc) if ctx.needs_input_grad[1] else None
        _lib.check(_L().asrk_cos_emb_loss_bwd_f32(_p(xc), _p(tb), V, _p(lb), B, L, E, _p(count), _p(go), _p(dx),
                                                  _p(dy), _stream()), "cos_emb_loss_bwd")
        dtable = None
        if dy is not None:       # trainable table: the gathered rows' gradients summed per label in row order
            dtable = torch.empty((V, E), dtype=torch.float32, device=dx.device)
            _lib.check(_L().asrk_cos_emb_table_grad_f32(_p(dy), _p(lb), lb.numel(), E, V, _p(dtable), _stream()),
                       "cos_emb_table_grad")
        return dx.reshape(ctx.x_shape), dtable, None


def cos_emb_loss(x, table, label):
    return CosEmbLossFn.apply(x, table, label)


class L2NormFn(Function):
    """torch.nn.functional.normalize(x, dim=-1) (src/plugin.py:107-108)."""

    @staticmethod
    def forward(ctx, x):
        _require_gpu(x)
        xc = _f32c(x)
        D = xc.shape[-1]
        rows = xc.numel() // D
        y = torch.empty_like(xc)
        norm = torch.empty((rows,), dtype=torch.float32, device=xc.device)
        _lib.check(_L().asrk_l2norm_fwd_f32(_p(xc), _p(y), _p(norm), rows, D, NORM_EPS, _stream()), "l2norm")
        ctx.save_for_backward(y, norm)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, norm = ctx.saved_tensors
        D = y.shape[-1]
        g = _f32c(dy)
        dx = torch.empty_like(y)
        _lib.check(_L().asrk_l2norm_bwd_f32(_p(y), _p(g), _p(norm), _p(dx), norm.numel(), D, NORM_EPS, _stream()),
                   "l2norm_bwd")
        return dx


def l2_normalize(x):
    return L2NormFn.apply(x)


class ReluFn(Function):
    """nn.ReLU between the two linears of emb_net (src/plugin.py:35-37), on asrk_relu_*."""

    @staticmethod
    def forward(ctx, x):
        _require_gpu(x)
        xc = _f32c(x)
        y = torch.empty_like(xc)
        _ops.copy_flat(y, xc)
        _lib.check(_L().asrk_relu_fwd_f32(_p(y), y.numel(), _stream()), "relu")
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        g = _f32c(dy)
        dx = torch.empty_like(y)
        _lib.check(_L().asrk_relu_bwd_f32(_p(y), _p(g), _p(dx), y.numel(), _stream()), "relu_bwd")
        return dx


def relu(x):
    return ReluFn.apply(x)


def relu_(x):
    """in place, no autograd (inference buffers); x contiguous float32"""
    _require_gpu(x)
    assert x.is_contiguous() and x.dtype == torch.float32
    _lib.check(_L().asrk_relu_fwd_f32(_p(x), x.numel(), _stream()), "relu")
    return x


def l2_normalize_infer(x):
    """normalize(x, dim=-1) without an autograd node"""
    _require_gpu(x)
    xc = _f32c(x)
    D = xc.shape[-1]
    rows = xc.numel() // D
    y = torch.empty_like(xc)
    norm = torch.empty((rows,), dtype=torch.float32, device=xc.device)
    _lib.check(_L().asrk_l2norm_fwd_f32(_p(xc), _p(y), _p(norm), rows, D, NORM_EPS, _stream()), "l2norm")
    return y
