"""GPU: the RNN-transducer kernels (csrc/rnnt.hip) against float64 on the same inputs (tests/rnnt_reference.py).

Tolerance rule (tests/test_mwer_gpu.py, tests/test_rescore_gpu.py): E is the error of the existing differentiable path on
the same case - ops.log_softmax, gathers, then the alpha recursion in f32 torch ops under autograd on the device (one
vectorised logaddexp per anti-diagonal) - and the new path must be within 2 * max(E, floor).  The floors count the
roundings along one lattice path and never look at the new kernels' results:

 * row pass: a log-probability z - lse of logits within +-S carries one rounding of lse (|lse| <= S + ln V) and one of the
   difference (|z - lse| <= 2S + ln V): floor_row = 2^-23 * (2S + ln V).
 * nll: a path has T + U steps; each adds one rounded log-probability to a partial sum and takes one logaddexp, three
   roundings of relative size 2^-24 on magnitudes bounded by A = the largest |alpha|, |beta| of the float64 reference:
   floor_nll = 3 (T + U) 2^-24 max(1, A).
 * gradient: every entry is gscale * (e^x - ...) with e^x <= 1 and x = (alpha + beta - ln P) + (z - lse), three lattice
   quantities with the error above and one row quantity: floor_grad = max|gscale| * (3 floor_nll + floor_row)."""
import ctypes
import functools
import importlib
import math

import pytest
import torch

import rnnt_reference as RR
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu
DEV = "cuda"
NEG = float("-inf")
WG = 2048                       # the wave-per-row / workgroup-per-row switch of the row and gradient passes


def _mod(name):
    return importlib.import_module(PKG_NAME + "." + name)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _strided(x, ld, offset, fill=0.0):
    """x [M,V] on the device with row stride ld, its base `offset` floats behind a 256-byte boundary -> (view, buffer)"""
    M, V = x.shape
    buf = torch.full((M * ld + offset + 4,), fill, dtype=torch.float32, device=DEV)
    view = buf[offset:offset + M * ld].view(M, ld)[:, :V]
    view.copy_(x)
    assert view.data_ptr() % 16 == (4 * offset) % 16
    return view, buf


def _inside(B, T, U1, enc_len, txt_len):
    m = torch.zeros((B, T, U1), dtype=torch.bool)
    for b in range(B):
        m[b, :int(enc_len[b]), :int(txt_len[b]) + 1] = True
    return m


# ---- the existing differentiable path (E) --------------------------------------------------------------------------------
def _alpha_diag_lnp(lpb, lpl, T, U):
    """ln P of one utterance from lpb [T, U+1], lpl [T, >= U] (device tensors under autograd): the alpha recursion, one
    vectorised logaddexp per anti-diagonal"""
    dev = lpb.device
    pad = torch.full((1,), NEG, device=dev, dtype=lpb.dtype)
    prev, plo = torch.zeros((1,), device=dev, dtype=lpb.dtype), 0
    for d in range(1, T + U):
        ulo, uhi = max(0, d - (T - 1)), min(U, d)
        us = torch.arange(ulo, uhi + 1, device=dev)
        ts = d - us
        pp = torch.cat([pad, prev, pad])                    # covers u in [plo - 1, phi + 1]
        top = pp[us - plo + 1] + lpb[(ts - 1).clamp(min=0), us]         # t = 0: the -inf pad
        left = pp[us - plo] + lpl[ts, (us - 1).clamp(min=0)]            # u = 0: the -inf pad
        prev, plo = torch.logaddexp(top, left), ulo
    return prev[0] + lpb[T - 1, U]


def _existing_path(ops, x, txt, enc_len, txt_len, w):
    """x [B,T,U1,V] f32 on the host -> (lp [B,T,U1,V] as the device path has it, nll [B], d (sum_b w_b nll_b) / dx),
    through ops.log_softmax and autograd on the device"""
    B, T, U1, V = x.shape
    xg = x.to(DEV).requires_grad_(True)
    lp = ops.log_softmax(xg.view(-1, V)).view(B, T, U1, V)
    nll = []
    for b in range(B):
        Tb, Ub = int(enc_len[b]), int(txt_len[b])
        y = txt[b, :Ub].to(DEV)
        lpb = lp[b, :Tb, :Ub + 1, 0]
        # (U_b = 0: one column that only ever meets the -inf pad)
        lpl = lp[b, :Tb, :Ub].gather(2, y.view(1, Ub, 1).expand(Tb, Ub, 1)).squeeze(2) if Ub else lpb.new_zeros((Tb, 1))
        nll.append(-_alpha_diag_lnp(lpb, lpl, Tb, Ub))
    nll = torch.stack(nll)
    (nll * w.to(DEV).float()).sum().backward()
    return lp.detach().cpu().double(), nll.detach().cpu().double(), xg.grad.cpu().double()


def _floors(T, U, S, V, A, wmax):
    f_row = 2.0 ** -23 * (2 * S + math.log(V))
    f_nll = 3 * (T + U) * 2.0 ** -24 * max(1.0, A)
    return f_row, f_nll, wmax * (3 * f_nll + f_row)


def _ref_extreme(x64, txt, enc_len, txt_len):
    """A: the largest |alpha|, |beta| of the float64 reference over the batch"""
    A = 0.0
    for b in range(x64.shape[0]):
        Tb, Ub = int(enc_len[b]), int(txt_len[b])
        lp = RR.log_probs(x64[b, :Tb, :Ub + 1])
        a, _ = RR.alpha_lattice(lp, txt[b, :Ub])
        bt, _ = RR.beta_lattice(lp, txt[b, :Ub])
        A = max(A, max(abs(float(v)) for row in a for v in row), max(abs(float(v)) for row in bt for v in row))
    return A


def _launch(L, ops, xd, ld, txt_d, el_d, tl_d, B, T, U1, V, want_beta=True):
    f = dict(dtype=torch.float32, device=DEV)
    lse, lpb, lpl = (torch.full((B, T, U1), float("nan"), **f) for _ in range(3))
    alpha, beta = torch.full((B, T, U1), 7.0, **f), torch.full((B, T, U1), 7.0, **f)
    nll = torch.full((B,), float("nan"), **f)
    st = ops._stream()
    assert L.asrk_rnnt_rows_f32(_p(xd), ld, _p(txt_d), txt_d.shape[1], _p(el_d), _p(tl_d), B, T, U1, V, 0, _p(lse),
                                _p(lpb), _p(lpl), st) == 0
    assert L.asrk_rnnt_lattice_f32(_p(lpb), _p(lpl), _p(el_d), _p(tl_d), B, T, U1, _p(alpha),
                                   _p(beta if want_beta else None), _p(nll), st) == 0
    return lse, lpb, lpl, alpha, beta, nll


# ---- row pass and gradient pass: every variant --------------------------------------------------------------------------
@pytest.mark.parametrize("V", [2, 3, 63, 64, 65, WG - 1, WG, WG + 1, 4099])
@pytest.mark.parametrize("pad,offset", [(0, 0), (3, 0), (0, 1), (3, 1)])
def test_rows_and_grad_variants_against_float64(ops, V, pad, offset):
    """a wave per row (V < 2048) and a workgroup per row, 16-byte accesses (aligned base, stride % 4 == 0) and scalar ones;
    logits scaled to +-80; the gradient out of place with a stride of its own and in place.  B = 2 ragged, T = 3, U = 2
    with a repeated label; the rows outside the lattices hold NaN, so reading one of them shows"""
    L = _mod("_lib").load()
    B, T, U1, S = 2, 3, 3, 80.0
    g = torch.Generator().manual_seed(V * 31 + pad * 7 + offset)
    x = (torch.rand((B, T, U1, V), generator=g) * 2 - 1) * S
    lab = int(torch.randint(1, V, (1,), generator=g))
    txt = torch.tensor([[lab, lab], [int(torch.randint(1, V, (1,), generator=g)), 0]])
    enc_len, txt_len = torch.tensor([3, 2]), torch.tensor([2, 1])
    w = torch.tensor([1.5, -0.75], dtype=torch.float64)
    inside = _inside(B, T, U1, enc_len, txt_len)
    M, ld = B * T * U1, V + pad
    x_nan = x.clone()
    x_nan[~inside] = float("nan")
    xd, xbuf = _strided(x_nan.view(M, V), ld, offset)
    txt_d, el_d, tl_d, w_d = txt.to(DEV), enc_len.to(DEV), txt_len.to(DEV), w.float().to(DEV)
    lse, lpb, lpl, alpha, beta, nll = _launch(L, ops, xd, ld, txt_d, el_d, tl_d, B, T, U1, V)
    # float64 reference, the existing path and the floors
    x64 = x.double()
    nll_r, grad_r = RR.batch_nll_grad(x64, txt, enc_len, txt_len, weight=w)
    lp_r = RR.log_probs(x64)
    lp_e, nll_e, grad_e = _existing_path(ops, x, txt, enc_len, txt_len, w)
    A = _ref_extreme(x64, txt, enc_len, txt_len)
    f_row, f_nll, f_grad = _floors(T, U1 - 1, S, V, A, float(w.abs().max()))
    E_row = float((lp_e - lp_r)[inside].abs().max())
    E_nll = float((nll_e - nll_r).abs().max())
    E_grad = float((grad_e - grad_r).abs().max())
    # row pass
    assert bool((lse.cpu()[~inside] == 0).all()) and bool((lpb.cpu()[~inside] == 0).all())
    assert bool((lpl.cpu()[~inside] == 0).all())
    lse_r = torch.logsumexp(x64, -1)
    err_lse = float((lse.cpu().double() - lse_r)[inside].abs().max())
    err_lpb = float((lpb.cpu().double() - lp_r[..., 0])[inside].abs().max())
    err_lpl = 0.0
    for b in range(B):
        for u in range(int(txt_len[b])):
            got = lpl.cpu().double()[b, :int(enc_len[b]), u]
            err_lpl = max(err_lpl, float((got - lp_r[b, :int(enc_len[b]), u, int(txt[b, u])]).abs().max()))
        assert bool((lpl[b, :, int(txt_len[b])] == 0).all())              # u = U_b: no label
    tol_row = 2 * max(E_row, f_row)
    err_nll = float((nll.cpu().double() - nll_r).abs().max())
    tol_nll = 2 * max(E_nll, f_nll)
    print("V", V, "ld", ld, "offset", offset, "| E_row", E_row, "err", err_lse, err_lpb, err_lpl, "tol", tol_row,
          "| E_nll", E_nll, "err", err_nll, "tol", tol_nll)
    assert err_lse <= tol_row and err_lpb <= tol_row and err_lpl <= tol_row
    assert err_nll <= tol_nll
    # gradient, out of place: NaN-filled dz with its own stride
    st = ops._stream()
    ldd = ld + 4                            # the same alignment class as x: the 16-byte variant stays one
    dzd, dbuf = _strided(torch.full((M, V), float("nan")), ldd, offset, fill=float("nan"))

    def grad(dst, ld_dst):
        return L.asrk_rnnt_grad_f32(_p(xd), ld, _p(txt_d), txt_d.shape[1], _p(el_d), _p(tl_d), B, T, U1, V, 0, _p(lse),
                                    _p(lpb), _p(lpl), _p(alpha), _p(beta), _p(nll), _p(w_d), _p(dst), ld_dst, st)
    assert grad(dzd, ldd) == 0
    got = dzd.cpu().double().view(B, T, U1, V)
    assert bool((got[~inside] == 0).all()), "cells outside the lattice must be written as exact zeros"
    err_grad = float((got - grad_r).abs().max())
    tol_grad = 2 * max(E_grad, f_grad)
    print("   E_grad", E_grad, "err", err_grad, "tol", tol_grad)
    assert err_grad <= tol_grad
    # nothing but the [M, V] elements was written: the padding columns and the slack keep their NaN
    mask = torch.ones_like(dbuf, dtype=torch.bool)
    mask[offset:offset + M * ldd].view(M, ldd)[:, :V] = False
    assert bool(torch.isnan(dbuf[mask]).all())
    if (pad, offset) == (0, 0):             # an odd dz stride beside an aligned x: scalar accesses, the same values
        odd, _ = _strided(torch.full((M, V), float("nan")), ld + 1, 0, fill=float("nan"))
        assert grad(odd, ld + 1) == 0
        assert torch.equal(odd, dzd)
    # a second run: bit-equal
    dz2, _ = _strided(torch.full((M, V), float("nan")), ldd, offset, fill=float("nan"))
    assert grad(dz2, ldd) == 0 and torch.equal(dz2, dzd)
    # in place: the same values, the padding columns untouched
    assert grad(xd, ld) == 0
    ops.check_errors()
    assert torch.equal(xd, dzd)
    if pad:
        assert bool((xbuf[offset:offset + M * ld].view(M, ld)[:, V:] == 0).all())


# ---- lattice --------------------------------------------------------------------------------------------------------------
LAT_V = 5


@functools.lru_cache(maxsize=None)
def _utt(T, U, b):
    """utterance b of the (T, U) lattice case: logits [T, U+1, V] and labels [U] (repeats included); shared, never modified"""
    g = torch.Generator().manual_seed(1000 * T + 10 * U + b)
    x = torch.randn((T, U + 1, LAT_V), generator=g) * 3
    y = torch.randint(1, LAT_V, (U,), generator=g)
    return x, y


@functools.lru_cache(maxsize=None)
def _utt_ref(T, U, b):
    """float64: (nll, gradient, A) of that utterance, computed once"""
    x, y = _utt(T, U, b)
    z = x.double().requires_grad_(True)
    lp = RR.log_probs(z)
    a, lnp = RR.alpha_lattice(lp, y)
    (-lnp).backward()
    with torch.no_grad():
        bt, lnp_b = RR.beta_lattice(lp, y)
    lnp_b = float(lnp_b.detach())
    assert abs(float(lnp.detach()) - lnp_b) <= 1e-9 * max(1.0, abs(lnp_b))
    A = max(max(abs(float(v)) for row in a for v in row), max(abs(float(v)) for row in bt for v in row))
    return float(-lnp.detach()), z.grad, A


@functools.lru_cache(maxsize=None)
def _utt_existing(T, U, b):
    """(E_nll, E_grad) of the existing path on that utterance alone (needs the device)"""
    ops = _mod("ops")
    x, y = _utt(T, U, b)
    nll_r, grad_r, _ = _utt_ref(T, U, b)
    _, nll_e, grad_e = _existing_path(ops, x.unsqueeze(0), y.view(1, -1), [T], [U], torch.ones(1, dtype=torch.float64))
    return abs(float(nll_e[0]) - nll_r), float((grad_e[0] - grad_r).abs().max())


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T,U", [(1, 0), (1, 1), (1, 5), (5, 0), (2, 1), (7, 3), (3, 7), (64, 63), (65, 64), (9, 300)])
def test_lattice_against_float64(ops, T, U, B):
    """rows -> lattice -> gradient through the ABI on full-length utterances; (9, 300) has U + 1 = 301 > 128 lanes per
    direction, so the lane loop runs (and (64, 63) fills the 64th lane, (65, 64) the first beyond a wave).  B = 3 holds
    utterance 0 of the B = 1 launch: its results must not depend on the others, bit for bit."""
    L = _mod("_lib").load()
    U1, V = U + 1, LAT_V
    x = torch.stack([_utt(T, U, b)[0] for b in range(B)])
    txt = torch.stack([_utt(T, U, b)[1] for b in range(B)]) if U else torch.zeros((B, 0), dtype=torch.int64)
    xd = x.to(DEV).view(-1, V).contiguous()
    txt_d = txt.to(DEV).contiguous() if U else torch.zeros((B, 1), dtype=torch.int64, device=DEV)
    el_d = torch.full((B,), T, dtype=torch.int64, device=DEV)
    tl_d = torch.full((B,), U, dtype=torch.int64, device=DEV)
    w_d = torch.ones((B,), dtype=torch.float32, device=DEV)
    st = ops._stream()

    def run():
        lse, lpb, lpl, alpha, beta, nll = _launch(L, ops, xd, V, txt_d, el_d, tl_d, B, T, U1, V)
        dz = torch.full((B * T * U1, V), float("nan"), dtype=torch.float32, device=DEV)
        assert L.asrk_rnnt_grad_f32(_p(xd), V, _p(txt_d), txt_d.shape[1], _p(el_d), _p(tl_d), B, T, U1, V, 0, _p(lse),
                                    _p(lpb), _p(lpl), _p(alpha), _p(beta), _p(nll), _p(w_d), _p(dz), V, st) == 0
        return alpha, beta, nll, dz.view(B, T, U1, V)
    alpha, beta, nll, dz = run()
    alpha2, beta2, nll2, dz2 = run()
    ops.check_errors()
    assert torch.equal(alpha, alpha2) and torch.equal(beta, beta2) and torch.equal(nll, nll2) and torch.equal(dz, dz2)
    # forward only: alpha alone, the same nll, beta untouched
    _, _, _, alpha_f, beta_f, nll_f = _launch(L, ops, xd, V, txt_d, el_d, tl_d, B, T, U1, V, want_beta=False)
    assert torch.equal(nll_f, nll) and torch.equal(alpha_f, alpha) and bool((beta_f == 7.0).all())
    # alpha-side and beta-side ln P of the kernel agree with each other as far as f32 lets them
    for b in range(B):
        nll_r, grad_r, A = _utt_ref(T, U, b)
        E_nll, E_grad = _utt_existing(T, U, b)
        _, f_nll, f_grad = _floors(T, U, 3.0 * 6, V, A, 1.0)       # |randn * 3| stays below 18
        err_nll = abs(float(nll[b]) - nll_r)
        err_beta = abs(float(beta[b, 0, 0]) + nll_r)
        err_grad = float((dz[b].cpu().double() - grad_r).abs().max())
        print("T", T, "U", U, "B", B, "b", b, "| E_nll", E_nll, "err", err_nll, err_beta, "tol", 2 * max(E_nll, f_nll),
              "| E_grad", E_grad, "err", err_grad, "tol", 2 * max(E_grad, f_grad))
        assert err_nll <= 2 * max(E_nll, f_nll) and err_beta <= 2 * max(E_nll, f_nll)
        assert err_grad <= 2 * max(E_grad, f_grad)
    if B == 3:
        one = _LAT_ONE.get((T, U))
        if one is not None:
            assert torch.equal(one[0], nll[:1].cpu()) and torch.equal(one[1], dz[:1].cpu())
            assert torch.equal(one[2], alpha[:1].cpu()) and torch.equal(one[3], beta[:1].cpu())
        else:                                            # run alone: the B = 1 launch of the same utterance
            lse1, lpb1, lpl1, a1, b1, n1 = _launch(L, ops, xd[:T * U1], V, txt_d[:1], el_d[:1], tl_d[:1], 1, T, U1, V)
            assert torch.equal(n1, nll[:1]) and torch.equal(a1, alpha[:1]) and torch.equal(b1, beta[:1])
    else:
        _LAT_ONE[(T, U)] = (nll.cpu(), dz.cpu(), alpha.cpu(), beta.cpu())


_LAT_ONE = {}


def test_loss_module_ragged_batch(ops):
    """ops.RNNTLoss end to end on one ragged batch: lengths below the padded sizes, one utterance with txt_len = 0,
    repeated labels, txt wider than U never read; every reduction; consume_logits writes the gradient over the logits"""
    B, T, U, V = 3, 7, 5, 6
    g = torch.Generator().manual_seed(11)
    x = torch.randn((B, T, U + 1, V), generator=g) * 3
    txt = torch.tensor([[2, 2, 3, 3, 1], [0, 0, 0, 0, 0], [4, 4, 4, 0, 0]])
    enc_len, txt_len = torch.tensor([7, 4, 5]), torch.tensor([5, 0, 3])
    inside = _inside(B, T, U + 1, enc_len, txt_len)
    x64 = x.double()
    A = _ref_extreme(x64, txt, enc_len, txt_len)
    for reduction, w in (("mean", torch.full((B,), 1.0 / B, dtype=torch.float64)),
                         ("sum", torch.ones(B, dtype=torch.float64)),
                         ("none", torch.tensor([0.5, -2.0, 1.25], dtype=torch.float64))):
        nll_r, grad_r = RR.batch_nll_grad(x64, txt, enc_len, txt_len, weight=w)
        _, nll_e, grad_e = _existing_path(ops, x, txt, enc_len, txt_len, w)
        _, f_nll, f_grad = _floors(T, U, 18.0, V, A, float(w.abs().max()))
        tol_nll = 2 * max(float((nll_e - nll_r).abs().max()), f_nll)
        tol_grad = 2 * max(float((grad_e - grad_r).abs().max()), f_grad)
        for consume in (False, True):
            xg = x.to(DEV).requires_grad_(True)
            logits = xg * 1.0                                   # a non-leaf the loss may overwrite
            keep = logits.detach().clone()
            loss = ops.RNNTLoss(blank=0, reduction=reduction)(logits, txt.to(DEV), enc_len.to(DEV), txt_len.to(DEV),
                                                              consume_logits=consume)
            if reduction == "none":
                assert loss.shape == (B,)
                assert float((loss.detach().cpu().double() - nll_r).abs().max()) <= tol_nll
                (loss * w.float().to(DEV)).sum().backward()
            else:
                want = nll_r.mean() if reduction == "mean" else nll_r.sum()
                assert abs(float(loss) - float(want)) <= tol_nll * (1 if reduction == "mean" else B)
                loss.backward()
            got = xg.grad.cpu().double()
            assert bool((got[~inside] == 0).all())
            assert float((got - grad_r).abs().max()) <= tol_grad
            if consume:
                assert torch.equal(logits.detach(), xg.grad)     # the logits' storage now holds the gradient
            else:
                assert torch.equal(logits.detach(), keep)
    # no gradient wanted: the forward alone (alpha only) gives the same loss
    with torch.no_grad():
        l0 = ops.RNNTLoss(reduction="none")(x.to(DEV), txt.to(DEV), enc_len.to(DEV), txt_len.to(DEV))
    assert torch.equal(l0, ops.RNNTLoss(reduction="none")(x.to(DEV).requires_grad_(True), txt.to(DEV), enc_len.to(DEV),
                                                          txt_len.to(DEV)).detach())
    ops.check_errors()


# ---- joint network ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("J", [1, 4, 63, 64, 130])
def test_joint_pair_against_float64(ops, J):
    """forward and backward of the joint, dense and in the gathered decode form, 16-byte (J % 4 == 0) and scalar variants,
    strides of their own.  E: the same function from existing ops (a broadcast add, ops.tanh) under autograd.  Floors:
    forward, one rounded add and one tanh with |tanh| <= 1 and |tanh'| <= 1: 2^-23 * max(1, |E + P|); backward, a sum
    of n = U + 1 (T) products dH (1 - H^2), each with three roundings, accumulated in f32: 4 n 2^-24 max|dH|."""
    L = _mod("_lib").load()
    B, T, U1 = 3, 5, 4
    g = torch.Generator().manual_seed(J)
    E, P = torch.randn((B, T, J), generator=g) * 1.5, torch.randn((B, U1, J), generator=g) * 1.5
    dH = torch.randn((B, T, U1, J), generator=g) * 2
    inside = _inside(B, T, U1, [5, 3, 4], [3, 0, 2])
    dH[~inside] = 0.0                                           # what the loss's gradient leaves in padded cells
    E64, P64 = E.double().requires_grad_(True), P.double().requires_grad_(True)
    H64 = torch.tanh(E64.unsqueeze(2) + P64.unsqueeze(1))
    H64.backward(dH.double())
    Ee, Pe = E.to(DEV).requires_grad_(True), P.to(DEV).requires_grad_(True)
    He = ops.tanh(Ee.unsqueeze(2) + Pe.unsqueeze(1))
    He.backward(dH.to(DEV))
    Ed, Pd = E.to(DEV).requires_grad_(True), P.to(DEV).requires_grad_(True)
    H = ops.RNNTJointFn.apply(Ed, Pd)
    H.backward(dH.to(DEV))
    ops.check_errors()
    s = float((E.double().unsqueeze(2) + P.double().unsqueeze(1)).abs().max())
    tol_f = 2 * max(float((He.detach().cpu().double() - H64.detach()).abs().max()), 2.0 ** -23 * max(1.0, s))
    dmax = float(dH.abs().max())
    E_e = float((Ee.grad.cpu().double() - E64.grad).abs().max())
    E_p = float((Pe.grad.cpu().double() - P64.grad).abs().max())
    tol_e, tol_p = 2 * max(E_e, 4 * U1 * 2.0 ** -24 * dmax), 2 * max(E_p, 4 * T * 2.0 ** -24 * dmax)
    err_f = float((H.detach().cpu().double() - H64.detach()).abs().max())
    err_e = float((Ed.grad.cpu().double() - E64.grad).abs().max())
    err_p = float((Pd.grad.cpu().double() - P64.grad).abs().max())
    print("J", J, "fwd", err_f, tol_f, "dE", err_e, tol_e, "dP", err_p, tol_p)
    assert err_f <= tol_f and err_e <= tol_e and err_p <= tol_p
    # strides of their own through the ABI: the same bits, the columns beyond J untouched
    st = ops._stream()
    ld = J + 3
    Ev, _ = _strided(E.view(-1, J), ld, 1)
    Pv, _ = _strided(P.view(-1, J), ld, 1)
    Hv, Hbuf = _strided(torch.full((B * T * U1, J), float("nan")), ld, 1, fill=float("nan"))
    assert L.asrk_rnnt_joint_f32(_p(Ev), ld, _p(Pv), ld, None, B, T, U1, J, _p(Hv), ld, st) == 0
    assert torch.equal(Hv, H.detach().view(-1, J))
    mask = torch.ones_like(Hbuf, dtype=torch.bool)
    mask[1:1 + B * T * U1 * ld].view(-1, ld)[:, :J] = False
    assert bool(torch.isnan(Hbuf[mask]).all())
    dHv, _ = _strided(dH.view(-1, J), ld, 1)
    dEv, dEbuf = _strided(torch.full((B * T, J), float("nan")), ld, 1, fill=float("nan"))
    dPv, dPbuf = _strided(torch.full((B * U1, J), float("nan")), ld, 1, fill=float("nan"))
    assert L.asrk_rnnt_joint_bwd_f32(_p(Hv), ld, _p(dHv), ld, B, T, U1, J, _p(dEv), ld, _p(dPv), ld, st) == 0
    assert torch.equal(dEv, Ed.grad.view(-1, J)) and torch.equal(dPv, Pd.grad.view(-1, J))
    for buf, rows in ((dEbuf, B * T), (dPbuf, B * U1)):
        mask = torch.ones_like(buf, dtype=torch.bool)
        mask[1:1 + rows * ld].view(-1, ld)[:, :J] = False
        assert bool(torch.isnan(buf[mask]).all())
    # two runs bit-equal
    H2 = ops.RNNTJointFn.apply(Ed.detach().requires_grad_(True), Pd.detach())
    assert torch.equal(H2.detach(), H.detach())
    # the gathered decode form: one (t_idx[b], row b) pair per utterance; an index past the last frame is clamped
    t_idx = torch.tensor([4, 0, 9], dtype=torch.int32, device=DEV)
    Hs = ops.rnnt_joint_step(Ed.detach(), Pd.detach()[:, 2].contiguous(), t_idx)
    want = torch.stack([H.detach()[0, 4, 2], H.detach()[1, 0, 2], H.detach()[2, T - 1, 2]])
    assert torch.equal(Hs, want)
    ops.check_errors()


# ---- greedy step ------------------------------------------------------------------------------------------------------------
def test_greedy_step_rules(ops):
    """ties (inside one lane: 7 and 71 = 7 + 64; across lanes: 40), blank, the max_symbols cap, the max_len cap, a
    finished row, the last frame; V = 80 spans two passes of the wave"""
    B, V, T, max_symbols, max_len = 8, 80, 6, 2, 3
    x = torch.full((B, V), -1.0)
    x[0, [7, 40, 71]] = 5.0           # ties: the lowest index wins
    x[1, [40, 71]] = 5.0              # ... across lanes too
    x[2, 0] = 9.0                     # blank
    x[3, 33] = 9.0                    # non-blank, but this frame already emitted max_symbols
    x[4, 33] = 9.0                    # non-blank, but the row already holds max_len tokens
    x[5, 33] = 9.0                    # finished: nothing moves
    x[6, 0] = 9.0                     # blank at the last frame: done
    x[7, 79] = 9.0                    # the last column
    x[5] = float("nan")               # a finished row is not read
    st = ops.rnnt_greedy_state(B, max_len, torch.device(DEV))
    enc_len = torch.tensor([6, 6, 6, 6, 6, 6, 4, 9], dtype=torch.int64, device=DEV)      # 9: clamped to T
    st.t_ptr.copy_(torch.tensor([0, 1, 2, 3, 4, 5, 3, 5], dtype=torch.int32))
    st.n_sym.copy_(torch.tensor([0, 1, 1, 2, 0, 0, 1, 0], dtype=torch.int32))
    st.n_tok.copy_(torch.tensor([0, 1, 2, 2, 3, 1, 0, 2], dtype=torch.int32))
    st.tokens.fill_(-1)
    st.last_tok.copy_(torch.tensor([0, 9, 9, 9, 9, 9, 0, 9]))
    st.done.copy_(torch.tensor([0, 0, 0, 0, 0, 1, 0, 0], dtype=torch.int32))
    st.emit.fill_(5)
    ops.rnnt_greedy_step(x.to(DEV), enc_len, T, st, max_symbols, max_len)
    ops.check_errors()
    assert st.emit.tolist() == [1, 1, 0, 0, 0, 0, 0, 1]
    assert st.t_ptr.tolist() == [0, 1, 3, 4, 5, 5, 4, 5]
    assert st.n_sym.tolist() == [1, 2, 0, 0, 0, 0, 0, 1]
    assert st.n_tok.tolist() == [1, 2, 2, 2, 3, 1, 0, 3]
    assert st.last_tok.tolist() == [7, 40, 9, 9, 9, 9, 0, 79]
    assert st.done.tolist() == [0, 0, 0, 0, 0, 1, 1, 0]
    tok = st.tokens.tolist()
    assert tok[0] == [7, -1, -1] and tok[1] == [-1, 40, -1] and tok[7] == [-1, -1, 79]
    assert all(tok[b] == [-1, -1, -1] for b in (2, 3, 4, 5, 6))
    # the next iteration: row 1 now sits at the cap, row 7 is full, row 6 is finished
    ops.rnnt_greedy_step(x.to(DEV), enc_len, T, st, max_symbols, max_len)
    assert st.emit.tolist() == [1, 0, 0, 1, 0, 0, 0, 0]
    assert st.t_ptr.tolist() == [0, 2, 4, 4, 6, 5, 4, 6] and st.done.tolist() == [0, 0, 0, 0, 1, 1, 1, 1]
    assert st.tokens.tolist()[3] == [-1, -1, 33] and st.n_tok.tolist() == [2, 2, 2, 3, 3, 1, 0, 3]
    ops.check_errors()
