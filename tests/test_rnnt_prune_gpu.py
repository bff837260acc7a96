"""GPU: the kernels of pruned transducer training (csrc/rnnt_prune.hip) against float64 on the same inputs
(tests/rnnt_prune_reference.py).

Tolerance rule (docstring of tests/test_rnnt_gpu.py): the new path must be within 2 * max(E, floor) of float64, where E is
the error against float64 of an f32 composition of EXISTING ops on the same inputs, never of the kernels under test:

 * simple joiner: ops.RNNTLoss on the dense sum am[:, :, None] + lm[:, None] (nll and, through autograd's broadcast sums,
   dam and dlm); for the row quantities ops.log_softmax on that sum, and for the occupations the f32 alpha recursion on
   those log-probabilities under autograd (d ln P / d lpb = eb, d ln P / d lpl = el);
 * band loss: ops.log_softmax on the band logits, gathers, and the f32 autograd alpha recursion that only ever steps
   inside the band (tests/rnnt_prune_reference.py: band_lnp);
 * band joint: torch.tanh on a gathered sum, f32, under autograd.

Floors are those of tests/test_rnnt_gpu.py (floor_row, floor_nll, floor_grad from the logit bound, V, T + U and the largest
|alpha|, |beta| of the float64 reference); the simple joiner's logits are sums of two values within +-40, so its bound is
80.  dam[t, v] adds at most U + 1 dense gradient entries and dlm[u, v] at most T, each with floor_grad: their floors are
(U + 1) floor_grad and T floor_grad.  The band joint's floors count roundings: the forward is one rounded sum and a tanh
(slope <= 1), 2^-23 max(1, max|E| + max|P|); a gradient adds n terms dH (1 - H^2) of four roundings each,
4 n 2^-24 max|dH| with n = S for dE and n = T S for dP.

The sets of the shapes: V in {2, 3, 63, 64, 65, 2049} and (T, U) in {(1,0), (1,3), (4,1), (7,3), (3,7), (65,64)}, every
pair except (65,64) with V > 65 (the float64 mirror of a [65, 65, 2049] sum is what takes long, the kernel's paths are
all taken at V = 65); B = 3 with mixed lengths, and utterance 1 again alone (B = 1)."""
import importlib
import math

import numpy as np
import pytest
import torch

import rnnt_reference as RR
import rnnt_prune_reference as PR
from conftest import PKG_NAME
from test_rnnt_gpu import _floors, _p, _strided

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
TUS = [(1, 0), (1, 3), (4, 1), (7, 3), (3, 7), (65, 64)]


def _mod(name):
    return importlib.import_module(PKG_NAME + "." + name)


def _lens(T, U):
    """B = 3 mixed lengths: the full shape, about half of it, and a transcript one shorter over all frames"""
    return [T, max(1, (T + 1) // 2), T], [U, U // 2, max(0, U - 1)]


def _nan_full(shape):
    return torch.full(shape, NAN, dtype=torch.float32, device=DEV)


# ---- simple joiner ---------------------------------------------------------------------------------------------------------
def _simple_launch(L, ops, amv, lda, lmv, ldl, txt_d, el_d, tl_d, w_d, B, T, U1, V, ldda, lddl, offset):
    """rows -> lattice -> occupation -> gradient over NaN-filled outputs -> dict of device tensors"""
    st = ops._stream()
    o = {k: _nan_full((B, T, U1)) for k in ("lse", "lpb", "lpl", "c", "eb", "el")}
    o["alpha"], o["beta"], o["nll"] = _nan_full((B, T, U1)), _nan_full((B, T, U1)), _nan_full((B,))
    assert L.asrk_rnnt_simple_rows_f32(_p(amv), lda, _p(lmv), ldl, _p(txt_d), txt_d.shape[1], _p(el_d), _p(tl_d), B, T, U1,
                                       V, 0, _p(o["lse"]), _p(o["lpb"]), _p(o["lpl"]), st) == 0
    assert L.asrk_rnnt_lattice_f32(_p(o["lpb"]), _p(o["lpl"]), _p(el_d), _p(tl_d), B, T, U1, _p(o["alpha"]), _p(o["beta"]),
                                   _p(o["nll"]), st) == 0
    assert L.asrk_rnnt_simple_occ_f32(_p(o["lpb"]), _p(o["lpl"]), _p(o["alpha"]), _p(o["beta"]), _p(o["nll"]), _p(el_d),
                                      _p(tl_d), B, T, U1, _p(o["c"]), _p(o["eb"]), _p(o["el"]), st) == 0
    o["dam"], o["dam_buf"] = _strided(torch.full((B * T, V), NAN), ldda, offset, fill=NAN)
    o["dlm"], o["dlm_buf"] = _strided(torch.full((B * U1, V), NAN), lddl, offset, fill=NAN)
    assert L.asrk_rnnt_simple_grad_f32(_p(amv), lda, _p(lmv), ldl, _p(txt_d), txt_d.shape[1], _p(el_d), _p(tl_d), B, T, U1,
                                       V, 0, _p(o["lse"]), _p(o["c"]), _p(o["eb"]), _p(o["el"]), _p(w_d), _p(o["dam"]),
                                       ldda, _p(o["dlm"]), lddl, st) == 0
    ops.check_errors()
    return o


def _simple_existing(ops, am, lm, txt, enc_len, txt_len, w):
    """the f32 compositions of existing ops -> (lp [B,T,U1,V], nll, eb, el, dam, dlm), float64 on the host"""
    B, T, V = am.shape
    U1 = lm.shape[1]
    a, l = am.to(DEV).requires_grad_(True), lm.to(DEV).requires_grad_(True)
    txt_d = txt.to(DEV)
    x = a[:, :, None, :] + l[:, None, :, :]
    nll = ops.RNNTLoss(blank=0, reduction="none")(x, txt_d, torch.tensor(enc_len), torch.tensor(txt_len))
    (nll * w.to(DEV).float()).sum().backward()
    dam, dlm = a.grad.cpu().double(), l.grad.cpu().double()
    with torch.no_grad():
        xd = am.to(DEV)[:, :, None, :] + lm.to(DEV)[:, None, :, :]
    lp = ops.log_softmax(xd.reshape(-1, V)).view(B, T, U1, V)
    eb, el = torch.zeros((B, T, U1), dtype=torch.float64), torch.zeros((B, T, U1), dtype=torch.float64)
    for b in range(B):
        Tb, Ub = enc_len[b], txt_len[b]
        lpq = lp[b].detach().clone().requires_grad_(True)
        lnp, lpb, lpl = PR.lattice_terms(lpq[:Tb, :Ub + 1], txt_d[b], Tb, Ub)
        lnp.backward()
        eb[b, :Tb, :Ub + 1] = lpb.grad.cpu().double()
        if Ub:
            el[b, :Tb, :Ub] = lpl.grad.cpu().double()
    return lp.detach().cpu().double(), nll.detach().cpu().double(), eb, el, dam, dlm


def _check_simple(ops, tag, got, am, lm, txt, enc_len, txt_len, w, S):
    """the rule for whatever of lse / lpb / lpl / c / eb / el / occ / nll / dam / dlm `got` holds (float64 host tensors)"""
    B, T, V = am.shape
    U = lm.shape[1] - 1
    inside = torch.zeros((B, T, U + 1), dtype=torch.bool)
    for b in range(B):
        inside[b, :enc_len[b], :txt_len[b] + 1] = True
    ref = PR.simple_pass(am.double(), lm.double(), txt, enc_len, txt_len, weight=w)
    lp_e, nll_e, eb_e, el_e, dam_e, dlm_e = _simple_existing(ops, am, lm, txt, enc_len, txt_len, w)
    A = max(PR.lattice_extreme(ref["lpb"][b], ref["lpl"][b], enc_len[b], txt_len[b]) for b in range(B))
    f_row, f_nll, f_grad = _floors(T, U, S, V, A, float(w.abs().max()))
    lp_r = RR.log_probs(am.double()[:, :, None, :] + lm.double()[:, None, :, :])
    E = {"row": float((lp_e - lp_r)[inside].abs().max()), "nll": float((nll_e - ref["nll"]).abs().max()),
         "occ": max(float((eb_e - ref["eb"]).abs().max()), float((el_e - ref["el"]).abs().max())),
         "dam": float((dam_e - ref["dam"]).abs().max()), "dlm": float((dlm_e - ref["dlm"]).abs().max())}
    floor = {"row": f_row, "nll": f_nll, "occ": 3 * f_nll + f_row, "dam": (U + 1) * f_grad, "dlm": T * f_grad}
    group = {"lse": "row", "lpb": "row", "lpl": "row", "c": "occ", "eb": "occ", "el": "occ", "occ": "occ", "nll": "nll",
             "dam": "dam", "dlm": "dlm"}
    err = {}
    for k, v in got.items():
        err[group[k]] = max(err.get(group[k], 0.0), float((v - ref[k]).abs().max()))
    print("SIMPLE", tag, " ".join("| %s E %.3g err %.3g tol %.3g" % (k, E[k], err[k], 2 * max(E[k], floor[k]))
                                  for k in sorted(err)))
    for k in err:
        assert err[k] <= 2 * max(E[k], floor[k]), k


SIMPLE_CASES = [(V, T, U) for V in (2, 3, 63, 64, 65, 2049) for T, U in TUS if not ((T, U) == (65, 64) and V > 65)]


@pytest.mark.parametrize("V,T,U", SIMPLE_CASES)
def test_simple_rows_occupation_and_gradient(ops, V, T, U):
    L = _mod("_lib").load()
    B, U1, S = 3, U + 1, 80.0
    enc_len, txt_len = _lens(T, U)
    g = torch.Generator().manual_seed(1000 * V + 10 * T + U)
    am = (torch.rand((B, T, V), generator=g) * 2 - 1) * 40
    lm = (torch.rand((B, U1, V), generator=g) * 2 - 1) * 40
    txt = torch.randint(1, V, (B, max(U, 1)), generator=g)
    if U >= 2:
        txt[:, 1] = txt[:, 0]                            # a repeated label
    w = torch.tensor([1.5, -0.75, 0.5], dtype=torch.float64)
    inside = torch.zeros((B, T, U1), dtype=torch.bool)
    for b in range(B):
        inside[b, :enc_len[b], :txt_len[b] + 1] = True
    pad, offset = [(0, 0), (3, 1), (1, 0), (4, 1)][(V + T + U) % 4]      # aligned / misaligned bases, odd / even strides
    am_nan, lm_nan = am.clone(), lm.clone()
    for b in range(B):                                   # rows outside the lattices hold NaN: reading one shows
        am_nan[b, enc_len[b]:] = NAN
        lm_nan[b, txt_len[b] + 1:] = NAN
    lda = ldl = V + pad
    amv, _ = _strided(am_nan.view(B * T, V), lda, offset)
    lmv, _ = _strided(lm_nan.view(B * U1, V), ldl, offset)
    txt_d = txt.to(DEV)
    el_d, tl_d = torch.tensor(enc_len, device=DEV), torch.tensor(txt_len, device=DEV)
    w_d = w.float().to(DEV)
    ldda, lddl = lda + 4, ldl + 1
    o = _simple_launch(L, ops, amv, lda, lmv, ldl, txt_d, el_d, tl_d, w_d, B, T, U1, V, ldda, lddl, offset)

    dam = o["dam"].cpu().double().view(B, T, V)
    dlm = o["dlm"].cpu().double().view(B, U1, V)
    got = {k: o[k].cpu().double() for k in ("lse", "lpb", "lpl", "c", "eb", "el", "nll")}
    got.update(dam=dam, dlm=dlm)
    for k in ("lse", "lpb", "lpl", "c", "eb", "el"):
        assert bool((got[k][~inside] == 0).all()), k + ": cells outside the lattice must be exact zeros"
    for b in range(B):
        assert bool((got["lpl"][b, :, txt_len[b]] == 0).all()) and bool((got["el"][b, :, txt_len[b]] == 0).all())
    _check_simple(ops, "V %d T %d U %d ld %d offset %d" % (V, T, U, lda, offset), got, am, lm, txt, enc_len, txt_len, w, S)
    for b in range(B):                                   # padded rows: exact zeros written over the NaN fill
        assert bool((dam[b, enc_len[b]:] == 0).all()) and bool((dlm[b, txt_len[b] + 1:] == 0).all())
    for name, M, ld in (("dam", B * T, ldda), ("dlm", B * U1, lddl)):   # nothing but the [M, V] elements was written
        buf = o[name + "_buf"]
        mask = torch.ones_like(buf, dtype=torch.bool)
        mask[offset:offset + M * ld].view(M, ld)[:, :V] = False
        assert bool(torch.isnan(buf[mask]).all()), name
    # a second run: bit-equal
    o2 = _simple_launch(L, ops, amv, lda, lmv, ldl, txt_d, el_d, tl_d, w_d, B, T, U1, V, ldda, lddl, offset)
    for k in ("lse", "lpb", "lpl", "c", "eb", "el", "nll", "dam", "dlm"):
        assert torch.equal(o[k], o2[k]), k
    # utterance 1 alone (B = 1, contiguous, aligned): the same bits as inside the batch
    b = 1
    a1, l1 = am_nan[b:b + 1].to(DEV).contiguous(), lm_nan[b:b + 1].to(DEV).contiguous()
    o1 = _simple_launch(L, ops, a1.view(T, V), V, l1.view(U1, V), V, txt_d[b:b + 1].contiguous(), el_d[b:b + 1].clone(),
                        tl_d[b:b + 1].clone(), w_d[b:b + 1].clone(), 1, T, U1, V, V, V, 0)
    for k in ("lse", "lpb", "lpl", "c", "eb", "el"):
        assert torch.equal(o1[k][0], o[k][b]), k
    assert torch.equal(o1["nll"][0], o["nll"][b])
    assert torch.equal(o1["dam"].view(T, V), o["dam"].view(B, T, V)[b])
    assert torch.equal(o1["dlm"].view(U1, V), o["dlm"].view(B, U1, V)[b])


def test_simple_loss_function_and_autograd(ops):
    """ops.RNNTSimpleLossFn: nll, the detached occupation and the gradients that reach am and lm through autograd"""
    am, lm, txt, enc_len, txt_len = PR.lattice_range_case(1)
    a, l = am.to(DEV).requires_grad_(True), lm.to(DEV).requires_grad_(True)
    nll, occ = ops.RNNTSimpleLossFn.apply(a, l, txt.to(DEV), torch.tensor(enc_len), torch.tensor(txt_len), 0)
    assert nll.shape == (3,) and occ.shape == (3, 12, 21) and not occ.requires_grad and nll.requires_grad
    w = torch.tensor([1.0, 0.5, -2.0], dtype=torch.float64)
    (nll * w.float().to(DEV)).sum().backward()
    ops.check_errors()
    got = {"nll": nll.detach().cpu().double(), "occ": occ.cpu().double(), "dam": a.grad.cpu().double(),
           "dlm": l.grad.cpu().double()}
    bound = float(am.abs().max() + lm.abs().max())
    _check_simple(ops, "autograd", got, am, lm, txt, enc_len, txt_len, w, bound)


# ---- ranges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PR.range_cases(), ids=lambda c: c[0])
def test_ranges_on_the_device_equal_the_mirror(ops, case):
    _, occ, enc_len, txt_len, S = case
    want, _ = PR.ranges(occ.astype(np.float64), enc_len, txt_len, S)
    occ_d = torch.from_numpy(occ).to(DEV)
    got = ops.rnnt_prune_ranges(occ_d, torch.tensor(enc_len), torch.tensor(txt_len), S)
    ops.check_errors()
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want), (got.cpu().numpy(), want)
    # occupations beyond the lengths are never read: NaN there changes nothing
    occ_nan = occ.copy()
    for b in range(occ.shape[0]):
        occ_nan[b, enc_len[b]:] = np.nan
        occ_nan[b, :, txt_len[b] + 1:] = np.nan
    got2 = ops.rnnt_prune_ranges(torch.from_numpy(occ_nan).to(DEV), torch.tensor(enc_len), torch.tensor(txt_len), S)
    assert torch.equal(got, got2)


@pytest.mark.parametrize("seed", PR.LATTICE_RANGE_SEEDS)
def test_ranges_from_a_real_simple_lattice(ops, seed):
    """the occupations of the device's own simple lattice: (1) the rule in f32 numpy on those very numbers gives the
    device's ranges exactly (the same sums in the same order); (2) against the float64 mirror of the whole chain, on the
    frames whose best and second-best float64 window sums differ by at least 1e-3 of the best - fewer than a tenth of
    the frames may be left out (checked for these seeds on the mirror alone in tests/test_rnnt_prune_cpu.py)"""
    am, lm, txt, enc_len, txt_len = PR.lattice_range_case(seed)
    S = PR.LATTICE_RANGE_S
    _, occ = ops.RNNTSimpleLossFn.apply(am.to(DEV), lm.to(DEV), txt.to(DEV), torch.tensor(enc_len), torch.tensor(txt_len), 0)
    got = ops.rnnt_prune_ranges(occ, torch.tensor(enc_len), torch.tensor(txt_len), S).cpu().numpy()
    ops.check_errors()
    same, _ = PR.ranges(occ.cpu().numpy(), enc_len, txt_len, S)
    assert np.array_equal(got, same)
    ref = PR.simple_pass(am.double(), lm.double(), txt, enc_len, txt_len)
    want, margin = PR.ranges(ref["occ"], enc_len, txt_len, S)
    frames = left_out = 0
    for b in range(len(enc_len)):
        PR.check_invariants(got[b], enc_len[b], txt_len[b], S)
        for t in range(enc_len[b]):
            frames += 1
            if margin[b, t] < PR.MIN_RANGE_MARGIN:
                left_out += 1
                continue
            assert got[b, t] == want[b, t], (b, t, got[b].tolist(), want[b].tolist())
    print("RANGES seed", seed, "frames", frames, "left out", left_out)
    assert 10 * left_out <= frames


# ---- band joint ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("U1", [12, 1])
@pytest.mark.parametrize("S", [2, 5])
@pytest.mark.parametrize("J", [4, 6, 512])
def test_band_joint_forward_and_gradients(ops, J, S, U1):
    """B = 2, T = 5.  Utterance 0: a range sequence with repeated and maximal (S - 1) steps, the last one past the end
    (clamped by the kernel); utterance 1: all starts 0.  U1 = 1 is U + 1 < S: every k reads the one row there is"""
    B, T = 2, 5
    g = torch.Generator().manual_seed(100 * J + S + U1)
    E, P = torch.randn((B, T, J), generator=g), torch.randn((B, U1, J), generator=g)
    dH = torch.randn((B, T, S, J), generator=g)
    s = np.array([[0, 0, S - 1, S - 1, 11], [0, 0, 0, 0, 0]], np.int32)      # 11 + k runs past U1 - 1: clamped
    Pq = P
    s_d = torch.from_numpy(s).to(DEV)
    Ed, Pd = E.to(DEV).requires_grad_(True), Pq.to(DEV).requires_grad_(True)
    H = ops.RNNTJointBandFn.apply(Ed, Pd, s_d, S)
    H.backward(dH.to(DEV))
    ops.check_errors()
    # float64
    E64, P64 = E.double().requires_grad_(True), Pq.double().requires_grad_(True)
    H64 = PR.joint_band(E64, P64, s, S)
    H64.backward(dH.double())
    # the existing f32 composition on the device
    Ee, Pe = E.to(DEV).requires_grad_(True), Pq.to(DEV).requires_grad_(True)
    idx = (s_d.long().clamp(0, U1 - 1).unsqueeze(2) + torch.arange(S, device=DEV)).clamp(max=U1 - 1)
    He = torch.tanh(Ee.unsqueeze(2) + Pe[torch.arange(B, device=DEV).view(B, 1, 1), idx])
    He.backward(dH.to(DEV))
    gmax = float(dH.abs().max())
    f_fwd = 2.0 ** -23 * max(1.0, float(E.abs().max() + P.abs().max()))
    f_dE, f_dP = 4 * S * 2.0 ** -24 * gmax, 4 * T * S * 2.0 ** -24 * gmax
    for what, got, exist, want, floor in (("H", H, He, H64, f_fwd), ("dE", Ed.grad, Ee.grad, E64.grad, f_dE),
                                          ("dP", Pd.grad, Pe.grad, P64.grad, f_dP)):
        Eerr = float((exist.detach().cpu().double() - want.detach()).abs().max())
        err = float((got.detach().cpu().double() - want.detach()).abs().max())
        print("JOINT J", J, "S", S, what, "E", Eerr, "err", err, "tol", 2 * max(Eerr, floor))
        assert err <= 2 * max(Eerr, floor), what
    # rows of P no band cell reads get an exact zero
    read = set(int(v) for v in idx.cpu().flatten().tolist())
    assert len(read) < U1 or U1 == 1
    for b in range(B):
        rows_b = set(int(v) for v in idx[b].cpu().flatten().tolist())
        for u in range(U1):
            if u not in rows_b:
                assert bool((Pd.grad[b, u] == 0).all())
    # two runs: the same bits
    Ed2, Pd2 = E.to(DEV).requires_grad_(True), Pq.to(DEV).requires_grad_(True)
    H2 = ops.RNNTJointBandFn.apply(Ed2, Pd2, s_d, S)
    H2.backward(dH.to(DEV))
    assert torch.equal(H, H2) and torch.equal(Ed.grad, Ed2.grad) and torch.equal(Pd.grad, Pd2.grad)


def test_band_cells_beyond_the_transcript_get_no_gradient(ops):
    """joint -> projection -> band loss: the band cells with s + k > U_b, clamped duplicates of the last row included,
    receive an exact zero dH from the loss, so the rows of P beyond U_b (and the frames of E beyond T_b) get none"""
    B, T, U, J, V, S = 2, 6, 4, 8, 7, 5
    enc_len, txt_len = [6, 4], [4, 1]                    # utterance 1: U_b + 1 < S
    g = torch.Generator().manual_seed(5)
    E = torch.randn((B, T, J), generator=g).to(DEV).requires_grad_(True)
    P = torch.randn((B, U + 1, J), generator=g).to(DEV).requires_grad_(True)
    W = torch.randn((V, J), generator=g).to(DEV)
    txt = torch.randint(1, V, (B, U), generator=g).to(DEV)
    s = np.zeros((B, T), np.int32)
    s_d = torch.from_numpy(s).to(DEV)
    H = ops.RNNTJointBandFn.apply(E, P, s_d, S)
    H.retain_grad()
    z = ops.linear(H, W, None)
    nll = ops.RNNTBandLossFn.apply(z, txt, torch.tensor(enc_len), torch.tensor(txt_len), s_d, U + 1, 0, "sum", True)
    nll.backward()
    ops.check_errors()
    assert bool(torch.isfinite(nll))
    for b in range(B):
        assert bool((H.grad[b, :, txt_len[b] + 1:] == 0).all()) and bool((H.grad[b, enc_len[b]:] == 0).all())
        assert bool((P.grad[b, txt_len[b] + 1:] == 0).all()) and bool((E.grad[b, enc_len[b]:] == 0).all())
        assert float(P.grad[b, :txt_len[b] + 1].abs().min(1)[0].min()) > 0


# ---- band loss ----------------------------------------------------------------------------------------------------------------
def _band_existing(ops, z, txt, enc_len, txt_len, s, w):
    """ops.log_softmax, gathers and the f32 autograd recursion inside the band -> (nll [B] (+inf without a path), grad)"""
    B, T, S, V = z.shape
    zd = z.to(DEV).requires_grad_(True)
    lp = ops.log_softmax(zd.view(-1, V)).view(B, T, S, V)
    nll, total = [], None
    for b in range(B):
        sb = [int(v) for v in s[b]]
        lpb, lpl = PR.band_terms(lp[b], txt[b], sb, enc_len[b], txt_len[b], S)
        lnp = PR.band_lnp(lpb, lpl, sb, enc_len[b], txt_len[b], S)
        if lnp is None:
            nll.append(float("inf"))
            continue
        nll.append(-float(lnp.detach()))
        term = -lnp * float(w[b])
        total = term if total is None else total + term
    if total is not None:
        total.backward()
    grad = zd.grad.cpu().double() if zd.grad is not None else torch.zeros(z.shape, dtype=torch.float64)
    return torch.tensor(nll, dtype=torch.float64), grad


BAND_CASES = [(T, U, S, [3, 64, 2049][(i + j) % 3]) for i, (T, U) in enumerate(TUS) for j, S in enumerate([2, 3, 5])]
BAND_CASES += [(9, 300, 5, 3), (9, 300, 5, 64)]


@pytest.mark.parametrize("T,U,S,V", BAND_CASES)
def test_band_loss_against_float64(ops, T, U, S, V):
    """B = 3 mixed lengths; the band starts come from the rule on random occupations, so every sequence is one the head
    can meet, infeasible utterances included ((1,3) with S = 2, (9,300) with S = 5, ...): +inf nll and zero gradient"""
    B, U1, SC = 3, U + 1, 20.0
    enc_len, txt_len = _lens(T, U)
    rng = np.random.default_rng(100 * T + 10 * U + S)
    s, _ = PR.ranges(rng.random((B, T, U1)), enc_len, txt_len, S)
    g = torch.Generator().manual_seed(1000 * V + 10 * T + U + S)
    z = (torch.rand((B, T, S, V), generator=g) * 2 - 1) * SC
    txt = torch.randint(1, V, (B, max(U, 1)), generator=g)
    if U >= 2:
        txt[:, 1] = txt[:, 0]
    w = torch.tensor([1.5, -0.75, 0.5], dtype=torch.float64)
    inside = torch.zeros((B, T, S), dtype=torch.bool)
    for b in range(B):
        for t in range(enc_len[b]):
            for k in range(S):
                inside[b, t, k] = bool(s[b, t] + k <= txt_len[b])
    z_nan = z.clone()
    z_nan[~inside] = NAN                                  # rows outside the lattices are never read
    s_d, txt_d = torch.from_numpy(s).to(DEV), txt.to(DEV)
    el, tl = torch.tensor(enc_len), torch.tensor(txt_len)

    def run(consume, zs=z_nan, sl=slice(None)):
        zd = zs[sl].to(DEV).clone().requires_grad_(True)
        zin = zd.clone()                                  # a non-leaf the loss may overwrite
        n = zin.shape[0]
        nll = ops.RNNTBandLossFn.apply(zin, txt_d[sl], el[sl], tl[sl], s_d[sl].contiguous(), U1, 0, "none", consume)
        (nll * w[sl].float().to(DEV)).sum().backward()
        ops.check_errors()
        assert n == nll.shape[0]
        return nll.detach().cpu().double(), zd.grad.detach().clone()
    nll, grad_d = run(False)
    nll_in, grad_in = run(True)
    assert torch.equal(nll, nll_in) and torch.equal(grad_d, grad_in), "in place equals out of place bit for bit"
    grad = grad_d.cpu().double()

    extreme = []
    nll_r, grad_r = PR.band_pass(z.double(), txt, enc_len, txt_len, s, weight=w, extreme=extreme)
    nll_e, grad_e = _band_existing(ops, z, txt, enc_len, txt_len, s, w)
    finite = torch.isfinite(nll_r)
    feas = torch.tensor([PR.feasible(enc_len[b], txt_len[b], S) for b in range(B)])
    assert torch.equal(finite, feas) and torch.equal(torch.isfinite(nll_e), finite)
    assert bool((nll[~finite] == float("inf")).all()) and bool(torch.isfinite(nll[finite]).all())
    A = max(extreme + [float(nll_r[finite].abs().max()) if finite.any() else 0.0])
    f_row, f_nll, f_grad = _floors(T, U, SC, V, A, float(w.abs().max()))
    E_nll = float((nll_e - nll_r)[finite].abs().max()) if finite.any() else 0.0
    err_nll = float((nll - nll_r)[finite].abs().max()) if finite.any() else 0.0
    E_grad, err_grad = float((grad_e - grad_r).abs().max()), float((grad - grad_r).abs().max())
    print("BAND T", T, "U", U, "S", S, "V", V, "feasible", feas.tolist(), "| nll E", E_nll, "err", err_nll, "tol",
          2 * max(E_nll, f_nll), "| grad E", E_grad, "err", err_grad, "tol", 2 * max(E_grad, f_grad))
    assert err_nll <= 2 * max(E_nll, f_nll)
    assert not bool(torch.isnan(grad).any())
    assert err_grad <= 2 * max(E_grad, f_grad)
    assert bool((grad[~inside] == 0).all()), "cells beyond U_b and frames beyond T_b get exact zeros"
    assert bool((grad[~finite] == 0).all()), "an utterance without a path contributes exact zeros"
    if finite.any():
        assert float(grad[finite].abs().max()) > 0
    # the rest of the batch does not notice its neighbours: utterance 0 alone, the same bits
    nll0, grad0 = run(False, sl=slice(0, 1))
    assert torch.equal(nll0[0], nll[0]) and torch.equal(grad0[0], grad_d[0])


def _dense_extreme(z64, txt, enc_len, txt_len):
    """the largest |alpha|, |beta| of the float64 reference over a dense batch"""
    A = 0.0
    for b in range(z64.shape[0]):
        Tb, Ub = enc_len[b], txt_len[b]
        lpb, lpl = RR._lpb_lpl(RR.log_probs(z64[b, :Tb, :Ub + 1]), txt[b, :Ub], 0)
        A = max(A, PR.lattice_extreme(lpb.numpy(), lpl.numpy() if Ub else np.zeros((Tb, 1)), Tb, Ub))
    return A


@pytest.mark.parametrize("V", [3, 64, 2049])
@pytest.mark.parametrize("T,U,S", [(4, 1, 2), (7, 3, 4), (7, 3, 5), (3, 7, 8)])
def test_full_band_reproduces_the_dense_loss(ops, T, U, S, V):
    """S >= U + 1 and s = 0: the band holds the whole lattice.  S = U + 1: the very logits through ops.RNNTLoss give the
    same nll and gradient (the comparison is printed bit for bit and asserted within the rule); S > U + 1: the extra
    cells are outside every lattice and get zeros"""
    B, U1, SC = 3, U + 1, 20.0
    enc_len, txt_len = _lens(T, U)
    g = torch.Generator().manual_seed(77 * V + 10 * T + U + S)
    z = (torch.rand((B, T, S, V), generator=g) * 2 - 1) * SC
    txt = torch.randint(1, V, (B, U), generator=g)
    w = torch.tensor([1.5, -0.75, 0.5], dtype=torch.float64)
    s = np.zeros((B, T), np.int32)
    assert np.array_equal(PR.ranges(np.random.default_rng(0).random((B, T, U1)), enc_len, txt_len, S)[0], s)
    el, tl = torch.tensor(enc_len), torch.tensor(txt_len)

    def grads(fn, x):
        xd = x.to(DEV).requires_grad_(True)
        nll = fn(xd)
        (nll * w.float().to(DEV)).sum().backward()
        return nll.detach().cpu(), xd.grad.cpu()
    nll_b, grad_b = grads(lambda x: ops.RNNTBandLossFn.apply(x, txt.to(DEV), el, tl, torch.from_numpy(s).to(DEV), U1, 0,
                                                             "none", False), z)
    zdense = z[:, :, :U1].contiguous()
    nll_d, grad_d = grads(lambda x: ops.RNNTLoss(blank=0, reduction="none")(x, txt.to(DEV), el, tl), zdense)
    ops.check_errors()
    nll_r, grad_r = RR.batch_nll_grad(zdense.double(), txt, enc_len, txt_len, weight=w)
    A = _dense_extreme(zdense.double(), txt, enc_len, txt_len)
    f_row, f_nll, f_grad = _floors(T, U, SC, V, A, float(w.abs().max()))
    E_nll, E_grad = float((nll_d.double() - nll_r).abs().max()), float((grad_d.double() - grad_r).abs().max())
    err_nll = float((nll_b.double() - nll_r).abs().max())
    err_grad = float((grad_b[:, :, :U1].double() - grad_r).abs().max())
    print("FULLBAND T", T, "U", U, "S", S, "V", V, "bit-equal nll", torch.equal(nll_b, nll_d), "grad",
          torch.equal(grad_b[:, :, :U1], grad_d), "| nll E", E_nll, "err", err_nll, "| grad E", E_grad, "err", err_grad)
    assert err_nll <= 2 * max(E_nll, f_nll) and err_grad <= 2 * max(E_grad, f_grad)
    assert bool((grad_b[:, :, U1:] == 0).all())
