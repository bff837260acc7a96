"""CPU: the float64 reference of the recurrence (tests/recurrence_reference.py) against the oracle.  The oracle's
lstm_layer(impl='loop') / gru_layer run in float64 under autograd on inputs that make its input projection the identity
(W_ih selects the direction's columns of x = G, biases zero except b_hn), so its outputs are the reference's Y and the
gradients it gives for x and the biases are the reference's dG and db - which the reference computes by a hand-written
BPTT from its own gates and cell states.  Everything agrees to 1e-10."""
import pytest
import torch

from oracle import asr_oracle as O
import recurrence_reference as R

TOL = 1e-10


def _inputs(B, H, ndir, gru, seed, Tn=R.T):
    g = torch.Generator().manual_seed(seed)
    G = torch.randn(Tn, B, ndir, 4, H, generator=g, dtype=torch.float64)
    bhn = torch.randn(ndir, H, generator=g, dtype=torch.float64)
    if gru:
        G[:, :, :, 3] = bhn
    whh = [torch.randn((3 if gru else 4) * H, H, generator=g, dtype=torch.float64) * min(0.4, 1.5 / H ** 0.5)
           for _ in range(ndir)]
    return G.reshape(Tn * B, ndir * 4 * H), whh, bhn, g


def _oracle_sd(H, ndir, whh, gru, bhn):
    """state dict under which the oracle's input projection copies direction d's gate columns out of x"""
    ng = 3 if gru else 4
    sd = {}
    for d, sfx in enumerate(("", "_reverse")[:ndir]):
        w_ih = torch.zeros(ng * H, ndir * 4 * H, dtype=torch.float64)
        w_ih[:, d * 4 * H:d * 4 * H + ng * H] = torch.eye(ng * H, dtype=torch.float64)
        b_hh = torch.zeros(ng * H, dtype=torch.float64)
        if gru:
            b_hh[2 * H:] = bhn[d]
        sd["l.weight_ih_l0" + sfx] = w_ih
        sd["l.weight_hh_l0" + sfx] = whh[d]
        sd["l.bias_ih_l0" + sfx] = torch.zeros(ng * H, dtype=torch.float64).requires_grad_(True)
        sd["l.bias_hh_l0" + sfx] = b_hh.requires_grad_(True)
    return sd


def _close(a, b):
    if a.numel() == 0:
        return a.shape == b.shape
    return float((a - b).abs().max()) <= TOL * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize("B,H,ndir", [(3, 20, 2), (2, 12, 1)])
@pytest.mark.parametrize("mode", R.MODES, ids=lambda m: R.MODE_NAMES[m])
def test_lstm_reference_matches_oracle_autograd(B, H, ndir, mode):
    Tn, (pm, r) = R.T, mode
    G, whh, bhn, g = _inputs(B, H, ndir, False, 3)
    Y, C, A = R.lstm_fwd(G, whh, Tn, B, H, ndir)
    dY2 = torch.randn(*R.dy_shape(pm, r, Tn, B, ndir * H), generator=g, dtype=torch.float64)
    dG, db = R.lstm_bwd(A, whh, C, R.expand_dy(dY2, pm, r, Tn), Tn, B, H, ndir)

    x = G.reshape(Tn, B, -1).transpose(0, 1).clone().requires_grad_(True)          # the oracle is batch-major
    sd = _oracle_sd(H, ndir, whh, False, bhn)
    y = O.lstm_layer(x, sd, "l.", ndir == 2, impl="loop")                          # [B, T, ndir*H]
    assert _close(Y, y.detach().transpose(0, 1))
    # the time reduction exactly as src/module.py:141-153 writes it, on the oracle's batch-major output
    if pm == 2:
        y2 = y[:, ::r, :].contiguous()
    elif pm == 1:
        yy = y[:, :-(Tn % r), :] if Tn % r else y
        y2 = yy.contiguous().view(B, Tn // r, ndir * H * r)
    else:
        y2 = y
    Y2 = R.reduce_time(Y, pm, r) if pm else Y
    assert _close(Y2, y2.detach().transpose(0, 1))
    (y2 * dY2.transpose(0, 1)).sum().backward()
    assert _close(dG, x.grad.transpose(0, 1))
    for d, sfx in enumerate(("", "_reverse")[:ndir]):
        assert _close(db[d * 4 * H:(d + 1) * 4 * H], sd["l.bias_ih_l0" + sfx].grad)
        assert _close(db[d * 4 * H:(d + 1) * 4 * H], sd["l.bias_hh_l0" + sfx].grad)
    # the states the BPTT consumed are the forward's own: c_t = f c_{t-1} + i g and h = o tanh(c), per direction
    A5, C4 = A.reshape(Tn, B, ndir, 4, H), C.reshape(Tn, B, ndir, H)
    assert _close(Y.reshape(Tn, B, ndir, H), A5[:, :, :, 3] * torch.tanh(C4))
    assert _close(C4[0, :, 0], A5[0, :, 0, 0] * A5[0, :, 0, 2])
    assert _close(C4[1, :, 0], A5[1, :, 0, 1] * C4[0, :, 0] + A5[1, :, 0, 0] * A5[1, :, 0, 2])
    if ndir == 2:
        assert _close(C4[Tn - 1, :, 1], A5[Tn - 1, :, 1, 0] * A5[Tn - 1, :, 1, 2])


@pytest.mark.parametrize("B,H,ndir", [(3, 20, 2), (2, 12, 1)])
@pytest.mark.parametrize("mode", R.MODES, ids=lambda m: R.MODE_NAMES[m])
def test_gru_reference_matches_oracle_autograd(B, H, ndir, mode):
    Tn, (pm, r) = R.T, mode
    G, whh, bhn, g = _inputs(B, H, ndir, True, 5)
    Y, A = R.gru_fwd(G, whh, Tn, B, H, ndir)
    dY2 = torch.randn(*R.dy_shape(pm, r, Tn, B, ndir * H), generator=g, dtype=torch.float64)
    dG, db = R.gru_bwd(A, whh, Y, R.expand_dy(dY2, pm, r, Tn), Tn, B, H, ndir)

    x = G.reshape(Tn, B, -1).transpose(0, 1).clone().requires_grad_(True)
    sd = _oracle_sd(H, ndir, whh, True, bhn)
    y = O.gru_layer(x, sd, "l.", ndir == 2)
    assert _close(Y, y.detach().transpose(0, 1))
    Y2 = R.reduce_time(Y, pm, r) if pm else Y
    (y.transpose(0, 1) * R.expand_dy(dY2, pm, r, Tn)).sum().backward()
    xg = x.grad.transpose(0, 1).reshape(Tn, B, ndir, 4, H)
    dG5 = dG.reshape(Tn, B, ndir, 4, H)
    assert _close(dG5[:, :, :, :3], xg[:, :, :, :3])                               # dr | dz | dn: the input side
    A5 = A.reshape(Tn, B, ndir, 4, H)
    assert _close(dG5[:, :, :, 3], dG5[:, :, :, 2] * A5[:, :, :, 0])               # dn * r
    for d, sfx in enumerate(("", "_reverse")[:ndir]):
        dbd = db[d * 4 * H:(d + 1) * 4 * H]
        assert _close(dbd[:3 * H], sd["l.bias_ih_l0" + sfx].grad)                  # db_ih = blocks 0..2
        assert _close(torch.cat([dbd[:2 * H], dbd[3 * H:]]), sd["l.bias_hh_l0" + sfx].grad)   # db_hh = 0, 1, 3
    assert Y2.shape == R.dy_shape(pm, r, Tn, B, ndir * H)


@pytest.mark.parametrize("mode", R.MODES, ids=lambda m: R.MODE_NAMES[m])
def test_lens_form_is_every_row_alone_and_unpadded(mode):
    """against the oracle run on each utterance by itself (batch 1, its own length), as the reference decodes"""
    Tn, B, H, ndir, (pm, r) = R.T, 5, 12, 2, mode
    G, whh, bhn, _ = _inputs(B, H, ndir, False, 9)
    lens = torch.tensor([1, 7, 4, 2, 5])
    Y, C, A, valid = R.lstm_fwd_len(G, whh, lens, Tn, B, H, ndir)
    Y2 = R.reduce_time(Y, pm, r, lens) if pm else None
    sd = _oracle_sd(H, ndir, whh, False, bhn)
    G3 = G.reshape(Tn, B, -1)
    for b in range(B):
        n = int(lens[b])
        y = O.lstm_layer(G3[:n, b][None], sd, "l.", True, impl="loop")[0].detach()     # [n, ndir*H]
        assert _close(Y[:n, b], y)
        assert bool((Y[n:, b] == 0).all() and (C[n:, b] == 0).all() and (A[n:, b] == 0).all())
        assert bool(valid[:n, b].all()) and not bool(valid[n:, b].any())
        if pm == 1:                                       # 'concat' trims lens[b] % r frames of this row by itself
            assert _close(Y2[:n // r, b], y[:(n // r) * r].reshape(n // r, r * ndir * H))
            assert bool((Y2[n // r:, b] == 0).all())
        elif pm == 2:
            assert _close(Y2[:-(-n // r), b], y[::r]) and bool((Y2[-(-n // r):, b] == 0).all())
    # a full-length row of the lens form is the plain form
    Yp, Cp, Ap = R.lstm_fwd(G, whh, Tn, B, H, ndir)
    assert _close(Y[:, 1], Yp[:, 1]) and _close(C[:, 1], Cp[:, 1]) and _close(A[:, 1], Ap[:, 1])


def test_reduced_layouts_round_trip():
    """expand_dy is the adjoint of reduce_time: <reduce(Y), D> == <Y, expand(D)> for every mode"""
    g = torch.Generator().manual_seed(1)
    Y = torch.randn(R.T, 3, 10, generator=g, dtype=torch.float64)
    for pm, r in R.MODES[1:]:
        D = torch.randn(*R.dy_shape(pm, r, R.T, 3, 10), generator=g, dtype=torch.float64)
        a = float((R.reduce_time(Y, pm, r) * D).sum())
        b = float((Y * R.expand_dy(D, pm, r, R.T)).sum())
        assert abs(a - b) < 1e-10
        dropped = R.expand_dy(torch.ones_like(D), pm, r, R.T)[:, 0, 0]
        want = [1.0 if (t % r == 0 if pm == 2 else t < (R.T // r) * r) else 0.0 for t in range(R.T)]
        assert dropped.tolist() == want


def test_table_inputs_are_f32_values_and_tolerances_stay_under_the_project_bar():
    c = R.CASE_BY_NAME["f_1x1_k4"]
    G, whh, dY = R.make_inputs(c)
    for x in (G, whh[0], dY):
        assert bool((x.float().double() == x).all())
    assert float(whh[0].std()) < 0.4
    e = R.e32(c)
    assert set(e) == {"Y", "C", "gates"} and all(0 < v < 1e-5 for v in e.values())
    assert R.MARGIN == 8.0 and R.CEILING == 1e-3


def test_bounds_would_catch_one_dropped_k_column():
    """what the 1e-3 bar alone can miss: W_hh with ONE of 516 columns zeroed moves every forward tensor and dG by far
    more than the derived bound of that case (and db of the backward case), in exact arithmetic"""
    for name, kinds in (("f_2x2_k16_sb", ("Y", "C", "gates", "Y2")), ("b_8x2", ("dG", "db"))):
        c = R.CASE_BY_NAME[name]
        G, whh, dY = R.make_inputs(c)
        broken = [w.clone() for w in whh]
        broken[0][:, 515] = 0
        got = R._run(c, G, broken, dY, torch.float64)
        ref = R.reference(c)
        for k in kinds:
            assert R.rel_err(got[k], ref[k]) > 10 * R.bound(c, k), (name, k)
            assert R.bound(c, k) < 1e-5
