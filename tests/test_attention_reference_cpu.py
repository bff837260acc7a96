"""CPU: the float64 reference of the per-step attention / decoder kernels (tests/attention_reference.py) against
autograd and against itself, so that the GPU test's yardstick is not the thing that is wrong: the hand-written softmax
backward against float64 autograd of the forward on true-softmax rows, the location convolution's gradients against a
direct sum, the three chained steps by hand against autograd of the chain, the cell and embedding references against
torch's own modules."""
import pytest
import torch

from helpers import rel_err
import attention_reference as R

TIGHT = 1e-10
SMALL_ENERGY = [c for c in R.ENERGY_CASES if c.B * c.N * c.T * c.A <= 200000 and c.bwd is not None]


def test_small_energy_rows_exist_in_both_modes():
    assert {c.loc for c in SMALL_ENERGY} == {0, 1} and len(SMALL_ENERGY) >= 10


@pytest.mark.parametrize("case", SMALL_ENERGY, ids=lambda c: c.name)
def test_energy_backward_equals_autograd_on_true_softmax_rows(case):
    c = case
    t = R.energy_inputs(c)
    names = ('key', 'q') + (('c', 'Wp', 'we', 'be') if c.loc else ())
    leaf = {k: t[k].double().clone().requires_grad_(True) for k in names}
    e, attn = R.energy(c.loc, leaf['key'], leaf['q'], t['lens'], c.temp, **{k: leaf[k] for k in names[2:]})
    dattn = t['dattn'].double()
    (attn * dattn).sum().backward()
    got = R.energy_bwd(c.loc, t['key'].double(), t['q'].double(), t['lens'], c.temp, attn.detach(), dattn,
                       **{k: t[k].double() for k in names[2:]})
    for k in names:
        if k == 'be':       # vanishes for a softmax: both sides are rounding noise of the sum of |de|
            assert abs(float(got['dbe'])) <= 1e-13 * float(got['de'].abs().sum()) and abs(float(leaf[k].grad)) <= 1e-13 * float(got['de'].abs().sum())
            continue
        assert rel_err(got['d' + k], leaf[k].grad) < TIGHT, (c.name, k)
    # masking: attn is exactly 0 and e exactly -inf beyond min(len, T), rows sum to 1
    mask = R.frame_mask(t['lens'], c.N, c.T)
    assert torch.equal(attn.detach()[mask], torch.zeros(int(mask.sum()), dtype=torch.float64))
    assert bool(torch.isinf(e.detach()[mask]).all()) and bool(torch.isfinite(e.detach()[~mask]).all())
    assert float((attn.detach().sum(-1) - 1).abs().max()) < 1e-12


def test_half_mass_rows_make_dbe_a_real_quantity():
    """sum_t de = (sum attn dattn)(1 - sum attn) / temperature: far from 0 when the rows sum to 0.5"""
    c = R.ENERGY_BY_NAME['l_a63']
    t = R.energy_inputs(c)
    a = t['attn'].double()
    assert float((a.sum(-1) - 0.5).abs().max()) < 1e-6 and float(a[~R.frame_mask(t['lens'], c.N, c.T)].min()) > 0
    assert torch.equal(a[R.frame_mask(t['lens'], c.N, c.T)], torch.zeros(int(R.frame_mask(t['lens'], c.N, c.T).sum()), dtype=torch.float64))
    r = R.energy_backward_of(c, t)
    want = ((a * t['dattn'].double()).sum(-1) * (1 - a.sum(-1)) / c.temp).sum()
    assert abs(float(r['dbe']) - float(want)) < 1e-12 * float(r['de'].abs().sum())
    assert abs(float(r['dbe'])) > 1e-2 * float(r['de'].abs().sum()) / c.T ** 0.5


@pytest.mark.parametrize("case", R.CONV_CASES, ids=lambda c: c.name)
def test_loc_conv_and_its_gradients_against_the_definition(case):
    """c[b,t,k] = sum_{n,j} prev[b,n,t+j-ks] Wc[k,n,j] written as an explicit padded-window contraction, and the
    gradients autograd gives loc_conv_grads against the same contraction's two transposes"""
    c = case
    t = R.conv_inputs(c)
    prev, Wc, dc = t['prev'].double(), t['Wc'].double(), t['dc'].double()
    KW = 2 * c.ks + 1
    pad = torch.zeros(c.B, c.N, c.T + 2 * c.ks, dtype=torch.float64)
    pad[:, :, c.ks:c.ks + c.T] = prev
    win = pad.unfold(2, KW, 1)                                            # [B,N,T,KW]: prev[b,n,t+j-ks]
    ref = R.conv_reference_of(c, t)
    assert rel_err(ref['c'], torch.einsum('bntj,knj->btk', win, Wc)) < TIGHT
    assert rel_err(ref['dWc'], torch.einsum('btk,bntj->knj', dc, win)) < TIGHT
    dwin = torch.einsum('btk,knj->bntj', dc, Wc)
    dpad = torch.zeros_like(pad)
    for j in range(KW):
        dpad[:, :, j:j + c.T] += dwin[:, :, :, j]
    assert rel_err(ref['dprev'], dpad[:, :, c.ks:c.ks + c.T]) < TIGHT


@pytest.mark.parametrize("case", R.CHAIN_CASES, ids=lambda c: c.name)
def test_chained_steps_by_hand_equal_autograd_of_the_chain(case):
    cc = case
    t = R.chain_inputs(cc)
    ref = R.chain_reference_of(cc, t)
    man, de_abs = R.chain_manual_grads(cc, t)
    assert set(man) == {'d' + k for k in R.chain_params(cc)} and de_abs > 0
    for k, v in man.items():
        if k == 'dbe':      # every row is a true softmax: dbe is rounding noise on both sides
            assert abs(float(v)) < 1e-13 * de_abs and abs(float(ref[k])) < 1e-13 * de_abs
            continue
        assert rel_err(v, ref[k]) < TIGHT, (cc.name, k)
    # step 1 reaches the loss through the chain only: in loc mode its q still has a gradient, in dot mode none
    assert (float(ref['dq1'].abs().max()) > 0) == bool(cc.loc)
    # the lengths {70, 33, 1}: the length-1 row attends to frame 0 alone
    for l in range(R.CHAIN['L']):
        a = ref['attn%d' % l]
        assert torch.equal(a[2, :, 0], torch.ones(cc.N, dtype=torch.float64)) and float(a[2, :, 1:].abs().max()) == 0.0
        assert float(a[1, :, 33:].abs().max()) == 0.0 and float(a[1, :, :33].min()) > 0.0


def test_context_reference():
    c = R.CTX_CASES[3]
    t = R.ctx_inputs(c)
    a, v = t['attn'].double().requires_grad_(True), t['value'].double()
    ctx = torch.einsum('bt,btd->bd', a, v)
    ctx.backward(t['dctx'].double())
    ref = R.ctx_reference_of(c, t)
    assert rel_err(ref['ctx'], ctx.detach()) < TIGHT and rel_err(ref['dattn'], a.grad) < TIGHT
    assert int((t['attn'] == 0).sum()) > 0


@pytest.mark.parametrize("mode", R.CELL_MODES)
def test_cell_reference_equals_nn_lstm_step(mode):
    """the (i, f, g, o) cell against torch.nn.LSTM on a length-1 sequence with identity input weights"""
    B, H = 7, 37
    t = R.cell_inputs(B, H)
    ref = R.cell_reference_of(t, mode)
    lstm = torch.nn.LSTM(4 * H, H).double()
    with torch.no_grad():
        lstm.weight_ih_l0.copy_(torch.eye(4 * H)), lstm.weight_hh_l0.zero_(), lstm.bias_ih_l0.zero_(), lstm.bias_hh_l0.zero_()
    x = t['gates'].double().clone().requires_grad_(True)
    cp = t['c_prev'].double().clone().requires_grad_(True)
    _, (h, c) = lstm(x.unsqueeze(0), (torch.zeros(1, B, H, dtype=torch.float64), cp.unsqueeze(0)))
    loss = (h[0] * t['dh'].double()).sum() * (mode != 'dc') + (c[0] * t['dc'].double()).sum() * (mode != 'dh')
    loss.backward()
    assert rel_err(ref['h'], h[0].detach()) < TIGHT and rel_err(ref['cell'], c[0].detach()) < TIGHT
    assert rel_err(ref['dgates'], x.grad) < TIGHT and rel_err(ref['dc_prev'], cp.grad) < TIGHT
    assert bool(torch.isfinite(ref['gates']).all()) and float(t['gates'].abs().max()) == 90.0


@pytest.mark.parametrize("shape", R.EMB_SHAPES, ids=str)
def test_embedding_reference(shape):
    n, D, V = shape
    t = R.emb_inputs(n, D, V)
    ref = R.emb_reference_of(t)
    ok = (t['idx'] >= 0) & (t['idx'] < V)
    w = t['W'].double().clone().requires_grad_(True)
    out = torch.nn.functional.embedding(t['idx'][ok], w)
    out.backward(t['dout'].double()[ok])
    assert torch.equal(ref['emb'][ok], out.detach()) and float(ref['emb'][~ok].abs().sum()) == 0.0
    assert rel_err(ref['dW'], w.grad) < TIGHT
    seq = R.embedding_bwd_sequential_f32(t['idx'], t['dout'], t['RdW'])
    assert rel_err(seq.double() - t['RdW'].double(), ref['dW']) < 1e-5
    if n >= 7:
        assert int((~ok).sum()) == 2 and len(set(t['idx'].tolist())) < n


def test_cell_chain_reference_uses_the_middle_step_through_the_chain_only():
    t = R.cell_chain_inputs()
    ref = R.cell_chain_reference_of(t)
    assert float(ref['dx1'].abs().max()) > 0 and ref['dw_ih'].shape == (36, 13)
    assert rel_err(ref['db_ih'], ref['db_hh']) == 0.0


def test_float32_runs_give_a_rounding_scale():
    """e32 of every tensor kind is a float32 rounding figure: above 0 and far below the hard limits"""
    c = R.ENERGY_BY_NAME['l_a63']
    t = R.energy_inputs(c)
    r64, r32 = R.energy_backward_of(c, t), R.energy_backward_of(c, t, torch.float32)
    for k in ('dkey', 'dq', 'dc', 'dWp', 'dwe', 'dbe'):
        assert r32[k].dtype == torch.float32 and 0 < rel_err(r32[k], r64[k]) < 1e-5, k
    assert R.bound(0.0, 'dq') == R.FLOOR and R.bound(1.0, 'dq') == R.HARD_GRAD and R.bound(1.0, 'attn') == R.HARD_OUT
