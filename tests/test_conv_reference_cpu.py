"""CPU: self-checks of what tests/test_conv_variants_gpu.py judges by (tests/conv_reference.py) - the length-aware
reference against its batch-1 definition, autograd's gradients against the three sums written at the top of
csrc/conv3x3.hip, the float32-vs-float64 figure e32 of every row, the layouts, and that every hlen / ties /
uncovered-input row has the property it is named for."""
import pytest
import torch
import torch.nn.functional as F

from helpers import rel_err
import conv_reference as R


@pytest.mark.parametrize("case", R.LEN_CASES, ids=lambda c: c.name)
def test_len_reference_is_the_batch1_run_of_every_image(case):
    """src/decode.py:88 decodes batch 1: image i of the padded batch = the convolution of that image cropped to its
    hlen rows - for the given hlen, and with hlen above H / below 0"""
    c, t = case, R.make_inputs(case)
    x, w, b = (t[k].double() for k in ('x', 'w', 'b'))
    for hlen in (c.hlen, tuple(h + 3 if h == c.H else -2 if h == 0 else h for h in c.hlen)):
        y = R.reference_of(c, t, hlen=hlen)['y']
        oh = R.out_hlen_of(c, hlen)
        for i, h in enumerate(hlen):
            h = max(0, min(h, c.H))
            n = h if oh is None else oh[i]
            assert float(y[i, :, n:].abs().max() if n < y.shape[2] else 0.0) == 0.0
            if h + 2 * c.p[0] < c.k[0]:
                assert n == 0                          # nothing to crop to: the kernel does not fit
                continue
            one = R.conv_reference(x[i:i + 1, :, :h], w, b, c.s, c.p, c.relu)
            assert one.shape[2] >= n > 0 or h <= 1
            # two float64 runs of one library on two shapes: equal to its summation order
            assert rel_err(y[i, :, :n], one[0, :, :n]) < 1e-13, (c.name, i)
    assert torch.equal(R.reference_of(c, t)['y'],
                       R.reference_of(c, t, hlen=tuple(h + 3 if h == c.H else h for h in c.hlen))['y'])
    assert torch.equal(R.reference_of(c, t)['y'],
                       R.reference_of(c, t, hlen=tuple(-2 if h == 0 else h for h in c.hlen))['y'])


def _three_sums(x, w, b, dy):
    """the sums at the top of csrc/conv3x3.hip in float64, positions (h, w), taps (kh, kw), 3x3 / stride 1 / pad 1:
    y[pos, n] = bias[n] + sum_{tap, c} x[pos + tap - (1,1), c] w[n][c][tap]
    dW[co][ci][tap] = sum_pos dy[pos, co] x[pos + tap - (1,1), ci];  db[co] = sum_pos dy[pos, co]
    dx[pos, c] = sum_{tap, n} dy[pos - tap + (1,1), n] w[n][c][tap]"""
    B, C, H, W = x.shape
    xp, dyp = F.pad(x, (1, 1, 1, 1)), F.pad(dy, (1, 1, 1, 1))
    y = b.view(1, -1, 1, 1).expand(B, w.shape[0], H, W).clone()
    dw, dx = torch.zeros_like(w), torch.zeros_like(x)
    for kh in range(3):
        for kw in range(3):
            xs = xp[:, :, kh:kh + H, kw:kw + W]
            y += torch.einsum('bchw,nc->bnhw', xs, w[:, :, kh, kw])
            dw[:, :, kh, kw] = torch.einsum('bnhw,bchw->nc', dy, xs)
            dx += torch.einsum('bnhw,nc->bchw', dyp[:, :, 2 - kh:2 - kh + H, 2 - kw:2 - kw + W], w[:, :, kh, kw])
    return y, dx, dw, dy.sum(dim=(0, 2, 3))


@pytest.mark.parametrize("B,H,W,C,Cout", [(2, 3, 4, 2, 3), (1, 5, 1, 3, 2)])
def test_autograd_gradients_are_the_three_sums(B, H, W, C, Cout):
    g = torch.Generator().manual_seed(H * W)
    x, w, b, dy = (torch.randn(*s, generator=g, dtype=torch.float64)
                   for s in ((B, C, H, W), (Cout, C, 3, 3), (Cout,), (B, Cout, H, W)))
    xr, wr, br = (v.clone().requires_grad_(True) for v in (x, w, b))
    yr = R.conv_reference(xr, wr, br, (1, 1), (1, 1), False)
    yr.backward(dy)
    for got, want in zip((yr.detach(), xr.grad, wr.grad, br.grad), _three_sums(x, w, b, dy)):
        assert rel_err(got, want) < 1e-14
    # with the ReLU, dy counts where the output is positive (the kernels' xmask / ymask)
    xr, wr, br = (v.clone().requires_grad_(True) for v in (x, w, b))
    yr = R.conv_reference(xr, wr, br, (1, 1), (1, 1), True)
    yr.backward(dy)
    gate = (yr.detach() > 0).double()
    assert 0 < float(gate.mean()) < 1
    for got, want in zip((xr.grad, wr.grad, br.grad), _three_sums(x, w, b, dy * gate)[1:]):
        assert rel_err(got, want) < 1e-14


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_e32_is_finite_and_nonzero(case):
    t = R.make_inputs(case)
    assert R.make_inputs(case) is t
    ref, r32 = R.reference_of(case, t), R.reference_of(case, t, dtype=torch.float32)
    assert set(ref) == set(r32) == ({'y'} if case.mode == 'len' else {'y'} | {'d' + k for k in case.grads})
    for k in ref:
        assert r32[k].dtype == torch.float32 and ref[k].dtype == torch.float64
        e32 = rel_err(r32[k], ref[k])
        assert 0.0 < e32 < 1e-5, (case.name, k, e32)
        assert R.bound(e32, 1.0, k) <= R.HARD[k]
    assert not t['x'].requires_grad and t['x'].grad is None
    if case.mode == 'train':
        # dy is random and dense; it is 0 exactly where the ReLU's gate could flip under float32 rounding
        zero = t['dy'] == 0
        if case.relu:
            pre = R.conv_reference(t['x'].double(), t['w'].double(), t['b'].double(), case.s, case.p, False).abs()
            assert float(zero.double().mean()) < 1e-3
            assert bool(zero[pre < R.GATE_EPS / 2].all())
            assert int(zero.sum()) <= int((pre < 2 * R.GATE_EPS).sum()) + 2           # randn itself may return a 0.0
            assert torch.equal(r32['y'] > 0, ref['y'] > 0) or bool((t['dy'][(r32['y'] > 0) != (ref['y'] > 0)] == 0).all())
        else:
            assert int(zero.sum()) <= 2


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_layout_addresses_every_element_once(case):
    c = case
    idx = R.layout_index(c)
    assert idx.shape == (c.B, c.C, c.H, c.W) and int(idx.min()) == 0
    assert idx.unique().numel() == idx.numel()
    sb, sh, sw, sc = R.strides(c)
    assert int(idx[-1, -1, -1, -1]) == (c.B - 1) * sb + (c.H - 1) * sh + (c.W - 1) * sw + (c.C - 1) * sc
    assert int(idx.max()) + 1 == idx.numel()           # dense: the device tensor holds nothing else


def test_named_properties_hold():
    for name in R.UNCOVERED:
        c = R.BY_NAME[name]
        unc = R.uncovered_inputs(c)
        assert 0 < int(unc.sum()) < unc.numel()
        dx = R.reference_of(c, R.make_inputs(c))['dx']
        assert float(dx[:, :, unc].abs().max()) == 0.0 and float(dx[:, :, ~unc].abs().min()) > 0.0
    for c in R.TRAIN_CASES:
        if c.name not in R.UNCOVERED:
            assert not bool(R.uncovered_inputs(c).any()) or c.layout == 'cnn' or c.k == (5, 5), c.name
    for c in R.LEN_CASES:
        x = R.make_inputs(c)['x']
        for i, h in enumerate(c.hlen):
            if h < c.H:
                assert float(x[i, :, h:].abs().min()) > 0.0        # the padding is not zero: the kernels must mask it
    # pooling: many windows tie (at 0), and F.max_pool2d sends the gradient of a tied window to its FIRST maximum
    x, dy = R.pool_ties_input()
    win = x.unfold(2, 2, 2).unfold(3, 2, 2).reshape(*x.shape[:2], 4, 7, 4)
    tied = (win == win.max(dim=-1, keepdim=True).values).sum(dim=-1) > 1
    assert float(tied.double().mean()) > 0.04
    xr = x.clone().requires_grad_(True)
    F.max_pool2d(xr, 2, stride=2).backward(dy)
    gw = xr.grad.unfold(2, 2, 2).unfold(3, 2, 2).reshape(*x.shape[:2], 4, 7, 4)
    first = (win == win.max(dim=-1, keepdim=True).values).double().argmax(dim=-1)
    assert torch.equal(gw.gather(-1, first.unsqueeze(-1)).squeeze(-1), dy)
    assert int((gw != 0).sum()) <= dy.numel()
    # relu_bwd: zeros of both signs where the gradient must stop
    y, g = R.relu_zero_input()
    assert int((y == 0).sum()) > 2000 and bool(torch.signbit(y[::7]).all()) and int((y > 0).sum()) > 1000
