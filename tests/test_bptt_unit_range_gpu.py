"""GPU: the bf16x6 BPTT kernel (csrc/lstm_rec_bwd_bf.hip) with each wave contracting a hidden-unit range of all four
gates - and polling only that range's producers - against the f32-MFMA BPTT kernel (ASRK_REC_BF_BWD=0), which keeps the
gate-per-wave split and is not touched: the same layer, the same inputs, every gradient.

Shapes: both widths the kernel is built for (H = 512: KS/4 = 4 k-steps per gate and wave, 32 canary words per wave;
H = 1024: 8 k-steps, 64 words, LDS-resident slice tail), a full and a ragged batch group (B = 32, 17), one and two
directions, LSTM and GRU (whose gate slot 3 is now spread over the four waves), T = 3 (the first step reads nothing, no
re-arm) and T = 64 (in-kernel re-arm of region s - 2 for 62 steps).

Tolerance: that of test_lstm_bf16x6_recurrence_equals_f32_recurrence - |a - b| < 2e-5 * max(1, max|b|) per tensor.
Both kernels compute the same f32 products exactly (three-way bf16 split) and differ in summation order only.

After the bf16x6 launches every pooled exchange buffer must be all 0xFF over its armed extent: the four waves of a
workgroup together still see every producer's canary before the barrier behind which region s - 2 is refilled."""
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
PKG_NAME = "end-to-end-asr-pytorch_amd"
D = 24


def _params(g, gates, H, ndir):
    shapes = ((gates * H, D), (gates * H, H), (gates * H,), (gates * H,))
    return [torch.randn(*s, generator=g) / np.sqrt(s[-1] if len(s) > 1 else 4.0) for s in shapes * ndir]


def _pool_is_armed(ops):
    free = [e for lst in ops._xchg_pool["free"].values() for e in lst]
    assert free, "no exchange buffer went back to the pool"
    return all(bool((e[0][:e[1]] == 0xFF).all()) for e in free)


@pytest.mark.parametrize("T", [3, 64])
@pytest.mark.parametrize("kind", ["lstm", "gru"])
@pytest.mark.parametrize("ndir", [1, 2])
@pytest.mark.parametrize("B", [32, 17])
@pytest.mark.parametrize("H", [1024, 512])
def test_bptt_unit_range_waves_equal_f32_bptt(ops, monkeypatch, H, B, ndir, kind, T):
    L = importlib.import_module(PKG_NAME + "._lib").load()
    assert L.asrk_lstm_plan_is_bf(T, B, H, ndir, 1, 0) == 1, "this shape does not run lstm_rec_bwd_bf_kernel"
    if kind == "gru":
        layer = importlib.import_module(PKG_NAME + ".gru_ops").gru_layer
    else:
        layer = ops.lstm_layer
    g = torch.Generator().manual_seed(((H * 64 + B) * 4 + ndir) * 128 + T + (1 << 20) * (kind == "gru"))
    x0 = torch.randn(T, B, D, generator=g)
    p0 = _params(g, 3 if kind == "gru" else 4, H, ndir)
    dy = torch.randn(T, B, ndir * H, generator=g).to(DEV)
    grads = []
    for flag in ("1", "0"):
        monkeypatch.setenv("ASRK_REC_BF_BWD", flag)
        ops.drop_exchange_pool()
        x = x0.clone().to(DEV).requires_grad_(True)
        ps = [q.clone().to(DEV).requires_grad_(True) for q in p0]
        y = layer(x, tuple(ps[:4]), tuple(ps[4:]) if ndir == 2 else None)
        y.backward(dy)
        ops.join_deferred()
        ops.check_errors()
        grads.append([x.grad.cpu()] + [q.grad.cpu() for q in ps])
        if flag == "1":
            assert _pool_is_armed(ops), "an exchange buffer did not come back all 0xFF"
    names = ["dx"] + ["%s%s" % (n, sfx) for sfx in ("", "_reverse")[:ndir] for n in ("dw_ih", "dw_hh", "db_ih", "db_hh")]
    figures = []
    for n, a, b in zip(names, *grads):
        assert torch.isfinite(a).all(), n
        figures.append((n, (a - b).abs().max().item(), 2e-5 * max(1.0, b.abs().max().item())))
    print(kind, H, B, ndir, T, " ".join("%s %.2e/%.2e" % f for f in figures))
    assert any(not torch.equal(a, b) for a, b in zip(*grads)), "both runs took the same kernel"
    bad = [f for f in figures if not f[1] < f[2]]
    assert not bad, bad
