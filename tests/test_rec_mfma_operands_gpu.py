"""GPU: the bf16x6 recurrence kernels around the operand-form MFMA statements of the forward fast path
(csrc/lstm_rec_fwd_bf.hip: mfma_res reads the resident W_hh planes from the accumulator half of the register file,
mfma_reg the LDS planes and the step that stays in VGPRs; csrc/lstm_rec_common.h) against the untouched f32-MFMA kernels:
one layer, forward and backward, through ops.lstm_layer / gru_ops.gru_layer, as tests/test_bptt_unit_range_gpu.py does.
The BPTT kernel (csrc/lstm_rec_bwd_bf.hip) kept its builtins - the same statements and a per-step scalar fragment base
were measured there and taken out again - and is covered here at the same shapes, so
that the next attempt on it starts with its test.

References: ASRK_REC_BF=0 for the forward output, ASRK_REC_BF_BWD=0 (same bf16x6 forward) for every gradient; bound of
that file, |a - b| < 2e-5 * max(1, max|b|) per tensor - both sides compute the same f32 products exactly (three-way bf16
split) and differ in summation order only.  The plan (asrk_lstm_plan_is_bf) says which launches are bf16x6: the BPTT of
every shape below, the forward of most (a forward the plan gives to the f32 kernel must then equal the reference bit
for bit); where the two runs differ in kernel and an MFMA ran (T >= 2) their results must not be identical.

Shapes, the smallest at which the changed code can go wrong:
  H = 1024: the 16-unit forward plan keeps 7 of its 8 k-steps' register planes in AGPRs and the last in VGPRs, plane 0 in
            LDS: one wave takes every operand form in one step; the BPTT slice crosses from registers to LDS at k-step
            21, inside gate 2.  H = 512: 8-unit forward plans (one register plane), all-register BPTT slice.
  T = 1 (no MFMA), 2 (first hand-off, no re-arm), 3 (first re-arm), 9 (every slot of the 8-deep fragment ring refilled).
  B = 32 (full groups), 17 (ragged second group), 5 (one group whose padded rows take the out-of-range vector offset).
  One and two directions, LSTM and GRU (its zero gate slot goes through the same operands).
  Panels: the matrix runs with the panels refused (ops._REC_PANELS False; a pooled panel would otherwise appear from a
  shape's second request on and change the route between repeats); two cases at H = 1024, two directions, needs_dx
  run the LSTM with both dG panels and ASRK_REC_BWD_NO_DG (a warm-up pass makes the pool hand panels out) and with
  the panels refused.  The panel stores share scalars with the fragment addressing.

W_hh has a wide dynamic range along K: block j of 32 input columns is scaled by 2**(j % 9 - 4), so a fragment read at a
wrong k-step moves the result far above the bound instead of averaging out.  The factors are then divided by their root
mean square (6.2), so that a row of W_hh has the norm 1 it has in test_bptt_unit_range_gpu.py, whose bound this is: with
the bare factors the recurrence has a gain of 6 per step and amplifies the summation-order difference between ANY two
kernels - 1.8e-6 at T = 2, 3.3e-6 at T = 3, 4.8e-5 at T = 9 for the GRU's Y - past a bound set for unit gain.  The
ratios between the blocks, 2 to 256, are what a misplaced fragment meets, and they are unchanged.

Every case runs three times on fresh tensors built from the same seed: the forward outputs (Y, the gates, the LSTM's
cell state) and the BPTT kernel's own output must be BITWISE equal across the repeats - a missing wait state corrupts
some waves of some launches, which one comparison against a reference need not see.  The BPTT kernel's output is the
f32 dG it stores in place over the gates; dx is that dG through the input-gradient GEMM, which by default splits K
across workgroups and adds the partial sums with f32 atomics (ASRK_DETERMINISTIC, read once when the library loads,
turns that off): at T = 1, where the recurrence runs no MFMA at all, dx already differs by 4.8e-7 from run to run.  So
dG is what is compared bit for bit, and dx, like dw_* and db_*, is held to the bound.  Where the plan skips the f32 dG
(panels on) dx comes from the kernel's dG panel through the panel GEMM, which never splits K: there dx is compared bit
for bit.  After every bf16x6 run the pooled exchange buffers must be all 0xFF."""
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
PKG_NAME = "end-to-end-asr-pytorch_amd"
D = 24
REPEATS = 3


def _params(g, gates, H, ndir):
    out = []
    scale = torch.tensor([2.0 ** (j % 9 - 4) for j in range(H // 32)]).repeat_interleave(32)
    scale = scale / scale.pow(2).mean().sqrt()      # a row keeps the norm of test_bptt_unit_range_gpu.py's rows
    for _ in range(ndir):
        out.append(torch.randn(gates * H, D, generator=g) / np.sqrt(D))
        out.append(torch.randn(gates * H, H, generator=g) / np.sqrt(H) * scale[None, :])
        out.append(torch.randn(gates * H, generator=g) / 2.0)
        out.append(torch.randn(gates * H, generator=g) / 2.0)
    return out


def _pool_is_armed(ops):
    free = [e for lst in ops._xchg_pool["free"].values() for e in lst]
    assert free, "no exchange buffer went back to the pool"
    return all(bool((e[0][:e[1]] == 0xFF).all()) for e in free)


def _run(ops, layer, x0, p0, dy, ndir, kind, backward=True):
    """one forward (+ backward) on fresh tensors: (forward outputs, gradients), all on the CPU"""
    ops.drop_exchange_pool()
    x = x0.clone().to(DEV).requires_grad_(True)
    ps = [q.clone().to(DEV).requires_grad_(True) for q in p0]
    y = layer(x, tuple(ps[:4]), tuple(ps[4:]) if ndir == 2 else None)
    # LSTMLayerFn saves (xc, w_ih_f, w_hh_f, w_ih_r, w_hh_r, G, C, Y, w_stack), GRURecLayerFn (..., G, Y): G holds the
    # activated gates after the forward and, in place, the BPTT kernel's f32 dG after the backward
    saved = y.grad_fn.saved_tensors
    G = saved[5]
    fwd = [y.detach().cpu(), G.detach().cpu().clone()] + ([saved[6].detach().cpu().clone()] if kind == "lstm" else [])
    grads = dG = None
    if backward:
        y.backward(dy)
        ops.join_deferred()
        grads = [x.grad.cpu()] + [q.grad.cpu() for q in ps]
        dG = G.detach().cpu().clone()
    ops.check_errors()
    return fwd, grads, dG


def _check(ops, monkeypatch, kind, H, B, ndir, T, warmup=0, dg_stored=True):
    L = importlib.import_module(PKG_NAME + "._lib").load()
    fwd_bf = L.asrk_lstm_plan_is_bf(T, B, H, ndir, 0, 0) == 1
    assert L.asrk_lstm_plan_is_bf(T, B, H, ndir, 1, 0) == 1, "this shape does not run lstm_rec_bwd_bf_kernel"
    assert L.asrk_lstm_plan_is_bf(T, B, H, ndir, 1, 1) == 0 and L.asrk_lstm_plan_is_bf(T, B, H, ndir, 0, 1) == 0
    layer = importlib.import_module(PKG_NAME + ".gru_ops").gru_layer if kind == "gru" else ops.lstm_layer
    g = torch.Generator().manual_seed(((H * 64 + B) * 4 + ndir) * 128 + T + (1 << 20) * (kind == "gru") + (1 << 21))
    x0 = torch.randn(T, B, D, generator=g)
    p0 = _params(g, 3 if kind == "gru" else 4, H, ndir)
    dy = torch.randn(T, B, ndir * H, generator=g).to(DEV)

    monkeypatch.setenv("ASRK_REC_BF", "1")
    monkeypatch.setenv("ASRK_REC_BF_BWD", "1")
    for _ in range(warmup):
        _run(ops, layer, x0, p0, dy, ndir, kind)
    runs = []
    for _ in range(REPEATS):
        runs.append(_run(ops, layer, x0, p0, dy, ndir, kind))
        assert _pool_is_armed(ops), "an exchange buffer did not come back all 0xFF"
    monkeypatch.setenv("ASRK_REC_BF_BWD", "0")
    _, g_ref, _ = _run(ops, layer, x0, p0, dy, ndir, kind)
    monkeypatch.setenv("ASRK_REC_BF", "0")
    f_ref, _, _ = _run(ops, layer, x0, p0, dy, ndir, kind, backward=False)

    fwd, grads, dG = runs[0]
    fnames = ["Y", "G", "C"][:len(fwd)]
    gnames = ["dx"] + ["%s%s" % (n, sfx) for sfx in ("", "_reverse")[:ndir] for n in ("dw_ih", "dw_hh", "db_ih", "db_hh")]
    for r in range(1, REPEATS):
        for n, a, b in zip(fnames, fwd, runs[r][0]):
            assert torch.equal(a, b), "%s differs between repeat 0 and %d: max %.3e" % (n, r, (a - b).abs().max().item())
        if dg_stored:
            assert torch.equal(dG, runs[r][2]), "dG differs between repeat 0 and %d: max %.3e" % (
                r, (dG - runs[r][2]).abs().max().item())
        else:
            assert torch.equal(grads[0], runs[r][1][0]), "dx differs between repeat 0 and %d: max %.3e" % (
                r, (grads[0] - runs[r][1][0]).abs().max().item())

    figures = []
    for r in range(REPEATS):
        # the f32 reference's gates / cell state are the same quantities: all three forward tensors are held to the bound
        for n, a, b in zip(fnames, runs[r][0], f_ref):
            assert torch.isfinite(a).all(), n
            figures.append((n, (a - b).abs().max().item(), 2e-5 * max(1.0, b.abs().max().item())))
        for n, a, b in zip(gnames, runs[r][1], g_ref):
            assert torch.isfinite(a).all(), n
            figures.append((n, (a - b).abs().max().item(), 2e-5 * max(1.0, b.abs().max().item())))
    n1 = len(fnames) + len(gnames)
    print(kind, H, B, ndir, T, "fwd_bf=%d" % fwd_bf, " ".join("%s %.2e/%.2e" % f for f in figures[:n1]))
    if fwd_bf:
        if T >= 2:
            assert not torch.equal(fwd[0], f_ref[0]), "both forward runs took the same kernel"
    else:
        assert torch.equal(fwd[0], f_ref[0]), "the plan gives both forward runs the f32 kernel, yet they differ"
    if T >= 2:
        assert any(not torch.equal(a, b) for a, b in zip(grads, g_ref)), "both backward runs took the same kernel"
    bad = [f for f in figures if not f[1] < f[2]]
    assert not bad, bad


@pytest.mark.parametrize("T", [1, 2, 3, 9])
@pytest.mark.parametrize("kind,ndir", [("lstm", 1), ("lstm", 2), ("gru", 1), ("gru", 2)])
@pytest.mark.parametrize("B", [32, 17, 5])
@pytest.mark.parametrize("H", [1024, 512])
def test_resident_fragment_operands_equal_f32_kernels(ops, monkeypatch, H, B, kind, ndir, T):
    monkeypatch.setattr(ops, "_REC_PANELS", False)
    _check(ops, monkeypatch, kind, H, B, ndir, T)


@pytest.mark.parametrize("panels", [True, False])
def test_resident_fragment_operands_with_and_without_panels(ops, monkeypatch, panels):
    H, B, ndir, T = 1024, 32, 2, 9
    monkeypatch.setattr(ops, "_REC_PANELS", panels)
    monkeypatch.setattr(ops, "_REC_SKIP_DG", True)
    st0 = dict(ops._panel_state["stats"])
    # the plan asks the split GEMM's routing rule whether dX / dW would multiply panels; at M = T * B = 288 tokens it
    # says no unless the split is forced (mode 2, as for bench.py's comparisons) - in both cases, so that they differ in
    # the panels alone.  The pool hands a panel out from a shape's second request on: one warm-up pass, then every
    # repeat writes both.
    split0 = ops.get_gemm_split()
    ops.set_gemm_split(2)
    try:
        _check(ops, monkeypatch, "lstm", H, B, ndir, T, warmup=1 if panels else 0, dg_stored=not panels)
    finally:
        ops.set_gemm_split(split0)
    st1 = ops._panel_state["stats"]
    got = tuple(st1[k] - st0[k] for k in ("dg", "dgt", "no_dg"))
    print("panels", panels, "dG panel %d, dG^T panel %d, f32 dG stores skipped %d" % got)
    if panels:
        # the three compared repeats; the ASRK_REC_BF_BWD=0 reference run writes no panel
        assert got[0] >= REPEATS and got[1] >= REPEATS and got[2] >= REPEATS, got
    else:
        assert got == (0, 0, 0), got
