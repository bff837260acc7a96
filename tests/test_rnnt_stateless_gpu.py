"""GPU: the kernels of the stateless prediction network (csrc/rnnt_ctx.hip) against the float64 mirrors of
tests/rnnt_stateless_reference.py, on shapes (B, U1, D, C) that reach every path: the minimum, U1 < C, D with a scalar
tail, D over one 256-lane tile with the largest C, the real head width.

 * exact inputs (multiples of 1/8: every product and sum is exact in f32): Y, dX and dw equal the mirror exactly, with
   pre-activations that are exactly 0 (derivative 0) and negative ones among them;
 * normal inputs: err <= 2 * max(E, floor), E the error against the same float64 values of the f32 composition that
   exists without the kernels (F.pad + F.conv1d + relu and their autograd, evaluated by torch on the host), floor =
   K 2^-23 max|want| with K = C + 1 for Y and dX (C products, C - 1 sums, the input rounding) and K = B*U1 + C for dw;
   elements whose float64 pre-activation lies within 1e-5 of 0 (under 1 % of them) are left out of the backward
   comparison, with everything their sign reaches;
 * two backward runs are bit-equal; row-strided X / Y give the contiguous result;
 * the decode step for int32 and int64 tokens, n_tok over {0, 1, C-1, C, Lc}: bit-equal to the matching row of the
   forward on the same labels; a label outside [0, V) makes that row NaN and no other; nothing around the rows is
   written."""
import functools

import numpy as np
import pytest
import torch

import rnnt_stateless_reference as SR

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 2.0 ** -23


@functools.lru_cache(maxsize=None)
def _mirror(shape, kind):
    """the inputs and the float64 results of one case, computed once and shared (read-only)"""
    X, w, dY = SR.exact_case(shape) if kind == "exact" else SR.random_case(shape)
    Y = SR.fwd_loops(X, w)
    dX, dw = SR.bwd_loops(X, w, dY)
    out = dict(X=X, w=w, dY=dY, Y=Y, dX=dX, dw=dw, A=SR.pre_loops(X, w))
    for a in out.values():
        a.setflags(write=False)
    return out


def _device_pass(ops, m):
    X = torch.tensor(m["X"], device=DEV).requires_grad_(True)
    w = torch.tensor(m["w"], device=DEV).requires_grad_(True)
    Y = ops.RNNTContextFn.apply(X, w)
    Y.backward(torch.tensor(m["dY"], device=DEV))
    ops.check_errors()
    assert Y.shape == X.shape and X.grad.shape == X.shape and w.grad.shape == w.shape
    return Y.detach().cpu().numpy(), X.grad.cpu().numpy(), w.grad.cpu().numpy()


@pytest.mark.parametrize("shape", SR.KERNEL_SHAPES)
def test_exact_inputs_equal_the_mirror_exactly(ops, shape):
    m = _mirror(shape, "exact")
    A = m["A"]
    if A.size > 1:
        assert (A == 0).any() and (A < 0).any(), "the case holds no exactly-zero / no negative pre-activation"
    Y, dX, dw = _device_pass(ops, m)
    for what, got in (("Y", Y), ("dX", dX), ("dw", dw)):
        assert got.dtype == np.float32
        assert np.array_equal(got.astype(np.float64), m[what]), (shape, what, np.abs(got - m[what]).max())


@pytest.mark.parametrize("shape", SR.KERNEL_SHAPES)
def test_normal_inputs_within_the_existing_composition_s_error(ops, shape):
    B, U1, D, C = shape
    m = _mirror(shape, "random")
    near = np.abs(m["A"]) <= SR.NEAR_ZERO
    assert near.mean() < 0.01
    # what the sign of a near-zero pre-activation reaches: dX at the C positions before it, dw of its channel
    skip_dx = np.zeros_like(near)
    for k in range(min(C, U1)):
        skip_dx[:, :U1 - k] |= near[:, k:]
    skip_dw = np.broadcast_to(near.any(axis=(0, 1))[:, None, None], m["dw"].shape)
    Ye, dXe, dwe = SR.bwd_conv(m["X"], m["w"], m["dY"], dtype=torch.float32)
    Y, dX, dw = _device_pass(ops, m)
    for what, got, exist, K, skip in (("Y", Y, Ye, C + 1, None), ("dX", dX, dXe, C + 1, skip_dx),
                                      ("dw", dw, dwe, B * U1 + C, skip_dw)):
        want = m[what]
        keep = np.ones(want.shape, bool) if skip is None else ~skip
        assert keep.any()
        E = float(np.abs(exist.astype(np.float64) - want)[keep].max())
        floor = K * EPS * max(float(np.abs(want).max()), 1e-30)
        err = float(np.abs(got.astype(np.float64) - want)[keep].max())
        print("ctx", shape, what, "E %.3g floor %.3g err %.3g" % (E, floor, err))
        assert err <= 2 * max(E, floor), (shape, what, err, E, floor)


@pytest.mark.parametrize("shape", [(3, 5, 260, 8), (4, 65, 512, 2)])
def test_two_backward_runs_are_bit_equal(ops, shape):
    m = _mirror(shape, "random")
    a, b = _device_pass(ops, m), _device_pass(ops, m)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("pad", [3, 4])
@pytest.mark.parametrize("shape", [(2, 1, 5, 3), (3, 7, 4, 2), (2, 9, 67, 4), (3, 5, 260, 8)])
def test_row_strided_views_give_the_contiguous_result(ops, shape, pad):
    """ld = D + 3 (never the 16-byte path) and ld = D + 4 (the 16-byte path where D % 4 == 0); the columns beyond D are
    poisoned and stay as they are"""
    B, U1, D, C = shape
    m = _mirror(shape, "random")
    w = torch.tensor(m["w"], device=DEV)
    want = ops.rnnt_ctx_fwd(torch.tensor(m["X"], device=DEV), w)
    xb = torch.full((B, U1, D + pad), float("nan"), device=DEV)
    xb[:, :, :D] = torch.tensor(m["X"], device=DEV)
    yb = torch.full((B, U1, D + pad), -7.0, device=DEV)
    out = ops.rnnt_ctx_fwd(xb[:, :, :D], w, out=yb[:, :, :D])
    ops.check_errors()
    assert out.data_ptr() == yb.data_ptr() and torch.equal(yb[:, :, :D], want)
    assert bool((yb[:, :, D:] == -7.0).all())


def _step_inputs(C, Lc, D, seed, dtype):
    tokens, n_tok, emb, w = SR.step_case(C, Lc, V=9, D=D, seed=seed)
    return (tokens, n_tok, emb, w, torch.tensor(tokens, dtype=dtype, device=DEV), torch.tensor(n_tok, device=DEV),
            torch.tensor(emb, device=DEV), torch.tensor(w, device=DEV))


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("C,Lc,D", [(1, 1, 12), (2, 6, 12), (3, 2, 67), (8, 5, 260), (8, 12, 512), (2, 6, 1)])
def test_step_equals_the_forward_row_bit_for_bit(ops, dtype, C, Lc, D):
    tokens, n_tok, emb, w, tok_d, n_d, emb_d, w_d = _step_inputs(C, Lc, D, C + Lc, dtype)
    R = tokens.shape[0]
    # the output rows sit inside a poisoned buffer: a guard row before and after, guard columns beside
    buf = torch.full((R + 2, D + 4), -7.0, device=DEV)
    out = buf[1:R + 1, :D]
    got = ops.rnnt_ctx_step(tok_d, n_d, emb_d, w_d, out=out)
    ops.check_errors()
    assert got.data_ptr() == out.data_ptr()
    assert bool((buf[0] == -7.0).all()) and bool((buf[R + 1] == -7.0).all()) and bool((buf[:, D:] == -7.0).all())
    # the forward on <sos> + the row's labels, teacher-forced
    seq = torch.cat([torch.zeros((R, 1), dtype=torch.int64, device=DEV), tok_d.long()], dim=1)        # [R, Lc + 1]
    Y = ops.RNNTContextFn.apply(emb_d[seq], w_d)
    want = Y[torch.arange(R, device=DEV), n_d.long()]
    assert torch.equal(out, want), float((out - want).abs().max())
    # and it is the mirror's step (the forward itself is compared with the mirror above)
    ref = np.stack([SR.step_loops(tokens[r], n_tok[r], emb, w) for r in range(R)])
    assert np.abs(out.cpu().numpy() - ref).max() <= 2 * (C + 1) * EPS * max(np.abs(ref).max(), 1e-30)
    # the allocated form, and [B, W, Lc] tokens of a beam buffer taken as rows
    assert torch.equal(ops.rnnt_ctx_step(tok_d, n_d, emb_d, w_d), want)
    assert torch.equal(ops.rnnt_ctx_step(tok_d.view(2, R // 2, Lc), n_d.view(2, R // 2), emb_d, w_d), want)


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("C,Lc,D", [(2, 6, 12), (8, 5, 260), (3, 4, 67)])
def test_step_bad_labels_poison_their_row_alone(ops, dtype, C, Lc, D):
    tokens, n_tok, emb, w, tok_d, n_d, emb_d, w_d = _step_inputs(C, Lc, D, 7, dtype)
    R, V = tokens.shape[0], emb.shape[0]
    clean = ops.rnnt_ctx_step(tok_d, n_d, emb_d, w_d)
    bad = tok_d.clone()
    full = [r for r in range(R) if int(n_tok[r]) == Lc]
    assert len(full) >= 2
    bad[full[0], Lc - 1] = V                           # the current label of a row with Lc labels: read
    bad[full[1], Lc - 1] = -1
    huge = -2 ** 31 if dtype == torch.int32 else 2 ** 40
    unread = [r for r in range(R) if int(n_tok[r]) < Lc]
    for r in unread:
        bad[r, int(n_tok[r]):] = huge                  # behind position n: never read, so no NaN
    got = ops.rnnt_ctx_step(bad, n_d, emb_d, w_d)
    ops.check_errors()
    for r in range(R):
        if r in full[:2]:
            assert bool(torch.isnan(got[r]).all()), r
        else:
            assert torch.equal(got[r], clean[r]), r
    # a label far outside the matrix among those that ARE read: NaN, and the launch stays clean
    bad2 = tok_d.clone()
    bad2[full[0], max(Lc - C, 0)] = 2 ** 31 - 1 if dtype == torch.int32 else 2 ** 62
    got = ops.rnnt_ctx_step(bad2, n_d, emb_d, w_d)
    ops.check_errors()
    assert bool(torch.isnan(got[full[0]]).all()) and torch.equal(got[full[1]], clean[full[1]])
    # n_tok outside [0, Lc] is clamped
    wild = n_d.clone()
    wild[full[0]], wild[0] = Lc + 5, -3
    assert torch.equal(ops.rnnt_ctx_step(tok_d, wild, emb_d, w_d), clean)
