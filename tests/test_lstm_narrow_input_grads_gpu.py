"""GPU: the weight gradients of a bidirectional LSTM layer whose BPTT kernel hands dG over in panels only.

 * narrow input (Din = 80, 36: a bottom layer, no input gradient): dW_ih = dG^T X has too few output tiles for the split
   GEMM's routing rule and multiplies the dG^T panel through the fixed-order split-K launch (ops.gemm_panels(splitk=0)),
   one launch over both directions' 8H rows;
 * every consumer of dG then takes a panel, so the BPTT launch carries ASRK_REC_BWD_NO_DG and does not store the f32 dG
   (ops._REC_SKIP_DG turns that off);
 * wide input with an input gradient (Din = 2048): dX multiplies the dG panel, the weight gradients dG^T - the flag is set
   together with both panels;
 * an input width no panel takes (Din = 38): the two directions' dW_hh share the one dG^T panel across two streams, dW_ih
   and with it the f32 dG stay.

T = 12, B = 32 (two 16-row batch groups), H = 1024: the smallest shapes at which the bf16x6 BPTT plan writes panels
(384 tokens = 12 k-tiles, three row tiles of X^T padding for Din < 128)."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
T, B, H = 12, 32, 1024


def make(Din, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, B, Din, generator=g)
    shapes = ((4 * H, Din), (4 * H, H), (4 * H,), (4 * H,))
    p0 = [torch.randn(*s, generator=g) / (s[-1] ** 0.5 if len(s) > 1 else 4.0) for s in shapes * 2]
    dy = torch.randn(T, B, 2 * H, generator=g)
    return x, p0, dy


def passes(ops, x0, p0, dy, xgrad, n):
    """n forward + backward passes from fresh leaves; the gradients (dx first when wanted) of the last one and the
    panel counters after every pass"""
    dyd = dy.to(DEV)
    stats = []
    for _ in range(n):
        x = x0.clone().to(DEV).requires_grad_(xgrad)
        ps = [q.clone().to(DEV).requires_grad_(True) for q in p0]
        ops.lstm_layer(x, tuple(ps[:4]), tuple(ps[4:])).backward(dyd)
        ops.join_deferred()
        stats.append(dict(ops._panel_state["stats"]))
    ops.check_errors()
    torch.cuda.synchronize()
    return ([x.grad.cpu()] if xgrad else []) + [q.grad.cpu() for q in ps], stats


def fresh_pools(ops):
    """_BlankPanel.take hands out a panel from the SECOND request of a shape on: forget what earlier tests asked for"""
    ops._panel_pool["seen"].clear()
    ops._panel_pool["free"].clear()
    ops._panel_pool["bytes"] = 0


def reference(ops, x0, p0, dy, xgrad):
    """per-GEMM splits and the f32 dW_ih: ASRK_SHARE_PANELS=0 (read by LSTMLayerFn.backward on every call)"""
    prev = os.environ.get("ASRK_SHARE_PANELS")
    os.environ["ASRK_SHARE_PANELS"] = "0"
    try:
        before = ops._panel_state["stats"].get("dgt", 0)
        ref, st = passes(ops, x0, p0, dy, xgrad, 2)
        assert st[-1].get("dgt", 0) == before                    # no dG^T panel: the old route
        return ref
    finally:
        if prev is None:
            del os.environ["ASRK_SHARE_PANELS"]
        else:
            os.environ["ASRK_SHARE_PANELS"] = prev


def close(got, ref):
    """the gradient tolerance of test_producer_written_panels_equal_split_passes"""
    assert len(got) == len(ref)
    for u, v in zip(got, ref):
        err, bound = float((u - v).abs().max()), 1e-5 * float(v.abs().max()) + 1e-12
        print("max |diff| %.3g  bound %.3g" % (err, bound))
        assert err <= bound


def pools_armed(ops):
    pooled = [e for lst in ops._xchg_pool["free"].values() for e in lst]
    assert pooled
    for buf, armed, _ in pooled:
        assert bool((buf[:armed] == 0xFF).all()), "pooled exchange buffer not armed over its recorded extent"


def counters(st, key):
    return [s.get(key, 0) for s in st]


@pytest.mark.parametrize("Din", [80, 36])
def test_narrow_input_dw_ih_through_splitk_panels(ops, Din):
    x0, p0, dy = make(Din, 100 + Din)
    ref = reference(ops, x0, p0, dy, False)
    ops.drop_exchange_pool()
    out = {}
    for skip in (True, False):
        fresh_pools(ops)
        prev = ops._REC_SKIP_DG
        ops._REC_SKIP_DG = skip
        try:
            s0 = dict(ops._panel_state["stats"])
            out[skip], st = passes(ops, x0, p0, dy, False, 3)
        finally:
            ops._REC_SKIP_DG = prev
        st = [s0] + st
        # pass 1: the shape is new, no panel, the old route; passes 2 and 3: dG^T from the kernel, dW_ih of both directions
        # in ONE split-K launch, and (switch on) no f32 dG
        assert counters(st, "dgt") == [s0.get("dgt", 0) + i for i in (0, 0, 1, 2)]
        assert counters(st, "dw_ih_splitk") == [s0.get("dw_ih_splitk", 0) + i for i in (0, 0, 1, 2)]
        assert counters(st, "no_dg") == [s0.get("no_dg", 0) + (i if skip else 0) for i in (0, 0, 1, 2)]
        close(out[skip], ref)
        pools_armed(ops)
        ops.check_errors()
    # the flag removes stores and nothing else: the same bits (bias sums: two batch groups, order-independent adds)
    close(out[True], out[False])
    for u, v in zip(out[True], out[False]):
        assert torch.equal(u, v)
    ops.drop_exchange_pool()


def test_odd_input_width_shares_the_panel_across_streams(ops):
    """Din = 38 (no panel takes an input width that is no multiple of 4), no input gradient: dW_hh of both directions
    multiplies row ranges of the ONE dG^T panel the kernel wrote, the reverse direction on the side stream, dW_ih reads
    the f32 dG (so the kernel keeps storing it) - and the pooled panel goes back only when the backward pass ends."""
    Din = 38
    x0, p0, dy = make(Din, 100 + Din)
    ref = reference(ops, x0, p0, dy, False)
    ops.drop_exchange_pool()
    fresh_pools(ops)
    s0 = dict(ops._panel_state["stats"])
    out, st = passes(ops, x0, p0, dy, False, 3)
    st = [s0] + st
    assert counters(st, "dgt") == [s0.get("dgt", 0) + i for i in (0, 0, 1, 2)]
    assert counters(st, "no_dg") == [s0.get("no_dg", 0)] * 4
    assert counters(st, "dw_ih_splitk") == [s0.get("dw_ih_splitk", 0)] * 4
    close(out, ref)
    pools_armed(ops)
    ops.check_errors()
    # the backward pass has ended and joined its side stream: nothing waits for release, the panel is back in the pool
    assert ops._defer["release"] == []
    assert [len(v) for k, v in ops._panel_pool["free"].items() if k[2:] == (8 * H, T * B)] == [1]
    ops.drop_exchange_pool()


def test_wide_layer_with_input_gradient_skips_dg_with_both_panels(ops):
    """Din = 2048 with dX wanted.  At 384 tokens the routing rule would keep dX off the split path (it wants
    2MN / (M + N) >= 1500), so the test runs with the split mode 'always' - the switch test_gemm_split_* use - to put the
    layer on the path the full-size wide layers take: dG panel for dX, dG^T panel for the weight gradients."""
    x0, p0, dy = make(2048, 7)
    mode = ops.get_gemm_split()
    ops.set_gemm_split(2)
    try:
        ref = reference(ops, x0, p0, dy, True)
        ops.drop_exchange_pool()
        out = {}
        for skip in (True, False):
            fresh_pools(ops)
            prev = ops._REC_SKIP_DG
            ops._REC_SKIP_DG = skip
            try:
                s0 = dict(ops._panel_state["stats"])
                out[skip], st = passes(ops, x0, p0, dy, True, 3)
            finally:
                ops._REC_SKIP_DG = prev
            st = [s0] + st
            assert counters(st, "dg") == [s0.get("dg", 0) + i for i in (0, 0, 1, 2)]
            assert counters(st, "dgt") == [s0.get("dgt", 0) + i for i in (0, 0, 1, 2)]
            assert counters(st, "no_dg") == [s0.get("no_dg", 0) + (i if skip else 0) for i in (0, 0, 1, 2)]
            assert counters(st, "dw_ih_splitk") == [s0.get("dw_ih_splitk", 0)] * 4      # wide: the plain panel launch
            close(out[skip], ref)
            pools_armed(ops)
            ops.check_errors()
        for u, v in zip(out[True], out[False]):
            assert torch.equal(u, v)
    finally:
        ops.set_gemm_split(mode)
        ops.drop_exchange_pool()
