"""GPU: every kernel variant of the fused decoder loop (csrc/speller.hip through speller_ops.SpellerLoopFn) and the
per-step attention kernels (csrc/attention.hip through decoder_ops) against the float64 reference of
tests/speller_reference.py, on the case table kept there: one small shape or more per forward / backward energy
kernel, per softmax/context kernel and per boundary between two of them (tests/test_speller_plan_cpu.py holds every
shape to its variant).  Outputs and the gradient of every input and weight; tolerances are those of
tests/test_cfg3_gpu.py: 1e-3 relative on outputs, 2e-3 on gradients, gen_energy.bias (exactly 0 by the shift
invariance of softmax) absolute on both sides."""
import importlib

import pytest
import torch

from conftest import PKG_NAME
from helpers import rel_err
import speller_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _grad_err(name, got, want):
    """-> (max abs error, scale of the float64 gradient, scale of the device gradient)"""
    got, want = got.detach().double().cpu(), want.detach()
    return float((got - want).abs().max()), float(want.abs().max()), float(got.abs().max())


def _grad_ok(name, e):
    """the rule of tests/test_cfg3_gpu.py: 2e-3 relative to the largest element of the float64 gradient; a tensor whose
    exact gradient is below 1e-6 everywhere (a single-frame utterance alone in the batch: its alignment is the constant
    1, nothing upstream of the softmax has a gradient) holds rounding noise and is compared absolutely; gen_energy.bias
    ('be'), exactly 0 by the shift invariance of softmax, stays below 1e-4 on both sides"""
    err, scale, got_scale = e
    if name == "be":
        return got_scale < 1e-4 and scale < 1e-4
    return err <= 1e-6 if scale < 1e-6 else err < 2e-3 * scale


def _run_loop_case(ops, case):
    sops = importlib.import_module(PKG_NAME + ".speller_ops")
    t, g1, g2 = R.make_loop_inputs(case, seed=11)
    lens = torch.tensor(case.lens)

    ref = {n: v.double().requires_grad_(True) for n, v in t.items()}
    st_r, att_r = R.loop_reference(*R.loop_args(case, ref))
    ((st_r * g1.double()).sum() + (att_r * g2.double()).sum()).backward()

    dev = {n: v.clone().to(DEV).requires_grad_(True) for n, v in t.items()}
    st, att = sops.SpellerLoopFn.apply(*R.loop_args(case, dev, gru_layout=sops.stack_gru_params))
    ((st * g1.to(DEV)).sum() + (att * g2.to(DEV)).sum()).backward()
    ops.join_deferred()
    ops.check_errors()

    st, att = st.detach().cpu(), att.detach().cpu()
    errs = {"states": rel_err(st, st_r.detach()), "att_seq": rel_err(att, att_r.detach())}
    gerrs = {}
    for n in t:
        assert dev[n].grad is not None and ref[n].grad is not None, n
        gerrs[n] = _grad_err(n, dev[n].grad, ref[n].grad)
    print(case.name, errs, gerrs)

    assert st.shape == (case.B, case.L, R.H) and att.shape == (case.B, case.N, case.L, case.Te)
    assert errs["states"] < 1e-3 and errs["att_seq"] < 1e-3, errs
    for b in range(case.B):
        n = int(lens[b])
        assert float(att[b, :, :, n:].abs().sum()) == 0.0           # exactly 0 beyond the utterance
        assert float((att[b, :, :, :n].double().sum(-1) - 1).abs().max()) < 1e-5
    bad = {n: e for n, e in gerrs.items() if not _grad_ok(n, e)}
    assert not bad, bad


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_loop_location_aware_variants_vs_float64(ops, case):
    """location-aware attention, one head: the five forward and five backward energy kernels, both softmax/context
    kernels, LSTM and GRU cells.  `k1`: before the a, k split of energy_bwd_kernel3 was made exact for K = 1, this case
    failed in Wp (loc_proj.weight) alone."""
    _run_loop_case(ops, case)


@pytest.mark.parametrize("case", R.DOT_CASES, ids=lambda c: c.name)
def test_loop_dot_product_variants_vs_float64(ops, case):
    """dot-product attention with one and several heads (merge_head), A up to DOT_NA's limit, a 2-layer decoder"""
    _run_loop_case(ops, case)


def _step_inputs(c, seed=13):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    BN = c.B * c.N
    t = dict(q=torch.tanh(rn(BN, c.A)), key=torch.tanh(rn(BN, c.Te, c.A)), value=rn(BN, c.Te, c.Dv))
    if c.mode == 'loc':
        t.update(prev=torch.softmax(rn(c.B, c.N, c.Te) * 2, dim=-1),
                 Wc=rn(c.K, c.N, c.taps) / (c.N * c.taps) ** 0.5, Wp=rn(c.A, c.K) / c.K ** 0.5,
                 we=rn(c.A) / c.A ** 0.5, be=rn(1) * 0.1)
    return t, rn(c.B, c.N, c.Te), rn(BN, c.Dv)


def _step_reference(c, t, g_attn, g_ctx):
    ref = {n: v.double().requires_grad_(True) for n, v in t.items()}
    a_r, c_r = R.attention_step_reference(ref['q'], ref.get('prev'), ref['key'], ref['value'], torch.tensor(c.lens),
                                          R.TEMPERATURE, c.N, ref.get('Wc'), ref.get('Wp'), ref.get('we'),
                                          ref.get('be'))
    ((a_r * g_attn.double()).sum() + (c_r * g_ctx.double()).sum()).backward()
    return ref, a_r.detach(), c_r.detach()


def _step_device(c, t):
    dops = importlib.import_module(PKG_NAME + ".decoder_ops")
    dev = {n: v.clone().to(DEV).requires_grad_(True) for n, v in t.items()}
    loc_w = tuple(dev[n] for n in ('Wc', 'Wp', 'we', 'be')) if c.mode == 'loc' else ()
    tape = dops.AttnTape(c.mode, dev['key'].detach(), dev['value'].detach(), torch.tensor(c.lens).to(DEV), c.N,
                         R.TEMPERATURE, tuple(w.detach() for w in loc_w) if loc_w else None)
    token = dops.AttnHubFn.apply(tape, dev['key'], dev['value'], *loc_w)
    attn, ctx = dops.AttnStepFn.apply(tape, token, dev['q'], dev.get('prev'))
    return dev, attn, ctx


@pytest.mark.parametrize("case", R.STEP_CASES, ids=lambda c: c.name)
def test_attention_step_kernels_vs_float64(ops, case):
    """AttnStepFn forward + every gradient: location-aware attention with one and TWO heads (the location convolution
    runs across the heads' alignments - this path only), K = 1 and K = 16, a window wider than the memory, and
    dot-product attention with one and three heads"""
    c = case
    t, g_attn, g_ctx = _step_inputs(c)
    ref, a_r, c_r = _step_reference(c, t, g_attn, g_ctx)
    dev, attn, ctx = _step_device(c, t)
    ((attn * g_attn.to(DEV)).sum() + (ctx * g_ctx.to(DEV)).sum()).backward()
    ops.check_errors()
    attn, ctx = attn.detach().cpu(), ctx.detach().cpu()
    errs = {"attn": rel_err(attn, a_r), "ctx": rel_err(ctx, c_r)}
    gerrs = {n: _grad_err(n, dev[n].grad, ref[n].grad) for n in t}
    print(c.name, errs, gerrs)
    assert attn.shape == (c.B, c.N, c.Te) and ctx.shape == (c.B * c.N, c.Dv)
    assert errs["attn"] < 1e-3 and errs["ctx"] < 1e-3, errs
    for b in range(c.B):
        assert float(attn[b, :, c.lens[b]:].abs().sum()) == 0.0
        assert float((attn[b, :, :c.lens[b]].double().sum(-1) - 1).abs().max()) < 1e-5
    bad = {n: e for n, e in gerrs.items() if not _grad_ok(n, e)}
    assert not bad, bad


def test_attention_step_k17_forward_matches_backward_refuses(ops):
    """more than 16 location kernels: the per-step forward has no such limit, the backward answers ASRK_ESHAPE
    (raised as AsrkError) instead of computing anything"""
    lib = importlib.import_module(PKG_NAME + "._lib")
    c = R.STEP_K17
    t, g_attn, g_ctx = _step_inputs(c)
    _, a_r, c_r = _step_reference(c, t, g_attn, g_ctx)
    dev, attn, ctx = _step_device(c, t)
    ops.check_errors()
    assert rel_err(attn.detach().cpu(), a_r) < 1e-3 and rel_err(ctx.detach().cpu(), c_r) < 1e-3
    with pytest.raises(lib.AsrkError):
        ((attn * g_attn.to(DEV)).sum() + (ctx * g_ctx.to(DEV)).sum()).backward()
