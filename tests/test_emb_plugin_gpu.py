"""GPU: the word-embedding plug-in's kernels (csrc/emb_fuse.hip) against the float64 restatement of
tests/emb_plugin_reference.py, the module against the recorded reference (tests/golden/emb_plugin.npz), the optimiser
step over both parameter groups and beam search with fusion against tests/golden/emb_fuse_decode.npz.

Bounds: the project's parity metric (helpers.rel_err) below 1e-3 on outputs and 2e-3 on gradients, as
tests/test_model_gpu.py uses."""
import importlib

import numpy as np
import pytest
import torch

import emb_plugin_reference as R
from conftest import PKG_NAME
from emb_plugin_helpers import SETTINGS, build, recorded_state, tokenizer, write_embedding, _mod
from helpers import CASES, load_golden, golden_state_dict, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
OUT_TOL, GRAD_TOL = 1e-3, 2e-3
F64 = torch.float64


@pytest.fixture(scope="module")
def E(ops):
    return _mod("emb_ops")


def _params(kind, V, g):
    """(temp, lam, lam_is_logit, temp is a parameter, lam is a parameter)"""
    if kind == "buffer":            # fuse = 0.3, temperature = 2
        return torch.tensor([2.0]), torch.tensor([0.3]), False, False, False
    if kind == "scalar":            # fuse = -1, temperature = -1
        return torch.tensor([1.7]), torch.tensor([-0.4]), True, True, True
    temp = 1.0 + 1.5 * torch.randn(V, generator=g)       # fuse = -2, temperature = -2
    temp[::3] = -temp[::3].abs() - 0.1                    # relu's flat side: gradient exactly 0 there
    return temp, 0.8 * torch.randn(V, generator=g), True, True, True


def _fuse_case(E, N, V, ld, kind, seed=0, scale=3.0):
    g = torch.Generator().manual_seed(seed + 1000 * V + N)
    d = scale * torch.randn(N, V, generator=g)
    e = torch.randn(N, V, generator=g)
    gy = torch.randn(N, V, generator=g)
    temp, lam, logit, t_par, l_par = _params(kind, V, g)
    # reference: float64 restatement, gradients by autograd
    d64, e64 = d.to(F64).requires_grad_(True), e.to(F64).requires_grad_(True)
    t64, l64 = temp.to(F64).requires_grad_(True), lam.to(F64).requires_grad_(True)
    y64 = R.fuse(d64, e64, t64, l64, logit)
    (y64 * gy.to(F64)).sum().backward()
    # device: dec_logit as a view with leading dimension ld
    buf = torch.full((N, ld), float("nan"), device=DEV)
    buf[:, :V] = d.to(DEV)
    dd = buf[:, :V].requires_grad_(True)
    ed = e.to(DEV).requires_grad_(True)
    td, ldv = temp.to(DEV).requires_grad_(t_par), lam.to(DEV).requires_grad_(l_par)
    runs = []
    for _ in range(2):
        for t in (dd, ed, td, ldv):
            t.grad = None
        y = E.fuse(dd, ed, td, ldv, logit, 1e-8)
        y.backward(gy.to(DEV))
        runs.append([y.detach().clone()] + [t.grad.clone() for t in (dd, ed, td, ldv) if t.grad is not None])
    for a, b in zip(*runs):             # no atomics anywhere: the two runs agree bit for bit
        assert torch.equal(a, b)
    assert torch.isfinite(runs[0][0]).all()
    assert rel_err(runs[0][0].cpu(), y64.detach()) < OUT_TOL
    assert rel_err(dd.grad.cpu(), d64.grad) < GRAD_TOL
    assert rel_err(ed.grad.cpu(), e64.grad) < GRAD_TOL
    if t_par:
        assert td.grad.shape == temp.shape and rel_err(td.grad.cpu(), t64.grad) < GRAD_TOL
        assert (td.grad.cpu()[temp <= 0] == 0).all()
    else:
        assert td.grad is None
    if l_par:
        assert ldv.grad.shape == lam.shape and rel_err(ldv.grad.cpu(), l64.grad) < GRAD_TOL
    else:
        assert ldv.grad is None


@pytest.mark.parametrize("kind", ["buffer", "scalar", "vocab"])
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("N", [1, 5, 130])
@pytest.mark.parametrize("V", [1, 7, 65, 257, 1031])
def test_fused_distribution_forward_backward(ops, E, V, N, pad, kind):
    _fuse_case(E, N, V, V + pad, kind)
    ops.check_errors()


@pytest.mark.parametrize("kind", ["buffer", "scalar", "vocab"])
def test_fused_distribution_at_the_shipped_vocabulary(ops, E, kind):
    _fuse_case(E, 3, 16000, 16000, kind)      # V % 4 == 0: the 16-byte path; 63 elements per thread
    ops.check_errors()


def test_fused_distribution_vector_path_with_padded_rows(ops, E):
    _fuse_case(E, 5, 64, 68, "vocab")         # V % 4 == 0 and ld % 4 == 0 with ld != V
    _fuse_case(E, 5, 64, 66, "vocab")         # ld % 4 != 0: rows lose their 16-byte alignment -> scalar path
    ops.check_errors()


def test_fused_distribution_stress_row(ops, E):
    """logits of +-80, a up to +-200: both softmaxes subtract their row maximum, nothing overflows; where both
    probabilities underflow to 0 the output is log(eps) exactly"""
    V = 40
    d = torch.zeros(2, V)
    d[0, ::2], d[0, 1::2] = 80.0, -80.0
    d[1] = torch.linspace(-80, 80, V)
    e = torch.zeros(2, V)
    e[0, :20], e[0, 20:] = 50.0, -50.0           # temp = 4: a = +-200
    e[1] = torch.linspace(50, -50, V)
    e[0, 1] = -50.0                               # d = -80 under a maximum of 80, a = -200 under 200: both underflow
    temp, lam, eps = torch.tensor([4.0]), torch.tensor([0.3]), 1e-8
    dd, ed = d.to(DEV).requires_grad_(True), e.to(DEV).requires_grad_(True)
    y = E.fuse(dd, ed, temp.to(DEV), lam.to(DEV), False, eps)
    y.backward(torch.ones_like(y))
    y64 = R.fuse(d.to(F64), e.to(F64), temp.to(F64), lam.to(F64), False, eps)
    assert torch.isfinite(y).all() and torch.isfinite(dd.grad).all() and torch.isfinite(ed.grad).all()
    assert rel_err(y.detach().cpu(), y64) < OUT_TOL
    log_eps = float(np.log(np.float64(np.float32(eps))).astype(np.float32))
    print("y at the underflow entry", repr(y[0, 1].item()), "log(eps) in f32", repr(log_eps))
    assert y[0, 1].item() == log_eps
    ops.check_errors()


@pytest.mark.parametrize("trainable", [False, True])
@pytest.mark.parametrize("Edim", [1, 10, 300])
def test_cosine_embedding_loss(ops, E, Edim, trainable):
    g = torch.Generator().manual_seed(Edim)
    B, L, V = 4, 6, 9
    table = torch.randn(V, Edim, generator=g)
    table[7] = 0                                         # a zero target row: its loss is exactly 1
    label = torch.tensor([[3, 5, 3, 3, 8, 1], [7, 1, 0, 0, 0, 0], [2, 3, 1, 0, 0, 0], [4, 4, 4, 4, 1, 0]])
    x = torch.randn(B * L, Edim, generator=g)
    x64, t64 = x.to(F64).requires_grad_(True), table.to(F64).requires_grad_(True)
    ref = R.cos_emb_loss(x64, t64, label)
    (1.7 * ref).backward()
    xd = x.to(DEV).requires_grad_(True)
    td = table.to(DEV).requires_grad_(trainable)
    runs = []
    for _ in range(2):
        xd.grad, td.grad = None, None
        loss = E.cos_emb_loss(xd, td, label.to(DEV))
        (1.7 * loss).backward()
        runs.append((loss.detach().clone(), xd.grad.clone(), td.grad.clone() if trainable else None))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    if trainable:       # the table's rows add their repeated labels (3 three times, 4 four times) in row order
        assert torch.equal(runs[0][2], runs[1][2])
    assert abs(loss.item() - ref.item()) < OUT_TOL * abs(ref.item())
    assert rel_err(xd.grad.cpu(), x64.grad) < GRAD_TOL
    pad = (label.reshape(-1) == 0)
    assert (xd.grad.cpu()[pad] == 0).all()               # all-pad tails contribute nothing
    if trainable:
        assert rel_err(td.grad.cpu(), t64.grad) < GRAD_TOL   # repeated labels (3, 4) add up in the table's rows
        assert (td.grad.cpu()[0] == 0).all()
    else:
        assert td.grad is None
    # the row against the zero target alone: loss exactly 1
    one = E.cos_emb_loss(x[:1].to(DEV), table.to(DEV), torch.tensor([[7]], device=DEV))
    assert one.item() == 1.0
    # an utterance without any label: 0/0, as in the reference
    nan = E.cos_emb_loss(x[:4].to(DEV), table.to(DEV), torch.tensor([[3, 1], [0, 0]], device=DEV))
    assert np.isnan(nan.item())
    ops.check_errors()


@pytest.mark.parametrize("V,R_", [(1, 3), (23, 15), (1031, 130)])
def test_nll_loss(ops, V, R_):
    g = torch.Generator().manual_seed(V)
    logp = torch.randn(R_, V, generator=g).log_softmax(-1)
    tgt = torch.randint(0, V, (R_,), generator=g)
    tgt[::4] = 0
    if V == 1:
        tgt[:] = 0
    l64 = logp.to(F64).requires_grad_(True)
    ref = torch.nn.NLLLoss(ignore_index=0)(l64, tgt)
    ld = logp.to(DEV).requires_grad_(True)
    loss = ops.NLLLoss(ignore_index=0)(ld, tgt.to(DEV))
    if V == 1:                                   # every row ignored: 0/0, same as torch
        assert np.isnan(ref.item()) and np.isnan(loss.item())
        return
    (2.5 * ref).backward()
    (2.5 * loss).backward()
    first = ld.grad.clone()
    ld.grad = None
    (2.5 * ops.NLLLoss(ignore_index=0)(ld, tgt.to(DEV))).backward()
    assert torch.equal(first, ld.grad)
    assert abs(loss.item() - ref.item()) < OUT_TOL * abs(ref.item())
    assert abs(loss.item() - R.nll(logp.to(F64), tgt).item()) < OUT_TOL * abs(ref.item())
    assert rel_err(ld.grad.cpu(), l64.grad) < GRAD_TOL
    # ignore_index other than 0, with a row that points at it
    ref2 = torch.nn.NLLLoss(ignore_index=2)(logp.to(F64), tgt)
    got2 = ops.NLLLoss(ignore_index=2)(logp.to(DEV), tgt.to(DEV))
    assert abs(got2.item() - ref2.item()) < OUT_TOL * abs(ref2.item())
    ops.check_errors()


@pytest.mark.parametrize("D_", [1, 10, 300])
def test_l2_normalisation(ops, E, D_):
    g = torch.Generator().manual_seed(D_)
    x = torch.randn(7, D_, generator=g)
    x[3] = 0                                             # a zero row: y = 0, dx = dy / 1e-12
    gy = torch.randn(7, D_, generator=g)
    x64 = x.to(F64).requires_grad_(True)
    y64 = R.normalize(x64)
    (y64 * gy.to(F64)).sum().backward()
    assert rel_err(y64.detach(), torch.nn.functional.normalize(x.to(F64), dim=-1)) < 1e-12
    xd = x.to(DEV).requires_grad_(True)
    y = E.l2_normalize(xd)
    y.backward(gy.to(DEV))
    first = xd.grad.clone()
    xd.grad = None
    E.l2_normalize(xd).backward(gy.to(DEV))
    assert torch.equal(first, xd.grad)
    assert (y[3] == 0).all()
    assert rel_err(y.detach().cpu(), y64.detach()) < OUT_TOL
    live = [0, 1, 2, 4, 5, 6]
    assert rel_err(xd.grad.cpu()[live], x64.grad[live]) < GRAD_TOL
    assert rel_err(xd.grad.cpu()[3], x64.grad[3]) < GRAD_TOL
    assert torch.equal(E.l2_normalize_infer(x.to(DEV)), y.detach())
    ops.check_errors()


@pytest.mark.parametrize("tag", list(SETTINGS))
def test_module_matches_the_recorded_reference(ops, tag, tmp_path):
    g = load_golden("emb_plugin")
    m = build(g, tag, tmp_path)
    m.load_state_dict(recorded_state(g, tag), strict=True)
    m = m.to(DEV).train()
    ds = torch.from_numpy(g["dec_state"]).to(DEV).requires_grad_(True)
    dl = torch.from_numpy(g["dec_logit"]).to(DEV).requires_grad_(True)
    label = torch.from_numpy(g["label"]).to(DEV)
    loss, fused = m(ds, dl, label=label)
    total = float(g["emb_weight"]) * loss
    if tag == "reg":
        assert fused is None
    else:
        assert rel_err(fused.detach().cpu(), g[tag + ".fused"]) < OUT_TOL
        total = total + (fused * torch.from_numpy(g["gy"]).to(DEV)).sum()
        with torch.no_grad():                            # the beam loops' entry: same numbers, no autograd node
            V = dl.shape[-1]
            inf = m.eval().infer(ds.detach().view(-1, ds.shape[-1]), dl.detach().view(-1, V))
            m.train()
        assert not inf.requires_grad and rel_err(inf.cpu(), g[tag + ".fused"].reshape(-1, V)) < OUT_TOL
    total.backward()
    assert abs(loss.item() - float(g[tag + ".loss"])) < OUT_TOL * abs(float(g[tag + ".loss"]))
    grads = dict({"dec_state": ds.grad, "dec_logit": dl.grad}, **{k: p.grad for k, p in m.named_parameters()})
    recorded = [k[len(tag) + 6:] for k in g if k.startswith(tag + ".grad.")]
    for k in recorded:
        assert grads[k] is not None, k
        assert rel_err(grads[k].cpu(), g["%s.grad.%s" % (tag, k)]) < GRAD_TOL, (tag, k)
    for k, v in grads.items():                           # and nothing the reference leaves without a gradient
        if k not in recorded:
            assert v is None, k
    ops.check_errors()


def test_fused_adadelta_steps_both_parameter_groups(ops, pkg, tmp_path):
    """model group clipped, plug-in group unclipped (the reference clips model.parameters() only), the frozen
    embedding table - no gradient - skipped; against torch.optim.Adadelta on the same gradients"""
    Optimizer = _mod("src.optim").Optimizer
    g = load_golden("emb_plugin")
    gen = torch.Generator().manual_seed(3)
    plug_dev = build(g, "learn", tmp_path).to(DEV)
    plug_ref = build(g, "learn", tmp_path)
    model_ref = [torch.randn(33, 5, generator=gen).requires_grad_(True), torch.randn(7, generator=gen).requires_grad_(True)]
    model_dev = [p.detach().clone().to(DEV).requires_grad_(True) for p in model_ref]
    hp = dict(optimizer='Adadelta', lr=1.0, eps=1e-8, lr_scheduler='fixed')
    o_dev = Optimizer([{'params': model_dev}, {'params': plug_dev.parameters()}], **hp)
    assert o_dev.fused and len(o_dev.opt.param_groups) == 2
    o_ref = torch.optim.Adadelta([{'params': model_ref}, {'params': plug_ref.parameters()}], lr=1.0, eps=1e-8,
                                 foreach=False)
    fo = importlib.import_module(pkg.__name__ + ".fused_optim")
    for step in range(4):
        o_dev.pre_step(step)
        o_ref.zero_grad()
        for pr, pd in list(zip(model_ref, model_dev)) + list(zip(plug_ref.parameters(), plug_dev.parameters())):
            if not pr.requires_grad:
                continue                                  # the frozen table
            gr = torch.randn(*pr.shape, generator=gen) * (4.0 if step % 2 else 0.3)
            pr.grad, pd.grad = gr.clone(), gr.clone().to(DEV)
        torch.nn.utils.clip_grad_norm_(model_ref, 5.0)
        o_ref.step()
        norm, coef = fo.grad_norm_and_coef(model_dev, 5.0)
        o_dev.step(norm, 5.0, coef=coef, clip_groups=1)
        for pr, pd in list(zip(model_ref, model_dev)) + list(zip(plug_ref.parameters(), plug_dev.parameters())):
            assert rel_err(pd.detach().cpu(), pr.detach()) < 2e-6
    assert not plug_dev.emb_table.weight.requires_grad and plug_dev.emb_table.weight not in o_dev.opt.state
    # a NaN norm skips the plug-in's group too, as the reference skips the whole step
    before = [p.detach().clone() for p in plug_dev.parameters()]
    model_dev[0].grad[0, 0] = float("nan")
    norm, coef = fo.grad_norm_and_coef(model_dev, 5.0)
    o_dev.step(norm, 5.0, coef=coef, clip_groups=1)
    assert all(torch.equal(a, b.detach()) for a, b in zip(before, plug_dev.parameters()))
    ops.check_errors()


def _asr(name):
    g = load_golden(name)
    cfg, D, V = CASES[name][0], CASES[name][1], CASES[name][2]
    model = _mod("src.asr").ASR(D, V, True, cfg["ctc_weight"], cfg["encoder"], cfg["attention"] or {},
                                cfg["decoder"] or {})
    model.load_state_dict(golden_state_dict(g), strict=True)
    feat = torch.from_numpy(g["feat"])[:1].to(DEV)
    flen = torch.from_numpy(g["feat_len"])[:1].to(DEV)
    return model.to(DEV).eval(), feat, flen


def _decode_plugin(g, model, tmp_path):
    src = write_embedding(g["emb_lines"], tmp_path / "emb_dec.txt")
    emb = _mod("src.plugin").EmbeddingRegularizer(tokenizer(g["chars"]), model.dec_dim, True, src, 'CosEmb', 1.0,
                                                  fuse=0.6, temperature=4)
    emb.load_state_dict({k[4:]: torch.from_numpy(v.copy()) for k, v in g.items() if k.startswith("emb.")},
                        strict=True)
    return emb.to(DEV).eval()


def _same_hyps(hyps, g, tag):
    """the comparison tests/test_decode_gpu.py applies to decode.npz"""
    assert len(hyps) == int(g[tag + ".n"])
    for i, h in enumerate(hyps):
        assert h.outIndex == g["%s.hyp%d" % (tag, i)].tolist(), (tag, i)
        ref = g["%s.score%d" % (tag, i)]
        assert np.allclose(np.asarray(h.output_scores, np.float32), ref, rtol=2e-3, atol=2e-3)


DECODE = [("b1_att", dict(beam_size=1, ctc_weight=0.0)), ("b1_ctc", dict(beam_size=1, ctc_weight=0.4)),
          ("b4_att", dict(beam_size=4, ctc_weight=0.0)), ("b4_ctc", dict(beam_size=4, ctc_weight=0.4))]


@pytest.mark.parametrize("host_beam", [False, True])
@pytest.mark.parametrize("tag,kw", DECODE)
def test_beam_search_with_fusion_matches_reference(ops, tmp_path, monkeypatch, tag, kw, host_beam):
    """forward (the device loop, and the host bookkeeping loop under ASRK_DECODE_HOST_BEAM=1) and forward_batch"""
    g = load_golden("emb_fuse_decode")
    model, feat, flen = _asr("las_hybrid_loc")
    dec = _mod("src.decode").BeamDecoder(model, _decode_plugin(g, model, tmp_path), min_len_ratio=0.01,
                                         max_len_ratio=float(g[tag + ".max_len_ratio"]), **kw)
    assert len(dec.create_msg()) == (3 if kw["ctc_weight"] > 0 else 2)
    if host_beam:
        monkeypatch.setenv("ASRK_DECODE_HOST_BEAM", "1")
        _same_hyps(dec(feat, flen), g, tag)
    else:
        _same_hyps(dec(feat, flen), g, tag)
        two = dec.forward_batch(torch.cat([feat, feat], 0), torch.cat([flen, flen], 0))
        assert len(two) == 2
        _same_hyps(two[0], g, tag)
        _same_hyps(two[1], g, tag)
    ops.check_errors()


def test_beam_search_without_plugin_is_unchanged(ops):
    g = load_golden("decode")
    fused = load_golden("emb_fuse_decode")
    model, feat, flen = _asr("las_hybrid_loc")
    dec = _mod("src.decode").BeamDecoder(model, None, min_len_ratio=0.01, max_len_ratio=0.5, beam_size=4,
                                         ctc_weight=0.0)
    hyps = dec(feat, flen)
    _same_hyps(hyps, g, "beam_att")
    # and the fixture does tell the two apart
    assert [h.outIndex for h in hyps] != [fused["b4_att.hyp%d" % i].tolist() for i in range(int(fused["b4_att.n"]))]
    ops.check_errors()
