"""CPU: the word-embedding plug-in's surface against the recorded reference (tests/golden/emb_plugin.npz, written by
tools/gen_emb_plugin_golden.py): the float64 restatement the GPU tests measure against, constructor / attributes /
state_dict layout / from-seed initialisation, load_embedding, the refused options and the host-side argument checks
of the new C entry points."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import emb_plugin_reference as R
from conftest import PKG_NAME, GOLDEN
from emb_plugin_helpers import SETTINGS, build, digest, recorded_state, tokenizer, write_embedding, _mod
from helpers import load_golden, rel_err


@pytest.fixture(scope="module")
def g():
    return load_golden("emb_plugin")


@pytest.mark.parametrize("tag", list(SETTINGS))
def test_restatement_equals_the_recorded_reference(g, tag):
    """f64 restatement against the reference's f32 run: 1e-6 relative covers the f32 rounding of the recording"""
    kw = SETTINGS[tag]
    p = {k: v.to(torch.float64).requires_grad_(True) for k, v in recorded_state(g, tag).items()}
    ds = torch.from_numpy(g["dec_state"]).to(torch.float64).requires_grad_(True)
    dl = torch.from_numpy(g["dec_logit"]).to(torch.float64).requires_grad_(True)
    label = torch.from_numpy(g["label"])
    loss, fused = R.plugin_forward(p, ds, dl, label, kw["fuse"] != 0, kw["fuse"] < 0,
                                   kw.get("fuse_normalize", False))
    total = float(g["emb_weight"]) * loss
    if fused is not None:
        total = total + (fused * torch.from_numpy(g["gy"]).to(torch.float64)).sum()
        print(tag, "fused", rel_err(fused.detach().numpy(), g[tag + ".fused"]))
        assert rel_err(fused.detach().numpy(), g[tag + ".fused"]) < 1e-6
    else:
        assert tag + ".fused" not in g
    total.backward()
    print(tag, "loss", loss.item(), float(g[tag + ".loss"]))
    assert abs(loss.item() - float(g[tag + ".loss"])) < 1e-6 * abs(float(g[tag + ".loss"]))
    grads = dict({"dec_state": ds.grad, "dec_logit": dl.grad}, **{k: v.grad for k, v in p.items()})
    recorded = [k[len(tag) + 6:] for k in g if k.startswith(tag + ".grad.")]
    assert "dec_state" in recorded and (fused is None or "dec_logit" in recorded)
    if kw["fuse"] < 0:
        assert "fuse_lambda" in recorded
    if kw["temperature"] < 0:
        assert "temp" in recorded
    for k in recorded:
        err = rel_err(grads[k].numpy(), g["%s.grad.%s" % (tag, k)])
        print(tag, "grad", k, err)
        assert err < 1e-6, (tag, k, err)
    if tag == "vocab":      # relu's flat side: the negative temperatures get exactly no gradient, here and there
        assert (g["vocab.param.temp"] < 0).sum() >= 2
        assert (g["vocab.grad.temp"][g["vocab.param.temp"] < 0] == 0).all()
        assert (grads["temp"].numpy()[g["vocab.param.temp"] < 0] == 0).all()


@pytest.mark.parametrize("tag", list(SETTINGS))
def test_constructor_attributes_state_dict_and_seeded_init(g, tag, tmp_path):
    kw = SETTINGS[tag]
    m = build(g, tag, tmp_path)
    assert list(m.state_dict().keys()) == [str(k) for k in g[tag + ".keys"]]
    assert [k for k, _ in m.named_parameters()] == [str(k) for k in g[tag + ".param_names"]]
    assert digest(m.state_dict()) == str(g[tag + ".digest"])          # same draws in the same order
    assert m.enable is True and m.weight == float(g["emb_weight"]) and m.distance == 'CosEmb' and m.dim == 10
    assert m.apply_fuse == (kw["fuse"] != 0) and m.apply_dropout is False
    if m.apply_fuse:
        assert m.eps == 1e-8
        assert m.fuse_type == {0.3: '0.3', -1: 'learnable', -2: 'vocab-wise learnable'}[kw["fuse"]]
        assert m.fuse_learnable == (kw["fuse"] < 0)
        assert m.temperature == {2: '2', -1: 'learnable', -2: 'elementwise'}[kw["temperature"]]
        assert isinstance(m.fuse_lambda, torch.nn.Parameter) == (kw["fuse"] < 0)
        assert isinstance(m.temp, torch.nn.Parameter) == (kw["temperature"] < 0)
        assert len(m.create_msg()) == 2 and 'Embedding-fusion decoder enabled' in m.create_msg()[1]
    else:
        assert len(m.create_msg()) == 1
    assert m.emb_table.weight.requires_grad == (not kw.get("freeze", True))
    m.load_state_dict(recorded_state(g, tag), strict=True)            # a reference checkpoint entry loads
    for meth in ("create_msg", "get_weight", "get_temp", "fuse_prob", "forward", "infer"):
        assert callable(getattr(m, meth))


def test_disabled_plugin_builds_nothing():
    m = _mod("src.plugin").EmbeddingRegularizer(None, 8, False, '', 'CosEmb', 1.0, 0, 1)
    assert m.enable is False and len(m.state_dict()) == 0


def test_load_embedding_both_token_modes(g, tmp_path):
    load_embedding = _mod("src.util").load_embedding
    got = load_embedding(tokenizer(g["chars"]), write_embedding(g["emb_lines"], tmp_path / "c.txt"))
    ref = g["load_embedding.character"]
    assert got.shape == ref.shape and got.dtype == ref.dtype and np.array_equal(got, ref)
    # a character vocabulary spells `<eos>` out: its first character is unknown, so `</s>` joins the averaged <unk>
    assert np.abs(ref[2]).max() > 0 and (ref[1] == 0).all()
    assert (ref[-2:] == 0).all() and (ref[0] == 0).all()                # rows no line names
    import os
    sub = _mod("src.text").load_text_encoder("subword", os.path.join(GOLDEN, "spm_tiny.model"))
    got = load_embedding(sub, write_embedding(g["emb_lines_subword"], tmp_path / "s.txt"))
    ref = g["load_embedding.subword"]
    assert got.shape == ref.shape and np.array_equal(got, ref)
    assert np.abs(ref[1]).max() > 0 and np.abs(ref[2]).max() > 0        # </s> -> the <eos> piece; averaged <unk>


def test_refused_options(g, tmp_path):
    P = _mod("src.plugin").EmbeddingRegularizer
    src = write_embedding(g["emb_lines"], tmp_path / "emb.txt")
    tok = tokenizer(g["chars"])
    with pytest.raises(NotImplementedError, match="MSE"):
        P(tok, 12, True, src, 'MSE', 1.0, 0, 1)
    with pytest.raises(NotImplementedError, match="BERT"):
        P(tok, 12, True, src, 'CosEmb', 1.0, 0, 1, bert='bert-base-uncased')
    with pytest.raises(NotImplementedError):
        P(tok, 12, True, src, 'L1', 1.0, 0, 1)


@pytest.fixture(scope="module")
def lib():
    importlib.import_module(PKG_NAME + ".build").build(verbose=False)
    return importlib.import_module(PKG_NAME + "._lib").load()


def test_new_entry_points_check_arguments_before_any_device_call(lib):
    L, z, f = lib, ctypes.c_void_p(0), ctypes.c_void_p(4096)
    EINVAL = -1
    fwd = lambda **o: L.asrk_emb_fuse_fwd_f32(*[o.get(k, d) for k, d in (
        ("d", f), ("ld", 8), ("e", f), ("temp", f), ("tl", 1), ("lam", f), ("ll", 8), ("logit", 1), ("eps", 1e-8),
        ("N", 2), ("V", 8), ("y", f), ("stats", f), ("s", z))])
    bwd = lambda **o: L.asrk_emb_fuse_bwd_f32(*[o.get(k, d) for k, d in (
        ("g", f), ("d", f), ("ld", 8), ("e", f), ("temp", f), ("tl", 1), ("lam", f), ("ll", 8), ("logit", 1),
        ("eps", 1e-8), ("stats", f), ("N", 2), ("V", 8), ("dd", f), ("de", f), ("dt", z), ("dl", z), ("ws", f),
        ("nws", 1 << 20), ("s", z))])
    for k in ("d", "e", "temp", "lam", "y", "stats"):
        assert fwd(**{k: z}) == EINVAL, k
    for k in ("g", "d", "e", "temp", "lam", "stats", "dd", "de"):
        assert bwd(**{k: z}) == EINVAL, k
    for call in (fwd, bwd):
        assert call(V=0) == EINVAL and call(V=-3) == EINVAL
        assert call(ld=7) == EINVAL                       # leading dimension below V
        assert call(tl=2) == EINVAL and call(tl=0) == EINVAL and call(ll=7) == EINVAL and call(ll=9) == EINVAL
        assert call(N=-1) == EINVAL
    # scratch is the caller's: too little is ASRK_EWORKSPACE, never a hidden allocation
    need = L.asrk_emb_fuse_bwd_ws_bytes(2, 8, 1, 8, 0, 1)
    assert need >= 2 * 2 * 4 and L.asrk_emb_fuse_bwd_ws_bytes(2, 8, 1, 8, 0, 1) > L.asrk_emb_fuse_bwd_ws_bytes(2, 8, 1, 8, 0, 0)
    assert bwd(dl=f, nws=need - 1) == -3 and bwd(ws=z) == -3
    assert L.asrk_emb_fuse_bwd_ws_bytes(2, 0, 1, 1, 0, 0) == 0
    # cosine loss, NLL, L2 normalisation
    assert L.asrk_cos_emb_loss_fwd_f32(z, f, 5, f, 2, 3, 4, f, f, f, z) == EINVAL
    assert L.asrk_cos_emb_loss_fwd_f32(f, f, 5, z, 2, 3, 4, f, f, f, z) == EINVAL
    assert L.asrk_cos_emb_loss_fwd_f32(f, f, 5, f, 2, 3, 0, f, f, f, z) == EINVAL
    assert L.asrk_cos_emb_loss_fwd_f32(f, f, 0, f, 2, 3, 4, f, f, f, z) == EINVAL
    assert L.asrk_cos_emb_loss_bwd_f32(f, f, 5, f, 2, 3, 4, f, f, z, z, z) == EINVAL      # dx is required, dy is not
    assert L.asrk_cos_emb_loss_bwd_f32(f, z, 5, f, 2, 3, 4, f, f, f, z, z) == EINVAL
    assert L.asrk_cos_emb_table_grad_f32(z, f, 6, 4, 5, f, z) == EINVAL
    assert L.asrk_cos_emb_table_grad_f32(f, z, 6, 4, 5, f, z) == EINVAL
    assert L.asrk_cos_emb_table_grad_f32(f, f, 6, 4, 5, z, z) == EINVAL
    assert L.asrk_cos_emb_table_grad_f32(f, f, 6, 0, 5, f, z) == EINVAL
    assert L.asrk_cos_emb_table_grad_f32(f, f, -1, 4, 5, f, z) == EINVAL
    assert L.asrk_nll_loss_fwd_f32(z, 2, 8, 8, f, 0, f, z) == EINVAL
    assert L.asrk_nll_loss_fwd_f32(f, 2, 0, 8, f, 0, f, z) == EINVAL
    assert L.asrk_nll_loss_fwd_f32(f, 2, 8, 7, f, 0, f, z) == EINVAL
    assert L.asrk_nll_loss_fwd_f32(f, 2, 8, 8, f, 0, z, z) == EINVAL
    assert L.asrk_nll_loss_bwd_f32(2, 8, 8, z, 0, f, f, z) == EINVAL
    assert L.asrk_nll_loss_bwd_f32(2, 0, 8, f, 0, f, f, z) == EINVAL
    assert L.asrk_l2norm_fwd_f32(z, f, f, 2, 8, 1e-12, z) == EINVAL
    assert L.asrk_l2norm_fwd_f32(f, f, f, 2, 0, 1e-12, z) == EINVAL
    assert L.asrk_l2norm_bwd_f32(f, z, f, f, 2, 8, 1e-12, z) == EINVAL
    assert L.asrk_l2norm_fwd_f32(f, f, f, 0, 8, 1e-12, z) == 0        # no rows: nothing to do


def test_cpu_tensors_are_refused(lib):
    AsrkError = importlib.import_module(PKG_NAME + "._lib").AsrkError
    E = _mod("emb_ops")
    ops = _mod("ops")
    x, t, lab = torch.zeros(6, 4), torch.zeros(5, 4), torch.ones(2, 3, dtype=torch.long)
    with pytest.raises(AsrkError):
        E.fuse(torch.zeros(2, 8), torch.zeros(2, 8), torch.ones(1), torch.ones(1), False, 1e-8)
    with pytest.raises(AsrkError):
        E.cos_emb_loss(x, t, lab)
    with pytest.raises(AsrkError):
        E.l2_normalize(x)
    with pytest.raises(AsrkError):
        E.relu(x)
    with pytest.raises(AsrkError):
        ops.NLLLoss(ignore_index=0)(torch.zeros(2, 8), torch.ones(2, dtype=torch.long))
