"""GPU: pruned transducer training in the model and in the solver.

 * ASR.transducer_loss_pruned on a tiny ASR (encoder dims [16, 16], V = 11, B = 3 ragged, transcripts of up to 6 tokens,
   LSTM and GRU prediction networks, range 2 and 3): the total loss, the gradient with respect to the encoder output
   and every head parameter's gradient, lin_am / lin_lm included, against the float64 mirror
   (tests/rnnt_prune_reference.py: PrunedHeadRef).  The band starts are no function to differentiate: the mirror's own
   (float64 occupations) are compared with the device's on every frame whose best and second-best window differ by
   1e-3 of the best, and the mirror then evaluates the pruned loss on the device's starts.
   Tolerance: E is the error of an f32 composition of existing ops on the same case - the same head, the simple joiner
   as ops.RNNTLoss on the dense sum, the band through torch.tanh on gathered rows, ops.log_softmax and the f32 autograd
   recursion inside the band - and the new path must be within 2 * max(E, floor), floor = K 2^-23 max|reference| with
   K = 2 ((T' + U) + 3) + (U + 1): two lattices with the linears in front of each, and the steps of the prediction
   network.  Never derived from the new path's results.
 * greedy decoding of a model built with the block equals that of the same weights without it.
 * the training solver in a subprocess (tests/rnnt_prune_worker.py): two steps with the block on; with the block off the
   losses and a SHA-1 over the parameters equal the run without the key."""
import importlib
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import rnnt_prune_reference as PR
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
D, V = 8, 11


def _mod(name):
    return importlib.import_module(PKG_NAME + "." + name)


def _tiny_asr(module, layer, seed, prune):
    asr = _mod("src.asr")
    torch.manual_seed(seed)
    head = {'enable': True, 'weight': 0.3, 'joint_dim': 16,
            'pred': {'module': module, 'dim': 12, 'layer': layer, 'emb_dim': 20, 'dropout': 0}}
    if prune is not None:
        head['prune'] = prune
    enc = dict(prenet='', module='LSTM', bidirection=True, dim=[16, 16], dropout=[0, 0], layer_norm=[False, False],
               proj=[True, True], sample_rate=[2, 1], sample_style='drop')
    return asr.ASR(D, V, True, 1.0, enc, None, None, transducer=head).to(DEV)


def _batch(seed):
    g = torch.Generator().manual_seed(seed)
    feat = torch.randn((3, 20, D), generator=g)
    feat_len = torch.tensor([20, 12, 16])
    for b in range(3):
        feat[b, int(feat_len[b]):] = 0
    txt = torch.tensor([[3, 3, 7, 1, 4, 2], [5, 1, 0, 0, 0, 0], [9, 2, 1, 8, 0, 0]])
    return feat, feat_len, txt, torch.tensor([6, 2, 4])


@pytest.mark.parametrize("S", [2, 3])
@pytest.mark.parametrize("module,layer", [("LSTM", 1), ("GRU", 2)])
def test_pruned_loss_and_gradients_against_the_float64_mirror(ops, module, layer, S):
    sw = 0.5
    model = _tiny_asr(module, layer, 3, {'enable': True, 'range': S, 'simple_weight': sw}).train()
    head = model.transducer
    feat, feat_len, txt, txt_len = _batch(4)
    with torch.no_grad():
        enc_out, enc_len = model.encoder(feat.to(DEV), feat_len.to(DEV))
        head.lin_am.weight.mul_(3.0)                    # a simple joiner with an opinion: the band moves
        head.lin_lm.weight.mul_(3.0)
    enc_len_h, txt_len_h = [int(v) for v in enc_len.tolist()], [int(v) for v in txt_len.tolist()]
    assert enc_out.shape[:2] == (3, 10) and enc_len_h == [10, 6, 8]
    B, T, U = 3, enc_out.shape[1], txt.shape[1]
    txt_d, tl_d = txt.to(DEV), txt_len.to(DEV)
    names = [k for k, _ in head.named_parameters()]
    assert "lin_am.weight" in names and "lin_lm.bias" in names

    # the device's band starts (what forward_pruned computes on the way)
    with torch.no_grad():
        pred = head._predict(txt_d)
        am = ops.linear(enc_out, head.lin_am.weight, head.lin_am.bias)
        lm = ops.linear(pred, head.lin_lm.weight, head.lin_lm.bias)
        _, occ = ops.RNNTSimpleLossFn.apply(am, lm, txt_d, enc_len, tl_d, 0)
        s_d = ops.rnnt_prune_ranges(occ, enc_len, tl_d, S)
    s_h = s_d.cpu().numpy()

    def collect(loss, enc):
        loss.backward()
        ops.check_errors()
        return (float(loss.detach()), enc.grad.cpu().double(),
                {k: p.grad.detach().cpu().double().clone() for k, p in head.named_parameters()})

    def new_pass():
        model.zero_grad()
        enc = enc_out.detach().clone().requires_grad_(True)
        total, pruned, simple = model.transducer_loss_pruned(enc, enc_len, txt_d, tl_d)
        assert abs(float(total) - (float(pruned) + sw * float(simple))) <= 1e-5 * abs(float(total))
        return collect(total, enc)

    def existing_pass():
        model.zero_grad()
        enc = enc_out.detach().clone().requires_grad_(True)
        pr = head._predict(txt_d)
        a = ops.linear(enc, head.lin_am.weight, head.lin_am.bias)
        l = ops.linear(pr, head.lin_lm.weight, head.lin_lm.bias)
        simple = ops.RNNTLoss(blank=0)(a[:, :, None, :] + l[:, None, :, :], txt_d, enc_len, tl_d)
        E = ops.linear(enc, head.lin_enc.weight, head.lin_enc.bias)
        P = ops.linear(pr, head.lin_pred.weight, head.lin_pred.bias)
        idx = (s_d.long().unsqueeze(2) + torch.arange(S, device=DEV)).clamp(max=U)
        H = torch.tanh(E.unsqueeze(2) + P[torch.arange(B, device=DEV).view(B, 1, 1), idx])
        z = ops.linear(H, head.lin_out.weight, head.lin_out.bias)
        lp = ops.log_softmax(z.view(-1, V)).view(B, T, S, V)
        nll = []
        for b in range(B):
            sb = [int(v) for v in s_h[b]]
            lpb, lpl = PR.band_terms(lp[b], txt[b], sb, enc_len_h[b], txt_len_h[b], S)
            nll.append(-PR.band_lnp(lpb, lpl, sb, enc_len_h[b], txt_len_h[b], S))
        return collect(torch.stack(nll).mean() + sw * simple, enc)

    # the float64 mirror
    ref = PR.PrunedHeadRef.of(head, model.encoder.out_dim)
    enc64 = enc_out.detach().cpu().double().requires_grad_(True)
    simple64, occ64 = ref.simple(enc64, txt, enc_len_h, txt_len_h)
    s64, margin = PR.ranges(occ64, enc_len_h, txt_len_h, S)
    decided = 0
    for b in range(B):
        PR.check_invariants(s_h[b], enc_len_h[b], txt_len_h[b], S)
        for t in range(enc_len_h[b]):
            if margin[b, t] >= PR.MIN_RANGE_MARGIN:
                decided += 1
                assert s_h[b, t] == s64[b, t], (b, t, s_h[b].tolist(), s64[b].tolist())
    print("MODEL", module, "S", S, "frames", sum(enc_len_h), "decided", decided, "starts", s_h.tolist())
    assert decided > 0
    loss64 = ref.pruned(enc64, txt, enc_len_h, txt_len_h, s_h, S).mean() + sw * simple64.mean()
    loss64.backward()
    pm = ref.param_map()
    assert set(pm) == set(names)

    loss_e, denc_e, g_e = existing_pass()
    loss_n, denc_n, g_n = new_pass()
    K = 2 * ((T + U) + 3) + (U + 1)

    def check(what, got, exist, want):
        E = float((exist - want).abs().max())
        floor = K * 2.0 ** -23 * max(float(want.abs().max()), 1e-30)
        err = float((got - want).abs().max())
        print("MODEL", module, "S", S, what, "E", E, "floor", floor, "err", err)
        assert err <= 2 * max(E, floor), what
    check("loss", torch.tensor(loss_n, dtype=torch.float64), torch.tensor(loss_e, dtype=torch.float64),
          loss64.detach())
    check("d enc", denc_n, denc_e, enc64.grad)
    pad = torch.ones((B, T), dtype=torch.bool)
    for b in range(B):
        pad[b, :enc_len_h[b]] = False
    assert bool((denc_n[pad] == 0).all()), "frames beyond encode_len get no gradient from the head"
    for k in names:
        assert float(pm[k].grad.abs().max()) > 0, k
        check(k, g_n[k], g_e[k], pm[k].grad)


def test_greedy_decoding_ignores_the_block(ops):
    """the same weights with and without the block decode the same tokens: lin_am and lin_lm are training's alone"""
    on = _tiny_asr("LSTM", 1, 5, {'enable': True, 'range': 3}).eval()
    off = _tiny_asr("LSTM", 1, 6, None).eval()
    sd = {k: v for k, v in on.state_dict().items() if ".lin_am." not in k and ".lin_lm." not in k}
    assert len(sd) == len(on.state_dict()) - 4
    off.load_state_dict(sd, strict=True)
    feat, feat_len, _, _ = _batch(6)
    t_on, n_on, _ = on.transducer_greedy(feat.to(DEV), feat_len.to(DEV), max_symbols=2, max_len_ratio=0.5)
    t_off, n_off, _ = off.transducer_greedy(feat.to(DEV), feat_len.to(DEV), max_symbols=2, max_len_ratio=0.5)
    ops.check_errors()
    assert torch.equal(t_on, t_off) and torch.equal(n_on, n_off)
    b_on = on.transducer_beam(feat.to(DEV), feat_len.to(DEV), 3, max_symbols=2, max_len_ratio=0.5)
    b_off = off.transducer_beam(feat.to(DEV), feat_len.to(DEV), 3, max_symbols=2, max_len_ratio=0.5)
    assert all(torch.equal(x, y) for x, y in zip(b_on[:3], b_off[:3]))


def test_solver_with_and_without_the_block(tmp_path):
    out = str(tmp_path / "prune.json")
    r = subprocess.run([sys.executable, os.path.join(HERE, "rnnt_prune_worker.py"), out], capture_output=True, text=True,
                       env=dict(os.environ, ASRK_DETERMINISTIC="1"), timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.load(open(out))
    parent, off, on = res["parent"], res["off"], res["on"]
    # enable: false is the run without the key, bit for bit
    assert parent["loss_hex"] == off["loss_hex"] and parent["param_sha1"] == off["param_sha1"]
    assert parent["head_keys"] == off["head_keys"] and parent["tr_rnnt"] == off["tr_rnnt"]
    assert parent["tr_rnnt_pruned"] == [] and off["tr_rnnt_pruned"] == [] and off["tr_rnnt_simple"] == []
    assert not any("runed" in m for m in parent["msgs"] + off["msgs"])
    # two steps with the block on
    assert len(on["loss_hex"]) >= 2
    assert len(on["tr_rnnt"]) == len(on["tr_rnnt_pruned"]) == len(on["tr_rnnt_simple"]) == len(on["loss_hex"])
    for tot, pr, si in zip(on["tr_rnnt"], on["tr_rnnt_pruned"], on["tr_rnnt_simple"]):
        assert all(math.isfinite(v) and v > 0 for v in (tot, pr, si))
        assert abs(tot - (pr + on["simple_weight"] * si)) <= 1e-5 * tot
    assert on["simple_weight"] == 0.25
    new = sorted(set(on["head_keys"]) - set(parent["head_keys"]))
    assert new == sorted("transducer." + k for k in ("lin_am.bias", "lin_am.weight", "lin_lm.bias", "lin_lm.weight"))
    assert on["head_moved"] == on["head_keys"], "every head parameter, lin_am / lin_lm included, takes a step"
    assert on["params_finite"] and all(math.isfinite(v) for v in on["grad_norm"])
    assert on["loss_hex"][0] != parent["loss_hex"][0]
    assert any("runed" in m for m in on["msgs"])
