"""GPU: the RNN-transducer head in the model and in the solver.

 * ASR.transducer_logits + ops.RNNTLoss(consume_logits=True) on a tiny ASR (encoder dims [16, 16], V = 11, B = 3 ragged,
   LSTM and GRU prediction networks): the loss, the gradient with respect to the encoder output and every head
   parameter's gradient against the float64 mirror (tests/rnnt_reference.py: HeadRef).  Tolerance: E is the error of the
   existing differentiable path on the same case - the same head, its logits through ops.log_softmax and the alpha
   recursion in f32 torch ops under autograd on the device - and the fused path must be within 2 * max(E, floor), with
   floor = K 2^-23 max|reference| and K = (T' + U) + (U + 1) + 3 the roundings along one path: the lattice steps, the
   steps of the prediction network and the three linears.  Never derived from the fused path's results.
 * TransducerHead.greedy / ASR.transducer_greedy against the reference loop, token for token, a batch of 3 against one
   at a time; the reference-side conditions (margins, blanks and non-blanks, the max_symbols cap, rows finishing at
   different iterations) are asserted first (and on the CPU in tests/test_rnnt_cpu.py).
 * the training solver and `main.py --test` in a subprocess (tests/rnnt_worker.py)."""
import importlib
import json
import math
import os
import subprocess
import sys

import pytest
import torch

import rnnt_reference as RR
from conftest import PKG_NAME
from test_rnnt_gpu import _alpha_diag_lnp

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
D, V = 8, 11


def _mod(name):
    return importlib.import_module(PKG_NAME + "." + name)


def _tiny_asr(module, layer, seed):
    asr = _mod("src.asr")
    torch.manual_seed(seed)
    head = {'enable': True, 'weight': 0.3, 'joint_dim': 16,
            'pred': {'module': module, 'dim': 12, 'layer': layer, 'emb_dim': 20, 'dropout': 0}}
    enc = dict(prenet='', module='LSTM', bidirection=True, dim=[16, 16], dropout=[0, 0], layer_norm=[False, False],
               proj=[True, True], sample_rate=[2, 1], sample_style='drop')
    return asr.ASR(D, V, True, 1.0, enc, None, None, transducer=head).to(DEV)


def _batch(seed):
    g = torch.Generator().manual_seed(seed)
    feat = torch.randn((3, 20, D), generator=g)
    feat_len = torch.tensor([20, 12, 16])
    for b in range(3):
        feat[b, int(feat_len[b]):] = 0
    txt = torch.tensor([[3, 3, 7, 1], [5, 1, 0, 0], [9, 2, 1, 0]])
    return feat, feat_len, txt, torch.tensor([4, 2, 3])


@pytest.mark.parametrize("module,layer", [("LSTM", 1), ("GRU", 2)])
def test_logits_loss_and_gradients_against_the_float64_mirror(ops, module, layer):
    model = _tiny_asr(module, layer, 3).train()
    head = model.transducer
    feat, feat_len, txt, txt_len = _batch(4)
    with torch.no_grad():
        enc_out, enc_len = model.encoder(feat.to(DEV), feat_len.to(DEV))
    enc_len_h = [int(v) for v in enc_len.tolist()]
    assert enc_out.shape[:2] == (3, 10) and enc_len_h == [10, 6, 8]
    B, T, U = 3, enc_out.shape[1], txt.shape[1]
    txt_d, tl_d = txt.to(DEV), txt_len.to(DEV)
    names = [k for k, _ in head.named_parameters()]

    def device_pass(fused):
        model.zero_grad()
        enc = enc_out.detach().clone().requires_grad_(True)
        logits = model.transducer_logits(enc, enc_len, txt_d, tl_d)
        assert logits.shape == (B, T, U + 1, V)
        if fused:
            loss = ops.RNNTLoss(blank=0)(logits, txt_d, enc_len, tl_d, consume_logits=True)
        else:
            lp = ops.log_softmax(logits.view(-1, V)).view(B, T, U + 1, V)
            nll = []
            for b in range(B):
                Tb, Ub = enc_len_h[b], int(txt_len[b])
                lpb = lp[b, :Tb, :Ub + 1, 0]
                lpl = lp[b, :Tb, :Ub].gather(2, txt_d[b, :Ub].view(1, Ub, 1).expand(Tb, Ub, 1)).squeeze(2)
                nll.append(-_alpha_diag_lnp(lpb, lpl, Tb, Ub))
            loss = torch.stack(nll).mean()
        loss.backward()
        ops.check_errors()
        grads = {k: p.grad.detach().cpu().double().clone() for k, p in head.named_parameters()}
        return float(loss.detach()), enc.grad.cpu().double(), grads

    # the float64 mirror
    ref = RR.HeadRef.of(head, model.encoder.out_dim)
    enc64 = enc_out.detach().cpu().double().requires_grad_(True)
    z64 = ref.logits(enc64, txt)
    loss64 = torch.stack([-RR.alpha_lnp(RR.log_probs(z64[b, :enc_len_h[b], :int(txt_len[b]) + 1]),
                                        txt[b, :int(txt_len[b])]) for b in range(B)]).mean()
    loss64.backward()
    pm = ref.param_map()
    assert set(pm) == set(names)

    loss_e, denc_e, g_e = device_pass(fused=False)
    loss_n, denc_n, g_n = device_pass(fused=True)
    K = (T + U) + (U + 1) + 3

    def check(what, got, exist, want):
        E = float((exist - want).abs().max())
        floor = K * 2.0 ** -23 * max(float(want.abs().max()), 1e-30)
        err = float((got - want).abs().max())
        print(module, what, "E", E, "floor", floor, "err", err)
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


@pytest.mark.parametrize("module,layer,seed,bias", RR.GREEDY_CASES)
def test_greedy_against_the_reference_loop(ops, module, layer, seed, bias):
    tr = _mod("src.transducer")
    head, enc, lens = RR.greedy_case(tr.TransducerHead, module, layer, seed, bias)
    ref = RR.HeadRef.of(head, RR.GREEDY_ENC_DIM)
    want = RR.check_greedy_case(ref, enc, lens)                                         # the reference side first
    head = head.to(DEV).eval()
    ms, ml = RR.GREEDY_MAX_SYMBOLS, RR.GREEDY_MAX_LEN
    tokens, n_tok = head.greedy(enc.to(DEV), lens.to(DEV), ms, ml)
    ops.check_errors()
    assert tokens.shape == (3, ml) and tokens.dtype == torch.int64 and n_tok.shape == (3,)
    got = [tokens[b, :int(n_tok[b])].tolist() for b in range(3)]
    assert got == want
    assert all(bool((tokens[b, int(n_tok[b]):] == 0).all()) for b in range(3))
    tokens2, n_tok2 = head.greedy(enc.to(DEV), lens.to(DEV), ms, ml)                    # two runs: the same
    assert torch.equal(tokens, tokens2) and torch.equal(n_tok, n_tok2)
    for b in range(3):                                                                  # one at a time
        t1, n1 = head.greedy(enc[b:b + 1, :int(lens[b])].to(DEV).contiguous(), lens[b:b + 1].to(DEV), ms, ml)
        assert t1[0, :int(n1[0])].tolist() == want[b]
    # a cap of one symbol per frame and two tokens in all: never more than that
    t3, n3 = head.greedy(enc.to(DEV), lens.to(DEV), 1, 2)
    assert t3.shape == (3, 2) and all(int(n) <= 2 for n in n3.tolist())
    for b in range(3):
        ref_tokens, trace = ref.greedy(enc[b, :int(lens[b])].double(), 1, 2)
        assert min(tr[2] for tr in trace) >= RR.MIN_MARGIN
        assert t3[b, :int(n3[b])].tolist() == ref_tokens
    ops.check_errors()


def test_asr_transducer_greedy_is_the_head_on_the_encoder(ops):
    model = _tiny_asr("LSTM", 1, 5).eval()
    feat, feat_len, _, _ = _batch(6)
    tokens, n_tok, enc_len = model.transducer_greedy(feat.to(DEV), feat_len.to(DEV), max_symbols=2, max_len_ratio=0.35)
    with torch.no_grad():
        enc_out, enc_len2 = model.encoder(feat.to(DEV), feat_len.to(DEV))
    max_len = math.ceil(enc_out.shape[1] * 0.35)
    t2, n2 = model.transducer.greedy(enc_out, enc_len2, 2, max_len)
    assert tokens.shape == (3, max_len) and torch.equal(tokens, t2) and torch.equal(n_tok, n2)
    assert torch.equal(enc_len.cpu(), enc_len2.cpu()) and bool((n_tok <= max_len).all())
    ops.check_errors()


def test_solver_and_decoding(tmp_path):
    out = str(tmp_path / "rnnt.json")
    r = subprocess.run([sys.executable, os.path.join(HERE, "rnnt_worker.py"), out], capture_output=True, text=True,
                       env=dict(os.environ, ASRK_DETERMINISTIC="1"), timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.load(open(out))
    plain, off, on = res["plain"], res["off"], res["on"]
    # without the block and with enable: false: the same steps, bit for bit
    assert plain["loss_hex"] == off["loss_hex"] and plain["param_sha1"] == off["param_sha1"]
    assert plain["rnnt_logs"] == [] and off["rnnt_logs"] == [] and not plain["head_keys"] and not off["head_keys"]
    assert "best_rnnt.pth" not in plain["ckpts"] and "best_rnnt.pth" not in off["ckpts"]
    # with the block
    assert len(on["rnnt_logs"]) == len(on["loss_hex"]) >= 2
    assert all(math.isfinite(v) and v > 0 for v in on["rnnt_logs"])
    assert on["head_keys"] and on["head_moved"] and on["params_finite"]
    assert all(math.isfinite(v) for v in on["grad_norm"])
    assert on["loss_hex"][0] != plain["loss_hex"][0]
    assert any("ransducer" in m for m in on["msgs"])
    assert "best_rnnt.pth" in on["ckpts"] and on["dv_rnnt"] and all(0 <= v < 50 for v in on["dv_rnnt"])
    assert on["reload_missing"] == [] and on["reload_unexpected"] == []
    assert res["decode"]["files"] == ["dec_rnnt_dev_output.csv", "dec_rnnt_test_output.csv"]
    assert res["decode"]["lines"] == [4, 3] and res["decode"]["heads"] == ["idx\thyp\ttruth"] * 2
    assert "transducer" in res["decode"]["no_head_error"]
