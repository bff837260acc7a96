"""GPU: a padded batch of utterances of different lengths through the VGG / CNN prenets, the encoder behind them and the
batched decoders = every utterance run alone and unpadded (how the reference decodes: src/decode.py:88 on batch 1).

The padded batches carry RANDOM NON-ZERO values beyond every utterance's length: the per-utterance valid height of the
length-aware convolution entries (asrk_conv3x3_len_f32, asrk_conv3x3_first_len_f32, asrk_im2col_*_len_f32) has to do
the work, not the caller's padding."""
import importlib

import numpy as np
import pytest
import torch

from conftest import PKG_NAME
from helpers import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _mod(name):
    return importlib.import_module(PKG_NAME + "." + name)


def _padded(lens, D, seed):
    """[U, max(lens), D] random features; frames beyond an utterance's length are random too (scaled up, never zero)"""
    g = torch.Generator().manual_seed(seed)
    U, T = len(lens), max(lens)
    feat = torch.randn(U, T, D, generator=g)
    for u, l in enumerate(lens):
        feat[u, l:] = 3.0 * torch.randn(T - l, D, generator=g) + 1.0
    return feat


def _check_prenet(pre, feat, lens, exact):
    U = len(lens)
    with torch.no_grad():
        out, out_len = pre.forward_bm2tm(feat.to(DEV), torch.tensor(lens).to(DEV), packed=True)
        assert out.shape[0] == max(lens) // 4 and out.shape[1] == U
        assert out_len.tolist() == [l // 4 for l in lens]
        out = out.cpu()
        for u, l in enumerate(lens):
            n = l // 4
            if out.shape[0] > n:
                assert float(out[n:, u].abs().max()) == 0.0, u            # exactly zero beyond the utterance
            if l < 4:
                continue                                                  # a zero-frame utterance: nothing to compare
            one, one_len = pre.forward_bm2tm(feat[u:u + 1, :l].contiguous().to(DEV), torch.tensor([l]).to(DEV))
            one = one.cpu()
            assert one.shape[0] == n and int(one_len[0]) == n
            assert float(one.abs().max()) > 0.0
            if exact:
                assert torch.equal(out[:n, u], one[:, 0]), (u, rel_err(out[:n, u], one[:, 0]))
            else:
                assert rel_err(out[:n, u], one[:, 0]) < 2e-6, u


VGG_CASES = [(40, [37, 23, 30, 8, 3]), (39, [21, 40, 6, 17])]


@pytest.mark.parametrize("D,lens", VGG_CASES)
def test_vgg_prenet_packed_direct_kernels_bitwise(ops, monkeypatch, D, lens):
    """implicit-GEMM 3x3 kernels and the first-layer kernel with a per-image valid height: bit-identical to batch-1 runs
    (every output element is summed over (channel half, tap, chunk, MFMA step) in an order that depends on neither the
    tile position nor the batch; masked inputs are selected to 0).  F = 40: an utterance's last row falls inside a
    128-position tile and whole tiles lie beyond the short ones (early exit); L = 3: zero frames; L % 4 != 0: the crop."""
    monkeypatch.delenv("ASRK_CONV_DIRECT", raising=False)
    torch.manual_seed(2)
    pre = _mod("src.module").VGGExtractor(D).to(DEV).eval()
    _check_prenet(pre, _padded(lens, D, 5), lens, exact=True)
    ops.check_errors()


@pytest.mark.parametrize("D,lens", VGG_CASES)
def test_vgg_prenet_packed_im2col_route(ops, monkeypatch, D, lens):
    """ASRK_CONV_DIRECT=0: length-aware im2col gathers + GEMM; the GEMM's row count differs between the batch and the
    batch-1 run, so agreement is to summation order"""
    monkeypatch.setenv("ASRK_CONV_DIRECT", "0")
    torch.manual_seed(2)
    pre = _mod("src.module").VGGExtractor(D).to(DEV).eval()
    _check_prenet(pre, _padded(lens, D, 5), lens, exact=False)
    ops.check_errors()


def test_cnn_prenet_packed(ops):
    torch.manual_seed(3)
    pre = _mod("src.module").CNNExtractor(40, out_dim=16).to(DEV).eval()
    lens = [37, 22, 9, 5, 3]
    _check_prenet(pre, _padded(lens, 40, 6), lens, exact=False)
    ops.check_errors()


def test_conv_len_is_inference_only(ops):
    C = _mod("conv_ops")
    x = torch.randn(2, 8, 40, device=DEV, requires_grad=True)
    w, b = torch.randn(64, 1, 3, 3, device=DEV), torch.randn(64, device=DEV)
    g = C.Geom(2, 8, 40, 1, 3, 3, 1, 1, 1, 1, 8 * 40, 40, 1, 40)
    with pytest.raises(_mod("_lib").AsrkError):
        C.conv_len(x, w, b, g, torch.tensor([8, 4], device=DEV), relu=True)
    ops.check_errors()


@pytest.mark.parametrize("prenet", ["vgg", "cnn"])
@pytest.mark.parametrize("shape", ["drop", "proj"])
def test_packed_encoder_with_prenet_equals_one_utterance_at_a_time(ops, prenet, shape):
    """as test_packed_encoder_equals_one_utterance_at_a_time, behind a prenet"""
    if shape == "drop":
        cfg = dict(prenet=prenet, module='LSTM', bidirection=True, dim=[16, 16], dropout=[0, 0],
                   layer_norm=[False, False], proj=[False, False], sample_rate=[2, 1], sample_style='drop')
    else:
        cfg = dict(prenet=prenet, module='LSTM', bidirection=True, dim=[16, 16], dropout=[0, 0],
                   layer_norm=[False, False], proj=[True, True], sample_rate=[1, 1], sample_style='drop')
    D, lens = 40, [61, 45, 52, 19]
    torch.manual_seed(1)
    enc = _mod("src.asr").Encoder(D, **cfg).to(DEV).eval()
    assert enc.supports_packed()
    feat = _padded(lens, D, 7)
    with torch.no_grad():
        out, out_len = enc(feat.to(DEV), torch.tensor(lens).to(DEV), packed=True)
        for u, l in enumerate(lens):
            one, one_len = enc(feat[u:u + 1, :l].contiguous().to(DEV), torch.tensor([l]).to(DEV))
            lo, fr = int(one_len[0]), one.shape[1]
            assert int(out_len[u]) == lo and int(enc.packed_frames[u]) == fr and fr - lo in (0, 1)
            assert fr > 0 and float(one.abs().max()) > 0.0
            assert rel_err(out[u, :fr].cpu(), one[0].cpu()) < 2e-6, (prenet, shape, u)
            if shape == "drop" and fr < out.shape[1]:
                assert float(out[u, fr:].abs().max().cpu()) == 0.0
    ops.check_errors()


def _same_hyps(a, b, tol=2e-3):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.outIndex == y.outIndex, i
        assert np.allclose(np.asarray(x.output_scores, np.float32), np.asarray(y.output_scores, np.float32),
                           rtol=tol, atol=tol), i


def _mini_shipped(prenet, ctc_weight):
    """the shipped architecture in miniature: prenet, 2 x BLSTM-24 with projection, location-aware attention with one
    head, one-layer LSTM decoder"""
    enc = dict(prenet=prenet, module='LSTM', bidirection=True, dim=[24, 24], dropout=[0, 0],
               layer_norm=[False, False], proj=[True, True], sample_rate=[1, 1], sample_style='drop')
    att = dict(mode='loc', dim=20, num_head=1, v_proj=False, temperature=0.6, loc_kernel_size=5, loc_kernel_num=3)
    dec = dict(module='LSTM', dim=28, layer=1, dropout=0)
    torch.manual_seed(11)
    if ctc_weight == 1.0:
        model = _mod("src.asr").ASR(40, 31, True, 1.0, enc, {}, {})
    else:
        model = _mod("src.asr").ASR(40, 31, True, ctc_weight, enc, att, dec)
    return model.to(DEV).eval()


@pytest.mark.parametrize("prenet", ["vgg", "cnn"])
def test_forward_batch_behind_a_prenet_equals_forward(ops, monkeypatch, prenet):
    """BeamDecoder.forward_batch batches a prenet model (batchable() is True) and returns, per utterance, what forward()
    returns for it alone with the host record loop"""
    model = _mini_shipped(prenet, 0.4)
    lens = [64, 50, 38]
    feat = _padded(lens, 40, 12).to(DEV)
    flen = torch.tensor(lens).to(DEV)
    # max_len_ratio: the prenet leaves L // 4 frames (16, 12, 9), and a hypothesis with more labels than the CTC head
    # can emit scores logzero (-1e6 per term) on every path.  Among such dead hypotheses the f32 device bookkeeping and
    # the float64 host loop rank differently - at |score| = 4e6 an f32 ulp is 0.25-0.5, the size of a label's score
    # difference - with or without a prenet and with or without batching, so the length limit keeps the search where
    # the CTC is alive: at most 7, 5 and 4 labels.
    dec = _mod("src.decode").BeamDecoder(model, None, beam_size=4, min_len_ratio=0.01, max_len_ratio=0.1, ctc_weight=0.4)
    assert dec.batchable()
    got = dec.forward_batch(feat, flen)
    ops.check_errors()
    assert len(got) == len(lens)
    monkeypatch.setenv("ASRK_DECODE_HOST_BEAM", "1")
    want = [dec(feat[u:u + 1, :l].contiguous(), flen[u:u + 1]) for u, l in enumerate(lens)]
    for u in range(len(lens)):
        _same_hyps(got[u], want[u], tol=1e-4)
    assert any(len(h.outIndex) > 1 for w in want for h in w)            # real hypotheses, not empty strings
    ops.check_errors()


def test_ctc_beam_forward_batch_behind_vgg_equals_forward(ops):
    model = _mini_shipped("vgg", 1.0)
    V = 31
    lens = [64, 50, 38]
    feat = _padded(lens, 40, 13).to(DEV)
    flen = torch.tensor(lens).to(DEV)
    dec = _mod("src.ctc").CTCBeamDecoder(model, [1] + list(range(3, V)), beam_size=3, vocab_candidate=4)
    assert model.encoder.supports_packed()
    got = dec.forward_batch(feat, flen)
    ops.check_errors()
    assert len(got) == len(lens)
    for u, l in enumerate(lens):
        assert got[u] == dec(feat[u:u + 1, :l].contiguous(), flen[u:u + 1]), u
    assert any(len(y) > 1 for hyps in got for y in hyps)
    ops.check_errors()
