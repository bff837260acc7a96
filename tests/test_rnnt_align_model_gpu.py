"""GPU: the transducer forced alignment in the head and in the model.

 * TransducerHead.lattice_logp on tiny heads (V = 7, encoder width 8, dim 8, joint_dim 8; LSTM x1, GRU x1, stateless with
   context 2): a max_logits_bytes that admits one utterance per group equals the single-group result bit for bit, and
   both equal log_softmax of head.forward(...) within test_rnnt_gpu.py's floor_row = 2^-23 (2 S + ln V), S the largest
   |logit| of that forward;
 * ASR.transducer_align on a small model of the kind test_rnnt_model_gpu.py builds: the path is the numpy reference's
   (tests/rnnt_align_reference.py) on the lpb / lpl the model used; frames are non-decreasing, below encode_len, and
   exactly txt_len of them per utterance; a model without the head raises."""
import importlib
import math

import numpy as np
import pytest
import torch

import rnnt_align_reference as AR
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu
DEV = "cuda"
V, ENC, DIM, JOINT = 7, 8, 8, 8
PREDS = [{'module': 'LSTM', 'dim': DIM, 'layer': 1, 'emb_dim': DIM, 'dropout': 0},
         {'module': 'GRU', 'dim': DIM, 'layer': 1, 'emb_dim': DIM, 'dropout': 0},
         {'module': 'stateless', 'dim': DIM, 'context': 2, 'dropout': 0}]


def _mod(name):
    return importlib.import_module(PKG_NAME + "." + name)


def _head_case(pred, seed):
    tr = _mod("src.transducer")
    torch.manual_seed(seed)
    head = tr.TransducerHead(V, ENC, dict(pred), JOINT).to(DEV).eval()
    g = torch.Generator().manual_seed(seed + 1)
    enc = torch.randn((3, 9, ENC), generator=g).to(DEV)
    txt = torch.tensor([[3, 3, 6, 1, 2], [5, 1, 0, 0, 0], [0, 0, 0, 0, 0]]).to(DEV)
    return head, enc, torch.tensor([9, 5, 7]).to(DEV), txt, torch.tensor([5, 2, 0]).to(DEV)


@pytest.mark.parametrize("pred", PREDS, ids=[p['module'] for p in PREDS])
def test_lattice_logp_grouping_and_values(ops, pred):
    head, enc, el, txt, tl = _head_case(pred, 11)
    B, T, U1 = 3, enc.shape[1], txt.shape[1] + 1
    whole = head.lattice_logp(enc, el, txt, tl)
    one = T * U1 * V * 4                                   # the logits of one utterance
    for budget in (one, 2 * one, 1):                       # one per group, two and one, and less than one: still one
        lpb, lpl = head.lattice_logp(enc, el, txt, tl, max_logits_bytes=budget)
        assert torch.equal(lpb, whole[0]) and torch.equal(lpl, whole[1])
    assert whole[0].shape == (B, T, U1) and whole[1].shape == (B, T, U1)
    with torch.no_grad():
        z = head(enc, el, txt, tl).double()
    S = float(z.abs().max())
    floor_row = 2.0 ** -23 * (2 * S + math.log(V))
    lp = torch.log_softmax(z, dim=-1)
    for b in range(B):
        Tb, Ub = int(el[b]), int(tl[b])
        want_b = lp[b, :Tb, :Ub + 1, 0]
        assert float((whole[0][b, :Tb, :Ub + 1].double() - want_b).abs().max()) <= floor_row
        if Ub:
            want_l = lp[b, :Tb, :Ub].gather(2, txt[b, :Ub].view(1, Ub, 1).expand(Tb, Ub, 1)).squeeze(2)
            assert float((whole[1][b, :Tb, :Ub].double() - want_l).abs().max()) <= floor_row
        # outside the lattice the row pass writes zeros
        assert bool((whole[0][b, Tb:] == 0).all()) and bool((whole[0][b, :, Ub + 1:] == 0).all())
    # the head's own alignment is the reference's on these arrays
    al = head.align(enc, el, txt, tl, confidence=True)
    for b in range(B):
        ref = AR.align_f32(whole[0][b].cpu().numpy(), whole[1][b].cpu().numpy(), int(el[b]), int(tl[b]))
        assert np.array_equal(al.frames[b].cpu().numpy(), ref["frames"])
        assert al.score[b:b + 1].cpu().numpy().tobytes() == np.float32(ref["score"]).tobytes()
    assert al.tok_post.shape == al.frames.shape and bool((al.tok_post >= 0).all()) and bool((al.tok_post <= 1.0001).all())


def _tiny_asr(module, seed, head=True):
    asr = _mod("src.asr")
    torch.manual_seed(seed)
    pred = {'module': module, 'dim': 12, 'dropout': 0}
    if module != 'stateless':
        pred.update(layer=1, emb_dim=20)
    block = {'enable': True, 'weight': 0.3, 'joint_dim': 16, 'pred': pred} if head else None
    enc = dict(prenet='', module='LSTM', bidirection=True, dim=[16, 16], dropout=[0, 0], layer_norm=[False, False],
               proj=[True, True], sample_rate=[2, 1], sample_style='drop')
    return asr.ASR(8, 11, True, 1.0, enc, None, None, transducer=block).to(DEV).eval()


@pytest.mark.parametrize("module", ["LSTM", "stateless"])
def test_model_alignment_is_the_reference_path(ops, module):
    model = _tiny_asr(module, 3)
    g = torch.Generator().manual_seed(4)
    feat = torch.randn((3, 20, 8), generator=g)
    feat_len = torch.tensor([20, 12, 16])
    for b in range(3):
        feat[b, int(feat_len[b]):] = 0
    txt = torch.tensor([[3, 3, 7, 1], [5, 1, 0, 0], [9, 2, 1, 0]]).to(DEV)
    txt_len = torch.tensor([4, 2, 3]).to(DEV)
    feat, feat_len = feat.to(DEV), feat_len.to(DEV)
    for confidence in (False, True):
        frames, done, logp, post, score, enc_len = model.transducer_align(feat, feat_len, txt, txt_len,
                                                                          confidence=confidence)
        assert (post is None) == (not confidence)
        assert [int(v) for v in enc_len.tolist()] == [10, 6, 8]
        enc_out, _ = model.encoder(feat, feat_len)
        lpb, lpl = model.transducer.lattice_logp(enc_out, enc_len, txt, txt_len)    # no atomics: the same bits again
        for b in range(3):
            Tb, Ub = int(enc_len[b]), int(txt_len[b])
            ref = AR.align_f32(lpb[b].cpu().numpy(), lpl[b].cpu().numpy(), Tb, Ub)
            f = frames[b].cpu().numpy()
            assert np.array_equal(f, ref["frames"]) and np.array_equal(done[b].cpu().numpy(), ref["labels_done"])
            assert logp[b].cpu().numpy().tobytes() == ref["tok_logp"].tobytes()
            assert score[b:b + 1].cpu().numpy().tobytes() == np.float32(ref["score"]).tobytes()
            assert int((f >= 0).sum()) == Ub and (f[Ub:] == -1).all()
            assert (np.diff(f[:Ub]) >= 0).all() and (f[:Ub] < Tb).all() and (f[:Ub] >= 0).all()
    # a small budget changes nothing
    again = model.transducer_align(feat, feat_len, txt, txt_len, confidence=True, max_logits_bytes=1)
    assert torch.equal(again[0], frames) and torch.equal(again[3], post) and torch.equal(again[4], score)


def test_model_without_the_head_raises(ops):
    model = _tiny_asr("LSTM", 3, head=False)
    with pytest.raises(RuntimeError, match="transducer"):
        model.transducer_align(None, None, None, None)
