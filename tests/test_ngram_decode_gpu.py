"""GPU: both beam searches fused with a back-off n-gram LM (an `.arpa` lm_path -> src/ngram.py: NGramLM) against the
CPU oracles of the searches given the float64 n-gram reference (tests/ngram_reference.py) as their LM."""
import importlib

import numpy as np
import pytest
import torch

import ngram_cases as NC
import ngram_reference as NR
from conftest import PKG_NAME
from helpers import CASES, load_golden, golden_state_dict
from oracle import beam_oracle as BO
from oracle import ctc_beam_oracle as CBO

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _mod(name):
    return importlib.import_module(PKG_NAME + "." + name)


class _StubASR:
    enable_ctc = True

    def __init__(self, V):
        self.vocab_size = V


@pytest.fixture(scope="module")
def search_lm(tmp_path_factory):
    path = NC.search_lm_arpa(tmp_path_factory.mktemp("slm") / "lm.arpa")
    return path, NR.read_arpa(path, NC.SEARCH_V)


def _ctc_decoder(path, lm_w):
    V = NC.SEARCH_V
    dec = _mod("src.ctc").CTCBeamDecoder(_StubASR(V), NC.vocab_range(V), NC.SEARCH_BEAM, NC.SEARCH_CAND, lm_path=path,
                                         lm_config='', lm_weight=lm_w, device=DEV)
    assert isinstance(dec.lm, _mod("src.ngram").NGramLM) and dec.lm.order == NC.SEARCH_LM_ORDER
    assert any("3-gram" in line for line in dec.create_msg())
    return dec


def _oracle(m, x, lm_w):
    return [list(y) for y in CBO.prefix_beam_search(x, NC.vocab_range(NC.SEARCH_V), NC.SEARCH_BEAM, NC.SEARCH_CAND,
                                                    lm_step=NR.f64_lm_step(m), lm_w=lm_w)]


# ---- CTC prefix beam search ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,lm_w", NC.SEARCH_CASES)
def test_search_device_with_arpa_lm_equals_oracle_with_float64_lm(ops, search_lm, seed, lm_w):
    path, m = search_lm
    x = NC.search_posteriors(seed)
    dec = _ctc_decoder(path, lm_w)
    assert dec._device_search_ok(NC.SEARCH_V)
    got = dec.search_device(torch.from_numpy(x).to(DEV).contiguous())
    ops.check_errors()
    assert [list(y) for y in got] == _oracle(m, x, lm_w)


def test_lock_step_search_equals_single_utterance_search_in_one_lm_call_per_frame(ops, search_lm):
    """U = 3 utterances of 30, 19 and 11 frames, the third all blank"""
    path, m = search_lm
    lens = [30, 19, 11]
    xs = [NC.search_posteriors(0), NC.search_posteriors(3)[:19], NC.search_posteriors(4)[:11].copy()]
    xs[2][:, 0] += 40.0
    xs[2] = torch.log_softmax(torch.from_numpy(xs[2]), -1).numpy()
    dec = _ctc_decoder(path, 0.3)
    alone = [dec.search_device(torch.from_numpy(x).to(DEV).contiguous()) for x in xs]
    assert alone[2] == [[]] and len(alone[0][0]) > 0 and len(alone[1][0]) > 0
    assert [list(y) for y in alone[1]] == _oracle(m, xs[1], 0.3)
    batch = torch.zeros((3, max(lens), NC.SEARCH_V))
    for u, x in enumerate(xs):
        batch[u, :len(x)] = torch.from_numpy(x)
    calls = []
    hook = dec.lm.register_forward_hook(lambda mod, a, o: calls.append(a[0].shape[0]))
    got = dec.search_device_batch(batch.to(DEV), lens)
    hook.remove()
    ops.check_errors()
    assert got == alone
    t_start = [int(np.nonzero(x.argmax(-1) != 0)[0][0]) for x in xs[:2]]
    frames = max(lens[u] - t_start[u] for u in range(2))
    assert len(calls) == frames, (calls, frames)                      # <s> once + one call per lock-step frame but the last
    assert calls[0] == 1 and set(calls[1:]) == {3 * NC.SEARCH_BEAM}


def test_ctc_forward_batch_with_arpa_lm_equals_forward(ops, tmp_path):
    """end to end on the enc_ctc_concat golden model: packed encoder pass + lock-step search with the n-gram LM"""
    gm = load_golden("enc_ctc_concat")
    cfg, D, V = CASES["enc_ctc_concat"][0], CASES["enc_ctc_concat"][1], CASES["enc_ctc_concat"][2]
    model = _mod("src.asr").ASR(D, V, True, cfg["ctc_weight"], cfg["encoder"], {}, {})
    model.load_state_dict(golden_state_dict(gm), strict=True)
    model = model.to(DEV).eval()
    path = NC.estimated_arpa(tmp_path / "lm.arpa.gz", NC.corpus(2, V=V, lines=300), 3)
    dec = _mod("src.ctc").CTCBeamDecoder(model, NC.vocab_range(V), beam_size=4, vocab_candidate=5, lm_path=path,
                                         lm_config='', lm_weight=0.6, device=DEV)
    flen = torch.from_numpy(gm["feat_len"])[:3]
    assert len(set(flen.tolist())) == 3
    feat = torch.zeros((3, int(flen.max()), D))
    for u in range(3):
        feat[u, :int(flen[u])] = torch.from_numpy(gm["feat"])[u, :int(flen[u])]
    feat, flen = feat.to(DEV), flen.to(DEV)
    calls = []
    hook = dec.lm.register_forward_hook(lambda mod, a, o: calls.append(a[0].shape[0]))
    got = dec.forward_batch(feat, flen)
    hook.remove()
    ops.check_errors()
    frames = [int(v) for v in model.encoder.packed_frames.cpu().tolist()]
    assert 1 < len(calls) <= 1 + max(frames)
    alone = [dec(feat[u:u + 1, :int(flen[u])].contiguous(), flen[u:u + 1]) for u in range(3)]
    assert [[list(y) for y in h] for h in got] == [[list(y) for y in h] for h in alone]
    assert any(len(y) > 0 for h in got for y in h)


def test_host_bookkeeping_fallback_gives_the_same_hypotheses(ops, search_lm, monkeypatch):
    path, m = search_lm
    seed, lm_w = NC.SEARCH_CASES[1]
    x = NC.search_posteriors(seed)
    dec = _ctc_decoder(path, lm_w)
    xd = torch.from_numpy(x).to(DEV).contiguous()
    want = dec.search_device(xd)
    monkeypatch.setenv("ASRK_CTC_BEAM_DEVICE", "0")
    assert not dec._device_search_ok(NC.SEARCH_V)
    got = dec._search_host(xd)
    ops.check_errors()
    assert [list(y) for y in got] == [list(y) for y in want] == _oracle(m, x, lm_w)


# ---- joint CTC-attention search --------------------------------------------------------------------------------------------
def _joint(tmp_path):
    g = load_golden("las_hybrid_loc")
    cfg, D, V = CASES["las_hybrid_loc"][0], CASES["las_hybrid_loc"][1], CASES["las_hybrid_loc"][2]
    model = _mod("src.asr").ASR(D, V, True, cfg["ctc_weight"], cfg["encoder"], cfg["attention"] or {},
                                cfg["decoder"] or {})
    model.load_state_dict(golden_state_dict(g), strict=True)
    path = NC.joint_lm_arpa(tmp_path / "joint.arpa", V)
    dec = _mod("src.decode").BeamDecoder(model.to(DEV).eval(), None, min_len_ratio=0.01, max_len_ratio=0.5,
                                         lm_path=path, lm_config='', **NC.JOINT_KW)
    assert any("3-gram" in line for line in dec.create_msg())
    return g, cfg, V, path, dec


@pytest.mark.parametrize("host_beam", ["0", "1"])
def test_beam_decoder_with_arpa_lm_equals_oracle_with_float64_lm(ops, tmp_path, monkeypatch, host_beam):
    """host_beam 0: forward() runs the device-resident loop (forward_batch with one utterance, the state read through
    `parent` inside the step's launch); 1: the single-utterance loop with host bookkeeping (the state gathered with
    index_select)"""
    monkeypatch.setenv("ASRK_DECODE_HOST_BEAM", host_beam)
    g, cfg, V, path, dec = _joint(tmp_path)
    step = NR.f64_lm_step(NR.read_arpa(path, V))

    def lm_step(lm_sd, lm_cfg, tok, hidden):                          # beam_oracle.lm_step's contract: (logits, state)
        row, st = step(int(tok[0]), hidden)                           # log_softmax of a normalised model: identity
        return torch.from_numpy(row).unsqueeze(0), st
    monkeypatch.setattr(BO, "lm_step", lm_step)
    sd = golden_state_dict(g)
    feat, flen = torch.from_numpy(g["feat"])[:1], torch.from_numpy(g["feat_len"])[:1]
    kw = dict(min_len_ratio=0.01, max_len_ratio=0.5, beam_size=NC.JOINT_KW["beam_size"],
              ctc_weight=NC.JOINT_KW["ctc_weight"])
    want = BO.beam_search(sd, cfg, feat, flen, lm_weight=NC.JOINT_KW["lm_weight"], **kw)
    no_lm = BO.beam_search(sd, cfg, feat, flen, lm_weight=0.0, **kw)
    means = [sum(s) / len(s) for _, s in want]
    print("oracle mean scores", means)
    assert all(a - b > 2e-2 for a, b in zip(means, means[1:]))        # the case is decided by more than the tolerance
    assert want[0][0] != no_lm[0][0]                                  # and by the LM
    hyps = dec(feat.to(DEV), flen.to(DEV))
    ops.check_errors()
    assert len(hyps) == len(want)
    for h, (seq, scores) in zip(hyps, want):
        print(h.outIndex, np.abs(np.asarray(h.output_scores) - np.asarray(scores)).max())
    for h, (seq, scores) in zip(hyps, want):
        assert h.outIndex == [int(t) for t in seq]
        assert np.allclose(np.asarray(h.output_scores, np.float32), np.asarray(scores, np.float32), rtol=2e-3, atol=2e-3)


def test_beam_decoder_forward_batch_with_arpa_lm_equals_forward_bit_for_bit(ops, tmp_path):
    g, cfg, V, path, dec = _joint(tmp_path)
    assert dec.batchable()
    flen = torch.from_numpy(g["feat_len"])[:2]
    assert flen[0] != flen[1]
    feat = torch.from_numpy(g["feat"])[:2, :int(flen.max())].clone()
    for u in range(2):
        feat[u, int(flen[u]):] = 0
    feat, flen = feat.to(DEV), flen.to(DEV)
    got = dec.forward_batch(feat, flen)
    ops.check_errors()
    for u in range(2):
        alone = dec(feat[u:u + 1, :int(flen[u])].contiguous(), flen[u:u + 1])
        assert len(alone) == len(got[u]) > 0
        for a, b in zip(alone, got[u]):
            print(u, a.outIndex, np.abs(np.asarray(a.output_scores) - np.asarray(b.output_scores)).max())
        for a, b in zip(alone, got[u]):
            assert a.outIndex == b.outIndex
            assert a.output_scores == b.output_scores                 # bit-equal
