"""GPU: the three beam searches with contextual biasing (src/bias.py: ContextBias alone, BiasedNGram beside the n-gram
LM) on tiny models.

 * transducer: TransducerHead.beam_search against rnnt_beam_reference.run_case given the numpy bias (+ n-gram) row as
   its LM, the pending bonus of every finished hypothesis taken back and the lists re-sorted - LSTM and stateless
   heads, beam 1 and 4.  Only settings whose float64 margins exceed rnnt_beam_reference.MIN_MARGIN are compared (at
   least three of every four must); scores under the rule of tests/test_rnnt_beam_gpu.py: within 2 * max(E, floor).
 * CTC: search_device and search_device_batch equal the decoder's host path with the same scorer and the CPU search
   oracle given the float32 restatement; a batch equals its utterances decoded alone.
 * joint: forward_batch equals forward with host bookkeeping.
 * one planted case per search: the phrase's tokens are the runner-up at every position; without biasing the search
   misses the phrase, with it the phrase is the output.
 * without a scorer the three searches give what they gave."""
import importlib

import numpy as np
import pytest
import torch

import bias_cases as BC
import bias_reference as BR
import ngram_cases as NC
import ngram_reference as NR
import rnnt_beam_reference as RB
import rnnt_reference as RR
from conftest import PKG_NAME
from helpers import CASES, load_golden, golden_state_dict
from oracle import ctc_beam_oracle as CBO
from test_rnnt_beam_gpu import _existing_lp, _lists

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 2.0 ** -23
MS, ML = RR.GREEDY_MAX_SYMBOLS, RR.GREEDY_MAX_LEN
CB = BC.bias_mod()


def _mod(name):
    return importlib.import_module(PKG_NAME + "." + name)


# ---- transducer -----------------------------------------------------------------------------------------------------
_compared = {}


def _rnnt_scorer(image):
    cb = CB.ContextBias(CB.build_image(BC.RNNT_PHRASES, RR.GREEDY_V, BC.RNNT_WEIGHT))
    if image is None:
        return cb.to(DEV)
    return CB.BiasedNGram.pair(_mod("src.ngram").NGramLM(image), cb, RB.BEAM_LM_WEIGHT).to(DEV)


@pytest.mark.parametrize("head_name,W,with_ngram", BC.RNNT_SETTINGS)
def test_transducer_search_against_the_reference(ops, head_name, W, with_ngram):
    f = BC.rnnt_setting(head_name, W, with_ngram)
    _compared[(head_name, W, with_ngram)] = f["margin"] >= RB.MIN_MARGIN
    print("setting", head_name, W, with_ngram, "margin %.3g" % f["margin"])
    if not _compared[(head_name, W, with_ngram)]:
        return                                              # counted by test_three_of_every_four_settings_were_compared
    head, enc, lens, lw = f["head"].to(DEV).eval(), f["enc"], f["lens"], f["weight"]
    scorer = _rnnt_scorer(f["ngram_image"])
    enc_d, lens_d = enc.to(DEV).contiguous(), lens.to(DEV)
    out = head.beam_search(enc_d, lens_d, W, MS, ML, nbest=W, lm=scorer, lm_weight=lw)
    ops.check_errors()
    exist = RB.run_case(f["ref"], enc, lens, W, MS, ML, f["lm_row"], lw,
                        lp_fn=lambda b: _existing_lp(head, enc_d[b, :int(lens[b])].contiguous()))
    out_h = [t.cpu() for t in out]
    pending = 0
    for b in range(enc.shape[0]):
        got, fin = _lists(out_h, b), f["banked"][b]
        raw, trace = f["want"][b]
        assert [g[0] for g in got] == [t for t, _ in fin], (b, got, fin)                 # tokens and order
        exist_b = BC.bank(exist[b][0], f["residual"], lw)
        assert [t for t, _ in exist_b] == [t for t, _ in fin]
        ref_s = np.array([s for _, s in fin])
        E = float(np.abs(np.array([s for _, s in exist_b]) - ref_s).max())
        # the row's own rounding: the fused row is one float32 add of values up to max_row in size per label
        max_row = max(float(np.abs(f["lm_row"](t[:k])[1:]).max()) for t, _ in fin for k in range(len(t) + 1))
        floor = (int(lens[b]) + ML) * EPS * max(trace["max_lp"], lw * max_row)
        err = float(np.abs(np.array([g[1] for g in got]) - ref_s).max())
        print("utt", b, "E %.3g floor %.3g err %.3g" % (E, floor, err))
        assert err <= 2 * max(E, floor), (b, err, E, floor)
        pending += sum(f["residual"](t) > 0 for t, _ in raw)
    if W > 1:
        assert pending > 0                                  # finished hypotheses stop inside a phrase: the correction ran
    # a batch = one utterance at a time, bit for bit; two runs: the same
    out2 = head.beam_search(enc_d, lens_d, W, MS, ML, nbest=W, lm=scorer, lm_weight=lw)
    assert all(torch.equal(a, b) for a, b in zip(out, out2))
    one = head.beam_search(enc_d[1:2, :int(lens[1])].contiguous(), lens_d[1:2], W, MS, ML, nbest=W, lm=scorer, lm_weight=lw)
    assert all(torch.equal(a[1], c[0]) for a, c in zip(out, one))
    ops.check_errors()


def test_three_of_every_four_settings_were_compared():
    if len(_compared) < len(BC.RNNT_SETTINGS):              # run alone: the reference side decides
        for s in BC.RNNT_SETTINGS:
            _compared.setdefault(s, BC.rnnt_setting(*s)["margin"] >= RB.MIN_MARGIN)
    assert 4 * sum(_compared.values()) >= 3 * len(_compared), _compared


def test_transducer_planted_phrase(ops):
    tr = _mod("src.transducer")
    head, enc, lens, best = BC.planted_rnnt_head(tr.TransducerHead)
    head = head.to(DEV).eval()
    cb = CB.ContextBias(CB.build_image([(BC.PLANTED_PHRASE, 1.0)], 11, CB.DEFAULT_WEIGHT)).to(DEV)
    plain = head.beam_search(enc.to(DEV), lens.to(DEV), 4, 1, 4, nbest=4)
    again = head.beam_search(enc.to(DEV), lens.to(DEV), 4, 1, 4, nbest=4, lm=None, lm_weight=0.0)
    assert all(torch.equal(a, b) for a, b in zip(plain, again))
    biased = head.beam_search(enc.to(DEV), lens.to(DEV), 4, 1, 4, nbest=4, lm=cb, lm_weight=1.0)
    ops.check_errors()
    assert _lists([t.cpu() for t in plain], 0)[0][0] == tuple(best)
    top = _lists([t.cpu() for t in biased], 0)
    assert top[0][0] == BC.PLANTED_PHRASE and top[0][1] - top[1][1] > 1.0
    # the whole phrase is banked: 4 edges of DEFAULT_WEIGHT on top of the acoustic score of the runner-up path
    ref = RR.HeadRef.of(head.cpu(), enc.shape[2])
    rb = BR.Ref([(BC.PLANTED_PHRASE, 1.0)], 11, CB.DEFAULT_WEIGHT)
    fin = RB.run_case(ref, enc, lens, 4, 1, 4, lambda tok: rb.row(rb.state(tok)).astype(np.float64), 1.0)[0][0]
    assert abs(top[0][1] - fin[0][1]) < 1e-4


# ---- CTC prefix beam search ---------------------------------------------------------------------------------------------
class _StubASR:
    enable_ctc = True

    def __init__(self, V):
        self.vocab_size = V


@pytest.fixture(scope="module")
def search_lm(tmp_path_factory):
    return NC.search_lm_arpa(tmp_path_factory.mktemp("blm") / "lm.arpa")


def _ctc_decoder(phrases, lm_path='', lm_w=0.0, weight=CB.DEFAULT_WEIGHT):
    V = NC.SEARCH_V
    cb = CB.ContextBias(CB.build_image(phrases, V, weight)) if phrases else None
    return _mod("src.ctc").CTCBeamDecoder(_StubASR(V), NC.vocab_range(V), NC.SEARCH_BEAM, NC.SEARCH_CAND, lm_path=lm_path,
                                          lm_config='', lm_weight=lm_w, device=DEV, bias=cb)


@pytest.mark.parametrize("lm_w", [0.0, 0.3])
def test_ctc_searches_equal_the_host_path_and_the_oracle(ops, search_lm, monkeypatch, lm_w):
    V = NC.SEARCH_V
    phrases = BC.search_phrases(V)
    dec = _ctc_decoder(phrases, search_lm if lm_w else '', lm_w)
    assert isinstance(dec.lm, CB.BiasedNGram if lm_w else CB.ContextBias)
    assert dec.lm_w == (lm_w if lm_w else 1.0) and any("Contextual biasing" in m for m in dec.create_msg())
    lens = [30, 19, 30, 11]
    xs = [NC.search_posteriors(0), NC.search_posteriors(3)[:19], NC.search_posteriors(5), NC.search_posteriors(4)[:11].copy()]
    xs[3][:, 0] += 40.0                                     # the fourth utterance is all blank
    xs[3] = torch.log_softmax(torch.from_numpy(xs[3]), -1).numpy()
    assert dec._device_search_ok(V)
    alone = [dec.search_device(torch.from_numpy(x).to(DEV).contiguous()) for x in xs]
    assert alone[3] == [[]] and all(len(alone[u][0]) > 0 for u in range(3))
    batch = torch.zeros((4, max(lens), V))
    for u, x in enumerate(xs):
        batch[u, :len(x)] = torch.from_numpy(x)
    got = dec.search_device_batch(batch.to(DEV), lens)      # reachable with bias alone
    ops.check_errors()
    assert got == alone
    monkeypatch.setenv("ASRK_CTC_BEAM_DEVICE", "0")
    assert not dec._device_search_ok(V)
    host = [dec._search_host(torch.from_numpy(x).to(DEV).contiguous()) for x in xs]
    assert [[list(y) for y in h] for h in host] == [[list(y) for y in h] for h in alone]
    if not lm_w:                                            # the CPU oracle with the float32 restatement as its scorer
        image = CB.build_image(phrases, V, CB.DEFAULT_WEIGHT)
        no_bias = _ctc_decoder(None)
        changed = 0
        for u in range(3):
            want = CBO.prefix_beam_search(xs[u], NC.vocab_range(V), NC.SEARCH_BEAM, NC.SEARCH_CAND,
                                          lm_step=BC.f32_step(BR, image), lm_w=1.0)
            assert [list(y) for y in alone[u]] == [list(y) for y in want], u
            changed += alone[u][0] != no_bias.search_device(torch.from_numpy(xs[u]).to(DEV).contiguous())[0]
        assert changed >= 2                                 # the scorer decides these searches
    ops.check_errors()


def test_ctc_planted_phrase_and_no_scorer(ops):
    V = NC.SEARCH_V
    x, best = BC.planted_ctc(V)
    xd = torch.from_numpy(x).to(DEV).contiguous()
    plain = _ctc_decoder(None)
    assert not plain.apply_lm and plain.bias is None
    assert list(plain.search_device(xd)[0]) == best
    assert plain.search_device(xd) == _mod("src.ctc").CTCBeamDecoder(
        _StubASR(V), NC.vocab_range(V), NC.SEARCH_BEAM, NC.SEARCH_CAND).search_device(xd)
    dec = _ctc_decoder([(BC.PLANTED_PHRASE, 1.0)])
    assert list(dec.search_device(xd)[0]) == list(BC.PLANTED_PHRASE)
    assert list(dec.search_device_batch(xd.unsqueeze(0), [x.shape[0]])[0][0]) == list(BC.PLANTED_PHRASE)
    ops.check_errors()


# ---- joint CTC-attention search --------------------------------------------------------------------------------------------
JOINT_PHRASES = [((8, 5, 9), 1.0), ((10, 6, 4), 1.0), ((7, 11, 3), 2.0)]


def _joint(tmp_path, phrases, lm=False, **kw):
    g = load_golden("las_hybrid_loc")
    cfg, D, V = CASES["las_hybrid_loc"][0], CASES["las_hybrid_loc"][1], CASES["las_hybrid_loc"][2]
    model = _mod("src.asr").ASR(D, V, True, cfg["ctc_weight"], cfg["encoder"], cfg["attention"] or {},
                                cfg["decoder"] or {})
    model.load_state_dict(golden_state_dict(g), strict=True)
    args = dict(NC.JOINT_KW)
    if lm:
        args["lm_path"] = NC.joint_lm_arpa(tmp_path / "joint.arpa", V)
    else:
        args["lm_weight"] = 0.0
    args.update(kw)
    cb = CB.ContextBias(CB.build_image(phrases, V, CB.DEFAULT_WEIGHT)) if phrases else None
    # max_len_ratio 0.25: at most 7 labels on 13 encoder frames, so that every hypothesis is feasible for the CTC prefix
    # scorer even when all its labels repeat (at 0.5 the tail of the beam is logzero-scored: ranked by float32 noise at 4e6)
    dec = _mod("src.decode").BeamDecoder(model.to(DEV).eval(), None, min_len_ratio=0.01, max_len_ratio=0.25,
                                         lm_config='', bias=cb, **args)
    return g, dec


def _feats(g, n):
    flen = torch.from_numpy(g["feat_len"])[:n]
    feat = torch.from_numpy(g["feat"])[:n, :int(flen.max())].clone()
    for u in range(n):
        feat[u, int(flen[u]):] = 0
    return feat.to(DEV), flen.to(DEV)


def _has(seq, phrase):
    return any(tuple(seq[i:i + len(phrase)]) == tuple(phrase) for i in range(len(seq)))


@pytest.mark.parametrize("lm", [False, True])
def test_joint_forward_batch_equals_forward_with_host_bookkeeping(ops, tmp_path, monkeypatch, lm):
    g, dec = _joint(tmp_path, JOINT_PHRASES, lm)
    assert dec.batchable() and isinstance(dec.lm, CB.BiasedNGram if lm else CB.ContextBias)
    assert dec.lm_w == (NC.JOINT_KW["lm_weight"] if lm else 1.0)
    assert any("Contextual biasing" in m for m in dec.create_msg())
    feat, flen = _feats(g, 2)
    got = dec.forward_batch(feat, flen)
    ops.check_errors()
    monkeypatch.setenv("ASRK_DECODE_HOST_BEAM", "1")
    for u in range(2):
        alone = dec(feat[u:u + 1, :int(flen[u])].contiguous(), flen[u:u + 1])
        assert len(alone) == len(got[u]) > 0
        for a, b in zip(alone, got[u]):
            print(u, a.outIndex, np.abs(np.asarray(a.output_scores) - np.asarray(b.output_scores)).max())
        for a, b in zip(alone, got[u]):
            assert a.outIndex == b.outIndex
            # the two paths run the same kernels on other row counts: GEMM summation order differs, ~1e-6 relative
            # (BeamDecoder.forward_batch); per-label scores stay below 10 in size, so 1e-4 is a hundred times that
            assert np.abs(np.asarray(a.output_scores) - np.asarray(b.output_scores)).max() < 1e-4
    ops.check_errors()


def test_joint_planted_phrase_and_no_scorer(ops, tmp_path):
    phrase = JOINT_PHRASES[1][0]
    g, plain = _joint(tmp_path, None)
    assert not plain.apply_lm and plain.bias is None
    feat, flen = _feats(g, 1)
    base = plain(feat, flen)
    g, same = _joint(tmp_path, None)                        # without a scorer: what the search gave before
    again = same.forward_batch(feat, flen)[0]
    assert [h.outIndex for h in base] == [h.outIndex for h in again]
    assert [h.output_scores for h in base] == [h.output_scores for h in again]
    assert not _has(base[0].outIndex, phrase)
    g, dec = _joint(tmp_path, [(phrase, 1.0)])
    best = dec(feat, flen)[0]
    ops.check_errors()
    assert _has(best.outIndex, phrase), best.outIndex


# ---- decode pass ----------------------------------------------------------------------------------------------------------
def test_decode_pass_with_the_bias_block(tmp_path):
    """`main.py --test` with a decode.bias block in each of the three decode modes writes the usual files"""
    import json
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    out = str(tmp_path / "bias.json")
    r = subprocess.run([sys.executable, os.path.join(here, "bias_worker.py"), out], capture_output=True, text=True,
                       env=dict(os.environ, ASRK_DETERMINISTIC="1"), timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.load(open(out))
    beam_files = ["{}_dev_beam-2-0.0.csv", "{}_dev_output.csv", "{}_test_beam-2-0.0.csv", "{}_test_output.csv"]
    assert res["plain"]["files"] == res["joint"]["files"] == res["ctc"]["files"] == beam_files
    assert res["rnnt_one"]["files"] == ["{}_dev_output.csv", "{}_test_output.csv"]
    assert res["rnnt_lm"]["files"] == ["{}_dev_beam-2-0.3.csv", "{}_dev_output.csv", "{}_test_beam-2-0.3.csv",
                                       "{}_test_output.csv"]
    n_dev, n_test = len(res["plain"]["texts"][1]), len(res["plain"]["texts"][3])
    assert n_dev == 4 and n_test == 3                                   # header + utterances
    for name in ("joint", "ctc", "rnnt_lm"):
        t = res[name]["texts"]
        assert t[1][0] == "idx\thyp\ttruth" and len(t[1]) == n_dev and len(t[3]) == n_test, name
        assert [ln.split("\t")[2] for ln in t[1][1:]] == [ln.split("\t")[2] for ln in res["plain"]["texts"][1][1:]]
    t = res["rnnt_one"]["texts"]
    assert len(t[0]) == n_dev and len(t[1]) == n_test
    assert "greedy" in res["greedy_error"]
