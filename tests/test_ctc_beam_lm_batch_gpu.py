"""GPU: pure-CTC prefix beam search with RNN-LM fusion for several utterances in lock-step
(CTCBeamDecoder.search_device_batch / forward_batch, csrc/prefix_beam.hip: prefix_beam_multi_kernel).
Hypotheses are integer lists and every comparison is equality."""
import ctypes
import importlib

import numpy as np
import pytest
import torch
import yaml

from conftest import PKG_NAME
from helpers import CASES, load_golden, golden_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _mod(name):
    return importlib.import_module(PKG_NAME + "." + name)


class _StubASR:
    enable_ctc = True

    def __init__(self, V):
        self.vocab_size = V


class _TableLM(torch.nn.Module):
    """bigram LM: the log-probs after token k are row k of a fixed table, gathered with index_select - a row's
    values are bit-identical however many rows are stepped together, so the search is the only thing compared"""

    def __init__(self, table):
        super().__init__()
        self.table = table

    def forward(self, x, lens, hidden=None):
        tok = x.reshape(-1).to(self.table.device)
        return self.table.index_select(0, tok).unsqueeze(1), torch.zeros((1, tok.numel(), 1), device=self.table.device)


LENS = (9, 1, 14, 6)
LM_W = 0.6


def _utterances(V):
    """four utterances of 9, 1, 14 and 6 frames; the fourth is all blank"""
    xs = []
    for u, T in enumerate(LENS):
        g = torch.Generator().manual_seed(100 + u)
        logits = torch.randn(T, V, generator=g) * 2
        logits[:, 0] += 3
        for k in (1, 3, 34, 35, V - 1):
            logits[:, k] += 4 * torch.rand(T, generator=g)
        if u == 3:
            logits[:, 0] += 30
        xs.append(torch.log_softmax(logits, -1))
    return xs


def _table_decoder(V, beam, cand, table):
    dec = _mod("src.ctc").CTCBeamDecoder(_StubASR(V), [1] + list(range(3, V)), beam, cand)
    dec.apply_lm, dec.lm_w, dec.device = True, LM_W, DEV
    dec.lm = _TableLM(table.to(DEV))
    assert dec._device_search_ok(V)
    return dec


_cache = {}


def _table_case(V, beam, cand):
    """per (V, beam, cand), computed once: inputs, the CPU oracle's hypotheses, search_device one utterance at a
    time, and the lock-step search with its workspace"""
    key = (V, beam, cand)
    if key not in _cache:
        from oracle import ctc_beam_oracle as CBO
        table = torch.log_softmax(torch.randn(V, V, generator=torch.Generator().manual_seed(7)) * 1.5, -1)
        tab_np = table.numpy()
        vr = [1] + list(range(3, V))
        xs = _utterances(V)
        want = [CBO.prefix_beam_search(x.numpy(), vr, beam, cand, lambda tok, hid: (tab_np[tok], None), LM_W)
                for x in xs]
        dec = _table_decoder(V, beam, cand, table)
        alone = [dec.search_device(x.to(DEV).contiguous()) for x in xs]
        batch = torch.zeros((len(xs), max(LENS), V))
        for u, x in enumerate(xs):
            batch[u, :len(x)] = x
        got, ws = dec.search_device_batch(batch.to(DEV), list(LENS), return_ws=True)
        _cache[key] = dict(xs=xs, want=want, alone=alone, got=got, ws=ws.cpu(), beam=beam)
    return _cache[key]


# (40, 4, 5): one wave ranks one row; (5200, 3, 4): V > 64 * 80 takes the workgroup-wide ranking with several rows,
# which only LM fusion reaches
@pytest.mark.parametrize("V,beam,cand", [(40, 4, 5), (5200, 3, 4)])
def test_lock_step_search_equals_oracle_and_single_utterance_search(ops, V, beam, cand):
    c = _table_case(V, beam, cand)
    ops.check_errors()
    assert len(c["got"]) == len(LENS)
    for u in range(len(LENS)):
        assert c["got"][u] == [list(y) for y in c["want"][u]], ("oracle", u)
        assert c["got"][u] == c["alone"][u], ("search_device", u)
    assert c["got"][3] == [[]]                                    # all blank
    assert len(c["got"][1]) >= 3                                  # the 1-frame utterance is searched: first = last frame
    assert len({len(y) for y in c["got"][0]} | {len(y) for y in c["got"][2]}) > 1


def test_all_blank_batch_returns_empty_hypotheses_before_any_lm_step(ops):
    """nothing to search: one empty hypothesis per utterance, and the return comes before the <sos> LM step that
    precedes the first launch (the LM is never called)"""
    V = 40
    x = torch.full((2, 5, V), -8.0)
    x[:, :, 0] = 5.0
    table = torch.log_softmax(torch.randn(V, V, generator=torch.Generator().manual_seed(7)), -1)
    dec = _table_decoder(V, 4, 5, table)
    calls = []
    dec.lm.register_forward_hook(lambda m, a, o: calls.append(1))
    assert dec.search_device_batch(torch.log_softmax(x, -1).to(DEV), [5, 3]) == [[[]], [[]]]
    assert calls == []


def _golden_lm_decoder(name, tmp_path):
    from oracle.gen_golden import CTC_BEAM_BIG, ctc_beam_big_logits
    V, T, beam, cand, seed, hot, lm_cfg, lm_w = CTC_BEAM_BIG[name]
    g = load_golden("ctcbeam_big")
    x = torch.log_softmax(ctc_beam_big_logits(name), dim=-1)
    pre = name + ".lm."
    yaml.safe_dump({"model": lm_cfg}, open(tmp_path / "lm.yaml", "w"))
    torch.save({"model": {k[len(pre):]: torch.from_numpy(v) for k, v in g.items() if k.startswith(pre)}},
               tmp_path / "lm.pth")
    dec = _mod("src.ctc").CTCBeamDecoder(_StubASR(V), [1] + list(range(3, V)), beam, cand,
                                         lm_path=str(tmp_path / "lm.pth"), lm_config=str(tmp_path / "lm.yaml"),
                                         lm_weight=lm_w, device=DEV)
    want = [g["%s.hyp%d" % (name, i)].tolist() for i in range(int(g[name + ".n"]))]
    return dec, x, want


@pytest.mark.parametrize("name", ["lm", "lm_gru"])
def test_lock_step_search_equals_real_reference_with_rnn_lm(ops, tmp_path, name):
    """the real reference's hypotheses (tests/golden/ctcbeam_big.npz, LSTM LM with an (h, c) state / tied GRU LM
    with a single state tensor) for the golden utterance at two positions of a batch that also holds shorter
    utterances: x[:50] and - shorter than every golden utterance - x[:23], which end while the others go on"""
    dec, x, want = _golden_lm_decoder(name, tmp_path)
    parts = [x, x[:50], x, x[:23]]
    lens = [len(p) for p in parts]
    batch = torch.zeros((len(parts), max(lens), x.shape[1]))
    for u, p in enumerate(parts):
        batch[u, :len(p)] = p
    got = dec.search_device_batch(batch.to(DEV), lens)
    ops.check_errors()
    assert got[0] == want
    assert got[2] == want
    assert got[1] == dec.search_device(x[:50].to(DEV).contiguous())
    assert got[3] == dec.search_device(x[:23].to(DEV).contiguous())


@pytest.mark.parametrize("tag,lm_cfg", [
    ("lstm", dict(emb_tying=False, emb_dim=6, module='LSTM', dim=9, n_layers=1, dropout=0.0)),
    ("gru", dict(emb_tying=True, emb_dim=8, module='GRU', dim=8, n_layers=2, dropout=0.0)),
])
def test_forward_batch_with_lm_matches_reference_in_one_lm_step_per_frame(ops, tmp_path, monkeypatch, tag, lm_cfg):
    """end to end: packed encoder pass + lock-step search on the enc_ctc_concat golden model, the LM called once per
    lock-step frame, not once per frame of every utterance.

    The goldens (tests/golden/ctcbeam_lm.npz) are what the real reference returned for feat[u:u+1] as stored: ALL 37
    frames of the row, zero padding included (its encoder does not pack, and its search walks the whole tensor -
    oracle/gen_golden.py:546-552, and how test_ctc_beam_decoder_with_lm_matches_reference feeds forward()).  A batch
    cut at each utterance's own feat_len (37, 35, 26) is therefore a different input for utterances 1 and 2 - on the
    MI355X utterance 1 of the 'lstm' case then ends [10, 8, 9] where the golden has [10, 8, 8], from forward() alone
    and from forward_batch alike.  So both are checked: the goldens on the rows as the reference saw them (three
    utterances of 37 frames), and the batch at the utterances' own lengths against forward() on every utterance
    alone and unpadded."""
    g = load_golden("ctcbeam_lm")
    gm = load_golden("enc_ctc_concat")
    cfg, D, V = CASES["enc_ctc_concat"][0], CASES["enc_ctc_concat"][1], CASES["enc_ctc_concat"][2]
    model = _mod("src.asr").ASR(D, V, True, cfg["ctc_weight"], cfg["encoder"], {}, {})
    model.load_state_dict(golden_state_dict(gm), strict=True)
    model = model.to(DEV).eval()
    yaml.safe_dump({"model": lm_cfg}, open(tmp_path / "lm.yaml", "w"))
    pre = tag + ".lm."
    torch.save({"model": {k[len(pre):]: torch.from_numpy(v) for k, v in g.items() if k.startswith(pre)}},
               tmp_path / "lm.pth")
    dec = _mod("src.ctc").CTCBeamDecoder(model, [1] + list(range(3, V)), beam_size=4, vocab_candidate=5,
                                         lm_path=str(tmp_path / "lm.pth"), lm_config=str(tmp_path / "lm.yaml"),
                                         lm_weight=0.6, device=DEV)
    want = [[g["%s.u%d.hyp%d" % (tag, u, i)].tolist() for i in range(int(g["%s.u%d.n" % (tag, u)]))]
            for u in range(3)]
    lists = lambda res: [[list(y) for y in h] for h in res]

    def batched(feat, flen):
        calls = []
        hook = dec.lm.register_forward_hook(lambda m, a, o: calls.append(a[0].shape[0]))
        got = dec.forward_batch(feat, flen)
        hook.remove()
        ops.check_errors()
        frames = [int(v) for v in model.encoder.packed_frames.cpu().tolist()]
        print("LM calls", len(calls), "rows per call", sorted(set(calls)), "encoder frames", frames)
        assert len(calls) <= 1 + max(frames)                      # the parent: 1 + frames per utterance, summed
        return lists(got)

    # the rows as the reference decoded them: equal to the goldens
    stored = torch.from_numpy(gm["feat"])[:3].to(DEV)
    full = torch.full((3,), stored.shape[1], dtype=torch.long, device=DEV)
    assert batched(stored, full) == want
    # a zero-padded batch of the three utterances at their own feat_len: each as forward() decodes it alone
    flen = torch.from_numpy(gm["feat_len"])[:3]
    assert len(set(flen.tolist())) == 3
    feat = torch.zeros((3, int(flen.max()), D))
    for u in range(3):
        feat[u, :int(flen[u])] = torch.from_numpy(gm["feat"])[u, :int(flen[u])]
    feat, flen = feat.to(DEV), flen.to(DEV)
    got = batched(feat, flen)
    alone = [lists([dec(feat[u:u + 1, :int(flen[u])].contiguous(), flen[u:u + 1])])[0] for u in range(3)]
    assert got == alone
    assert got[0] == want[0]                                      # utterance 0 fills the row: the golden itself
    # the fallback (host bookkeeping, one utterance at a time) is unchanged
    monkeypatch.setenv("ASRK_CTC_BEAM_DEVICE", "0")
    assert lists(dec.forward_batch(stored, full)) == want
    assert lists(dec.forward_batch(feat, flen)) == got


def test_finished_utterance_slab_is_left_alone(ops):
    """the 1-frame utterance of the V = 40 batch ends after step 0; thirteen more launches follow.  Its slab, read
    through asrk_ctc_prefix_beam_ws_offsets at its final buffer (T_u - t_start_u) & 1, still holds the beam that
    search_device leaves for that utterance alone: live-row count, lengths, tokens"""
    c = _table_case(40, 4, 5)
    L = importlib.import_module(PKG_NAME + "._lib").load()
    W, Tmax, u = c["beam"], max(LENS), 1
    assert int(c["xs"][u][0].argmax()) != 0                       # t_start = 0, T = 1: final buffer 1
    o = [ctypes.c_int64(0) for _ in range(6)]
    assert L.asrk_ctc_prefix_beam_ws_offsets(W, Tmax, (LENS[u] - 0) & 1, *[ctypes.byref(v) for v in o]) == 0
    nb_off, len_off, tok_off = (int(v.value) // 4 for v in o[:3])
    slab = c["ws"][u]
    nb = int(slab[nb_off])
    lens = slab[len_off:len_off + W].tolist()
    toks = slab[tok_off:tok_off + W * (Tmax + 1)].view(W, Tmax + 1)
    alone = c["alone"][u]
    assert nb == len(alone)
    assert lens[:nb] == [len(y) for y in alone]
    assert [toks[r, :lens[r]].tolist() for r in range(nb)] == alone
    # the all-blank utterance never ran: its slab is as the caller allocated it
    assert int(np.abs(c["ws"][3].numpy()).max()) == 0
