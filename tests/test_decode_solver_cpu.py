"""CPU: the testing solver of `main.py --test` (bin/decode_asr.py) hands pure-CTC beam search WITH an RNN-LM to
`forward_batch` in groups of ASRK_DECODE_BATCH utterances (default 16), in corpus order, and goes back to the parent
class's one-at-a-time loop for ASRK_DECODE_BATCH=1.  The decoder is a recorder: no GPU, no model."""
import importlib
import types

import torch

from conftest import PKG_NAME


class _Recorder:
    """stands for CTCBeamDecoder: returns [[first frame's first feature as a token]] per utterance"""
    apply_lm = True

    def __init__(self):
        self.batches, self.singles = [], 0

    def forward_batch(self, feat, feat_len):
        self.batches.append([int(v) for v in feat_len.tolist()])
        return [[[int(feat[u, 0, 0])]] for u in range(feat.shape[0])]

    def __call__(self, feat, feat_len):
        self.singles += 1
        return [[int(feat[0, 0, 0])]]


class _Tok:
    def decode(self, ids, ignore_repeat=False):
        return ' '.join(str(i) for i in ids)


def _solver(tmp_path, n):
    mod = importlib.import_module(PKG_NAME + ".bin.decode_asr")
    s = object.__new__(mod.Solver)
    items = []
    for i in range(n):
        T = 3 + i % 4
        feat = torch.zeros(1, T, 2)
        feat[0, :, 0] = 100 + i
        items.append((['utt%d' % i], feat, torch.tensor([T]), torch.tensor([[5, i]])))
    s.config = {'decode': {'beam_size': 4, 'lm_weight': 0.5}}
    s.paras = types.SimpleNamespace(verbose=False)
    s.rank, s.world, s.dist, s.step = 0, 1, None, 0
    s.device = torch.device('cpu')
    s.greedy, s.ctc_only, s.enable_att = False, True, False
    s.decoder, s.tokenizer = _Recorder(), _Tok()
    s.dv_set, s.tt_set = items, items[:3]
    s.output_file = str(tmp_path / 'run') + '_{}_{}.csv'
    return s, items


def test_ctc_lm_decoding_goes_to_forward_batch_in_groups(tmp_path, monkeypatch):
    monkeypatch.delenv('ASRK_DECODE_BATCH', raising=False)
    s, items = _solver(tmp_path, 37)
    s.exec()
    lens = [int(d[2][0]) for d in items]
    assert s.decoder.singles == 0
    assert s.decoder.batches == [lens[:16], lens[16:32], lens[32:], lens[:3]]       # dev: 16 + 16 + 5, test: 3
    rows = open(str(tmp_path / 'run') + '_dev_output.csv').read().splitlines()
    assert rows[0] == 'idx\thyp\ttruth'
    assert rows[1:] == ['utt%d\t%d\t5 %d' % (i, 100 + i, i) for i in range(37)]     # corpus order, own hypothesis
    beams = open(str(tmp_path / 'run') + '_dev_beam-4-0.5.csv').read().splitlines()
    assert beams[0] == 'idx\tbeam\thyp\ttruth' and len(beams) == 38


def test_group_size_follows_the_environment(tmp_path, monkeypatch):
    monkeypatch.setenv('ASRK_DECODE_BATCH', '5')
    s, items = _solver(tmp_path, 12)
    s.exec()
    assert [len(b) for b in s.decoder.batches] == [5, 5, 2, 3]
    monkeypatch.setenv('ASRK_DECODE_BATCH', '1')                   # one utterance at a time: the parent's loop
    s, items = _solver(tmp_path, 12)
    s.exec()
    assert s.decoder.batches == [] and s.decoder.singles == 15
    rows = open(str(tmp_path / 'run') + '_dev_output.csv').read().splitlines()
    assert rows[1:] == ['utt%d\t%d\t5 %d' % (i, 100 + i, i) for i in range(12)]
