"""End to end on the GPU: `main.py --test` with `decode: {align: true}` force-aligns the dev and test sets of a
synthetic wav corpus with a seeded tiny hybrid CTC-attention model and writes the alignment files; the rows equal
ASR.ctc_align called on every utterance alone (so grouping / padding change nothing), the seconds follow from the
config, and without the key `--test` writes what it always wrote."""
import importlib
import os

import pytest
import torch

from test_e2e_gpu import _configs, _decode_cfg, _make_corpus

pytestmark = pytest.mark.gpu
PKG = "end-to-end-asr-pytorch_amd"


def _seeded_checkpoint(tmp, train, vocab):
    asr = importlib.import_module(PKG + '.src.asr')
    text = importlib.import_module(PKG + '.src.text')
    vocab_size = text.load_text_encoder('character', vocab).vocab_size
    feat_dim = train['data']['audio']['feat_dim'] * (train['data']['audio']['delta_order'] + 1)
    torch.manual_seed(0)
    model = asr.ASR(feat_dim, vocab_size, True, **train['model'])
    path = os.path.join(tmp, 'seeded.pth')
    torch.save({'model': model.state_dict(), 'global_step': 0}, path)
    return path


def _rows(path):
    lines = open(path, encoding='UTF-8').read().split('\n')
    assert lines[-1] == ''
    return lines[0], [l.split('\t') for l in lines[1:-1]]


def test_align_through_main(tmp_path, monkeypatch):
    main = importlib.import_module(PKG + '.main')
    align_asr = importlib.import_module(PKG + '.bin.align_asr')
    monkeypatch.delenv('ASRK_DECODE_BATCH', raising=False)
    groups, many = [], align_asr.align_many
    monkeypatch.setattr(align_asr, 'align_many', lambda items, *a: groups.append(len(items)) or many(items, *a))
    tmp = str(tmp_path)
    root = os.path.join(tmp, 'corpus')
    vocab = _make_corpus(root)
    train, tr_path = _configs(root, vocab, tmp)
    ckpt = _seeded_checkpoint(tmp, train, vocab)
    result = os.path.join(tmp, 'result')
    common = ['--logdir', os.path.join(tmp, 'log'), '--ckpdir', os.path.join(tmp, 'ckpt'), '--outdir', result,
              '--njobs', '1', '--no-msg']
    enc = train['model']['encoder']
    assert enc['prenet'] == '' and enc['sample_rate'] == [2, 2] and train['data']['audio']['frame_shift'] == 10
    sec = (2 * 2) * 10 * 0.001                        # encoder subsampling x feature frame shift

    acfg = _decode_cfg(tmp, tr_path, ckpt, 'dec_align', align=True)
    solver = main.main(['--config', acfg, '--test'] + common)
    # the run took the grouped path: each set went through the packed encoder as ONE padded batch
    assert solver.model.encoder.supports_packed() and groups == [3, 2]
    assert sorted(os.listdir(result)) == ['dec_align_dev_align.tsv', 'dec_align_dev_align_score.tsv',
                                          'dec_align_test_align.tsv', 'dec_align_test_align_score.tsv']
    n_rows = 0
    for s, ds, n_utt in (('dev', solver.dv_set, 3), ('test', solver.tt_set, 2)):
        head, rows = _rows(os.path.join(result, 'dec_align_%s_align.tsv' % s))
        assert head == 'idx\tpos\ttoken\tstart_frame\tend_frame\tstart_s\tend_s'
        shead, scores = _rows(os.path.join(result, 'dec_align_%s_align_score.tsv' % s))
        assert shead == 'idx\tscore' and len(scores) == n_utt
        want_rows, want_scores = [], []
        for name, feat, feat_len, txt in ds:          # every utterance alone, unpadded, through the plain encoder
            txt = txt.to(solver.device)
            txt_len = (txt != 0).sum(-1)
            states, tokens, spans, score, enc_len = solver.model.ctc_align(
                feat.to(solver.device), feat_len.to(solver.device), txt, txt_len)
            L, T = int(txt_len[0]), int(enc_len[0])
            assert states.shape[0] == 1 and L >= 1
            want_scores.append([name[0], repr(float(score[0]))])
            if not float(score[0]) > float('-inf'):
                continue
            sp = spans[0, :L].cpu().tolist()
            assert sp[0][0] >= 0 and sp[-1][1] <= T and (states[0, :T] >= 0).all() and (states[0, T:] == -1).all()
            for l in range(L):
                want_rows.append([name[0], str(l), solver.tokenizer.idx_to_vocab(int(txt[0, l])),
                                  str(sp[l][0]), str(sp[l][1])])
        assert scores == want_scores
        assert [r[:5] for r in rows] == want_rows
        for r in rows:                                 # seconds = frames x subsampling x shift
            assert abs(float(r[5]) - int(r[3]) * sec) <= 5e-7 and abs(float(r[6]) - int(r[4]) * sec) <= 5e-7
        n_rows += len(rows)
    assert n_rows > 0

    # without the key: the files `--test` always wrote, and no alignment file
    gcfg = _decode_cfg(tmp, tr_path, ckpt, 'dec_plain', beam_size=1, min_len_ratio=0.01, max_len_ratio=0.3)
    main.main(['--config', gcfg, '--test'] + common)
    plain = sorted(f for f in os.listdir(result) if f.startswith('dec_plain'))
    assert plain == ['dec_plain_dev_output.csv', 'dec_plain_test_output.csv']
    for s, n in (('dev', 3), ('test', 2)):
        lines = open(os.path.join(result, 'dec_plain_%s_output.csv' % s)).read().splitlines()
        assert lines[0] == 'idx\thyp\ttruth' and len(lines) == n + 1


def test_align_needs_a_ctc_head():
    asr = importlib.import_module(PKG + '.src.asr')
    cfg = dict(encoder=dict(prenet='', module='LSTM', bidirection=True, dim=[16], dropout=[0], layer_norm=[False],
                            proj=[False], sample_rate=[1], sample_style='drop'),
               attention=dict(mode='dot', dim=16, num_head=1, v_proj=False, temperature=1.0, loc_kernel_size=5,
                              loc_kernel_num=2),
               decoder=dict(module='LSTM', dim=16, layer=1, dropout=0))
    model = asr.ASR(8, 10, True, 0.0, cfg['encoder'], cfg['attention'], cfg['decoder'])
    with pytest.raises(RuntimeError, match='CTC head'):
        model.ctc_align(torch.zeros((1, 6, 8)), torch.tensor([6]), torch.ones((1, 2), dtype=torch.int64),
                        torch.tensor([2]))
