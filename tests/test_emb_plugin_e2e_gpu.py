"""End to end on the GPU: `main.py` trains with an `emb:` block (word-embedding regulariser + embedding-fusion decoder)
on the synthetic corpus of tests/test_e2e_gpu.py, the checkpoint carries the plug-in, a resumed run loads it, the test
solver decodes with fusion (greedy and beam); without the block nothing of the plug-in is touched."""
import importlib
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from test_e2e_gpu import PKG, WORDS, _make_corpus, _configs, _decode_cfg

pytestmark = pytest.mark.gpu
EMB_DIM = 8


def _embedding_file(tmp):
    """fastText-style vectors for the corpus' letters (the space token has no line: its row stays zero), `</s>` and
    two words the character vocabulary does not know"""
    rng = np.random.RandomState(0)
    names = ['</s>'] + sorted(set(''.join(WORDS))) + ['?', '!']
    path = os.path.join(tmp, 'emb.txt')
    with open(path, 'w') as f:
        f.write('%d %d\n' % (len(names), EMB_DIM))
        for w in names:
            f.write(w + ' ' + ' '.join('%.4f' % v for v in rng.uniform(-1, 1, EMB_DIM)) + '\n')
    return path


def _spy_first_loss(mod):
    seen = []
    orig = mod.Solver.backward

    def spy(self, loss):
        seen.append(float(loss.detach()))
        return orig(self, loss)
    mod.Solver.backward = spy
    return seen, lambda: setattr(mod.Solver, 'backward', orig)


def test_train_resume_and_decode_with_the_embedding_plugin(tmp_path):
    main = importlib.import_module(PKG + '.main')
    plugin = importlib.import_module(PKG + '.src.plugin')
    tmp = str(tmp_path)
    root = os.path.join(tmp, 'corpus')
    vocab = _make_corpus(root)
    train, tr_path = _configs(root, vocab, tmp)
    train['hparas'].update(max_step=3, valid_step=3)
    emb = {'enable': True, 'src': _embedding_file(tmp), 'distance': 'CosEmb', 'weight': 0.5, 'fuse': 0.3,
           'temperature': 2, 'freeze': True, 'fuse_normalize': False, 'dropout': 0.0}
    train['emb'] = emb
    yaml.safe_dump(train, open(tr_path, 'w'))
    common = ['--logdir', os.path.join(tmp, 'log'), '--ckpdir', os.path.join(tmp, 'ckpt'),
              '--outdir', os.path.join(tmp, 'result'), '--njobs', '2', '--no-msg']

    # ---- three training steps with regulariser + fusion (validation with fusion at steps 1 and 3)
    train_mod = importlib.import_module(PKG + '.bin.train_asr')
    logged = []                                     # what the solver hands its logger, whichever backend writes it
    orig_log = train_mod.Solver.write_log

    def spy_log(self, name, d):
        logged.append((name, dict(d) if isinstance(d, dict) else d))
        return orig_log(self, name, d)
    train_mod.Solver.write_log = spy_log
    try:
        solver = main.main(['--config', tr_path] + common)
    finally:
        train_mod.Solver.write_log = orig_log
    assert solver.step >= 3 and solver.emb_reg and solver.emb_fuse
    assert type(solver.seq_loss).__name__ == 'NLLLoss'
    assert len(solver.optimizer.opt.param_groups) == 2
    latest = os.path.join(tmp, 'ckpt', 'asr_tiny_sd0', 'latest.pth')
    ck = torch.load(latest, map_location='cpu')
    assert set(ck.keys()) == {'model', 'optimizer', 'global_step', 'wer', 'emb_decoder'}
    assert list(ck['emb_decoder'].keys()) == ['fuse_lambda', 'temp', 'emb_table.weight', 'emb_net.0.weight',
                                              'emb_net.0.bias', 'emb_net.2.weight', 'emb_net.2.bias']
    assert all(torch.isfinite(v).all() for v in ck['emb_decoder'].values())
    assert all(torch.isfinite(v).all() for v in ck['model'].values())
    # the frozen table did not move and never got a gradient
    assert ck['emb_decoder']['emb_table.weight'].shape == (solver.vocab_size, EMB_DIM)
    assert torch.equal(ck['emb_decoder']['emb_table.weight'], solver.emb_decoder.emb_table.weight.cpu())
    assert 'emb_table.weight' not in [k for k, p in solver.emb_decoder.named_parameters() if p.grad is not None]
    # emb_loss and fuse_temp are logged with the training statistics (step 1), fuse_lambda only when it is learnable
    names = [n for n, _ in logged]
    assert 'emb_loss' in names and 'fuse_temp' in names and 'fuse_lambda' not in names
    emb_logged = [d for n, d in logged if n == 'emb_loss'][0]
    assert set(emb_logged) == {'tr'} and math.isfinite(float(emb_logged['tr'].detach())) and float(emb_logged['tr'].detach()) > 0
    assert float([d for n, d in logged if n == 'fuse_temp'][0]['temp']) == 2.0
    assert all(math.isfinite(float(v)) for n, d in logged if n == 'loss' for v in d.values() if v is not None)

    # ---- a resumed run loads the plug-in's entry (and the optimiser state of both parameter groups)
    loaded = []
    orig_load = plugin.EmbeddingRegularizer.load_state_dict

    def spy_load(self, sd, *a, **k):
        loaded.append(list(sd.keys()))
        return orig_load(self, sd, *a, **k)
    plugin.EmbeddingRegularizer.load_state_dict = spy_load
    try:
        train['hparas']['max_step'] = 4
        yaml.safe_dump(train, open(tr_path, 'w'))
        solver2 = main.main(['--config', tr_path, '--load', latest] + common)
        assert solver2.step >= 4 and loaded == [list(ck['emb_decoder'].keys())]

        # ---- the test solver decodes with fusion: greedy (per-step loop) and joint CTC-attention beam search
        calls = {'forward': 0, 'infer': 0}
        orig_fw, orig_inf = plugin.EmbeddingRegularizer.forward, plugin.EmbeddingRegularizer.infer

        def spy_fw(self, *a, **k):
            calls['forward'] += 1
            return orig_fw(self, *a, **k)

        def spy_inf(self, *a, **k):
            calls['infer'] += 1
            return orig_inf(self, *a, **k)
        plugin.EmbeddingRegularizer.forward, plugin.EmbeddingRegularizer.infer = spy_fw, spy_inf
        try:
            for name, kw in (('dec_greedy', dict(beam_size=1, min_len_ratio=0.01, max_len_ratio=0.3)),
                             ('dec_beam', dict(beam_size=2, min_len_ratio=0.01, max_len_ratio=0.1, lm_path='',
                                               lm_config='', lm_weight=0.0, ctc_weight=0.3))):
                p = _decode_cfg(tmp, tr_path, latest, name, **kw)
                cfg = yaml.safe_load(open(p))
                cfg['emb'] = emb
                yaml.safe_dump(cfg, open(p, 'w'))
                tester = main.main(['--config', p, '--test'] + common)
                assert tester.emb_decoder is not None and not tester.emb_decoder.training
                assert len(loaded) == (2 if name == 'dec_greedy' else 3)
            assert calls['forward'] > 0 and calls['infer'] > 0
        finally:
            plugin.EmbeddingRegularizer.forward, plugin.EmbeddingRegularizer.infer = orig_fw, orig_inf
    finally:
        plugin.EmbeddingRegularizer.load_state_dict = orig_load
    for s, n in (('dev', 3), ('test', 2)):
        lines = open(os.path.join(tmp, 'result', 'dec_greedy_%s_output.csv' % s)).read().splitlines()
        assert lines[0] == 'idx\thyp\ttruth' and len(lines) == n + 1
    out = open(os.path.join(tmp, 'result', 'dec_beam_test_output.csv')).read().splitlines()
    beams = open(os.path.join(tmp, 'result', 'dec_beam_test_beam-2-0.0.csv')).read().splitlines()
    assert len(out) == 3 and beams[0] == 'idx\tbeam\thyp\ttruth' and len(beams) >= 3


def test_without_the_emb_block_nothing_of_the_plugin_runs(tmp_path):
    """no `emb:` block, or one with enable: false: the solver takes the path it took before the plug-in existed - the
    plug-in is never constructed, the first step's loss is the same number, the checkpoint has no plug-in entry"""
    main = importlib.import_module(PKG + '.main')
    plugin = importlib.import_module(PKG + '.src.plugin')
    mod = importlib.import_module(PKG + '.bin.train_asr')

    class Refuse:
        def __init__(self, *a, **k):
            raise AssertionError('the plug-in was constructed')
    orig_cls = plugin.EmbeddingRegularizer
    plugin.EmbeddingRegularizer = Refuse
    first = {}
    try:
        for tag, block in (('plain', None), ('disabled', {'enable': False})):
            tmp = str(tmp_path / tag)
            os.makedirs(tmp)
            root = os.path.join(tmp, 'corpus')
            vocab = _make_corpus(root)
            train, tr_path = _configs(root, vocab, tmp)
            train['hparas'].update(max_step=3, valid_step=3)
            if block is not None:
                train['emb'] = block
            yaml.safe_dump(train, open(tr_path, 'w'))
            seen, restore = _spy_first_loss(mod)
            try:
                solver = main.main(['--config', tr_path, '--logdir', os.path.join(tmp, 'log'), '--ckpdir',
                                    os.path.join(tmp, 'ckpt'), '--njobs', '2', '--no-msg'])
            finally:
                restore()
            assert solver.emb_decoder is None and not solver.emb_reg and not solver.emb_fuse
            assert type(solver.seq_loss).__name__ == 'CrossEntropyLoss'
            ck = torch.load(os.path.join(tmp, 'ckpt', 'asr_tiny_sd0', 'latest.pth'), map_location='cpu')
            assert set(ck.keys()) == {'model', 'optimizer', 'global_step', 'wer'}
            first[tag] = seen[0]
    finally:
        plugin.EmbeddingRegularizer = orig_cls
    # the same number up to the order in which the existing loss kernels' float atomics land (a few ulp)
    assert math.isfinite(first['plain']) and abs(first['plain'] - first['disabled']) <= 1e-5 * abs(first['plain'])


def test_without_the_emb_block_the_first_step_is_the_parent_commits(tmp_path):
    """tests/golden/emb_noemb_first_loss.json holds the loss the first training step back-propagates on the commit
    BEFORE the plug-in (tests/emb_plugin_noemb_worker.py run there under ASRK_DETERMINISTIC=1: fixed-order sums, so the
    number has no run-to-run noise).  The same worker on this tree gives the same float, bit for bit."""
    here = os.path.dirname(os.path.abspath(__file__))
    rec = json.load(open(os.path.join(here, 'golden', 'emb_noemb_first_loss.json')))
    r = subprocess.run([sys.executable, os.path.join(here, 'emb_plugin_noemb_worker.py'), str(tmp_path)],
                       capture_output=True, text=True, env=dict(os.environ, ASRK_DETERMINISTIC='1'), timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith('FIRST_LOSS ')][-1]
    got = json.loads(line[len('FIRST_LOSS '):])
    print('first-step loss', got, 'recorded', rec['first_step_loss_hex'])
    assert got['first_step_loss_hex'] == rec['first_step_loss_hex']
