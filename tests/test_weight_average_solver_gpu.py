"""GPU: the weight average (src/optim.py WeightAverage) through the solvers - swapped into the live model around validation and
back bit for bit, saved beside the live weights and restored on resume, every cache of derived weights dropped on the way
(the bf16 split panels of decoder_ops.weight_panel are keyed by data_ptr and _version, and a raw write changes neither), and
the whole of it through main.py: training with AdamW, weight decay and the average on, decoding with the averaged and with
the live weights."""
import importlib
import os

import numpy as np
import pytest
import torch
import yaml

from conftest import PKG_NAME
from test_e2e_gpu import _configs, _decode_cfg, _make_corpus

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _mod(name):
    return importlib.import_module(PKG_NAME + "." + name)


def same_bits(a, b):
    return torch.equal(a.detach().cpu().contiguous().view(torch.int32), b.detach().cpu().contiguous().view(torch.int32))


def _solver(tmp, hparas, load='', seed=0):
    """a BaseSolver around a Linear(6, 3), as tests/test_optim_gpu.py builds it, with what save_checkpoint / load_ckpt read"""
    solver_mod, optim, util = _mod("src.solver"), _mod("src.optim"), _mod("src.util")

    class Paras:
        verbose = True
    s = object.__new__(solver_mod.BaseSolver)
    s.paras, s.rank, s.world, s.dist, s.dp, s.step = Paras(), 0, 1, None, None, 0
    s.paras.load = load
    s.GRAD_CLIP, s.timer = 5.0, util.Timer()
    s.msgs = []
    s.verbose = lambda m: s.msgs.append(m)
    s.mode, s.ckpdir, s.emb_decoder, s.device = 'train', str(tmp), None, torch.device(DEV)
    torch.manual_seed(seed)
    s.model = torch.nn.Linear(6, 3).to(DEV)
    s.optimizer = optim.Optimizer(s.model.parameters(), **hparas)
    return s


def _train(s, steps):
    for _ in range(steps):
        g = torch.Generator().manual_seed(100 + s.step)
        x = torch.randn(4, 6, generator=g).to(DEV)
        s.optimizer.pre_step(s.step)
        s.backward(s.model(x).pow(2).mean())
        s.step += 1


HP = dict(optimizer='Adadelta', lr=1.0, eps=1e-8, lr_scheduler='fixed', weight_decay=0.01,
          average=dict(enable=True, mode='ema', decay=0.5, warmup=False))


def test_swap_and_restore_around_validation(ops, tmp_path):
    """five steps with averaging on: inside applied() the module computes what a fresh module loaded from the model_avg it
    would save computes, the checkpoint is the same from inside and from outside, and afterwards the live weights are their
    snapshot bit for bit - also when the body raises"""
    s = _solver(tmp_path, HP)
    assert s.optimizer.fused and s.optimizer.device_nan_skip
    _train(s, 5)
    avg = s.optimizer.average
    assert avg.k == 5
    live = [p.detach().clone() for p in s.model.parameters()]
    x = torch.randn(7, 6, device=DEV)
    y_live = s.model(x).detach().clone()
    s.save_checkpoint('outside.pth', 'wer', 1.0, show_msg=False)
    with s.averaged_weights():
        assert avg.swapped
        y_in = s.model(x).detach().clone()
        s.save_checkpoint('inside.pth', 'wer', 1.0, show_msg=False)
    out, ins = (torch.load(os.path.join(str(tmp_path), f), map_location=DEV) for f in ('outside.pth', 'inside.pth'))
    assert set(out) == {'model', 'model_avg', 'average', 'optimizer', 'global_step', 'wer'}
    assert out['average'] == {'k': 5, 'mode': 'ema'} == ins['average']
    for key in ('model', 'model_avg'):
        assert all(same_bits(out[key][k], ins[key][k]) for k in out[key]), key
    assert all(same_bits(out['model'][k], p) for k, p in s.model.named_parameters())
    assert not any(same_bits(out['model'][k], out['model_avg'][k]) for k in out['model'])
    fresh = torch.nn.Linear(6, 3).to(DEV)
    fresh.load_state_dict(out['model_avg'])
    assert same_bits(fresh(x), y_in) and not same_bits(y_in, y_live)
    assert all(same_bits(p, l) for p, l in zip(s.model.parameters(), live)) and same_bits(s.model(x), y_live)
    with pytest.raises(ZeroDivisionError):
        with s.averaged_weights():
            1 / 0
    assert not avg.swapped and all(same_bits(p, l) for p, l in zip(s.model.parameters(), live))
    ops.check_errors()


@pytest.mark.parametrize("mode", ['ema', 'mean'])
def test_resume_is_exact(ops, tmp_path, mode):
    """save at step 3, load into a fresh solver, two more steps: weights, optimiser state, average and k of an uninterrupted
    five-step run, bit for bit; a checkpoint without the average starts a fresh one and says so"""
    hp = dict(HP, average=dict(HP['average'], mode=mode))
    whole = _solver(tmp_path, hp)
    _train(whole, 5)
    first = _solver(tmp_path, hp)
    _train(first, 3)
    first.save_checkpoint('step3.pth', 'wer', 1.0, show_msg=False)
    second = _solver(tmp_path, hp, load=os.path.join(str(tmp_path), 'step3.pth'), seed=99)
    second.load_ckpt()
    assert second.step == 3 and second.optimizer.average.k == 3
    _train(second, 2)
    ops.check_errors()
    for a, b in zip(whole.model.parameters(), second.model.parameters()):
        assert same_bits(a, b)
    sa, sb = whole.optimizer.opt.state_dict()['state'], second.optimizer.opt.state_dict()['state']
    assert sa.keys() == sb.keys()
    for i in sa:
        for k in sa[i]:
            assert same_bits(sa[i][k].float(), sb[i][k].float()), (i, k)
    wa, wb = whole.optimizer.average, second.optimizer.average
    assert wa.k == wb.k == 5
    assert all(same_bits(a, b) for a, b in zip(wa.tensors[0], wb.tensors[0]))
    assert not any(same_bits(e, p) for e, p in zip(wa.tensors[0], whole.model.parameters()))
    # a checkpoint from before this change (no averaged weights), under a config with averaging on
    ck = torch.load(os.path.join(str(tmp_path), 'step3.pth'), map_location=DEV)
    old = {k: v for k, v in ck.items() if k not in ('model_avg', 'average')}
    torch.save(old, os.path.join(str(tmp_path), 'old.pth'))
    third = _solver(tmp_path, hp, load=os.path.join(str(tmp_path), 'old.pth'), seed=98)
    third.load_ckpt()
    assert any('average starts afresh' in m for m in third.msgs) and not third.optimizer.average.started()
    _train(third, 1)
    assert third.optimizer.average.k == 1


# ====================================================================================================== stale caches
def _transducer_asr(seed):
    """the smallest model decoder_ops.weight_panel caches for: the prediction network's LSTM cell takes the panel GEMMs from
    128 rows on with widths that are multiples of 32 (decoder_ops.lstm_cell_infer), and the greedy transducer search steps
    one row per utterance"""
    torch.manual_seed(seed)
    head = {'enable': True, 'weight': 0.3, 'joint_dim': 16,
            'pred': {'module': 'LSTM', 'dim': 32, 'layer': 1, 'emb_dim': 32, 'dropout': 0}}
    enc = dict(prenet='', module='LSTM', bidirection=True, dim=[16, 16], dropout=[0, 0], layer_norm=[False, False],
               proj=[True, True], sample_rate=[2, 1], sample_style='drop')
    return _mod("src.asr").ASR(8, 11, True, 1.0, enc, None, None, transducer=head).to(DEV)


def test_no_stale_weight_panels_across_the_swap(ops):
    """decode with the live weights, inside applied(), live again: the middle result is that of a fresh model loaded with the
    averaged state dict, the outer two are equal.  The search does not drop the panel cache itself, so without the
    drop_weight_panels() of WeightAverage.swap the middle decode multiplies by the live weights' panels"""
    dops, optim = _mod("decoder_ops"), _mod("src.optim")
    model = _transducer_asr(0)
    o = optim.Optimizer(model.parameters(), 'Adam', 0.05, 1e-8, 'fixed',
                        average=dict(enable=True, mode='ema', decay=0.5, warmup=False))
    g = torch.Generator().manual_seed(1)
    for step in range(3):                                             # weights that are far from their average
        o.pre_step(step)
        for p in model.parameters():
            p.grad = torch.randn(*p.shape, generator=g).to(DEV)
        o.step()
    model.eval()
    rows = dops.LSTM_CELL_GEMM_ROWS
    feat = torch.randn(rows, 12, 8, generator=g).to(DEV)
    flen = torch.full((rows,), 12, dtype=torch.int64, device=DEV)

    def decode(m):
        tok, n, _ = m.transducer_greedy(feat, flen, max_symbols=2, max_len_ratio=0.7)
        ops.check_errors()
        return tok.cpu().numpy().copy(), n.cpu().numpy().copy()

    def same(a, b):
        return np.array_equal(a[1], b[1]) and all(np.array_equal(x[:k], y[:k]) for x, y, k in zip(a[0], b[0], a[1]))
    assert not dops._weight_panels                                    # the optimiser step dropped them
    live = decode(model)
    assert dops._weight_panels, "this shape was chosen to take the cached-panel route"
    avg = o.average
    fresh = _transducer_asr(5).eval()
    fresh.load_state_dict(avg.averaged_state_dict(model))
    with avg.applied():
        inside = decode(model)
    again = decode(model)
    want = decode(fresh)
    assert live[1].sum() > 0 and want[1].sum() > 0                     # real hypotheses
    assert not same(live, want), "the live and the averaged weights decode alike: the test would show nothing"
    assert same(inside, want)
    assert same(again, live)


# ====================================================================================================== through main.py
def test_train_and_decode_through_main(tmp_path):
    """one pass on the tiny corpus of tests/test_e2e_gpu.py: AdamW with weight decay and the average on; the checkpoint holds
    the live and the averaged weights; --test decodes with model_avg, with `decode: {averaged: false}` with model - each
    compared with decoding a checkpoint that holds that state dict alone (the layout from before this change)"""
    main = _mod('main')
    tmp = str(tmp_path)
    root = os.path.join(tmp, 'corpus')
    vocab = _make_corpus(root)
    train, tr_path = _configs(root, vocab, tmp)
    train['hparas'].update(optimizer='AdamW', lr=0.01, weight_decay=0.01, valid_step=3, max_step=6,
                           average={'enable': True, 'mode': 'ema', 'decay': 0.5, 'warmup': False})
    yaml.safe_dump(train, open(tr_path, 'w'))
    common = ['--logdir', os.path.join(tmp, 'log'), '--ckpdir', os.path.join(tmp, 'ckpt'),
              '--outdir', os.path.join(tmp, 'result'), '--njobs', '2', '--no-msg']
    solver = main.main(['--config', tr_path] + common)
    fo = _mod('fused_optim')
    assert solver.optimizer.fused and isinstance(solver.optimizer.opt, fo.FusedAdamW)
    g0 = solver.optimizer.opt.param_groups[0]
    assert g0['weight_decay'] == 0.01 and g0['decay_min_dim'] == 2 and solver.optimizer.average.k == solver.step
    latest = os.path.join(tmp, 'ckpt', 'asr_tiny_sd0', 'latest.pth')
    ck = torch.load(latest, map_location='cpu')
    assert set(ck) == {'model', 'model_avg', 'average', 'optimizer', 'global_step', 'wer'}
    assert ck['average'] == {'k': 6, 'mode': 'ema'} and ck['global_step'] == 6
    assert ck['model'].keys() == ck['model_avg'].keys()
    differ = [k for k in ck['model'] if ck['model'][k].is_floating_point() and not torch.equal(ck['model'][k], ck['model_avg'][k])]
    assert len(differ) == len(list(solver.model.parameters()))
    alone = {}
    for key in ('model', 'model_avg'):                                # the old layout, one state dict each
        alone[key] = os.path.join(tmp, key + '_alone.pth')
        torch.save({'model': ck[key], 'optimizer': ck['optimizer'], 'global_step': 6, 'wer': ck['wer']}, alone[key])

    def decode(name, ckpt, **extra):
        cfg = _decode_cfg(tmp, tr_path, ckpt, name, beam_size=2, min_len_ratio=0.01, max_len_ratio=0.1, lm_path='',
                          lm_config='', lm_weight=0.0, ctc_weight=0.3, **extra)
        main.main(['--config', cfg, '--test'] + common)
        return open(os.path.join(tmp, 'result', '%s_test_beam-2-0.0.csv' % name)).read()
    averaged, live = decode('dec_avg', latest), decode('dec_live', latest, averaged=False)
    assert averaged == decode('dec_avg_alone', alone['model_avg'])
    assert live == decode('dec_live_alone', alone['model'])
    assert live == decode('dec_live_alone_flag', alone['model'], averaged=False)
