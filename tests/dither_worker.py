"""Worker of tests/test_dither_gpu.py::test_solver_trains_with_dither (a subprocess, so that ASRK_DETERMINISTIC is read
by a fresh library): the product solver (bin/train_asr.py) on the miniature wav corpus of tests/speed_perturb_worker.py
with the same seed - twice with `dither: 3.05e-5` (three steps and more, several validation passes), once with
`dither: 0`, and once with `dither: 0` on a solver whose load_dataset is called WITHOUT the dither keyword (the data path
as it was before the feature).  Each run writes <out>/<name>.npz: the features that entered model.forward (training steps and validation
passes apart), their lengths, the utterance names of every training batch and the loss of every step."""
import importlib
import os
import sys

import numpy as np
import torch
import yaml

import speed_perturb_worker as SW

PKG, SEED = SW.PKG, SW.SEED
DITHER = 3.05e-5


def run(name, cfg, tmp, out, without_keyword=False):
    main_mod = importlib.import_module(PKG + '.main')
    train_asr = importlib.import_module(PKG + '.bin.train_asr')
    data_mod = importlib.import_module(PKG + '.src.data')
    cfg_path = os.path.join(tmp, name + '.yaml')
    yaml.safe_dump(cfg, open(cfg_path, 'w'))
    paras = main_mod.build_parser().parse_args(['--config', cfg_path, '--logdir', os.path.join(tmp, 'log'),
                                                '--ckpdir', os.path.join(tmp, 'ckpt'), '--njobs', '1', '--no-msg',
                                                '--seed', str(SEED)])
    paras.gpu, paras.pin_memory, paras.verbose = True, True, False
    np.random.seed(SEED)
    torch.manual_seed(SEED)
    torch.cuda.manual_seed_all(SEED)
    if without_keyword:
        # the data path of a solver that never heard of the feature: load_dataset as it was called before it
        def plain_load_dataset(*args, dither=None, **kwargs):
            assert dither is None
            return data_mod.load_dataset(*args, **kwargs)
        train_asr.load_dataset = plain_load_dataset
    try:
        solver = train_asr.Solver(cfg, paras, 'train')
        solver.load_data()
    finally:
        train_asr.load_dataset = data_mod.load_dataset
    assert (solver.dither is None) == (cfg['data']['audio']['dither'] == 0)
    solver.set_model()
    seen = {'train': [], 'valid': [], 'loss': [], 'names': []}

    def pre_hook(module, args):
        feat, feat_len = args[0], args[1]
        seen['train' if module.training else 'valid'].append((feat.detach().cpu().numpy().copy(),
                                                              feat_len.detach().cpu().numpy().copy()))
    solver.model.register_forward_pre_hook(pre_hook)
    backward, fetch = solver.backward, solver.fetch_data

    def spy(loss):
        seen['loss'].append(loss.detach().cpu().numpy().astype(np.float32).reshape(()))
        return backward(loss)

    def fetch_spy(data):
        if solver.model.training:
            seen['names'].append(list(data[0]))
        return fetch(data)
    solver.backward, solver.fetch_data = spy, fetch_spy
    solver.exec()
    arrays = {'loss': np.stack(seen['loss']), 'n_valid': np.int64(len(seen['valid'])), 'seed': np.int64(SEED),
              'n_train': np.int64(len(seen['train'])), 'n_dev_batches': np.int64(len(solver.dv_set)),
              'dither': np.float64(cfg['data']['audio']['dither'])}
    for k, (f, l) in enumerate(seen['train']):
        arrays['train_feat_%d' % k], arrays['train_len_%d' % k] = f, l
        arrays['train_names_%d' % k] = np.asarray(seen['names'][k])
    for k, (f, l) in enumerate(seen['valid']):
        arrays['valid_feat_%d' % k], arrays['valid_len_%d' % k] = f, l
    np.savez(os.path.join(out, name + '.npz'), **arrays)
    print('RUN', name, 'steps', len(seen['train']), 'valid', len(seen['valid']), 'loss', [float(v) for v in seen['loss']],
          flush=True)


def _config(root, vocab, max_step, dither):
    cfg = SW._config(root, vocab, max_step)
    cfg['data']['audio']['dither'] = dither
    cfg['hparas']['valid_step'] = 2              # validation after steps 1 and 2: at least two passes
    return cfg


def main():
    out = sys.argv[1]
    tmp = os.path.join(out, 'work')
    root = os.path.join(tmp, 'corpus')
    os.makedirs(root)
    vocab, _ = SW._make_corpus(root)
    for name in ('dither_a', 'dither_b'):
        run(name, _config(root, vocab, 3, DITHER), tmp, out)
    run('plain', _config(root, vocab, 1, 0), tmp, out)
    run('never', _config(root, vocab, 1, 0), tmp, out, without_keyword=True)


if __name__ == '__main__':
    main()
