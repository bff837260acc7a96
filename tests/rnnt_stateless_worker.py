"""Worker of tests/test_rnnt_stateless_model_gpu.py::test_solver_and_decode_pass (a subprocess, so that
ASRK_DETERMINISTIC is read by a fresh library): the product solver of tests/rnnt_worker.py on the miniature wav corpus
for two steps with `pred: {module: stateless, dim: 12, context: 2}` and the `prune:` block, then `main.py --test` on its
best_rnnt.pth with `decode: {transducer: {enable: true, beam_size: 4, nbest: 3}}`.  Writes one JSON record: the training
run's log entries and head keys, the decode run's files (prefix replaced by {}) and their lines."""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rnnt_worker as RW            # noqa: E402  (the training run)
import test_e2e_gpu as E2E          # noqa: E402  (corpus and config helpers)

HEAD = {'enable': True, 'weight': 0.3, 'joint_dim': 16, 'pred': {'module': 'stateless', 'dim': 12, 'context': 2},
        'prune': {'enable': True, 'range': 3, 'simple_weight': 0.25}}


def main():
    out_path = sys.argv[1]
    tmp = os.path.join(os.path.dirname(os.path.abspath(out_path)), 'work')
    root = os.path.join(tmp, 'corpus')
    os.makedirs(root)
    vocab = E2E._make_corpus(root)
    cfg, _ = E2E._configs(root, vocab, tmp)
    cfg['hparas'].update(max_step=2, valid_step=2)
    cfg['model']['transducer'] = dict(HEAD)
    seen = RW.run('on', cfg, tmp)
    best = os.path.join(seen['ckpdir'], 'best_rnnt.pth')

    main_mod = importlib.import_module(RW.PKG + '.main')
    result = os.path.join(tmp, 'result')
    common = ['--logdir', os.path.join(tmp, 'log'), '--ckpdir', os.path.join(tmp, 'ckpt'), '--outdir', result,
              '--njobs', '1', '--no-msg']
    dcfg = E2E._decode_cfg(tmp, os.path.join(tmp, 'on.yaml'), best, 'dec_beam', beam_size=4, max_len_ratio=0.3,
                           min_len_ratio=0.01, transducer={'enable': True, 'max_symbols': 2, 'max_len_ratio': 0.4,
                                                           'beam_size': 4, 'nbest': 3})
    main_mod.main(['--config', dcfg, '--test'] + common)
    files = sorted(f for f in os.listdir(result) if f.startswith('dec_beam_'))
    res = {'train': {k: seen[k] for k in ('rnnt_logs', 'dv_rnnt', 'head_keys', 'head_moved', 'params_finite', 'msgs',
                                          'ckpts', 'grad_norm')},
           'decode': {'files': ['{}' + f[len('dec_beam'):] for f in files],
                      'texts': [open(os.path.join(result, f), encoding='UTF-8').read().splitlines() for f in files]}}
    with open(out_path, 'w') as f:
        json.dump(res, f)
    print('DONE', flush=True)


if __name__ == '__main__':
    main()
