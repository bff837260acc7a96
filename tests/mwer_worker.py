"""Worker of tests/test_mwer_gpu.py::test_solver_with_and_without_the_block (a subprocess, so that ASRK_DETERMINISTIC is
read by a fresh library): the product solver (bin/train_asr.py) on the miniature wav corpus of tests/specaug_worker.py,
four times with the same seed - without a `mwer:` block, with `enable: false`, with a start_step the run never reaches,
and with start_step 1.  Writes one JSON record per run: the loss of every step (the float32 bits), a SHA-1 over the
parameters after the run, the `mwer` log entries, the gradient norms and the number of searches."""
import hashlib
import importlib
import json
import os
import sys

import numpy as np
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "end-to-end-asr-pytorch_amd"
import specaug_worker as SW          # noqa: E402  (corpus and config helpers)

SEED = 5
MWER = {'enable': True, 'nbest': 3, 'beam_size': 4, 'ce_weight': 0.1, 'unit': 'word', 'ctc_weight': 0.2,
        'min_len_ratio': 0.01, 'max_len_ratio': 0.1, 'start_step': 1}


def run(name, cfg, tmp):
    main_mod = importlib.import_module(PKG + '.main')
    train_asr = importlib.import_module(PKG + '.bin.train_asr')
    cfg_path = os.path.join(tmp, name + '.yaml')
    yaml.safe_dump(cfg, open(cfg_path, 'w'))
    paras = main_mod.build_parser().parse_args(['--config', cfg_path, '--logdir', os.path.join(tmp, 'log'),
                                                '--ckpdir', os.path.join(tmp, 'ckpt'), '--njobs', '1', '--no-msg',
                                                '--seed', str(SEED)])
    paras.gpu, paras.pin_memory, paras.verbose = True, True, False
    np.random.seed(SEED)
    torch.manual_seed(SEED)
    torch.cuda.manual_seed_all(SEED)
    solver = train_asr.Solver(cfg, paras, 'train')
    solver.PROGRESS_STEP = 1             # every step logs (the three steps of a run would otherwise log only the first)
    seen = {'loss_hex': [], 'grad_norm': [], 'mwer_logs': [], 'msgs': [], 'searches': 0}
    verbose = solver.verbose

    def spy_verbose(msg):
        seen['msgs'] += [str(m) for m in (msg if isinstance(msg, list) else [msg])]
        return verbose(msg)
    solver.verbose = spy_verbose
    solver.load_data()
    solver.set_model()
    backward, write_log = solver.backward, solver.write_log

    def spy_backward(loss):
        seen['loss_hex'].append(loss.detach().cpu().numpy().astype(np.float32).tobytes().hex())
        norm = backward(loss)
        seen['grad_norm'].append(float(norm))
        return norm

    def spy_log(log_name, d):
        if log_name == 'mwer':
            seen['mwer_logs'].append({k: float(v) for k, v in d.items()})
        return write_log(log_name, d)
    solver.backward, solver.write_log = spy_backward, spy_log
    if solver.mwer is not None:
        search = solver.mwer.search

        def spy_search(feat, feat_len):
            seen['searches'] += 1
            assert solver.model.training
            out = search(feat, feat_len)
            assert solver.model.training
            return out
        solver.mwer.search = spy_search
    solver.exec()
    torch.cuda.synchronize()
    h = hashlib.sha1()
    for p in solver.model.parameters():
        h.update(p.detach().cpu().numpy().tobytes())
    seen.update(param_sha1=h.hexdigest(), has_search=solver.mwer is not None,
                params_finite=all(bool(torch.isfinite(p).all()) for p in solver.model.parameters()))
    print('RUN', name, json.dumps(seen)[:1500], flush=True)
    return seen


def main():
    out_path = sys.argv[1]
    tmp = os.path.join(os.path.dirname(os.path.abspath(out_path)), 'work')
    root = os.path.join(tmp, 'corpus')
    os.makedirs(root)
    vocab = SW._make_corpus(root)

    def cfg(**mwer):
        c = SW._config(root, vocab)
        c['hparas']['max_step'] = 2
        if mwer:
            c['mwer'] = dict(MWER, **mwer)
        return c
    res = {'plain': run('plain', cfg(), tmp),
           'off': run('off', cfg(enable=False), tmp),
           'late': run('late', cfg(start_step=1000), tmp),
           'on': run('on', cfg(start_step=1), tmp)}
    with open(out_path, 'w') as f:
        json.dump(res, f)
    print('DONE', flush=True)


if __name__ == '__main__':
    main()
