"""Worker of tests/test_rnnt_beam_gpu.py::test_decode_pass_with_the_beam_block (a subprocess, so that ASRK_DETERMINISTIC
is read by a fresh library): trains the tiny transducer model of tests/rnnt_worker.py for two steps, then runs
`main.py --test` on its best_rnnt.pth four times - greedy (no beam key), `beam_size: 1`, `beam_size: 4, nbest: 3`, and
`beam_size: 2, nbest: 2, lm_weight: 0.3` with a small ARPA file - and once with an RNN-LM path, which must be refused.
Writes one JSON record: per run the files (prefix replaced by {}) and their lines."""
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rnnt_worker as RW            # noqa: E402  (the training run)
import test_e2e_gpu as E2E          # noqa: E402  (corpus and config helpers)


def write_arpa(path, V):
    """unigrams for every token (words are token ids; 0, 1, 2 by their names) and a few bigrams"""
    names = {0: '<s>', 1: '</s>', 2: '<unk>'}
    uni = ['%.4f\t%s\t-0.3' % (-1.0 - 0.05 * (w % 7), names.get(w, str(w))) for w in range(V)]
    bi = ['%.4f\t%s %s' % (-0.4 - 0.1 * (w % 3), names.get(w, str(w)), names.get(w + 1, str(w + 1)))
          for w in range(0, V - 1, 2) if w + 1 != 0]
    with open(path, 'w') as f:
        f.write('\\data\\\nngram 1=%d\nngram 2=%d\n\n\\1-grams:\n%s\n\n\\2-grams:\n%s\n\n\\end\\\n'
                % (len(uni), len(bi), '\n'.join(uni), '\n'.join(bi)))


def main():
    out_path = sys.argv[1]
    tmp = os.path.join(os.path.dirname(os.path.abspath(out_path)), 'work')
    root = os.path.join(tmp, 'corpus')
    os.makedirs(root)
    vocab = E2E._make_corpus(root)
    cfg, _ = E2E._configs(root, vocab, tmp)
    cfg['hparas'].update(max_step=2, valid_step=2)
    cfg['model']['transducer'] = dict(RW.HEAD)
    seen = RW.run('on', cfg, tmp)
    best = os.path.join(seen['ckpdir'], 'best_rnnt.pth')
    V = torch.load(best, map_location='cpu')['model']['ctc_layer.weight'].shape[0]
    arpa = os.path.join(tmp, 'tiny.arpa')
    write_arpa(arpa, V)

    main_mod = importlib.import_module(RW.PKG + '.main')
    result = os.path.join(tmp, 'result')
    common = ['--logdir', os.path.join(tmp, 'log'), '--ckpdir', os.path.join(tmp, 'ckpt'), '--outdir', result,
              '--njobs', '1', '--no-msg']
    base = {'enable': True, 'max_symbols': 2, 'max_len_ratio': 0.4}

    def decode(name, block, **extra):
        dcfg = E2E._decode_cfg(tmp, os.path.join(tmp, 'on.yaml'), best, name, beam_size=4, max_len_ratio=0.3,
                               min_len_ratio=0.01, transducer=block, **extra)
        main_mod.main(['--config', dcfg, '--test'] + common)
        files = sorted(f for f in os.listdir(result) if f.startswith(name + '_'))
        return {'files': ['{}' + f[len(name):] for f in files],
                'texts': [open(os.path.join(result, f), encoding='UTF-8').read().splitlines() for f in files]}

    res = {'greedy': decode('dec_greedy', dict(base)),
           'one': decode('dec_one', dict(base, beam_size=1)),
           'beam': decode('dec_beam', dict(base, beam_size=4, nbest=3)),
           'lm': decode('dec_lm', dict(base, beam_size=2, nbest=2, lm_weight=0.3), lm_path=arpa)}
    try:
        decode('dec_bad', dict(base, beam_size=2, lm_weight=0.3), lm_path=os.path.join(tmp, 'rnnlm.pth'))
        res['rnnlm_error'] = ''
    except ValueError as e:
        res['rnnlm_error'] = str(e)
    with open(out_path, 'w') as f:
        json.dump(res, f)
    print('DONE', flush=True)


if __name__ == '__main__':
    main()
