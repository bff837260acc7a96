"""Worker of tests/test_bias_decode_gpu.py::test_decode_pass_with_the_bias_block (a subprocess, as
tests/rnnt_beam_worker.py is): trains the tiny transducer model of tests/rnnt_worker.py for two steps, then runs
`main.py --test` on its best_rnnt.pth with a `decode.bias` block in each decode mode - the joint CTC-attention search,
the CTC prefix search, the transducer search at `beam_size: 1` (which the block turns into the beam search) and the
transducer beam search with the n-gram LM - and once greedy, which must be refused.  Writes one JSON record: per run
the files (prefix replaced by {}) and their lines."""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rnnt_beam_worker as BW       # noqa: E402  (the ARPA file)
import rnnt_worker as RW            # noqa: E402  (the training run)
import test_e2e_gpu as E2E          # noqa: E402  (corpus and config helpers)


def main():
    import torch
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
    BW.write_arpa(arpa, V)
    phrases = os.path.join(tmp, 'phrases.txt')
    with open(phrases, 'w', encoding='utf-8') as f:
        f.write('# names\n%s\n%s %s\t2.0\n\n' % (E2E.WORDS[0], E2E.WORDS[1], E2E.WORDS[2]))
    bias = {'path': phrases, 'weight': 1.5}

    main_mod = importlib.import_module(RW.PKG + '.main')
    result = os.path.join(tmp, 'result')
    common = ['--logdir', os.path.join(tmp, 'log'), '--ckpdir', os.path.join(tmp, 'ckpt'), '--outdir', result,
              '--njobs', '1', '--no-msg']
    base = {'enable': True, 'max_symbols': 2, 'max_len_ratio': 0.4}

    def decode(name, **dcfg):
        dcfg.setdefault('beam_size', 2)
        path = E2E._decode_cfg(tmp, os.path.join(tmp, 'on.yaml'), best, name, max_len_ratio=0.3, min_len_ratio=0.01,
                               **dcfg)
        main_mod.main(['--config', path, '--test'] + common)
        files = sorted(f for f in os.listdir(result) if f.startswith(name + '_'))
        return {'files': ['{}' + f[len(name):] for f in files],
                'texts': [open(os.path.join(result, f), encoding='UTF-8').read().splitlines() for f in files]}

    res = {'plain': decode('b_plain', ctc_weight=0.3),
           'joint': decode('b_joint', ctc_weight=0.3, bias=dict(bias)),
           'ctc': decode('b_ctc', ctc_weight=1.0, vocab_candidate=5, bias=dict(bias)),
           'rnnt_one': decode('b_rnnt1', transducer=dict(base, beam_size=1), bias=dict(bias)),
           'rnnt_lm': decode('b_rnntlm', transducer=dict(base, beam_size=2, nbest=2, lm_weight=0.3), lm_path=arpa,
                             bias=dict(bias))}
    try:
        decode('b_bad', beam_size=1, bias=dict(bias))
        res['greedy_error'] = ''
    except ValueError as e:
        res['greedy_error'] = str(e)
    with open(out_path, 'w') as f:
        json.dump(res, f)
    print('DONE', flush=True)


if __name__ == '__main__':
    main()
