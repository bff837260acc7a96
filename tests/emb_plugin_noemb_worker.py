"""Worker of tests/test_emb_plugin_e2e_gpu.py (a subprocess, so that ASRK_DETERMINISTIC=1 is read by a fresh library):
one training step through `main.py` on the synthetic corpus of tests/test_e2e_gpu.py WITHOUT an `emb:` block; prints
the loss that step back-propagates as a float's hex string.  It uses nothing the plug-in added, so the same file runs on
the commit before the plug-in: that is where tests/golden/emb_noemb_first_loss.json was recorded."""
import importlib
import json
import os
import sys

import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_e2e_gpu import PKG, _make_corpus, _configs          # noqa: E402

tmp = sys.argv[1]
main = importlib.import_module(PKG + '.main')
mod = importlib.import_module(PKG + '.bin.train_asr')
root = os.path.join(tmp, 'corpus')
vocab = _make_corpus(root)
train, tr_path = _configs(root, vocab, tmp)
train['hparas'].update(max_step=1, valid_step=1000)
yaml.safe_dump(train, open(tr_path, 'w'))
seen = []
orig = mod.Solver.backward


def spy(self, loss):
    seen.append(float(loss.detach()))
    return orig(self, loss)


mod.Solver.backward = spy
main.main(['--config', tr_path, '--logdir', os.path.join(tmp, 'log'), '--ckpdir', os.path.join(tmp, 'ckpt'),
           '--njobs', '2', '--no-msg'])
print("FIRST_LOSS " + json.dumps({"first_step_loss_hex": seen[0].hex(), "first_step_loss": seen[0]}))
