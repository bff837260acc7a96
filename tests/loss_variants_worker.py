"""Worker of tests/test_loss_variants_gpu.py (a subprocess, so that ASRK_DETERMINISTIC is read by a fresh library).

    loss_variants_worker.py <out.npz>   the plain cross entropy, forward + backward, twice at every row count of
                                        loss_reference.CE_DET_ROWS: loss_<rows>, grad_<rows> of the first run and
                                        same_<rows> = the second run gave the same bits
"""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "end-to-end-asr-pytorch_amd"
import loss_reference as R          # noqa: E402


def main():
    assert os.environ.get("ASRK_DETERMINISTIC") == "1"
    ops = importlib.import_module(PKG + ".ops")
    out = {}
    for rows in R.CE_DET_ROWS:
        c, x, t = R.ce_inputs('det_%d' % rows)
        runs = []
        for _ in range(2):
            xg = x.cuda().requires_grad_(True)
            loss = ops.CrossEntropyLoss(ignore_index=c.ignore)(xg, t.cuda())
            (loss * R.CE_W).backward()
            runs.append((loss.detach().cpu().numpy(), xg.grad.cpu().numpy()))
        ops.check_errors()
        out['loss_%d' % rows], out['grad_%d' % rows] = runs[0]
        out['same_%d' % rows] = np.asarray(runs[0][0].tobytes() == runs[1][0].tobytes()
                                           and runs[0][1].tobytes() == runs[1][1].tobytes())
    np.savez(sys.argv[1], **out)
    print('DONE', flush=True)


if __name__ == '__main__':
    main()
