"""Worker of tests/test_attention_variants_gpu.py (run as a subprocess with ASRK_DETERMINISTIC=1 so that a fresh library
reads the knob): asrk_embedding_bwd_f32 then takes embedding_bwd_ordered_kernel.  For every shape of
attention_reference.EMB_SHAPES: dW_acc pre-filled with random values, two runs; both must equal, bit for bit, a
sequential float32 accumulation on the host in token order, with the guard bands around dW_acc untouched.  Prints one
`ORDERED n D V ok` line per shape; exits non-zero at the first difference."""
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "end-to-end-asr-pytorch_amd"
import attention_reference as R          # noqa: E402

assert os.environ.get("ASRK_DETERMINISTIC") == "1"
ops = importlib.import_module(PKG + ".ops")
lib = importlib.import_module(PKG + "._lib")
L, p, st = ops._L(), ops._p, ops._stream
GUARD, SENT = 64, 777.25

for n, D, V in R.EMB_SHAPES:
    t = R.emb_inputs(n, D, V)
    want = R.embedding_bwd_sequential_f32(t['idx'], t['dout'], t['RdW'])
    idx, dout = t['idx'].cuda(), t['dout'].cuda()
    runs = []
    for _ in range(2):
        flat = torch.full((V * D + 2 * GUARD,), SENT, dtype=torch.float32, device="cuda")
        dW = flat[GUARD:GUARD + V * D].view(V, D)
        dW.copy_(t['RdW'])
        lib.check(L.asrk_embedding_bwd_f32(p(idx), p(dout), p(dW), n, D, V, st()), "embedding_bwd")
        ops.check_errors()
        g = torch.cat([flat[:GUARD], flat[GUARD + V * D:]]).cpu()
        if not torch.equal(g, torch.full_like(g, SENT)):
            sys.exit("ORDERED %d %d %d wrote outside dW" % (n, D, V))
        runs.append(dW.cpu())
    if not (torch.equal(runs[0], want) and torch.equal(runs[1], want)):
        sys.exit("ORDERED %d %d %d differs from the sequential float32 sum by %.3e" % (
            n, D, V, float((runs[0] - want).abs().max())))
    print("ORDERED %d %d %d ok" % (n, D, V), flush=True)
