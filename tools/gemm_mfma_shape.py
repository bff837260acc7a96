"""The split GEMM kernels alone (operands split once, only the panel GEMM timed) on the cfg3 step's shapes, for comparing
the two MFMA shapes: run it once per value of ASRK_SPLIT_MFMA (16 / 32; knobs are read once per process), alternating.
    ASRK_SPLIT_MFMA=16 python tools/gemm_mfma_shape.py [reps]
One line per shape: the median and the min..max of `reps` timings of 5 launches each, random data.
`ksweep` as a further argument: 25600 x 8192 x K over shallow K instead (where the epilogue's store pattern decides)."""
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

ops = importlib.import_module("end-to-end-asr-pytorch_amd.ops")
# (name, M, N, K, splitk): splitk None = one workgroup per tile, 0 = the library's slice count
SHAPES = [("25600x8192x4096  wide", 25600, 8192, 4096, None),
          ("8192x4096x25600  wide (dW_ih)", 8192, 4096, 25600, None),
          ("4096x1024x51200  128x128 (dW_hh)", 4096, 1024, 51200, None),
          ("6400x8192x4096   wide + 128x128 tail", 6400, 8192, 4096, None),
          ("51200x8192x80    wide, shallow", 51200, 8192, 80, None),
          ("8192x80x51200    128x128 split-K", 8192, 80, 51200, 0)]
if "ksweep" in sys.argv:
    SHAPES = [("25600x8192x%d" % k, 25600, 8192, k, None) for k in (80, 160, 256, 384, 512, 768, 1024, 1536, 2048)]
nums = [int(a) for a in sys.argv[1:] if a.isdigit()]
reps = nums[0] if nums else 5
mf = os.environ.get("ASRK_SPLIT_MFMA", "default")
for name, M, N, K, sk in SHAPES:
    A, B = torch.randn(M, K, device="cuda"), torch.randn(N, K, device="cuda")
    C = torch.empty(M, N, device="cuda")
    pa, pb = ops.SplitPanel(A, K, M, K, False), ops.SplitPanel(B, K, N, K, False)
    del A, B
    run = lambda: ops.gemm_panels(M, N, K, pa, 0, 0, pb, 0, 0, C, N, splitk=sk)
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            run()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / 5)
    ts.sort()
    med = ts[len(ts) // 2]
    print("MFMA=%s %-38s median %.4f ms  min %.4f  max %.4f  %.1f TF/s-equivalent" % (
        mf, name, med, ts[0], ts[-1], 2.0 * M * N * K / med * 1e-9), flush=True)
    del pa, pb, C
    torch.cuda.empty_cache()
