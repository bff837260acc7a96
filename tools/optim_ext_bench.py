#!/usr/bin/env python
"""The optimiser step on the cfg3 parameter set (bench.py WORKLOADS['cfg3']: 173.1 M elements in the model's own tensor
list), one param_group through the C ABI on prebuilt tables:

    plain        asrk_adadelta_multi_f32 / asrk_adam_multi_f32 (unchanged by the feature)          28 B / element
    l2           the extended entry with lambda = 0.01 on every tensor                              28
    adamw        the extended entry, decoupled decay                                                28
    avg_fused    the extended entry with the weight average attached                                36
    avg_separate the plain entry followed by asrk_avg_multi_f32                                     40
    plain_again  the plain rows once more at the end of every block: the spread to read the others against

    python tools/optim_ext_bench.py [--reps 20] [--blocks 7] [--warmup 5] [--out profiles/optim_ext.json]

Durations are hipEvent times over `reps` back-to-back steps (launch gaps included: 3 launches of up to 24 tensors per
step at cfg3); every block times every row, in the same order, in one process on the same buffers; the figure of a row is
the median over the blocks, with min and max beside it.  Each row is also given as a fraction of the time its own byte
count needs at 8 TB/s.  Clocks are left as found (recorded where the tool that reads them is there).  Without a GPU
this fails: nothing is timed on the host."""
import argparse
import ctypes
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "end-to-end-asr-pytorch_amd"
HBM_BYTES_PER_S = 8.0e12
LAMBDA = 0.01


def _clocks():
    try:
        r = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30)
        return [l.strip() for l in r.stdout.splitlines() if "clk" in l.lower()][:16] or "not reported"
    except (OSError, subprocess.SubprocessError):
        return "not reported"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_ext_bench: no GPU - nothing is measured on the host")
    import bench
    ops = importlib.import_module(PKG + ".ops")
    L = importlib.import_module(PKG + "._lib").load()
    dev = torch.device("cuda")
    model = bench.build_model(bench.WORKLOADS["cfg3"], dev)
    params = [p.detach() for p in model.parameters()]
    count, total = len(params), sum(p.numel() for p in params)
    g = torch.Generator(device=dev).manual_seed(0)
    like = lambda scale: [torch.randn(p.shape, generator=g, device=dev) * scale for p in params]
    zeros = lambda: [torch.zeros_like(p) for p in params]
    grads, avg = like(0.01), [p.clone() for p in params]
    states = [zeros() for _ in range(4)]                 # Adadelta's pair and Adam's: neither reads the other's
    ptrs = lambda ts: (ctypes.c_void_p * count)(*[t.data_ptr() for t in ts])
    P, G, E = ptrs(params), ptrs(grads), ptrs(avg)
    D0, D1, S0, S1 = (ptrs(t) for t in states)
    numel = (ctypes.c_int64 * count)(*[p.numel() for p in params])
    wd = (ctypes.c_float * count)(*([LAMBDA] * count))
    coef = torch.tensor([0.7], device=dev)
    st, cf = ops._stream(), ops._p(coef)
    ada = (1.0, 0.95, 1e-8)
    adam = (1e-3, 0.9, 0.999, 1e-8, 10)

    def check(rc):
        assert rc == 0, rc

    rows = {
        "adadelta_plain": (28, lambda: check(L.asrk_adadelta_multi_f32(count, P, G, D0, D1, numel, *ada, cf, st))),
        "adam_plain": (28, lambda: check(L.asrk_adam_multi_f32(count, P, G, S0, S1, numel, *adam, cf, st))),
        "adadelta_l2": (28, lambda: check(L.asrk_adadelta_multi_ext_f32(count, P, G, D0, D1, numel, *ada, cf, wd, 1, None, 0.0, st))),
        "adam_l2": (28, lambda: check(L.asrk_adam_multi_ext_f32(count, P, G, S0, S1, numel, *adam, cf, wd, 1, None, 0.0, st))),
        "adamw": (28, lambda: check(L.asrk_adam_multi_ext_f32(count, P, G, S0, S1, numel, *adam, cf, wd, 2, None, 0.0, st))),
        "adadelta_avg_fused": (36, lambda: check(L.asrk_adadelta_multi_ext_f32(count, P, G, D0, D1, numel, *ada, cf, None, 0, E, 0.001, st))),
        "adam_avg_fused": (36, lambda: check(L.asrk_adam_multi_ext_f32(count, P, G, S0, S1, numel, *adam, cf, None, 0, E, 0.001, st))),
        "adadelta_avg_separate": (40, lambda: (check(L.asrk_adadelta_multi_f32(count, P, G, D0, D1, numel, *ada, cf, st)),
                                               check(L.asrk_avg_multi_f32(count, E, P, numel, 0.001, cf, st)))),
        "adam_avg_separate": (40, lambda: (check(L.asrk_adam_multi_f32(count, P, G, S0, S1, numel, *adam, cf, st)),
                                           check(L.asrk_avg_multi_f32(count, E, P, numel, 0.001, cf, st)))),
    }
    rows["adadelta_plain_again"] = rows["adadelta_plain"]
    rows["adam_plain_again"] = rows["adam_plain"]

    def timed(step):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            step()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.reps

    clocks_before = _clocks()
    for _, step in rows.values():                        # warm-up: code objects loaded, clocks up
        for _ in range(args.warmup):
            step()
    torch.cuda.synchronize()
    blocks = [{name: timed(step) for name, (_, step) in rows.items()} for _ in range(args.blocks)]
    ops.check_errors()
    assert all(bool(torch.isfinite(t).all()) for t in params + avg + sum(states, []))
    out_rows = {}
    for name, (bpe, _) in rows.items():
        us = [b[name] for b in blocks]
        floor_us = bpe * total / HBM_BYTES_PER_S * 1e6
        out_rows[name] = {"bytes_per_element": bpe, "median_us": float(np.median(us)), "min_us": float(np.min(us)),
                          "max_us": float(np.max(us)), "floor_us_at_8TBps": floor_us,
                          "fraction_of_floor_rate": floor_us / float(np.median(us))}
    med = lambda n: out_rows[n]["median_us"]
    res = {"what": "optimiser step on the cfg3 parameter set through the C ABI, hipEvents over back-to-back steps (launch "
                   "gaps included), microseconds per step; %d blocks of %d steps per row, median / min / max over the "
                   "blocks" % (args.blocks, args.reps),
           "tensors": count, "elements": total, "launches_per_step": -(-count // 24), "weight_decay": LAMBDA,
           "clocks_as_found": clocks_before, "rows": out_rows,
           "ratios_over_plain": {k: {n: med("%s_%s" % (k, n)) / med(k + "_plain")
                                     for n in ("l2", "avg_fused", "avg_separate", "plain_again")}
                                 for k in ("adadelta", "adam")},
           "adamw_over_adam_plain": med("adamw") / med("adam_plain"),
           "expected_from_bytes": {"avg_fused": 36 / 28, "avg_separate": 40 / 28},
           "blocks_us": blocks}
    print(json.dumps(res))
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
