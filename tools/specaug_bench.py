#!/usr/bin/env python
"""The SpecAugment kernel (csrc/spec_augment.hip) alone on a cfg3-shaped feature batch (32 utterances x 1600 frames x
80 mel bins), stated against its compulsory HBM traffic - one read and one write of the batch - over the 8 TB/s that
bench.py's `roofline_hbm` uses.

    python tools/specaug_bench.py [--B 32] [--T 1600] [--mel 80] [--channels 1] [--reps 200] [--out file.json]

Two figures: `rotating` walks over enough (x, y) pairs that no launch finds its batch in the 256-MB Infinity Cache
(what a training step sees: the front end has just written x, but a whole model step lies between two launches), `same
buffers` re-runs one pair (cache-resident: the ceiling of the kernel itself).  Durations are hipEvent times over `reps`
back-to-back launches; a per-launch figure from `rocprofv3 --kernel-trace --stats` belongs beside them."""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "end-to-end-asr-pytorch_amd"
HBM_BYTES_PER_S = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--T", type=int, default=1600)
    ap.add_argument("--mel", type=int, default=80)
    ap.add_argument("--channels", type=int, default=1)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    ops = importlib.import_module(PKG + ".ops")
    audio = importlib.import_module(PKG + ".src.audio")
    B, T, C, D = args.B, args.T, args.channels, args.mel
    sa = audio.SpecAugment(D, C)                                   # the default policy: W = 80, 2 x F <= 27, 2 x T <= 100
    lens_host = [T - 7 * b for b in range(B)]
    lens = torch.tensor(lens_host, dtype=torch.int64, device="cuda")
    nbytes = 2 * B * T * C * D * 4
    pairs = max(2, int(2 * 256 * 2 ** 20 // nbytes) + 1)           # twice the Infinity Cache
    g = torch.Generator().manual_seed(0)
    xs = [torch.randn(B, T, C * D, generator=g).cuda() for _ in range(pairs)]
    tabs = [sa.sample(lens_host, 0, k).cuda() for k in range(pairs)]

    def timed(n_pairs):
        for k in range(n_pairs):
            ops.spec_augment(xs[k], lens, tabs[k], sa.n_freq_mask, sa.n_time_mask, 0.0, channels=C)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for r in range(args.reps):
            k = r % n_pairs
            ops.spec_augment(xs[k], lens, tabs[k], sa.n_freq_mask, sa.n_time_mask, 0.0, channels=C)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / args.reps
        return {"us_per_launch": us, "TB_per_s": nbytes / (us * 1e-6) / 1e12,
                "fraction_of_8TBs": nbytes / (us * 1e-6) / HBM_BYTES_PER_S}

    res = {"what": "asrk_spec_augment_f32 alone, hipEvents over back-to-back launches (includes the launch gaps)",
           "shape": {"B": B, "T": T, "channels": C, "mel": D, "ld": C * D}, "policy": sa.create_msg(),
           "compulsory_bytes": nbytes, "floor_us_at_8TBs": nbytes / HBM_BYTES_PER_S * 1e6, "reps": args.reps,
           "rotating": dict(timed(pairs), buffer_pairs=pairs), "same_buffers": timed(1)}
    print(json.dumps(res))
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
