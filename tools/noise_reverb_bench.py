#!/usr/bin/env python
"""The reverberation / noise entry (csrc/reverb_mix.hip) alone on a cfg3-shaped PCM batch (32 utterances x 16 s of int16
at 16 kHz), at K = 1024, 4096 and 8192 taps:

  * `all_reverb`: every row convolved, no noise - stated against the convolution's arithmetic floor
    2 * sum_b K_b n_b / 157.3 TFLOP/s (the f32 vector peak; the f32 MFMA has the same rate);
  * `half_reverb_noise`: every second row convolved, every row with noise (what prob = 0.5 costs on average);
  * `noise_only` (no K): no row convolved, every row with noise - both passes are then streams, stated against their
    compulsory HBM traffic over the 8 TB/s that bench.py's `roofline_hbm` uses: pass 1 reads x and v (2 B each) and
    writes out (4 B), pass 2 reads out (4 B) and v (2 B) and writes out (4 B).

    python tools/noise_reverb_bench.py [--B 32] [--seconds 16] [--reps 20] [--blocks 3] [--block-ms 250] [--step-ms MS] [--out profiles/noise_reverb.json]

Durations are hipEvent times over blocks of back-to-back calls of the C ABI on preallocated buffers (the launch gaps are
included; a call is two launches; a block is at least --reps calls and at least --block-ms long; us_per_call is the mean
of the blocks, us_blocks lists them).  --step-ms: the duration of one cfg3 training step (python bench.py on the same box)
for the share of a step that one batch's augmentation takes."""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "end-to-end-asr-pytorch_amd"
HBM_BYTES_PER_S = 8.0e12
F32_FLOPS = 157.3e12
TAPS = (1024, 4096, 8192)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=16.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--block-ms", type=float, default=250.0)
    ap.add_argument("--step-ms", type=float, default=0.0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    ops = importlib.import_module(PKG + ".ops")
    lib = importlib.import_module(PKG + "._lib").load()
    B, n = args.B, int(16000 * args.seconds)
    rng = np.random.default_rng(0)
    pcm = lambda rows, cols: torch.from_numpy(
        np.clip(np.round(rng.standard_normal((rows, cols)) * 3000), -32768, 32767).astype(np.int16)).cuda()
    x, v = pcm(B, n), pcm(B, n)
    ld_out = (n + 3) // 4 * 4
    out = torch.empty((B, ld_out), dtype=torch.float32, device="cuda")
    ns = np.full(B, n, dtype=np.int64)
    n_dev = torch.from_numpy(ns).cuda()
    snr_dev = torch.full((B,), 10.0, dtype=torch.float32, device="cuda")
    ws_bytes = lib.asrk_reverb_mix_ws_bytes(B, n)
    ws = torch.empty((ws_bytes // 8,), dtype=torch.float64, device="cuda")
    stream = ops._stream()
    P = ops._p

    def timed(bank, idx, ms):
        idx = np.asarray(idx, dtype=np.int32)
        ms = np.asarray(ms, dtype=np.int64)
        idx_dev, m_dev = torch.from_numpy(idx).cuda(), torch.from_numpy(ms).cuda()
        R = 0 if bank is None else len(bank)

        def call():
            rc = lib.asrk_reverb_mix_f32(
                P(x), 2, n, ns.ctypes.data, P(n_dev), P(bank.taps) if bank else None, bank.ld if bank else 0,
                bank.lens.ctypes.data if bank else None, bank.meta.data_ptr() if bank else None,
                bank.peaks.ctypes.data if bank else None, bank.meta.data_ptr() + 4 * R if bank else None, R,
                idx.ctypes.data, P(idx_dev), P(v), n, ms.ctypes.data, P(m_dev), P(snr_dev), B, P(out), ld_out,
                1.0 / 32768.0, P(ws), ws_bytes, stream)
            assert rc == 0, rc

        def block(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                call()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3 / reps
        call()
        call()
        torch.cuda.synchronize()
        reps = max(args.reps, int(args.block_ms * 1e3 / block(5)) + 1)      # a block lasts at least --block-ms
        return [block(reps) for _ in range(args.blocks)], reps

    def report(timing, flops, nbytes):
        (blocks, reps), us = timing, float(np.mean(timing[0]))
        r = {"us_per_call": us, "us_blocks": blocks, "calls_per_block": reps}
        if flops:
            r.update(conv_flops=flops, conv_floor_us=flops / F32_FLOPS * 1e6, TFLOPs=flops / (us * 1e-6) / 1e12,
                     fraction_of_conv_floor=flops / F32_FLOPS * 1e6 / us)
        if nbytes:
            r.update(stream_bytes=nbytes, stream_floor_us=nbytes / HBM_BYTES_PER_S * 1e6)
        if args.step_ms > 0:
            r["share_of_cfg3_step"] = us * 1e-3 / args.step_ms
        return r

    res = {"what": "asrk_reverb_mix_f32 alone, hipEvents over back-to-back calls (two launches each, gaps included)",
           "shape": {"B": B, "samples_per_row": n, "sample_bytes": 2, "ld_out": ld_out}, "reps": args.reps,
           "cfg3_step_ms": args.step_ms, "configs": {}}
    mix_bytes = B * n * (4 + 2 + 4)
    r = report(timed(None, [-1] * B, [n] * B), 0, B * n * (2 + 2 + 4) + mix_bytes)
    r["fraction_of_8TBs"] = r["stream_floor_us"] / r["us_per_call"]
    res["configs"]["noise_only"] = r
    for K in TAPS:
        h = rng.standard_normal((2, K)) * np.exp(-np.arange(K) / (K / 7.0))
        h[:, 3] = 4.0
        bank = ops.RirBank(list(h.astype(np.float32)))
        res["configs"]["all_reverb_K%d" % K] = report(timed(bank, [b % 2 for b in range(B)], [0] * B),
                                                      2.0 * B * K * n, B * n * (4 + 4))
        half = [0 if b % 2 == 0 else -1 for b in range(B)]
        res["configs"]["half_reverb_noise_K%d" % K] = report(timed(bank, half, [n] * B),
                                                             2.0 * (B // 2 + B % 2) * K * n, mix_bytes)
    print(json.dumps(res))
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
