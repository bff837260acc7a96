#!/usr/bin/env python
"""The speed-perturbation resampler (csrc/resample.hip) alone on a cfg3-shaped PCM batch (32 utterances x 16 s of int16
at 16 kHz, factors 0.9 / 1.0 / 1.1 mixed over the rows), stated against its compulsory HBM traffic - one read of the PCM
and one write of the float waveforms - over the 8 TB/s that bench.py's `roofline_hbm` uses; then the whole batch front
end (BatchFeatureTransform: host padding, pinned upload, resampler, fbank, delta + CMVN) with and without perturbation, on
the same build in the same process, in alternating blocks.

    python tools/speed_perturb_bench.py [--B 32] [--seconds 16] [--reps 200] [--out profiles/speed_perturb.json]

Kernel figures: `rotating` walks over enough (x, y) pairs that no launch finds its batch in the 256-MB Infinity Cache
(what a training step sees: a whole model step lies between two front ends), `same buffers` re-runs one pair
(cache-resident: the ceiling of the kernel itself).  Durations are hipEvent times over `reps` back-to-back launches of
the C ABI on preallocated buffers (the launch gaps are included); a per-launch figure from `rocprofv3 --kernel-trace
--stats` belongs beside them."""
import argparse
import ctypes
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "end-to-end-asr-pytorch_amd"
HBM_BYTES_PER_S = 8.0e12
FACTORS = (0.9, 1.0, 1.1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=16.0)
    ap.add_argument("--mel", type=int, default=80)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--front-end-reps", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    ops = importlib.import_module(PKG + ".ops")
    audio = importlib.import_module(PKG + ".src.audio")
    lib = importlib.import_module(PKG + "._lib").load()
    SP = audio.SpeedPerturb
    B, n = args.B, int(16000 * args.seconds)
    speeds = [FACTORS[b % len(FACTORS)] for b in range(B)]
    ratios = [SP.ratio(f) for f in FACTORS]
    idx = np.asarray([b % len(FACTORS) for b in range(B)], dtype=np.int32)
    ns = np.full(B, n, dtype=np.int64)
    rat = np.ascontiguousarray(np.asarray(ratios, dtype=np.int32))
    n_out = np.asarray([SP.out_samples(n, f) for f in speeds], dtype=np.int64)
    ld_out = (int(n_out.max()) + 3) // 4 * 4
    nbytes = B * n * 2 + int(n_out.sum()) * 4
    pairs = max(2, int(2 * 256 * 2 ** 20 // (B * n * 2 + B * ld_out * 4)) + 1)     # twice the Infinity Cache
    rng = np.random.default_rng(0)
    xs = [torch.from_numpy(np.clip(np.round(rng.standard_normal((B, n)) * 3000), -32768, 32767).astype(np.int16)).cuda()
          for _ in range(pairs)]
    ys = [torch.empty((B, ld_out), dtype=torch.float32, device="cuda") for _ in range(pairs)]
    n_dev, idx_dev = torch.from_numpy(ns).cuda(), torch.from_numpy(idx).cuda()
    tabs = [None if r == (1, 1) else ops._resample_taps_dev(r[0], r[1], xs[0].device) for r in ratios]
    taps = (ctypes.c_void_p * len(tabs))(*[None if t is None else t.data_ptr() for t in tabs])
    stream = ops._stream()

    def launch(k):
        rc = lib.asrk_resample_rows_f32(ops._p(xs[k]), 2, n, ns.ctypes.data, ops._p(n_dev), idx.ctypes.data,
                                        ops._p(idx_dev), B, rat.ctypes.data, taps, len(tabs), ops._p(ys[k]), ld_out,
                                        1.0 / 32768.0, stream)
        assert rc == 0, rc

    def timed(n_pairs):
        for k in range(n_pairs):
            launch(k)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for r in range(args.reps):
            launch(r % n_pairs)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / args.reps
        return {"us_per_launch": us, "TB_per_s": nbytes / (us * 1e-6) / 1e12,
                "fraction_of_8TBs": nbytes / (us * 1e-6) / HBM_BYTES_PER_S}

    res = {"what": "asrk_resample_rows_f32 alone, hipEvents over back-to-back launches (includes the launch gaps)",
           "shape": {"B": B, "samples_per_row": n, "sample_bytes": 2, "ld_out": ld_out, "factors": list(FACTORS),
                     "ratios": [list(r) for r in ratios], "rows_per_factor": [speeds.count(f) for f in FACTORS]},
           "compulsory_bytes": nbytes, "floor_us_at_8TBs": nbytes / HBM_BYTES_PER_S * 1e6, "reps": args.reps,
           "rotating": dict(timed(pairs), buffer_pairs=pairs), "same_buffers": timed(1)}
    del xs, ys
    torch.cuda.empty_cache()

    # the whole front end with and without perturbation: the same object, alternating blocks, host clock around calls
    # that end in a device synchronise, and the device time of the front end's own kernels from the library's hooks
    bt = audio.BatchFeatureTransform(dict(feat_type="fbank", feat_dim=args.mel, frame_length=25, frame_shift=10,
                                          dither=0, apply_cmvn=True, delta_order=0))
    pcm = [np.clip(np.round(rng.standard_normal(n) * 3000), -32768, 32767).astype(np.int16) for _ in range(B)]
    reps = args.front_end_reps

    def front_end(sp):
        fn = (lambda: bt(pcm, 16000, speeds=sp)) if sp is not None else (lambda: bt(pcm, 16000))
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / reps
        lib.asrk_profile_reset()
        lib.asrk_profile_enable(1)
        fn()
        torch.cuda.synchronize()
        lib.asrk_profile_enable(0)
        ms, cnt = ctypes.c_double(0), ctypes.c_int64(0)
        lib.asrk_profile_get(7, ctypes.byref(ms), ctypes.byref(cnt))                # PROF_FBANK: the front end's kernels
        return {"ms_per_batch": wall * 1e3, "front_end_kernels_ms": ms.value, "front_end_launches": cnt.value}

    blocks = []
    for _ in range(3):
        blocks.append({"plain": front_end(None), "perturbed": front_end(speeds)})
    res["front_end"] = {
        "what": "BatchFeatureTransform on the same PCM (host padding + pinned int16 upload + kernels), %d calls per block, "
                "three alternating pairs of blocks; front_end_kernels_ms = device time of one call's fbank-family "
                "launches (the resampler among them) between the library's profiling events" % reps,
        "blocks": blocks,
        "plain_ms_per_batch_mean": float(np.mean([b["plain"]["ms_per_batch"] for b in blocks])),
        "perturbed_ms_per_batch_mean": float(np.mean([b["perturbed"]["ms_per_batch"] for b in blocks])),
        "plain_kernels_ms_mean": float(np.mean([b["plain"]["front_end_kernels_ms"] for b in blocks])),
        "perturbed_kernels_ms_mean": float(np.mean([b["perturbed"]["front_end_kernels_ms"] for b in blocks]))}
    print(json.dumps(res))
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
