#!/usr/bin/env python
"""The fused log-mel launch (csrc/audio.hip fbank_logmel_batch_kernel) with and without dither on a cfg3-shaped PCM batch:
32 utterances x 16 s of int16 at 16 kHz, 25 ms frames, 80 mel bins.  `plain` is asrk_fbank_logmel_batch_f32 (the
instantiation without dither, unchanged by the feature), `dithered` is asrk_fbank_logmel_batch_dither_f32 at
dither = 1 / 32768 with one key per utterance; same build, same process, same buffers, in alternating blocks.

    python tools/dither_bench.py [--B 32] [--seconds 16] [--mel 80] [--reps 200] [--blocks 5] [--out profiles/dither.json]

Durations are hipEvent times over `reps` back-to-back launches of the C ABI on preallocated buffers (the launch gaps are
included; at these sizes a launch is hundreds of microseconds).  The spread over the blocks is the noise a difference
has to exceed.  A per-launch figure from `rocprofv3 --kernel-trace --stats` belongs beside them (a run of its own: the
two kernels carry their instantiation in the name, ...ELb0EE / ...ELb1EE).  Without a GPU this fails: nothing is timed
on the host."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=16.0)
    ap.add_argument("--mel", type=int, default=80)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--dither", type=float, default=1.0 / 32768.0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dither_bench: no GPU - nothing is measured on the host")
    ops = importlib.import_module(PKG + ".ops")
    audio = importlib.import_module(PKG + ".src.audio")
    lib = importlib.import_module(PKG + "._lib").load()
    B, n, dev = args.B, int(16000 * args.seconds), torch.device("cuda")
    tb = audio._FbankTables.get(16000, 25.0, 10.0, args.mel, 20.0, 0.0, dev)
    m = 1 + (n - tb.win) // tb.shift
    rng = np.random.default_rng(0)
    pcm = torch.from_numpy(np.clip(np.round(rng.standard_normal((B, n)) * 3000), -32768, 32767).astype(np.int16)).to(dev)
    frame_off = torch.arange(B + 1, dtype=torch.int64, device=dev) * m
    keys = audio._keys_to_device([audio.Dither(args.dither, 0).key("utt%d" % b, False) for b in range(B)], dev)
    mel = {k: torch.empty((B * m, args.mel), dtype=torch.float32, device=dev) for k in ("plain", "dithered")}
    stream = ops._stream()
    common = (ops._p(pcm), 2, n, None, ops._p(frame_off), B, m, ops._p(tb.window), ops._p(tb.tw_fft), ops._p(tb.tw_unpack),
              ops._p(tb.melT), ops._p(tb.mel_range), args.mel, args.mel)
    tail = (tb.win, tb.shift, tb.log2n, 1.0 / 32768.0, 0.97, 1, audio.FLT_EPS)

    def launch(kind):
        if kind == "plain":
            rc = lib.asrk_fbank_logmel_batch_f32(*common, ops._p(mel[kind]), *tail, stream)
        else:
            rc = lib.asrk_fbank_logmel_batch_dither_f32(*common, ops._p(mel[kind]), *tail, args.dither, ops._p(keys),
                                                        stream)
        assert rc == 0, rc

    def timed(kind):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            launch(kind)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.reps

    for kind in ("plain", "dithered"):                   # warm-up: code objects loaded, clocks up
        for _ in range(20):
            launch(kind)
    torch.cuda.synchronize()
    blocks = [{kind: timed(kind) for kind in ("plain", "dithered")} for _ in range(args.blocks)]
    diff = float((mel["plain"] - mel["dithered"]).abs().max().cpu())
    assert bool(torch.isfinite(mel["dithered"]).all()) and diff > 0.0
    stat = lambda kind: {"mean": float(np.mean([b[kind] for b in blocks])), "min": float(np.min([b[kind] for b in blocks])),
                         "max": float(np.max([b[kind] for b in blocks]))}
    plain, dithered = stat("plain"), stat("dithered")
    groups = (tb.win + 3) // 4
    res = {"what": "fused log-mel launch alone, hipEvents over back-to-back launches (includes the launch gaps), "
                   "microseconds per launch; alternating blocks of %d launches" % args.reps,
           "shape": {"B": B, "samples_per_row": n, "sample_bytes": 2, "frames_per_row": m, "win": tb.win, "fft": tb.padded,
                     "mel": args.mel, "dither": args.dither},
           "philox_calls_per_frame": groups, "philox_calls_per_launch": groups * B * m,
           "blocks_us": blocks, "plain_us": plain, "dithered_us": dithered,
           "ratio_dithered_over_plain": dithered["mean"] / plain["mean"],
           "max_abs_logmel_difference": diff}
    print(json.dumps(res))
    if args.out:
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
