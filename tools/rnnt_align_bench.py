#!/usr/bin/env python
"""Transducer forced alignment (asrk_rnnt_align_f32: Viterbi lattice + backtrace + token outputs, csrc/rnnt_align.hip)
timed against the alpha-only lattice of the loss (asrk_rnnt_lattice_f32 with beta = NULL), which is the yardstick - the
same anti-diagonal walk with logaddexp where the aligner has a compare, and no backtrace.

    python tools/rnnt_align_bench.py [--reps 50] [--rounds 7] [--out profiles/rnnt_align.json]

Shape: B = 32, T' = 200, U + 1 = 65.  The variants (alpha-only, alignment with the backpointers in LDS, alignment with
them in the workspace) ALTERNATE in one process: every round times `reps` back-to-back launches of each between two
device events, after a warm-up of every variant; the figure is the median over the rounds and the spread is max - min
over the rounds.  One further launch per route fills the kernel's phase stamps (wall_clock64 per utterance: start,
lattice done, backtrace done, end).

Then the whole ASR.transducer_align (encoder, prediction network, joint, lin_out, row pass, lattice, alignment, with
confidence) at V = 5000 on a model with the same T' and U: with the default logits budget (1 GiB: groups of 4
utterances here) and with one utterance per group; a host clock around calls that end in a device synchronise.

Clocks: whatever the device runs at under its default power management; nothing is pinned, the spread says how steady
they were."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "end-to-end-asr-pytorch_amd"
AUTO, LDS, GLOBAL = 0, 1, 2
WALL_CLOCK_HZ = 1.0e8      # wall_clock64() of gfx950: the 100 MHz constant clock


def bench_kernel(lib, ops, B, T, U1, reps, rounds):
    dev = "cuda"
    torch.manual_seed(0)
    V = 64                                                 # a head's log-probabilities, labels drawn per cell
    lp = torch.log_softmax(torch.randn((B, T, U1, V), device=dev) * 3, dim=-1)
    lpb = lp[..., 0].contiguous()
    lpl = lp[..., 1:].gather(3, torch.randint(0, V - 1, (B, T, U1, 1), device=dev)).squeeze(3).contiguous()
    el = torch.full((B,), T, dtype=torch.int64, device=dev)
    tl = torch.full((B,), U1 - 1, dtype=torch.int64, device=dev)
    alpha = torch.empty((B, T, U1), device=dev)
    nll = torch.empty((B,), device=dev)
    frames = torch.empty((B, U1 - 1), dtype=torch.int32, device=dev)
    done = torch.empty((B, T), dtype=torch.int32, device=dev)
    logp = torch.empty((B, U1 - 1), device=dev)
    score = torch.empty((B,), device=dev)
    stamps = torch.zeros((B, 4), dtype=torch.int64, device=dev)
    p = ops._p

    def run_alpha():
        return lib.asrk_rnnt_lattice_f32(p(lpb), p(lpl), p(el), p(tl), B, T, U1, p(alpha), None, p(nll), ops._stream())

    def make_align(flags):
        need = lib.asrk_rnnt_align_ws_bytes(B, T, U1, flags)
        ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)

        def run(st=None):
            return lib.asrk_rnnt_align_f32(p(lpb), p(lpl), p(el), p(tl), B, T, U1, flags, None, None, None, p(frames),
                                           p(done), p(logp), None, p(score), p(st), p(ws), need, ops._stream())
        return run, need

    variants, ws_bytes = {"alpha_only": run_alpha}, {}
    for name, flags in (("align_lds", LDS), ("align_global", GLOBAL)):
        variants[name], ws_bytes[name] = make_align(flags)
    for fn in variants.values():                      # warm-up: code objects, allocator, clocks
        for _ in range(10):
            assert fn() == 0
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / reps)
    res = {"shape": {"B": B, "T": T, "U1": U1}, "reps": reps, "rounds": rounds,
           "auto_route": "lds" if lib.asrk_rnnt_align_ws_bytes(B, T, U1, AUTO) == 0 else "global",
           "workspace_bytes": ws_bytes}
    for name, v in times.items():
        res[name] = {"us_per_call_median": statistics.median(v), "us_min": min(v), "us_max": max(v),
                     "spread_us": max(v) - min(v), "rounds_us": v}
    a = res["alpha_only"]["us_per_call_median"]
    for name in ("align_lds", "align_global"):
        res[name]["ratio_to_alpha_only"] = res[name]["us_per_call_median"] / a
        stamps.zero_()                                # per-phase stamps of one extra launch
        assert variants[name](stamps) == 0
        torch.cuda.synchronize()
        s = stamps.cpu().double()
        ph = {"lattice": s[:, 1] - s[:, 0], "backtrace": s[:, 2] - s[:, 1], "token_outputs": s[:, 3] - s[:, 2],
              "whole_workgroup": s[:, 3] - s[:, 0]}
        res[name]["phase_stamps"] = {k: {"ticks_mean": float(v.mean()), "ticks_max": float(v.max()),
                                         "us_mean": float(v.mean()) / WALL_CLOCK_HZ * 1e6,
                                         "us_max": float(v.max()) / WALL_CLOCK_HZ * 1e6} for k, v in ph.items()}
    return res


def bench_model(B, T, U, V, rounds):
    asr = importlib.import_module(PKG + ".src.asr")
    dev = "cuda"
    torch.manual_seed(0)
    head = {'enable': True, 'weight': 0.3, 'joint_dim': 512,
            'pred': {'module': 'LSTM', 'dim': 512, 'layer': 1, 'emb_dim': 512, 'dropout': 0}}
    enc = dict(prenet='', module='LSTM', bidirection=True, dim=[256, 256], dropout=[0, 0], layer_norm=[False, False],
               proj=[True, True], sample_rate=[2, 2], sample_style='drop')
    model = asr.ASR(120, V, True, 1.0, enc, None, None, transducer=head).to(dev).eval()
    feat = torch.randn((B, 4 * T, 120), device=dev)
    feat_len = torch.full((B,), 4 * T, dtype=torch.int64, device=dev)
    txt = torch.randint(1, V, (B, U), device=dev)
    txt_len = torch.full((B,), U, dtype=torch.int64, device=dev)
    one = T * (U + 1) * V * 4
    res = {"shape": {"B": B, "T": T, "U": U, "V": V, "joint_dim": 512, "logits_bytes_per_utterance": one}}
    for name, budget in (("default_budget", 1 << 30), ("one_utterance_per_group", one)):
        def run():
            out = model.transducer_align(feat, feat_len, txt, txt_len, confidence=True, max_logits_bytes=budget)
            torch.cuda.synchronize()
            return out
        out = run()                                   # warm-up
        assert int(out[5][0]) == T and bool((out[0] >= 0).all())
        ms = []
        for _ in range(rounds):
            t0 = time.perf_counter()
            run()
            ms.append((time.perf_counter() - t0) * 1e3)
        res[name] = {"max_logits_bytes": budget, "utterances_per_group": max(1, budget // one),
                     "ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms), "rounds_ms": ms}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/rnnt_align_bench.py measures on the GPU; none is visible")
    ops = importlib.import_module(PKG + ".ops")
    lib = importlib.import_module(PKG + "._lib").load()
    res = {"what": "asrk_rnnt_align_f32 (Viterbi lattice + backtrace + token outputs) against asrk_rnnt_lattice_f32 with "
                   "beta = NULL (the alpha lattice alone); device events around back-to-back launches, variants "
                   "alternated per round in one process, us per call; then ASR.transducer_align as a whole, host clock "
                   "around synchronised calls, ms per call",
           "clocks": "default power management, nothing pinned",
           "assumed": {"wall_clock_hz": WALL_CLOCK_HZ},
           "device": torch.cuda.get_device_name(0),
           "kernel": bench_kernel(lib, ops, 32, 200, 65, args.reps, args.rounds),
           "model": bench_model(32, 200, 64, 5000, min(args.rounds, 5))}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
