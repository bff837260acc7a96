#!/usr/bin/env python
"""CTC forced alignment (asrk_ctc_align_f32: gather + Viterbi lattice + backtrace, csrc/ctc.hip) timed against the
alpha-only CTC forward (asrk_ctc_loss_fwd_f32 with beta = NULL: gather + alpha lattice), which is the yardstick - the
same walk with lse3 in place of max, and no backtrace.

    python tools/ctc_align_bench.py [--reps 20] [--rounds 7] [--out profiles/ctc_align.json]

Two shapes: B = 32, T = 400, L = 64, V = 5000 (cfg3's encoder output) and B = 32, T = 1600, L = 256.  Per shape the
variants (alpha-only, alignment with the backpointers in LDS, alignment with them in the workspace) ALTERNATE in one
process: every round times `reps` back-to-back launches of each between two device events, after a warm-up of every
variant; the figure is the median over the rounds and the spread is max - min over the rounds.  A forced LDS route
that does not fit the budget is reported as such (ASRK_ESHAPE), not timed.  One further launch per route fills the
kernel's phase stamps (wall_clock64 per utterance: start, lattice done, backtrace done, end).

The expectation the figures are held against: lattice no slower than alpha's; on top, the backtrace at ~100 cycles per
frame (one dependent LDS read of ~50 cycles plus the bit extraction), plus the run-to-run spread of alpha-only."""
import argparse
import ctypes
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "end-to-end-asr-pytorch_amd"
AUTO, LDS, GLOBAL = 0, 1, 2
SHADER_HZ = 2.4e9          # nominal shader clock the cycle budget is converted with
WALL_CLOCK_HZ = 1.0e8      # wall_clock64() of gfx950: the 100 MHz constant clock


def bench_shape(lib, ops, B, T, L, V, reps, rounds):
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    torch.manual_seed(0)
    lp = torch.log_softmax(torch.randn((B, T, V), device=dev), dim=-1).transpose(0, 1)             # the solver's view
    targets = torch.randint(1, V, (B, L), generator=g).to(dev)
    il = torch.full((B,), T, dtype=torch.int64, device=dev)
    tl = torch.full((B,), L, dtype=torch.int64, device=dev)
    S = 2 * L + 1
    alpha = torch.empty((B, T, S), device=dev)
    lpg = torch.empty((B, T, S), device=dev)
    nll = torch.empty((B,), device=dev)
    states = torch.empty((B, T), dtype=torch.int32, device=dev)
    tokens = torch.empty((B, T), dtype=torch.int32, device=dev)
    spans = torch.empty((B, L, 2), dtype=torch.int32, device=dev)
    score = torch.empty((B,), device=dev)
    stamps = torch.zeros((B, 4), dtype=torch.int64, device=dev)
    p, z = ops._p, ctypes.c_void_p(0)

    def run_alpha():
        return lib.asrk_ctc_loss_fwd_f32(p(lp), lp.stride(0), lp.stride(1), T, B, V, p(targets), targets.stride(0), L,
                                         p(il), p(tl), 0, p(alpha), z, p(lpg), p(nll), ops._stream())

    def make_align(flags):
        need = lib.asrk_ctc_align_ws_bytes(B, T, L, flags)
        ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)

        def run(st=None):
            return lib.asrk_ctc_align_f32(p(lp), lp.stride(0), lp.stride(1), T, B, V, p(targets), targets.stride(0),
                                          L, p(il), p(tl), 0, flags, p(states), p(tokens), p(spans), p(score),
                                          p(st), p(ws), need, ops._stream())
        return run, need

    variants = {"alpha_only": run_alpha}
    skipped, ws_bytes = {}, {}
    for name, flags in (("align_lds", LDS), ("align_global", GLOBAL)):
        run, need = make_align(flags)
        rc = run()
        torch.cuda.synchronize()
        if rc != 0:
            skipped[name] = "rc=%d (%s)" % (rc, lib.asrk_strerror(rc).decode())
            continue
        variants[name], ws_bytes[name] = run, need
    for fn in variants.values():                      # warm-up: code objects, allocator, clocks
        for _ in range(5):
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
    res = {"shape": {"B": B, "T": T, "L": L, "V": V, "states": S}, "reps": reps, "rounds": rounds,
           "auto_route": "lds" if lib.asrk_ctc_align_ws_bytes(B, T, L, AUTO) == lib.asrk_ctc_align_ws_bytes(B, T, L, LDS)
           and "align_lds" in variants else "global", "skipped": skipped, "workspace_bytes": ws_bytes}
    for name, v in times.items():
        res[name] = {"us_per_call_median": statistics.median(v), "us_min": min(v), "us_max": max(v),
                     "spread_us": max(v) - min(v), "rounds_us": v}
    a = res["alpha_only"]
    backtrace_budget = T * 100 / SHADER_HZ * 1e6
    res["budget"] = {"alpha_only_us": a["us_per_call_median"], "backtrace_100_cycles_per_frame_us": backtrace_budget,
                     "alpha_spread_us": a["spread_us"],
                     "sum_us": a["us_per_call_median"] + backtrace_budget + a["spread_us"]}
    if "align_lds" in res:
        res["budget"]["align_lds_within"] = res["align_lds"]["us_per_call_median"] <= res["budget"]["sum_us"]
    for name in ("align_lds", "align_global"):        # per-phase stamps of one extra launch
        if name not in variants:
            continue
        stamps.zero_()
        assert variants[name](stamps) == 0
        torch.cuda.synchronize()
        s = stamps.cpu().double()
        ph = {"lattice": s[:, 1] - s[:, 0], "backtrace": s[:, 2] - s[:, 1], "tokens_spans_fill": s[:, 3] - s[:, 2],
              "whole_wave": s[:, 3] - s[:, 0]}
        res[name]["phase_stamps"] = {k: {"ticks_mean": float(v.mean()), "ticks_max": float(v.max()),
                                         "us_mean": float(v.mean()) / WALL_CLOCK_HZ * 1e6,
                                         "us_max": float(v.max()) / WALL_CLOCK_HZ * 1e6} for k, v in ph.items()}
        res[name]["phase_stamps"]["backtrace_cycles_per_frame_at_2.4GHz"] = \
            float(ph["backtrace"].mean()) / WALL_CLOCK_HZ * SHADER_HZ / T
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/ctc_align_bench.py measures on the GPU; none is visible")
    ops = importlib.import_module(PKG + ".ops")
    lib = importlib.import_module(PKG + "._lib").load()
    res = {"what": "asrk_ctc_align_f32 (gather + Viterbi lattice + backtrace) against asrk_ctc_loss_fwd_f32 with "
                   "beta = NULL (gather + alpha lattice); device events around back-to-back launches, variants "
                   "alternated per round in one process; us per call",
           "assumed": {"shader_hz_for_cycle_budget": SHADER_HZ, "wall_clock_hz": WALL_CLOCK_HZ},
           "device": torch.cuda.get_device_name(0),
           "shapes": [bench_shape(lib, ops, 32, 400, 64, 5000, args.reps, args.rounds),
                      bench_shape(lib, ops, 32, 1600, 256, 5000, args.reps, args.rounds)]}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
