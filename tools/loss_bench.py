#!/usr/bin/env python
"""The two loss options timed against the plain kernels they sit beside (C ABI calls, no autograd around them):

  * label-smoothed cross entropy (asrk_cross_entropy_ls_{fwd,bwd}_f32) against asrk_cross_entropy_{fwd,bwd}_f32 at
    (rows 2048, V 5000) and (rows 1024, V 16000), a third of the targets ignored;
  * CTC with ASRK_CTC_ZERO_INFINITY (asrk_ctc_loss_{fwd,bwd}_ex_f32) against flags = 0 on an all-feasible batch at
    T = 400, B = 32, L = 64, V = 5000 (alpha and beta lattices in the forward, as in training).

    python tools/loss_bench.py [--reps 20] [--rounds 9] [--out profiles/loss_options.json]

Per shape and direction the variants ALTERNATE in one process: after a warm-up of every variant, each round times
`reps` back-to-back launches of each variant between two device events; the figure is the median over the rounds.  The
plain variant is in the rotation TWICE (plain, plain_again): the ratio of those two is the run-to-run spread the other
ratios are read against.  Expectation: each ratio <= 1.10 (the same bytes move; one more accumulator per lane in the
smoothed forward, one compare per utterance for the flag)."""
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
BOUND = 1.10
ZERO_INFINITY = 1          # ASRK_CTC_ZERO_INFINITY


def alternate(variants, reps, rounds):
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
    res = {name: {"us_per_call_median": statistics.median(v), "us_min": min(v), "us_max": max(v), "rounds_us": v}
           for name, v in times.items()}
    base = res["plain"]["us_per_call_median"]
    res["spread_plain_vs_plain"] = res["plain_again"]["us_per_call_median"] / base
    for name in variants:
        if name not in ("plain", "plain_again"):
            res["ratio_" + name] = res[name]["us_per_call_median"] / base
            res["within_bound_" + name] = res["ratio_" + name] <= BOUND
    return res


def bench_ce(lib, ops, R, V, eps, reps, rounds):
    dev = "cuda"
    torch.manual_seed(0)
    x = torch.randn((R, V), device=dev) * 3.0
    t = torch.randint(1, V, (R,), device=dev)
    t[torch.arange(R, device=dev) % 3 == 1] = 0
    lse, smooth = torch.empty((R,), device=dev), torch.empty((R,), device=dev)
    sums = torch.empty((3,), device=dev)
    gscale = torch.full((1,), 1.0 / R, device=dev)
    dx = torch.empty_like(x)
    p, s = ops._p, ops._stream

    def plain_fwd():
        return lib.asrk_cross_entropy_fwd_f32(p(x), R, V, V, p(t), 0, p(lse), p(sums), s())

    def smooth_fwd():
        return lib.asrk_cross_entropy_ls_fwd_f32(p(x), R, V, V, p(t), 0, p(lse), p(smooth), p(sums), s())

    def plain_bwd():
        return lib.asrk_cross_entropy_bwd_f32(p(x), R, V, V, p(t), 0, p(lse), p(gscale), p(dx), s())

    def smooth_bwd():
        return lib.asrk_cross_entropy_ls_bwd_f32(p(x), R, V, V, p(t), 0, eps, p(lse), p(gscale), p(dx), s())
    assert plain_fwd() == 0
    return {"shape": {"rows": R, "V": V, "label_smoothing": eps, "logit_bytes": R * V * 4}, "reps": reps, "rounds": rounds,
            "forward": alternate({"plain": plain_fwd, "smoothed": smooth_fwd, "plain_again": plain_fwd}, reps, rounds),
            "backward": alternate({"plain": plain_bwd, "smoothed": smooth_bwd, "plain_again": plain_bwd}, reps, rounds)}


def bench_ctc(lib, ops, T, B, L, V, reps, rounds):
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    torch.manual_seed(0)
    lp = torch.log_softmax(torch.randn((B, T, V), device=dev), dim=-1).transpose(0, 1)             # the solver's view
    targets = torch.randint(1, V, (B, L), generator=g).to(dev)
    il = torch.full((B,), T, dtype=torch.int64, device=dev)
    tl = torch.full((B,), L, dtype=torch.int64, device=dev)
    S = 2 * L + 1
    alpha, beta, lpg = (torch.empty((B, T, S), device=dev) for _ in range(3))
    nll, loss = torch.empty((B,), device=dev), torch.empty((B,), device=dev)
    count = torch.zeros((), dtype=torch.int32, device=dev)
    gscale = torch.full((B,), 1.0 / (B * L), device=dev)
    grad = torch.empty((B, T, V), device=dev).transpose(0, 1)
    p, s, z = ops._p, ops._stream, ctypes.c_void_p(0)
    head = lambda: (p(lp), lp.stride(0), lp.stride(1), T, B, V, p(targets), targets.stride(0), L, p(il), p(tl), 0)

    def plain_fwd():
        return lib.asrk_ctc_loss_fwd_f32(*head(), p(alpha), p(beta), p(lpg), p(nll), s())

    def flag_fwd():
        return lib.asrk_ctc_loss_fwd_ex_f32(*head(), p(alpha), p(beta), p(lpg), p(nll), ZERO_INFINITY, p(loss), p(count),
                                            s())

    def plain_bwd():
        return lib.asrk_ctc_loss_bwd_f32(*head(), p(alpha), p(beta), p(lpg), p(nll), p(gscale), p(grad), grad.stride(0),
                                         grad.stride(1), s())

    def flag_bwd():
        return lib.asrk_ctc_loss_bwd_ex_f32(*head(), p(alpha), p(beta), p(lpg), p(nll), p(gscale), p(grad),
                                            grad.stride(0), grad.stride(1), ZERO_INFINITY, s())
    assert plain_fwd() == 0 and flag_fwd() == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(nll).all()) and int(count) == 0 and torch.equal(nll, loss)          # all feasible
    return {"shape": {"T": T, "B": B, "L": L, "V": V}, "reps": reps, "rounds": rounds,
            "forward": alternate({"plain": plain_fwd, "zero_infinity": flag_fwd, "plain_again": plain_fwd}, reps, rounds),
            "backward": alternate({"plain": plain_bwd, "zero_infinity": flag_bwd, "plain_again": plain_bwd}, reps,
                                  rounds)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/loss_bench.py measures on the GPU; none is visible")
    ops = importlib.import_module(PKG + ".ops")
    lib = importlib.import_module(PKG + "._lib").load()
    res = {"what": "label-smoothed cross entropy and CTC zero_infinity against the plain kernels; device events around "
                   "back-to-back C-ABI launches, variants alternated per round in one process, the plain one twice "
                   "(spread); us per call, ratios of medians",
           "bound": BOUND,
           "device": torch.cuda.get_device_name(0),
           "cross_entropy": [bench_ce(lib, ops, 2048, 5000, 0.1, args.reps, args.rounds),
                             bench_ce(lib, ops, 1024, 16000, 0.1, args.reps, args.rounds)],
           "ctc": [bench_ctc(lib, ops, 400, 32, 64, 5000, args.reps, args.rounds)]}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
