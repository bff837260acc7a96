#!/usr/bin/env python
"""Pruned transducer training (src/transducer.py: forward_pruned, csrc/rnnt_prune.hip) timed on the GPU ->
profiles/rnnt_prune.json.

    python tools/rnnt_prune_bench.py [--rounds 5] [--window 0.3] [--steps 3] [--skip-step] [--out profiles/rnnt_prune.json]

Kernels, at the cfg3 shape (B 32, T' 200, U1 65, V 5000, J 512, S 5) and at [16, 200, 65, 16000], every utterance full
length: each new entry point on its own against its HBM floor (the bytes it must move at 8 TB/s) and, for the simple
joiner's row and gradient passes, against its exp floor: B T' U1 V exponentials (twice that for the two gradient
launches) at one 64-lane v_exp_f32 per 8 cycles per SIMD, 1024 SIMDs, 2.4 GHz = 1.97e13 per second.  The larger floor is
the bound that applies.
Step: the cfg3-shaped training step with the pruned head, with the dense head and with no head, alternated in one run,
with the peak memory of each variant's window (all three models stay resident; the peak counter is reset before each
window).

Variants alternate in one process; a figure is the median over `rounds` windows of at least `window` seconds of
back-to-back calls between two device events, after a warm-up of every shape.
Recognition accuracy is not measured: no corpus with transcripts is available to this repository's tools."""
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
from tools.rnnt_bench import HBM_PEAK, HEAD, _model, alternate  # noqa: E402

EXP_PER_S = 1024 * 64 / 8 * 2.4e9        # SIMDs x lanes / issue cycles of v_exp_f32 x clock


def bench_kernels(lib, ops, B, T, U1, V, J, S, rounds, window):
    dev = "cuda"
    torch.manual_seed(0)
    U = U1 - 1
    p, st = ops._p, ops._stream
    f = dict(dtype=torch.float32, device=dev)
    am, lm = torch.randn((B, T, V), **f) * 2, torch.randn((B, U1, V), **f) * 2
    txt = torch.randint(1, V, (B, U), device=dev)
    el = torch.full((B,), T, dtype=torch.int64, device=dev)
    tl = torch.full((B,), U, dtype=torch.int64, device=dev)
    gs = torch.full((B,), 1.0 / B, **f)
    cell = lambda: torch.empty((B, T, U1), **f)
    lse, lpb, lpl, alpha, beta, c, eb, elab = (cell() for _ in range(8))
    nll = torch.empty((B,), **f)
    dam, dlm = torch.empty_like(am), torch.empty_like(lm)
    s = torch.empty((B, T), dtype=torch.int32, device=dev)

    def simple_rows():
        assert lib.asrk_rnnt_simple_rows_f32(p(am), V, p(lm), V, p(txt), U, p(el), p(tl), B, T, U1, V, 0, p(lse), p(lpb),
                                             p(lpl), st()) == 0

    def lattice():
        assert lib.asrk_rnnt_lattice_f32(p(lpb), p(lpl), p(el), p(tl), B, T, U1, p(alpha), p(beta), p(nll), st()) == 0

    def simple_occ():
        assert lib.asrk_rnnt_simple_occ_f32(p(lpb), p(lpl), p(alpha), p(beta), p(nll), p(el), p(tl), B, T, U1, p(c), p(eb),
                                            p(elab), st()) == 0

    def simple_grad():
        assert lib.asrk_rnnt_simple_grad_f32(p(am), V, p(lm), V, p(txt), U, p(el), p(tl), B, T, U1, V, 0, p(lse), p(c),
                                             p(eb), p(elab), p(gs), p(dam), V, p(dlm), V, st()) == 0
    simple_rows()
    lattice()
    simple_occ()
    occ = eb + elab

    def ranges():
        assert lib.asrk_rnnt_prune_ranges_f32(p(occ), p(el), p(tl), B, T, U1, S, p(s), st()) == 0
    ranges()
    E, P = torch.randn((B, T, J), **f), torch.randn((B, U1, J), **f)
    H, dH = torch.empty((B, T, S, J), **f), torch.randn((B, T, S, J), **f)
    dE, dP = torch.empty_like(E), torch.empty_like(P)

    def joint_band():
        assert lib.asrk_rnnt_joint_band_f32(p(E), J, p(P), J, p(s), B, T, S, U1, J, p(H), J, st()) == 0

    def joint_band_bwd():
        assert lib.asrk_rnnt_joint_band_bwd_f32(p(H), J, p(dH), J, p(s), B, T, S, U1, J, p(dE), J, p(dP), J, st()) == 0
    z = torch.randn((B, T, S, V), **f) * 3
    dz = torch.empty_like(z)
    lse_b, lpb_b, lpl_b = (torch.empty((B, T, S), **f) for _ in range(3))
    lpb_d, lpl_d, alpha_d, beta_d = (cell() for _ in range(4))
    nll_b = torch.empty((B,), **f)

    def rows_band():
        assert lib.asrk_rnnt_rows_band_f32(p(z), V, p(txt), U, p(el), p(tl), p(s), B, T, S, U1, V, 0, p(lse_b), p(lpb_b),
                                           p(lpl_b), st()) == 0

    def band_scatter():
        assert lib.asrk_rnnt_band_scatter_f32(p(lpb_b), p(lpl_b), p(s), p(el), p(tl), B, T, S, U1, p(lpb_d), p(lpl_d),
                                              st()) == 0

    def band_lattice():
        assert lib.asrk_rnnt_lattice_f32(p(lpb_d), p(lpl_d), p(el), p(tl), B, T, U1, p(alpha_d), p(beta_d), p(nll_b),
                                         st()) == 0

    def grad_band():
        assert lib.asrk_rnnt_grad_band_f32(p(z), V, p(txt), U, p(el), p(tl), p(s), B, T, S, U1, V, 0, p(lse_b), p(lpb_d),
                                           p(lpl_d), p(alpha_d), p(beta_d), p(nll_b), p(gs), p(dz), V, st()) == 0
    for fn in (joint_band, joint_band_bwd, rows_band, band_scatter, band_lattice, grad_band):
        fn()
    ops.check_errors()
    cells, small = B * T * U1 * 4, (B * T * V + B * U1 * V) * 4
    hb, zb = B * T * S * J * 4, B * T * S * V * 4
    n_exp = B * T * U1 * V
    bytes_moved = {
        "simple_rows": small + 3 * cells, "simple_occ": 8 * cells, "simple_grad": 2 * small + 4 * cells,
        "prune_ranges": cells + B * T * 4, "joint_band": (B * T * J + B * U1 * J) * 4 + hb,
        "joint_band_bwd": 4 * hb + (B * T * J + B * U1 * J) * 4, "rows_band": zb + 3 * B * T * S * 4,
        "band_scatter": 2 * B * T * S * 4 + 2 * cells, "grad_band": 2 * zb, "lattice_simple": 4 * cells,
        "lattice_band": 4 * cells}
    exps = {"simple_rows": n_exp, "simple_grad": 2 * n_exp}
    timing = alternate({"simple_rows": simple_rows, "lattice_simple": lattice, "simple_occ": simple_occ,
                        "simple_grad": simple_grad, "prune_ranges": ranges, "joint_band": joint_band,
                        "joint_band_bwd": joint_band_bwd, "rows_band": rows_band, "band_scatter": band_scatter,
                        "lattice_band": band_lattice, "grad_band": grad_band}, rounds, window)
    out = {"shape": {"B": B, "T": T, "U1": U1, "V": V, "J": J, "S": S, "band_logit_bytes": zb,
                     "dense_logit_bytes": B * T * U1 * V * 4},
           "band_nll_finite": bool(torch.isfinite(nll_b).all()), "kernels": {}}
    for k, t in timing.items():
        ms = t["ms_per_call_median"]
        hbm = bytes_moved[k] / HBM_PEAK * 1e3
        r = {"ms": ms, "ms_min": t["ms_min"], "ms_max": t["ms_max"], "bytes": bytes_moved[k], "hbm_floor_ms": hbm,
             "GBps": bytes_moved[k] / (ms * 1e-3) / 1e9}
        if k in exps:
            r["exp_floor_ms"] = exps[k] / EXP_PER_S * 1e3
            r["exp_per_s"] = exps[k] / (ms * 1e-3)
        floor = max(hbm, r.get("exp_floor_ms", 0.0))
        r["bound"] = "exp" if r.get("exp_floor_ms", 0.0) > hbm else "hbm"
        r["over_floor"] = ms / floor
        out["kernels"][k] = r
    out["sum_of_kernels_ms"] = sum(r["ms"] for r in out["kernels"].values())
    return out


def bench_step(bench, ops, steps, rounds):
    dev = torch.device("cuda")
    w = bench.WORKLOADS["cfg3"]
    fused_optim = importlib.import_module(PKG + ".fused_optim")
    feat, feat_len, txt = bench.synth(w, seed=0, device=dev)
    txt_len = torch.sum(txt != 0, dim=-1)
    L = int(txt_len.max())
    ctc_fn, ce_fn, rnnt_fn = ops.CTCLoss(blank=0), ops.CrossEntropyLoss(ignore_index=0), ops.RNNTLoss(blank=0)

    def make(head):
        model = _model(bench, w, dev, head).train()
        opt = fused_optim.FusedAdadelta(list(model.parameters()), lr=1.0, eps=1e-8)

        def step():
            opt.zero_grad(set_to_none=True)
            encoded = model.encoder(feat, feat_len) if head else None
            ctc_out, enc_len, att_out, _, _ = model(feat, feat_len, L, tf_rate=1.0, teacher=txt, encoded=encoded)
            total = ctc_fn(ctc_out.transpose(0, 1), txt, enc_len, txt_len) * model.ctc_weight
            b, t, _ = att_out.shape
            total = total + ce_fn(att_out.view(b * t, -1), txt.view(-1)) * (1 - model.ctc_weight)
            if head and model.rnnt_prune is not None:
                total = total + model.transducer_loss_pruned(encoded[0], enc_len, txt, txt_len)[0] * model.rnnt_weight
            elif head:
                logits = model.transducer_logits(encoded[0], enc_len, txt, txt_len)
                total = total + rnnt_fn(logits, txt, enc_len, txt_len, consume_logits=True) * model.rnnt_weight
            total.backward()
            opt.clip_and_step(5.0)
        return step
    variants = {"no_head": make(None), "dense_head": make(HEAD),
                "pruned_head": make(dict(HEAD, prune={'enable': True, 'range': 5, 'simple_weight': 0.5}))}

    def wall(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3, torch.cuda.max_memory_allocated() / 1e9
    for fn in variants.values():
        fn()
    resident = torch.cuda.memory_allocated() / 1e9
    times, peaks = {k: [] for k in variants}, {k: 0.0 for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            ms, peak = wall(fn)
            times[k].append(ms)
            peaks[k] = max(peaks[k], peak)
    ops.check_errors()
    out = {"workload": "cfg3: B %d, T %d, V %d, L %d; head: weight 0.3, joint 512, LSTM-512 x1; prune: range 5, "
                       "simple_weight 0.5; random weights" % (w["B"], w["T"], w["V"], w["L"]),
           "steps_per_window": steps, "rounds": rounds, "resident_GB_all_three_models": resident}
    for k in variants:
        out[k] = {"step_ms_median": statistics.median(times[k]), "step_ms_all": times[k], "peak_memory_GB": peaks[k],
                  "peak_above_resident_GB": peaks[k] - resident}
    out["pruned_over_dense"] = out["pruned_head"]["step_ms_median"] / out["dense_head"]["step_ms_median"]
    out["head_cost_ms"] = {k: out[k]["step_ms_median"] - out["no_head"]["step_ms_median"]
                           for k in ("dense_head", "pruned_head")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rnnt_prune.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/rnnt_prune_bench.py measures on the GPU; none is visible")
    ops = importlib.import_module(PKG + ".ops")
    lib = importlib.import_module(PKG + "._lib").load()
    bench = importlib.import_module("bench")
    res = {"what": "pruned transducer training: every new kernel against its HBM floor at 8 TB/s (and its exp floor at "
                   "%.3g exp/s where it has one), a cfg3-shaped step with the pruned head, the dense head and no head "
                   "(device events, windows of >= %.2f s, variants alternated per round, medians)" % (EXP_PER_S,
                                                                                                     args.window),
           "command": "python tools/rnnt_prune_bench.py --rounds %d --window %g --steps %d%s" % (
               args.rounds, args.window, args.steps, " --skip-step" if args.skip_step else ""),
           "device": torch.cuda.get_device_name(0)}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    res["kernels"] = [bench_kernels(lib, ops, 32, 200, 65, 5000, 512, 5, args.rounds, args.window)]
    save()
    torch.cuda.empty_cache()
    res["kernels"].append(bench_kernels(lib, ops, 16, 200, 65, 16000, 512, 5, args.rounds, args.window))
    save()
    torch.cuda.empty_cache()
    if not args.skip_step:
        res["step"] = bench_step(bench, ops, args.steps, args.rounds)
    res["accuracy"] = "not measured: no corpus with transcripts is available to this repository's tools"
    save()
    ops.check_errors()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
