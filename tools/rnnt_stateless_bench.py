#!/usr/bin/env python
"""Stateless prediction network of the transducer head (src/transducer.py with pred.module = stateless,
csrc/rnnt_ctx.hip) against the LSTM x1 head, timed on the GPU -> profiles/rnnt_stateless.json.

    python tools/rnnt_stateless_bench.py [--rounds 5] [--window 0.5] [--steps 3] [--skip-step] [--out FILE]

Search: the shape of tools/rnnt_beam_bench.py - 32 utterances of 8 s, the cfg3 encoder, joint 512, V = 5000, max_symbols
3, max_len 50 - decoded by the greedy search and by the beam search with 4, 8 and 16 slots, once with the stateless head
(dim 512, context 2) and once with the LSTM-512 x1 head, the search alone on the same encoder output.  Every search runs
T' + max_len lock-step iterations whatever it emits, so the two heads do the same number of iterations; per search the
time of one iteration and the library calls one iteration makes.
Kernels: the three entry points alone at the cfg3 shape (B 32, U1 65, D 512, C 2; the step on 256 rows) against the
bytes they must move at 8 TB/s.
Step: the cfg3-shaped training step of tools/rnnt_prune_bench.py (pruned head, range 5) with each predictor.

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
sys.path.insert(0, os.path.join(ROOT, "tools"))
PKG = "end-to-end-asr-pytorch_amd"

import rnnt_bench as RB                          # noqa: E402  (alternate, the model and the LSTM head)
from rnnt_beam_bench import count_calls          # noqa: E402

BEAMS = (4, 8, 16)
MAX_SYMBOLS, MAX_LEN = 3, 50
CONTEXT = 2
STATELESS = dict(RB.HEAD, pred={'module': 'stateless', 'dim': 512, 'context': CONTEXT, 'dropout': 0})
PRUNE = {'enable': True, 'range': 5, 'simple_weight': 0.5}


def bench_search(bench, lib_mod, rounds, window):
    dev = torch.device("cuda")
    w = dict(bench.WORKLOADS["cfg3"], T=800)                 # 8 s of 10 ms frames
    models = {"lstm": RB._model(bench, w, dev, RB.HEAD).eval(), "stateless": RB._model(bench, w, dev, STATELESS).eval()}
    feat, feat_len, _ = bench.synth(w, seed=0, device=dev)
    with torch.no_grad():
        enc, enc_len = models["lstm"].encoder(feat, feat_len)      # the same seed builds the same encoder in both
    T = int(enc.shape[1])
    iters = T + MAX_LEN
    searches = {}
    for name, model in models.items():
        head = model.transducer
        searches["greedy_" + name] = lambda head=head: head.greedy(enc, enc_len, MAX_SYMBOLS, MAX_LEN)
        for W in BEAMS:
            searches["beam%d_%s" % (W, name)] = (lambda head=head, W=W: head.beam_search(enc, enc_len, W, MAX_SYMBOLS,
                                                                                         MAX_LEN, nbest=W))
    timing = RB.alternate(searches, rounds, window)
    out = {"workload": "32 utterances of 8 s (T 800 -> T' %d), V %d, joint 512, max_symbols %d, max_len %d, %d iterations, "
                       "random weights; stateless: dim 512, context %d; lstm: LSTM-512 x1" % (
                           T, w["V"], MAX_SYMBOLS, MAX_LEN, iters, CONTEXT), "iterations": iters, "searches": {}}
    for name, fn in searches.items():
        ms = timing[name]["ms_per_call_median"]
        calls = count_calls(lib_mod, fn)
        out["searches"][name] = {"ms_search_alone": ms, "ms_min": timing[name]["ms_min"], "ms_max": timing[name]["ms_max"],
                                 "utt_per_s_search_alone": w["B"] / (ms * 1e-3), "us_per_iteration": ms * 1e3 / iters,
                                 "library_calls_per_iteration": calls / float(iters)}
    out["stateless_over_lstm_utt_per_s"] = {
        k: out["searches"][k + "_stateless"]["utt_per_s_search_alone"] / out["searches"][k + "_lstm"]["utt_per_s_search_alone"]
        for k in ["greedy"] + ["beam%d" % W for W in BEAMS]}
    for name, model in models.items():
        res = model.transducer.beam_search(enc, enc_len, 8, MAX_SYMBOLS, MAX_LEN, nbest=8)
        out["mean_tokens_best_beam8_" + name] = float(res[1][:, 0].float().mean())
    return out


def bench_kernels(ops, rounds, window, B=32, U1=65, D=512, C=CONTEXT, V=5000, R=256, Lc=50):
    dev = "cuda"
    torch.manual_seed(0)
    X = torch.randn((B, U1, D), device=dev)
    w = torch.randn((D, 1, C), device=dev) / C ** 0.5
    dY = torch.randn((B, U1, D), device=dev)
    emb = torch.randn((V, D), device=dev)
    tokens = torch.randint(1, V, (R, Lc), dtype=torch.int32, device=dev)
    n_tok = torch.randint(0, Lc + 1, (R,), dtype=torch.int32, device=dev)
    Y = ops.rnnt_ctx_fwd(X, w)
    out = torch.empty((R, D), device=dev)
    Xg, wg = X.clone().requires_grad_(True), w.clone().requires_grad_(True)

    def fwd_bwd():
        Xg.grad = wg.grad = None
        ops.RNNTContextFn.apply(Xg, wg).backward(dY)
    timing = RB.alternate({"fwd": lambda: ops.rnnt_ctx_fwd(X, w, out=Y), "fwd_bwd": fwd_bwd,
                           "step": lambda: ops.rnnt_ctx_step(tokens, n_tok, emb, w, out=out)}, rounds, window)
    n = B * U1 * D * 4
    # fwd: X read, Y written; the backward reads Y and dY in the dX pass and X, Y and dY in the dw pass, writes dX
    moved = {"fwd": 2 * n, "fwd_bwd": 2 * n + 6 * n, "step": (C + 1) * R * D * 4}
    res = {"shape": {"B": B, "U1": U1, "D": D, "C": C, "step_rows": R, "V": V}, "kernels": {}}
    for k, t in timing.items():
        us = t["ms_per_call_median"] * 1e3
        res["kernels"][k] = {"us_per_call": us, "us_min": t["ms_min"] * 1e3, "us_max": t["ms_max"] * 1e3,
                             "bytes": moved[k], "hbm_floor_us": moved[k] / RB.HBM_PEAK * 1e6,
                             "launches": {"fwd": 1, "fwd_bwd": 4, "step": 1}[k]}
    res["note"] = ("a call includes its host side (autograd and the allocation of the results in fwd_bwd, the ctypes "
                   "call): at this size the kernels are launch bound, the HBM floor is printed for scale only")
    return res


def bench_step(bench, ops, steps, rounds):
    dev = torch.device("cuda")
    w = bench.WORKLOADS["cfg3"]
    fused_optim = importlib.import_module(PKG + ".fused_optim")
    feat, feat_len, txt = bench.synth(w, seed=0, device=dev)
    txt_len = torch.sum(txt != 0, dim=-1)
    L = int(txt_len.max())
    ctc_fn, ce_fn = ops.CTCLoss(blank=0), ops.CrossEntropyLoss(ignore_index=0)

    def make(head):
        model = RB._model(bench, w, dev, head).train()
        opt = fused_optim.FusedAdadelta(list(model.parameters()), lr=1.0, eps=1e-8)

        def step():
            opt.zero_grad(set_to_none=True)
            encoded = model.encoder(feat, feat_len)
            ctc_out, enc_len, att_out, _, _ = model(feat, feat_len, L, tf_rate=1.0, teacher=txt, encoded=encoded)
            total = ctc_fn(ctc_out.transpose(0, 1), txt, enc_len, txt_len) * model.ctc_weight
            b, t, _ = att_out.shape
            total = total + ce_fn(att_out.view(b * t, -1), txt.view(-1)) * (1 - model.ctc_weight)
            total = total + model.transducer_loss_pruned(encoded[0], enc_len, txt, txt_len)[0] * model.rnnt_weight
            total.backward()
            opt.clip_and_step(5.0)

        def predictor():                 # the prediction network alone, forward and backward
            model.zero_grad(set_to_none=True)
            model.transducer._predict(txt).sum().backward()
        return step, predictor
    made = {"lstm": make(dict(RB.HEAD, prune=PRUNE)), "stateless": make(dict(STATELESS, prune=PRUNE))}
    variants = {"pruned_head_" + k: v[0] for k, v in made.items()}

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3
    for fn in variants.values():
        fn()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(wall(fn))
    ops.check_errors()
    out = {"workload": "cfg3: B %d, T %d, V %d, L %d; head: weight 0.3, joint 512, prune: range 5, simple_weight 0.5; "
                       "predictor LSTM-512 x1 or stateless dim 512 context %d; random weights" % (
                           w["B"], w["T"], w["V"], w["L"], CONTEXT), "steps_per_window": steps, "rounds": rounds}
    for k in variants:
        out[k] = {"step_ms_median": statistics.median(times[k]), "step_ms_all": times[k]}
    out["stateless_over_lstm"] = out["pruned_head_stateless"]["step_ms_median"] / out["pruned_head_lstm"]["step_ms_median"]
    pred = RB.alternate({"predictor_fwd_bwd_" + k: v[1] for k, v in made.items()}, rounds, 0.2)
    out["predictor_alone_ms"] = {k: v["ms_per_call_median"] for k, v in pred.items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rnnt_stateless.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/rnnt_stateless_bench.py measures on the GPU; none is visible")
    ops = importlib.import_module(PKG + ".ops")
    lib_mod = importlib.import_module(PKG + "._lib")
    lib_mod.load()
    bench = importlib.import_module("bench")
    res = {"what": "stateless prediction network (context %d) against the LSTM x1 head: greedy and beam 4 / 8 / 16, the "
                   "search alone on one encoder output; the three context kernels alone; the pruned cfg3-shaped training "
                   "step with each predictor (device events, windows of >= %.2f s, variants alternated per round, medians "
                   "of %d rounds; the step by a host clock around %d synchronised steps)" % (
                       CONTEXT, args.window, args.rounds, args.steps),
           "command": "python tools/rnnt_stateless_bench.py --rounds %d --window %g --steps %d%s" % (
               args.rounds, args.window, args.steps, " --skip-step" if args.skip_step else ""),
           "device": torch.cuda.get_device_name(0)}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    res["kernels"] = bench_kernels(ops, args.rounds, min(args.window, 0.2))
    save()
    res["search"] = bench_search(bench, lib_mod, args.rounds, args.window)
    save()
    torch.cuda.empty_cache()
    if not args.skip_step:
        res["step"] = bench_step(bench, ops, args.steps, args.rounds)
    res["accuracy"] = "not measured: no corpus with transcripts is available to this repository's tools"
    save()
    ops.check_errors()
    print(json.dumps({k: {kk: round(vv, 2) if isinstance(vv, float) else vv for kk, vv in v.items()}
                      for k, v in res["search"]["searches"].items()}))
    print(json.dumps(res["search"]["stateless_over_lstm_utt_per_s"]))
    print(json.dumps(res["kernels"]["kernels"]))
    if "step" in res:
        print(json.dumps({k: v for k, v in res["step"].items() if k != "workload"}))


if __name__ == "__main__":
    main()
