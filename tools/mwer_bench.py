#!/usr/bin/env python
"""MWER training (src/mwer.py, csrc/mwer.hip, csrc/rescore.hip) timed on the GPU -> profiles/mwer.json.

    python tools/mwer_bench.py [--reps 10] [--rounds 7] [--steps 3] [--skip-step] [--out profiles/mwer.json]

Kernels: the asrk_seq_logp_lse_f32 + asrk_seq_logp_bwd_f32 pair against the asrk_cross_entropy_fwd_f32 +
asrk_cross_entropy_bwd_f32 pair on the same [8192, 5000] and [8192, 16000] logits (C-ABI calls, no autograd around
them).  The headline comparison has NO skipped rows: both pairs then read the logits once per direction and write them
once - 3 * M * V * 4 bytes each - so the cross-entropy pair is the yardstick; no ratio is fixed in advance.  A second
comparison skips a third of the rows (padding) and counts the bytes each pair must then move: a skipped row is never
read by seq_logp_lse / seq_logp_bwd / cross_entropy_bwd, but cross_entropy_fwd reduces every row before it looks at the
target, so seq_logp moves (1 + 2 * live) and cross entropy (2 + live) times M * V * 4.  Bandwidths are those byte counts
over the measured time.  (The cross-entropy forward walks a row twice, max then sum; the second walk is counted as a
cache hit, not as bytes.)  Variants alternate in one process; a figure is the median over `rounds` of the time of
`reps` back-to-back calls between two device events; the cross-entropy pair is in the rotation twice (its spread).

Step: a cfg3-shaped synthetic MWER step (bench.py's cfg3 model and batch: B = 32, T = 1600; N = 4, beam 4, unit token)
against the plain step of the same commit, and the MWER step's stages between host synchronisations: search, training
forward + losses, scoring forward (hypothesis_logp + error counts + loss), backward + update.

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


def alternate(variants, reps, rounds):
    for fn in variants.values():
        for _ in range(3):
            fn()
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
    return {k: {"us_per_call_median": statistics.median(v), "us_min": min(v), "us_max": max(v)}
            for k, v in times.items()}


def bench_pair(lib, ops, M, V, L, reps, rounds, skip_third):
    dev = "cuda"
    torch.manual_seed(0)
    x = torch.randn((M, V), device=dev) * 3.0
    t = torch.randint(1, V, (M,), device=dev)
    skip = (torch.arange(M, device=dev) % 3 == 1) if skip_third else torch.zeros((M,), dtype=torch.bool, device=dev)
    live = 1.0 - float(skip.float().mean())
    t_ce = torch.where(skip, torch.zeros_like(t), t)
    t_sl = torch.where(skip, torch.full_like(t, -1), t)
    R = M // L
    seg = torch.arange(R + 1, dtype=torch.int64, device=dev) * L
    gseq = torch.randn((R,), dtype=torch.float64, device=dev)
    lse, tok = torch.empty((M,), device=dev), torch.empty((M,), device=dev)
    seq = torch.empty((R,), dtype=torch.float64, device=dev)
    sums = torch.empty((2,), device=dev)
    gscale = torch.full((1,), 1.0 / M, device=dev)
    dx = torch.empty_like(x)
    p, s = ops._p, ops._stream

    def ce_fwd():
        assert lib.asrk_cross_entropy_fwd_f32(p(x), M, V, V, p(t_ce), 0, p(lse), p(sums), s()) == 0

    def ce_bwd():
        assert lib.asrk_cross_entropy_bwd_f32(p(x), M, V, V, p(t_ce), 0, p(lse), p(gscale), p(dx), s()) == 0

    def sl_fwd():
        assert lib.asrk_seq_logp_lse_f32(p(x), V, p(t_sl), p(seg), M, V, R, 0, p(tok), p(lse), p(seq), s()) == 0

    def sl_bwd():
        assert lib.asrk_seq_logp_bwd_f32(p(x), V, p(t_sl), p(lse), p(seg), p(gseq), M, V, R, p(dx), V, s()) == 0

    def ce_pair():
        ce_fwd()
        ce_bwd()

    def sl_pair():
        sl_fwd()
        sl_bwd()
    nbytes = M * V * 4
    out = {"shape": {"rows": M, "V": V, "rows_per_sequence": L, "logit_bytes": nbytes, "live_fraction": live},
           "bytes_moved": {"seq_logp_pair": nbytes * (1 + 2 * live), "cross_entropy_pair": nbytes * (2 + live)},
           "reps": reps, "rounds": rounds}
    sl_fwd()
    out["forward"] = alternate({"cross_entropy": ce_fwd, "seq_logp_lse": sl_fwd, "cross_entropy_again": ce_fwd}, reps,
                               rounds)
    sl_fwd()                                                    # lse of the seq_logp targets for its backward
    out["backward_seq_logp"] = alternate({"seq_logp_bwd": sl_bwd}, reps, rounds)
    ce_fwd()
    out["backward_cross_entropy"] = alternate({"cross_entropy_bwd": ce_bwd}, reps, rounds)
    out["pair"] = alternate({"cross_entropy": ce_pair, "seq_logp": sl_pair, "cross_entropy_again": ce_pair}, reps, rounds)
    base = out["pair"]["cross_entropy"]["us_per_call_median"]
    out["pair"]["ratio_seq_logp"] = out["pair"]["seq_logp"]["us_per_call_median"] / base
    out["pair"]["spread_ce_vs_ce"] = out["pair"]["cross_entropy_again"]["us_per_call_median"] / base
    out["pair"]["seq_logp_GBps"] = out["bytes_moved"]["seq_logp_pair"] / (
        out["pair"]["seq_logp"]["us_per_call_median"] * 1e-6) / 1e9
    out["pair"]["cross_entropy_GBps"] = out["bytes_moved"]["cross_entropy_pair"] / (base * 1e-6) / 1e9
    return out


def bench_step(ops, steps, nbest, beam):
    bench = importlib.import_module("bench")
    mwer = importlib.import_module(PKG + ".src.mwer")
    dev = torch.device("cuda")
    w = bench.WORKLOADS["cfg3"]
    model = bench.build_model(w, dev).train()
    params = list(model.parameters())
    opt = importlib.import_module(PKG + ".fused_optim").FusedAdadelta(params, lr=1.0, eps=1e-8)
    feat, feat_len, txt = bench.synth(w, seed=0, device=dev)
    txt_host = txt.cpu()
    txt_len = torch.sum(txt != 0, dim=-1)
    L = int(txt_len.max())
    ctc_fn, ce_fn = ops.CTCLoss(blank=0), ops.CrossEntropyLoss(ignore_index=0)
    opts = mwer.MWEROptions(nbest=nbest, beam_size=beam, ce_weight=0.01, unit='token',
                            max_len_ratio=float(w["L"]) / w["T"], min_len_ratio=0.0)
    crit = mwer.MWERLoss(model, None, opts)

    def base_loss(encoded=None):
        ctc_out, enc_len, att_out, _, _ = model(feat, feat_len, L, tf_rate=1.0, teacher=txt, encoded=encoded)
        total = ctc_fn(ctc_out.transpose(0, 1), txt, enc_len, txt_len) * model.ctc_weight if ctc_out is not None else 0
        b, t, _ = att_out.shape
        return total + ce_fn(att_out.view(b * t, -1), txt.view(-1)) * (1 - model.ctc_weight), enc_len

    def plain_step():
        opt.zero_grad(set_to_none=True)
        total, _ = base_loss()
        total.backward()
        opt.clip_and_step(5.0)

    stages = {"search": 0.0, "train_forward": 0.0, "scoring_forward": 0.0, "backward_update": 0.0}
    info = {}

    def mwer_step(record=False):
        sync = torch.cuda.synchronize if record else (lambda: None)
        sync()
        t0 = time.perf_counter()
        opt.zero_grad(set_to_none=True)
        nb = crit.nbest(feat, feat_len)
        sync()
        t1 = time.perf_counter()
        encoded = model.encoder(feat, feat_len)
        total, enc_len = base_loss(encoded)
        sync()
        t2 = time.perf_counter()
        loss, stats = crit(nb, encoded[0], enc_len, txt_host)
        total = loss.to(torch.float32) + opts.ce_weight * total
        sync()
        t3 = time.perf_counter()
        total.backward()
        opt.clip_and_step(5.0)
        sync()
        t4 = time.perf_counter()
        if record:
            for k, v in zip(stages, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                stages[k] += v
            info.update(rows=int(nb[0].shape[0]), positions=int(nb[0].shape[1]),
                        mean_count=float(nb[2].float().mean()), exp_err=float(stats['exp_err']))

    def wall(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3

    out = {"workload": "cfg3: B %d, T %d, V %d, L %d; N %d, beam %d, unit token, random weights" % (
        w["B"], w["T"], w["V"], w["L"], nbest, beam), "steps": steps}
    out["plain_step_ms"] = wall(plain_step)
    out["mwer_step_ms"] = wall(mwer_step)
    out["plain_step_again_ms"] = wall(plain_step)
    for _ in range(steps):
        mwer_step(record=True)
    out["mwer_stages_ms"] = {k: v / steps * 1e3 for k, v in stages.items()}
    out["scoring"] = info
    ops.check_errors()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--nbest", type=int, default=4)
    ap.add_argument("--beam", type=int, default=4)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mwer.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/mwer_bench.py measures on the GPU; none is visible")
    ops = importlib.import_module(PKG + ".ops")
    lib = importlib.import_module(PKG + "._lib").load()
    res = {"what": "MWER training: the seq_logp forward/backward pair against the cross-entropy pair on the same logits "
                   "(device events, variants alternated per round, medians), and a cfg3-shaped MWER step against the plain "
                   "step with its stages",
           "command": "python tools/mwer_bench.py --reps %d --rounds %d --steps %d --nbest %d --beam %d%s" % (
               args.reps, args.rounds, args.steps, args.nbest, args.beam, " --skip-step" if args.skip_step else ""),
           "device": torch.cuda.get_device_name(0),
           "kernels": [bench_pair(lib, ops, 8192, 5000, 64, args.reps, args.rounds, False),
                       bench_pair(lib, ops, 8192, 16000, 64, args.reps, args.rounds, False)],
           "kernels_third_of_rows_skipped": [bench_pair(lib, ops, 8192, 5000, 64, args.reps, args.rounds, True),
                                             bench_pair(lib, ops, 8192, 16000, 64, args.reps, args.rounds, True)]}
    if not args.skip_step:
        res["step"] = bench_step(ops, args.steps, args.nbest, args.beam)
    res["accuracy"] = "not measured: no corpus with transcripts is available to this repository's tools"
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
