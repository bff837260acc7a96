#!/usr/bin/env python
"""Two-pass decoding (src/rescore.py, csrc/rescore.hip) timed on the GPU -> profiles/rescore.json.

    python tools/rescore_bench.py [--reps 5] [--rounds 5] [--skip-e2e] [--out profiles/rescore.json]

Kernels: ops.seq_logp on [640*100, 16000] and [640*100, 5000] logits against ops.log_softmax on the same tensor (the
same bytes read, none written), and ops.ctc_score_rows at 32 x 20 rows of 64 tokens on 400 frames (V = 5000) - the
yardstick for that one is the alpha-only CTC forward of 32 rows in profiles/ctc_align.json.  Variants alternate in one
process; a figure is the median over `rounds` of the time of `reps` back-to-back calls between two device events.

End to end: the cfg5 model of `bench.py --workload cfg5` (32 utterances of 8 s per device batch, beam 16, RNN-LM)
through BeamDecoder.forward_batch and through RescoreDecoder.forward_batch, utterances per second each, and the
rescoring time split into encoder, first pass and second pass (each stage between host synchronisations)."""
import argparse
import importlib
import json
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "end-to-end-asr-pytorch_amd"


def timed(fns, reps, rounds):
    """{name: median ms per call} for callables that alternate round by round"""
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                f()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) / reps)
    return {k: {"ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in out.items()}


def bench_kernels(ops, reps, rounds):
    dev = "cuda"
    res = {}
    for V in (16000, 5000):
        M = 640 * 100
        x = torch.randn((M, V), device=dev) * 4
        tgt = torch.randint(0, V, (M,), device=dev)
        seg = torch.arange(641, device=dev) * 100
        r = timed({"seq_logp": lambda: ops.seq_logp(x, tgt, seg), "log_softmax": lambda: ops.log_softmax(x)}, reps, rounds)
        for k in r:
            r[k]["read_GBps"] = 4.0 * M * V / (r[k]["ms"] * 1e-3) / 1e9
        res["seq_logp_%dx%d" % (M, V)] = r
        del x
    U, nb, L, T, V = 32, 20, 64, 400, 5000
    lp = torch.log_softmax(torch.randn((U, T, V), device=dev), -1)
    targets = torch.randint(1, V, (U * nb, L), device=dev)
    row_mem = torch.arange(U * nb, device=dev) // nb
    ml = torch.full((U,), T, dtype=torch.int64, device=dev)
    tl = torch.full((U * nb,), L, dtype=torch.int64, device=dev)
    res["ctc_score_rows_%dx%d_L%d_T%d" % (U, nb, L, T)] = timed(
        {"ctc_score_rows": lambda: ops.ctc_score_rows(lp, ml, row_mem, targets, tl)}, reps * 4, rounds)
    return res


def bench_e2e(ops, steps):
    import yaml
    bench = importlib.import_module("bench")
    decode = importlib.import_module(PKG + ".src.decode")
    rescore = importlib.import_module(PKG + ".src.rescore")
    lm_mod = importlib.import_module(PKG + ".src.lm")
    dev = torch.device("cuda")
    w = bench.WORKLOADS["cfg3"]
    model = bench.build_model(w, dev).eval()
    torch.manual_seed(1)
    tmp = tempfile.mkdtemp()
    torch.save({'model': lm_mod.RNNLM(w["V"], **bench.CFG5_LM).state_dict()}, os.path.join(tmp, 'lm.pth'))
    yaml.safe_dump({'model': bench.CFG5_LM}, open(os.path.join(tmp, 'lm.yaml'), 'w'))
    lm = dict(lm_path=os.path.join(tmp, 'lm.pth'), lm_config=os.path.join(tmp, 'lm.yaml'))
    joint = decode.BeamDecoder(model, None, **dict(bench.CFG5_DECODE, **lm)).to(dev)
    two = rescore.RescoreDecoder(model, bench.CFG5_DECODE['beam_size'], 24, ctc_weight=bench.CFG5_DECODE['ctc_weight'],
                                 lm_weight=bench.CFG5_DECODE['lm_weight'], device=dev, **lm)
    U, T = bench.CFG5["U"], bench.CFG5["T"]
    feat = torch.cat([bench.cfg5_utterance(T, seed=5 + u)[0] for u in range(U)]).to(dev)
    flen = torch.full((U,), T, dtype=torch.int64, device=dev)
    out = {"workload": "cfg5: %d utterances of %d frames, beam %d, ctc_weight %s, lm_weight %s" % (
        U, T, bench.CFG5_DECODE['beam_size'], bench.CFG5_DECODE['ctc_weight'], bench.CFG5_DECODE['lm_weight'])}
    with torch.no_grad():
        for name, dec in (("joint_beam_search", joint), ("rescore", two)):
            dec.forward_batch(feat, flen)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                hyps = dec.forward_batch(feat, flen)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / steps
            out[name] = {"s_per_batch": dt, "utt_per_s": U / dt}
        out["rescore"]["hyps_per_utt"] = sum(len(h) for h in hyps) / U
        stages = {"encoder": 0.0, "first_pass": 0.0, "second_pass": 0.0}
        for _ in range(steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            enc, enc_len, frames = two._encode(feat, flen)
            ctc = ops.log_softmax(ops.linear(enc, model.ctc_layer.weight, model.ctc_layer.bias))
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            nbest = two.first_pass(ctc, frames)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            two.score_nbest(enc, enc_len, ctc, frames, nbest)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            for k, v in zip(stages, (t1 - t0, t2 - t1, t3 - t2)):
                stages[k] += v / steps
        out["rescore"]["stages_s"] = stages
    ops.check_errors()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rescore.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/rescore_bench.py measures on the GPU; none is visible")
    ops = importlib.import_module(PKG + ".ops")
    res = {"what": "second-pass rescoring: kernels of csrc/rescore.hip and RescoreDecoder against the joint beam search",
           "command": "python tools/rescore_bench.py --reps %d --rounds %d --steps %d%s" % (
               args.reps, args.rounds, args.steps, " --skip-e2e" if args.skip_e2e else ""),
           "device": torch.cuda.get_device_name(0),
           "kernels": bench_kernels(ops, args.reps, args.rounds)}
    if not args.skip_e2e:
        res["end_to_end"] = bench_e2e(ops, args.steps)
    res["accuracy"] = "not measured: no corpus with transcripts is available to this repository's tools"
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
