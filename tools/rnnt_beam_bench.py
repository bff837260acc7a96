#!/usr/bin/env python
"""Transducer beam search (TransducerHead.beam_search, csrc/rnnt_beam.hip) timed on the GPU -> profiles/rnnt_beam.json.

    python tools/rnnt_beam_bench.py [--rounds 5] [--window 0.5] [--out profiles/rnnt_beam.json]

Search: the greedy bench's shape - 32 utterances of 8 s, the cfg3 encoder, LSTM-512 prediction network, joint 512,
V = 5000, max_symbols 3, max_len 50 - decoded by the greedy search and by the beam search with 1, 4, 8 and 16 slots, the
search alone on the encoder's output and with the encoder, all in the same run; per beam the time of one iteration and
the library calls one iteration makes.  N-gram: beam 8 with the synthetic 4-gram of tools/ngram_bench.py fused at
weight 0.3.
Row pass: asrk_rnnt_beam_rows_f32 alone on [512, 5000] (K = 16) and [256, 16000] (K = 16) logits, without and with LM
rows, against the time of reading its inputs once at 8 TB/s.

Variants alternate in one process; a figure is the median over `rounds` windows of at least `window` seconds of
back-to-back calls between two device events, after a warm-up of every shape.
Recognition accuracy is not measured: no corpus with transcripts is available to this repository's tools."""
import argparse
import importlib
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
PKG = "end-to-end-asr-pytorch_amd"
HBM_PEAK = 8.0e12
BEAMS = (1, 4, 8, 16)
MAX_SYMBOLS, MAX_LEN = 3, 50

import rnnt_bench as RB          # noqa: E402  (alternate, the model and the head of the greedy bench)


def count_calls(lib_mod, fn):
    """library calls (asrk_* entry points checked through _lib.check) one run of fn makes"""
    n = [0]
    check = lib_mod.check

    def counting(rc, what=""):
        n[0] += 1
        return check(rc, what)
    lib_mod.check = counting
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        lib_mod.check = check
    return n[0]


def bench_search(bench, lib_mod, rounds, window):
    dev = torch.device("cuda")
    w = dict(bench.WORKLOADS["cfg3"], T=800)                 # 8 s of 10 ms frames
    model = RB._model(bench, w, dev, RB.HEAD).eval()
    feat, feat_len, _ = bench.synth(w, seed=0, device=dev)
    with torch.no_grad():
        enc, enc_len = model.encoder(feat, feat_len)
    head = model.transducer
    T = int(enc.shape[1])
    iters = T + MAX_LEN
    ngram = importlib.import_module(PKG + ".src.ngram")
    NB = importlib.import_module("ngram_bench")
    lm = ngram.NGramLM(ngram.build_image(4, NB.synthetic_tables(w["V"]), w["V"])).to(dev)

    def encoder():
        with torch.no_grad():
            return model.encoder(feat, feat_len)

    def with_encoder(search):
        def run():
            e, n = encoder()
            search(e, n)
        return run
    searches = {"greedy": lambda e=enc, n=enc_len: head.greedy(e, n, MAX_SYMBOLS, MAX_LEN)}
    for W in BEAMS:
        searches["beam%d" % W] = (lambda e=enc, n=enc_len, W=W: head.beam_search(e, n, W, MAX_SYMBOLS, MAX_LEN, nbest=W))
    searches["beam8_ngram"] = lambda e=enc, n=enc_len: head.beam_search(e, n, 8, MAX_SYMBOLS, MAX_LEN, nbest=8, lm=lm,
                                                                          lm_weight=0.3)
    variants = {}
    for name, fn in searches.items():
        variants[name + "_search_alone"] = fn
        variants[name + "_with_encoder"] = with_encoder(fn)
    timing = RB.alternate(variants, rounds, window)
    out = {"workload": "32 utterances of 8 s (T 800 -> T' %d), V %d, max_symbols %d, max_len %d, %d iterations, random "
                       "weights" % (T, w["V"], MAX_SYMBOLS, MAX_LEN, iters), "iterations": iters, "searches": {}}
    setup = count_calls(lib_mod, lambda: head.beam_search(enc[:, :1].contiguous(), torch.ones_like(enc_len), 4,
                                                          MAX_SYMBOLS, 0))
    per_iter1 = (count_calls(lib_mod, lambda: head.beam_search(enc[:, :2].contiguous(), torch.ones_like(enc_len), 4,
                                                               MAX_SYMBOLS, 0)) - setup)
    for name, fn in searches.items():
        alone = timing[name + "_search_alone"]["ms_per_call_median"]
        whole = timing[name + "_with_encoder"]["ms_per_call_median"]
        calls = count_calls(lib_mod, fn)
        out["searches"][name] = {
            "ms_search_alone": alone, "ms_with_encoder": whole,
            "utt_per_s_search_alone": w["B"] / (alone * 1e-3), "utt_per_s_with_encoder": w["B"] / (whole * 1e-3),
            "us_per_iteration": alone * 1e3 / iters, "library_calls": calls,
            "library_calls_per_iteration": calls / float(iters)}
    out["beam_calls_per_iteration_exact"] = per_iter1
    out["timing"] = timing
    res = head.beam_search(enc, enc_len, 8, MAX_SYMBOLS, MAX_LEN, nbest=8)
    out["mean_tokens_best_beam8"] = float(res[1][:, 0].float().mean())
    out["mean_hypotheses_beam8"] = float(res[3].float().mean())
    return out


def bench_rows(ops, rounds, window):
    dev = torch.device("cuda")
    out = []
    for M, V, W, K in ((512, 5000, 16, 16), (256, 16000, 16, 16)):
        g = torch.Generator(device="cpu").manual_seed(V)
        z = (torch.randn((M, V), generator=g) * 4).to(dev)
        lm = torch.log_softmax(torch.randn((M, V), generator=g) * 2, dim=1).to(dev)
        bufs = (torch.empty((M,), dtype=torch.float32, device=dev), torch.empty((M,), dtype=torch.float32, device=dev),
                torch.empty((M, K), dtype=torch.float32, device=dev), torch.empty((M, K), dtype=torch.int32, device=dev))
        timing = RB.alternate({"no_lm": lambda: ops.rnnt_beam_rows(z, W, K, out=bufs),
                               "with_lm": lambda: ops.rnnt_beam_rows(z, W, K, lm, 0.3, out=bufs),
                               "log_softmax": lambda: ops.log_softmax(z)}, rounds, window)
        rec = {"rows": M, "V": V, "K": K, "timing": timing}
        for name, nbytes in (("no_lm", 4 * M * V), ("with_lm", 8 * M * V), ("log_softmax", 8 * M * V)):
            us = timing[name]["ms_per_call_median"] * 1e3
            rec[name] = {"us": us, "single_pass_us_at_8TBps": nbytes / HBM_PEAK * 1e6,
                         "fraction_of_hbm_peak": nbytes / HBM_PEAK * 1e6 / us}
        out.append(rec)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rnnt_beam.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/rnnt_beam_bench.py measures on the GPU; none is visible")
    ops = importlib.import_module(PKG + ".ops")
    lib_mod = importlib.import_module(PKG + "._lib")
    lib_mod.load()
    bench = importlib.import_module("bench")
    res = {"what": "transducer beam search: greedy and beam 1 / 4 / 8 / 16 (+ n-gram at beam 8) on the greedy bench's "
                   "shape, the search alone and with the encoder, and the row pass alone against one read of its inputs "
                   "(device events, windows of >= %.2f s, variants alternated per round, medians of %d rounds)" % (
                       args.window, args.rounds),
           "command": "python tools/rnnt_beam_bench.py --rounds %d --window %g" % (args.rounds, args.window),
           "device": torch.cuda.get_device_name(0)}
    res["rows"] = bench_rows(ops, args.rounds, args.window)
    res["search"] = bench_search(bench, lib_mod, args.rounds, args.window)
    res["accuracy"] = "not measured: no corpus with transcripts is available to this repository's tools"
    ops.check_errors()
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "search"}))
    print(json.dumps({k: {kk: round(vv, 2) for kk, vv in v.items()} for k, v in res["search"]["searches"].items()}))


if __name__ == "__main__":
    main()
