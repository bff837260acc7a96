"""Contextual biasing: the step kernels alone and two whole searches.

    python tools/bias_bench.py [--out profiles/bias.json] [--skip-search]

1. asrk_bias_step_f32, asrk_ngram_step_f32 and asrk_ngram_bias_step_f32 on the same 640 rows at V in {5000, 16000}:
   1000 random phrases of 2 to 6 tokens and the synthetic 4-gram of tools/ngram_bench.py.  Each launch is captured 24
   times into one graph (no host call between launches) writing 8 output matrices in turn; reported are the time per
   launch, the bytes computed from shapes (R * V * 4 written + the dense tables read once) and the share of the 8 TB/s
   HBM floor, plus the fused launch against the n-gram launch alone and against the sum of the two separate ones.
2. the lock-step CTC prefix beam search (beam 20, 30 candidates, T = 200, 16 utterances) with bias alone, with the
   n-gram, with n-gram + bias, against the search without a scorer (one launch per utterance on 16 streams);
3. the transducer beam search (beam 8, 32 utterances of 100 encoder frames, an LSTM head of width 512 on random
   weights) without a scorer, with bias alone, with the n-gram and with n-gram + bias.
Every figure: warmed, device events around a synchronised window of at least 0.5 s, the variants alternated over three
rounds inside this one call with clocks as found; the median is reported with the rounds beside it.  Needs the GPU."""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
PKG = "end-to-end-asr-pytorch_amd"
ROWS, N_PHRASES, GRAPH_CALLS, BUFFERS = 640, 1000, 24, 8

import ngram_bench as NB          # noqa: E402  (the synthetic 4-gram, timed_window, median_rounds)


def random_phrases(V, n=N_PHRASES, seed=0):
    rng = np.random.RandomState(seed)
    return [(tuple(int(t) for t in rng.randint(3, V, size=int(rng.randint(2, 7)))), 1.0) for _ in range(n)]


def graph_of(launch, R, V, width):
    """GRAPH_CALLS launches of launch(out, state_out) in one graph, BUFFERS output matrices in turn"""
    outs = [torch.empty((R, V), dtype=torch.float32, device="cuda") for _ in range(BUFFERS)]
    state_out = torch.empty((R, width), dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch(outs[0], state_out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(GRAPH_CALLS):
            launch(outs[i % BUFFERS], state_out)
    return g, (outs, state_out)


def bench_kernels(res):
    ngram = importlib.import_module(PKG + ".src.ngram")
    bias = importlib.import_module(PKG + ".src.bias")
    models = {}
    for V in (5000, 16000):
        g_img = ngram.build_image(4, NB.synthetic_tables(V), V)
        lm = ngram.NGramLM(g_img).cuda()
        cb = bias.ContextBias(bias.build_image(random_phrases(V), V, 1.5)).cuda()
        both = bias.BiasedNGram.pair(lm, cb, 0.5).cuda()
        models[V] = (lm, cb, both)
        b_img = cb.image()
        rng = np.random.RandomState(1)
        R = ROWS
        # rows that sit inside a phrase and inside an n-gram context: the node / context and a token that continues it
        e = rng.randint(0, len(b_img["ext_word"]), size=R)
        owner = np.repeat(np.arange(len(b_img["phi"])), np.diff(b_img["ext_off"]))
        b_state, tokens = owner[e].astype(np.int32), b_img["ext_word"][e].astype(np.int64)
        g_state = rng.randint(0, len(g_img["bo"]), size=R).astype(np.int32)
        tok = torch.from_numpy(tokens).view(R, 1).cuda()
        st_b = torch.from_numpy(b_state).view(1, R, 1).cuda()
        st_g = torch.from_numpy(g_state).view(1, R, 1).cuda()
        st_2 = torch.from_numpy(np.stack([g_state, b_state], 1)).view(1, R, 2).contiguous().cuda()
        launches = {"bias": (lambda o, s: cb(tok, None, hidden=st_b, out=o.view(-1), state_out=s.view(-1)), 1),
                    "ngram": (lambda o, s: lm(tok, None, hidden=st_g, out=o.view(-1), state_out=s.view(-1)), 1),
                    "ngram_bias": (lambda o, s: both(tok, None, hidden=st_2, out=o.view(-1), state_out=s.view(-1)), 2)}
        graphs = {k: graph_of(fn, R, V, w) for k, (fn, w) in launches.items()}
        times = NB.median_rounds({k: g.replay for k, (g, _) in graphs.items()})
        nbytes = {"bias": R * V * 4 + V * 4, "ngram": R * V * 4 + V * 4, "ngram_bias": R * V * 4 + 2 * V * 4}
        rec = {"V": V, "R": R, "phrases": N_PHRASES, "bias_nodes": int(len(b_img["phi"])),
               "bias_merged_entries": int(len(b_img["ext_word"])), "ngram_contexts": int(len(g_img["bo"]))}
        for k, (t, rounds) in times.items():
            t, rounds = t / GRAPH_CALLS, [x / GRAPH_CALLS for x in rounds]
            rec[k] = {"kernel_us": t * 1e6, "kernel_us_rounds": [x * 1e6 for x in rounds], "bytes": nbytes[k],
                      "share_of_hbm_floor": (nbytes[k] / NB.HBM_BYTES_PER_S) / t}
        rec["fused_over_ngram_alone"] = rec["ngram_bias"]["kernel_us"] / rec["ngram"]["kernel_us"]
        rec["fused_over_sum_of_separate"] = rec["ngram_bias"]["kernel_us"] / (rec["ngram"]["kernel_us"]
                                                                              + rec["bias"]["kernel_us"])
        res["step_kernels"].append(rec)
        print(json.dumps(rec))
    return models


def bench_ctc(res, models, args):
    ctc = importlib.import_module(PKG + ".src.ctc")
    U = args.U
    for V in (5000, 16000):
        lm, cb, _ = models[V]

        def posteriors(seed):                                           # tools/ctc_beam_bench.py's generator
            g = torch.Generator().manual_seed(seed)
            logits = torch.randn(args.T, V, generator=g) * 1.5
            logits[:, 0] += 9.0
            spikes = torch.randperm(args.T, generator=g)[:args.T // 4]
            logits[spikes, 0] -= 9.0
            return torch.log_softmax(logits, -1)
        xs = torch.stack([posteriors(u) for u in range(U)]).cuda()
        vr = [1] + list(range(3, V))

        def decoder(with_lm, with_bias):
            d = ctc.CTCBeamDecoder(NB.Stub(V), vr, args.beam, args.cand, device="cuda",
                                   bias=cb.rebuilt().cpu() if with_bias and not with_lm else None)
            if with_lm:                                                 # the synthetic model has no file: set the slot
                d.apply_lm, d.lm_w, d.lm_path, d.lm, d.device = True, 0.5, "synthetic", lm, "cuda"
                if with_bias:
                    bias = importlib.import_module(PKG + ".src.bias")
                    d.lm = bias.BiasedNGram.pair(lm, cb, 0.5).cuda()
            return d
        decs = {"bias": decoder(False, True), "ngram": decoder(True, False), "ngram_bias": decoder(True, True)}
        dec_no = decoder(False, False)
        streams = [torch.cuda.Stream() for _ in range(min(U, 16))]
        rows = [xs[u].contiguous() for u in range(U)]

        def no_scorer():
            main_s = torch.cuda.current_stream()
            fetch = []
            for u in range(U):
                s = streams[u % len(streams)]
                s.wait_stream(main_s)
                with torch.cuda.stream(s):
                    fetch.append((s, dec_no.search_device(rows[u], t_start=0, defer=True)))
            out = []
            for s, f in fetch:
                with torch.cuda.stream(s):
                    out.append(f())
            for s in streams:
                main_s.wait_stream(s)
            return out
        lens = [args.T] * U
        variants = {k: (lambda d=d: d.search_device_batch(xs, lens)) for k, d in decs.items()}
        variants["no_scorer"] = no_scorer
        with torch.no_grad():
            times = NB.median_rounds(variants)
        rec = {"V": V, "U": U, "T": args.T, "beam": args.beam, "cand": args.cand}
        for k, (t, rounds) in times.items():
            rec[k] = {"s_per_batch": t, "utt_per_s": U / t, "utt_per_s_rounds": [U / x for x in rounds]}
        res["ctc_search"].append(rec)
        print(json.dumps(rec))


def bench_transducer(res, models):
    tr = importlib.import_module(PKG + ".src.transducer")
    V, B, T, D = 5000, 32, 100, 512
    lm, cb, both = models[V]
    torch.manual_seed(0)
    head = tr.TransducerHead(V, D, dict(module="LSTM", dim=512, layer=1, emb_dim=256, dropout=0), 512).cuda().eval()
    enc = torch.randn((B, T, D), device="cuda")
    lens = torch.full((B,), T, dtype=torch.int64, device="cuda")
    run = lambda lm_, w: (lambda: head.beam_search(enc, lens, 8, 3, 50, nbest=8, lm=lm_, lm_weight=w))
    both3 = importlib.import_module(PKG + ".src.bias").BiasedNGram.pair(lm, cb, 0.3).cuda()
    with torch.no_grad():
        times = NB.median_rounds({"no_scorer": run(None, 0.0), "bias": run(cb, 1.0), "ngram": run(lm, 0.3),
                                  "ngram_bias": run(both3, 0.3)})
    rec = {"workload": "32 utterances of 100 encoder frames, V 5000, LSTM head 512, beam 8, max_symbols 3, max_len 50, "
                       "random weights"}
    for k, (t, rounds) in times.items():
        rec[k] = {"ms_per_search": t * 1e3, "utt_per_s": B / t, "utt_per_s_rounds": [B / x for x in rounds]}
    res["transducer_beam8"] = rec
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bias.json"))
    ap.add_argument("--skip-search", action="store_true")
    ap.add_argument("--T", type=int, default=200)
    ap.add_argument("--beam", type=int, default=20)
    ap.add_argument("--cand", type=int, default=30)
    ap.add_argument("--U", type=int, default=16)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bias_bench.py measures on the GPU; none found")
    res = {"config": vars(args), "hbm_floor_bytes_per_s": NB.HBM_BYTES_PER_S, "step_kernels": [], "ctc_search": []}
    models = bench_kernels(res)
    if not args.skip_search:
        bench_ctc(res, models, args)
        bench_transducer(res, models)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
