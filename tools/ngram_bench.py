"""N-gram LM shallow fusion: the step kernel alone and the whole CTC search.

    python tools/ngram_bench.py [--out profiles/ngram_lm.json] [--skip-search]

1. asrk_ngram_step_f32 alone on a synthetic 4-gram (fan-out per level below), R in {20, 320, 512} rows, V in {5000,
   16000}: kernel time (24 launches replayed as one graph, so that no host call sits between them), achieved bytes/s
   and the share of the 8 TB/s HBM floor, and the time of NGramLM.forward called back to back from Python.  The bytes
   are computed here from shapes: R * V * 4 written + V * 4 (the unigram table, read once from HBM) + 8 bytes (word,
   logp) per explicit entry of every row's back-off chain.
2. the lock-step CTC prefix beam search of tools/ctc_beam_bench.py --lm-batch 16 (beam 20, 30 candidates, T = 200) on
   the same posteriors with the n-gram LM, with the 2 x LSTM-1024 RNN-LM and with no LM (one launch per utterance on
   16 streams, as CTCBeamDecoder.forward_batch runs them), in utterances per second.
Every figure: warmed, device events around a synchronised window of at least 0.5 s, the variants alternated over three
rounds inside this one call; the median is reported with the rounds beside it.  Needs the GPU."""
import argparse
import importlib
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "end-to-end-asr-pytorch_amd"
HBM_BYTES_PER_S = 8.0e12
FANOUT = dict(hot_words=200, bigrams_per_hot_word=120, trigram_contexts=4000, trigrams_per_context=30,
              fourgram_contexts=2000, fourgrams_per_context=10)


def synthetic_tables(V, seed=0):
    """a 4-gram over V ids: every one of `hot_words` contexts holds 120 bigrams (20 of them onto hot words), 4000 of
    those hot bigrams hold 30 trigrams each, 2000 hot trigrams hold 10 four-grams each; values are random"""
    rng = np.random.RandomState(seed)
    f = FANOUT
    val = lambda: (float(rng.uniform(-9.0, -0.5)), float(rng.uniform(-1.0, 0.0)))
    grams = [dict() for _ in range(4)]
    for w in range(1, V):
        grams[0][(w,)] = val()
    grams[0][(0,)] = (-99.0 * np.log(10.0), -0.3)
    hot = [int(w) for w in rng.choice(np.arange(3, V), size=f["hot_words"], replace=False)]
    hot_bi, hot_after = [], {}
    for a in hot:
        to_hot = hot_after[a] = [int(w) for w in rng.choice(hot, size=20, replace=False)]
        others = [int(w) for w in rng.choice(np.arange(3, V), size=f["bigrams_per_hot_word"] - 20, replace=False)]
        for b in to_hot + others:
            grams[1][(a, b)] = val()
        hot_bi += [(a, b) for b in to_hot]
    tri_ctx = [hot_bi[i] for i in rng.choice(len(hot_bi), size=f["trigram_contexts"], replace=False)]
    hot_tri = []
    for h in tri_ctx:
        ws = [int(w) for w in rng.choice(np.arange(3, V), size=f["trigrams_per_context"] - 4, replace=False)]
        nxt = hot_after[h[1]][:4]                                       # (h[1], c) is a hot bigram: the suffix exists
        for c in ws + nxt:
            grams[2][h + (c,)] = val()
        hot_tri += [h + (c,) for c in nxt]
    for i in rng.choice(len(hot_tri), size=f["fourgram_contexts"], replace=False):
        for w in rng.choice(np.arange(3, V), size=f["fourgrams_per_context"], replace=False):
            grams[3][hot_tri[i] + (int(w),)] = val()
    return grams


def chain_entries(image, states):
    """explicit entries on the back-off chain of every state (what step 4 of the kernel reads)"""
    kids = np.diff(image["child_off"].astype(np.int64))
    n = np.zeros(len(states), np.int64)
    s = states.astype(np.int64).copy()
    for _ in range(8):
        n += kids[s]
        s = image["fail"][s].astype(np.int64)
    return n


def step_bytes(R, V, entries):
    return R * V * 4 + V * 4 + int(entries) * 8


def timed_window(fn, min_s=0.5):
    """fn enqueues one call; -> seconds per call from device events around >= min_s of back-to-back calls"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 4
    while True:
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        t = a.elapsed_time(b) * 1e-3
        if t >= min_s:
            return t / n
        n = max(n * 2, int(n * 1.2 * min_s / max(t, 1e-6)) + 1)


def raw_step(lm, st, tok, state_out, out):
    """asrk_ngram_step_f32 into caller buffers: the launch without NGramLM.forward's two allocations"""
    _lib = importlib.import_module(PKG + "._lib")
    ops = importlib.import_module(PKG + ".ops")
    p = ops._p
    _lib.check(_lib.load().asrk_ngram_step_f32(
        lm.order, lm.vocab_size, lm.img_bo.numel(), lm.img_word.numel(), p(lm.img_uni_logp), p(lm.img_uni_next),
        p(lm.img_bo), p(lm.img_fail), p(lm.img_child_off), p(lm.img_word), p(lm.img_logp), p(lm.img_next), p(st),
        st.numel(), p(tok), None, 0, p(state_out), p(out), lm.vocab_size, tok.numel(), ops._stream()), "ngram_step")


GRAPH_CALLS = 24


def graph_of_steps(lm, st, tok, calls=GRAPH_CALLS, buffers=8):
    """`calls` launches captured into one graph (a plain chain, replayed without a host call per launch), writing
    `buffers` output matrices in turn so that a replay does not keep rewriting lines the caches still hold
    (8 x 33 MB at R = 512, V = 16000 against a 256 MB last-level cache).  -> (graph, tensors it uses)"""
    R = tok.numel()
    outs = [torch.empty((R, lm.vocab_size), dtype=torch.float32, device="cuda") for _ in range(buffers)]
    state_out = torch.empty(R, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        raw_step(lm, st, tok, state_out, outs[0])
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(calls):
            raw_step(lm, st, tok, state_out, outs[i % buffers])
    return g, (outs, state_out)


def median_rounds(variants, rounds=3):
    """variants: {name: fn}; the variants are alternated `rounds` times -> {name: (median, [rounds])}"""
    got = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            got[k].append(timed_window(fn))
    return {k: (float(np.median(v)), v) for k, v in got.items()}


class Stub:
    enable_ctc = True

    def __init__(self, V):
        self.vocab_size = V


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ngram_lm.json"))
    ap.add_argument("--skip-search", action="store_true")
    ap.add_argument("--T", type=int, default=200)
    ap.add_argument("--beam", type=int, default=20)
    ap.add_argument("--cand", type=int, default=30)
    ap.add_argument("--U", type=int, default=16)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/ngram_bench.py measures on the GPU; none found")
    ngram = importlib.import_module(PKG + ".src.ngram")
    ctc = importlib.import_module(PKG + ".src.ctc")
    res = {"config": vars(args), "fanout": FANOUT, "hbm_floor_bytes_per_s": HBM_BYTES_PER_S, "step_kernel": [],
           "ctc_search": []}
    tmp = tempfile.mkdtemp()
    lm_files = {}
    for V in (5000, 16000):
        image = ngram.build_image(4, synthetic_tables(V), V)
        lm = ngram.NGramLM(image).cuda()
        lm_files[V] = os.path.join(tmp, "synthetic%d.ngram.npz" % V)
        lm.save(lm_files[V])
        kids = np.diff(image["child_off"])
        depth = np.zeros(len(image["bo"]), np.int64)
        for s in range(1, len(depth)):
            depth[s] = depth[image["fail"][s]] + 1                     # fail[s] < s
        model = {"V": V, "contexts": int(len(depth)), "entries": int(len(image["word"])),
                 "contexts_per_depth": np.bincount(depth).tolist(),
                 "mean_children_per_depth": [float(kids[depth == d].mean()) for d in range(1, 4)]}
        rng = np.random.RandomState(1)
        owner = np.repeat(np.arange(len(depth)), kids)
        nxt = image["next"].astype(np.int64)
        deep = np.nonzero((depth[nxt] == 3) & (kids[nxt] > 0) & (depth[owner] == 2))[0]   # entries that lead to a full chain
        variants, meta, graphs = {}, {}, []
        for R in (20, 320, 512):
            # 80 % of the rows step into a three-word context that has entries at every level (the most a row can
            # read), the others are random (state, token) pairs, most of which fall back to the unigram level
            e = rng.choice(deep, size=R)
            full = rng.rand(R) < 0.8
            states = np.where(full, owner[e], rng.randint(0, len(depth), size=R))
            tokens = np.where(full, image["word"][e], rng.randint(3, V, size=R))
            st = torch.from_numpy(states.astype(np.int32)).view(1, R, 1).cuda()
            tok = torch.from_numpy(tokens.astype(np.int64)).view(R, 1).cuda()
            _, new = lm(tok, None, hidden=st)
            entries = int(chain_entries(image, new.view(-1).cpu().numpy()).sum())
            meta[R] = step_bytes(R, V, entries), entries
            variants[("call", R)] = (lambda tok=tok, st=st: lm(tok, None, hidden=st))
            graph, keep = graph_of_steps(lm, st.view(-1), tok.view(-1))
            graphs.append((graph, keep))
            variants[("kernel", R)] = graph.replay
        times = median_rounds(variants)
        for R in (20, 320, 512):
            nbytes, entries = meta[R]
            t_call, r_call = times[("call", R)]
            t_k, r_k = times[("kernel", R)]
            t_k, r_k = t_k / GRAPH_CALLS, [x / GRAPH_CALLS for x in r_k]
            res["step_kernel"].append({
                "model": model, "V": V, "R": R, "bytes": nbytes, "chain_entries": entries,
                "kernel_us": t_k * 1e6, "kernel_us_rounds": [x * 1e6 for x in r_k], "bytes_per_s": nbytes / t_k,
                "share_of_hbm_floor": (nbytes / HBM_BYTES_PER_S) / t_k,
                "forward_call_us": t_call * 1e6, "forward_call_us_rounds": [x * 1e6 for x in r_call],
                "note": "kernel_us: %d launches replayed as one graph, per launch; forward_call_us: NGramLM.forward "
                        "(two allocations + one launch) called back to back from Python - bound by the host when it "
                        "exceeds kernel_us" % GRAPH_CALLS})
            print(json.dumps(res["step_kernel"][-1]))

    if not args.skip_search:
        import yaml
        lm_mod = importlib.import_module(PKG + ".src.lm")
        U = args.U
        for V in (5000, 16000):
            def posteriors(seed):                                       # tools/ctc_beam_bench.py's generator
                g = torch.Generator().manual_seed(seed)
                logits = torch.randn(args.T, V, generator=g) * 1.5
                logits[:, 0] += 9.0
                spikes = torch.randperm(args.T, generator=g)[:args.T // 4]
                logits[spikes, 0] -= 9.0
                return torch.log_softmax(logits, -1)
            xs = torch.stack([posteriors(u) for u in range(U)]).cuda()
            vr = [1] + list(range(3, V))
            lm_cfg = dict(emb_tying=False, emb_dim=1024, module="LSTM", dim=1024, n_layers=2, dropout=0.0)
            torch.manual_seed(3)
            yaml.safe_dump({"model": lm_cfg}, open(os.path.join(tmp, "lm.yaml"), "w"))
            torch.save({"model": lm_mod.RNNLM(V, **lm_cfg).state_dict()}, os.path.join(tmp, "lm.pth"))
            dec_rnn = ctc.CTCBeamDecoder(Stub(V), vr, args.beam, args.cand, lm_path=os.path.join(tmp, "lm.pth"),
                                         lm_config=os.path.join(tmp, "lm.yaml"), lm_weight=0.5, device="cuda")
            dec_ng = ctc.CTCBeamDecoder(Stub(V), vr, args.beam, args.cand, lm_path=lm_files[V], lm_config="",
                                        lm_weight=0.5, device="cuda")
            dec_no = ctc.CTCBeamDecoder(Stub(V), vr, args.beam, args.cand)
            streams = [torch.cuda.Stream() for _ in range(min(U, 16))]
            rows = [xs[u].contiguous() for u in range(U)]

            def no_lm():
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
            with torch.no_grad():
                times = median_rounds({"ngram_lm": lambda: dec_ng.search_device_batch(xs, lens),
                                       "rnn_lm_2xLSTM1024": lambda: dec_rnn.search_device_batch(xs, lens),
                                       "no_lm": no_lm})
            rec = {"V": V, "U": U, "T": args.T, "beam": args.beam, "cand": args.cand}
            for k, (t, rounds) in times.items():
                rec[k] = {"s_per_batch": t, "utt_per_s": U / t, "utt_per_s_rounds": [U / x for x in rounds]}
            r = {k: rec[k]["utt_per_s"] for k in times}
            rec["ngram_between_rnn_and_no_lm"] = bool(r["rnn_lm_2xLSTM1024"] <= r["ngram_lm"] <= r["no_lm"])
            res["ctc_search"].append(rec)
            print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
