#!/usr/bin/env python
"""RNN-transducer head (src/transducer.py, csrc/rnnt.hip) timed on the GPU -> profiles/rnnt.json.

    python tools/rnnt_bench.py [--rounds 5] [--window 0.5] [--steps 3] [--skip-step] [--out profiles/rnnt.json]

Loss: ops.RNNTLoss forward + backward (consume_logits: rows pass, lattice, gradient pass in place) on [32, 200, 65, 5000]
and [16, 200, 65, 16000] logits, every utterance full length, against the composed path one would write from the ops
that existed before: ops.log_softmax, the two gathers, the lattice kernel, the sparse gradient of the gathered
log-probabilities scattered by autograd, the dense log-softmax backward.  Both give the same gradient (the largest
difference is recorded).  The HBM floor is three passes over the logits (two reads, one write) at 8 TB/s.
Joint: ops.RNNTJointFn forward + backward on [32, 200, 65, 512] against the bytes it must move (forward: read E and P,
write H; backward: read H and dH once per output, write dE and dP).
Greedy: ASR.transducer_greedy on 32 utterances of 8 s (cfg3 encoder, LSTM-512 prediction network, joint 512), encoder
included, and the search alone on the encoder's output.
Step: a cfg3-shaped training step with the head (weight 0.3) against the plain step of the same commit.

Variants alternate in one process; a figure is the median over `rounds` windows of at least `window` seconds of
back-to-back calls between two device events, after a warm-up of every shape.
Recognition accuracy is not measured: no corpus with transcripts is available to this repository's tools."""
import argparse
import importlib
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "end-to-end-asr-pytorch_amd"
HBM_PEAK = 8.0e12


def _once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def alternate(variants, rounds, window):
    reps = {}
    for k, fn in variants.items():
        for _ in range(2):
            fn()
        reps[k] = max(1, int(math.ceil(window / max(_once(fn), 1e-6))))
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps[name]):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / reps[name])
    return {k: {"ms_per_call_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v), "reps": reps[k]}
            for k, v in times.items()}


class _Producer(torch.autograd.Function):
    """stands for the producer of the logits (the vocabulary projection): hands them on as a non-leaf and takes their
    gradient without touching it.  (A leaf would make autograd's accumulation CLONE a gradient that aliases the
    logits - two more passes over the tensor that no training step has.)"""

    @staticmethod
    def forward(ctx, x, hook):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return None, None


def bench_loss(lib, ops, B, T, U1, V, rounds, window):
    dev = "cuda"
    torch.manual_seed(0)
    U = U1 - 1
    x0 = torch.randn((B, T, U1, V), device=dev) * 3.0
    txt = torch.randint(1, V, (B, U), device=dev)
    el = torch.full((B,), T, dtype=torch.int64, device=dev)
    tl = torch.full((B,), U, dtype=torch.int64, device=dev)
    crit = ops.RNNTLoss(blank=0)
    p, s = ops._p, ops._stream
    x = x0.clone()
    out = {}

    hook = torch.zeros((), device=dev, requires_grad=True)

    def fused():
        # (in place: the next call reads the previous gradient as logits - the same traffic, finite values)
        crit(_Producer.apply(x, hook), txt, el, tl, consume_logits=True).backward()

    def composed(leaf=None):
        xg = leaf if leaf is not None else _Producer.apply(x, hook)
        lp = ops.log_softmax(xg.view(-1, V)).view(B, T, U1, V)
        lpb = lp[..., 0]
        lpl = lp[:, :, :U].gather(3, txt.view(B, 1, U, 1).expand(B, T, U, 1)).squeeze(3)
        with torch.no_grad():
            lpb_c = lpb.contiguous()
            lpl_c = torch.zeros((B, T, U1), device=dev)
            lpl_c[:, :, :U] = lpl
            alpha, beta = torch.empty_like(lpb_c), torch.empty_like(lpb_c)
            nll = torch.empty((B,), device=dev)
            assert lib.asrk_rnnt_lattice_f32(p(lpb_c), p(lpl_c), p(el), p(tl), B, T, U1, p(alpha), p(beta), p(nll),
                                             s()) == 0
            bt = torch.full_like(beta, float("-inf"))
            bt[:, :-1] = beta[:, 1:]
            bt[:, T - 1, U] = 0.0
            n = nll.view(B, 1, 1)
            g_b = -torch.exp(alpha + lpb_c + bt + n) / B
            g_l = -torch.exp(alpha[:, :, :U] + lpl + beta[:, :, 1:] + n) / B
        torch.autograd.backward([lpb, lpl], [g_b, g_l])

    # the two paths give the same gradient (on the same logits, as leaves, out of place)
    xc, xg = x0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
    composed(xc)
    crit(xg, txt, el, tl).backward()
    out["max_abs_grad_difference"] = float((xg.grad - xc.grad).abs().max())
    out["max_abs_grad"] = float(xg.grad.abs().max())
    del xc, xg
    nbytes = B * T * U1 * V * 4
    out["shape"] = {"B": B, "T": T, "U1": U1, "V": V, "logit_bytes": nbytes}
    out["timing"] = alternate({"fused": fused, "composed": composed, "fused_again": fused}, rounds, window)
    t = out["timing"]["fused"]["ms_per_call_median"]
    floor_ms = 3 * nbytes / HBM_PEAK * 1e3
    out["hbm_floor_ms_3_passes_at_8TBps"] = floor_ms
    out["fused_over_floor"] = t / floor_ms
    out["fused_GBps_on_3_passes"] = 3 * nbytes / (t * 1e-3) / 1e9
    out["composed_over_fused"] = out["timing"]["composed"]["ms_per_call_median"] / t
    out["spread_fused_vs_fused"] = out["timing"]["fused_again"]["ms_per_call_median"] / t
    # the three kernels of the fused path on their own
    lse, lpb, lpl = (torch.empty((B, T, U1), device=dev) for _ in range(3))
    alpha, beta = torch.empty_like(lse), torch.empty_like(lse)
    nll, gs = torch.empty((B,), device=dev), torch.full((B,), 1.0 / B, device=dev)
    x.copy_(x0)

    def rows():
        assert lib.asrk_rnnt_rows_f32(p(x), V, p(txt), U, p(el), p(tl), B, T, U1, V, 0, p(lse), p(lpb), p(lpl), s()) == 0

    def lattice():
        assert lib.asrk_rnnt_lattice_f32(p(lpb), p(lpl), p(el), p(tl), B, T, U1, p(alpha), p(beta), p(nll), s()) == 0
    dz = torch.empty_like(x)

    def grad():
        assert lib.asrk_rnnt_grad_f32(p(x), V, p(txt), U, p(el), p(tl), B, T, U1, V, 0, p(lse), p(lpb), p(lpl), p(alpha),
                                      p(beta), p(nll), p(gs), p(dz), V, s()) == 0
    rows()
    lattice()
    out["kernels"] = alternate({"rows": rows, "lattice": lattice, "grad_out_of_place": grad}, rounds, window / 2)
    out["kernels"]["rows_GBps"] = nbytes / (out["kernels"]["rows"]["ms_per_call_median"] * 1e-3) / 1e9
    out["kernels"]["grad_GBps"] = 2 * nbytes / (out["kernels"]["grad_out_of_place"]["ms_per_call_median"] * 1e-3) / 1e9
    return out


def bench_joint(ops, B, T, U1, J, rounds, window):
    dev = "cuda"
    torch.manual_seed(1)
    E = torch.randn((B, T, J), device=dev, requires_grad=True)
    P = torch.randn((B, U1, J), device=dev, requires_grad=True)
    dH = torch.randn((B, T, U1, J), device=dev)

    def pair():
        H = ops.RNNTJointFn.apply(E, P)
        H.backward(dH)
        E.grad = P.grad = None
    hb = B * T * U1 * J * 4
    small = (B * T * J + B * U1 * J) * 4
    moved = (small + hb) + (4 * hb + small)
    out = {"shape": {"B": B, "T": T, "U1": U1, "J": J, "H_bytes": hb}, "bytes_moved": moved,
           "timing": alternate({"pair": pair}, rounds, window)}
    t = out["timing"]["pair"]["ms_per_call_median"]
    out["floor_ms_at_8TBps"] = moved / HBM_PEAK * 1e3
    out["pair_over_floor"] = t / out["floor_ms_at_8TBps"]
    out["GBps"] = moved / (t * 1e-3) / 1e9
    return out


HEAD = {'enable': True, 'weight': 0.3, 'joint_dim': 512,
        'pred': {'module': 'LSTM', 'dim': 512, 'layer': 1, 'emb_dim': 512, 'dropout': 0}}


def _model(bench, w, dev, head):
    asr = importlib.import_module(PKG + ".src.asr")
    torch.manual_seed(0)
    m = w["model"]
    return asr.ASR(w["D"], w["V"], True, m["ctc_weight"], m["encoder"], m["attention"], m["decoder"],
                   transducer=head).to(dev)


def bench_greedy(bench, rounds, window):
    dev = torch.device("cuda")
    w = dict(bench.WORKLOADS["cfg3"], T=800)                 # 8 s of 10 ms frames
    model = _model(bench, w, dev, HEAD).eval()
    feat, feat_len, _ = bench.synth(w, seed=0, device=dev)
    with torch.no_grad():
        enc, enc_len = model.encoder(feat, feat_len)
    max_len = int(math.ceil(enc.shape[1] * 0.5))

    def whole():
        model.transducer_greedy(feat, feat_len, 3, 0.5)

    def search():
        model.transducer.greedy(enc, enc_len, 3, max_len)
    tokens, n_tok, _ = model.transducer_greedy(feat, feat_len, 3, 0.5)
    out = {"workload": "32 utterances of 8 s (T 800 -> T' %d), V %d, max_symbols 3, max_len %d, random weights" % (
        enc.shape[1], w["V"], max_len), "mean_tokens": float(n_tok.float().mean()),
        "iterations": int(enc.shape[1]) + max_len,
        "timing": alternate({"encoder_and_search": whole, "search_alone": search}, rounds, window)}
    out["utt_per_s_encoder_and_search"] = w["B"] / (out["timing"]["encoder_and_search"]["ms_per_call_median"] * 1e-3)
    out["utt_per_s_search_alone"] = w["B"] / (out["timing"]["search_alone"]["ms_per_call_median"] * 1e-3)
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
            if head:
                logits = model.transducer_logits(encoded[0], enc_len, txt, txt_len)
                total = total + rnnt_fn(logits, txt, enc_len, txt_len, consume_logits=True) * model.rnnt_weight
            total.backward()
            opt.clip_and_step(5.0)
        return step
    torch.cuda.reset_peak_memory_stats()        # the figure below is this section's, both models resident
    plain, with_head = make(None), make(HEAD)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3
    plain()
    with_head()
    times = {"plain": [], "with_head": []}
    for _ in range(rounds):
        times["plain"].append(wall(plain))
        times["with_head"].append(wall(with_head))
    ops.check_errors()
    out = {"workload": "cfg3: B %d, T %d, V %d, L %d; head: weight 0.3, joint 512, LSTM-512 x1; random weights" % (
        w["B"], w["T"], w["V"], w["L"]), "steps_per_window": steps, "rounds": rounds,
        "plain_step_ms_median": statistics.median(times["plain"]),
        "with_head_step_ms_median": statistics.median(times["with_head"]),
        "plain_step_ms_all": times["plain"], "with_head_step_ms_all": times["with_head"],
        "peak_memory_GB": torch.cuda.max_memory_allocated() / 1e9}
    out["ratio"] = out["with_head_step_ms_median"] / out["plain_step_ms_median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rnnt.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/rnnt_bench.py measures on the GPU; none is visible")
    ops = importlib.import_module(PKG + ".ops")
    lib = importlib.import_module(PKG + "._lib").load()
    bench = importlib.import_module("bench")
    res = {"what": "RNN-transducer head: fused loss against the composed path and the HBM floor, the joint pair against "
                   "its bytes, greedy decoding, a cfg3-shaped step with the head against the plain step (device events, "
                   "windows of >= %.2f s, variants alternated per round, medians)" % args.window,
           "command": "python tools/rnnt_bench.py --rounds %d --window %g --steps %d%s" % (
               args.rounds, args.window, args.steps, " --skip-step" if args.skip_step else ""),
           "device": torch.cuda.get_device_name(0)}

    def save():
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    res["loss"] = [bench_loss(lib, ops, 32, 200, 65, 5000, args.rounds, args.window)]
    save()
    torch.cuda.empty_cache()
    res["loss"].append(bench_loss(lib, ops, 16, 200, 65, 16000, args.rounds, args.window))
    save()
    torch.cuda.empty_cache()
    res["joint"] = bench_joint(ops, 32, 200, 65, 512, args.rounds, args.window)
    save()
    res["greedy"] = bench_greedy(bench, args.rounds, args.window)
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
