"""Kernel times of the word-embedding plug-in (csrc/emb_fuse.hip) at the shipped shape - N = 16 x 100 decoder rows,
V = 16000 labels, E = 300 embedding dimensions - next to the existing log-softmax forward / backward on the same [N,V]
as the memory-bound yardstick.

    python tools/emb_fuse_bench.py [--out profiles/emb_fuse.json] [--N 1600] [--V 16000] [--E 300]

Times are device events around back-to-back launches on preallocated buffers (no allocation, no host sync inside the
window; as many launches as fill `--window-s`, a quarter of a second), the median of `--windows` windows after a warm-up of every shape; the spread (min / max window) is
recorded with it.  Bytes are the algorithmic HBM traffic computed from the shapes (each [N,V] tensor once per kernel:
3 for the fusion forward, 5 for its backward; re-reads of a row inside a kernel come from the cache), so GB/s = those
bytes over the time, and the share is of the 6.29 TB/s a float4 copy reaches on this chip.  Needs the GPU: without one
it fails."""
import argparse
import ctypes
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "end-to-end-asr-pytorch_amd"
COPY_TBS = 6.29     # measured float4-copy bandwidth of the MI355X, TB/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--N", type=int, default=1600)
    ap.add_argument("--V", type=int, default=16000)
    ap.add_argument("--E", type=int, default=300)
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--window-s", type=float, default=0.25, help="least length of a timed window, seconds")
    ap.add_argument("--windows", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("emb_fuse_bench needs the MI355X: a CPU run measures nothing")
    lib = importlib.import_module(PKG + "._lib")
    ops = importlib.import_module(PKG + ".ops")
    L = lib.load()
    N, V, E, B = args.N, args.V, args.E, args.B
    assert N % B == 0
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)
    d, e, gy = 3.0 * rnd(N, V), rnd(N, V), rnd(N, V)
    y, dd, de = torch.empty_like(d), torch.empty_like(d), torch.empty_like(d)
    stats = torch.empty(N, 4, device=dev)
    t1, l1 = torch.tensor([2.0], device=dev), torch.tensor([0.3], device=dev)
    tv, lv = (1.0 + rnd(V)).contiguous(), rnd(V)
    dt1, dl1, dtv, dlv = torch.empty(1, device=dev), torch.empty(1, device=dev), torch.empty(V, device=dev), \
        torch.empty(V, device=dev)
    nws = max(int(L.asrk_emb_fuse_bwd_ws_bytes(N, V, V, V, 1, 1)), 4)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    x, table = rnd(N, E), rnd(V, E)
    label = torch.randint(1, V, (B, N // B), generator=g).to(dev)
    label[:, -7:] = 0
    row_loss, count, closs = torch.empty(N, device=dev), torch.empty(B, device=dev), torch.empty(1, device=dev)
    dx, dy, one = torch.empty_like(x), torch.empty_like(x), torch.ones(1, device=dev)
    tgt = label.reshape(-1).contiguous()
    sums = torch.empty(2, device=dev)
    p, s = ops._p, ops._stream
    z = ctypes.c_void_p(0)

    def fuse_fwd(t, l, logit):
        return lambda: L.asrk_emb_fuse_fwd_f32(p(d), V, p(e), p(t), t.numel(), p(l), l.numel(), logit, 1e-8, N, V,
                                               p(y), p(stats), s())

    def fuse_bwd(t, l, logit, dt, dl):
        return lambda: L.asrk_emb_fuse_bwd_f32(p(gy), p(d), V, p(e), p(t), t.numel(), p(l), l.numel(), logit, 1e-8,
                                               p(stats), N, V, p(dd), p(de), p(dt) if dt is not None else z,
                                               p(dl) if dl is not None else z, p(ws), nws, s())
    nv = 4.0 * N * V
    cases = [
        ("log_softmax_fwd", lambda: L.asrk_log_softmax_fwd_f32(p(d), p(y), N, V, V, s()), 2 * nv),
        ("log_softmax_bwd", lambda: L.asrk_log_softmax_bwd_f32(p(y), p(gy), p(dd), N, V, V, s()), 3 * nv),
        ("fuse_fwd_fixed", fuse_fwd(t1, l1, 0), 3 * nv),
        ("fuse_fwd_vocabwise", fuse_fwd(tv, lv, 1), 3 * nv),
        ("fuse_bwd_fixed", fuse_bwd(t1, l1, 0, None, None), 5 * nv),
        ("fuse_bwd_scalar_learnable", fuse_bwd(t1, l1, 1, dt1, dl1), 5 * nv),
        ("fuse_bwd_vocabwise_learnable", fuse_bwd(tv, lv, 1, dtv, dlv), 8 * nv),     # + the column pass: g, d, e again
        ("nll_fwd", lambda: L.asrk_nll_loss_fwd_f32(p(y), N, V, V, p(tgt), 0, p(sums), s()), 4.0 * N * 16),
        ("nll_bwd", lambda: L.asrk_nll_loss_bwd_f32(N, V, V, p(tgt), 0, p(one), p(dd), s()), nv),
        ("cos_emb_loss_fwd", lambda: L.asrk_cos_emb_loss_fwd_f32(p(x), p(table), V, p(label), B, N // B, E,
                                                                  p(row_loss), p(count), p(closs), s()), 8.0 * N * E),
        ("cos_emb_loss_bwd", lambda: L.asrk_cos_emb_loss_bwd_f32(p(x), p(table), V, p(label), B, N // B, E, p(count),
                                                                  p(one), p(dx), p(dy), s()), 16.0 * N * E),
    ]
    for _, fn, _ in cases:                      # warm up every shape; a non-zero return code is an error, not a time
        for _ in range(3):
            lib.check(fn(), "warm-up")
    torch.cuda.synchronize()
    ops.check_errors()
    def window(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps
    # launches per window: enough for --window-s of device time, from a 50-launch trial of each kernel
    reps = {name: max(50, int(args.window_s * 1e3 / max(window(fn, 50), 1e-4)) + 1) for name, fn, _ in cases}
    times = {name: [] for name, _, _ in cases}
    for _ in range(args.windows):               # windows of all kernels alternate: drift hits every kernel alike
        for name, fn, _ in cases:
            times[name].append(window(fn, reps[name]))
    res = {"shape": {"N": N, "V": V, "E": E, "B": B}, "window_s": args.window_s, "windows": args.windows,
           "device": torch.cuda.get_device_name(0), "copy_bandwidth_TBs": COPY_TBS,
           "method": "device events around back-to-back launches filling `window_s` seconds, median over `windows` "
                     "windows; bytes = algorithmic traffic from the shapes (an upper bound on HBM traffic: buffers "
                     "that fit the 256 MB Infinity Cache between launches are served from it)", "kernels": {}}
    for name, _, nbytes in cases:
        ts = sorted(times[name])
        med = ts[len(ts) // 2]
        gbs = nbytes / (med * 1e-3) / 1e9
        res["kernels"][name] = {"launches_per_window": reps[name], "ms": round(med, 5), "ms_min": round(ts[0], 5),
                                "ms_max": round(ts[-1], 5),
                                "bytes": int(nbytes), "GBs": round(gbs, 1),
                                "share_of_copy_bandwidth": round(gbs / (COPY_TBS * 1e3), 3)}
        print("%-30s %9.4f ms  [%8.4f .. %8.4f]  %8.1f GB/s  %5.1f %% of copy" % (
            name, med, ts[0], ts[-1], gbs, 100 * gbs / (COPY_TBS * 1e3)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
    print(json.dumps({"emb_fuse_bench": {k: v["ms"] for k, v in res["kernels"].items()}}))


if __name__ == "__main__":
    main()
