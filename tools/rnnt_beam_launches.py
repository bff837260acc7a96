#!/usr/bin/env python
"""Kernel launches per iteration of the transducer searches, counted from kernel dispatch traces.

One search per process, so that a trace holds nothing else:

    rocprofv3 --kernel-trace --output-format csv -d DIR/<variant>_<frames> -- \\
        python tools/rnnt_beam_launches.py run <variant> <frames>

for variant in greedy, beam1, beam4, beam8, beam16, beam8_ngram, greedy_stateless, beam8_stateless,
beam8_ngram_stateless and two frame counts (10 and 30); then

    python tools/rnnt_beam_launches.py summarise DIR [--out profiles/rnnt_beam_launches.json]

counts the dispatches of every trace: with max_len fixed the two runs of a variant differ by 20 iterations and nothing
else (the set-up launches cancel), so launches per iteration = (count at 30 frames - count at 10 frames) / 20.  The
count does not depend on the data: every iteration enqueues the same kernels whatever the hypotheses are.
Shape: 32 utterances, the head of tools/rnnt_bench.py (LSTM-512, joint 512, V = 5000) on a random encoder output of
width 1024, max_symbols 3, max_len 10; the n-gram is the synthetic 4-gram of tools/ngram_bench.py.  The *_stateless variants
run the same searches on a head with `pred: {module: stateless, dim: 512, context: 2}`: summarise refuses a result in
which one of them is not strictly below its LSTM counterpart (then something is still moving state)."""
import csv
import glob
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
PKG = "end-to-end-asr-pytorch_amd"
VARIANTS = ("greedy", "beam1", "beam4", "beam8", "beam16", "beam8_ngram", "greedy_stateless", "beam8_stateless",
            "beam8_ngram_stateless")
STATELESS = "_stateless"
FRAMES = (10, 30)
MAX_SYMBOLS, MAX_LEN, B, V, ENC = 3, 10, 32, 5000, 1024


def run(variant, frames):
    import torch
    tr = importlib.import_module(PKG + ".src.transducer")
    torch.manual_seed(0)
    pred = dict(module="LSTM", dim=512, layer=1, emb_dim=512, dropout=0)
    if variant.endswith(STATELESS):
        variant, pred = variant[:-len(STATELESS)], dict(module="stateless", dim=512, context=2, dropout=0)
    head = tr.TransducerHead(V, ENC, pred, 512).cuda().eval()
    enc = torch.randn((B, frames, ENC), device="cuda")
    lens = torch.full((B,), frames, dtype=torch.int64, device="cuda")
    if variant == "greedy":
        head.greedy(enc, lens, MAX_SYMBOLS, MAX_LEN)
    else:
        lm = None
        if variant.endswith("_ngram"):
            ngram = importlib.import_module(PKG + ".src.ngram")
            NB = importlib.import_module("ngram_bench")
            lm = ngram.NGramLM(ngram.build_image(4, NB.synthetic_tables(V), V)).cuda()
        W = int(variant.split("_")[0][4:])
        head.beam_search(enc, lens, W, MAX_SYMBOLS, MAX_LEN, nbest=W, lm=lm, lm_weight=0.3 if lm is not None else 0.0)
    torch.cuda.synchronize()
    importlib.import_module(PKG + ".ops").check_errors()


def dispatches(directory):
    n = 0
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            n += sum(1 for _ in csv.DictReader(f))
    return n


def summarise(root, out):
    res = {"what": "kernel dispatches per search iteration from rocprofv3 --kernel-trace: (count at %d frames - count at "
                   "%d frames) / %d, one search per traced process" % (FRAMES[1], FRAMES[0], FRAMES[1] - FRAMES[0]),
           "shape": "B %d, V %d, LSTM-512 prediction network, joint 512, max_symbols %d, max_len %d" % (
               B, V, MAX_SYMBOLS, MAX_LEN) + "; *_stateless: stateless prediction network, dim 512, context 2",
           "variants": {}}
    for v in VARIANTS:
        counts = [dispatches(os.path.join(root, "%s_%d" % (v, f))) for f in FRAMES]
        if not all(counts):
            raise SystemExit("no kernel trace for %s under %s" % (v, root))
        res["variants"][v] = {"dispatches": dict(zip(map(str, FRAMES), counts)),
                              "launches_per_iteration": (counts[1] - counts[0]) / float(FRAMES[1] - FRAMES[0])}
    for v in VARIANTS:
        if v.endswith(STATELESS):
            mine, theirs = (res["variants"][k]["launches_per_iteration"] for k in (v, v[:-len(STATELESS)]))
            if not mine < theirs:
                raise SystemExit("%s makes %g launches per iteration, the LSTM head %g: not strictly fewer" % (
                    v, mine, theirs))
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res["variants"]))


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "run" and sys.argv[2] in VARIANTS:
        run(sys.argv[2], int(sys.argv[3]))
    elif len(sys.argv) >= 3 and sys.argv[1] == "summarise":
        out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(
            ROOT, "profiles", "rnnt_beam_launches.json")
        summarise(sys.argv[2], out)
    else:
        raise SystemExit(__doc__)
