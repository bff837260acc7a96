"""From text to a fused n-gram decode with nothing but this checkout.

    python tools/ngram_lm.py encode TEXT OUT.ids --config config/libri/asr_example.yaml
    python tools/ngram_lm.py estimate OUT.ids LM.arpa --order 3
    python tools/ngram_lm.py build LM.arpa LM.ngram.npz --vocab-size V

`encode` writes a corpus as lines of token ids with the project's tokenizer (the `data.text` block of the ASR
config), so that any ARPA estimator can be run on it elsewhere; `estimate` is a small interpolated Witten-Bell
estimator written in back-off form (numpy only): properly normalised models for the tests and a way to an ARPA file
when no other estimator is at hand; `build` turns an ARPA file into the saved trie image NGramLM.load reads (parsing
a multi-million-entry ARPA file in Python takes minutes: pay it once).  The decoders take either file as `lm_path`
(`.arpa`, `.arpa.gz`, `.ngram.npz`)."""
import argparse
import gzip
import importlib
import math
import os
import sys
from collections import defaultdict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "end-to-end-asr-pytorch_amd"
SOS, EOS, UNK = 0, 1, 2
NAMES = {SOS: "<s>", EOS: "</s>", UNK: "<unk>"}


def witten_bell(sentences, order):
    """sentences: lists of token ids (no <s> / </s>).  Interpolated Witten-Bell, p(w | h) = (c(hw) + t(h) p(w | h')) /
    (c(h) + t(h)) with t(h) the number of distinct words seen after h, in back-off form: an explicit entry for every
    seen h.w and bo(h) = t(h) / (c(h) + t(h)), which makes the back-off recursion reproduce the interpolated value of
    an unseen word exactly.  The unigram level interpolates with the uniform distribution over the words that get a
    unigram (the seen ones, </s> and <unk>); <s> is written with log10 p = -99 as ARPA files do.
    -> grams[k - 1]: {k-tuple: (log10 p, log10 bo or None)}"""
    counts = [defaultdict(int) for _ in range(order)]
    for s in sentences:
        seq = [SOS] + [int(t) for t in s] + [EOS]
        for i in range(1, len(seq)):
            for k in range(1, order + 1):
                if i - k + 1 >= 0:
                    counts[k - 1][tuple(seq[i - k + 1:i + 1])] += 1
    ctx_c = [defaultdict(int) for _ in range(order)]          # per context length: c(h), t(h)
    ctx_t = [defaultdict(int) for _ in range(order)]
    for k in range(order):
        for g, c in counts[k].items():
            ctx_c[k][g[:-1]] += c
            ctx_t[k][g[:-1]] += 1
    words = sorted(set(g[0] for g in counts[0]) | {EOS, UNK})
    c0, t0 = ctx_c[0][()], ctx_t[0][()]
    uni = np.array([counts[0].get((w,), 0) for w in words], np.float64)
    p_uni = dict(zip(words, (uni + t0 / len(words)) / (c0 + t0)))

    def p_int(g):                                             # float64, by the definition above
        if len(g) == 1:
            return p_uni[g[0]]
        h = g[:-1]
        c, t = ctx_c[len(h)].get(h, 0), ctx_t[len(h)].get(h, 0)
        if c == 0:
            return p_int(g[1:])
        return (counts[len(g) - 1].get(g, 0) + t * p_int(g[1:])) / (c + t)

    def bo(h):
        if len(h) >= order:
            return None
        c, t = ctx_c[len(h)].get(h, 0), ctx_t[len(h)].get(h, 0)
        return None if c == 0 else math.log10(t / (c + t))

    grams = [dict() for _ in range(order)]
    grams[0][(SOS,)] = (-99.0, bo((SOS,)))
    for w in words:
        grams[0][(w,)] = (math.log10(p_uni[w]), bo((w,)))
    for k in range(1, order):
        for g in counts[k]:
            grams[k][g] = (math.log10(p_int(g)), bo(g))
    return grams


def write_arpa(grams, path):
    opener = gzip.open if str(path).endswith(".gz") else open
    name = lambda t: NAMES.get(t, str(t))
    with opener(path, "wt", encoding="utf-8") as f:
        f.write("\\data\\\n")
        for k, g in enumerate(grams, 1):
            f.write("ngram %d=%d\n" % (k, len(g)))
        for k, g in enumerate(grams, 1):
            f.write("\n\\%d-grams:\n" % k)
            for key in sorted(g):
                lp, b = g[key]
                f.write("%.15g\t%s" % (lp, " ".join(name(t) for t in key)))
                f.write("\n" if b is None else "\t%.15g\n" % b)
        f.write("\n\\end\\\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    e = sub.add_parser("encode")
    e.add_argument("text")
    e.add_argument("out")
    e.add_argument("--config", required=True)
    s = sub.add_parser("estimate")
    s.add_argument("ids")
    s.add_argument("out")
    s.add_argument("--order", type=int, default=3)
    b = sub.add_parser("build")
    b.add_argument("arpa")
    b.add_argument("out")
    b.add_argument("--vocab-size", type=int, required=True)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    if args.cmd == "encode":
        import yaml
        cfg = yaml.load(open(args.config), Loader=yaml.FullLoader)["data"]["text"]
        tok = importlib.import_module(PKG + ".src.text").load_text_encoder(**cfg)
        n = 0
        with open(args.text) as f, open(args.out, "w") as o:
            for line in f:
                ids = [int(t) for t in tok.encode(line.strip()) if int(t) not in (SOS, EOS)]
                if ids:
                    o.write(" ".join(NAMES.get(t, str(t)) for t in ids) + "\n")
                    n += 1
        print("%d lines, vocabulary of %d tokens -> %s" % (n, tok.vocab_size, args.out))
    elif args.cmd == "estimate":
        if not 1 <= args.order <= 8:
            ap.error("--order must be in 1..8")
        sents = [[UNK if t == "<unk>" else int(t) for t in line.split()] for line in open(args.ids) if line.strip()]
        grams = witten_bell(sents, args.order)
        write_arpa(grams, args.out)
        print("%s: %s n-grams" % (args.out, " / ".join(str(len(g)) for g in grams)))
    else:
        if not args.out.endswith(".ngram.npz"):
            ap.error("the image's name must end in .ngram.npz (that is how the decoders recognise it)")
        ngram = importlib.import_module(PKG + ".src.ngram")
        lm = ngram.NGramLM.from_arpa(args.arpa, args.vocab_size)
        lm.save(args.out)
        print("\n".join(lm.create_msg()))


if __name__ == "__main__":
    main()
