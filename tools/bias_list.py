"""Contextual biasing: compile a phrase list once.

    python tools/bias_list.py build PHRASES.txt LIST.bias.npz --config config/libri/asr_example.yaml [--weight 1.5]
    python tools/bias_list.py show LIST.bias.npz

`build` encodes every line of PHRASES.txt (UTF-8, one phrase per line, an optional <TAB>multiplier, `#` comments) with
the project's tokenizer (the `data.text` block of the ASR config), compiles the automaton (src/bias.py) and saves the
image ContextBias.load reads; the decoders take either file as `decode.bias.path`.  `show` prints what an image holds."""
import argparse
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "end-to-end-asr-pytorch_amd"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    b = sub.add_parser("build")
    b.add_argument("phrases")
    b.add_argument("out")
    b.add_argument("--config", required=True)
    b.add_argument("--weight", type=float, default=None)
    s = sub.add_parser("show")
    s.add_argument("image")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    bias = importlib.import_module(PKG + ".src.bias")
    if args.cmd == "build":
        if not bias.is_bias_path(args.out):
            ap.error("the image's name must end in %s (that is how the decoders recognise it)" % bias.SUFFIX)
        import yaml
        cfg = yaml.load(open(args.config), Loader=yaml.FullLoader)["data"]["text"]
        tok = importlib.import_module(PKG + ".src.text").load_text_encoder(**cfg)
        cb = bias.ContextBias.from_file(args.phrases, tok.vocab_size, weight=args.weight,
                                        encode=bias.tokenizer_encode(tok))
        cb.save(args.out)
    else:
        cb = bias.ContextBias.load(args.image)
        cb.src = args.image
        print("vocabulary of %d tokens, %d merged transitions" % (cb.vocab_size, cb.img_ext_word.numel()))
    print("\n".join(cb.create_msg()))


if __name__ == "__main__":
    main()
