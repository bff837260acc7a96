"""Register-traffic audit of the bf16x6 recurrence kernels (no GPU needed, one to two minutes).

    python tools/rec_isa_audit.py [-o report.txt]

Compiles csrc/lstm_rec_fwd_bf.hip and csrc/lstm_rec_bwd_bf.hip with build.py's own HIPCC, ARCH and CFLAGS plus
``-S --cuda-device-only`` into a temporary directory and prints, for every instantiation of
lstm_rec_fwd_bf_kernel / lstm_rec_bwd_bf_kernel:

  * VGPR and AGPR counts, both spill counts and the scratch size from the kernel metadata;
  * the instruction histogram of the fast-path span and of the whole time-step loop.

The time-step loop is the widest backward-branch interval around the kernel's first v_mfma.  The fast path is the
longest run of that loop without a label or a branch that holds MFMAs (the slow path re-polls inside loops, so its runs
are one fragment ring long at the most); the span goes from the first to the last v_mfma of that run: what one wave
executes per step when no sentinel is hit.

Exit status 1 if an instantiation has a VGPR spill, scratch, or a v_readlane_b32 or a compiler-generated
v_accvgpr_read_b32 inside the fast-path span (one inside an inline-assembly statement is the author's, not a copy the
compiler added).  Every instantiation in the two units is one launch_fwd_bf / launch_bwd_bf can select: the
kernels are instantiated by those launchers alone.

It looks at register traffic and spill metadata, nothing else.
"""
import collections
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "end-to-end-asr-pytorch_amd")
UNITS = ("lstm_rec_fwd_bf.hip", "lstm_rec_bwd_bf.hip")
KERNEL_RE = re.compile(r"lstm_rec_(fwd|bwd)_bf_kernelI([A-Za-z0-9_]*?)EEv")
META_KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
             "private_segment_fixed_size")
BRANCH_RE = re.compile(r"^s_(?:c?branch\w*)\s+(\S+)")
# mnemonics listed first in a histogram line; the rest follows by count
WATCHED = ("v_mfma", "v_accvgpr_read_b32", "v_accvgpr_write_b32", "v_accvgpr_mov_b32", "v_readlane_b32",
           "v_writelane_b32", "s_nop", "s_waitcnt", "ds_read_b128", "buffer_load_dwordx4", "scratch_load", "scratch_store")


def pretty_name(mangled):
    m = KERNEL_RE.search(mangled)
    if not m:
        return mangled
    args = []
    for tok in re.findall(r"L([a-z])(n?\d+)E", m.group(2)):
        v = int(tok[1].replace("n", "-"))
        args.append(("true" if v else "false") if tok[0] == "b" else str(v))
    return "lstm_rec_%s_bf_kernel<%s>" % (m.group(1), ",".join(args))


def _metadata(text):
    """{kernel symbol: {key: int}} from the amdhsa.kernels list at the end of the assembly."""
    out, cur = {}, None
    for line in text.splitlines():
        if line.startswith("  - ."):
            cur = {}
            line = "    " + line[4:]
        m = re.match(r"^    \.(\w+):\s+(\S+)\s*$", line)
        if cur is None or not m:
            continue
        if m.group(1) == "name":
            out[m.group(2)] = cur
        elif m.group(1) in META_KEYS:
            cur[m.group(1)] = int(m.group(2))
    return out


class Inst(object):
    __slots__ = ("op", "text", "in_asm")

    def __init__(self, op, text, in_asm):
        self.op, self.text, self.in_asm = op, text, in_asm


def _body(lines):
    """Instructions and labels of one function: [('L', name) | ('I', Inst)]."""
    items, in_asm = [], False
    for raw in lines:
        line = raw.strip()
        if line.startswith(";;#ASMSTART"):
            in_asm = True
            continue
        if line.startswith(";;#ASMEND"):
            in_asm = False
            continue
        line = line.split(";", 1)[0].strip()
        if not line:
            continue
        m = re.match(r"^([.\w$]+):$", line)
        if m:
            items.append(("L", m.group(1)))
            continue
        if line.startswith("."):
            continue
        items.append(("I", Inst(line.split()[0], line, in_asm)))
    return items


def _histogram(insts):
    h = collections.Counter()
    for i in insts:
        op = "v_mfma" if i.op.startswith("v_mfma") else i.op
        for fam in ("scratch_load", "scratch_store"):
            if op.startswith(fam):
                op = fam
        h[op] += 1
    return h


def _analyse(items):
    """Locate the time-step loop and the fast-path span; returns (loop insts, span insts)."""
    label_at = {it[1]: n for n, it in enumerate(items) if it[0] == "L"}
    first_mfma = next((n for n, it in enumerate(items) if it[0] == "I" and it[1].op.startswith("v_mfma")), None)
    if first_mfma is None:
        return [], []
    lo, hi = None, None
    for n, it in enumerate(items):
        if it[0] != "I":
            continue
        m = BRANCH_RE.match(it[1].text)
        if not m or m.group(1) not in label_at:
            continue
        tgt = label_at[m.group(1)]
        if tgt <= first_mfma <= n and (lo is None or n - tgt > hi - lo):
            lo, hi = tgt, n
    if lo is None:                       # no loop around the MFMAs: take the whole function
        lo, hi = 0, len(items) - 1
    loop = items[lo:hi + 1]
    # straight-line runs of the loop
    best, run = [], []
    for it in loop + [("L", None)]:
        if it[0] == "L" or BRANCH_RE.match(it[1].text):
            idx = [k for k, i in enumerate(run) if i.op.startswith("v_mfma")]
            if idx:
                cand = run[idx[0]:idx[-1] + 1]
                if len(idx) > sum(1 for i in best if i.op.startswith("v_mfma")):
                    best = cand
            run = []
        else:
            run.append(it[1])
    return [it[1] for it in loop if it[0] == "I"], best


class KernelAudit(object):
    def __init__(self, symbol, meta, loop, span):
        self.symbol, self.name, self.meta = symbol, pretty_name(symbol), meta
        self.loop, self.span = _histogram(loop), _histogram(span)
        self.loop_len, self.span_len = len(loop), len(span)
        self.span_readlane = sum(1 for i in span if i.op == "v_readlane_b32")
        self.span_compiler_accread = sum(1 for i in span if i.op == "v_accvgpr_read_b32" and not i.in_asm)
        self.span_compiler_accmov = sum(1 for i in span if i.op == "v_accvgpr_mov_b32" and not i.in_asm)

    def violations(self):
        v = []
        if self.meta.get("vgpr_spill_count", 0):
            v.append("%d VGPR spills" % self.meta["vgpr_spill_count"])
        if self.meta.get("private_segment_fixed_size", 0):
            v.append("%d B scratch" % self.meta["private_segment_fixed_size"])
        if self.span_readlane:
            v.append("%d v_readlane_b32 in the fast-path span" % self.span_readlane)
        if self.span_compiler_accread:
            v.append("%d compiler v_accvgpr_read_b32 in the fast-path span" % self.span_compiler_accread)
        return v


def parse(text):
    """All bf16x6 recurrence kernels of one assembly file, in file order."""
    meta = _metadata(text)
    lines = text.splitlines()
    out, n = [], 0
    while n < len(lines):
        m = re.match(r"^(_Z\w+):", lines[n])
        if m and KERNEL_RE.search(m.group(1)):
            end = n + 1
            while end < len(lines) and not lines[end].startswith(".Lfunc_end"):
                end += 1
            loop, span = _analyse(_body(lines[n + 1:end]))
            out.append(KernelAudit(m.group(1), meta.get(m.group(1), {}), loop, span))
            n = end
        n += 1
    return out


def _fmt_hist(h, total, others=None):
    rest = [k for k, _ in h.most_common() if k not in WATCHED]
    keys = [k for k in WATCHED if h.get(k)] + rest[:others]
    tail = ", ... (%d more mnemonics)" % (len(rest) - others) if others is not None and len(rest) > others else ""
    return "%d instructions: %s%s" % (total, ", ".join("%s %d" % (k, h[k]) for k in keys), tail)


def report(kernels):
    """(text, exit status) for a list of KernelAudit."""
    out, bad = [], 0
    for k in kernels:
        m = k.meta
        out.append(k.name)
        out.append("  registers: %d VGPRs of which %d AGPRs, %d SGPRs; spills: %d VGPR, %d SGPR; scratch %d B" % tuple(
            m.get(key, -1) for key in ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count",
                                       "sgpr_spill_count", "private_segment_fixed_size")))
        out.append("  fast-path span: " + _fmt_hist(k.span, k.span_len))
        out.append("    in the span: v_readlane_b32 %d, compiler v_accvgpr_read_b32 %d, compiler v_accvgpr_mov_b32 %d" % (
            k.span_readlane, k.span_compiler_accread, k.span_compiler_accmov))
        out.append("  time-step loop: " + _fmt_hist(k.loop, k.loop_len, others=8))
        v = k.violations()
        out.append("  verdict: " + ("FAIL - " + "; ".join(v) if v else "ok"))
        bad += bool(v)
    out.append("%d kernels, %d failing" % (len(kernels), bad))
    return "\n".join(out) + "\n", 1 if bad or not kernels else 0


def audit_text(text):
    return report(parse(text))


def compile_units(tmpdir, extra=()):
    spec = importlib.util.spec_from_file_location("asrk_build", os.path.join(PKG_DIR, "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    procs = []
    for u in UNITS:
        out = os.path.join(tmpdir, os.path.splitext(u)[0] + ".s")
        cmd = [b.HIPCC] + b.CFLAGS + list(extra) + ["-S", "--cuda-device-only", os.path.join(b.CSRC, u), "-o", out]
        procs.append((out, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)))
    texts = []
    for out, pr in procs:
        _, err = pr.communicate()
        if pr.returncode != 0:
            raise RuntimeError("hipcc failed for %s:\n%s" % (out, err))
        with open(out) as f:
            texts.append(f.read())
    return texts


def main(argv):
    dest = argv[argv.index("-o") + 1] if "-o" in argv else None
    extra = [a for a in argv if a.startswith("-D")]
    with tempfile.TemporaryDirectory() as tmp:
        kernels = [k for t in compile_units(tmp, extra) for k in parse(t)]
    text, status = report(kernels)
    sys.stdout.write(text)
    if dest:
        with open(dest, "w") as f:
            f.write(text)
    return status


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
