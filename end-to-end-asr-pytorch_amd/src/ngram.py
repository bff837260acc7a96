"""Back-off n-gram language model (ARPA) for shallow fusion in both beam searches.

The reference fuses an RNN-LM only (src/lm.py); a CTC decoder is usually paired with a back-off n-gram trained on
text alone.  To the searches an LM is three things: a per-row state moved by gather indices, one token fed per row
and one dense [rows, V] matrix of log-probabilities back.  Here the state is ONE int32 (a context node of a trie)
and the step (csrc/ngram.hip, asrk_ngram_step_f32) is a trie walk plus the expansion of one row.

* `parse_arpa` reads plain / gzip ARPA files whose words are the model's token ids as decimal strings
  (`<s>` = 0, `</s>` = 1, `<unk>` = 2), stdlib + numpy only;
* `build_image` turns the n-grams into the flat image the kernel walks (node 0 = empty context; dense unigram
  tables; per node back-off, fail link and a CSR range of children; per child word / logp / next state), after
  completing pruned files so that every context's prefix and suffix is a context too;
* `NGramLM` holds the image as device buffers and has RNNLM's decode-time call contract
  (`forward(x [B,1], lens, hidden) -> (out [B,1,V], state)`), except that `out` is already log-probabilities
  (`returns_logp`): pruned models are not normalised and the decoders must not renormalise them.
"""
import gzip
import math

import numpy as np
import torch
from torch import nn

LN10 = math.log(10.0)
UNSEEN_LOG10 = -99.0                     # score of a predicted word that has no unigram, as ARPA writes <s>
SPECIALS = {'<s>': 0, '</s>': 1, '<unk>': 2}
MAX_ORDER = 8                            # NG_MAX_ORDER of csrc/ngram.inc
SUFFIXES = ('.arpa', '.arpa.gz', '.ngram.npz')
IMAGE_KEYS = ('uni_logp', 'uni_next', 'bo', 'fail', 'child_off', 'word', 'logp', 'next')


def is_ngram_path(path):
    """the decoders' rule: these file names select NGramLM, every other lm_path the RNN-LM"""
    return isinstance(path, str) and path.endswith(SUFFIXES)


def _word_id(word, vocab_size, line_no):
    if word in SPECIALS:
        return SPECIALS[word]
    if not (word.isascii() and word.isdigit()):
        raise ValueError("ARPA line %d: word %r is neither a token id nor <s>, </s>, <unk>" % (line_no, word))
    tok = int(word)
    if tok in (0, 1, 2):
        raise ValueError("ARPA line %d: word %r must be written as %s" % (
            line_no, word, ('<s>', '</s>', '<unk>')[tok]))
    if tok >= vocab_size:
        raise ValueError("ARPA line %d: word %r is outside the vocabulary [0, %d)" % (line_no, word, vocab_size))
    return tok


def parse_arpa(path, vocab_size):
    """-> (order, grams): grams[k - 1] maps a k-tuple of token ids to (ln p, ln back-off) in float64; a missing
    back-off column is 0.  ValueError (naming the word and the line) for a word that is no token id of the model."""
    opener = gzip.open if str(path).endswith('.gz') else open
    declared, grams, cur = {}, {}, 0
    with opener(path, 'rt', encoding='utf-8') as f:
        in_data = False
        for line_no, line in enumerate(f, 1):
            line = line.strip()
            if not line:
                continue
            if line.startswith('\\'):
                if line == '\\data\\':
                    in_data = True
                elif line == '\\end\\':
                    break
                elif line.endswith('-grams:'):
                    cur = int(line[1:line.index('-')])
                    in_data = False
                    grams.setdefault(cur, {})
                else:
                    raise ValueError("ARPA line %d: unknown section %r" % (line_no, line))
                continue
            if in_data:
                if line.startswith('ngram '):
                    k, n = line[6:].split('=')
                    declared[int(k)] = int(n)
                continue
            if cur == 0:
                continue                                    # free text in front of \data\
            fields = line.split()
            if len(fields) not in (cur + 1, cur + 2):
                raise ValueError("ARPA line %d: a %d-gram line has %d fields" % (line_no, cur, len(fields)))
            key = tuple(_word_id(w, vocab_size, line_no) for w in fields[1:cur + 1])
            bo = float(fields[cur + 1]) * LN10 if len(fields) == cur + 2 else 0.0
            grams[cur][key] = (float(fields[0]) * LN10, bo)
    order = max(grams) if grams else 0
    if not 1 <= order <= MAX_ORDER:
        raise ValueError("ARPA order %d is outside 1..%d" % (order, MAX_ORDER))
    for k in range(1, order + 1):
        if k not in grams:
            raise ValueError("ARPA file has no \\%d-grams: section" % k)
        if k in declared and declared[k] != len(grams[k]):
            raise ValueError("ARPA header declares %d %d-grams, the section holds %d" % (declared[k], k, len(grams[k])))
    return order, [grams[k] for k in range(1, order + 1)]


def _backoff_logp(grams, gram):
    """ln p(gram[-1] | gram[:-1]) by the back-off recursion (float64); a word without a unigram has the
    constant ln(10) * -99 at the unigram level"""
    acc = 0.0
    while True:
        hit = grams[len(gram) - 1].get(gram)
        if hit is not None:
            return acc + hit[0]
        if len(gram) == 1:
            return acc + UNSEEN_LOG10 * LN10
        ctx = grams[len(gram) - 2].get(gram[:-1])
        if ctx is not None:
            acc += ctx[1]
        gram = gram[1:]


def complete(grams):
    """Pruned files may lack the prefix or the suffix of an n-gram they hold (`a b c` without `b c`).  Insert each
    missing one with its backed-off probability and a back-off weight of 0 - no probability changes - so that
    every context has its fail link and every entry its context.  Returns the number of n-grams inserted."""
    inserted = 0
    work = [g for k in range(len(grams) - 1, 0, -1) for g in grams[k]]
    while work:
        g = work.pop()
        for part in (g[:-1], g[1:]):
            table = grams[len(part) - 1]
            if part in table:
                continue
            table[part] = (_backoff_logp(grams, part), 0.0)
            inserted += 1
            if len(part) > 1:
                work.append(part)
    return inserted


def build_image(order, grams, vocab_size):
    """the flat trie image (numpy arrays, see the module docstring); `grams` is completed in place first"""
    V = int(vocab_size)
    complete(grams)
    # contexts = every n-gram of order < n; sorted by (length, tokens): a fail link always points to a smaller id
    ctxs = [g for k in range(order - 1) for g in sorted(grams[k])]
    node = {(): 0}
    for g in ctxs:
        node[g] = len(node)
    N = len(node)
    bo = np.zeros(N, np.float32)
    fail = np.zeros(N, np.int32)
    for g in ctxs:
        bo[node[g]] = np.float32(grams[len(g) - 1][g][1])
        fail[node[g]] = node[g[1:]]

    def state_after(g):                                     # longest suffix of g, at most n - 1 tokens, that is a context
        g = g[-(order - 1):] if order > 1 else ()
        while g not in node:
            g = g[1:]
        return node[g]

    uni_logp = np.full(V, np.float32(UNSEEN_LOG10 * LN10), np.float32)
    uni_next = np.zeros(V, np.int32)
    for (w,), (lp, _) in grams[0].items():
        uni_logp[w] = np.float32(lp)
        uni_next[w] = state_after((w,))
    rows = [(node[g[:-1]], g[-1], lp, state_after(g)) for k in range(1, order) for g, (lp, _) in grams[k].items()]
    rows.sort(key=lambda r: (r[0], r[1]))
    E = len(rows)
    word = np.fromiter((r[1] for r in rows), np.int32, E)
    logp = np.fromiter((r[2] for r in rows), np.float64, E).astype(np.float32)
    nxt = np.fromiter((r[3] for r in rows), np.int32, E)
    counts = np.bincount(np.fromiter((r[0] for r in rows), np.int64, E), minlength=N)
    child_off = np.zeros(N + 1, np.int32)
    child_off[1:] = np.cumsum(counts)
    image = dict(order=int(order), vocab_size=V, uni_logp=uni_logp, uni_next=uni_next, bo=bo, fail=fail,
                 child_off=child_off, word=word, logp=logp, next=nxt)
    check_image(image)
    return image


def check_image(image):
    """every index the kernel follows stays inside the image (a saved file may come from anywhere)"""
    order, V = int(image['order']), int(image['vocab_size'])
    dt = dict(uni_logp=np.float32, uni_next=np.int32, bo=np.float32, fail=np.int32, child_off=np.int32,
              word=np.int32, logp=np.float32, next=np.int32)
    for k, t in dt.items():
        if image[k].dtype != t or image[k].ndim != 1:
            raise ValueError("n-gram image: %s must be a 1-d %s array" % (k, np.dtype(t).name))
    N, E = len(image['bo']), len(image['word'])
    ok = (1 <= order <= MAX_ORDER and V > 0 and N >= 1 and len(image['uni_logp']) == V and len(image['uni_next']) == V
          and len(image['fail']) == N and len(image['child_off']) == N + 1 and len(image['logp']) == E
          and len(image['next']) == E)
    if ok:
        off = image['child_off'].astype(np.int64)
        ok = off[0] == 0 and off[-1] == E and bool((np.diff(off) >= 0).all()) and off[1] == 0
        ok = ok and image['fail'][0] == 0 and bool((image['fail'][1:] >= 0).all()) \
            and bool((image['fail'][1:] < np.arange(1, N)).all())
        for k in ('uni_next', 'next'):
            ok = ok and bool(((image[k] >= 0) & (image[k] < N)).all())
        ok = ok and bool(((image['word'] >= 0) & (image['word'] < V)).all())
        if ok and E:                                        # words ascend inside a node: the kernel's binary search
            same = np.repeat(np.arange(N), np.diff(off))
            ok = bool((np.diff(image['word'].astype(np.int64))[same[1:] == same[:-1]] > 0).all())
    if not ok:
        raise ValueError("n-gram image is inconsistent (sizes, offsets, links or word order)")


class NGramLM(nn.Module):
    """The image as device buffers + the step kernel, behind RNNLM's decode-time contract."""
    returns_logp = True                  # forward() returns log-probabilities: no log_softmax on top
    rnn_type = 'NGRAM'                   # neither 'LSTM' nor 'GRU': one state tensor (BeamDecoder asks)

    def __init__(self, image):
        super().__init__()
        check_image(image)
        self.order = int(image['order'])
        self.vocab_size = int(image['vocab_size'])
        for k in IMAGE_KEYS:
            self.register_buffer('img_' + k, torch.from_numpy(np.ascontiguousarray(image[k])), persistent=False)

    # ---- construction ------------------------------------------------------------------------------------------
    @classmethod
    def from_arpa(cls, path, vocab_size):
        order, grams = parse_arpa(path, vocab_size)
        return cls(build_image(order, grams, vocab_size))

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            image = {k: z[k] for k in IMAGE_KEYS}
            image['order'], image['vocab_size'] = int(z['order']), int(z['vocab_size'])
        return cls(image)

    @classmethod
    def from_file(cls, path, vocab_size):
        """what the decoders call for an lm_path that is_ngram_path() accepts"""
        if str(path).endswith('.ngram.npz'):
            lm = cls.load(path)
            if lm.vocab_size != int(vocab_size):
                raise ValueError("%s was built for %d tokens, the model has %d" % (path, lm.vocab_size, vocab_size))
            return lm
        return cls.from_arpa(path, vocab_size)

    def image(self):
        img = {k: getattr(self, 'img_' + k).cpu().numpy() for k in IMAGE_KEYS}
        img['order'], img['vocab_size'] = self.order, self.vocab_size
        return img

    def save(self, path):
        img = self.image()
        with open(path, 'wb') as f:                          # a file object: numpy appends no suffix of its own
            np.savez(f, order=np.int32(self.order), vocab_size=np.int32(self.vocab_size),
                     **{k: img[k] for k in IMAGE_KEYS})

    def create_msg(self):
        return ['Model spec.| {}-gram back-off LM (ARPA), # of contexts = {}, # of higher-order entries = {}'.format(
            self.order, self.img_bo.numel(), self.img_word.numel())]

    # ---- the step ----------------------------------------------------------------------------------------------
    def forward(self, x, lens=None, hidden=None, parent=None, out=None, state_out=None):
        ''' x [B,1] int64 token ids, hidden None (every row starts from the empty context) or the int32 state
            [1,rows,1] of an earlier call, parent None or [B] int32 / int64 (row r continues hidden[parent[r]]: the
            survivors' gather folded into the launch) -> (logp [B,1,V] float32, state [1,B,1] int32).
            out / state_out: contiguous float32 [B*V] / int32 [B] storage of the caller's to write them into '''
        from .. import _lib, ops
        dev = self.img_bo.device
        if dev.type != 'cuda':
            raise RuntimeError("NGramLM.forward runs on the GPU (asrk_ngram_step_f32); move the module there first")
        B, L = x.shape
        assert L == 1, "the n-gram LM is stepped one token per row"
        tok = x.to(device=dev, dtype=torch.int64).contiguous()
        n_state, par, par64 = 0, None, 0
        if hidden is not None:
            assert hidden.dtype == torch.int32
            hidden = hidden.to(dev).contiguous()
            n_state = hidden.numel()
            if parent is not None:
                assert parent.dtype in (torch.int32, torch.int64) and parent.numel() == B
                par, par64 = parent.to(dev).contiguous(), int(parent.dtype == torch.int64)
            else:
                assert n_state == B
        if out is None:
            out = torch.empty((B, 1, self.vocab_size), dtype=torch.float32, device=dev)
        else:
            assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == B * self.vocab_size
            out = out.view(B, 1, self.vocab_size)
        if state_out is None:
            state = torch.empty((1, B, 1), dtype=torch.int32, device=dev)
        else:
            assert state_out.dtype == torch.int32 and state_out.is_contiguous() and state_out.numel() == B
            state = state_out.view(1, B, 1)
        p = ops._p
        _lib.check(_lib.load().asrk_ngram_step_f32(
            self.order, self.vocab_size, self.img_bo.numel(), self.img_word.numel(), p(self.img_uni_logp),
            p(self.img_uni_next), p(self.img_bo), p(self.img_fail), p(self.img_child_off), p(self.img_word),
            p(self.img_logp), p(self.img_next), p(hidden), n_state, p(tok), p(par), par64, p(state), p(out),
            self.vocab_size, B, ops._stream()), "ngram_step")
        return out, state
