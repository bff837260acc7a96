"""Contextual biasing: a list of phrases (names, product terms, a contact list) boosted in all three beam searches.

The phrases are compiled into an Aho-Corasick automaton over the model's tokens.  A hypothesis earns a bonus while it
walks into a phrase, keeps it when the phrase completes and loses it when the match breaks.  To the searches this is
one more external scorer behind the contract of the n-gram LM (src/ngram.py): one small state per row, one token fed
per row, one dense [rows, V] matrix back that the search adds with a weight.  The state is ONE int32 (a node) and the
step (csrc/ctx_bias.hip) is one row expansion: a dense fill plus the sparse overwrites of the node's transitions.

Semantics.  Nodes are numbered breadth first with children in ascending token order (node 0 = the
root; a fail link points to a smaller id).  end[n]: a phrase ends at n.  The edge into n carries e[n] = weight *
scale * max(multiplier of the phrases through it).  In float64, stored as float32:

    full[n]   = full[parent] + e[n]                      the whole phrase's bonus
    psi[n]    = phi[parent] + e[n]
    phi[n]    = 0 if end[n] else psi[n]                  the pending, not yet banked bonus
    credit[n] = 0 if end[n] else full[f], f the nearest node with end[f] on n's fail chain (0 if none)
    arrive[n] = psi[n] + credit[n],  arrive[0] = phi[0] = 0

and the step is delta(s, v) = arrive[goto(s, v)] - phi[s], ONE float32 subtraction of the two stored values.  Summed
along a token sequence the deltas telescope to (banked phrases) + phi[final state]; phi[final state] is the residual
of a hypothesis that stops mid-phrase.  Overlapping completions are both counted.

* `parse_phrases` reads the phrase file (UTF-8, one phrase per line, optional <TAB>multiplier, `#` comments);
* `build_image` compiles phrases into the flat image the kernels walk (phi; dense root tables; per node the merged
  transitions of its fail chain as a CSR list, deepest node first);
* `ContextBias` holds the image as device buffers behind NGramLM's call contract; `BiasedNGram` pairs it with an
  NGramLM in one launch that writes the row once (asrk_ngram_bias_step_f32).
"""
import math

import numpy as np
import torch
from torch import nn

SUFFIX = '.bias.npz'
DEFAULT_WEIGHT = 1.5
SPECIAL_TOKENS = (0, 1, 2)               # <pad>/<sos>, <eos>, <unk>: a phrase that holds one is dropped
TABLE_KEYS = ('phi', 'root_arrive', 'root_next', 'ext_off', 'ext_word', 'ext_arrive', 'ext_next')
PHRASE_KEYS = ('ph_tok', 'ph_off', 'ph_mult')
_DTYPES = dict(phi=np.float32, root_arrive=np.float32, root_next=np.int32, ext_off=np.int32, ext_word=np.int32,
               ext_arrive=np.float32, ext_next=np.int32, ph_tok=np.int32, ph_off=np.int64, ph_mult=np.float64)


def is_bias_path(path):
    """the decoders' rule: this file name is a saved image, every other `decode.bias.path` a phrase file"""
    return isinstance(path, str) and path.endswith(SUFFIX)


def tokenizer_encode(tokenizer):
    """str -> token ids of the model's text encoder (src/text.py) without the <eos> its encode() appends"""
    def encode(text):
        ids = [int(t) for t in tokenizer.encode(text)]
        return ids[:-1] if ids and ids[-1] == 1 else ids
    return encode


def parse_phrases(path, encode):
    """-> (phrases, n_dropped): phrases = [(token tuple, multiplier)] in file order.  `encode`: str -> token ids.
    A phrase that encodes to nothing or holds token 0, 1 or 2 is dropped and counted; ValueError for a multiplier
    that is no float > 0 and for a file that leaves no phrase."""
    phrases, dropped = [], 0
    with open(path, 'r', encoding='utf-8') as f:
        for line_no, line in enumerate(f, 1):
            line = line.rstrip('\r\n')
            if not line.strip() or line.lstrip().startswith('#'):
                continue
            text, mult = line, 1.0
            if '\t' in line:
                text, field = line.split('\t', 1)
                try:
                    mult = float(field.strip())
                except ValueError:
                    mult = float('nan')
                if not (mult > 0 and math.isfinite(mult)):
                    raise ValueError("%s line %d: multiplier %r is not a number > 0" % (path, line_no, field))
            ids = tuple(int(t) for t in encode(text.strip()))
            if not ids or any(t in SPECIAL_TOKENS for t in ids):
                dropped += 1
                continue
            phrases.append((ids, mult))
    if not phrases:
        raise ValueError("%s holds no usable phrase (%d dropped)" % (path, dropped))
    return phrases, dropped


def build_image(phrases, vocab_size, weight, scale=1.0, n_dropped=0):
    """the flat automaton image (numpy arrays, see the module docstring) of phrases = [(token ids, multiplier)];
    every edge bonus is weight * scale * multiplier in float64 (scale = 1 / lm_weight folds the search's weight)"""
    V, weight, scale = int(vocab_size), float(weight), float(scale)
    if not (weight > 0 and math.isfinite(weight) and scale > 0 and math.isfinite(scale)):
        raise ValueError("bias weight and scale must be finite and > 0, got %r, %r" % (weight, scale))
    phrases = [(tuple(int(t) for t in p), float(m)) for p, m in phrases]
    if not phrases:
        raise ValueError("contextual biasing needs at least one phrase")
    for p, m in phrases:
        if not p or not (m > 0 and math.isfinite(m)):
            raise ValueError("bias phrase %r: empty, or multiplier %r not > 0" % (p, m))
        if any(t < 0 or t >= V for t in p):
            raise ValueError("bias phrase %r holds a token outside the vocabulary [0, %d)" % (p, V))
    # trie with provisional ids, then breadth-first numbering with children in ascending token order
    kids, mult, ends = [{}], [0.0], [False]
    for p, m in phrases:
        n = 0
        for t in p:
            c = kids[n].get(t)
            if c is None:
                c = len(kids)
                kids[n][t] = c
                kids.append({})
                mult.append(0.0)
                ends.append(False)
            mult[c] = max(mult[c], m)
            n = c
        ends[n] = True
    order, new_id = [0], {0: 0}
    for old in order:                                       # the list grows while it is walked: breadth first
        for t in sorted(kids[old]):
            new_id[kids[old][t]] = len(order)
            order.append(kids[old][t])
    N = len(order)
    child = [dict() for _ in range(N)]
    parent, end, e = [0] * N, [False] * N, [0.0] * N
    for old in order:
        n = new_id[old]
        end[n] = ends[old]
        e[n] = weight * mult[old] * scale
        for t, c in kids[old].items():
            child[n][t] = new_id[c]
            parent[new_id[c]] = n
    fail, tok_of = [0] * N, [0] * N
    for n in range(N):
        for t, c in child[n].items():
            tok_of[c] = t
    for n in range(1, N):                                   # parents come first in breadth-first order
        p = parent[n]
        if p == 0:
            continue
        f = fail[p]
        while f != 0 and tok_of[n] not in child[f]:
            f = fail[f]
        fail[n] = child[f].get(tok_of[n], 0)
    full, psi, phi, arrive = [0.0] * N, [0.0] * N, [0.0] * N, [0.0] * N
    for n in range(1, N):
        full[n] = full[parent[n]] + e[n]
        psi[n] = phi[parent[n]] + e[n]
        phi[n] = 0.0 if end[n] else psi[n]
        credit = 0.0
        if not end[n]:
            f = fail[n]
            while f != 0 and not end[f]:
                f = fail[f]
            credit = full[f] if f != 0 else 0.0
        arrive[n] = psi[n] + credit
    root_arrive = np.zeros(V, np.float64)
    root_next = np.zeros(V, np.int32)
    for t, c in child[0].items():
        root_next[t], root_arrive[t] = c, arrive[c]
    ext_off = np.zeros(N + 1, np.int64)
    words, arrs, nexts = [], [], []
    for n in range(1, N):
        merged, m = {}, n
        while m != 0:                                       # the deepest node of the chain wins a word
            for t, c in child[m].items():
                merged.setdefault(t, c)
            m = fail[m]
        for t in sorted(merged):
            words.append(t)
            arrs.append(arrive[merged[t]])
            nexts.append(merged[t])
        ext_off[n + 1] = len(words)
    ext_off[1] = 0
    if len(words) >= 2 ** 31:
        raise ValueError("bias image: %d merged transitions do not fit int32 offsets" % len(words))
    image = dict(vocab_size=V, weight=weight, scale=scale, n_phrases=len(set(p for p, _ in phrases)),
                 n_dropped=int(n_dropped), phi=np.asarray(phi, np.float64).astype(np.float32),
                 root_arrive=root_arrive.astype(np.float32), root_next=root_next, ext_off=ext_off.astype(np.int32),
                 ext_word=np.asarray(words, np.int32), ext_arrive=np.asarray(arrs, np.float64).astype(np.float32),
                 ext_next=np.asarray(nexts, np.int32),
                 ph_tok=np.asarray([t for p, _ in phrases for t in p], np.int32),
                 ph_off=np.cumsum([0] + [len(p) for p, _ in phrases]).astype(np.int64),
                 ph_mult=np.asarray([m for _, m in phrases], np.float64))
    check_image(image)
    return image


def image_phrases(image):
    """the phrase list an image was built from"""
    off = image['ph_off']
    return [(tuple(int(t) for t in image['ph_tok'][off[i]:off[i + 1]]), float(image['ph_mult'][i]))
            for i in range(len(off) - 1)]


def check_image(image):
    """every index the kernels follow stays inside the image (a saved file may come from anywhere)"""
    V = int(image['vocab_size'])
    for k in TABLE_KEYS + PHRASE_KEYS:
        if not isinstance(image.get(k), np.ndarray) or image[k].dtype != _DTYPES[k] or image[k].ndim != 1:
            raise ValueError("bias image: %s must be a 1-d %s array" % (k, np.dtype(_DTYPES[k]).name))
    N, E = len(image['phi']), len(image['ext_word'])
    weight, scale = float(image['weight']), float(image['scale'])
    ok = (V > 0 and N >= 1 and len(image['root_arrive']) == V and len(image['root_next']) == V
          and len(image['ext_off']) == N + 1 and len(image['ext_arrive']) == E and len(image['ext_next']) == E
          and weight > 0 and math.isfinite(weight) and scale > 0 and math.isfinite(scale))
    if ok:
        off = image['ext_off'].astype(np.int64)
        ok = off[0] == 0 and off[-1] == E and bool((np.diff(off) >= 0).all()) and off[1] == 0
        ok = ok and image['phi'][0] == 0 and bool(np.isfinite(image['phi']).all()) \
            and bool(np.isfinite(image['root_arrive']).all()) and bool(np.isfinite(image['ext_arrive']).all())
        for k in ('root_next', 'ext_next'):
            ok = ok and bool(((image[k] >= 0) & (image[k] < N)).all())
        ok = ok and bool(((image['ext_word'] >= 0) & (image['ext_word'] < V)).all())
        if ok and E:                                        # words ascend strictly inside a node: the binary search,
            same = np.repeat(np.arange(N), np.diff(off))    # and one lane per word in the overwrite pass
            ok = bool((np.diff(image['ext_word'].astype(np.int64))[same[1:] == same[:-1]] > 0).all())
    if ok:
        po, P = image['ph_off'], len(image['ph_mult'])
        ok = (len(po) == P + 1 and P >= 1 and po[0] == 0 and po[-1] == len(image['ph_tok'])
              and bool((np.diff(po) > 0).all()) and bool(((image['ph_tok'] >= 0) & (image['ph_tok'] < V)).all())
              and bool((image['ph_mult'] > 0).all()) and bool(np.isfinite(image['ph_mult']).all()))
    if not ok:
        raise ValueError("bias image is inconsistent (sizes, offsets, links, word order or phrase list)")


def _launch_args(x, hidden, parent, out, state_out, dev, V, width):
    """the argument handling NGramLM.forward does, for a state of `width` int32 per row"""
    B, L = x.shape
    assert L == 1, "the biasing automaton is stepped one token per row"
    tok = x.to(device=dev, dtype=torch.int64).contiguous()
    n_state, par, par64 = 0, None, 0
    if hidden is not None:
        assert hidden.dtype == torch.int32 and hidden.numel() % width == 0
        hidden = hidden.to(dev).contiguous()
        n_state = hidden.numel() // width
        if parent is not None:
            assert parent.dtype in (torch.int32, torch.int64) and parent.numel() == B
            par, par64 = parent.to(dev).contiguous(), int(parent.dtype == torch.int64)
        else:
            assert n_state == B
    if out is None:
        out = torch.empty((B, 1, V), dtype=torch.float32, device=dev)
    else:
        assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == B * V
        out = out.view(B, 1, V)
    if state_out is None:
        state = torch.empty((1, B, width), dtype=torch.int32, device=dev)
    else:
        assert state_out.dtype == torch.int32 and state_out.is_contiguous() and state_out.numel() == B * width
        state = state_out.view(1, B, width)
    return B, tok, hidden, n_state, par, par64, out, state


class ContextBias(nn.Module):
    """The automaton image as device buffers + the step kernel, behind NGramLM's decode-time contract."""
    returns_logp = True                  # forward() returns what the search adds: no log_softmax on top
    rnn_type = 'BIAS'                    # neither 'LSTM' nor 'GRU': one state tensor (BeamDecoder asks)
    state_width = 1                      # int32 per row

    def __init__(self, image):
        super().__init__()
        check_image(image)
        self.vocab_size = int(image['vocab_size'])
        self.weight, self.scale = float(image['weight']), float(image['scale'])
        self.n_phrases, self.n_dropped = int(image['n_phrases']), int(image['n_dropped'])
        self.src = ''
        self._phrases = {k: np.ascontiguousarray(image[k]) for k in PHRASE_KEYS}
        for k in TABLE_KEYS:
            self.register_buffer('img_' + k, torch.from_numpy(np.ascontiguousarray(image[k])), persistent=False)

    # ---- construction ------------------------------------------------------------------------------------------
    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            image = {k: z[k] for k in TABLE_KEYS + PHRASE_KEYS}
            for k, t in (('vocab_size', int), ('n_phrases', int), ('n_dropped', int), ('weight', float), ('scale', float)):
                image[k] = t(z[k])
        return cls(image)

    @classmethod
    def from_file(cls, path, vocab_size, weight=None, scale=1.0, encode=None):
        """what the decoders call: a saved image (`.bias.npz`, checked against the vocabulary size; rebuilt from its
        phrase list when `weight` or `scale` differ from what it was saved with) or a phrase file (`encode` needed)"""
        if is_bias_path(path):
            cb = cls.load(path)
            if cb.vocab_size != int(vocab_size):
                raise ValueError("%s was built for %d tokens, the model has %d" % (path, cb.vocab_size, vocab_size))
            weight = cb.weight if weight is None else float(weight)
            if weight != cb.weight or float(scale) != cb.scale:
                cb = cb.rebuilt(weight, scale)
        else:
            if encode is None:
                raise ValueError("a phrase file needs the model's text encoder; only %s files stand alone" % SUFFIX)
            phrases, dropped = parse_phrases(path, encode)
            cb = cls(build_image(phrases, vocab_size, DEFAULT_WEIGHT if weight is None else weight, scale, dropped))
        cb.src = str(path)
        return cb

    def rebuilt(self, weight=None, scale=1.0):
        """the same phrases with another weight / scale (BiasedNGram folds 1 / lm_weight into the image)"""
        img = self.image()
        cb = ContextBias(build_image(image_phrases(img), self.vocab_size, self.weight if weight is None else weight,
                                     scale, self.n_dropped))
        cb.src = self.src
        return cb.to(self.img_phi.device)

    def image(self):
        img = {k: getattr(self, 'img_' + k).cpu().numpy() for k in TABLE_KEYS}
        img.update(self._phrases)
        img.update(vocab_size=self.vocab_size, weight=self.weight, scale=self.scale, n_phrases=self.n_phrases,
                   n_dropped=self.n_dropped)
        return img

    def save(self, path):
        img = self.image()
        with open(path, 'wb') as f:                          # a file object: numpy appends no suffix of its own
            np.savez(f, vocab_size=np.int32(self.vocab_size), n_phrases=np.int32(self.n_phrases),
                     n_dropped=np.int32(self.n_dropped), weight=np.float64(self.weight), scale=np.float64(self.scale),
                     **{k: img[k] for k in TABLE_KEYS + PHRASE_KEYS})

    def create_msg(self):
        return ['           |Contextual biasing enabled \t| weight = {:.2f}\t| src = {}'.format(self.weight, self.src),
                '           |  # of phrases = {}, # of nodes = {}, # of dropped phrases = {}'.format(
                    self.n_phrases, self.img_phi.numel(), self.n_dropped)]

    def _tables(self):
        from .. import ops
        p = ops._p
        return (self.img_phi.numel(), self.img_ext_word.numel(), p(self.img_phi), p(self.img_root_arrive),
                p(self.img_root_next), p(self.img_ext_off), p(self.img_ext_word), p(self.img_ext_arrive),
                p(self.img_ext_next))

    def _device(self, what):
        dev = self.img_phi.device
        if dev.type != 'cuda':
            raise RuntimeError("%s runs on the GPU (csrc/ctx_bias.hip); move the module there first" % what)
        return dev

    # ---- the step ----------------------------------------------------------------------------------------------
    def forward(self, x, lens=None, hidden=None, parent=None, out=None, state_out=None):
        ''' NGramLM.forward's contract: x [B,1] token ids, hidden None (every row starts at the root) or the int32
            state [1,rows,1] of an earlier call, parent None or [B] int32 / int64 -> (delta [B,1,V] float32, state
            [1,B,1] int32); out / state_out: the caller's contiguous storage to write them into '''
        from .. import _lib, ops
        dev = self._device("ContextBias.forward")
        B, tok, hidden, n_state, par, par64, out, state = _launch_args(x, hidden, parent, out, state_out, dev,
                                                                       self.vocab_size, 1)
        p = ops._p
        _lib.check(_lib.load().asrk_bias_step_f32(
            self.vocab_size, *self._tables(), p(hidden), n_state, p(tok), p(par), par64, p(state), p(out),
            self.vocab_size, B, ops._stream()), "bias_step")
        return out, state

    def walk(self, tokens, n_tok):
        ''' tokens [H, L] token ids, n_tok [H] -> (final state int32 [H], total float32 [H], residual float32 [H]):
            every sequence walked from the root, `total` the float32 sum of its deltas in token order, `residual` the
            pending bonus phi[final state] of a hypothesis that stops there '''
        from .. import _lib, ops
        dev = self._device("ContextBias.walk")
        H, L = tokens.shape
        tok = tokens.to(device=dev, dtype=torch.int64).contiguous()
        n = n_tok.to(device=dev, dtype=torch.int32).contiguous().view(-1)
        assert n.numel() == H
        state = torch.empty((H,), dtype=torch.int32, device=dev)
        total = torch.empty((H,), dtype=torch.float32, device=dev)
        residual = torch.empty((H,), dtype=torch.float32, device=dev)
        p = ops._p
        _lib.check(_lib.load().asrk_bias_walk(
            self.vocab_size, *self._tables(), p(tok) if L > 0 and H > 0 else None, L, p(n), L, H, p(state), p(total),
            p(residual), ops._stream()), "bias_walk")
        return state, total, residual


class BiasedNGram(nn.Module):
    """An NGramLM and a ContextBias behind one scorer: row[v] = L(v) + delta(s, v), the row written once
    (asrk_ngram_bias_step_f32).  The search multiplies the row by lm_weight, so `bias` must have been built with
    scale = 1 / lm_weight (`pair` does that).  State: [1, B, 2] int32 (n-gram node, automaton node)."""
    returns_logp = True
    rnn_type = 'NGRAM+BIAS'
    state_width = 2

    def __init__(self, ngram, bias):
        super().__init__()
        if ngram.vocab_size != bias.vocab_size:
            raise ValueError("the n-gram LM has %d tokens, the bias list %d" % (ngram.vocab_size, bias.vocab_size))
        self.ngram, self.bias = ngram, bias
        self.vocab_size = ngram.vocab_size
        self.order = ngram.order

    @classmethod
    def pair(cls, ngram, bias, lm_weight):
        """`bias` rebuilt with its bonuses divided by lm_weight, beside `ngram`"""
        return cls(ngram, bias.rebuilt(scale=1.0 / float(lm_weight)))

    def create_msg(self):
        return self.ngram.create_msg() + self.bias.create_msg()

    def walk(self, tokens, n_tok):
        return self.bias.walk(tokens, n_tok)

    def forward(self, x, lens=None, hidden=None, parent=None, out=None, state_out=None):
        from .. import _lib, ops
        g, b = self.ngram, self.bias
        dev = b._device("BiasedNGram.forward")
        if g.img_bo.device != dev:
            raise RuntimeError("BiasedNGram: the n-gram image and the bias image are on different devices")
        B, tok, hidden, n_state, par, par64, out, state = _launch_args(x, hidden, parent, out, state_out, dev,
                                                                       self.vocab_size, 2)
        p = ops._p
        _lib.check(_lib.load().asrk_ngram_bias_step_f32(
            g.order, g.vocab_size, g.img_bo.numel(), g.img_word.numel(), p(g.img_uni_logp), p(g.img_uni_next),
            p(g.img_bo), p(g.img_fail), p(g.img_child_off), p(g.img_word), p(g.img_logp), p(g.img_next),
            *b._tables(), p(hidden), n_state, p(tok), p(par), par64, p(state), p(out), self.vocab_size, B,
            ops._stream()), "ngram_bias_step")
        return out, state


def attach_bias(decoder, bias):
    """put `bias` (a ContextBias built with scale 1) into the scorer slot of a BeamDecoder / CTCBeamDecoder: alone the
    search adds its rows with weight exactly 1.0; beside the n-gram LM the two become one BiasedNGram whose bias image
    holds every bonus divided by lm_weight.  An RNN-LM cannot be combined with it."""
    from .ngram import NGramLM
    if not isinstance(bias, ContextBias):
        raise TypeError("bias must be a ContextBias, got %s" % type(bias).__name__)
    if bias.vocab_size != decoder.asr.vocab_size:
        raise ValueError("the bias list was built for %d tokens, the model has %d" % (
            bias.vocab_size, decoder.asr.vocab_size))
    decoder.lm_w_config = decoder.lm_w if decoder.apply_lm else 0
    if decoder.apply_lm:
        if not isinstance(decoder.lm, NGramLM):
            raise ValueError("contextual biasing cannot be combined with an RNN-LM")
        decoder.lm = BiasedNGram.pair(decoder.lm, bias, decoder.lm_w)
    else:
        decoder.apply_lm, decoder.lm_w, decoder.lm_path = True, 1.0, ''
        decoder.lm = bias
    decoder.lm.eval()


def install_bias(decoder, bias, device):
    """attach_bias on a decoder that exists already (the solver's: built by its parent class from the decode block)"""
    decoder.bias = bias
    decoder.device = device
    attach_bias(decoder, bias)
    decoder.lm.to(device)


def scorer_state_width(lm):
    """int32 per row of an external scorer's state (NGramLM: 1)"""
    return int(getattr(lm, 'state_width', 1))


def take_bias_block(dcfg):
    """removes `bias` from the decode block (the rest reaches the beam decoders as keyword arguments) and returns
    {path, weight} or None.  ValueError for a malformed block."""
    block = dcfg.pop('bias', None)
    if block is None:
        return None
    if not isinstance(block, dict) or set(block) - {'path', 'weight'}:
        raise ValueError("decode.bias: expected a mapping with `path` and optionally `weight`, got %r" % (block,))
    path, weight = block.get('path'), block.get('weight', DEFAULT_WEIGHT)
    if not isinstance(path, str) or not path:
        raise ValueError("decode.bias: path must name a phrase file or a %s image, got %r" % (SUFFIX, path))
    ok = not isinstance(weight, bool) and isinstance(weight, (int, float)) and math.isfinite(weight) and weight > 0
    if not ok:
        raise ValueError("decode.bias: weight must be a finite number > 0, got %r" % (weight,))
    return {'path': path, 'weight': float(weight)}


def check_bias_config(dcfg, bias, transducer=None, greedy=False):
    """the combinations contextual biasing excludes, checked at set-up: `dcfg` the decode block, `bias` what
    take_bias_block returned, `transducer` the transducer options (or None), `greedy` a CTC / attention decode
    without a beam search"""
    if bias is None:
        return
    from .ngram import is_ngram_path
    if dcfg.get('lm_weight', 0.0) > 0 and not is_ngram_path(dcfg.get('lm_path')):
        raise ValueError("decode.bias cannot be combined with an RNN-LM (lm_weight > 0 with a non-n-gram lm_path)")
    if (dcfg.get('rescore') or {}).get('enable', False):
        raise ValueError("decode.bias cannot be combined with decode.rescore")
    if transducer is not None and transducer.get('align', False):
        raise ValueError("decode.bias cannot be combined with decode.transducer.align")
    if greedy:
        raise ValueError("decode.bias needs a beam search: greedy CTC / attention decoding cannot use it")
