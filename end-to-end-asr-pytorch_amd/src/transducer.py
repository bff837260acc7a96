"""RNN-transducer head (Graves 2012) on the pyramidal encoder: embedding + unidirectional LSTM/GRU prediction network
(or the stateless one of Ghodsi et al. 2020: a causal depthwise convolution over the last `context` label embeddings and
a ReLU; csrc/rnnt_ctx.hip), joint network tanh(lin_enc(enc)[b,t] + lin_pred(pred)[b,u]) -> lin_out -> [B, T', U+1, V]
logits for ops.RNNTLoss, and batched greedy decoding with device-resident bookkeeping (csrc/rnnt.hip) and an
alignment-length-synchronous beam search with merged alignments and n-gram LM fusion (csrc/rnnt_beam.hip).
Blank = <sos> = 0.
Forced alignment (lattice_logp, align; csrc/rnnt_align.hip): the best path through the lattice gives every label its
emission frame, log-probability and posterior.
With the `prune:` sub-block the training loss is the pruned one (Kuang et al. 2022; csrc/rnnt_prune.hip): an additive
joiner lin_am(enc)[b,t] + lin_lm(pred)[b,u] on the whole lattice picks `range` label positions per frame, and the joint
network and the loss run on that band only.
"""
import math

import torch
import torch.nn as nn

from .. import ops
from .. import decoder_ops as dops
from .. import gru_ops
from .module import RNNParams


PRED_KEYS = ('module', 'dim', 'layer', 'emb_dim', 'dropout', 'context')
CONTEXT_MAX = 8             # ops.RNNT_CTX_MAX


class ContextParams(nn.Module):
    """Parameter container of the stateless prediction network: `weight` [dim, 1, context] with the name, shape and
    default init of nn.Conv1d(dim, dim, context, groups=dim, bias=False), so a torch module built at the same point of
    the random stream holds the same values.  It never runs ATen's convolution (ops.RNNTContextFn does the work)."""

    def __init__(self, dim, context):
        super().__init__()
        self.dim, self.context = dim, context
        self.weight = nn.Parameter(torch.empty(dim, 1, context))
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))     # uniform(+-1/sqrt(context)), as nn.Conv1d


def transducer_enabled(cfg):
    ''' the `model: transducer:` block is present and not switched off '''
    return bool(cfg) and bool(cfg.get('enable', True))


def check_exclusive(config):
    ''' the transducer head is trained beside CTC (and attention) only: `mwer:` and `emb:` build their losses on the
        attention decoder's hypotheses and are refused together with it '''
    if not transducer_enabled((config.get('model') or {}).get('transducer')):
        return
    mwer = config.get('mwer')
    if isinstance(mwer, dict) and mwer.get('enable', True):
        raise ValueError('config blocks `model: transducer:` and `mwer:` cannot be combined')
    if bool((config.get('emb') or {}).get('enable', False)):
        raise ValueError('config blocks `model: transducer:` and `emb:` cannot be combined')


PRUNE_KEYS = ('enable', 'range', 'simple_weight')
PRUNE_MAX_RANGE = 32


def take_prune_block(block):
    ''' validates the `model: transducer: prune:` sub-block and returns {range, simple_weight} when it is enabled, else
        None.  range (whole number in 2..32, default 5) is the number of label positions kept per frame, simple_weight
        (>= 0, default 0.5) the weight of the simple joiner's loss beside the pruned one. '''
    if block is None:
        return None
    if not isinstance(block, dict):
        raise ValueError('model.transducer.prune: expected a mapping, got %r' % (block,))
    unknown = sorted(set(block) - set(PRUNE_KEYS), key=str)
    if unknown:
        raise ValueError('model.transducer.prune: unknown key(s) {}'.format(unknown))
    opts = {}
    for key, default in (('range', 5), ('simple_weight', 0.5)):
        v = block.get(key, default)
        ok = not isinstance(v, bool) and isinstance(v, (int, float)) and v == v and abs(v) != float('inf')
        if not ok or (key == 'range' and v != int(v)):
            raise ValueError('model.transducer.prune: {} must be a {}, got {!r}'.format(
                key, 'whole number' if key == 'range' else 'finite number', v))
        opts[key] = int(v) if key == 'range' else float(v)
    if not 2 <= opts['range'] <= PRUNE_MAX_RANGE:
        raise ValueError('model.transducer.prune: range must be in 2..{}, got {}'.format(PRUNE_MAX_RANGE, opts['range']))
    if not opts['simple_weight'] >= 0:
        raise ValueError('model.transducer.prune: simple_weight must be >= 0, got {}'.format(opts['simple_weight']))
    if not isinstance(block.get('enable', True), (bool, int)):
        raise ValueError('model.transducer.prune: enable must be true or false, got {!r}'.format(block.get('enable')))
    return opts if block.get('enable', True) else None


def infeasible_utterances(enc_len, txt_len, prune_range):
    ''' indices b with (T_b - 1)(S - 1) < max(0, U_b + 1 - S): a band of S positions that moves at most S - 1 per frame
        cannot cover such a transcript (host lengths) '''
    S = int(prune_range)
    return [b for b, (t, u) in enumerate(zip(enc_len, txt_len))
            if (max(int(t), 1) - 1) * (S - 1) < max(0, int(u) + 1 - S)]


BEAM_KEYS = ('beam_size', 'nbest', 'lm_weight')
ALIGN_KEYS = ('align', 'timestamps')


def take_decode_block(dcfg):
    ''' removes `transducer` from the decode block (the parent solver hands the rest to the beam decoders) and returns
        {max_symbols, max_len_ratio} when it is enabled, else None.  The beam-search keys beam_size (1..32), nbest
        (1..beam_size) and lm_weight (>= 0) are validated and returned only when the block names them: beam_size > 1 or
        lm_weight > 0 selects ASR.transducer_beam, and lm_weight > 0 needs an n-gram `decode.lm_path`.  The same holds
        for the two booleans of the forced alignment (ASR.transducer_align; bin/align_rnnt.py): `align: true` aligns
        every utterance to its reference transcript instead of searching (no beam_size > 1, no lm_weight > 0, no
        timestamps beside it), `timestamps: true` aligns the best hypothesis of the search and writes its token times
        beside the usual output. '''
    block = dcfg.pop('transducer', None) or {}
    if not isinstance(block, dict):
        raise ValueError('decode.transducer: expected a mapping, got %r' % (block,))
    unknown = sorted(set(block) - {'enable', 'max_symbols', 'max_len_ratio'} - set(BEAM_KEYS) - set(ALIGN_KEYS),
                     key=str)
    if unknown:
        raise ValueError('decode.transducer: unknown key(s) {}'.format(unknown))
    if not block.get('enable', False):
        return None
    if dcfg.get('align', False) or (dcfg.get('rescore') or {}).get('enable', False):
        raise ValueError('decode.transducer excludes decode.align and decode.rescore')
    opts = {'max_symbols': int(block.get('max_symbols', 3)), 'max_len_ratio': float(block.get('max_len_ratio', 0.5))}
    if opts['max_symbols'] < 1 or not opts['max_len_ratio'] > 0:
        raise ValueError('decode.transducer: max_symbols must be >= 1 and max_len_ratio > 0')
    for key in BEAM_KEYS:
        if key in block:
            v = block[key]
            ok = not isinstance(v, bool) and isinstance(v, (int, float)) and v == v and abs(v) != float('inf')
            if not ok or (key != 'lm_weight' and v != int(v)):
                raise ValueError('decode.transducer: {} must be a {}, got {!r}'.format(
                    key, 'finite number' if key == 'lm_weight' else 'whole number', v))
            opts[key] = float(v) if key == 'lm_weight' else int(v)
    beam_size = opts.get('beam_size', 1)
    if not 1 <= beam_size <= 32:
        raise ValueError('decode.transducer: beam_size must be in 1..32, got {}'.format(beam_size))
    if not 1 <= opts.get('nbest', 1) <= beam_size:
        raise ValueError('decode.transducer: nbest must be in 1..beam_size, got {}'.format(opts['nbest']))
    if not opts.get('lm_weight', 0.0) >= 0:
        raise ValueError('decode.transducer: lm_weight must be >= 0, got {}'.format(opts['lm_weight']))
    if opts.get('lm_weight', 0.0) > 0:
        from .ngram import is_ngram_path
        if not is_ngram_path(dcfg.get('lm_path')):
            raise ValueError('decode.transducer: lm_weight > 0 fuses an n-gram LM only: decode.lm_path must end in '
                             '.arpa, .arpa.gz or .ngram.npz, got {!r}'.format(dcfg.get('lm_path')))
    for key in ALIGN_KEYS:
        if key in block:
            if not isinstance(block[key], bool):
                raise ValueError('decode.transducer: {} must be true or false, got {!r}'.format(key, block[key]))
            opts[key] = block[key]
    if opts.get('align', False):
        if beam_size > 1 or opts.get('lm_weight', 0.0) > 0 or opts.get('timestamps', False):
            raise ValueError('decode.transducer: align aligns the reference transcripts without a search: it excludes '
                             'beam_size > 1, lm_weight > 0 and timestamps')
    return opts


def uses_beam(opts):
    ''' the decode block (take_decode_block's result) asks for the beam search rather than the greedy one '''
    return bool(opts) and (opts.get('beam_size', 1) > 1 or opts.get('lm_weight', 0.0) > 0 or bool(opts.get('bias')))


class TransducerHead(nn.Module):
    ''' vocab_size: V (index 0 is blank and <sos>); enc_dim: encoder output width;
        pred = {module: LSTM|GRU, dim, layer, emb_dim, dropout} or {module: stateless, dim, context, dropout} (context:
        whole number in 1..8, default 2; the head then owns emb [V, dim] and ctx.weight [dim, 1, context] and no pred.*);
        joint_dim: J;
        prune = {range, simple_weight} (take_prune_block's result) or None: with it the head owns the simple joiner's
        two projections lin_am and lin_lm and forward_pruned is its training forward '''

    def __init__(self, vocab_size, enc_dim, pred, joint_dim, prune=None):
        super().__init__()
        module = str(pred.get('module', 'LSTM')).upper()
        self.stateless = module == 'STATELESS'
        unknown = set(pred) - set(PRED_KEYS if self.stateless else PRED_KEYS[:-1])
        if unknown:
            raise ValueError('transducer: unknown pred keys {}'.format(sorted(unknown, key=str)))
        if module not in ('LSTM', 'GRU', 'STATELESS'):
            raise NotImplementedError("transducer prediction network '{}' is not supported (LSTM / GRU / stateless)"
                                      .format(module))
        self.vocab_size = vocab_size
        self.rnn_type = module
        self.dim = int(pred.get('dim', 512))
        self.layer = int(pred.get('layer', 1))
        self.emb_dim = int(pred.get('emb_dim', self.dim))
        self.dropout = float(pred.get('dropout', 0.0))
        self.joint_dim = int(joint_dim)
        self.blank = 0
        if self.stateless:
            c = pred.get('context', 2)
            if isinstance(c, bool) or not isinstance(c, (int, float)) or c != c or c != int(c) \
                    or not 1 <= int(c) <= CONTEXT_MAX:
                raise ValueError('transducer: pred.context must be a whole number in 1..{}, got {!r}'.format(
                    CONTEXT_MAX, c))
            if self.emb_dim != self.dim:
                raise ValueError('transducer: the stateless prediction network is depthwise: pred.emb_dim ({}) must '
                                 'equal pred.dim ({})'.format(self.emb_dim, self.dim))
            if self.layer != 1:
                raise ValueError('transducer: the stateless prediction network has one layer, got pred.layer = {}'
                                 .format(self.layer))
            self.context = int(c)
            self.emb = nn.Embedding(vocab_size, self.dim)
            self.ctx = ContextParams(self.dim, self.context)
        else:
            self.emb = nn.Embedding(vocab_size, self.emb_dim)
            self.pred = RNNParams(module, self.emb_dim, self.dim, num_layers=self.layer, dropout=self.dropout,
                                  batch_first=True)
        self.lin_enc = nn.Linear(enc_dim, self.joint_dim)
        self.lin_pred = nn.Linear(self.dim, self.joint_dim)
        self.lin_out = nn.Linear(self.joint_dim, vocab_size)
        self.prune = dict(prune) if prune else None
        if self.prune:
            self.lin_am = nn.Linear(enc_dim, vocab_size)
            self.lin_lm = nn.Linear(self.dim, vocab_size)

    def create_msg(self):
        if self.stateless:
            msg = '           | Transducer head enabled ( stateless predictor, context {}, dim {}, joint dim {}).'.format(
                self.context, self.dim, self.joint_dim)
        else:
            msg = '           | Transducer head enabled ( {} x{} dim {}, joint dim {}).'.format(
                self.rnn_type, self.layer, self.dim, self.joint_dim)
        if self.prune:
            msg += ' Pruned loss ( range {}, simple weight {}).'.format(self.prune['range'], self.prune['simple_weight'])
        return msg

    def _predict(self, txt):
        ''' txt [B,U] -> prediction-network output [B,U+1,dim] on <sos> + txt, from a zero state (as
            RNNLM._forward_sequence: unidirectional, so the padded tail changes no valid position) '''
        dev = self.emb.weight.device
        B = txt.shape[0]
        inp = torch.cat([torch.zeros((B, 1), dtype=torch.int64, device=dev), txt.to(device=dev, dtype=torch.int64)],
                        dim=1)
        if self.stateless:      # embedding -> dropout -> context convolution + ReLU: one pass, no recurrence
            return ops.RNNTContextFn.apply(ops.dropout(dops.embedding(inp, self.emb.weight), self.dropout, self.training),
                                           self.ctx.weight)
        h = ops.swap_bt(ops.dropout(dops.embedding(inp, self.emb.weight), self.dropout, self.training))
        for l in range(self.layer):
            if self.rnn_type == 'LSTM':
                h = ops.lstm_layer(h, self.pred.layer_params(l))
            else:
                h = gru_ops.gru_layer(h, self.pred.layer_params(l))
            if l + 1 < self.layer:
                h = ops.dropout(h, self.dropout, self.training)
        return ops.swap_bt(h)

    def forward(self, encode_feature, encode_len, txt, txt_len):
        ''' encode_feature [B,T',D], txt [B,L] padded labels (eos included), txt_len [B] -> logits [B,T',U+1,V] with
            U = L.  encode_len / txt_len are the loss's business: the joint is dense, padded cells get zero gradient
            there.  The [B*T'*(U+1), J] x [J, V] product is ops.linear's (the split-GEMM path at training shapes). '''
        E = ops.linear(encode_feature, self.lin_enc.weight, self.lin_enc.bias)
        P = ops.linear(self._predict(txt), self.lin_pred.weight, self.lin_pred.bias)
        H = ops.RNNTJointFn.apply(E, P)
        return ops.linear(H, self.lin_out.weight, self.lin_out.bias)

    def forward_pruned(self, encode_feature, encode_len, txt, txt_len):
        ''' the pruned training forward -> (pruned nll, simple nll), both means over the B utterances.
            1. the simple joiner lin_am(enc)[b,t] + lin_lm(pred)[b,u] on the whole lattice (ops.RNNTSimpleLossFn: no
               [B,T',U+1,V] tensor) gives its loss and the occupation of every cell;
            2. ops.rnnt_prune_ranges picks the first of the S = prune.range label positions kept at every frame;
            3. the joint network and lin_out run on the band, [B,T',S,V] logits, and ops.RNNTBandLoss is the transducer
               loss with everything outside the band impossible; its backward writes over the logits.
            An utterance with (T_b - 1)(S - 1) < U_b + 1 - S has no path (nll = +inf, zero gradient): with lengths on
            the host that is a ValueError here; device lengths are not read back. '''
        if not self.prune:
            raise RuntimeError('TransducerHead.forward_pruned needs the `model: transducer: prune:` block')
        S = self.prune['range']
        if all(torch.is_tensor(x) and x.device.type == 'cpu' for x in (encode_len, txt_len)):
            bad = infeasible_utterances(encode_len.tolist(), txt_len.tolist(), S)
            if bad:
                raise ValueError('transducer.prune: range {} cannot cover utterance(s) {} (encoder lengths {}, transcript '
                                 'lengths {}): (T - 1)(range - 1) >= U + 1 - range is needed'.format(
                                     S, bad, [int(encode_len[b]) for b in bad], [int(txt_len[b]) for b in bad]))
        pred = self._predict(txt)
        am = ops.linear(encode_feature, self.lin_am.weight, self.lin_am.bias)
        lm = ops.linear(pred, self.lin_lm.weight, self.lin_lm.bias)
        simple_nll, occ = ops.RNNTSimpleLossFn.apply(am, lm, txt, encode_len, txt_len, self.blank)
        s = ops.rnnt_prune_ranges(occ, encode_len, txt_len, S)
        E = ops.linear(encode_feature, self.lin_enc.weight, self.lin_enc.bias)
        P = ops.linear(pred, self.lin_pred.weight, self.lin_pred.bias)
        H = ops.RNNTJointBandFn.apply(E, P, s, S)
        logits = ops.linear(H, self.lin_out.weight, self.lin_out.bias)
        pruned_nll = ops.RNNTBandLossFn.apply(logits, txt, encode_len, txt_len, s, P.shape[1], self.blank, 'mean', True)
        return pruned_nll, simple_nll.mean()

    @torch.no_grad()
    def lattice_logp(self, encode_feature, encode_len, txt, txt_len, max_logits_bytes=1 << 30):
        ''' encode_feature [B,T',D], txt [B,U] padded labels, lengths [B] -> (lpb, lpl) f32 [B,T',U+1]: the
            log-probabilities of blank and of label u + 1 at every lattice cell (zeros outside every lattice), without
            ever holding more than max_logits_bytes of [.., V] logits (one utterance alone may always run).  The
            prediction network runs once; then groups of consecutive utterances go through the joint, lin_out and the
            row pass (ops.rnnt_rows), which writes into slices of the two outputs.  A row's lpb / lpl depend on that row
            alone, so every grouping gives the same bits.  The pruned model's lin_am / lin_lm are not used. '''
        dev = encode_feature.device
        B, T, _ = encode_feature.shape
        txt = torch.as_tensor(txt).to(device=dev, dtype=torch.int64).contiguous()
        U1 = txt.shape[1] + 1
        el = torch.as_tensor(encode_len).to(device=dev, dtype=torch.int64).contiguous()
        tl = torch.as_tensor(txt_len).to(device=dev, dtype=torch.int64).contiguous()
        E = ops.linear(encode_feature, self.lin_enc.weight, self.lin_enc.bias)
        P = ops.linear(self._predict(txt), self.lin_pred.weight, self.lin_pred.bias)
        lpb = torch.empty((B, T, U1), dtype=torch.float32, device=dev)
        lpl = torch.empty((B, T, U1), dtype=torch.float32, device=dev)
        group = max(1, int(max_logits_bytes) // (T * U1 * self.vocab_size * 4))
        for b0 in range(0, B, group):
            b1 = min(B, b0 + group)
            H = ops.RNNTJointFn.apply(E[b0:b1], P[b0:b1])
            logits = ops.linear(H, self.lin_out.weight, self.lin_out.bias)
            ops.rnnt_rows(logits, txt[b0:b1], el[b0:b1], tl[b0:b1], self.blank, out=(lpb[b0:b1], lpl[b0:b1]))
            del H, logits
        return lpb, lpl

    @torch.no_grad()
    def align(self, encode_feature, encode_len, txt, txt_len, confidence=False, max_logits_bytes=1 << 30,
              flags=ops.ALIGN_BP_AUTO):
        ''' forced alignment of every utterance to txt: lattice_logp, then the best path through the lattice, found and
            traced back on the device (ops.rnnt_align) -> ops.RNNTAlignment(frames [B,U], labels_done [B,T'], tok_logp
            [B,U], tok_post [B,U] or None, score [B]).  Frames are encoder frames; among equal-scoring paths every
            label is emitted as early as possible.  confidence=True also runs the alpha / beta lattice of the loss and
            returns the posterior of every chosen emission as tok_post. '''
        lpb, lpl = self.lattice_logp(encode_feature, encode_len, txt, txt_len, max_logits_bytes)
        lattice = ops.rnnt_lattice(lpb, lpl, encode_len, txt_len) if confidence else None
        return ops.rnnt_align(lpb, lpl, encode_len, txt_len, flags=flags, lattice=lattice)

    @torch.no_grad()
    def greedy(self, encode_feature, encode_len, max_symbols, max_len):
        ''' lock-step greedy search over the batch -> (tokens int64 [B, max_len], n_tokens int32 [B]), both on the
            device.  Every utterance keeps its own frame pointer; each of the T' + max_len iterations (exact: an
            iteration advances a frame or emits one of at most max_len tokens) embeds the last emitted token, steps
            the cells, projects, takes the joint at the row's frame, and asrk_rnnt_greedy_step_f32 updates the
            bookkeeping.  The new prediction-network state and P row are kept only where a token was emitted
            (dops.gather_rows_multi).  Nothing is read back inside the loop. '''
        dev = encode_feature.device
        B, T, _ = encode_feature.shape
        max_symbols, max_len = int(max_symbols), int(max_len)
        enc_len = torch.as_tensor(encode_len).to(device=dev, dtype=torch.int64).contiguous()
        E = ops.linear(encode_feature, self.lin_enc.weight, self.lin_enc.bias)
        st = ops.rnnt_greedy_state(B, max_len, dev)
        if self.stateless:
            # no state to keep: the last `context` labels of every row are in st.tokens / st.n_tok, so the P rows of the
            # next iteration are one context step on the bookkeeping just written and lin_pred
            P = self._ctx_rows(st.tokens, st.n_tok)
            for _ in range(T + max_len):
                H = ops.rnnt_joint_step(E, P, st.t_ptr)
                logits = ops.linear(H, self.lin_out.weight, self.lin_out.bias)
                ops.rnnt_greedy_step(logits, enc_len, T, st, max_symbols, max_len, self.blank)
                P = self._ctx_rows(st.tokens, st.n_tok)
            return st.tokens[:, :max_len], st.n_tok
        lstm = self.rnn_type == 'LSTM'
        n_state = self.layer * (2 if lstm else 1)
        widths = [self.dim] * n_state + [self.joint_dim]
        # per kept tensor two [2,B,W] buffers (ping-pong): slot 0 = the kept value, slot 1 = this iteration's candidate
        bufs = [[torch.zeros((2, B, w), dtype=torch.float32, device=dev) for w in widths] for _ in range(2)]
        ar = torch.arange(B, dtype=torch.int64, device=dev)

        def step_cells(cur, tok):
            ''' candidates (slot 1 of `cur`) from the kept state (slot 0) and the token `tok` [B] '''
            inp = dops.embedding(tok, self.emb.weight)
            for l in range(self.layer):
                if lstm:
                    hb, cb = cur[2 * l], cur[2 * l + 1]
                    dops.lstm_cell_infer(inp, hb[0], cb[0], *self.pred.layer_params(l), out=(hb[1], cb[1]))
                    inp = hb[1]
                else:
                    ops.copy_flat(cur[l][1], gru_ops.gru_cell_infer(inp, cur[l][0], *self.pred.layer_params(l)))
                    inp = cur[l][1]
            ops.copy_flat(cur[-1][1], ops.linear(inp, self.lin_pred.weight, self.lin_pred.bias))

        # <sos> from the zero state is every row's first kept state: step it, then keep slot 1 everywhere
        step_cells(bufs[0], st.last_tok)
        self._select(bufs[0], bufs[1], ar + B, widths)
        k = 1
        for _ in range(T + max_len):
            cur, nxt = bufs[k], bufs[1 - k]
            H = ops.rnnt_joint_step(E, cur[-1][0], st.t_ptr)
            logits = ops.linear(H, self.lin_out.weight, self.lin_out.bias)
            ops.rnnt_greedy_step(logits, enc_len, T, st, max_symbols, max_len, self.blank)
            # the candidate a row would move to if it emitted now is the step on ITS new last token; rows that did not
            # emit keep slot 0, so stepping all rows on last_tok is harmless for them
            step_cells(cur, st.last_tok)
            self._select(cur, nxt, torch.add(ar, st.emit, alpha=B), widths)
            k = 1 - k
        return st.tokens[:, :max_len], st.n_tok

    def _ctx_rows(self, tokens, n_tok):
        ''' stateless head: lin_pred of the prediction-network output after <sos> and the n_tok[r] labels of row r '''
        return ops.linear(ops.rnnt_ctx_step(tokens, n_tok.view(-1), self.emb.weight, self.ctx.weight),
                          self.lin_pred.weight, self.lin_pred.bias)

    @staticmethod
    def _select(src, dst, parent, widths):
        ''' dst slot 0 [b] = src slot (parent[b] // B) [b] for every kept tensor, 8 segments per launch '''
        segs = [(s, d[0], w, 1, False) for s, d, w in zip(src, dst, widths)]
        for i in range(0, len(segs), 8):
            dops.gather_rows_multi(segs[i:i + 8], parent)

    @torch.no_grad()
    def beam_search(self, encode_feature, encode_len, beam_size, max_symbols, max_len, nbest=1, lm=None, lm_weight=0.0):
        ''' alignment-length-synchronous beam search (Saon et al. 2020) in lock-step over the batch, W = beam_size slots
            per utterance (rows r = b * W + w) -> (tokens int64 [B, nbest, max_len] zero-padded, n_tok int32 [B, nbest],
            score float64 [B, nbest] = ln of the summed probability of the kept alignments (+ lm_weight * LM), n_hyp
            int32 [B]), best first, all on the device.  Each of the T' + max_len iterations runs the joint at every
            row's own frame, lin_out, one row pass (log-sum-exp, blank, the K = min(W, V - 1) best labels by
            lp + lm_weight * lm; csrc/rnnt_beam.hip) and one select launch (candidates, merge of equal sequences, cut to
            W, finished list); then the survivors' states are gathered from their parents, the cells, lin_pred and the
            LM step on the appended token, and the stepped state is kept where a token was appended.  Nothing is read
            back inside the loop.  lm: an NGramLM (its log-probabilities are added to the labels, never to blank), a
            ContextBias (src/bias.py; lm_weight 1.0) or a BiasedNGram; with biasing the pending bonus of a hypothesis that
            stops inside a phrase is taken back after the loop and the finished lists are re-sorted (_bank_bias). '''
        nbest, max_len = int(nbest), int(max_len)
        if not 1 <= nbest <= int(beam_size):
            raise ValueError('beam_search: 1 <= nbest <= beam_size, got nbest = {}'.format(nbest))
        st = None
        for _, st in self.beam_steps(encode_feature, encode_len, beam_size, max_symbols, max_len, lm, lm_weight):
            pass
        dev = encode_feature.device
        B, T, _ = encode_feature.shape
        f = (T + max_len) & 1                       # the buffer the last iteration wrote
        fin_tok, fin_len, fin_score = st.fin_tok[f], st.fin_len[f], st.fin_score[f]
        if lm is not None and float(lm_weight) > 0 and hasattr(lm, 'walk'):
            fin_tok, fin_len, fin_score = self._bank_bias(lm, lm_weight, fin_tok, fin_len, fin_score, st.fin_n[f])
        tokens = torch.zeros((B, nbest, max_len), dtype=torch.int64, device=dev)
        n_tok = fin_len[:, :nbest].clone()
        valid = torch.arange(nbest, device=dev).view(1, nbest) < st.fin_n[f].view(B, 1)
        n_tok = torch.where(valid, n_tok, torch.zeros_like(n_tok))
        if max_len > 0:
            pos = torch.arange(max_len, device=dev).view(1, 1, max_len)
            tokens = torch.where(pos < n_tok.unsqueeze(2), fin_tok[:, :nbest, :max_len].to(torch.int64), tokens)
        score = torch.where(valid, fin_score[:, :nbest], torch.full_like(fin_score[:, :nbest], float('-inf')))
        return tokens, n_tok, score, torch.clamp(st.fin_n[f], max=nbest)

    @staticmethod
    def _bank_bias(lm, lm_weight, fin_tok, fin_len, fin_score, fin_n):
        ''' contextual biasing: a finished hypothesis that stops inside a phrase still holds the phrase's pending bonus
            (ContextBias.walk's residual, in the row's units: times lm_weight).  It is taken back and each utterance's
            finished list [B, W] re-sorted best first (stable: equal scores keep their order), all on the device. '''
        B, W, Lc = fin_tok.shape
        _, _, residual = lm.walk(fin_tok.reshape(B * W, Lc), torch.clamp(fin_len.reshape(B * W), min=0, max=Lc))
        valid = torch.arange(W, device=fin_tok.device).view(1, W) < fin_n.view(B, 1)
        score = fin_score - residual.view(B, W).to(torch.float64) * float(lm_weight)
        score = torch.where(valid, score, torch.full_like(score, float('-inf')))
        order = torch.sort(score, dim=1, descending=True, stable=True)[1]
        return (torch.gather(fin_tok, 1, order.view(B, W, 1).expand(B, W, Lc)), torch.gather(fin_len, 1, order),
                torch.gather(score, 1, order))

    @torch.no_grad()
    def beam_steps(self, encode_feature, encode_len, beam_size, max_symbols, max_len, lm=None, lm_weight=0.0):
        ''' the loop of beam_search as a generator: yields (i, state) after iteration i = 0 .. T' + max_len - 1, `state`
            the ops.RNNTBeamState whose buffer 1 - (i & 1) iteration i has just written (the next beam and the finished
            list so far).  Nothing is read back; a caller that stops early leaves the search unfinished. '''
        from .bias import BiasedNGram, ContextBias
        from .ngram import NGramLM
        if lm is not None and not isinstance(lm, (NGramLM, ContextBias, BiasedNGram)):
            raise NotImplementedError('TransducerHead.beam_search fuses an NGramLM (with or without a ContextBias) or a '
                                      'ContextBias only, got {}'.format(type(lm).__name__))
        dev = encode_feature.device
        B, T, _ = encode_feature.shape
        W, max_symbols, max_len = int(beam_size), int(max_symbols), int(max_len)
        if not 1 <= W <= ops.RNNT_BEAM_MAX or max_symbols < 0 or max_len < 0:
            raise ValueError('beam_search: 1 <= beam_size <= {}, max_symbols >= 0, max_len >= 0'.format(
                ops.RNNT_BEAM_MAX))
        V = self.vocab_size
        if lm is not None and lm.vocab_size != V:
            raise ValueError('beam_search: the LM has {} tokens, the head {}'.format(lm.vocab_size, V))
        use_lm = lm is not None and float(lm_weight) > 0
        K = min(W, V - 1)
        R = B * W
        enc_len = torch.as_tensor(encode_len).to(device=dev, dtype=torch.int64).contiguous()
        E = ops.linear(encode_feature, self.lin_enc.weight, self.lin_enc.bias)
        st = ops.rnnt_beam_state(B, W, K, max_len, dev)
        if self.stateless:
            yield from self._beam_steps_stateless(E, enc_len, st, T, max_symbols, max_len, lm if use_lm else None,
                                                  lm_weight)
            return
        lstm = self.rnn_type == 'LSTM'
        n_state = self.layer * (2 if lstm else 1)
        widths = [self.dim] * n_state + [self.joint_dim]
        # kept[x][0] = the kept value of every row; work[x] = [gathered from the parents, stepped on the appended token]
        kept = [torch.zeros((2, R, w), dtype=torch.float32, device=dev) for w in widths]
        work = [torch.zeros((2, R, w), dtype=torch.float32, device=dev) for w in widths]
        ar = torch.arange(R, dtype=torch.int64, device=dev)

        def step_cells(cur, tok):
            ''' slot 1 of `cur` from slot 0 and the token `tok` [R] '''
            inp = dops.embedding(tok, self.emb.weight)
            for l in range(self.layer):
                if lstm:
                    hb, cb = cur[2 * l], cur[2 * l + 1]
                    dops.lstm_cell_infer(inp, hb[0], cb[0], *self.pred.layer_params(l), out=(hb[1], cb[1]))
                    inp = hb[1]
                else:
                    ops.copy_flat(cur[l][1], gru_ops.gru_cell_infer(inp, cur[l][0], *self.pred.layer_params(l)))
                    inp = cur[l][1]
            ops.copy_flat(cur[-1][1], ops.linear(inp, self.lin_pred.weight, self.lin_pred.bias))

        # <sos> from the zero state is every row's first kept state
        step_cells(work, st.last_tok)
        self._select(work, kept, ar + R, widths)
        if use_lm:
            # LM rows and the int32 LM state (moved as 4-byte rows): [kept | stepped], two such buffers in turn
            lm_rows = [torch.zeros((2, R, V), dtype=torch.float32, device=dev) for _ in range(2)]
            S = int(getattr(lm, 'state_width', 1))       # int32 per row: 1 (n-gram or bias), 2 (both)
            lm_state = [torch.zeros((2, R, S), dtype=torch.float32, device=dev) for _ in range(2)]
            lm(st.last_tok.view(R, 1), None, None, out=lm_rows[0][0], state_out=lm_state[0][0].view(torch.int32))
        table = (st.lse, st.lpb, st.val, st.lab)
        k = 0
        for i in range(T + max_len):
            cur = i & 1
            H = ops.rnnt_joint_slots(E, kept[-1][0], st.t_ptr[cur].view(-1), W)
            logits = ops.linear(H, self.lin_out.weight, self.lin_out.bias)
            ops.rnnt_beam_rows(logits, W, K, lm_rows[k][0] if use_lm else None, lm_weight if use_lm else 0.0,
                               st.n_live[cur], self.blank, out=table)
            ops.rnnt_beam_select(st, enc_len, T, max_symbols, cur)
            # every row continues its parent: gather the kept states, step them on the appended token, keep the step
            # where a token was appended
            self._gather(kept, work, st.parent, widths)
            step_cells(work, st.last_tok)
            self._select(work, kept, st.sel, widths)
            if use_lm:
                lm(st.last_tok.view(R, 1), None, lm_state[k][0].view(torch.int32), parent=st.parent,
                   out=lm_rows[k][1], state_out=lm_state[k][1].view(torch.int32))
                dops.gather_rows_multi([(lm_rows[k], lm_rows[1 - k][0], V, 1, False),
                                        (lm_state[k], lm_state[1 - k][0], S, 1, False)], st.lm_sel)
                k = 1 - k
            yield i, st

    def _beam_steps_stateless(self, E, enc_len, st, T, max_symbols, max_len, lm, lm_weight):
        ''' the loop of beam_steps for the stateless head: no kept / work buffers, no gather, no select.  After the select
            launch has written beam buffer 1 - cur, the P rows of the next iteration are one context step on that buffer's
            tokens / n_tok and lin_pred.  The n-gram LM branch is the one of the LSTM / GRU loop: its int32 state still
            moves by lm_sel. '''
        dev = E.device
        B, W, K, V = st.B, st.W, st.K, self.vocab_size
        R = B * W
        if lm is not None:
            lm_rows = [torch.zeros((2, R, V), dtype=torch.float32, device=dev) for _ in range(2)]
            S = int(getattr(lm, 'state_width', 1))       # int32 per row: 1 (n-gram or bias), 2 (both)
            lm_state = [torch.zeros((2, R, S), dtype=torch.float32, device=dev) for _ in range(2)]
            lm(st.last_tok.view(R, 1), None, None, out=lm_rows[0][0], state_out=lm_state[0][0].view(torch.int32))
        table = (st.lse, st.lpb, st.val, st.lab)
        P = self._ctx_rows(st.tokens[0], st.n_tok[0])
        k = 0
        for i in range(T + max_len):
            cur = i & 1
            H = ops.rnnt_joint_slots(E, P, st.t_ptr[cur].view(-1), W)
            logits = ops.linear(H, self.lin_out.weight, self.lin_out.bias)
            ops.rnnt_beam_rows(logits, W, K, lm_rows[k][0] if lm is not None else None,
                               lm_weight if lm is not None else 0.0, st.n_live[cur], self.blank, out=table)
            ops.rnnt_beam_select(st, enc_len, T, max_symbols, cur)
            P = self._ctx_rows(st.tokens[1 - cur], st.n_tok[1 - cur])
            if lm is not None:
                lm(st.last_tok.view(R, 1), None, lm_state[k][0].view(torch.int32), parent=st.parent,
                   out=lm_rows[k][1], state_out=lm_state[k][1].view(torch.int32))
                dops.gather_rows_multi([(lm_rows[k], lm_rows[1 - k][0], V, 1, False),
                                        (lm_state[k], lm_state[1 - k][0], S, 1, False)], st.lm_sel)
                k = 1 - k
            yield i, st

    @staticmethod
    def _gather(src, dst, parent, widths):
        ''' dst slot 0 [r] = src slot 0 [parent[r]] for every kept tensor, 8 segments per launch '''
        segs = [(s[0], d[0], w, 1, False) for s, d, w in zip(src, dst, widths)]
        for i in range(0, len(segs), 8):
            dops.gather_rows_multi(segs[i:i + 8], parent)
