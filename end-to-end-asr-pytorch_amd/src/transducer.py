"""RNN-transducer head (Graves 2012) on the pyramidal encoder: embedding + unidirectional LSTM/GRU prediction network,
joint network tanh(lin_enc(enc)[b,t] + lin_pred(pred)[b,u]) -> lin_out -> [B, T', U+1, V] logits for ops.RNNTLoss, and
batched greedy decoding with device-resident bookkeeping (csrc/rnnt.hip).  Blank = <sos> = 0.
"""
import torch
import torch.nn as nn

from .. import ops
from .. import decoder_ops as dops
from .. import gru_ops
from .module import RNNParams


PRED_KEYS = ('module', 'dim', 'layer', 'emb_dim', 'dropout')


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


def take_decode_block(dcfg):
    ''' removes `transducer` from the decode block (the parent solver hands the rest to the beam decoders) and returns
        {max_symbols, max_len_ratio} when it is enabled, else None '''
    block = dcfg.pop('transducer', None) or {}
    if not isinstance(block, dict):
        raise ValueError('decode.transducer: expected a mapping, got %r' % (block,))
    unknown = sorted(set(block) - {'enable', 'max_symbols', 'max_len_ratio'}, key=str)
    if unknown:
        raise ValueError('decode.transducer: unknown key(s) {}'.format(unknown))
    if not block.get('enable', False):
        return None
    if dcfg.get('align', False) or (dcfg.get('rescore') or {}).get('enable', False):
        raise ValueError('decode.transducer excludes decode.align and decode.rescore')
    opts = {'max_symbols': int(block.get('max_symbols', 3)), 'max_len_ratio': float(block.get('max_len_ratio', 0.5))}
    if opts['max_symbols'] < 1 or not opts['max_len_ratio'] > 0:
        raise ValueError('decode.transducer: max_symbols must be >= 1 and max_len_ratio > 0')
    return opts


class TransducerHead(nn.Module):
    ''' vocab_size: V (index 0 is blank and <sos>); enc_dim: encoder output width;
        pred = {module: LSTM|GRU, dim, layer, emb_dim, dropout}; joint_dim: J '''

    def __init__(self, vocab_size, enc_dim, pred, joint_dim):
        super().__init__()
        unknown = set(pred) - set(PRED_KEYS)
        if unknown:
            raise ValueError('transducer: unknown pred keys {}'.format(sorted(unknown)))
        module = str(pred.get('module', 'LSTM')).upper()
        if module not in ('LSTM', 'GRU'):
            raise NotImplementedError("transducer prediction network '{}' is not supported (LSTM / GRU)".format(module))
        self.vocab_size = vocab_size
        self.rnn_type = module
        self.dim = int(pred.get('dim', 512))
        self.layer = int(pred.get('layer', 1))
        self.emb_dim = int(pred.get('emb_dim', self.dim))
        self.dropout = float(pred.get('dropout', 0.0))
        self.joint_dim = int(joint_dim)
        self.blank = 0
        self.emb = nn.Embedding(vocab_size, self.emb_dim)
        self.pred = RNNParams(module, self.emb_dim, self.dim, num_layers=self.layer, dropout=self.dropout,
                              batch_first=True)
        self.lin_enc = nn.Linear(enc_dim, self.joint_dim)
        self.lin_pred = nn.Linear(self.dim, self.joint_dim)
        self.lin_out = nn.Linear(self.joint_dim, vocab_size)

    def create_msg(self):
        return '           | Transducer head enabled ( {} x{} dim {}, joint dim {}).'.format(
            self.rnn_type, self.layer, self.dim, self.joint_dim)

    def _predict(self, txt):
        ''' txt [B,U] -> prediction-network output [B,U+1,dim] on <sos> + txt, from a zero state (as
            RNNLM._forward_sequence: unidirectional, so the padded tail changes no valid position) '''
        dev = self.emb.weight.device
        B = txt.shape[0]
        inp = torch.cat([torch.zeros((B, 1), dtype=torch.int64, device=dev), txt.to(device=dev, dtype=torch.int64)],
                        dim=1)
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

    @staticmethod
    def _select(src, dst, parent, widths):
        ''' dst slot 0 [b] = src slot (parent[b] // B) [b] for every kept tensor, 8 segments per launch '''
        segs = [(s, d[0], w, 1, False) for s, d, w in zip(src, dst, widths)]
        for i in range(0, len(segs), 8):
            dops.gather_rows_multi(segs[i:i + 8], parent)
