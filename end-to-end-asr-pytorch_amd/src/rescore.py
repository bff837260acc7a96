"""Two-pass decoding: attention (+LM) rescoring of CTC n-best lists.

First pass: the pure-CTC prefix beam search (CTCBeamDecoder, unchanged) gives every utterance up to `beam_size`
distinct prefixes.  Second pass: every hypothesis y = y_1..y_n is scored by

    s_ctc(y) = log p_ctc(y | h_u)                                  (ops.ctc_score_rows, all rows in one launch)
    s_att(y) = sum_t log softmax(att_logits_t)[y_{t+1}], <eos> included   (ASR.score_hypotheses, teacher-forced)
    s_lm(y)  = sum_t log p_lm(y_{t+1} | <sos>, y_1..y_t), <eos> included  (only with lm_weight > 0)
    score(y) = ctc_weight * s_ctc + (1 - ctc_weight) * s_att + lm_weight * s_lm      (float64, on the host)

and the list is re-ranked on `score`, descending, ties in first-pass order; a hypothesis without a CTC path
(s_ctc = -inf) ranks last.  The encoder runs once per batch: both passes read the same posteriors.
"""
import collections
import types

import numpy as np
import torch
import yaml
from torch import nn

from .. import ops
from .ctc import CTCBeamDecoder
from .lm import RNNLM
from .ngram import NGramLM, is_ngram_path

EOS = 1          # <eos> (src/text.py); <sos> = 0 is what the decoder and the LMs start from

_Fields = collections.namedtuple('RescoredHyp', ['tokens', 'score', 'ctc', 'att', 'lm', 'first_rank'])


class RescoredHyp(_Fields):
    ''' one hypothesis of a rescored n-best list: token ids (no <eos>), the combined score, the three model scores
        (lm is 0.0 without an LM) and its rank in the first-pass list '''
    __slots__ = ()

    @property
    def outIndex(self):
        return list(self.tokens)


def combine_scores(ctc, att, lm, ctc_weight, lm_weight):
    ''' score [n] float64 from the three score vectors (lm may be None); a hypothesis without a CTC path gets -inf
        whatever the weights are (0 * -inf would be NaN) '''
    ctc = np.asarray(ctc, dtype=np.float64)
    att = np.asarray(att, dtype=np.float64)
    lm = np.zeros_like(att) if lm is None else np.asarray(lm, dtype=np.float64)
    finite = np.where(np.isneginf(ctc), 0.0, ctc)
    score = ctc_weight * finite + (1.0 - ctc_weight) * att + (lm_weight * lm if lm_weight > 0 else 0.0)
    return np.where(np.isneginf(ctc), -np.inf, score)


def rank_hypotheses(hyps, ctc, att, lm, ctc_weight, lm_weight):
    ''' first-pass list `hyps` (token lists, best first) + its score vectors -> [RescoredHyp], best first: descending
        score, ties broken by first-pass rank (a stable sort); -inf and NaN scores rank last '''
    score = combine_scores(ctc, att, lm, ctc_weight, lm_weight)
    key = np.where(np.isnan(score), -np.inf, score)
    order = sorted(range(len(hyps)), key=lambda i: -key[i])
    lm_v = np.zeros(len(hyps)) if lm is None else np.asarray(lm, dtype=np.float64)
    return [RescoredHyp(tuple(int(t) for t in hyps[i]), float(score[i]), float(ctc[i]), float(att[i]), float(lm_v[i]),
                        i) for i in order]


def check_decode_config(dcfg, emb_cfg=None):
    ''' what the solver refuses before it builds anything: `dcfg` is the decode block WITH its rescore entry '''
    rs = dcfg.get('rescore') or {}
    if not rs.get('enable', False):
        return
    unknown = set(rs) - {'enable', 'first_pass_lm', 'workspace_mb'}
    if unknown:
        raise ValueError('decode.rescore: unknown keys {}'.format(sorted(unknown)))
    if dcfg.get('beam_size', 1) == 1:
        raise ValueError('decode.rescore needs an n-best list: beam_size must be above 1')
    if dcfg.get('align', False):
        raise ValueError('decode.rescore and decode.align exclude each other')
    if dcfg.get('ctc_weight', 0.0) == 1.0:
        raise ValueError('decode.rescore with ctc_weight = 1.0 would leave the first-pass order: use CTC beam search')
    if emb_cfg and emb_cfg.get('enable') and emb_cfg.get('fuse', 0) > 0:
        raise ValueError('decode.rescore does not cover the emb: plug-in with fuse > 0 (its output is a mixture '
                         'distribution)')


class RescoreDecoder(nn.Module):
    ''' CTC prefix beam search, then attention (+LM) rescoring of its n-best list '''

    def __init__(self, asr, beam_size, vocab_candidate, ctc_weight=0.0, lm_path='', lm_config='', lm_weight=0.0,
                 first_pass_lm=False, workspace_mb=1024, device=None):
        super().__init__()
        if not getattr(asr, 'enable_att', False):
            raise ValueError('RescoreDecoder: the model has no attention decoder to rescore with')
        if not getattr(asr, 'enable_ctc', False):
            raise ValueError('RescoreDecoder: the model has no CTC head for the first pass')
        if not 0.0 <= ctc_weight < 1.0:
            raise ValueError('RescoreDecoder: ctc_weight must be in [0, 1), got {}'.format(ctc_weight))
        vocab_range = [1] + [r for r in range(3, asr.vocab_size)]
        probe = types.SimpleNamespace(vocab_range=vocab_range, beam_size=beam_size, vocab_cand=vocab_candidate)
        if not CTCBeamDecoder._device_search_ok(probe, asr.vocab_size):
            raise ValueError('RescoreDecoder: beam_size = {} / vocab_candidate = {} are outside what the device '
                             'prefix-beam search takes'.format(beam_size, vocab_candidate))
        if workspace_mb <= 0:
            raise ValueError('RescoreDecoder: workspace_mb must be positive')
        self.asr = asr
        self.beam_size = beam_size
        self.ctc_w = float(ctc_weight)
        self.lm_w = float(lm_weight)
        self.apply_lm = lm_weight > 0
        self.first_pass_lm = bool(first_pass_lm) and self.apply_lm
        self.workspace_mb = workspace_mb
        self.device = device
        self.lm_path = lm_path
        self.first = CTCBeamDecoder(asr, vocab_range, beam_size, vocab_candidate, lm_path=lm_path,
                                    lm_config=lm_config, lm_weight=lm_weight if self.first_pass_lm else 0.0,
                                    device=device)
        if self.first_pass_lm:
            self.lm = self.first.lm
        elif self.apply_lm:
            if is_ngram_path(lm_path):              # back-off n-gram (ARPA / saved image): lm_config is not read
                self.lm = NGramLM.from_file(lm_path, asr.vocab_size).to(device)
            else:
                lm_config = yaml.load(open(lm_config, 'r'), Loader=yaml.FullLoader)
                self.lm = RNNLM(asr.vocab_size, **lm_config['model']).to(device)
                self.lm.load_state_dict(torch.load(lm_path, map_location='cpu')['model'])
            self.lm.eval()

    def create_msg(self):
        msg = ['Decode spec| CTC n-best rescoring \t| Beam size = {} \t| CTC weight = {:.2f}'.format(
            self.beam_size, self.ctc_w)]
        if self.apply_lm:
            msg.append('           |LM rescoring enabled \t| weight = {:.2f}\t| first pass = {}\t| src = {}'.format(
                self.lm_w, self.first_pass_lm, self.lm_path))
            if isinstance(self.lm, NGramLM):
                msg += self.lm.create_msg()
        return msg

    # ---- first pass ----------------------------------------------------------------------------------------------
    def _encode(self, feat, feat_len):
        ''' -> (enc [U,T',D], enc_len [U] device, frames: U host ints = the frames the first pass searches) '''
        asr = self.asr
        U = feat.shape[0]
        dev = feat.device
        lens = torch.as_tensor(feat_len).to(dev)
        if U > 1 and asr.encoder.supports_packed():
            enc, enc_len = asr.encoder(feat, lens, packed=True)
            return enc, enc_len.to(dev), [int(v) for v in asr.encoder.packed_frames.cpu().tolist()]
        lens_h = [int(v) for v in lens.cpu().tolist()]
        outs = [asr.encoder(feat[u:u + 1, :lens_h[u]].contiguous(), lens[u:u + 1]) for u in range(U)]
        if U == 1:
            return outs[0][0], outs[0][1].to(dev), [outs[0][0].shape[1]]
        frames = [e.shape[1] for e, _ in outs]
        enc = torch.zeros((U, max(frames), outs[0][0].shape[2]), dtype=torch.float32, device=dev)
        for u, (e, _) in enumerate(outs):
            enc[u, :frames[u]] = e[0]
        return enc, torch.cat([l.to(dev) for _, l in outs]), frames

    def first_pass(self, ctc_output, frames):
        ''' n-best lists of the U utterances from the model's CTC log-probs [U,T',V] '''
        ctc2 = ops.log_softmax(ctc_output)           # the first-pass search reads log_softmax applied twice (src/ctc.py)
        if ctc_output.shape[0] == 1:
            return [self.first.search_device(ctc2[0, :frames[0]].contiguous())]
        return self.first.search_batch(ctc2, frames)

    # ---- second pass ---------------------------------------------------------------------------------------------
    def _lm_scores(self, ids, lens, target):
        ''' s_lm [R] float64: the LM teacher-forced on <sos>, y_1..y_n, scored on y_1..y_n, <eos> '''
        R, L = ids.shape
        dev = ids.device
        inp = torch.cat([torch.zeros((R, 1), dtype=torch.int64, device=dev), ids[:, :-1]], 1).contiguous()
        V = self.asr.vocab_size
        if getattr(self.lm, 'returns_logp', False):
            # n-gram: one step per position for all rows; its log-probs are used as they are (not renormalised)
            state, cols = None, []
            for t in range(L):
                out, state = self.lm(inp[:, t:t + 1].contiguous(), None, state)
                cols.append(ops.seq_logp(out.view(R, V), target[:, t].contiguous(), normalized=True)[0])
            tok = torch.stack(cols, 1).contiguous()                                    # [R,L], 0 on padding
            seg = torch.arange(R + 1, dtype=torch.int64, device=dev) * L
            return ops.seq_logp(tok.view(R * L, 1), torch.zeros((R * L,), dtype=torch.int64, device=dev), seg,
                                normalized=True)[1]
        out = torch.zeros((R,), dtype=torch.float64, device=dev)
        chunk = max(1, int(self.workspace_mb * 2 ** 20) // (4 * L * (V + 4 * self.lm.dim)))
        for r0 in range(0, R, chunk):
            r1 = min(R, r0 + chunk)
            n = r1 - r0
            logits, _ = self.lm(inp[r0:r1], torch.full((n,), L, dtype=torch.long))
            seg = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
            out[r0:r1] = ops.seq_logp(logits.reshape(n * L, V), target[r0:r1].reshape(-1), seg)[1]
        return out

    @torch.no_grad()
    def score_nbest(self, enc, enc_len, ctc_output, frames, nbest):
        ''' the three score vectors of every hypothesis of every list -> (ctc, att, lm | None) numpy float64 [R] in
            list order, after ONE read-back '''
        dev = enc.device
        rows = [(u, h) for u, hyps in enumerate(nbest) for h in hyps]
        R = len(rows)
        if R == 0:
            z = np.zeros((0,), dtype=np.float64)
            return z, z, (z if self.apply_lm else None)
        Lmax = max(len(h) for _, h in rows)
        tgt = np.zeros((R, max(Lmax, 1)), dtype=np.int64)
        ids = np.zeros((R, Lmax + 1), dtype=np.int64)
        for r, (_, h) in enumerate(rows):
            tgt[r, :len(h)] = h
            ids[r, :len(h)] = h
            ids[r, len(h)] = EOS
        tl = torch.tensor([len(h) for _, h in rows], dtype=torch.int64, device=dev)
        row_mem = torch.tensor([u for u, _ in rows], dtype=torch.int64, device=dev)
        ids = torch.from_numpy(ids).to(dev)
        s_ctc = ops.ctc_score_rows(ctc_output, torch.tensor(frames, dtype=torch.int64), row_mem,
                                   torch.from_numpy(tgt), tl, blank=0)
        _, s_att = self.asr.score_hypotheses(enc, enc_len, row_mem, ids, tl + 1, workspace_mb=self.workspace_mb)
        parts = [s_ctc.double(), s_att]
        if self.apply_lm:
            L = ids.shape[1]
            target = torch.where(torch.arange(L, device=dev).unsqueeze(0) < (tl + 1).unsqueeze(1), ids,
                                 torch.full_like(ids, -1))
            parts.append(self._lm_scores(ids, tl + 1, target))
        host = torch.stack(parts, 0).cpu().numpy()          # the one read-back of the score vectors
        return host[0], host[1], (host[2] if self.apply_lm else None)

    @torch.no_grad()
    def forward_batch(self, feat, feat_len):
        ''' feat [U,Tmax,D] zero-padded, feat_len [U] -> U lists of RescoredHyp, best first '''
        asr = self.asr
        enc, enc_len, frames = self._encode(feat, feat_len)
        ctc_output = ops.log_softmax(ops.linear(enc, asr.ctc_layer.weight, asr.ctc_layer.bias))
        nbest = self.first_pass(ctc_output, frames)
        ctc, att, lm = self.score_nbest(enc, enc_len, ctc_output, frames, nbest)
        out, r0 = [], 0
        for hyps in nbest:
            r1 = r0 + len(hyps)
            out.append(rank_hypotheses(hyps, ctc[r0:r1], att[r0:r1], None if lm is None else lm[r0:r1],
                                       self.ctc_w, self.lm_w))
            r0 = r1
        return out

    @torch.no_grad()
    def forward(self, feat, feat_len):
        assert feat.shape[0] == 1, "Batchsize == 1 is required for beam search"
        return self.forward_batch(feat, feat_len)[0]
