"""Minimum word error rate training on n-best lists (Prabhavalkar et al. 2018): the top-level `mwer:` block.

    mwer:
      enable: true
      nbest: 4              # N, 2..32: hypotheses per utterance that enter the loss
      beam_size: 4          # >= nbest: width of the search that produces them
      ce_weight: 0.01       # lambda on the existing loss (CE on the reference, + CTC for hybrid models)
      unit: word            # word | token: what an error is counted in
      ctc_weight: 0.0       # joint CTC score in the SEARCH only
      min_len_ratio: 0.01
      max_len_ratio: 0.30
      start_step: 0         # steps below it are plain steps

For utterance u with reference y*_u and the n_u <= N distinct hypotheses y_{u,i} at the top of its beam list:

    s_{u,i} = log p_att(y_{u,i}, <eos> | x_u)      teacher-forced, the model in TRAINING mode (ASR.hypothesis_logp)
    e_{u,i} = edit distance(y_{u,i}, y*_u)         in words or tokens, an integer
    p_{u,i} = softmax_i(s_{u,.})                   over the n_u valid hypotheses
    L_u     = sum_i p_{u,i} (e_{u,i} - mean_i e_{u,i})
    L_mwer  = mean_u L_u                           the step's loss is L_mwer + ce_weight * (the existing loss)

The search (NBestSearch) is the batched device beam search of src/decode.py on the training model in eval mode, without
an LM; scoring, the loss and both gradients are kernels (csrc/rescore.hip, csrc/mwer.hip, csrc/metrics.hip).  An
absent or disabled block changes nothing.  Recognition accuracy under this criterion has not been measured: the
repository has no corpus with transcripts."""
import torch

from .. import ops
from .. import decoder_ops as dops
from .decode import BeamDecoder

EOS = 1
MAX_NBEST = 32            # asrk_mwer_loss_f64 and the beam search's own limit


class MWEROptions:
    KEYS = ('enable', 'nbest', 'beam_size', 'ce_weight', 'unit', 'ctc_weight', 'min_len_ratio', 'max_len_ratio',
            'start_step')

    def __init__(self, enable=True, nbest=4, beam_size=None, ce_weight=0.01, unit='word', ctc_weight=0.0,
                 min_len_ratio=0.01, max_len_ratio=0.30, start_step=0):
        def number(name, v, lo, hi=None):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or v < lo or (hi is not None and v > hi):
                raise ValueError('mwer: %s must be a number %s, got %r' % (
                    name, ('in [%g, %g]' % (lo, hi)) if hi is not None else ('>= %g' % lo), v))
            return float(v)

        def integer(name, v, lo, hi=None):
            if isinstance(v, bool) or not isinstance(v, int) or v < lo or (hi is not None and v > hi):
                raise ValueError('mwer: %s must be an integer %s, got %r' % (
                    name, ('in %d..%d' % (lo, hi)) if hi is not None else ('>= %d' % lo), v))
            return v

        if not isinstance(enable, bool):
            raise ValueError('mwer: enable must be true or false, got %r' % (enable,))
        self.enable = enable
        self.nbest = integer('nbest', nbest, 2, MAX_NBEST)
        beam_size = self.nbest if beam_size is None else beam_size
        self.beam_size = integer('beam_size', beam_size, 1, MAX_NBEST)
        if self.beam_size < self.nbest:
            raise ValueError('mwer: beam_size (%d) must be at least nbest (%d)' % (self.beam_size, self.nbest))
        self.ce_weight = number('ce_weight', ce_weight, 0.0)
        if unit not in ('word', 'token'):
            raise ValueError("mwer: unit must be 'word' or 'token', got %r" % (unit,))
        self.unit = unit
        self.ctc_weight = number('ctc_weight', ctc_weight, 0.0, 1.0)
        if self.ctc_weight >= 1.0:
            raise ValueError('mwer: ctc_weight must be below 1 (the lists come from the attention decoder)')
        self.min_len_ratio = number('min_len_ratio', min_len_ratio, 0.0)
        self.max_len_ratio = number('max_len_ratio', max_len_ratio, 0.0)
        if self.max_len_ratio <= 0.0 or self.max_len_ratio < self.min_len_ratio:
            raise ValueError('mwer: max_len_ratio must be positive and at least min_len_ratio')
        self.start_step = integer('start_step', start_step, 0)

    @classmethod
    def from_config(cls, cfg):
        """cfg: the whole yaml config (a mapping) -> MWEROptions, or None for an absent / disabled block"""
        block = cfg.get('mwer') if cfg is not None else None
        if block is None:
            return None
        if not isinstance(block, dict):
            raise ValueError('mwer: expected a mapping, got %r' % (block,))
        unknown = sorted(set(block) - set(cls.KEYS), key=str)
        if unknown:
            raise ValueError('mwer: unknown key(s) %s (known: %s)' % (unknown, ', '.join(cls.KEYS)))
        opts = cls(**block)
        if not opts.enable:
            return None
        model_ctc = float((cfg.get('model') or {}).get('ctc_weight', 0.0))
        if model_ctc == 1.0:
            raise ValueError('mwer: the model has no attention decoder (model.ctc_weight = 1)')
        if bool((cfg.get('emb') or {}).get('enable', False)):
            raise ValueError('mwer: not available with emb.enable (the plug-in\'s mixture output is not a logit)')
        if opts.ctc_weight > 0 and model_ctc == 0.0:
            raise ValueError('mwer: ctc_weight > 0 needs a model with a CTC head (model.ctc_weight = 0)')
        return opts

    def create_msg(self):
        return ('MWER training| N-best = {} (beam {}) | unit = {} | CE weight = {:g} | search CTC weight = {:g} | '
                'from step {}'.format(self.nbest, self.beam_size, self.unit, self.ce_weight, self.ctc_weight,
                                      self.start_step))


def pack_nbest(lists, nbest):
    """The n-best lists of U utterances (each a list of token-id lists in the search's order, possibly with a trailing
    <eos>, possibly with repeats, possibly empty) -> (ids [nbest*U, L] int64 with <eos> appended and zero padding,
    lens [nbest*U] int64 (<eos> included), count [U] int32, hyps: the kept token lists per utterance).  Row n*U + u holds
    hypothesis n of utterance u; slots n >= count[u] hold a copy of the utterance's first hypothesis.  An utterance
    without hypotheses gets the single hypothesis [] (just <eos>).  All on the host."""
    U = len(lists)
    hyps, count = [], []
    for raw in lists:
        kept, seen = [], set()
        for y in raw:
            y = [int(t) for t in y]
            while y and y[-1] == EOS:
                y.pop()
            if tuple(y) not in seen and len(kept) < nbest:
                seen.add(tuple(y))
                kept.append(y)
        if not kept:
            kept = [[]]
        hyps.append(kept)
        count.append(len(kept))
    L = max(len(y) for kept in hyps for y in kept) + 1
    ids = torch.zeros((nbest * U, L), dtype=torch.int64)
    lens = torch.zeros((nbest * U,), dtype=torch.int64)
    for u, kept in enumerate(hyps):
        for n in range(nbest):
            y = kept[n] if n < len(kept) else kept[0]
            r = n * U + u
            if y:
                ids[r, :len(y)] = torch.tensor(y, dtype=torch.int64)
            ids[r, len(y)] = EOS
            lens[r] = len(y) + 1
    return ids, lens, torch.tensor(count, dtype=torch.int32), hyps


class NBestSearch:
    """One BeamDecoder on the TRAINING model (no LM, no plug-in): per call model.eval(), the cached weight panels
    dropped, forward_batch under no_grad, attention.reset_mem(), model.train().
    The panel cache is keyed by data_ptr / _version and the fused optimiser writes through raw pointers, so a cached
    bf16 panel does not notice an update.  The device-resident search (BeamDecoder.batchable(): single-head
    location-aware attention, one-layer LSTM decoder, an encoder that encodes packed) drops the cache itself on every
    call; every other model is searched by one host-driven forward() per utterance, which does not - the call here
    covers that path.  `last_hyps` keeps the Hypothesis lists of the latest call (scores for logging and tests)."""

    def __init__(self, model, opts):
        self.model, self.opts = model, opts
        self.decoder = BeamDecoder(model, None, opts.beam_size, opts.min_len_ratio, opts.max_len_ratio,
                                   ctc_weight=opts.ctc_weight)
        self.last_hyps = None

    def create_msg(self):
        msg = self.decoder.create_msg()
        if not self.decoder.batchable():
            msg.append('           | This model is outside the device-resident batched search: every MWER step runs one '
                       'host-driven beam search per utterance (many times slower)')
        return msg

    def __call__(self, feat, feat_len):
        """-> (ids [N*U, L], lens [N*U], count [U]) on the host (see pack_nbest), hyps"""
        model = self.model
        was_training = model.training
        model.eval()
        try:
            dops.drop_weight_panels()
            with torch.no_grad():
                lists = self.decoder.forward_batch(feat, feat_len)
            model.attention.reset_mem()
        finally:
            model.train(was_training)
        self.last_hyps = lists
        return pack_nbest([[h.outIndex for h in hyps] for hyps in lists], self.opts.nbest)


def _rows(seqs, device):
    """lists of integers -> (padded int64 [B, >= 1] and int32 lengths) on the device"""
    W = max(1, max((len(s) for s in seqs), default=1))
    out = torch.zeros((len(seqs), W), dtype=torch.int64)
    for r, s in enumerate(seqs):
        if s:
            out[r, :len(s)] = torch.tensor(s, dtype=torch.int64)
    return out.to(device), torch.tensor([len(s) for s in seqs], dtype=torch.int32).to(device)


def word_ids(tokenizer, hyps, refs):
    """Token-id lists -> lists of integers, one per WORD of tokenizer.decode(...).split(): the same word gets the same
    integer throughout the batch, however it was segmented into tokens."""
    table = {}

    def words(y):
        return [table.setdefault(w, len(table) + 1) for w in tokenizer.decode(list(y)).split()]
    return [words(y) for y in hyps], [words(y) for y in refs]


def error_counts(tokenizer, hyps, refs, unit, device='cuda'):
    """hyps: N*U hypothesis token lists (no <eos>) in row order n*U + u; refs: the U reference token lists -> err int32
    [N*U] on the device, the edit distance of every row to its utterance's reference in `unit` (ops.edit_distance).
    unit 'token': the ids go to the kernel as they are; 'word': the lists are decoded and split on the host (they are
    there after the search's final read-back), words mapped to integers by a dictionary built for the batch, and the
    rows uploaded."""
    U = len(refs)
    if U == 0 or len(hyps) % U != 0:
        raise ValueError('error_counts: %d hypotheses do not divide into %d utterances' % (len(hyps), U))
    flat_h = [list(y) for y in hyps]
    flat_r = [list(refs[r % U]) for r in range(len(hyps))]
    if unit == 'word':
        flat_h, flat_r = word_ids(tokenizer, flat_h, flat_r)
    elif unit != 'token':
        raise ValueError("error_counts: unit must be 'word' or 'token', got %r" % (unit,))
    a, a_len = _rows(flat_h, device)
    b, b_len = _rows(flat_r, device)
    return ops.edit_distance(a, a_len, b, b_len)


def mwer_from_scores(s, err, count, nbest):
    """s f64 [N*U] (row n*U + u), err int32 [N*U], count int32 [U] -> (L_mwer, mean expected errors, mean 1-best
    errors): 0-d float64 device tensors; only L_mwer carries a gradient."""
    U = count.numel()
    loss_u, exp_err_u = ops.MWERLossFn.apply(s.view(nbest, U), err.view(nbest, U), count)
    return loss_u.mean(), exp_err_u.mean(), err.view(nbest, U)[0].to(torch.float64).mean()


class MWERLoss:
    """Ties the search, the scoring pass, the error counts and the loss kernel together for the training solver."""

    def __init__(self, model, tokenizer, opts):
        self.model, self.tokenizer, self.opts = model, tokenizer, opts
        self.search = NBestSearch(model, opts)

    def create_msg(self):
        return [self.opts.create_msg()] + self.search.create_msg()

    def nbest(self, feat, feat_len):
        """step 1, before the training forward (it resets the attention memory): the lists of this batch"""
        return self.search(feat, feat_len)

    def forward(self, nbest, encode_feature, encode_len, txt):
        """nbest: what nbest() returned; encode_feature / encode_len: the encoder output of the TRAINING forward; txt
        [U, L] the zero-padded reference ids (pass the HOST copy: a device tensor is read back) ->
        (L_mwer, {'exp_err', 'best_err'}) as device scalars"""
        ids, lens, count, hyps = nbest
        N, dev = self.opts.nbest, encode_feature.device
        U = count.numel()
        refs = [[t for t in row if t != 0] for row in torch.as_tensor(txt).cpu().tolist()]
        slots = [hyps[u][n] if n < len(hyps[u]) else hyps[u][0] for n in range(N) for u in range(U)]
        err = error_counts(self.tokenizer, slots, refs, self.opts.unit, dev)
        s = self.model.hypothesis_logp(encode_feature, encode_len, ids.to(dev), lens.to(dev))
        loss, exp_err, best_err = mwer_from_scores(s, err, count.to(dev), N)
        return loss, {'exp_err': exp_err.detach(), 'best_err': best_err}

    __call__ = forward
