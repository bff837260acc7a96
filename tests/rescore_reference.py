"""Host reference of two-pass decoding (checker only; the product path is src/rescore.py + csrc/rescore.hip): numpy
float64 scores of a hypothesis under the CTC head, the attention decoder and an LM, their combination and the ranking.
The acoustic quantities come from the CPU oracle (oracle/asr_oracle.py) run in float64."""
import numpy as np
import torch

from oracle import asr_oracle as AO

EOS = 1


def log_softmax(x):
    x = np.asarray(x, np.float64)
    m = x.max(-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))


def seq_logp(logits, targets, normalized=False):
    """tok[m] = log softmax(logits[m])[targets[m]] (0 where targets[m] < 0) in float64"""
    lp = np.asarray(logits, np.float64) if normalized else log_softmax(logits)
    t = np.asarray(targets)
    return np.where(t >= 0, lp[np.arange(len(t)), np.maximum(t, 0)], 0.0)


def ctc_logp(lp, y, blank=0):
    """log p_ctc(y | lp) for log-probs lp [T,V]: the forward variable over the blank-extended labels, one vector
    operation per frame (np.logaddexp.reduce over the up to three predecessors)"""
    lp = np.asarray(lp, np.float64)
    T = lp.shape[0]
    ext = np.full(2 * len(y) + 1, blank, dtype=np.int64)
    ext[1::2] = y
    S = len(ext)
    if T == 0:
        return 0.0 if len(y) == 0 else -np.inf
    skip = np.zeros(S, dtype=bool)
    skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
    a = np.full(S, -np.inf)
    a[:2] = lp[0, ext[:2]]
    with np.errstate(all='ignore'):
        for t in range(1, T):
            pad = np.concatenate([[-np.inf, -np.inf], a])
            p1 = pad[1:1 + S]
            p2 = np.where(skip, pad[:S], -np.inf)
            st = np.stack([a, p1, p2])
            m = st.max(0)
            a = np.where(np.isneginf(m), -np.inf, m + np.log(np.exp(st - np.where(np.isneginf(m), 0, m)).sum(0))) \
                + lp[t, ext]
        return float(np.logaddexp.reduce(a[-2:]))


def att_logp(att_logits, y):
    """s_att and its tokens from the teacher-forced logits [>= n+1, V] of y_1..y_n, <eos>"""
    tgt = list(y) + [EOS]
    tok = seq_logp(np.asarray(att_logits, np.float64)[:len(tgt)], tgt)
    return float(sum(tok.tolist())), tok


def combine(ctc, att, lm, ctc_weight, lm_weight):
    if ctc == -np.inf:
        return -np.inf
    return ctc_weight * ctc + (1.0 - ctc_weight) * att + (lm_weight * lm if lm_weight > 0 else 0.0)


def rank(scores):
    """indices, best first: descending score, ties by first-pass rank, -inf last"""
    idx = list(range(len(scores)))
    out = []
    while idx:                                  # selection: the first of the largest remaining
        best = idx[0]
        for i in idx[1:]:
            if scores[i] > scores[best]:
                best = i
        out.append(best)
        idx.remove(best)
    return out


def f64_state_dict(sd):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


def acoustic_scores(sd64, cfg, feat, flen, hyps):
    """(s_ctc, s_att) float64 lists for the hypotheses of ONE utterance (feat [1,T,D], flen [1]) from the CPU oracle's
    asr_forward in float64, teacher-forced on every hypothesis"""
    Lmax = max(len(h) for h in hyps) + 1
    teacher = torch.zeros((len(hyps), Lmax), dtype=torch.long)
    for r, h in enumerate(hyps):
        teacher[r, :len(h)] = torch.tensor(list(h), dtype=torch.long)
        teacher[r, len(h)] = EOS
    n = len(hyps)
    with torch.no_grad():
        ctc_out, enc_len, att_out, _, _ = AO.asr_forward(sd64, cfg, feat.double().repeat(n, 1, 1), flen.repeat(n), Lmax,
                                                         teacher=teacher)
    lp = ctc_out[0].numpy()
    s_ctc = [ctc_logp(lp, list(h)) for h in hyps]
    s_att = [att_logp(att_out[r].numpy(), list(h))[0] for r, h in enumerate(hyps)]
    return s_ctc, s_att, lp
