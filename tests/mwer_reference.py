"""Host reference of MWER training (checker only; the product path is src/mwer.py + csrc/mwer.hip + csrc/rescore.hip):
torch float64 with autograd on the CPU - seq_logp and its gradient, the MWER loss by literal softmax, and the whole
criterion on the CPU oracle (oracle/asr_oracle.py) without dropout.  Also the fixed inputs the CPU and GPU end-to-end
tests share."""
import functools

import numpy as np
import torch

import rescore_cases as RC
from helpers import CASES, load_golden, golden_state_dict
from oracle import asr_oracle as AO

EOS = 1


# ---- kernels ----------------------------------------------------------------------------------------------------------
def seq_logp(x, target, seg_off):
    """x [M,V] float64 (may require grad), target [M] (< 0: skipped), seg_off [R+1] -> (tok [M], seq [R], lse [M]);
    differentiable"""
    x = x.double()
    target = torch.as_tensor(target, dtype=torch.long)
    lse = torch.logsumexp(x, -1)
    tok = x.gather(1, target.clamp(min=0).unsqueeze(1)).squeeze(1) - lse
    tok = torch.where(target >= 0, tok, torch.zeros_like(tok))
    M = x.shape[0]
    seq = []
    for r in range(len(seg_off) - 1):
        a, b = max(0, int(seg_off[r])), min(M, int(seg_off[r + 1]))
        seq.append(tok[a:b].sum() if b > a else tok.new_zeros(()))
    seq = torch.stack(seq) if seq else tok.new_zeros((0,))
    return tok, seq, torch.where(target >= 0, lse, torch.zeros_like(lse))


def mwer_loss(s, err, count):
    """s [N,U] float64 (may require grad), err [N,U] integers, count [U] -> (loss_u [U], exp_err_u [U], p [N,U]) by the
    literal definition: softmax over the valid hypotheses, errors minus their mean"""
    N, U = s.shape
    e = torch.as_tensor(np.asarray(err), dtype=torch.float64).view(N, U)
    loss, ee = [], []
    p_all = torch.zeros((N, U), dtype=torch.float64)
    for u in range(U):
        n = int(count[u])
        if n == 0:
            loss.append(s.new_zeros(()))
            ee.append(s.new_zeros(()))
            continue
        p = torch.softmax(s[:n, u], 0)
        p_all[:n, u] = p.detach()
        loss.append((p * (e[:n, u] - e[:n, u].mean())).sum())
        ee.append((p * e[:n, u]).sum())
    return torch.stack(loss), torch.stack(ee), p_all


def closed_form_g(s, err, count):
    """dL_u/ds_{u,i} = p_i (e_i - sum_j p_j e_j), 0 on invalid slots"""
    with torch.no_grad():
        _, ee, p = mwer_loss(s.detach(), err, count)
    e = torch.as_tensor(np.asarray(err), dtype=torch.float64).view(s.shape)
    valid = torch.arange(s.shape[0]).unsqueeze(1) < torch.as_tensor(np.asarray(count)).unsqueeze(0)
    return torch.where(valid, p * (e - ee.unsqueeze(0)), torch.zeros_like(p))


def edit_distance(a, b):
    a, b = list(a), list(b)
    row = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        prev, row[0] = row[0], i
        for j, y in enumerate(b, 1):
            prev, row[j] = row[j], min(row[j] + 1, row[j - 1] + 1, prev + (x != y))
    return row[-1]


class Pieces:
    """a subword tokenizer's decode(): pieces joined, the word-boundary mark turned into a space"""
    TABLE = {3: '_he', 4: 'llo', 5: '_hello', 6: '_world', 7: '_wor', 8: 'ld', 9: '_there'}

    def decode(self, ids):
        return ''.join(self.TABLE[i] for i in ids).replace('_', ' ').strip()


# ---- the fixed end-to-end inputs -----------------------------------------------------------------------------------------
E2E_CASES = ["las_hybrid_loc", "las_gru", "las_loc_mh"]   # fused loop / step-by-step GRU / step-by-step, two heads
NBEST = 3
CE_WEIGHT = 0.1
# seeds of the synthetic lists, picked on the CPU so that on the float64 oracle every list with more than one hypothesis
# has its largest p below 0.9 and at least two different error counts (tests/test_mwer_cpu.py asserts it)
LIST_SEEDS = {"las_hybrid_loc": 0, "las_gru": 0, "las_loc_mh": 0}
# tokens per hypothesis: 0 (the hypothesis [] of the empty list) to 6.  Within a list the lengths differ by at most one
# token: a random-weight model gives every token about -log V, so a hypothesis two tokens shorter would take all the mass
HYP_LENS = [[5, 6, 5], [2, 2], []]       # utterance 1: a short list; utterance 2: an empty one
REF_LENS = [4, 3, 5]


def e2e_inputs(case):
    """-> (feat [3,37,D], feat_len [3], txt [3,5] zero-padded references, lists: per utterance its hypothesis lists)"""
    D, V = CASES[case][1], CASES[case][2]
    feat, flen = RC.utterances(case, D)
    rs = np.random.RandomState(4000 + LIST_SEEDS[case])
    txt = torch.zeros((len(REF_LENS), max(REF_LENS)), dtype=torch.long)
    for u, n in enumerate(REF_LENS):
        txt[u, :n] = torch.from_numpy(rs.randint(3, V, size=n))
    lists = []
    for u, lens in enumerate(HYP_LENS):
        ref = txt[u, :REF_LENS[u]].tolist()
        hyps = []
        for i, n in enumerate(lens):
            y = [int(t) for t in rs.randint(3, V, size=n)]
            k = min(n, len(ref), i + 1)
            y[:k] = ref[:k]                           # i + 1 tokens of the reference: the error counts differ
            hyps.append(y)
        lists.append(hyps)
    return feat, flen, txt, lists


def pack(lists, nbest):
    """the layout of src/mwer.pack_nbest for lists WITHOUT repeats or <eos>, written out independently"""
    U = len(lists)
    kept = [(h[:nbest] if h else [[]]) for h in lists]
    L = max(len(y) for h in kept for y in h) + 1
    ids = torch.zeros((nbest * U, L), dtype=torch.long)
    lens = torch.zeros((nbest * U,), dtype=torch.long)
    for u, h in enumerate(kept):
        for n in range(nbest):
            y = h[n] if n < len(h) else h[0]
            ids[n * U + u, :len(y)] = torch.tensor(y, dtype=torch.long)
            ids[n * U + u, len(y)] = EOS
            lens[n * U + u] = len(y) + 1
    return ids, lens, [len(h) for h in kept], kept


@functools.lru_cache(maxsize=None)
def criterion(case):
    """The whole MWER step of `case` on the float64 oracle (dropout 0, unit token): a dict with loss, mwer, base, s,
    p, err, count and grads (name -> float64 array).  Computed once per process."""
    g = load_golden(case)
    cfg = CASES[case][0]
    feat, flen, txt, lists = e2e_inputs(case)
    sd = {k: (v.double().requires_grad_(True) if v.is_floating_point() else v)
          for k, v in golden_state_dict(g).items()}
    ids, lens, count, kept = pack(lists, NBEST)
    U, N = len(lists), NBEST
    L_ref = int((txt != 0).sum(-1).max())
    enc, enc_len = AO.encoder_forward(sd, cfg['encoder'], feat.double(), flen)
    ctc_out = AO.ctc_head(sd, enc) if cfg['ctc_weight'] > 0 else None
    att_out, _, _ = AO.attention_decode(sd, cfg['attention'], cfg['decoder'], enc, enc_len, L_ref, txt)
    base, _, _ = AO.asr_losses(cfg, ctc_out, enc_len, att_out, txt)
    L = ids.shape[1]
    logits, _, _ = AO.attention_decode(sd, cfg['attention'], cfg['decoder'], enc.repeat(N, 1, 1), enc_len.repeat(N), L,
                                       ids)
    V = logits.shape[-1]
    target = torch.where(torch.arange(L).unsqueeze(0) < lens.unsqueeze(1), ids, torch.full_like(ids, -1))
    _, s, _ = seq_logp(logits.reshape(N * U * L, V), target.reshape(-1), [r * L for r in range(N * U + 1)])
    refs = [[t for t in row if t != 0] for row in txt.tolist()]
    err = np.zeros((N, U), dtype=np.int32)
    for u in range(U):
        for n in range(N):
            err[n, u] = edit_distance(kept[u][n] if n < count[u] else kept[u][0], refs[u])
    loss_u, ee, p = mwer_loss(s.view(N, U), err, count)
    mwer = loss_u.mean()
    loss = mwer + CE_WEIGHT * base
    loss.backward()
    grads = {k: v.grad.numpy().copy() for k, v in sd.items() if v.is_floating_point() and v.grad is not None}
    return dict(loss=float(loss.detach()), mwer=float(mwer.detach()), base=float(base.detach()),
                s=s.detach().numpy().copy(), p=p.numpy(), err=err, count=count, grads=grads,
                exp_err=float(ee.detach().mean()), best_err=float(err[0].mean()), enc_len=enc_len)
