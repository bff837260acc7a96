"""float64 mirror of pruned transducer training (Kuang et al. 2022), written from the definitions, for the rnnt_prune
tests.  Plain torch / numpy on the CPU; every gradient comes from float64 autograd.

 * diag_lnp         ln P of one utterance from lpb / lpl [T, U+1] (one logaddexp per anti-diagonal, any dtype / device)
 * simple_pass      the additive joiner am[t] + lm[u]: nll, the row quantities, the occupations c / eb / el and the
                    gradients with respect to am and lm
 * window_sums / ranges   the pruning rule, with the margin between the best and the second-best window of every frame
 * band_lnp         ln P with everything outside the band impossible, on band-layout lpb / lpl (any dtype / device)
 * band_pass        nll and the gradient with respect to band logits [B, T, S, V]
 * joint_band       tanh(E[b,t] + P[b, min(s + k, U)])
 * PrunedHeadRef    float64 mirror of TransducerHead with the `prune:` block

Pruning rule, with E_b = max(0, U_b + 1 - S):
   raw(t) = argmax_{0 <= s <= E_b} sum_{u = s}^{min(s + S - 1, U_b)} occ(t, u), the lowest s among equal sums
   s'(0) = 0;  s'(t) = clamp(raw(t), s'(t-1), s'(t-1) + S - 1);  s(t) = max(s'(t), E_b - (T_b - 1 - t)(S - 1))
   frames beyond T_b repeat s(T_b - 1)."""
import numpy as np
import torch

import rnnt_reference as RR

NEG = float("-inf")


def diag_lnp(lpb, lpl, T, U):
    """lpb [T, U+1], lpl [T, >= max(U, 1)] -> ln P; differentiable in whatever dtype the inputs have"""
    dev = lpb.device
    pad = torch.full((1,), NEG, device=dev, dtype=lpb.dtype)
    prev, plo = torch.zeros((1,), device=dev, dtype=lpb.dtype), 0
    for d in range(1, T + U):
        ulo, uhi = max(0, d - (T - 1)), min(U, d)
        us = torch.arange(ulo, uhi + 1, device=dev)
        ts = d - us
        pp = torch.cat([pad, prev, pad])
        top = pp[us - plo + 1] + lpb[(ts - 1).clamp(min=0), us]
        left = pp[us - plo] + lpl[ts, (us - 1).clamp(min=0)]
        prev, plo = torch.logaddexp(top, left), ulo
    return prev[0] + lpb[T - 1, U]


def lattice_terms(lp, y, Tb, Ub, lnp_fn=diag_lnp):
    """lp [T, U1, V] log-probabilities (rows beyond Tb / Ub ignored) -> (ln P, lpb leaf [Tb, Ub+1], lpl leaf [Tb, max(Ub,
    1)]): the leaves are detached-from-nothing views that keep their gradient, so that after backward of ln P
    lpb.grad = eb and lpl.grad = el (the occupation of the blank and the label arc of every cell)"""
    lpb = lp[:Tb, :Ub + 1, 0]
    if Ub:
        lpl = lp[:Tb, :Ub].gather(2, y[:Ub].view(1, Ub, 1).expand(Tb, Ub, 1)).squeeze(2)
    else:
        lpl = lpb.new_zeros((Tb, 1))
    lpb.retain_grad()
    if Ub:
        lpl.retain_grad()
    return lnp_fn(lpb, lpl, Tb, Ub), lpb, lpl


def simple_pass(am, lm, txt, enc_len, txt_len, weight=None):
    """am [B,T,V], lm [B,U1,V] float64 -> dict of float64 results, zeros outside every lattice:
    lse, lpb, lpl, c, eb, el [B,T,U1]; nll [B]; dam, dlm = d (sum_b weight_b nll_b) / d am, d lm"""
    B, T, V = am.shape
    U1 = lm.shape[1]
    a = am.detach().double().clone().requires_grad_(True)
    l = lm.detach().double().clone().requires_grad_(True)
    out = {k: torch.zeros((B, T, U1), dtype=torch.float64) for k in ("lse", "lpb", "lpl", "c", "eb", "el")}
    nll, total = [], 0.0
    for b in range(B):
        Tb, Ub = int(enc_len[b]), int(txt_len[b])
        z = a[b, :Tb, None, :] + l[b, None, :Ub + 1, :]
        lse = torch.logsumexp(z, -1)
        lp = z - lse.unsqueeze(-1)
        lnp, lpb, lpl = lattice_terms(lp, txt[b].long(), Tb, Ub)
        w = 1.0 if weight is None else float(weight[b])
        lnp.backward(retain_graph=True)
        with torch.no_grad():
            out["lse"][b, :Tb, :Ub + 1] = lse
            out["lpb"][b, :Tb, :Ub + 1] = lpb
            out["eb"][b, :Tb, :Ub + 1] = lpb.grad
            if Ub:
                out["lpl"][b, :Tb, :Ub] = lpl
                out["el"][b, :Tb, :Ub] = lpl.grad
        nll.append(-lnp.detach())
        total = total + w * -lnp
    out["c"] = out["eb"] + out["el"]          # every path through a cell leaves it by one of its two arcs
    a.grad = l.grad = None
    total.backward()
    out.update(nll=torch.stack(nll), dam=a.grad.clone(), dlm=l.grad.clone(), occ=out["eb"] + out["el"])
    return out


def lattice_extreme(lpb, lpl, Tb, Ub):
    """the largest |alpha|, |beta| of one utterance from float64 lpb / lpl [>= Tb, >= Ub + 1] (plain loops)"""
    lpb, lpl = np.asarray(lpb, np.float64), np.asarray(lpl, np.float64)
    a = np.full((Tb, Ub + 1), -np.inf)
    bt = np.full((Tb, Ub + 1), -np.inf)
    for t in range(Tb):
        for u in range(Ub + 1):
            if t == 0 and u == 0:
                a[t, u] = 0.0
                continue
            x = a[t - 1, u] + lpb[t - 1, u] if t > 0 else -np.inf
            y = a[t, u - 1] + lpl[t, u - 1] if u > 0 else -np.inf
            a[t, u] = np.logaddexp(x, y)
    for t in range(Tb - 1, -1, -1):
        for u in range(Ub, -1, -1):
            if t == Tb - 1 and u == Ub:
                bt[t, u] = lpb[t, u]
                continue
            x = lpb[t, u] + bt[t + 1, u] if t + 1 < Tb else -np.inf
            y = lpl[t, u] + bt[t, u + 1] if u < Ub else -np.inf
            bt[t, u] = np.logaddexp(x, y)
    return float(max(np.abs(a).max(), np.abs(bt).max()))


# ---- the pruning rule ---------------------------------------------------------------------------------------------------
def window_sums(occ_row, Ub, S):
    """occ_row [U1] -> the E_b + 1 window sums, each added in ascending u"""
    E = max(0, Ub + 1 - S)
    sums = []
    for s in range(E + 1):
        w = occ_row.dtype.type(0)
        for u in range(s, min(s + S - 1, Ub) + 1):
            w = w + occ_row[u]
        sums.append(w)
    return sums


def ranges_one(occ, Tb, Ub, S):
    """occ [T, U1] numpy -> (s [T] int32, margin [T]): margin(t) = (best - second best window sum) / best of frame t
    (inf where the frame has one window, or where t = 0 or t >= T_b: the rule does not look at the sums there)"""
    T = occ.shape[0]
    E = max(0, Ub + 1 - S)
    s = np.zeros(T, np.int32)
    margin = np.full(T, np.inf)
    sp = last = 0
    for t in range(T):
        if t < Tb:
            sums = window_sums(occ[t], Ub, S)
            raw = int(np.argmax(np.array(sums)))        # the first of equal maxima
            if t > 0 and len(sums) > 1:
                srt = sorted(float(v) for v in sums)
                margin[t] = (srt[-1] - srt[-2]) / srt[-1] if srt[-1] > 0 else 0.0
            cur = 0 if t == 0 else min(max(raw, sp), sp + S - 1)
            sp = cur
            last = max(cur, E - (Tb - 1 - t) * (S - 1))
        s[t] = last
    return s, margin


def ranges(occ, enc_len, txt_len, S):
    """occ [B, T, U1] (numpy or tensor, any float dtype) -> (s int32 [B, T], margin [B, T])"""
    occ = occ.detach().cpu().numpy() if torch.is_tensor(occ) else np.asarray(occ)
    res = [ranges_one(occ[b], int(enc_len[b]), int(txt_len[b]), S) for b in range(occ.shape[0])]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


def feasible(Tb, Ub, S):
    return (Tb - 1) * (S - 1) >= max(0, Ub + 1 - S)


def check_invariants(s, Tb, Ub, S):
    """the four properties of the rule for one utterance (s [T])"""
    E = max(0, Ub + 1 - S)
    d = np.diff(s[:Tb].astype(np.int64))
    assert (d >= 0).all(), "non-decreasing"
    assert (d <= S - 1).all(), "at most S - 1 per frame"
    assert int(s[Tb - 1]) == E, "ends at E_b"
    assert (int(s[0]) == 0) == feasible(Tb, Ub, S), "starts at 0 exactly when feasible"
    assert (s[Tb:] == s[Tb - 1]).all(), "padded frames repeat the last start"


# ---- the band ---------------------------------------------------------------------------------------------------------------
def band_lnp(lpb, lpl, s, Tb, Ub, S, extreme=None):
    """lpb, lpl [T, S] in band layout (cell (t, k) stands for u = s[t] + k; any dtype / device, differentiable), s a list
    of ints -> ln P over the paths that stay inside the band, or None when there is none.  A cell is computed from its
    predecessors inside the band only, so no -inf ever enters the arithmetic."""
    alpha = {}
    for t in range(Tb):
        for k in range(S):
            u = s[t] + k
            if u > Ub:
                break
            if t == 0 and u == 0:
                alpha[(0, 0)] = lpb.new_zeros(())
                continue
            terms = []
            if t > 0 and (t - 1, u) in alpha:
                terms.append(alpha[(t - 1, u)] + lpb[t - 1, u - s[t - 1]])
            if k > 0 and (t, u - 1) in alpha:
                terms.append(alpha[(t, u - 1)] + lpl[t, k - 1])
            if terms:
                alpha[(t, u)] = terms[0] if len(terms) == 1 else torch.logaddexp(terms[0], terms[1])
    if extreme is not None:                 # the caller's list receives the largest |alpha| inside the band
        extreme.append(max(abs(float(v)) for v in alpha.values()) if alpha else 0.0)
    if (Tb - 1, Ub) not in alpha:
        return None
    return alpha[(Tb - 1, Ub)] + lpb[Tb - 1, Ub - s[Tb - 1]]


def band_terms(lp, y, s, Tb, Ub, S):
    """lp [T, S, V] log-probabilities in band layout -> (lpb [T, S], lpl [T, S]): lpl(t, k) = lp[t, k, y[s[t] + k]] where
    that label exists, 0 elsewhere (never read)"""
    T = lp.shape[0]
    idx = torch.zeros((T, S), dtype=torch.int64)
    for t in range(T):
        for k in range(S):
            u = s[t] + k
            if t < Tb and u < Ub:
                idx[t, k] = int(y[u])
    return lp[:, :, 0], lp.gather(2, idx.to(lp.device).unsqueeze(2)).squeeze(2)


def band_pass(z, txt, enc_len, txt_len, s, weight=None, extreme=None):
    """z [B, T, S, V] float64 band logits, s int [B, T] -> (nll [B] with +inf for an utterance without a path,
    d (sum_b weight_b nll_b) / dz with zeros outside the lattices and for such utterances)"""
    B, T, S, V = z.shape
    zz = z.detach().double().clone().requires_grad_(True)
    nll, total = [], 0.0
    for b in range(B):
        Tb, Ub = int(enc_len[b]), int(txt_len[b])
        sb = [int(v) for v in s[b]]
        lp = RR.log_probs(zz[b])
        lpb, lpl = band_terms(lp, txt[b], sb, Tb, Ub, S)
        lnp = band_lnp(lpb, lpl, sb, Tb, Ub, S, extreme)
        if lnp is None:
            nll.append(torch.tensor(float("inf"), dtype=torch.float64))
            continue
        nll.append(-lnp.detach())
        total = total + (1.0 if weight is None else float(weight[b])) * -lnp
    if torch.is_tensor(total):
        total.backward()
    grad = zz.grad if zz.grad is not None else torch.zeros_like(zz)
    return torch.stack(nll), grad.clone()


def joint_band(E, P, s, S):
    """E [B,T,J], P [B,U1,J], s int [B,T] -> H [B,T,S,J] = tanh(E[b,t] + P[b, min(s + k, U1 - 1)]) (differentiable)"""
    U1 = P.shape[1]
    idx = (torch.as_tensor(np.asarray(s), dtype=torch.int64).clamp(0, U1 - 1).unsqueeze(2) + torch.arange(S)).clamp(
        max=U1 - 1)                                                     # [B, T, S]
    B, T = idx.shape[:2]
    rows = P[torch.arange(B).view(B, 1, 1), idx]                        # [B, T, S, J]
    return torch.tanh(E.unsqueeze(2) + rows)


# ---- the head -----------------------------------------------------------------------------------------------------------------
class PrunedHeadRef(RR.HeadRef):
    """float64 mirror of a TransducerHead built with the `prune:` block: HeadRef plus lin_am and lin_lm"""

    def __init__(self, vocab_size, enc_dim, module, dim, layer, emb_dim, joint_dim):
        super().__init__(vocab_size, enc_dim, module, dim, layer, emb_dim, joint_dim)
        self.lin_am = torch.nn.Linear(enc_dim, vocab_size)
        self.lin_lm = torch.nn.Linear(dim, vocab_size)
        self.double()

    def load(self, head):
        sd = {k: v.detach().cpu().double() for k, v in head.state_dict().items()}
        extra = {k: sd[k] for k in ("lin_am.weight", "lin_am.bias", "lin_lm.weight", "lin_lm.bias")}

        class _Plain:                      # the head without the simple joiner, for HeadRef.load's completeness check
            def state_dict(self_inner):
                return {k: v for k, v in sd.items() if k not in extra}
        own = {k: v for k, v in self.state_dict().items()}
        base = RR.HeadRef(self.emb.num_embeddings, self.lin_enc.in_features, self.module, self.dim, self.layer,
                          self.emb.embedding_dim, self.lin_enc.out_features).load(_Plain())
        own.update(base.state_dict())
        own.update(extra)
        self.load_state_dict(own, strict=True)
        return self

    def param_map(self):
        m = super().param_map()
        for name in ("lin_am", "lin_lm"):
            m[name + ".weight"] = getattr(self, name).weight
            m[name + ".bias"] = getattr(self, name).bias
        return m

    def predict(self, txt):
        inp = torch.cat([txt.new_zeros((txt.shape[0], 1)), txt], dim=1)
        return self.rnn(self.emb(inp))[0]

    def simple(self, enc, txt, enc_len, txt_len):
        """-> (simple nll [B] (differentiable), occ [B,T,U1] detached)"""
        pred = self.predict(txt)
        am, lm = self.lin_am(enc), self.lin_lm(pred)
        B, T, U1 = enc.shape[0], enc.shape[1], pred.shape[1]
        occ = torch.zeros((B, T, U1), dtype=torch.float64)
        nll = []
        for b in range(B):
            Tb, Ub = int(enc_len[b]), int(txt_len[b])
            z = am[b, :Tb, None, :] + lm[b, None, :Ub + 1, :]
            lnp, lpb, lpl = lattice_terms(RR.log_probs(z), txt[b], Tb, Ub)
            gb, gl = torch.autograd.grad(lnp, [lpb, lpl] if Ub else [lpb, lpb], retain_graph=True)
            occ[b, :Tb, :Ub + 1] = gb
            if Ub:
                occ[b, :Tb, :Ub] += gl
            nll.append(-lnp)
        return torch.stack(nll), occ

    def pruned(self, enc, txt, enc_len, txt_len, s, S):
        """-> pruned nll [B] on the band `s` (int [B,T]), differentiable"""
        pred = self.predict(txt)
        H = joint_band(self.lin_enc(enc), self.lin_pred(pred), s, S)
        z = self.lin_out(H)
        nll = []
        for b in range(enc.shape[0]):
            Tb, Ub = int(enc_len[b]), int(txt_len[b])
            sb = [int(v) for v in s[b]]
            lpb, lpl = band_terms(RR.log_probs(z[b]), txt[b], sb, Tb, Ub, S)
            nll.append(-band_lnp(lpb, lpl, sb, Tb, Ub, S))
        return torch.stack(nll)


# ---- the cases of the range rule (shared by the CPU and the GPU test) -------------------------------------------------------
def range_diagnostics(occ, Tb, Ub, S):
    """which clauses of the rule decide a frame of one utterance: counts of frames where the monotone clamp binds
    (raw < s'(t-1)), where the step clamp binds (raw > s'(t-1) + S - 1), where the end constraint binds
    (s(t) > s'(t)), and where the best window sum is attained twice"""
    E = max(0, Ub + 1 - S)
    sp = 0
    d = dict(monotone=0, step=0, end=0, tie=0)
    for t in range(Tb):
        sums = [float(v) for v in window_sums(occ[t], Ub, S)]
        raw = int(np.argmax(np.array(sums)))
        d["tie"] += int(sums.count(max(sums)) > 1)
        if t > 0:
            d["monotone"] += int(raw < sp)
            d["step"] += int(raw > sp + S - 1)
            sp = min(max(raw, sp), sp + S - 1)
        d["end"] += int(E - (Tb - 1 - t) * (S - 1) > sp)
    return d


def _grid_occ(rng, B, T, U1):
    """multiples of 2^-10 below 1: every window sum of at most 32 of them is exact in f32 and in float64"""
    return (rng.integers(0, 1024, size=(B, T, U1)) / 1024.0).astype(np.float32)


def _peaks(rng, T, U1, starts, S):
    """half the mass on each of the S positions from starts[t] on: raw(t) = starts[t]"""
    occ = (_grid_occ(rng, 1, T, U1) / 64.0).astype(np.float32)      # still multiples of 2^-16, sums still exact
    for t, c in enumerate(starts):
        occ[0, t, c:c + S] = 0.5
    return occ


def lattice_range_case(seed, B=3, T=12, U=20, V=16, scale=2.0):
    """a simple-joiner batch whose occupations are spread over several cells -> (am, lm f32 [B,T,V] / [B,U+1,V], txt,
    enc_len, txt_len)"""
    g = torch.Generator().manual_seed(seed)
    am = torch.randn((B, T, V), generator=g) * scale
    lm = torch.randn((B, U + 1, V), generator=g) * scale
    txt = torch.randint(1, V, (B, U), generator=g)
    enc_len = [T, max(1, T - 3), max(1, T // 2)][:B]
    txt_len = [U, max(0, U - 5), U // 2][:B]
    return am, lm, txt, enc_len, txt_len


LATTICE_RANGE_SEEDS = (1, 6, 7)        # seeds for which the float64 mirror alone leaves under a tenth of the frames undecided
LATTICE_RANGE_S = 4
MIN_RANGE_MARGIN = 1e-3


def range_cases():
    """-> list of (name, occ f32 [B,T,U1], enc_len, txt_len, S)"""
    rng = np.random.default_rng(2022)
    cases = [
        ("short_transcript", _grid_occ(rng, 1, 4, 3), [4], [2], 5),                     # U_b + 1 <= S: all zeros
        ("one_frame", _grid_occ(rng, 1, 1, 4), [1], [3], 5),
        ("one_frame_infeasible", _grid_occ(rng, 1, 1, 9), [1], [8], 3),
        ("monotone", _peaks(rng, 6, 13, [0, 2, 0, 1, 4, 6], 3), [6], [12], 3),           # the peak walks backwards
        ("step", _peaks(rng, 5, 17, [0, 12, 13, 14, 14], 3), [5], [16], 3),             # the peak jumps ahead
        ("end", _peaks(rng, 8, 13, [0] * 8, 3), [8], [12], 3),                          # the mass never leaves u = 0
        ("tie", np.full((1, 5, 9), 0.25, np.float32), [5], [8], 3),
        ("infeasible", _grid_occ(rng, 1, 2, 11), [2], [10], 3),
        ("batch", _grid_occ(rng, 3, 9, 14), [9, 4, 6], [13, 5, 0], 4),                  # mixed lengths, padded frames
        ("wide", _grid_occ(rng, 2, 5, 80), [5, 3], [79, 70], 32),                       # more band starts than lanes, S = 32
        ("many_starts", _grid_occ(rng, 1, 70, 140), [70], [139], 2),
    ]
    return cases
