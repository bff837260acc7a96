"""Host reference of CTC forced alignment (checker only; the product path is csrc/ctc.hip: ctc_viterbi_kernel).

`viterbi` is a numpy float32 Viterbi over the blank-extended label sequence with the contract's tie rule: a candidate
replaces the current best only if strictly greater, tried in the order stay, s-1, s-2; the path ends in state S-1
unless delta[S-2] is strictly greater.  The arithmetic per state and frame is one float32 add behind float32 compares,
in the kernel's order, so the kernel's score equals this one bit for bit.  `brute_force` enumerates every admissible
state path (tiny shapes only) and is what `viterbi` itself is checked against.
"""
import itertools

import numpy as np


def ext_labels(target, blank=0):
    ext = np.full(2 * len(target) + 1, blank, dtype=np.int64)
    ext[1::2] = np.asarray(target, dtype=np.int64)
    return ext


def viterbi(lp, target, blank=0):
    """lp [T,V] float32 log-probs of ONE utterance (its T_b frames only), target: its L_b labels ->
    (states [T] int32, tokens [T] int32, spans [L_b,2] int32, score float32), or (None, None, None, score) when no
    path has non-zero probability (score -inf) or a label lies outside [0,V) (score NaN)."""
    lp = np.asarray(lp, dtype=np.float32)
    T, V = lp.shape
    target = [int(v) for v in target]
    L = len(target)
    if any(c < 0 or c >= V for c in target):
        return None, None, None, np.float32(np.nan)
    if T <= 0:
        return None, None, None, np.float32(0.0 if L == 0 else -np.inf)
    ext = ext_labels(target, blank)
    S = len(ext)
    ninf = np.float32(-np.inf)
    delta = np.full(S, ninf, dtype=np.float32)
    delta[0] = lp[0, ext[0]]
    if S > 1:
        delta[1] = lp[0, ext[1]]
    skip = np.zeros(S, dtype=bool)                     # s odd, s >= 2 and a different label two states back
    skip[3::2] = ext[3::2] != ext[1:-2:2]
    bp = np.zeros((T, S), dtype=np.int8)
    for t in range(1, T):
        a1 = np.concatenate(([ninf], delta[:-1]))
        a2 = np.where(skip, np.concatenate(([ninf, ninf], delta[:-2]))[:S], ninf)
        best, jump = delta.copy(), np.zeros(S, dtype=np.int8)
        for k, cand in ((1, a1), (2, a2)):             # strictly greater only, tried in the order 0, 1, 2
            m = cand > best
            best[m], jump[m] = cand[m], k
        delta = (best + lp[t, ext]).astype(np.float32)
        bp[t] = jump
    s = S - 1
    if S >= 2 and delta[S - 2] > delta[S - 1]:
        s = S - 2
    score = delta[s]
    if not score > ninf:
        return None, None, None, score
    states = np.empty(T, dtype=np.int32)
    for t in range(T - 1, -1, -1):
        states[t] = s
        s -= int(bp[t, s])
    tokens = ext[states].astype(np.int32)
    spans = np.full((L, 2), -1, dtype=np.int32)
    for l in range(L):
        at = np.nonzero(states == 2 * l + 1)[0]
        spans[l] = (at[0], at[-1] + 1)
    return states, tokens, spans, score


def align_batch(lp_tbv, targets, input_lengths, target_lengths, blank=0):
    """Batched form with the device op's output contract: lp [T,B,V], targets [B,Lmax] ->
    states, tokens int32 [B,T], spans int32 [B,Lmax,2], score float32 [B] (-1 where nothing is aligned)."""
    lp_tbv = np.asarray(lp_tbv, dtype=np.float32)
    T, B, _ = lp_tbv.shape
    targets = np.asarray(targets).reshape(B, -1)
    Lmax = targets.shape[1]
    states = np.full((B, T), -1, dtype=np.int32)
    tokens = np.full((B, T), -1, dtype=np.int32)
    spans = np.full((B, Lmax, 2), -1, dtype=np.int32)
    score = np.zeros(B, dtype=np.float32)
    for b in range(B):
        Tb = min(int(input_lengths[b]), T)
        Lb = max(min(int(target_lengths[b]), Lmax), 0)
        st, tk, sp, sc = viterbi(lp_tbv[:max(Tb, 0), b], targets[b, :Lb], blank)
        score[b] = sc
        if st is not None:
            states[b, :Tb], tokens[b, :Tb], spans[b, :Lb] = st, tk, sp
    return states, tokens, spans, score


def feasible(T, target):
    """the count rule: T frames hold `target` iff T >= L + number of adjacent repeats (and T > 0 or L == 0)"""
    L = len(target)
    rep = sum(1 for i in range(1, L) if target[i] == target[i - 1])
    return T >= L + rep and (T > 0 or L == 0)


def brute_force(lp, target, blank=0):
    """max over every admissible state path, in float64: (best score or -inf, number of admissible paths)"""
    lp = np.asarray(lp, dtype=np.float64)
    T = lp.shape[0]
    ext = ext_labels(target, blank)
    S = len(ext)
    best, count = -np.inf, 0
    for path in itertools.product(range(S), repeat=T):
        if path[0] > 1 or path[-1] < S - 2:
            continue
        ok = True
        for t in range(1, T):
            d = path[t] - path[t - 1]
            if d < 0 or d > 2 or (d == 2 and not ((path[t] & 1) and ext[path[t]] != ext[path[t] - 2])):
                ok = False
                break
        if not ok:
            continue
        count += 1
        best = max(best, float(sum(lp[t, ext[path[t]]] for t in range(T))))
    return best, count
