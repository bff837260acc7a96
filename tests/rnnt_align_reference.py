"""Reference of the transducer forced alignment (csrc/rnnt_align.inc), for the CPU and GPU tests.

 * align_f32: numpy float32, the same operations in the same order as the kernel (one add per arc, one compare per
   cell, ties to the blank arc, NaN taken), so its outputs are compared bit for bit;
 * enumerate_best: float64 over every path of a small lattice (T, U <= 7);
 * viterbi64: the same recurrence in float64 and the largest |delta| it met;
 * path_score64: a given path scored in float64.

One utterance at a time: lpb / lpl are [T, U1] arrays (any padding), T_b and U_b the utterance's sizes."""
import itertools

import numpy as np

NEG_INF = float("-inf")


def _walk(lpb, lpl, Tb, Ub, dtype):
    """delta [Tb, Ub+1] and the bit of every cell (True: the label arc was taken), cells visited by anti-diagonals"""
    ninf = dtype(NEG_INF)
    delta = np.full((Tb, Ub + 1), ninf, dtype)
    taken = np.zeros((Tb, Ub + 1), bool)
    delta[0, 0] = dtype(0)
    with np.errstate(invalid="ignore", over="ignore"):
        for d in range(1, Tb + Ub):
            for u in range(max(0, d - (Tb - 1)), min(d, Ub) + 1):
                t = d - u
                a = dtype(delta[t - 1, u] + dtype(lpb[t - 1, u])) if t > 0 else ninf
                b = dtype(delta[t, u - 1] + dtype(lpl[t, u - 1])) if u > 0 else ninf
                tk = bool(b > a) or bool(b != b)
                taken[t, u] = tk
                delta[t, u] = b if tk else a
        score = dtype(delta[Tb - 1, Ub] + dtype(lpb[Tb - 1, Ub]))
    return delta, taken, score


def _backtrace(taken, Tb, Ub):
    frames, done = [0] * Ub, [0] * Tb
    t, u = Tb - 1, Ub
    done[t] = u
    while t > 0 or u > 0:
        if t == 0 or (u > 0 and taken[t, u]):
            u -= 1
            frames[u] = t
        else:
            t -= 1
            done[t] = u
    return frames, done


def align_f32(lpb, lpl, Tb, Ub):
    """-> dict(frames int32 [U1-1], labels_done int32 [T], tok_logp float32 [U1-1], score float32) with the kernel's
    padding: -1 / 0 beyond the utterance, and everywhere when the score is -inf or NaN"""
    lpb, lpl = np.asarray(lpb, np.float32), np.asarray(lpl, np.float32)
    T, U1 = lpb.shape
    _, taken, score = _walk(lpb, lpl, Tb, Ub, np.float32)
    frames = np.full(U1 - 1, -1, np.int32)
    done = np.full(T, -1, np.int32)
    logp = np.zeros(U1 - 1, np.float32)
    if score > NEG_INF:
        f, dn = _backtrace(taken, Tb, Ub)
        frames[:Ub] = f
        done[:Tb] = dn
        for u in range(Ub):
            logp[u] = lpl[f[u], u]
    return dict(frames=frames, labels_done=done, tok_logp=logp, score=np.float32(score))


def viterbi64(lpb, lpl, Tb, Ub):
    """-> (frames, score, A): the float64 optimum and the largest finite |delta| of its lattice (0 when none)"""
    lpb, lpl = np.asarray(lpb, np.float64), np.asarray(lpl, np.float64)
    delta, taken, score = _walk(lpb, lpl, Tb, Ub, np.float64)
    fin = np.abs(delta[np.isfinite(delta)])
    A = float(fin.max()) if fin.size else 0.0
    frames = _backtrace(taken, Tb, Ub)[0] if score > NEG_INF else None
    return frames, float(score), A


def path_score64(lpb, lpl, frames, Tb, Ub):
    """the log-probability, in float64, of the path that emits label u at frame frames[u]"""
    lpb, lpl = np.asarray(lpb, np.float64), np.asarray(lpl, np.float64)
    s, u = 0.0, 0
    for t in range(Tb):
        while u < Ub and frames[u] == t:
            s += lpl[t, u]
            u += 1
        s += lpb[t, u]
    assert u == Ub, "not a path: %r" % (list(frames),)
    return s


def enumerate_best(lpb, lpl, Tb, Ub):
    """every path of the lattice (non-decreasing emission frames), float64 -> (frames of the best, its score)"""
    assert Tb <= 7 and Ub <= 7
    best, best_f = NEG_INF, None
    for f in itertools.combinations_with_replacement(range(Tb), Ub):
        s = path_score64(lpb, lpl, f, Tb, Ub)
        if best_f is None or s > best:
            best, best_f = s, list(f)
    return best_f, best


def random_lattice(T, U, seed, V=5, scale=3.0):
    """lpb / lpl [T, U+1] float32 of a random V-way head (logits scaled by `scale`, labels in 1..V-1)"""
    rng = np.random.RandomState(seed)
    z = rng.randn(T, U + 1, V) * scale
    m = z.max(-1, keepdims=True)
    lp = z - (m + np.log(np.exp(z - m).sum(-1, keepdims=True)))
    y = rng.randint(1, V, size=U)
    lpb = lp[:, :, 0].astype(np.float32)
    lpl = np.zeros((T, U + 1), np.float32)
    for u in range(U):
        lpl[:, u] = lp[:, u, y[u]]
    return np.ascontiguousarray(lpb), np.ascontiguousarray(lpl)
