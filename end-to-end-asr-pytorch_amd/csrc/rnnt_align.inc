// RNN-transducer forced alignment: the best (Viterbi) path of one utterance through its lattice, shared by the gfx950
// kernel (rnnt_align.hip) and the host build of the tests (tests/native/rnnt_align_host.cpp).  Included after rnnt.inc
// (lengths, diagonal ranges, rnnt_coef); the includer defines RNNT_HD.
// Plain C++: no HIP call, no float atomics, f32 operations in one fixed order.
//
// Cells (t, u), 0 <= t < T_b, 0 <= u <= U_b, stored at t * U1 + u as the row pass writes lpb / lpl:
//   delta(0,0) = 0
//   a = delta(t-1,u) + lpb(t-1,u)   (t > 0, else -inf)     the blank arc
//   b = delta(t,u-1) + lpl(t,u-1)   (u > 0, else -inf)     the label arc
//   the label arc is taken iff (b > a) or (b != b);  delta(t,u) = taken ? b : a
//   score = delta(T_b-1, U_b) + lpb(T_b-1, U_b)
// One add per arc and one compare per cell.  Ties go to the blank arc, so among equal-scoring paths every label is
// emitted as early as possible; a NaN on either arc reaches the score.
// Backpointers: one bit per cell (1 = the label arc was taken), bit (u & 63) of the 64-bit word
// bp[d * nslot + (u >> 6)] of anti-diagonal d = t + u, nslot = ceil(U1 / 64).  A word holds the bits of 64 consecutive
// u of one diagonal: on the device it is one wave's ballot.

RNNT_HD inline int rnnt_align_nslot(int U1) { return (U1 + 63) >> 6; }

// prev: the previous anti-diagonal (d - 1), indexed by u
RNNT_HD inline float rnnt_align_cell(int t, int u, int U1, const float *lpb, const float *lpl, const float *prev,
                                     bool *taken) {
    *taken = false;
    if (t == 0 && u == 0) return 0.f;
    float a = -INFINITY, b = -INFINITY;
    if (t > 0) a = prev[u] + lpb[(size_t)(t - 1) * U1 + u];
    if (u > 0) b = prev[u - 1] + lpl[(size_t)t * U1 + u - 1];
    *taken = (b > a) || (b != b);
    return *taken ? b : a;
}

// Anti-diagonal d for lane tid of nthr (nthr = 1 or a multiple of 64): the lane's cells are u = base + tid with base a
// multiple of 64, so lane l of a wave owns bit l of the word of its slot.  put(d, u, taken) is called by every lane
// of a wave whose slot holds a cell of the diagonal (uniformly: a collective may sit inside), with taken = false for
// the lanes beside the diagonal; u >> 6 < nslot in every call.  diag: two diagonals [2][U1]; the lane that owns cell
// (T_b - 1, U_b) writes *score.
template <class Put>
RNNT_HD inline void rnnt_align_diag(int d, int tid, int nthr, int Tb, int Ub, int U1, const float *lpb, const float *lpl,
                                    float *diag, float *score, Put put) {
    int ulo, uhi;
    rnnt_diag_range(d, Tb, Ub, &ulo, &uhi);
    const float *prev = diag + (size_t)((d + 1) & 1) * U1;
    float *cur = diag + (size_t)(d & 1) * U1;
    for (int base = ulo & ~63; base <= uhi; base += nthr) {
        const int u = base + tid;
        if ((u & ~63) > uhi) continue;      // the whole slot lies beside the diagonal
        bool taken = false;
        if (u >= ulo && u <= uhi) {
            const int t = d - u;
            const float v = rnnt_align_cell(t, u, U1, lpb, lpl, prev, &taken);
            cur[u] = v;
            if (d == Tb + Ub - 1) *score = v + lpb[(size_t)t * U1 + u];   // the one cell (T_b - 1, U_b)
        }
        put(d, u, taken);
    }
}

// the T_b + U_b anti-diagonals; sync(): a barrier of every lane that walks, once per diagonal
template <class Sync, class Put>
RNNT_HD inline void rnnt_align_walk(int tid, int nthr, int Tb, int Ub, int U1, const float *lpb, const float *lpl,
                                    float *diag, float *score, Sync sync, Put put) {
    const int nd = Tb + Ub;
    for (int d = 0; d < nd; ++d) {
        rnnt_align_diag(d, tid, nthr, Tb, Ub, U1, lpb, lpl, diag, score, put);
        sync();
    }
}

// One lane follows the bits back from (T_b - 1, U_b).  A label arc into (t, u) emitted y_u at frame t: frames[u - 1]
// = t; a blank arc out of (t, u) left frame t with u labels done: labels_done[t] = u.  Only behind a score above -inf
// (every bit on the path was written then); at t == 0 and at u == 0 the only arc there is is taken whatever the bit
// says, so no index leaves the lattice.
RNNT_HD inline void rnnt_align_backtrace(int Tb, int Ub, int U1, const unsigned long long *bp, int *frames,
                                         int *labels_done) {
    const int nslot = rnnt_align_nslot(U1);
    int t = Tb - 1, u = Ub;
    labels_done[t] = u;
    while (t > 0 || u > 0) {
        const unsigned long long w = bp[(size_t)(t + u) * nslot + (u >> 6)];
        const bool label = t == 0 || (u > 0 && ((w >> (u & 63)) & 1));
        if (label) {
            --u;
            frames[u] = t;
        } else {
            --t;
            labels_done[t] = u;
        }
    }
}

// Every lane, after the backtrace is visible: the per-token outputs of the U1 - 1 label positions and the padding.
// ok: the utterance has a path (score above -inf, not NaN).  tok_post (with alpha, beta, nll; all three or none) is
// the posterior of the chosen emission arc, rnnt_coef's el at the emitting cell.
RNNT_HD inline void rnnt_align_tokens(int tid, int nthr, bool ok, int T, int Tb, int Ub, int U1, const float *lpb,
                                      const float *lpl, const float *alpha, const float *beta, float nll, int *frames,
                                      int *labels_done, float *tok_logp, float *tok_post) {
    for (int u = tid; u < U1 - 1; u += nthr) {
        if (ok && u < Ub) {
            const int t = frames[u];
            tok_logp[u] = lpl[(size_t)t * U1 + u];
            if (tok_post) tok_post[u] = rnnt_coef(t, u, Tb, Ub, U1, alpha, beta, lpb, lpl, nll).el;
        } else {
            frames[u] = -1;
            tok_logp[u] = 0.f;
            if (tok_post) tok_post[u] = 0.f;
        }
    }
    for (int t = tid; t < T; t += nthr)
        if (!ok || t >= Tb) labels_done[t] = -1;
}
