// Pruned transducer training (Kuang et al. 2022): the cell logic shared by the gfx950 kernels (rnnt_prune.hip) and the
// host build of the tests (tests/native/rnnt_prune_host.cpp).  The includer defines RNNT_HD (`__device__` or nothing)
// and includes rnnt.inc first (the length clamps).  Plain C++: no HIP call, f32 operations in one fixed order.
//
// Pruning bounds of one utterance with T_b frames, U_b labels and a band of S label positions per frame:
//   E_b   = max(0, U_b + 1 - S)                       the last band start
//   raw(t) = argmax_{0 <= s <= E_b} sum_{u = s}^{min(s + S - 1, U_b)} occ(t, u), the lowest s among equal sums
//   s'(0) = 0;  s'(t) = clamp(raw(t), s'(t-1), s'(t-1) + S - 1)
//   s(t)  = max(s'(t), E_b - (T_b - 1 - t)(S - 1))    so that the band can still reach E_b at the last frame
// s is non-decreasing, moves at most S - 1 per frame and ends at E_b; it starts at 0 exactly when the utterance is
// feasible, (T_b - 1)(S - 1) >= E_b.  An infeasible utterance has no path inside its band.

RNNT_HD inline int rnntp_last_start(int Ub, int S) { return Ub + 1 - S > 0 ? Ub + 1 - S : 0; }

RNNT_HD inline bool rnntp_feasible(int Tb, int Ub, int S) {
    return (long long)(Tb - 1) * (S - 1) >= (long long)rnntp_last_start(Ub, S);
}

// sum of occ_row[s .. min(s + S - 1, Ub)], in ascending u
RNNT_HD inline float rnntp_window(const float *occ_row, int s, int S, int Ub) {
    const int hi = s + S - 1 < Ub ? s + S - 1 : Ub;
    float w = 0.f;
    for (int u = s; u <= hi; ++u) w += occ_row[u];
    return w;
}

// a candidate (value, start) replaces the best one when its sum is larger, or equal with a lower start; a NaN sum is
// no candidate (arg < 0: nothing yet)
RNNT_HD inline void rnntp_better(float v, int s, float *best, int *arg) {
    if (v > *best || (*arg < 0 && v == v) || (v == *best && s < *arg)) {
        *best = v;
        *arg = s;
    }
}

// one frame of the scan: *sp is s'(t-1) on entry and s'(t) on return; the result is s(t)
RNNT_HD inline int rnntp_step(int raw, int *sp, int t, int Tb, int Ub, int S) {
    const int E = rnntp_last_start(Ub, S);
    int cur = 0;
    if (t > 0) {
        const int lo = *sp, hi = *sp + S - 1;
        cur = raw < lo ? lo : (raw > hi ? hi : raw);
    }
    *sp = cur;
    const long long need = (long long)E - (long long)(Tb - 1 - t) * (S - 1);
    return need > cur ? (int)need : cur;
}

// the whole rule for one utterance by one thread: occ [T, U1] -> s [T] (frames beyond T_b repeat s(T_b - 1))
RNNT_HD inline void rnntp_ranges_one(const float *occ, int T, int U1, int Tb, int Ub, int S, int *s_out) {
    const int E = rnntp_last_start(Ub, S);
    int sp = 0, last = 0;
    for (int t = 0; t < T; ++t) {
        if (t < Tb) {
            float best = -INFINITY;
            int arg = -1;
            for (int s = 0; s <= E; ++s) rnntp_better(rnntp_window(occ + (size_t)t * U1, s, S, Ub), s, &best, &arg);
            last = rnntp_step(arg < 0 ? 0 : arg, &sp, t, Tb, Ub, S);
        }
        s_out[t] = last;
    }
}

// band cell (t, k) of an utterance stands for u = s(t) + k; s is clamped, never trusted
RNNT_HD inline int rnntp_band_u(int s, int k, int U1) { return (s < 0 ? 0 : (s > U1 - 1 ? U1 - 1 : s)) + k; }
