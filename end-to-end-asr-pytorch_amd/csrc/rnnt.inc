// RNN-transducer lattice (Graves 2012): the cell recursions, the anti-diagonal walk and the coefficients of the
// closed-form gradient, shared by the gfx950 kernels (rnnt.hip) and the host build of the tests
// (tests/native/rnnt_host.cpp).  The includer defines RNNT_HD (`__device__` or nothing).
// Plain C++: no HIP call, no float atomics, f32 operations in one fixed order.
//
// One utterance: T frames, U labels, cells (t, u) with 0 <= t < T and 0 <= u <= U, stored at t * U1 + u (U1 = padded
// U + 1).  lpb(t, u) = log p(blank | t, u), lpl(t, u) = log p(y_{u+1} | t, u) (lpl is never read at u = U).
//   alpha(0,0) = 0;  alpha(t,u) = logaddexp(alpha(t-1,u) + lpb(t-1,u), alpha(t,u-1) + lpl(t,u-1))
//   beta(T-1,U) = lpb(T-1,U);  beta(t,u) = logaddexp(lpb(t,u) + beta(t+1,u), lpl(t,u) + beta(t,u+1))
//   ln P = alpha(T-1,U) + lpb(T-1,U) = beta(0,0)
// A term whose neighbour lies outside the lattice is dropped.

// lengths are clamped, never trusted: 1 <= T_b <= T, 0 <= U_b <= U1 - 1
RNNT_HD inline int rnnt_clamp_T(long long n, int T) { return n < 1 ? 1 : (n > T ? T : (int)n); }
RNNT_HD inline int rnnt_clamp_U(long long n, int U1) { return n < 0 ? 0 : (n > U1 - 1 ? U1 - 1 : (int)n); }

RNNT_HD inline float rnnt_log_add(float a, float b) {
    const float m = a > b ? a : b;
    if (m == -INFINITY) return -INFINITY;
    return m + log1pf(expf(-fabsf(a - b)));
}

// the cells of anti-diagonal d (t + u = d) are u in [*ulo, *uhi]
RNNT_HD inline void rnnt_diag_range(int d, int Tb, int Ub, int *ulo, int *uhi) {
    *ulo = d - (Tb - 1) > 0 ? d - (Tb - 1) : 0;
    *uhi = d < Ub ? d : Ub;
}

// prev: the previous anti-diagonal (d - 1), indexed by u
RNNT_HD inline float rnnt_alpha_cell(int t, int u, int U1, const float *lpb, const float *lpl, const float *prev) {
    if (t == 0 && u == 0) return 0.f;
    float a = -INFINITY, b = -INFINITY;
    if (t > 0) a = prev[u] + lpb[(size_t)(t - 1) * U1 + u];
    if (u > 0) b = prev[u - 1] + lpl[(size_t)t * U1 + u - 1];
    return rnnt_log_add(a, b);
}

// prev: the next anti-diagonal (d + 1), indexed by u
RNNT_HD inline float rnnt_beta_cell(int t, int u, int Tb, int Ub, int U1, const float *lpb, const float *lpl,
                                    const float *prev) {
    const size_t i = (size_t)t * U1 + u;
    if (t == Tb - 1 && u == Ub) return lpb[i];
    float a = -INFINITY, b = -INFINITY;
    if (t + 1 < Tb) a = lpb[i] + prev[u];
    if (u < Ub) b = lpl[i] + prev[u + 1];
    return rnnt_log_add(a, b);
}

// One direction of the walk over the T_b + U_b anti-diagonals of one utterance, run by lanes tid, tid + nthr, ...
// of that direction (dir 0: alpha from the top-left, dir 1: beta from the bottom-right).  lat: the direction's
// [T, U1] output; diag: its two diagonals [2][U1] (LDS on the device); sync(): a barrier of everything that walks
// together, called once per diagonal by every lane (a no-op for a single host thread).  Direction 0 writes *nll.
template <class Sync>
RNNT_HD inline void rnnt_walk(int dir, int tid, int nthr, int Tb, int Ub, int U1, const float *lpb, const float *lpl,
                              float *lat, float *diag, float *nll, Sync sync) {
    const int nd = Tb + Ub;
    for (int step = 0; step < nd; ++step) {
        const int d = dir ? nd - 1 - step : step;
        int ulo, uhi;
        rnnt_diag_range(d, Tb, Ub, &ulo, &uhi);
        const float *prev = diag + (size_t)((step + 1) & 1) * U1;
        float *cur = diag + (size_t)(step & 1) * U1;
        if (lat) {
            for (int u = ulo + tid; u <= uhi; u += nthr) {
                const int t = d - u;
                const float v = dir ? rnnt_beta_cell(t, u, Tb, Ub, U1, lpb, lpl, prev)
                                    : rnnt_alpha_cell(t, u, U1, lpb, lpl, prev);
                cur[u] = v;
                lat[(size_t)t * U1 + u] = v;
                if (!dir && step == nd - 1) *nll = -(v + lpb[(size_t)t * U1 + u]);   // the one cell (T_b - 1, U_b)
            }
        }
        sync();
    }
}

// d nll / d z[t, u, v] = exp((z[v] - lse) + c) - [v == blank] * eb - [v == label] * el
struct RnntCoef {
    float c, eb, el;
};

// alpha, beta, lpb, lpl: the utterance's [T, U1] arrays; nll = -ln P.  beta(T_b, U_b) := 0, every other beta outside
// the lattice is -inf
RNNT_HD inline RnntCoef rnnt_coef(int t, int u, int Tb, int Ub, int U1, const float *alpha, const float *beta,
                                  const float *lpb, const float *lpl, float nll) {
    const size_t i = (size_t)t * U1 + u;
    const float a = alpha[i];
    RnntCoef k;
    k.c = (a + beta[i]) + nll;
    const float bt = t + 1 < Tb ? beta[i + U1] : (u == Ub ? 0.f : -INFINITY);
    k.eb = expf(((a + lpb[i]) + bt) + nll);
    k.el = u < Ub ? expf(((a + lpl[i]) + beta[i + 1]) + nll) : 0.f;
    return k;
}
