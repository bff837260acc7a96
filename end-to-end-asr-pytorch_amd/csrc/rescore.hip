// Second-pass (n-best rescoring) kernels for gfx950: scoring only; the gradient of seq_logp lives in mwer.hip.
//
//   asrk_seq_logp_f32        log-probability of one target per row of [M, V] logits, and per-sequence sums, without
//                            writing a [M, V] log_softmax: one pass over the row (running max and sum per lane),
//                            reads the logits once and writes 4 bytes per row.
//   asrk_seq_logp_lse_f32    the same launch with the row's log-sum-exp as one more output (what the backward needs).
//   asrk_ctc_score_rows_f32  log p_ctc of R hypotheses against the posteriors of U < R utterances: every row walks
//                            the frames of ITS utterance (row_mem), so the [T, V] posteriors are never repeated per
//                            hypothesis; alpha only, no lattice is stored.
#include "common.h"

namespace {

// ---------------------------------------------------------------------------------------------
// seq_logp

constexpr int SEQ_LOGP_WG_MIN_V = 2048;   // rows at least this long get a whole 256-thread workgroup

// running (max, sum of exp(x - max)) of one lane; -inf entries contribute nothing, an all -inf lane stays (-inf, 0)
struct MaxSum {
    float m, s;
};

__device__ __forceinline__ void ms_add(MaxSum &a, float v) {
    if (v > a.m) {
        a.s = a.s * expf(a.m - v) + 1.f;   // a.m == -inf: a.s is 0 and exp(-inf) = 0
        a.m = v;
    } else if (!(v == -INFINITY)) {
        a.s += expf(v - a.m);              // NaN propagates
    }
}

__device__ __forceinline__ void ms_add4(MaxSum &a, const f32x4 v) {
    const float cm = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
    if (cm > a.m) {
        a.s *= expf(a.m - cm);
        a.m = cm;
    }
    if (a.m > -INFINITY) a.s += expf(v[0] - a.m) + expf(v[1] - a.m) + expf(v[2] - a.m) + expf(v[3] - a.m);
}

// all lanes of the wave receive the combined (max, sum)
__device__ __forceinline__ MaxSum ms_wave(MaxSum a) {
    const float M = wave_max(a.m);
    const float s = (a.m == -INFINITY) ? 0.f : a.s * expf(a.m - M);
    return MaxSum{M, wave_sum(s)};
}

template <bool VEC>
__device__ __forceinline__ MaxSum ms_row(const float *__restrict__ xr, int V, int tid, int nthreads) {
    MaxSum a{-INFINITY, 0.f};
    if (VEC) {
        // the row starts on a 16-byte boundary (checked by the launcher); the V % 4 tail is read as scalars
        const int nv = V >> 2;
#pragma unroll 4
        for (int i = tid; i < nv; i += nthreads) ms_add4(a, reinterpret_cast<const f32x4 *>(xr)[i]);
        for (int i = (nv << 2) + tid; i < V; i += nthreads) ms_add(a, xr[i]);
    } else {
#pragma unroll 4
        for (int i = tid; i < V; i += nthreads) ms_add(a, xr[i]);
    }
    return a;
}

// the value of row m once its log-sum-exp is known; target >= V: NaN (nothing is read), as ctc.hip treats bad labels
__device__ __forceinline__ float tok_value(const float *xr, int64_t tg, int V, float lse) {
    if (tg >= V) return __builtin_nanf("");
    return xr[tg] - lse;
}

// one wave per row, 4 rows per workgroup
template <bool VEC>
__global__ __launch_bounds__(256) void seq_logp_wave_kernel(const float *__restrict__ x, int64_t ldx,
                                                            const int64_t *__restrict__ target, int M, int V,
                                                            int normalized, float *__restrict__ tok,
                                                            float *__restrict__ lse_out) {
    const int row = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= M) return;
    const int64_t tg = target[row];
    if (tg < 0) {   // skipped row: never read
        if (lane == 0) {
            tok[row] = 0.f;
            if (lse_out) lse_out[row] = 0.f;
        }
        return;
    }
    const float *xr = x + (size_t)row * ldx;
    if (normalized || tg >= V) {
        if (lane == 0) {
            tok[row] = tok_value(xr, tg, V, 0.f);
            if (lse_out) lse_out[row] = 0.f;
        }
        return;
    }
    const MaxSum r = ms_wave(ms_row<VEC>(xr, V, lane, 64));
    if (lane == 0) {
        const float lse = r.m + logf(r.s);
        tok[row] = tok_value(xr, tg, V, lse);
        if (lse_out) lse_out[row] = lse;
    }
}

// one 256-thread workgroup per row
template <bool VEC>
__global__ __launch_bounds__(256) void seq_logp_wg_kernel(const float *__restrict__ x, int64_t ldx,
                                                          const int64_t *__restrict__ target, int M, int V,
                                                          int normalized, float *__restrict__ tok,
                                                          float *__restrict__ lse_out) {
    __shared__ float sm_m[4], sm_s[4];
    const int row = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t tg = target[row];   // uniform over the workgroup: every thread leaves together
    if (tg < 0) {
        if (threadIdx.x == 0) {
            tok[row] = 0.f;
            if (lse_out) lse_out[row] = 0.f;
        }
        return;
    }
    const float *xr = x + (size_t)row * ldx;
    if (normalized || tg >= V) {
        if (threadIdx.x == 0) {
            tok[row] = tok_value(xr, tg, V, 0.f);
            if (lse_out) lse_out[row] = 0.f;
        }
        return;
    }
    const MaxSum w = ms_wave(ms_row<VEC>(xr, V, threadIdx.x, 256));
    if (lane == 0) {
        sm_m[wave] = w.m;
        sm_s[wave] = w.s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const float Mx = fmaxf(fmaxf(sm_m[0], sm_m[1]), fmaxf(sm_m[2], sm_m[3]));
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (sm_m[k] > -INFINITY || sm_m[k] != sm_m[k]) s += sm_s[k] * expf(sm_m[k] - Mx);
        const float lse = Mx + logf(s);
        tok[row] = tok_value(xr, tg, V, lse);
        if (lse_out) lse_out[row] = lse;
    }
}

// seq[r] = sum over m in [seg_off[r], seg_off[r+1]) of (double)tok[m], added one after the other in ascending m: a
// fixed order, so the result is reproducible bit for bit (segments are a few tens of tokens; one thread each)
__global__ __launch_bounds__(64) void seq_logp_sum_kernel(const float *__restrict__ tok,
                                                          const int64_t *__restrict__ seg_off, int M, int R,
                                                          double *__restrict__ seq) {
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= R) return;
    int64_t a = seg_off[r], b = seg_off[r + 1];
    a = a < 0 ? 0 : a;               // offsets outside [0, M] never read out of bounds
    b = b > M ? (int64_t)M : b;
    double acc = 0.0;
    for (int64_t m = a; m < b; ++m) acc += (double)tok[m];
    seq[r] = acc;
}

// ---------------------------------------------------------------------------------------------
// ctc_score_rows: the alpha walk of ctc.hip's ctc_lattice_kernel (same state layout s = lane*spl + j, same lse3, same
// switch to the library expf/logf for long lattices, the next CTC_PF gathered rows in registers), without the lattice
// stores and without a beta direction.

constexpr int CTC_THREADS = 64;
constexpr int CTC_MAX_SPL = 32;   // states per lane -> S <= 2048 (L <= 1023)
constexpr int CTC_PF = 8;
constexpr int GATHER_ROWS = 8;

template <bool FAST>
__device__ __forceinline__ float lse3(float a, float b, float c) {
    const float m = fmaxf(a, fmaxf(b, c));
    if (m == -INFINITY) return -INFINITY;
    if (!FAST) return m + logf(expf(a - m) + expf(b - m) + expf(c - m));
    return m + __logf(__expf(a - m) + __expf(b - m) + __expf(c - m));
}

struct ScoreArgs {
    const float *lp;         // frame t of utterance u at lp + u*su + t*st
    int64_t su, st;
    int U, Tmax, V;
    const int64_t *mem_len;  // [U]
    const int64_t *row_mem;  // [R]
    const int64_t *targets;  // [R, tgt_stride]
    int64_t tgt_stride;
    int Lmax;
    const int64_t *tgt_len;  // [R]
    int R, blank;
    float *score;            // [R]
    float *lpg;              // [R, Tmax, Smax] gathered log-probs lp[row_mem[r], t, ext_r[s]]
};

__device__ __forceinline__ int ext_label(const int64_t *tgt, int s, int blank) {
    return (s & 1) ? (int)tgt[s >> 1] : blank;
}

// frames and target length of row r; false for a row_mem outside [0, U) (nothing of that row is read)
__device__ __forceinline__ bool row_shape(const ScoreArgs &p, int r, int &u, int &Tr, int &tl) {
    const int64_t um = p.row_mem[r];
    if (um < 0 || um >= p.U) return false;
    u = (int)um;
    const int64_t ml = p.mem_len[u], tg = p.tgt_len[r];
    Tr = (int)(ml < 0 ? 0 : (ml > p.Tmax ? p.Tmax : ml));
    tl = (int)(tg < 0 ? 0 : (tg > p.Lmax ? p.Lmax : tg));
    return true;
}

__global__ __launch_bounds__(256) void score_gather_kernel(ScoreArgs p) {
    const int r = blockIdx.x;
    int u, Tr, tl;
    if (!row_shape(p, r, u, Tr, tl)) return;
    const int Smax = 2 * p.Lmax + 1, S = 2 * tl + 1;
    const int t0 = blockIdx.y * GATHER_ROWS;
    if (t0 >= Tr) return;
    const int64_t *tgt = p.targets + (int64_t)r * p.tgt_stride;
    const float *lpu = p.lp + (int64_t)u * p.su;
    float *out = p.lpg + (size_t)r * p.Tmax * Smax;
    for (int idx = threadIdx.x; idx < GATHER_ROWS * Smax; idx += 256) {
        const int k = idx / Smax, s = idx - k * Smax;
        const int t = t0 + k;
        if (t < Tr && s < S)   // frames >= mem_len[u] are never read; a bad label is clamped here and reported below
            out[(size_t)t * Smax + s] = lpu[(int64_t)t * p.st + min(max(ext_label(tgt, s, p.blank), 0), p.V - 1)];
    }
}

template <int SPL, bool FAST>
__global__ __launch_bounds__(CTC_THREADS) void score_alpha_kernel(ScoreArgs p) {
    extern __shared__ float srow[];   // [2][Smax]
    const int r = blockIdx.x, lane = threadIdx.x;
    const int Smax = 2 * p.Lmax + 1;
    const int spl = (Smax + CTC_THREADS - 1) / CTC_THREADS;   // <= SPL
    int u, Tr, tl;
    if (!row_shape(p, r, u, Tr, tl)) {
        if (lane == 0) p.score[r] = __builtin_nanf("");
        return;
    }
    const int S = 2 * tl + 1;
    const int64_t *tgt = p.targets + (int64_t)r * p.tgt_stride;
    const float *g = p.lpg + (size_t)r * p.Tmax * Smax;
    {
        bool bad = false;
        for (int i = lane; i < tl; i += CTC_THREADS) bad |= tgt[i] < 0 || tgt[i] >= p.V;
        if (__any(bad)) {
            if (lane == 0) p.score[r] = __builtin_nanf("");
            return;
        }
    }
    if (Tr <= 0) {   // no frames: the empty hypothesis has the empty product, every other one no path
        if (lane == 0) p.score[r] = (tl == 0) ? 0.f : -INFINITY;
        return;
    }

    bool skip_ok[SPL];   // may take the s-2 transition
#pragma unroll
    for (int j = 0; j < SPL; ++j) {
        skip_ok[j] = false;
        const int s = lane * spl + j;
        if (j < spl && s < S && (s & 1) && s >= 2)
            skip_ok[j] = ext_label(tgt, s, p.blank) != ext_label(tgt, s - 2, p.blank);
    }

    float cur[SPL], pre[CTC_PF][SPL];
#pragma unroll
    for (int j = 0; j < SPL; ++j) {
        cur[j] = -INFINITY;
        const int s = lane * spl + j;
        if (j < spl && s < S && s <= 1) cur[j] = g[s];
    }
#pragma unroll
    for (int d = 0; d < CTC_PF; ++d)
#pragma unroll
        for (int j = 0; j < SPL; ++j) {
            pre[d][j] = 0.f;
            const int s = lane * spl + j;
            if (j < spl && s < S && 1 + d < Tr) pre[d][j] = g[(size_t)(1 + d) * Smax + s];
        }

    for (int base = 0; base < Tr; base += CTC_PF) {
#pragma unroll
        for (int d = 0; d < CTC_PF; ++d) {
            const int step = base + d;
            if (step >= Tr) break;
            float *row = srow + (step & 1) * Smax;
#pragma unroll
            for (int j = 0; j < SPL; ++j) {
                const int s = lane * spl + j;
                if (j < spl && s < Smax) row[s] = cur[j];
            }
            if (step + 1 == Tr) break;
            float lpn[SPL];
            const int sp = step + 1 + CTC_PF;
#pragma unroll
            for (int j = 0; j < SPL; ++j) {
                lpn[j] = pre[d][j];
                const int s = lane * spl + j;
                if (j < spl && s < S && sp < Tr) pre[d][j] = g[(size_t)sp * Smax + s];
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < SPL; ++j) {
                const int s = lane * spl + j;
                if (j < spl) {
                    if (s < S) {
                        const float a0 = row[s];
                        float a1 = -INFINITY, a2 = -INFINITY;
                        if (s >= 1) a1 = row[s - 1];
                        if (skip_ok[j]) a2 = row[s - 2];
                        cur[j] = lse3<FAST>(a0, a1, a2) + lpn[j];
                    } else {
                        cur[j] = -INFINITY;
                    }
                }
            }
        }
    }
    __syncthreads();
    if (lane == 0) {
        const float *row = srow + ((Tr - 1) & 1) * Smax;
        const float l1 = row[S - 1];
        const float l2 = S >= 2 ? row[S - 2] : -INFINITY;
        p.score[r] = log_add(l1, l2);
    }
}

static inline size_t score_ws_bytes(int R, int Tmax, int Lmax) {
    return ((size_t)R * Tmax * (2 * (size_t)Lmax + 1) * sizeof(float) + 15) & ~(size_t)15;
}

static inline bool al16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

// asrk_seq_logp_f32 and asrk_seq_logp_lse_f32 (lse != nullptr): the same kernels, the same arithmetic
static int seq_logp_launch(const float *x, int64_t ldx, const int64_t *target, const int64_t *seg_off, int M, int V,
                           int R, int flags, float *tok_logp, float *lse, double *seq_logp, void *stream) {
    if (M < 0 || V <= 0 || R < 0 || ldx < V) return ASRK_EINVAL;
    if (flags & ~ASRK_SEQ_LOGP_NORMALIZED) return ASRK_EINVAL;
    if ((seg_off == nullptr) != (seq_logp == nullptr)) return ASRK_EINVAL;
    if (M > 0 && (!x || !target || !tok_logp)) return ASRK_EINVAL;
    const bool sums = seg_off != nullptr && R > 0;
    if (M == 0 && !sums) return ASRK_OK;
    hipStream_t s = (hipStream_t)stream;
    const int normalized = (flags & ASRK_SEQ_LOGP_NORMALIZED) ? 1 : 0;
    asrk_prof_begin_(PROF_ROWOPS, s);
    if (M > 0) {
        const bool vec = al16(x) && (ldx % 4 == 0);
        if (V >= SEQ_LOGP_WG_MIN_V) {
            if (vec)
                hipLaunchKernelGGL((seq_logp_wg_kernel<true>), dim3(M), dim3(256), 0, s, x, ldx, target, M, V,
                                   normalized, tok_logp, lse);
            else
                hipLaunchKernelGGL((seq_logp_wg_kernel<false>), dim3(M), dim3(256), 0, s, x, ldx, target, M, V,
                                   normalized, tok_logp, lse);
        } else {
            const unsigned grid = (unsigned)asrk_div_up(M, 4);
            if (vec)
                hipLaunchKernelGGL((seq_logp_wave_kernel<true>), dim3(grid), dim3(256), 0, s, x, ldx, target, M, V,
                                   normalized, tok_logp, lse);
            else
                hipLaunchKernelGGL((seq_logp_wave_kernel<false>), dim3(grid), dim3(256), 0, s, x, ldx, target, M, V,
                                   normalized, tok_logp, lse);
        }
    }
    if (sums)
        hipLaunchKernelGGL(seq_logp_sum_kernel, dim3(asrk_div_up(R, 64)), dim3(64), 0, s, tok_logp, seg_off, M, R,
                           seq_logp);
    asrk_prof_end_(PROF_ROWOPS, s);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}

extern "C" int asrk_seq_logp_f32(const float *x, int64_t ldx, const int64_t *target, const int64_t *seg_off, int M,
                                 int V, int R, int flags, float *tok_logp, double *seq_logp, void *stream) {
    return seq_logp_launch(x, ldx, target, seg_off, M, V, R, flags, tok_logp, nullptr, seq_logp, stream);
}

extern "C" int asrk_seq_logp_lse_f32(const float *x, int64_t ldx, const int64_t *target, const int64_t *seg_off, int M,
                                     int V, int R, int flags, float *tok_logp, float *lse, double *seq_logp,
                                     void *stream) {
    if (M > 0 && !lse) return ASRK_EINVAL;
    return seq_logp_launch(x, ldx, target, seg_off, M, V, R, flags, tok_logp, lse, seq_logp, stream);
}

extern "C" size_t asrk_ctc_score_rows_ws_bytes(int R, int Tmax, int Lmax) {
    if (R <= 0 || Tmax <= 0 || Lmax < 0 || Lmax > (CTC_THREADS * CTC_MAX_SPL - 1) / 2) return 0;
    return score_ws_bytes(R, Tmax, Lmax);
}

extern "C" int asrk_ctc_score_rows_f32(const float *lp, int64_t stride_u, int64_t stride_t, int U, int Tmax, int V,
                                       const int64_t *mem_len, const int64_t *row_mem, const int64_t *targets,
                                       int64_t tgt_stride, int Lmax, const int64_t *tgt_len, int R, int blank,
                                       float *score, void *ws, size_t ws_bytes, void *stream) {
    if (U < 0 || Tmax < 0 || V <= 0 || Lmax < 0 || R < 0 || blank < 0 || blank >= V) return ASRK_EINVAL;
    if (stride_u < 0 || stride_t < 0 || tgt_stride < 0 || tgt_stride < Lmax) return ASRK_EINVAL;
    if (R == 0) return ASRK_OK;
    if (!mem_len || !row_mem || !tgt_len || !score) return ASRK_EINVAL;
    if (U > 0 && Tmax > 0 && !lp) return ASRK_EINVAL;
    if (Lmax > 0 && !targets) return ASRK_EINVAL;
    const int Smax = 2 * Lmax + 1;
    if (Smax > CTC_THREADS * CTC_MAX_SPL) return ASRK_ESHAPE;
    const size_t need = Tmax > 0 ? score_ws_bytes(R, Tmax, Lmax) : 0;
    if (need > 0 && (!ws || !al16(ws) || ws_bytes < need)) return ASRK_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    ScoreArgs a{lp, stride_u, stride_t, U, Tmax, V, mem_len, row_mem, targets, tgt_stride, Lmax, tgt_len, R, blank,
                score, reinterpret_cast<float *>(ws)};
    asrk_prof_begin_(PROF_CTC, s);
    if (Tmax > 0)
        hipLaunchKernelGGL(score_gather_kernel, dim3(R, asrk_div_up(Tmax, GATHER_ROWS)), dim3(256), 0, s, a);
    const size_t lds = 2 * (size_t)Smax * sizeof(float);
    if (Smax <= CTC_THREADS * 4 && Tmax <= 512)
        hipLaunchKernelGGL((score_alpha_kernel<4, true>), dim3(R), dim3(CTC_THREADS), lds, s, a);
    else if (Smax <= CTC_THREADS * 4)
        hipLaunchKernelGGL((score_alpha_kernel<4, false>), dim3(R), dim3(CTC_THREADS), lds, s, a);
    else if (Smax <= CTC_THREADS * 16)
        hipLaunchKernelGGL((score_alpha_kernel<16, false>), dim3(R), dim3(CTC_THREADS), lds, s, a);
    else
        hipLaunchKernelGGL((score_alpha_kernel<CTC_MAX_SPL, false>), dim3(R), dim3(CTC_THREADS), lds, s, a);
    asrk_prof_end_(PROF_CTC, s);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}
