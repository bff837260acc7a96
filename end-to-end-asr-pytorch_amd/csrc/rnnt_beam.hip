// Transducer beam search for gfx950 (src/transducer.py: TransducerHead.beam_search), alignment-length synchronous, a
// batch of utterances in lock-step with W slots each.  Per iteration:
//
//   asrk_rnnt_joint_slots_f32   H[r,:] = tanh(E[r / W, t_ptr[r], :] + P[r,:]): E is not repeated per slot.
//   asrk_rnnt_beam_rows_f32     ONE read of the [B*W, V] logits (and of the LM rows): per live row the log-sum-exp, the
//                               blank's log-probability and the K best labels by lp[k] + lm_weight * lm[k]; K + 2 numbers
//                               out, no [rows, V] log-softmax.  The row lives in the registers of its wave (V < 2048) or
//                               of its 256-thread workgroup while K rounds of an arg-max take the winners.
//   asrk_rnnt_beam_select       one workgroup per utterance: candidates, merge of equal sequences, cut to W, finished
//                               list, next beam and the gather indices of the caller (rnnt_beam.inc).
//
// wave64, no float atomics: every result is a pure function of its inputs, reproducible bit for bit.
#include "common.h"

#define RB_HD __device__
#define RB_HHD __host__ __device__
#define RB_FOR(i, n) for (int i = (int)threadIdx.x; i < (n); i += (int)blockDim.x)
#define RB_SYNC() __syncthreads()
#include "rnnt_beam.inc"

namespace {

constexpr int RB_WG_MIN_V = 2048;       // the case split of asrk_rnnt_rows_f32
constexpr int RB_GROUPS_WAVE = 8;       // 16-byte groups per lane: 64 * 8 * 4 = 2048 values
constexpr int RB_GROUPS_WG = 16;        // 256 * 16 * 4 = 16384 values
constexpr int RB_MAX_V = 256 * RB_GROUPS_WG * 4;
constexpr int RB_NONE = 0x7fffffff;
constexpr int RB_SELECT_THREADS = 256;

static inline bool al16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

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

__device__ __forceinline__ MaxSum ms_wave(MaxSum a) {
    const float M = wave_max(a.m);
    const float s = (a.m == -INFINITY) ? 0.f : a.s * expf(a.m - M);
    return MaxSum{M, wave_sum(s)};
}

// every lane ends with the best (value, index): the larger value, the smaller index on equal values.  The four steps
// inside a 16-lane row are DPP moves, the two across rows shuffles (as pb_wave_best of prefix_beam.hip).
template <int CTRL>
__device__ __forceinline__ void dpp_best_step(float &bv, int &bi) {
    const float ov = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, bv), CTRL, 0xf, 0xf, true));
    const int oi = __builtin_amdgcn_mov_dpp(bi, CTRL, 0xf, 0xf, true);
    if (oi != RB_NONE && (bi == RB_NONE || ov > bv || (ov == bv && oi < bi))) {
        bv = ov;
        bi = oi;
    }
}
__device__ __forceinline__ void wave_best(float &bv, int &bi) {
    dpp_best_step<0xB1>(bv, bi);        // quad_perm [1,0,3,2]
    dpp_best_step<0x4E>(bv, bi);        // quad_perm [2,3,0,1]
    dpp_best_step<0x141>(bv, bi);       // row_half_mirror
    dpp_best_step<0x140>(bv, bi);       // row_mirror
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (oi != RB_NONE && (bi == RB_NONE || ov > bv || (ov == bv && oi < bi))) {
            bv = ov;
            bi = oi;
        }
    }
}

struct RowsArgs {
    const float *z, *lm;
    int64_t ldz, ldlm;
    float lw;
    const int32_t *n_live;
    int M, W, V, K, blank;
    float *lse, *lpb, *val;
    int32_t *lab;
};

// WG = false: one wave per row, 4 rows per workgroup; WG = true: one 256-thread workgroup per row.
// Thread `tid` holds the 16-byte groups tid, tid + NT, ...: value (group * 4 + c) in component c.
template <bool VEC, bool WG>
__global__ __launch_bounds__(256) void rb_rows_kernel(RowsArgs p) {
    constexpr int NT = WG ? 256 : 64, G = WG ? RB_GROUPS_WG : RB_GROUPS_WAVE;
    __shared__ float sm_m[4], sm_s[4], sm_lse;
    __shared__ float st_v[4 * RB_MAX_BEAM];
    __shared__ int st_i[4 * RB_MAX_BEAM];
    const int row = WG ? (int)blockIdx.x : (int)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tid = WG ? (int)threadIdx.x : (int)(threadIdx.x & 63);
    const int lane = threadIdx.x & 63;
    if (row >= p.M) return;
    const int K = p.K, V = p.V;
    float *val = p.val + (size_t)row * K;
    int32_t *lab = p.lab + (size_t)row * K;
    if (p.n_live && (row % p.W) >= p.n_live[row / p.W]) {   // uniform over the row's threads; the row is never read
        if (tid == 0) {
            p.lse[row] = 0.f;
            p.lpb[row] = 0.f;
        }
        for (int c = tid; c < K; c += NT) {
            val[c] = -INFINITY;
            lab[c] = -1;
        }
        return;
    }
    const float *zr = p.z + (size_t)row * p.ldz;
    const float *lr = p.lm ? p.lm + (size_t)row * p.ldlm : nullptr;
    const float lw = p.lw;
    f32x4 a[G];                         // the ranking values; NaN: no candidate (blank, beyond V, -inf)
    const int ng = min(G, (V + NT * 4 - 1) / (NT * 4));   // groups any thread holds a value of: the rest is skipped (uniform)
    MaxSum acc{-INFINITY, 0.f};
#pragma unroll
    for (int q = 0; q < G; ++q) {
        if (q >= ng) continue;
        const int i0 = (tid + NT * q) << 2;
        f32x4 x = {0.f, 0.f, 0.f, 0.f}, l = {0.f, 0.f, 0.f, 0.f};
        if (VEC && i0 + 4 <= V) {
            x = *reinterpret_cast<const f32x4 *>(zr + i0);
            if (lr) l = *reinterpret_cast<const f32x4 *>(lr + i0);
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (i0 + c < V) {
                    x[c] = zr[i0 + c];
                    if (lr) l[c] = lr[i0 + c];
                }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int i = i0 + c;
            float r = __builtin_nanf("");
            if (i < V) {
                ms_add(acc, x[c]);
                const float f = lr ? x[c] + lw * l[c] : x[c];
                if (i != p.blank && f > -INFINITY) r = f;
            }
            a[q][c] = r;
        }
    }
    MaxSum red = ms_wave(acc);
    if (WG) {
        const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        if (lane == 0) {
            sm_m[wave] = red.m;
            sm_s[wave] = red.s;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const float Mx = fmaxf(fmaxf(sm_m[0], sm_m[1]), fmaxf(sm_m[2], sm_m[3]));
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (sm_m[k] > -INFINITY || sm_m[k] != sm_m[k]) s += sm_s[k] * expf(sm_m[k] - Mx);
            sm_lse = Mx + logf(s);
        }
        __syncthreads();
    }
    const float lse = WG ? sm_lse : red.m + logf(red.s);
    if (tid == 0) {
        p.lse[row] = lse;
        p.lpb[row] = zr[p.blank] - lse;
    }
    // K rounds: round c takes the best value that sorts strictly after round c - 1's winner (no "taken" flags)
    const int wave = WG ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) : 0;
    float pv = INFINITY;
    int pi = -1;
    for (int c = 0; c < K; ++c) {
        float bv = -INFINITY;
        int bi = RB_NONE;
#pragma unroll
        for (int q = 0; q < G; ++q) {
            if (q >= ng) continue;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = ((tid + NT * q) << 2) + e;
                const float v = a[q][e];
                const bool eligible = v < pv || (v == pv && i > pi);     // NaN: never
                if (eligible && (bi == RB_NONE || v > bv)) {             // ascending i: the first maximum stays
                    bv = v;
                    bi = i;
                }
            }
        }
        wave_best(bv, bi);
        pv = bv;
        pi = bi;
        if (WG) {
            if (lane == 0) {
                st_v[wave * K + c] = bv;
                st_i[wave * K + c] = bi;
            }
            if (bi == RB_NONE) {                                         // this wave's share is exhausted
                for (int c2 = c + 1 + lane; c2 < K; c2 += 64) {
                    st_v[wave * K + c2] = -INFINITY;
                    st_i[wave * K + c2] = RB_NONE;
                }
                break;
            }
        } else {
            if (lane == 0) {
                const bool ok = bi != RB_NONE;
                lab[c] = ok ? bi : -1;
                val[c] = ok ? (lr ? (zr[bi] - lse) + lw * lr[bi] : zr[bi] - lse) : -INFINITY;
            }
            if (bi == RB_NONE) {
                for (int c2 = c + 1 + lane; c2 < K; c2 += 64) {
                    val[c2] = -INFINITY;
                    lab[c2] = -1;
                }
                break;
            }
        }
    }
    if (WG) {
        __syncthreads();
        if (wave == 0) {                // the K best of the 4 x K survivors, the same order
            const int n = 4 * K;        // <= 128: two per lane
            pv = INFINITY;
            pi = -1;
            for (int c = 0; c < K; ++c) {
                float bv = -INFINITY;
                int bi = RB_NONE;
                for (int q = lane; q < n; q += 64) {
                    const float v = st_v[q];
                    const int i = st_i[q];
                    const bool eligible = i != RB_NONE && (v < pv || (v == pv && i > pi));
                    if (eligible && (bi == RB_NONE || v > bv || (v == bv && i < bi))) {
                        bv = v;
                        bi = i;
                    }
                }
                wave_best(bv, bi);
                pv = bv;
                pi = bi;
                if (lane == 0) {
                    const bool ok = bi != RB_NONE;
                    lab[c] = ok ? bi : -1;
                    val[c] = ok ? (lr ? (zr[bi] - lse) + lw * lr[bi] : zr[bi] - lse) : -INFINITY;
                }
            }
        }
    }
}

__global__ __launch_bounds__(RB_SELECT_THREADS) void rb_select_kernel(RBArgs a) {
    __shared__ double e_sc[RB_MAX_ENTRIES];
    __shared__ double f_sc[2 * RB_MAX_BEAM];
    __shared__ int32_t e_src[RB_MAX_ENTRIES];
    __shared__ int32_t order[RB_MAX_BEAM], r_fin[RB_MAX_BEAM];
    __shared__ unsigned char e_alive[RB_MAX_ENTRIES];
    RBState s;
    rb_bind(a, (int)blockIdx.x, s);
    s.e_sc = e_sc;
    s.f_sc = f_sc;
    s.e_src = e_src;
    s.order = order;
    s.r_fin = r_fin;
    s.e_alive = e_alive;
    rb_select(s);
}

// one thread per output element (VEC: per 16-byte group) of H [B*W, J]
template <bool VEC>
__global__ __launch_bounds__(256) void rb_joint_kernel(const float *__restrict__ E, int64_t lde,
                                                       const float *__restrict__ P, int64_t ldp,
                                                       const int32_t *__restrict__ t_ptr, int T, int W, int J,
                                                       float *__restrict__ H, int64_t ldh, int64_t total) {
    const int per_row = VEC ? (J >> 2) : J;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / per_row;
        const int j = (int)(i - r * per_row);
        const int64_t b = r / W;
        int t = t_ptr[r];
        t = t < 0 ? 0 : (t > T - 1 ? T - 1 : t);   // a dead or finished row points anywhere
        const float *e = E + (b * T + t) * lde;
        const float *q = P + r * ldp;
        float *h = H + r * ldh;
        if (VEC) {
            const f32x4 x = reinterpret_cast<const f32x4 *>(e)[j], y = reinterpret_cast<const f32x4 *>(q)[j];
            f32x4 o;
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = tanhf(x[k] + y[k]);
            reinterpret_cast<f32x4 *>(h)[j] = o;
        } else {
            h[j] = tanhf(e[j] + q[j]);
        }
    }
}

static inline unsigned grid_for64(int64_t n, int block) {
    const int64_t g = (n + block - 1) / block;
    return (unsigned)(g > 65536 ? 65536 : (g < 1 ? 1 : g));
}

}  // namespace

extern "C" int asrk_rnnt_joint_slots_f32(const float *E, int64_t lde, const float *P, int64_t ldp, const int32_t *t_ptr,
                                         int B, int T, int W, int J, float *H, int64_t ldh, void *stream) {
    if (B < 0 || T <= 0 || W <= 0 || J <= 0 || lde < J || ldp < J || ldh < J) return ASRK_EINVAL;
    if ((int64_t)B * W > (int64_t)INT32_MAX) return ASRK_ESHAPE;
    if (B == 0) return ASRK_OK;
    if (!E || !P || !H || !t_ptr) return ASRK_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const bool vec = al16(E) && al16(P) && al16(H) && J % 4 == 0 && lde % 4 == 0 && ldp % 4 == 0 && ldh % 4 == 0;
    const int64_t total = (int64_t)B * W * (vec ? J / 4 : J);
    asrk_prof_begin_(PROF_ROWOPS, s);
    if (vec)
        hipLaunchKernelGGL((rb_joint_kernel<true>), dim3(grid_for64(total, 256)), dim3(256), 0, s, E, lde, P, ldp, t_ptr,
                           T, W, J, H, ldh, total);
    else
        hipLaunchKernelGGL((rb_joint_kernel<false>), dim3(grid_for64(total, 256)), dim3(256), 0, s, E, lde, P, ldp,
                           t_ptr, T, W, J, H, ldh, total);
    asrk_prof_end_(PROF_ROWOPS, s);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}

extern "C" int asrk_rnnt_beam_rows_f32(const float *z, int64_t ldz, const float *lm, int64_t ldlm, float lm_weight,
                                       const int32_t *n_live, int B, int W, int V, int K, int blank, float *lse,
                                       float *lpb, float *val, int32_t *lab, void *stream) {
    if (B < 0 || W < 1 || W > RB_MAX_BEAM || V < 2 || K < 1 || K > RB_MAX_BEAM || K > V - 1 || ldz < V || blank < 0 ||
        blank >= V || (lm && ldlm < V))
        return ASRK_EINVAL;
    if (V > RB_MAX_V || (int64_t)B * W > (int64_t)INT32_MAX) return ASRK_ESHAPE;
    if (B == 0) return ASRK_OK;
    if (!z || !lse || !lpb || !val || !lab) return ASRK_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int M = B * W;
    const RowsArgs p{z, lm, ldz, ldlm, lm_weight, n_live, M, W, V, K, blank, lse, lpb, val, lab};
    const bool vec = al16(z) && ldz % 4 == 0 && (!lm || (al16(lm) && ldlm % 4 == 0));
    asrk_prof_begin_(PROF_ROWOPS, s);
    if (V >= RB_WG_MIN_V) {
        if (vec)
            hipLaunchKernelGGL((rb_rows_kernel<true, true>), dim3(M), dim3(256), 0, s, p);
        else
            hipLaunchKernelGGL((rb_rows_kernel<false, true>), dim3(M), dim3(256), 0, s, p);
    } else {
        const unsigned grid = (unsigned)asrk_div_up(M, 4);
        if (vec)
            hipLaunchKernelGGL((rb_rows_kernel<true, false>), dim3(grid), dim3(256), 0, s, p);
        else
            hipLaunchKernelGGL((rb_rows_kernel<false, false>), dim3(grid), dim3(256), 0, s, p);
    }
    asrk_prof_end_(PROF_ROWOPS, s);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}

extern "C" int asrk_rnnt_beam_select(const float *lpb, const float *val, const int32_t *lab, const int64_t *enc_len,
                                     int B, int T, int W, int K, int max_symbols, int max_len, int64_t tok_stride,
                                     int cur, int32_t *n_live, int32_t *t_ptr, int32_t *n_sym, int32_t *n_tok,
                                     double *score, int32_t *tokens, int32_t *fin_n, int32_t *fin_len, double *fin_score,
                                     int32_t *fin_tok, int64_t *parent, int64_t *last_tok, int32_t *emit, int64_t *sel,
                                     int64_t *lm_sel, void *stream) {
    const RBArgs a{lpb,     val,    lab,     enc_len,   B,      T,      W,     K,       max_symbols,
                   max_len, cur,    tok_stride, n_live, t_ptr,  n_sym,  n_tok, tokens,  score,
                   fin_n,   fin_len, fin_tok, fin_score, parent, last_tok, sel,  lm_sel,  emit};
    if (rb_args_bad(a)) return ASRK_EINVAL;
    if ((int64_t)B * W > (int64_t)INT32_MAX) return ASRK_ESHAPE;
    if (B == 0) return ASRK_OK;
    if (!lpb || !val || !lab || !enc_len || !n_live || !t_ptr || !n_sym || !n_tok || !score || !tokens || !fin_n ||
        !fin_len || !fin_score || !fin_tok || !parent || !last_tok || !emit || !sel || !lm_sel)
        return ASRK_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    asrk_prof_begin_(PROF_ROWOPS, s);
    hipLaunchKernelGGL(rb_select_kernel, dim3(B), dim3(RB_SELECT_THREADS), 0, s, a);
    asrk_prof_end_(PROF_ROWOPS, s);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}
