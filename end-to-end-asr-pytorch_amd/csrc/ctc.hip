// CTC loss forward (alpha) and backward (beta + gradient) for gfx950.
//
// Replaces torch.nn.CTCLoss(blank=0, zero_infinity=False) as called at
// bin/train_asr.py:49,123-124 (ATen ctc_loss / ctc_loss_backward): log-space alpha/beta over the
// blank-extended label sequence (S = 2L+1), nll_b = -logsumexp(alpha[T_b-1][S-1], alpha[..][S-2]),
// grad = (exp(lp) - exp(logsum_{s:ext[s]=c}(alpha+beta) + nll - lp)) * scale.
//
// Only 2L+1 of the V log-probs per frame are ever read by the lattices (3.3 MB of the 128 MB tensor
// at cfg3): a gather pre-pass compacts them to [B,T,S]; then alpha and beta run CONCURRENTLY in one
// launch (one wave per utterance and direction, previous lattice row in LDS, the next 8 frames'
// gathered rows already in registers, so no memory latency sits on the T-step dependent chain).
// The dense gradient write is a separate streaming pass (HBM-bound: read lp + write grad once),
// followed by a sparse overwrite of the <= L+1 label columns per frame.
#include "common.h"

namespace {

constexpr int CTC_THREADS = 64;
constexpr int CTC_MAX_SPL = 32;  // states per lane -> S <= 2048 (L <= 1023)
constexpr int GATHER_ROWS = 8;   // frames per ctc_gather_kernel workgroup

// What the loss launches do for a shape: the one place the dispatch arithmetic lives (both launchers and
// asrk_ctc_loss_plan_info read it).
struct CtcPlan {
    int spl_tmpl;     // ctc_lattice_kernel's states-per-lane template: 4, 16 or CTC_MAX_SPL
    int fast;         // its FAST flag (hardware exp / log): short lattices only
    int spl;          // states per lane in use, ceil(Smax / 64) <= spl_tmpl
    int gather_y;     // ctc_gather_kernel grid y (0: no launch)
    int t_per_block;  // ctc_grad_fix_kernel: frames per workgroup (a multiple of 4) and
    int tchunks;      //   its grid y; both 0 where the backward launches nothing
    int dense_grid;   // ctc_grad_dense_kernel grid x (4 rows of [T*B] per workgroup)
};

inline CtcPlan ctc_plan(int T, int B, int Lmax) {
    CtcPlan pl{};
    const int Smax = 2 * Lmax + 1;
    pl.spl_tmpl = Smax <= CTC_THREADS * 4 ? 4 : Smax <= CTC_THREADS * 16 ? 16 : CTC_MAX_SPL;
    // T > 512 or more than 256 states: library expf / logf (see lse3)
    pl.fast = (Smax <= CTC_THREADS * 4 && T <= 512) ? 1 : 0;
    pl.spl = asrk_div_up(Smax, CTC_THREADS);
    if (B <= 0) return pl;
    pl.gather_y = asrk_div_up(T, GATHER_ROWS);
    if (T <= 0) return pl;
    int tchunks = asrk_div_up(512, B);
    if (tchunks > asrk_div_up(T, 4)) tchunks = asrk_div_up(T, 4);
    if (tchunks < 1) tchunks = 1;
    pl.t_per_block = asrk_div_up(asrk_div_up(T, tchunks), 4) * 4;
    pl.tchunks = asrk_div_up(T, pl.t_per_block);
    pl.dense_grid = asrk_div_up(T * B, 4);
    return pl;
}

template <bool FAST>
__device__ __forceinline__ float lse3(float a, float b, float c) {
    const float m = fmaxf(a, fmaxf(b, c));
    if (m == -INFINITY) return -INFINITY;
    // long lattices (T > 512 or more than 256 states) use the library functions: the ~1e-7 per-step
    // error of the hardware approximations accumulates to ~1e-3 in alpha + beta after ~1000 frames
    if (!FAST) return m + logf(expf(a - m) + expf(b - m) + expf(c - m));
    // hardware exp2/log2 (v_exp_f32 / v_log_f32, ~1 ulp): the library expf/logf are ~15 instructions
    // each and this is the dependent chain of the lattice (one wave per lattice: the step was
    // ALU-bound at ~2k cycles).  The largest term is exp(0) = 1 exactly, the others only matter
    // when they are close to it, so the absolute error per step stays ~1e-7.
    return m + __logf(__expf(a - m) + __expf(b - m) + __expf(c - m));
}

struct CtcArgs {
    const float *lp;
    int64_t st, sb;
    int T, B, V;
    const int64_t *targets;
    int64_t tgt_stride;
    int Lmax;
    const int64_t *in_len, *tg_len;
    int blank;
    float *alpha;  // [B, T, S]
    float *beta;   // [B, T, S]  (nullptr: alpha only)
    float *lpg;    // [B, T, S]  gathered log-probs lp[t, b, ext_b[s]]
    float *nll;    // [B]
    // zero_infinity (asrk_ctc_loss_fwd_ex_f32): loss[b] = nll[b], or 0 where nll[b] == +inf and zero_inf is set; those
    // utterances are counted in n_inf.  All three stay 0 / NULL for the plain entry point and the aligner.
    float *loss;   // [B] or nullptr
    int *n_inf;    // device counter or nullptr
    int zero_inf;
};

// nll[b] keeps +inf as the marker the backward tests; a NaN (targets outside [0,V)) is never zeroed
__device__ __forceinline__ void ctc_store_nll(const CtcArgs &p, int b, float v) {
    p.nll[b] = v;
    if (p.loss) {
        const bool zeroed = p.zero_inf && v == INFINITY;
        p.loss[b] = zeroed ? 0.f : v;
        if (zeroed && p.n_inf) atomicAdd(p.n_inf, 1);
    }
}

// ext[s]: blank for even s, target[(s-1)/2] for odd s
__device__ __forceinline__ int ext_label(const int64_t *tgt, int s, int blank) {
    return (s & 1) ? (int)tgt[s >> 1] : blank;
}

// K0: lpg[b][t][s] = lp[t, b, ext_b[s]] for t < T_b, s < S_b.  Fully parallel scattered gather; every
// later CTC kernel reads these compact rows (coalesced, L2-resident) instead of the [T,B,V] tensor.
__global__ __launch_bounds__(256) void ctc_gather_kernel(CtcArgs p) {
    const int b = blockIdx.x;
    const int Smax = 2 * p.Lmax + 1;
    int Tb = min((int)p.in_len[b], p.T);
    int tl = min((int)p.tg_len[b], p.Lmax);
    const int S = 2 * tl + 1;
    const int64_t *tgt = p.targets + (int64_t)b * p.tgt_stride;
    const int t0 = blockIdx.y * GATHER_ROWS;
    const float *lpb = p.lp + (int64_t)b * p.sb;
    float *out = p.lpg + (size_t)b * p.T * Smax;
    for (int idx = threadIdx.x; idx < GATHER_ROWS * Smax; idx += 256) {
        const int r = idx / Smax, sidx = idx - r * Smax;
        const int t = t0 + r;
        if (t < Tb && sidx < S)
            // a label outside [0,V) never reads out of bounds; the lattice kernel reports it (NaN loss)
            out[(size_t)t * Smax + sidx] =
                lpb[(int64_t)t * p.st + min(max(ext_label(tgt, sidx, p.blank), 0), p.V - 1)];
    }
}

// K1: alpha (blockIdx.y == 0) and beta (blockIdx.y == 1) lattices of utterance blockIdx.x, one wave
// each.  The gathered log-prob rows of the next PF frames are kept in registers (ring refilled PF
// steps ahead), so a step is: publish row -> barrier -> 3-way log-sum-exp; no memory latency on
// the dependent chain.
constexpr int CTC_PF = 8;
template <int SPL, bool FAST>
__global__ __launch_bounds__(CTC_THREADS) void ctc_lattice_kernel(CtcArgs p) {
    extern __shared__ float srow[];  // [2][Smax]
    const int b = blockIdx.x, lane = threadIdx.x;
    const bool bw = blockIdx.y == 1;
    const int Smax = 2 * p.Lmax + 1;
    const int spl = (Smax + CTC_THREADS - 1) / CTC_THREADS;   // <= SPL
    int Tb = min((int)p.in_len[b], p.T);
    int tl = min((int)p.tg_len[b], p.Lmax);
    const int S = 2 * tl + 1;
    const int64_t *tgt = p.targets + (int64_t)b * p.tgt_stride;
    float *out = (bw ? p.beta : p.alpha) + (size_t)b * p.T * Smax;
    const float *g = p.lpg + (size_t)b * p.T * Smax;

    bool skip_ok[SPL];  // may take the s-2 (alpha) / s+2 (beta) transition
#pragma unroll
    for (int j = 0; j < SPL; ++j) {
        skip_ok[j] = false;
        const int s = lane * spl + j;
        if (j < spl && s < S && (s & 1)) {
            const int lab = ext_label(tgt, s, p.blank);
            if (!bw) {
                if (s >= 2) skip_ok[j] = lab != ext_label(tgt, s - 2, p.blank);
            } else {
                if (s + 2 < S) skip_ok[j] = lab != ext_label(tgt, s + 2, p.blank);
            }
        }
    }

    if (Tb <= 0) {
        if (!bw && lane == 0) ctc_store_nll(p, b, (tl == 0) ? 0.f : INFINITY);
        return;
    }
    {   // torch.nn.CTCLoss rejects targets outside [0,V); here the utterance's loss becomes NaN (no
        // host sync), which the solver's NaN-gradient guard (src/solver.py:85-89) then skips
        bool bad = false;
        for (int i = lane; i < tl; i += CTC_THREADS) bad |= tgt[i] < 0 || tgt[i] >= p.V;
        if (__any(bad)) {
            if (!bw && lane == 0) ctc_store_nll(p, b, __builtin_nanf(""));
            return;
        }
    }
    const int t_first = bw ? Tb - 1 : 0;
    const int dt = bw ? -1 : 1;

    float cur[SPL], pre[CTC_PF][SPL];
#pragma unroll
    for (int j = 0; j < SPL; ++j) {
        cur[j] = -INFINITY;
        const int s = lane * spl + j;
        if (j < spl && s < S) {
            const bool init = bw ? (s >= S - 2) : (s <= 1);
            if (init) cur[j] = g[(size_t)t_first * Smax + s];
        }
    }
#pragma unroll
    for (int d = 0; d < CTC_PF; ++d)
#pragma unroll
        for (int j = 0; j < SPL; ++j) {
            pre[d][j] = 0.f;
            const int s = lane * spl + j;
            if (j < spl && s < S && 1 + d < Tb) pre[d][j] = g[(size_t)(t_first + dt * (1 + d)) * Smax + s];
        }

    for (int base = 0; base < Tb; base += CTC_PF) {
#pragma unroll
        for (int d = 0; d < CTC_PF; ++d) {
            const int step = base + d;
            if (step >= Tb) break;
            const int t = t_first + dt * step;
            float *row = srow + (step & 1) * Smax;
#pragma unroll
            for (int j = 0; j < SPL; ++j) {
                const int s = lane * spl + j;
                if (j < spl && s < Smax) {
                    row[s] = cur[j];
                    out[(size_t)t * Smax + s] = cur[j];
                }
            }
            if (step + 1 == Tb) break;
            float lpn[SPL];
            const int sp = step + 1 + CTC_PF;
#pragma unroll
            for (int j = 0; j < SPL; ++j) {
                lpn[j] = pre[d][j];
                const int s = lane * spl + j;
                if (j < spl && s < S && sp < Tb) pre[d][j] = g[(size_t)(t_first + dt * sp) * Smax + s];
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < SPL; ++j) {
                const int s = lane * spl + j;
                if (j < spl) {
                    if (s < S) {
                        float a0 = row[s], a1 = -INFINITY, a2 = -INFINITY;
                        if (!bw) {
                            if (s >= 1) a1 = row[s - 1];
                            if (skip_ok[j]) a2 = row[s - 2];
                        } else {
                            if (s + 1 < S) a1 = row[s + 1];
                            if (skip_ok[j]) a2 = row[s + 2];
                        }
                        cur[j] = lse3<FAST>(a0, a1, a2) + lpn[j];
                    } else {
                        cur[j] = -INFINITY;
                    }
                }
            }
        }
    }

    // rows beyond the utterance length are never read by the gradient kernels
    if (!bw) {
        __syncthreads();
        if (lane == 0) {
            const float *row = srow + ((Tb - 1) & 1) * Smax;
            const float l1 = row[S - 1];
            const float l2 = S >= 2 ? row[S - 2] : -INFINITY;
            ctc_store_nll(p, b, -log_add(l1, l2));
        }
    }
}

// dense part: grad = exp(lp) * scale (t < T_b) or 0; with zero_inf every row of an utterance whose nll is +inf is 0.
// An utterance the lattice flagged (nll NaN: a label outside [0,V), its alpha / beta rows were never written) gets NaN
// in every element of its frames t < T_b, so the gradient norm is NaN and the solver skips the step.
__global__ __launch_bounds__(256) void ctc_grad_dense_kernel(const float *__restrict__ lp,
                                                             int64_t st, int64_t sb, int T, int B,
                                                             int V, const int64_t *in_len,
                                                             const float *gscale,
                                                             float *__restrict__ grad, int64_t gst,
                                                             int64_t gsb, const float *nll, int zero_inf) {
    const int row = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // row = t*B + b
    const int lane = threadIdx.x & 63;
    if (row >= T * B) return;
    const int t = row / B, b = row - t * B;
    const float *x = lp + (int64_t)t * st + (int64_t)b * sb;
    float *g = grad + (int64_t)t * gst + (int64_t)b * gsb;
    const float nl = nll[b];
    const bool live = t < (int)in_len[b] && !(zero_inf && nl == INFINITY);
    const bool flagged = nl != nl;
    const float sc = gscale[b];
    const bool vec = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(g)) & 15) == 0 &&
                     (V % 4 == 0);
    if (vec) {
        const int nv = V >> 2;
        for (int i = lane; i < nv; i += 64) {
            f32x4 o = {0.f, 0.f, 0.f, 0.f};
            if (live && flagged) {
                o[0] = nl; o[1] = nl; o[2] = nl; o[3] = nl;
            } else if (live) {
                const f32x4 v = reinterpret_cast<const f32x4 *>(x)[i];
                o[0] = expf(v[0]) * sc; o[1] = expf(v[1]) * sc;
                o[2] = expf(v[2]) * sc; o[3] = expf(v[3]) * sc;
            }
            reinterpret_cast<f32x4 *>(g)[i] = o;
        }
    } else {
        for (int i = lane; i < V; i += 64) g[i] = !live ? 0.f : flagged ? nl : expf(x[i]) * sc;
    }
}

// sparse part: the label columns are OVERWRITTEN with (exp(lp) - exp(lcab + nll - lp)) * scale
// (runs after the dense pass; no read-modify-write of the gradient)
struct CtcFixArgs {
    int T, B;
    const int64_t *targets;
    int64_t tgt_stride;
    int Lmax;
    const int64_t *in_len, *tg_len;
    int blank;
    const float *alpha, *beta, *lpg, *nll, *gscale;
    float *grad;
    int64_t gst, gsb;
    int t_per_block;
    int zero_inf;
};

__global__ __launch_bounds__(256) void ctc_grad_fix_kernel(CtcFixArgs p) {
    extern __shared__ int sm_i[];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // zeroed utterance: the dense pass wrote 0 to all of its rows and the label columns stay 0 (nothing is
    // computed from the +inf, so no inf * 0); the whole workgroup shares b and leaves together
    if (p.zero_inf && p.nll[b] == INFINITY) return;
    // flagged utterance (NaN nll): its frames are NaN from the dense pass.  The labels that caused the flag lie outside
    // [0,V) and must never become a column index, and its alpha / beta rows were never written.
    if (p.nll[b] != p.nll[b]) return;
    const int Smax = 2 * p.Lmax + 1;
    int *ext = sm_i;                 // [Smax]
    int *nxt = sm_i + Smax;          // [Smax] next state with the same label (or -1)
    int *leader = sm_i + 2 * Smax;   // [Smax] 1 if first occurrence
    float *ab = reinterpret_cast<float *>(sm_i + 3 * Smax) + wave * Smax;  // [4 waves][Smax]
    int Tb = min((int)p.in_len[b], p.T);
    int tl = min((int)p.tg_len[b], p.Lmax);
    const int S = 2 * tl + 1;
    const int64_t *tgt = p.targets + (int64_t)b * p.tgt_stride;
    for (int s = threadIdx.x; s < S; s += blockDim.x) ext[s] = ext_label(tgt, s, p.blank);
    __syncthreads();
    for (int s = threadIdx.x; s < S; s += blockDim.x) {
        const int c = ext[s];
        int n = -1;
        for (int s2 = s + 1; s2 < S; ++s2)
            if (ext[s2] == c) { n = s2; break; }
        nxt[s] = n;
        int first = 1;
        for (int s2 = 0; s2 < s; ++s2)
            if (ext[s2] == c) { first = 0; break; }
        leader[s] = first;
    }
    __syncthreads();
    const float nll = p.nll[b], sc = p.gscale[b];
    const int t0 = blockIdx.y * p.t_per_block;
    const int t1 = min(Tb, t0 + p.t_per_block);
    const float *al = p.alpha + (size_t)b * p.T * Smax;
    const float *be = p.beta + (size_t)b * p.T * Smax;
    const float *lg = p.lpg + (size_t)b * p.T * Smax;
    for (int tb = t0; tb < t1; tb += 4) {       // 4 frames per iteration, one per wave
        const int t = tb + wave;
        const bool live = t < t1;
        if (live)
            for (int s = lane; s < S; s += 64) ab[s] = al[(size_t)t * Smax + s] + be[(size_t)t * Smax + s];
        __syncthreads();
        if (live) {
            // the blank sits on every even state (tl+1 of them): the whole wave reduces that column
            // as max + sum-of-exp instead of lane 0 walking a tl-long log_add chain per frame
            float m = -INFINITY;
            for (int s = lane; s < S; s += 64)
                if (ext[s] == p.blank) m = fmaxf(m, ab[s]);   // even states (+ a label equal to blank)
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
            float sum = 0.f;
            if (m > -INFINITY)
                for (int s = lane; s < S; s += 64)
                    if (ext[s] == p.blank) sum += expf(ab[s] - m);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
            if (lane == 0) {
                const float acc = m > -INFINITY ? m + logf(sum) : -INFINITY;
                const float x = lg[(size_t)t * Smax];
                p.grad[(int64_t)t * p.gst + (int64_t)b * p.gsb + p.blank] =
                    (expf(x) - expf(acc + nll - x)) * sc;
            }
            for (int s = 1 + 2 * lane; s < S; s += 128) {   // label states (odd), first occurrences
                if (leader[s] && ext[s] != p.blank) {
                    float acc = ab[s];
                    for (int n = nxt[s]; n >= 0; n = nxt[n]) acc = log_add(acc, ab[n]);
                    const float x = lg[(size_t)t * Smax + s];
                    p.grad[(int64_t)t * p.gst + (int64_t)b * p.gsb + ext[s]] =
                        (expf(x) - expf(acc + nll - x)) * sc;
                }
            }
        }
        __syncthreads();
    }
}

}  // namespace

extern "C" int asrk_ctc_loss_plan_info(int T, int B, int Lmax, int *info, int n) {
    if (!info || n < ASRK_CTC_LOSS_PLAN_INFO_LEN) return ASRK_EINVAL;
    for (int i = 0; i < n; ++i) info[i] = 0;
    if (T < 0 || B < 0 || Lmax < 0) return ASRK_EINVAL;
    if (Lmax > (CTC_THREADS * CTC_MAX_SPL - 1) / 2) return ASRK_ESHAPE;
    const CtcPlan pl = ctc_plan(T, B, Lmax);
    info[0] = pl.spl_tmpl;
    info[1] = pl.fast;
    info[2] = pl.spl;
    info[3] = pl.gather_y;
    info[4] = pl.t_per_block;
    info[5] = pl.tchunks;
    info[6] = pl.dense_grid;
    info[7] = 2 * Lmax + 1;
    return ASRK_OK;
}

extern "C" int asrk_ctc_loss_fwd_f32(const float *lp, int64_t stride_t, int64_t stride_b, int T,
                                     int B, int V, const int64_t *targets, int64_t tgt_stride,
                                     int Lmax, const int64_t *input_lengths,
                                     const int64_t *target_lengths, int blank, float *alpha,
                                     float *beta, float *lpg, float *nll, void *stream) {
    return asrk_ctc_loss_fwd_ex_f32(lp, stride_t, stride_b, T, B, V, targets, tgt_stride, Lmax, input_lengths,
                                    target_lengths, blank, alpha, beta, lpg, nll, 0, nullptr, nullptr, stream);
}

extern "C" int asrk_ctc_loss_fwd_ex_f32(const float *lp, int64_t stride_t, int64_t stride_b, int T, int B, int V,
                                        const int64_t *targets, int64_t tgt_stride, int Lmax,
                                        const int64_t *input_lengths, const int64_t *target_lengths, int blank,
                                        float *alpha, float *beta, float *lpg, float *nll, int flags, float *loss,
                                        int32_t *n_infeasible, void *stream) {
    if (T < 0 || B < 0 || V <= 0 || Lmax < 0 || blank < 0 || blank >= V) return ASRK_EINVAL;
    if (flags & ~ASRK_CTC_ZERO_INFINITY) return ASRK_EINVAL;
    if ((flags & ASRK_CTC_ZERO_INFINITY) && !loss) return ASRK_EINVAL;
    if (B == 0) return ASRK_OK;
    if (!lp || !input_lengths || !target_lengths || !alpha || !lpg || !nll) return ASRK_EINVAL;
    if (Lmax > 0 && !targets) return ASRK_EINVAL;
    const int Smax = 2 * Lmax + 1;
    if (Smax > CTC_THREADS * CTC_MAX_SPL) return ASRK_ESHAPE;
    hipStream_t s = (hipStream_t)stream;
    if (loss && n_infeasible) ASRK_HIP(hipMemsetAsync(n_infeasible, 0, sizeof(int32_t), s));
    CtcArgs a{lp, stride_t, stride_b, T, B, V, targets, tgt_stride, Lmax, input_lengths,
              target_lengths, blank, alpha, beta, lpg, nll, loss, loss ? n_infeasible : nullptr,
              (flags & ASRK_CTC_ZERO_INFINITY) ? 1 : 0};
    asrk_prof_begin_(PROF_CTC, s);
    const CtcPlan pl = ctc_plan(T, B, Lmax);
    if (pl.gather_y > 0)
        hipLaunchKernelGGL(ctc_gather_kernel, dim3(B, pl.gather_y), dim3(256), 0, s, a);
    const dim3 grid(B, beta ? 2 : 1);
    if (pl.spl_tmpl == 4 && pl.fast)
        hipLaunchKernelGGL((ctc_lattice_kernel<4, true>), grid, dim3(CTC_THREADS), 2 * Smax * sizeof(float), s, a);
    else if (pl.spl_tmpl == 4)
        hipLaunchKernelGGL((ctc_lattice_kernel<4, false>), grid, dim3(CTC_THREADS), 2 * Smax * sizeof(float), s, a);
    else if (pl.spl_tmpl == 16)
        hipLaunchKernelGGL((ctc_lattice_kernel<16, false>), grid, dim3(CTC_THREADS), 2 * Smax * sizeof(float), s, a);
    else   // character-level transcripts of the longest LibriSpeech utterances (L up to 1023)
        hipLaunchKernelGGL((ctc_lattice_kernel<CTC_MAX_SPL, false>), grid, dim3(CTC_THREADS),
                           2 * Smax * sizeof(float), s, a);
    asrk_prof_end_(PROF_CTC, s);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}

extern "C" int asrk_ctc_loss_bwd_f32(const float *lp, int64_t stride_t, int64_t stride_b, int T,
                                     int B, int V, const int64_t *targets, int64_t tgt_stride,
                                     int Lmax, const int64_t *input_lengths,
                                     const int64_t *target_lengths, int blank, const float *alpha,
                                     const float *beta, const float *lpg, const float *nll,
                                     const float *gscale, float *grad, int64_t g_stride_t,
                                     int64_t g_stride_b, void *stream) {
    return asrk_ctc_loss_bwd_ex_f32(lp, stride_t, stride_b, T, B, V, targets, tgt_stride, Lmax, input_lengths,
                                    target_lengths, blank, alpha, beta, lpg, nll, gscale, grad, g_stride_t,
                                    g_stride_b, 0, stream);
}

extern "C" int asrk_ctc_loss_bwd_ex_f32(const float *lp, int64_t stride_t, int64_t stride_b, int T, int B, int V,
                                        const int64_t *targets, int64_t tgt_stride, int Lmax,
                                        const int64_t *input_lengths, const int64_t *target_lengths, int blank,
                                        const float *alpha, const float *beta, const float *lpg, const float *nll,
                                        const float *gscale, float *grad, int64_t g_stride_t, int64_t g_stride_b,
                                        int flags, void *stream) {
    if (T < 0 || B < 0 || V <= 0 || Lmax < 0 || blank < 0 || blank >= V) return ASRK_EINVAL;
    if (flags & ~ASRK_CTC_ZERO_INFINITY) return ASRK_EINVAL;
    const int zero_inf = (flags & ASRK_CTC_ZERO_INFINITY) ? 1 : 0;
    if (B == 0 || T == 0) return ASRK_OK;
    if (!lp || !input_lengths || !target_lengths || !alpha || !beta || !lpg || !nll || !gscale || !grad)
        return ASRK_EINVAL;
    if (Lmax > 0 && !targets) return ASRK_EINVAL;
    const int Smax = 2 * Lmax + 1;
    if (Smax > CTC_THREADS * CTC_MAX_SPL) return ASRK_ESHAPE;
    hipStream_t s = (hipStream_t)stream;
    // dense gradient: every log-prob read, every gradient element written (the lattice itself is a few MB)
    asrk_prof_work_(PROF_CTC, 8.0 * (double)T * (double)B * (double)V);
    asrk_prof_begin_(PROF_CTC, s);
    const CtcPlan pl = ctc_plan(T, B, Lmax);
    hipLaunchKernelGGL(ctc_grad_dense_kernel, dim3(pl.dense_grid), dim3(256), 0, s, lp,
                       stride_t, stride_b, T, B, V, input_lengths, gscale, grad, g_stride_t,
                       g_stride_b, nll, zero_inf);
    CtcFixArgs f{T, B, targets, tgt_stride, Lmax, input_lengths, target_lengths, blank, alpha, beta,
                 lpg, nll, gscale, grad, g_stride_t, g_stride_b, pl.t_per_block, zero_inf};
    hipLaunchKernelGGL(ctc_grad_fix_kernel, dim3(B, pl.tchunks), dim3(256),
                       (size_t)Smax * (3 * sizeof(int) + 4 * sizeof(float)), s, f);
    asrk_prof_end_(PROF_CTC, s);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}

// ---------------------------------------------------------------------------------------------
// CTC forced alignment: the best (Viterbi) path of every utterance through its blank-extended label
// sequence.  The walk is ctc_lattice_kernel's alpha walk (one wave per utterance, states s = lane*spl + j,
// previous row in LDS, the next CTC_PF gathered rows in registers) with max in place of lse3:
//     delta_t[s] = max(delta_{t-1}[s], delta_{t-1}[s-1], delta_{t-1}[s-2] if skip_ok) + lp_t[ext[s]]
// plain f32 compares and one add, so a host f32 computation in the same order gives the same bits.  Ties
// take the smallest jump (a candidate replaces the best only if strictly greater, tried 0, 1, 2).
// Backpointers: jump 0..2 of every state and frame, stored as bit planes - for frame t and register slot
// j two 64-bit lane masks (__ballot of the jump's low and high bit), i.e. 2 bits per state slot and
// 4*spl 32-bit words per frame, written by lane 0 - either into LDS behind the two lattice rows or into the
// caller's workspace.  The backtrace runs in the same launch: lane 0 follows the chain (one dependent 16-byte
// read per frame) and stores the state of every frame; then all lanes derive tokens and spans from the states.
namespace {

struct AlignArgs {
    CtcArgs c;            // lp, lengths, targets, lpg (alpha / beta / nll unused)
    int32_t *states;      // [B, T]
    int32_t *tokens;      // [B, T]
    int32_t *spans;       // [B, Lmax, 2]
    float *score;         // [B]
    uint64_t *bp;         // global route: [B, T, spl, 2]
    int64_t *stamps;      // optional [B, 4]: wall_clock64 at start / lattice done / backtrace done / end
};

constexpr size_t ALIGN_LDS_BP_BUDGET = 128 * 1024;   // bytes of LDS backpointers per utterance (+ <= 16 KiB rows)

struct alignas(16) BpPair { uint64_t lo, hi; };

static inline size_t align_rows_bytes(int Smax) { return ((size_t)2 * Smax * sizeof(float) + 15) & ~(size_t)15; }
static inline int align_spl(int Smax) { return (Smax + CTC_THREADS - 1) / CTC_THREADS; }
static inline size_t align_bp_bytes(int T, int Smax) { return (size_t)T * align_spl(Smax) * sizeof(BpPair); }

template <int SPL, bool BP_LDS>
__global__ __launch_bounds__(CTC_THREADS) void ctc_viterbi_kernel(AlignArgs a, int rows_bytes) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const CtcArgs &p = a.c;
    float *srow = reinterpret_cast<float *>(smem);   // [2][Smax]
    const int b = blockIdx.x, lane = threadIdx.x;
    const int Smax = 2 * p.Lmax + 1;
    const int spl = (Smax + CTC_THREADS - 1) / CTC_THREADS;   // <= SPL
    const int Tb = min((int)p.in_len[b], p.T);
    const int tl = max(min((int)p.tg_len[b], p.Lmax), 0);
    const int S = 2 * tl + 1;
    const int64_t *tgt = p.targets + (int64_t)b * p.tgt_stride;
    const float *g = p.lpg + (size_t)b * p.T * Smax;
    int32_t *st = a.states + (size_t)b * p.T;
    int32_t *tok = a.tokens + (size_t)b * p.T;
    int32_t *sp = a.spans + (size_t)b * p.Lmax * 2;
    BpPair *bp = BP_LDS ? reinterpret_cast<BpPair *>(smem + rows_bytes)
                        : reinterpret_cast<BpPair *>(a.bp) + (size_t)b * p.T * spl;
    int64_t *stamp = a.stamps ? a.stamps + (size_t)b * 4 : nullptr;
    if (stamp && lane == 0) stamp[0] = (int64_t)wall_clock64();

    bool bad = false;     // a target outside [0,V): NaN score like the loss, and nothing is aligned
    for (int i = lane; i < tl; i += CTC_THREADS) bad |= tgt[i] < 0 || tgt[i] >= p.V;
    bad = __any(bad);

    float score = bad ? __builtin_nanf("") : (tl == 0 ? 0.f : -INFINITY);   // value when there is no frame
    int sfin = 0;
    if (!bad && Tb > 0) {
        // bit j: register slot j holds a state of this utterance / may take the s-2 transition (per-lane bit sets in
        // one VGPR each: SPL separate lane predicates would cost two SGPRs apiece)
        unsigned live = 0, skip = 0;
#pragma unroll
        for (int j = 0; j < SPL; ++j) {
            const int s = lane * spl + j;
            if (j < spl && s < S) {
                live |= 1u << j;
                if ((s & 1) && s >= 2 && ext_label(tgt, s, p.blank) != ext_label(tgt, s - 2, p.blank))
                    skip |= 1u << j;
            }
        }
        float cur[SPL], pre[CTC_PF][SPL];
#pragma unroll
        for (int j = 0; j < SPL; ++j) {
            cur[j] = -INFINITY;
            const int s = lane * spl + j;
            if (((live >> j) & 1) && s <= 1) cur[j] = g[s];
        }
#pragma unroll
        for (int d = 0; d < CTC_PF; ++d)
#pragma unroll
            for (int j = 0; j < SPL; ++j) {
                pre[d][j] = 0.f;
                const int s = lane * spl + j;
                if (((live >> j) & 1) && 1 + d < Tb) pre[d][j] = g[(size_t)(1 + d) * Smax + s];
            }

        for (int base = 0; base < Tb; base += CTC_PF) {
#pragma unroll
            for (int d = 0; d < CTC_PF; ++d) {
                const int step = base + d;
                if (step >= Tb) break;
                float *row = srow + (step & 1) * Smax;
#pragma unroll
                for (int j = 0; j < SPL; ++j) {
                    const int s = lane * spl + j;
                    if (j < spl && s < Smax) row[s] = cur[j];
                }
                if (step + 1 == Tb) break;
                float lpn[SPL];
                const int nx = step + 1 + CTC_PF;
#pragma unroll
                for (int j = 0; j < SPL; ++j) {
                    lpn[j] = pre[d][j];
                    const int s = lane * spl + j;
                    if (((live >> j) & 1) && nx < Tb) pre[d][j] = g[(size_t)nx * Smax + s];
                }
                __syncthreads();
#pragma unroll
                for (int j = 0; j < SPL; ++j) {
                    if (j < spl) {          // uniform over the wave: every lane reaches the ballots
                        const int s = lane * spl + j;
                        int jump = 0;
                        if ((live >> j) & 1) {
                            float best = row[s];
                            if (s >= 1) {
                                const float a1 = row[s - 1];
                                if (a1 > best) { best = a1; jump = 1; }
                            }
                            if ((skip >> j) & 1) {
                                const float a2 = row[s - 2];
                                if (a2 > best) { best = a2; jump = 2; }
                            }
                            cur[j] = best + lpn[j];
                        } else {
                            cur[j] = -INFINITY;
                        }
                        const uint64_t lo = __ballot(jump & 1), hi = __ballot(jump & 2);
                        if (lane == 0) bp[(size_t)(step + 1) * spl + j] = BpPair{lo, hi};
                    }
                }
            }
        }
        __syncthreads();
        {   // final state: S-1 unless delta[S-2] is strictly greater (all lanes read the same two words)
            const float *row = srow + ((Tb - 1) & 1) * Smax;
            const float l1 = row[S - 1];
            const float l2 = S >= 2 ? row[S - 2] : -INFINITY;
            sfin = S - 1;
            score = l1;
            if (l2 > l1) { sfin = S - 2; score = l2; }
        }
    }
    if (stamp && lane == 0) stamp[1] = (int64_t)wall_clock64();

    // a path exists only behind a score above -inf (false for -inf: too few frames for the target or no path of
    // non-zero probability; false for NaN)
    const bool ok = !bad && Tb > 0 && score > -INFINITY;
    if (ok && lane == 0) {
        int s = sfin;
        int ln = s / spl, j = s - ln * spl;     // the lane and register slot that own state s
        for (int t = Tb - 1; t >= 1; --t) {
            st[t] = s;
            const BpPair w = bp[(size_t)t * spl + j];
            const int jump = (int)((w.lo >> ln) & 1) | ((int)((w.hi >> ln) & 1) << 1);
            s -= jump;
            j -= jump;
            if (j < 0) { j += spl; --ln; }
            if (j < 0) { j += spl; --ln; }      // spl == 1 and a jump of 2
            if (s < 0) { s = 0; ln = 0; j = 0; }   // cannot happen behind a finite score; keeps every read in bounds
        }
        st[0] = s;
    }
    __syncthreads();    // the states lane 0 stored are visible to the whole wave
    if (stamp && lane == 0) stamp[2] = (int64_t)wall_clock64();

    const int Tv = ok ? Tb : 0, Lv = ok ? tl : 0;
    for (int t = lane; t < p.T; t += CTC_THREADS) {
        if (t >= Tv) {
            st[t] = -1;
            tok[t] = -1;
            continue;
        }
        const int s = st[t];
        tok[t] = ext_label(tgt, s, p.blank);
        if (s & 1) {      // every target token owns one run of frames
            if (t == 0 || st[t - 1] != s) sp[s - 1] = t;               // spans[s >> 1][0]
            if (t == Tv - 1 || st[t + 1] != s) sp[s] = t + 1;          // spans[s >> 1][1]
        }
    }
    for (int i = 2 * Lv + lane; i < 2 * p.Lmax; i += CTC_THREADS) sp[i] = -1;
    if (lane == 0) {
        a.score[b] = score;
        if (stamp) stamp[3] = (int64_t)wall_clock64();
    }
}

// 0 = bad flags / shape, else ASRK_ALIGN_BP_LDS or ASRK_ALIGN_BP_GLOBAL
static int align_route(int T, int Smax, int flags) {
    const bool fits = align_bp_bytes(T, Smax) <= ALIGN_LDS_BP_BUDGET;
    if (flags == ASRK_ALIGN_BP_AUTO) return fits ? ASRK_ALIGN_BP_LDS : ASRK_ALIGN_BP_GLOBAL;
    if (flags == ASRK_ALIGN_BP_LDS) return fits ? ASRK_ALIGN_BP_LDS : 0;
    return flags == ASRK_ALIGN_BP_GLOBAL ? ASRK_ALIGN_BP_GLOBAL : 0;
}

static inline size_t align_lpg_bytes(int B, int T, int Smax) {
    return ((size_t)B * T * Smax * sizeof(float) + 15) & ~(size_t)15;
}

template <int SPL, bool BP_LDS>
static int align_launch(const AlignArgs &a, int B, size_t rows_bytes, size_t lds, hipStream_t s) {
    static AsrkLdsLatch latch;
    if (BP_LDS)
        ASRK_HIP(asrk_max_lds_once(latch, reinterpret_cast<const void *>(ctc_viterbi_kernel<SPL, BP_LDS>),
                               (int)(align_rows_bytes(CTC_THREADS * CTC_MAX_SPL) + ALIGN_LDS_BP_BUDGET)));
    hipLaunchKernelGGL((ctc_viterbi_kernel<SPL, BP_LDS>), dim3(B), dim3(CTC_THREADS), lds, s, a, (int)rows_bytes);
    return ASRK_OK;
}

}  // namespace

extern "C" size_t asrk_ctc_align_ws_bytes(int B, int T, int Lmax, int flags) {
    if (B <= 0 || T <= 0 || Lmax < 0 || Lmax > (CTC_THREADS * CTC_MAX_SPL - 1) / 2) return 0;
    const int Smax = 2 * Lmax + 1;
    const int route = align_route(T, Smax, flags);
    if (!route) return 0;
    return align_lpg_bytes(B, T, Smax) + (route == ASRK_ALIGN_BP_GLOBAL ? (size_t)B * align_bp_bytes(T, Smax) : 0);
}

extern "C" int asrk_ctc_align_f32(const float *lp, int64_t stride_t, int64_t stride_b, int T, int B, int V,
                                  const int64_t *targets, int64_t tgt_stride, int Lmax,
                                  const int64_t *input_lengths, const int64_t *target_lengths, int blank,
                                  int flags, int32_t *states, int32_t *tokens, int32_t *spans, float *score,
                                  int64_t *stamps, void *ws, size_t ws_bytes, void *stream) {
    if (T < 0 || B < 0 || V <= 0 || Lmax < 0 || blank < 0 || blank >= V) return ASRK_EINVAL;
    if (flags != ASRK_ALIGN_BP_AUTO && flags != ASRK_ALIGN_BP_LDS && flags != ASRK_ALIGN_BP_GLOBAL)
        return ASRK_EINVAL;
    if (B == 0) return ASRK_OK;
    if (!input_lengths || !target_lengths || !score) return ASRK_EINVAL;
    if (T > 0 && (!lp || !states || !tokens)) return ASRK_EINVAL;
    if (Lmax > 0 && (!targets || !spans)) return ASRK_EINVAL;
    const int Smax = 2 * Lmax + 1;
    if (Smax > CTC_THREADS * CTC_MAX_SPL) return ASRK_ESHAPE;
    const int route = align_route(T, Smax, flags);
    if (!route) return ASRK_ESHAPE;       // a forced LDS route whose backpointers do not fit the budget
    const size_t lpg_bytes = align_lpg_bytes(B, T, Smax);
    const size_t need = lpg_bytes + (route == ASRK_ALIGN_BP_GLOBAL ? (size_t)B * align_bp_bytes(T, Smax) : 0);
    if (need > 0 && (!ws || ((uintptr_t)ws & 15))) return ASRK_EINVAL;
    if (ws_bytes < need) return ASRK_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    AlignArgs a{};
    a.c = CtcArgs{lp, stride_t, stride_b, T, B, V, targets, tgt_stride, Lmax, input_lengths, target_lengths, blank,
                  nullptr, nullptr, reinterpret_cast<float *>(ws), nullptr};
    a.states = states;
    a.tokens = tokens;
    a.spans = spans;
    a.score = score;
    a.bp = route == ASRK_ALIGN_BP_GLOBAL ? reinterpret_cast<uint64_t *>(static_cast<char *>(ws) + lpg_bytes) : nullptr;
    a.stamps = stamps;
    asrk_prof_begin_(PROF_CTC, s);
    if (T > 0)
        hipLaunchKernelGGL(ctc_gather_kernel, dim3(B, asrk_div_up(T, GATHER_ROWS)), dim3(256), 0, s, a.c);
    const size_t rows = align_rows_bytes(Smax);
    const bool lds_bp = route == ASRK_ALIGN_BP_LDS;
    const size_t lds = rows + (lds_bp ? align_bp_bytes(T, Smax) : 0);
    int rc;
    if (Smax <= CTC_THREADS * 4)
        rc = lds_bp ? align_launch<4, true>(a, B, rows, lds, s) : align_launch<4, false>(a, B, rows, lds, s);
    else if (Smax <= CTC_THREADS * 16)
        rc = lds_bp ? align_launch<16, true>(a, B, rows, lds, s) : align_launch<16, false>(a, B, rows, lds, s);
    else
        rc = lds_bp ? align_launch<CTC_MAX_SPL, true>(a, B, rows, lds, s)
                    : align_launch<CTC_MAX_SPL, false>(a, B, rows, lds, s);
    asrk_prof_end_(PROF_CTC, s);
    if (rc != ASRK_OK) return rc;
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}

// ---------------------------------------------------------------------------------------------
// CTC prefix scoring for joint CTC-attention beam search (reference: src/ctc.py:76-116,
// CTCPrefixScore.cheap_compute — numpy on the host, one hypothesis at a time).  Here ALL
// (hypothesis, candidate) pairs of a beam step run in one launch: one lane per pair walks the
// T' frames with its two running log-probabilities in registers.
namespace {

__device__ __forceinline__ float lae(float a, float b) {   // np.logaddexp for finite inputs
    const float m = fmaxf(a, b);
    return m + log1pf(expf(-fabsf(a - b)));
}

struct PrefixArgs {
    const float *x;        // [T, V] log-probs of the utterance
    const float *r_prev;   // [n, T, 2] previous state of each hypothesis (0 = non-blank, 1 = blank)
    const int *plen;       // [n] prefix length |g|
    const int *last;       // [n] last token of the prefix (ignored when plen == 0)
    const int *cand;       // [n, C]
    float *psi;            // [n, C]
    float *r_out;          // [n, C, T, 2]
    int n, C, T, V, blank, eos;
    float logzero;
    const int *row_mem;    // optional [n]: hypothesis h scores against utterance row_mem[h] of x [U, T, V]
    const int *mem_len;    // optional [U]: frames of every utterance (<= T, the common stride)
};

__global__ void ctc_prefix_kernel(PrefixArgs p) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.n * p.C) return;
    const int h = i / p.C;
    const int c = p.cand[i];
    const int TS = p.T, V = p.V;                       // TS: stride of the state arrays
    const int u = p.row_mem ? p.row_mem[h] : 0;
    const int T = p.mem_len ? min(p.mem_len[u], TS) : TS;   // frames of this hypothesis' utterance
    const float *px = p.x + (size_t)u * TS * V;
    const float *rp = p.r_prev + (size_t)h * TS * 2;
    float *ro = p.r_out + (size_t)i * TS * 2;
    const int plen = p.plen[h];
    const bool same = plen > 0 && c == p.last[h];   // phi uses only the blank path (ctc.py:97-99)
    const int start = plen > 1 ? plen : 1;
    for (int t = 0; t < TS; ++t) {
        ro[2 * t] = p.logzero;
        ro[2 * t + 1] = p.logzero;
    }
    if (plen == 0) ro[0] = px[c];                   // r[0,0] = x[0, c] if g = <sos>
    float rn = (start - 1 < T) ? ro[2 * (start - 1)] : p.logzero;       // r[t-1, 0]
    float rb = (start - 1 < T) ? ro[2 * (start - 1) + 1] : p.logzero;   // r[t-1, 1]
    float psi = rn;
    for (int t = start; t < T; ++t) {
        const float phi = same ? rp[2 * (t - 1) + 1] : lae(rp[2 * (t - 1)], rp[2 * (t - 1) + 1]);
        const float xc = px[(size_t)t * V + c], xb = px[(size_t)t * V + p.blank];
        const float nn = lae(rn, phi) + xc;
        const float nb = lae(rb, rn) + xb;
        psi = lae(psi, phi + xc);
        rn = nn;
        rb = nb;
        ro[2 * t] = rn;
        ro[2 * t + 1] = rb;
    }
    // P(<eos>) = P(g); an utterance with no frames left after the encoder's time reduction has no path at all
    if (c == p.eos) psi = T > 0 ? lae(rp[2 * (T - 1)], rp[2 * (T - 1) + 1]) : p.logzero;
    p.psi[i] = psi;
}

// One 64-thread workgroup per hypothesis, one lane per candidate.  Everything the T'-step chain reads is
// staged in LDS first by all lanes in parallel (the candidate's log-prob column x[t, c] - a stride-V
// gather -, phi[t] and the blank terms, which only depend on the hypothesis), so the dependent chain is
// 2 LDS reads + 3 log-add-exps per frame instead of 4 global loads (206 -> ~25 us per beam step at
// T' = 200); the new states leave through LDS as coalesced rows.
__device__ __forceinline__ float lae_fast(float a, float b) {
    const float m = fmaxf(a, b);
    return m + __logf(1.f + __expf(-fabsf(a - b)));
}

__global__ __launch_bounds__(64) void ctc_prefix_lds_kernel(PrefixArgs p) {
    extern __shared__ float sm[];
    const int h = blockIdx.x, lane = threadIdx.x;
    const int TS = p.T, V = p.V, C = p.C;              // TS: stride of the state arrays (LDS images included)
    const int u = p.row_mem ? p.row_mem[h] : 0;
    const int T = p.mem_len ? min(p.mem_len[u], TS) : TS;   // frames of this hypothesis' utterance
    const float *px = p.x + (size_t)u * TS * V;
    float *s_phi = sm;                 // [TS] logaddexp(r_prev[t,0], r_prev[t,1])
    float *s_rb = s_phi + TS;          // [TS] r_prev[t,1]
    float *s_xb = s_rb + TS;           // [TS] x[t, blank]
    float *s_xc = s_xb + TS;           // [TS][C]
    float *s_ro = s_xc + (size_t)TS * C;   // [C][2 TS]
    const float *rp = p.r_prev + (size_t)h * TS * 2;
    for (int t = lane; t < T; t += 64) {
        const float a = rp[2 * t], b = rp[2 * t + 1];
        s_phi[t] = lae_fast(a, b);
        s_rb[t] = b;
        s_xb[t] = px[(size_t)t * V + p.blank];
    }
    for (int i = lane; i < T * C; i += 64) {
        const int t = i / C, c = i - t * C;
        s_xc[i] = px[(size_t)t * V + p.cand[(size_t)h * C + c]];
    }
    for (int i = lane; i < 2 * TS * C; i += 64) s_ro[i] = p.logzero;
    __syncthreads();
    const int plen = p.plen[h];
    if (lane < C) {
        const int c = p.cand[(size_t)h * C + lane];
        const bool same = plen > 0 && c == p.last[h];
        const int start = plen > 1 ? plen : 1;
        float *ro = s_ro + (size_t)lane * 2 * TS;
        if (plen == 0) ro[0] = s_xc[lane];
        float rn = (start - 1 < T) ? ro[2 * (start - 1)] : p.logzero;
        float rb = (start - 1 < T) ? ro[2 * (start - 1) + 1] : p.logzero;
        float psi = rn;
        for (int t = start; t < T; ++t) {
            const float phi = same ? s_rb[t - 1] : s_phi[t - 1];
            const float xc = s_xc[t * C + lane];
            const float nn = lae_fast(rn, phi) + xc;
            const float nb = lae_fast(rb, rn) + s_xb[t];
            psi = lae_fast(psi, phi + xc);
            rn = nn;
            rb = nb;
            ro[2 * t] = rn;
            ro[2 * t + 1] = rb;
        }
        if (c == p.eos) psi = T > 0 ? s_phi[T - 1] : p.logzero;
        p.psi[(size_t)h * C + lane] = psi;
    }
    __syncthreads();
    float *out = p.r_out + (size_t)h * C * 2 * TS;
    for (int i = lane; i < 2 * TS * C; i += 64) out[i] = s_ro[i];
}

}  // namespace

extern "C" int asrk_ctc_prefix_score_f32(const float *x, const float *r_prev, const int *prefix_len,
                                         const int *last_char, const int *candidates, float *psi,
                                         float *r_out, int n, int C, int T, int V, int blank, int eos,
                                         float logzero, void *stream) {
    return asrk_ctc_prefix_score_multi_f32(x, nullptr, nullptr, r_prev, prefix_len, last_char, candidates, psi,
                                           r_out, n, C, T, V, 1, blank, eos, logzero, stream);
}

extern "C" int asrk_ctc_prefix_score_multi_f32(const float *x, const int *row_mem, const int *mem_len,
                                               const float *r_prev, const int *prefix_len, const int *last_char,
                                               const int *candidates, float *psi, float *r_out, int n, int C,
                                               int T, int V, int U, int blank, int eos, float logzero,
                                               void *stream) {
    if (n < 0 || C < 0 || T <= 0 || V <= 0 || U <= 0) return ASRK_EINVAL;
    if ((row_mem == nullptr) != (mem_len == nullptr)) return ASRK_EINVAL;
    if (n == 0 || C == 0) return ASRK_OK;
    if (!x || !r_prev || !prefix_len || !last_char || !candidates || !psi || !r_out) return ASRK_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    PrefixArgs a{x, r_prev, prefix_len, last_char, candidates, psi, r_out, n, C, T, V, blank, eos, logzero,
                 row_mem, mem_len};
    asrk_prof_begin_(PROF_CTC, s);
    const size_t lds = ((size_t)3 * T + (size_t)3 * T * C) * sizeof(float);
    if (C <= 64 && lds <= 150 * 1024) {
        ASRK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(ctc_prefix_lds_kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(ctc_prefix_lds_kernel, dim3(n), dim3(64), lds, s, a);
    } else {
        hipLaunchKernelGGL(ctc_prefix_kernel, dim3(asrk_div_up(n * C, 64)), dim3(64), 0, s, a);
    }
    asrk_prof_end_(PROF_CTC, s);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}
