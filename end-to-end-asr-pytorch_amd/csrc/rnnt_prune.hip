// Pruned transducer training for gfx950 (Kuang et al. 2022; src/transducer.py: TransducerHead.forward_pruned).
//
//   asrk_rnnt_simple_rows_f32    the additive joiner am[b,t,:] + lm[b,u,:] on the whole lattice: per cell the log-sum-exp
//                                over v and the blank / label log-probabilities.  A workgroup owns 16 x 16 cells and
//                                streams V through LDS in chunks of 64 columns; nothing of size [.., U1, V] exists.
//   asrk_rnnt_simple_occ_f32     occupation of every cell and of its two arcs from alpha, beta (rnnt.inc: rnnt_coef).
//   asrk_rnnt_simple_grad_f32    dam and dlm, two launches: a thread owns output elements and adds its terms in
//                                ascending order of the reduced index (u for dam, t for dlm).
//   asrk_rnnt_prune_ranges_f32   the band start s(t) of every frame, one wave per utterance (rule: rnnt_prune.inc).
//   asrk_rnnt_joint_band_f32     H[b,t,k,:] = tanh(E[b,t,:] + P[b, min(s(t)+k, U1-1), :]) and its backward.
//   asrk_rnnt_rows_band_f32      row pass of the band loss on logits [B,T,S,V]; the arithmetic of asrk_rnnt_rows_f32.
//   asrk_rnnt_band_scatter_f32   band lpb / lpl -> dense [B,T,U1] arrays, -inf outside the band, for the dense lattice.
//   asrk_rnnt_grad_band_f32      gradient pass of the band loss, in place or out of place.
//
// wave64, no float atomics: every result is a pure function of its inputs, reproducible bit for bit.
#include "rnnt_rows.h"
#include "rnnt_prune.inc"

namespace {

constexpr int SJ_T = 16, SJ_U = 16;     // cells per workgroup of the simple row pass
constexpr int SJ_VC = 64;               // columns per LDS chunk
constexpr int SJ_LD = SJ_VC + 4;        // row stride in LDS: 16-byte aligned rows, 16 label rows on distinct banks
constexpr int SG_R = 4;                 // output rows per thread of the simple gradient
constexpr int PRUNE_MAX_S = 32;

struct SimpleArgs {
    const float *am;         // [B, T, V], row stride lda
    int64_t lda;
    const float *lm;         // [B, U1, V], row stride ldl
    int64_t ldl;
    const int64_t *txt;      // [B, txt_stride]
    int64_t txt_stride;
    const int64_t *enc_len, *txt_len;
    int B, T, U1, V, blank;
};

// ---------------------------------------------------------------------------------------------
// simple joiner: row pass

__global__ __launch_bounds__(256) void rnnt_simple_rows_kernel(SimpleArgs p, float *__restrict__ lse_out,
                                                               float *__restrict__ lpb, float *__restrict__ lpl) {
    __shared__ __attribute__((aligned(16))) float sa[SJ_T][SJ_LD];
    __shared__ __attribute__((aligned(16))) float sl[SJ_U][SJ_LD];
    const int b = blockIdx.z, t0 = blockIdx.y * SJ_T, u0 = blockIdx.x * SJ_U;
    const int tid = threadIdx.x, ui = tid & (SJ_U - 1), ti = tid / SJ_U;
    const int t = t0 + ti, u = u0 + ui;
    const int Tb = rnnt_clamp_T(p.enc_len[b], p.T), Ub = rnnt_clamp_U(p.txt_len[b], p.U1);
    const bool in_tile = t < p.T && u < p.U1, inside = t < Tb && u <= Ub;
    const size_t cell = ((size_t)b * p.T + t) * p.U1 + u;
    if (t0 >= Tb || u0 > Ub) {          // uniform: the whole tile lies outside the lattice, nothing is read
        if (in_tile) lse_out[cell] = lpb[cell] = lpl[cell] = 0.f;
        return;
    }
    const float *amb = p.am + (size_t)b * p.T * p.lda, *lmb = p.lm + (size_t)b * p.U1 * p.ldl;
    const int V = p.V;
    const int lc = tid & (SJ_VC - 1), lr = tid / SJ_VC;      // this thread's column and first row of a chunk load
    MaxSum acc{-INFINITY, 0.f};
    for (int v0 = 0; v0 < V; v0 += SJ_VC) {
        const bool col = v0 + lc < V;
#pragma unroll
        for (int i = 0; i < SJ_T; i += 256 / SJ_VC) {        // rows outside the lattice are not read
            const int r = lr + i;
            sa[r][lc] = (col && t0 + r < Tb) ? amb[(size_t)(t0 + r) * p.lda + v0 + lc] : 0.f;
            sl[r][lc] = (col && u0 + r <= Ub) ? lmb[(size_t)(u0 + r) * p.ldl + v0 + lc] : 0.f;
        }
        __syncthreads();
        if (inside) {
            const int n = V - v0 < SJ_VC ? V - v0 : SJ_VC;
            if (n == SJ_VC) {
#pragma unroll
                for (int j = 0; j < SJ_VC; j += 4)
                    ms_add4(acc, *reinterpret_cast<const f32x4 *>(&sa[ti][j]) +
                                     *reinterpret_cast<const f32x4 *>(&sl[ui][j]));
            } else {
                for (int j = 0; j < n; ++j) ms_add(acc, sa[ti][j] + sl[ui][j]);
            }
        }
        __syncthreads();
    }
    if (!in_tile) return;
    if (!inside) {
        lse_out[cell] = lpb[cell] = lpl[cell] = 0.f;
        return;
    }
    const float *ar = amb + (size_t)t * p.lda, *lr_ = lmb + (size_t)u * p.ldl;
    const float lse = acc.m + logf(acc.s);
    lse_out[cell] = lse;
    lpb[cell] = (ar[p.blank] + lr_[p.blank]) - lse;
    float l = 0.f;                      // u == U_b: no label
    if (u < Ub) {
        const int64_t y = p.txt[(int64_t)b * p.txt_stride + u];
        l = (y < 0 || y >= V) ? __builtin_nanf("") : (ar[y] + lr_[y]) - lse;
    }
    lpl[cell] = l;
}

// ---------------------------------------------------------------------------------------------
// simple joiner: occupation

__global__ __launch_bounds__(256) void rnnt_simple_occ_kernel(const float *__restrict__ lpb, const float *__restrict__ lpl,
                                                              const float *__restrict__ alpha,
                                                              const float *__restrict__ beta,
                                                              const float *__restrict__ nll,
                                                              const int64_t *__restrict__ enc_len,
                                                              const int64_t *__restrict__ txt_len, int T, int U1, int M,
                                                              float *__restrict__ c, float *__restrict__ eb,
                                                              float *__restrict__ el) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const int tu = T * U1, b = i / tu, r = i - b * tu, t = r / U1, u = r - t * U1;
    const int Tb = rnnt_clamp_T(enc_len[b], T), Ub = rnnt_clamp_U(txt_len[b], U1);
    if (!(t < Tb && u <= Ub)) {
        c[i] = eb[i] = el[i] = 0.f;
        return;
    }
    const size_t off = (size_t)b * tu;
    const RnntCoef k = rnnt_coef(t, u, Tb, Ub, U1, alpha + off, beta + off, lpb + off, lpl + off, nll[b]);
    c[i] = expf(k.c);
    eb[i] = k.eb;
    el[i] = k.el;
}

// ---------------------------------------------------------------------------------------------
// simple joiner: gradient.  OVER_T = false: dam[b,t,v], the kept rows are frames and u is reduced; true: dlm[b,u,v], the
// kept rows are label positions and t is reduced.  A thread owns column v of SG_R kept rows.

__device__ __forceinline__ int lab_of(int64_t y, int V) { return (y >= 0 && y < V) ? (int)y : -1; }   // a bad label matches no v

template <bool OVER_T>
__global__ __launch_bounds__(256) void rnnt_simple_grad_kernel(SimpleArgs p, const float *__restrict__ lse,
                                                               const float *__restrict__ c, const float *__restrict__ eb,
                                                               const float *__restrict__ el,
                                                               const float *__restrict__ gscale, float *__restrict__ out,
                                                               int64_t ldo) {
    const int b = blockIdx.z, r0 = blockIdx.y * SG_R, v = blockIdx.x * 256 + threadIdx.x;
    if (v >= p.V) return;
    const int T = p.T, U1 = p.U1;
    const int Tb = rnnt_clamp_T(p.enc_len[b], T), Ub = rnnt_clamp_U(p.txt_len[b], U1);
    const int n_kept = OVER_T ? U1 : T, n_valid = OVER_T ? Ub + 1 : Tb, n_red = OVER_T ? Tb : Ub + 1;
    const float *amb = p.am + (size_t)b * T * p.lda, *lmb = p.lm + (size_t)b * U1 * p.ldl;
    const float *kept = OVER_T ? lmb : amb, *red = OVER_T ? amb : lmb;
    const int64_t ldk = OVER_T ? p.ldl : p.lda, ldr = OVER_T ? p.lda : p.ldl;
    const int64_t *y = p.txt + (int64_t)b * p.txt_stride;
    const size_t off = (size_t)b * T * U1;
    float x[SG_R], acc[SG_R];
    int lab[SG_R];
#pragma unroll
    for (int i = 0; i < SG_R; ++i) {
        const int r = r0 + i;
        x[i] = r < n_valid ? kept[(size_t)r * ldk + v] : 0.f;      // a padded row is not read
        acc[i] = 0.f;
        lab[i] = (OVER_T && r < Ub) ? lab_of(y[r], p.V) : -1;
    }
    const bool isb = v == p.blank;
    for (int q = 0; q < n_red; ++q) {
        const float z = red[(size_t)q * ldr + v];
        const int labq = (!OVER_T && q < Ub) ? lab_of(y[q], p.V) : -1;
#pragma unroll
        for (int i = 0; i < SG_R; ++i) {
            const int r = r0 + i;
            if (r >= n_valid) continue;                            // uniform over the workgroup
            const size_t cell = off + (OVER_T ? (size_t)q * U1 + r : (size_t)r * U1 + q);
            float g = acc[i] + c[cell] * expf((OVER_T ? z + x[i] : x[i] + z) - lse[cell]);
            if (isb) g -= eb[cell];
            if (v == (OVER_T ? lab[i] : labq)) g -= el[cell];
            acc[i] = g;
        }
    }
    const float gs = gscale[b];
#pragma unroll
    for (int i = 0; i < SG_R; ++i) {
        const int r = r0 + i;
        if (r < n_kept) out[((size_t)b * n_kept + r) * ldo + v] = r < n_valid ? gs * acc[i] : 0.f;
    }
}

// ---------------------------------------------------------------------------------------------
// pruning bounds: one wave per utterance; lanes share the band starts of a frame, the scan over t is sequential

__global__ __launch_bounds__(64) void rnnt_prune_ranges_kernel(const float *__restrict__ occ,
                                                               const int64_t *__restrict__ enc_len,
                                                               const int64_t *__restrict__ txt_len, int T, int U1, int S,
                                                               int32_t *__restrict__ s_out) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int Tb = rnnt_clamp_T(enc_len[b], T), Ub = rnnt_clamp_U(txt_len[b], U1);
    const int E = rnntp_last_start(Ub, S);
    const float *ob = occ + (size_t)b * T * U1;
    int sp = 0, last = 0;
    for (int t = 0; t < T; ++t) {
        if (t < Tb) {
            float best = -INFINITY;
            int arg = -1;
            for (int s = lane; s <= E; s += 64) rnntp_better(rnntp_window(ob + (size_t)t * U1, s, S, Ub), s, &best, &arg);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ov = __shfl_xor(best, o, 64);
                const int oa = __shfl_xor(arg, o, 64);
                if (oa >= 0) rnntp_better(ov, oa, &best, &arg);
            }
            last = rnntp_step(arg < 0 ? 0 : arg, &sp, t, Tb, Ub, S);
        }
        if (lane == 0) s_out[(size_t)b * T + t] = last;
    }
}

// ---------------------------------------------------------------------------------------------
// band joint: row r = (b * T + t) * S + k reads label row min(s(t) + k, U1 - 1)

template <bool VEC>
__global__ __launch_bounds__(256) void rnnt_joint_band_kernel(const float *__restrict__ E, int64_t lde,
                                                              const float *__restrict__ P, int64_t ldp,
                                                              const int32_t *__restrict__ s, int T, int S, int U1, int J,
                                                              float *__restrict__ H, int64_t ldh, int64_t total) {
    const int per_row = VEC ? (J >> 2) : J;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / per_row;
        const int j = (int)(i - r * per_row);
        const int k = (int)(r % S);
        const int64_t bt = r / S;
        const int64_t b = bt / T;
        int u = rnntp_band_u(s[bt], k, U1);
        u = u > U1 - 1 ? U1 - 1 : u;
        const float *e = E + bt * lde;
        const float *q = P + (b * U1 + u) * ldp;
        float *h = H + r * ldh;
        if (VEC) {
            const f32x4 x = reinterpret_cast<const f32x4 *>(e)[j], y = reinterpret_cast<const f32x4 *>(q)[j];
            f32x4 o;
#pragma unroll
            for (int c = 0; c < 4; ++c) o[c] = tanhf(x[c] + y[c]);
            reinterpret_cast<f32x4 *>(h)[j] = o;
        } else {
            h[j] = tanhf(e[j] + q[j]);
        }
    }
}

// dE[b,t,:] = sum_k dH (1 - H^2), ascending k
__global__ __launch_bounds__(256) void rnnt_joint_band_bwd_e_kernel(const float *__restrict__ H, int64_t ldh,
                                                                    const float *__restrict__ dH, int64_t lddh, int S,
                                                                    int J, float *__restrict__ dE, int64_t ldde,
                                                                    int64_t total) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t bt = i / J;
        const int j = (int)(i - bt * J);
        float acc = 0.f;
        for (int k = 0; k < S; ++k) {
            const int64_t row = bt * S + k;
            const float h = H[row * ldh + j];
            acc += dH[row * lddh + j] * (1.f - h * h);
        }
        dE[bt * ldde + j] = acc;
    }
}

// dP[b,u,:] = sum over the (t, k) with min(s(t) + k, U1 - 1) == u of dH (1 - H^2), ascending t, then ascending k
__global__ __launch_bounds__(256) void rnnt_joint_band_bwd_p_kernel(const float *__restrict__ H, int64_t ldh,
                                                                    const float *__restrict__ dH, int64_t lddh,
                                                                    const int32_t *__restrict__ s, int T, int S, int U1,
                                                                    int J, float *__restrict__ dP, int64_t lddp,
                                                                    int64_t total) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t bu = i / J;
        const int j = (int)(i - bu * J);
        const int64_t b = bu / U1;
        const int u = (int)(bu - b * U1);
        float acc = 0.f;
        for (int t = 0; t < T; ++t) {
            const int k0 = u - rnntp_band_u(s[b * T + t], 0, U1);
            if (k0 >= S) continue;
            const int klo = k0 < 0 ? (u == U1 - 1 ? 0 : S) : k0;
            const int khi = u == U1 - 1 ? S - 1 : k0;          // the last row also stands for every clamped k
            for (int k = klo; k <= khi; ++k) {
                const int64_t row = (b * T + t) * S + k;
                const float h = H[row * ldh + j];
                acc += dH[row * lddh + j] * (1.f - h * h);
            }
        }
        dP[bu * lddp + j] = acc;
    }
}

static inline unsigned grid_for64(int64_t n, int block) {
    const int64_t g = (n + block - 1) / block;
    return (unsigned)(g > 65536 ? 65536 : (g < 1 ? 1 : g));
}

// ---------------------------------------------------------------------------------------------
// band loss: the row and gradient passes of rnnt.hip with the cell (t, k) standing for u = s(t) + k

struct BandArgs {
    const int64_t *txt;      // [B, txt_stride]
    int64_t txt_stride;
    const int64_t *enc_len, *txt_len;
    const int32_t *s;        // [B, T]
    int B, T, S, U1, V, blank;
};

__device__ __forceinline__ bool band_cell(const BandArgs &p, int row, int &b, int &t, int &u, int &Tb, int &Ub) {
    const int ts = p.T * p.S;
    b = row / ts;
    const int r = row - b * ts;
    t = r / p.S;
    const int k = r - t * p.S;
    Tb = rnnt_clamp_T(p.enc_len[b], p.T);
    Ub = rnnt_clamp_U(p.txt_len[b], p.U1);
    u = rnntp_band_u(p.s[(size_t)b * p.T + t], k, p.U1);
    return t < Tb && u <= Ub;
}

// the four waves' (max, sum) of a 256-thread workgroup -> thread 0
__device__ __forceinline__ MaxSum ms_block(MaxSum r, float *sm_m, float *sm_s) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (lane == 0) {
        sm_m[wave] = r.m;
        sm_s[wave] = r.s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const float Mx = fmaxf(fmaxf(sm_m[0], sm_m[1]), fmaxf(sm_m[2], sm_m[3]));
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (sm_m[k] > -INFINITY || sm_m[k] != sm_m[k]) s += sm_s[k] * expf(sm_m[k] - Mx);
        r = MaxSum{Mx, s};
    }
    return r;
}

// WG = false: one wave per row, 4 rows per workgroup; WG = true: one 256-thread workgroup per row
template <bool VEC, bool WG>
__global__ __launch_bounds__(256) void rnnt_rows_band_kernel(const float *__restrict__ z, int64_t ldz, BandArgs p, int M,
                                                             float *__restrict__ lse_out, float *__restrict__ lpb,
                                                             float *__restrict__ lpl) {
    __shared__ float sm_m[4], sm_s[4];
    const int row = WG ? (int)blockIdx.x : (int)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tid = WG ? (int)threadIdx.x : (int)(threadIdx.x & 63);
    if (row >= M) return;
    int b, t, u, Tb, Ub;
    if (!band_cell(p, row, b, t, u, Tb, Ub)) {   // uniform over the row's threads; the row is never read
        if (tid == 0) lse_out[row] = lpb[row] = lpl[row] = 0.f;
        return;
    }
    const float *zr = z + (size_t)row * ldz;
    MaxSum r = ms_wave(ms_row<VEC>(zr, p.V, tid, WG ? 256 : 64));
    if (WG) r = ms_block(r, sm_m, sm_s);
    if (tid == 0) {
        const float lse = r.m + logf(r.s);
        lse_out[row] = lse;
        lpb[row] = zr[p.blank] - lse;
        float l = 0.f;                 // u == U_b: no label
        if (u < Ub) {
            const int64_t y = p.txt[(int64_t)b * p.txt_stride + u];
            l = (y < 0 || y >= p.V) ? __builtin_nanf("") : zr[y] - lse;
        }
        lpl[row] = l;
    }
}

// dense [B,T,U1] lpb / lpl for the lattice: the band's values inside the band and the lattice, -inf elsewhere
__global__ __launch_bounds__(256) void rnnt_band_scatter_kernel(const float *__restrict__ lpb_band,
                                                                const float *__restrict__ lpl_band,
                                                                const int32_t *__restrict__ s,
                                                                const int64_t *__restrict__ enc_len,
                                                                const int64_t *__restrict__ txt_len, int T, int S, int U1,
                                                                int M, float *__restrict__ lpb, float *__restrict__ lpl) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const int bt = i / U1, u = i - bt * U1, b = bt / T, t = bt - b * T;
    const int Tb = rnnt_clamp_T(enc_len[b], T), Ub = rnnt_clamp_U(txt_len[b], U1);
    const int k = u - rnntp_band_u(s[bt], 0, U1);
    float vb = -INFINITY, vl = -INFINITY;
    if (t < Tb && u <= Ub && k >= 0 && k < S) {
        vb = lpb_band[(size_t)bt * S + k];
        vl = lpl_band[(size_t)bt * S + k];
    }
    lpb[i] = vb;
    lpl[i] = vl;
}

struct BandGradArgs {
    const float *lse;                           // [B, T, S]
    const float *lpb, *lpl, *alpha, *beta;      // dense [B, T, U1]
    const float *nll, *gscale;                  // [B]
};

// z and dz may be the same memory (the rule of rnnt_grad_kernel).  An utterance without a path (nll = +inf) gets zeros.
template <bool VEC, bool WG>
__global__ __launch_bounds__(256) void rnnt_grad_band_kernel(const float *z, int64_t ldz, BandArgs p, BandGradArgs a, int M,
                                                             float *dz, int64_t lddz) {
    const int row = WG ? (int)blockIdx.x : (int)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tid = WG ? (int)threadIdx.x : (int)(threadIdx.x & 63);
    constexpr int NT = WG ? 256 : 64;
    if (row >= M) return;
    const int V = p.V;
    float *dr = dz + (size_t)row * lddz;
    int b, t, u, Tb, Ub;
    const bool inside = band_cell(p, row, b, t, u, Tb, Ub);
    if (!inside || a.nll[b] == INFINITY) {      // exact zeros are WRITTEN, z is never read
        if (VEC) {
            const int nv = V >> 2;
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            for (int i = tid; i < nv; i += NT) reinterpret_cast<f32x4 *>(dr)[i] = zero;
            for (int i = (nv << 2) + tid; i < V; i += NT) dr[i] = 0.f;
        } else {
            for (int i = tid; i < V; i += NT) dr[i] = 0.f;
        }
        return;
    }
    const size_t off = (size_t)b * p.T * p.U1;
    const RnntCoef k = rnnt_coef(t, u, Tb, Ub, p.U1, a.alpha + off, a.beta + off, a.lpb + off, a.lpl + off, a.nll[b]);
    const float lse = a.lse[row], gs = a.gscale[b];
    int lab = -1;
    if (u < Ub) {
        const int64_t y = p.txt[(int64_t)b * p.txt_stride + u];
        if (y >= 0 && y < V) lab = (int)y;
    }
    const int bl = p.blank;
    const float *zr = z + (size_t)row * ldz;
    if (VEC) {
        const int nv = V >> 2;
#pragma unroll 4
        for (int i = tid; i < nv; i += NT) {
            const f32x4 v = reinterpret_cast<const f32x4 *>(zr)[i];
            const int c = i << 2;
            f32x4 o;
            o[0] = grad_value(v[0], lse, k, gs, c == bl, c == lab);
            o[1] = grad_value(v[1], lse, k, gs, c + 1 == bl, c + 1 == lab);
            o[2] = grad_value(v[2], lse, k, gs, c + 2 == bl, c + 2 == lab);
            o[3] = grad_value(v[3], lse, k, gs, c + 3 == bl, c + 3 == lab);
            reinterpret_cast<f32x4 *>(dr)[i] = o;
        }
        for (int i = (nv << 2) + tid; i < V; i += NT) dr[i] = grad_value(zr[i], lse, k, gs, i == bl, i == lab);
    } else {
#pragma unroll 4
        for (int i = tid; i < V; i += NT) dr[i] = grad_value(zr[i], lse, k, gs, i == bl, i == lab);
    }
}

static inline bool fits31(int64_t n) { return n <= (int64_t)INT32_MAX; }

static int simple_check(int64_t lda, int64_t ldl, int64_t txt_stride, int B, int T, int U1, int V, int blank) {
    if (B < 0 || T <= 0 || U1 <= 0 || V <= 0 || lda < V || ldl < V || blank < 0 || blank >= V) return ASRK_EINVAL;
    if (txt_stride < U1 - 1) return ASRK_EINVAL;
    if (!fits31((int64_t)B * T * U1) || B > 65535 || asrk_div_up(T, SG_R) > 65535 || asrk_div_up(U1, SG_R) > 65535)
        return ASRK_ESHAPE;
    return ASRK_OK;
}

static int band_check(int64_t ldz, int64_t txt_stride, int B, int T, int S, int U1, int V, int blank) {
    if (B < 0 || T <= 0 || U1 <= 0 || V <= 0 || ldz < V || blank < 0 || blank >= V) return ASRK_EINVAL;
    if (S < 1 || S > PRUNE_MAX_S || txt_stride < U1 - 1) return ASRK_EINVAL;
    if (!fits31((int64_t)B * T * S) || !fits31((int64_t)B * T * U1)) return ASRK_ESHAPE;
    return ASRK_OK;
}

}  // namespace

extern "C" int asrk_rnnt_simple_rows_f32(const float *am, int64_t lda, const float *lm, int64_t ldl, const int64_t *txt,
                                         int64_t txt_stride, const int64_t *enc_len, const int64_t *txt_len, int B, int T,
                                         int U1, int V, int blank, float *lse, float *lpb, float *lpl, void *stream) {
    const int rc = simple_check(lda, ldl, txt_stride, B, T, U1, V, blank);
    if (rc != ASRK_OK) return rc;
    if (B == 0) return ASRK_OK;
    if (!am || !lm || !enc_len || !txt_len || !lse || !lpb || !lpl || (U1 > 1 && !txt)) return ASRK_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const SimpleArgs p{am, lda, lm, ldl, txt, txt_stride, enc_len, txt_len, B, T, U1, V, blank};
    asrk_prof_begin_(PROF_ROWOPS, s);
    hipLaunchKernelGGL(rnnt_simple_rows_kernel, dim3(asrk_div_up(U1, SJ_U), asrk_div_up(T, SJ_T), B), dim3(256), 0, s, p,
                       lse, lpb, lpl);
    asrk_prof_end_(PROF_ROWOPS, s);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}

extern "C" int asrk_rnnt_simple_occ_f32(const float *lpb, const float *lpl, const float *alpha, const float *beta,
                                        const float *nll, const int64_t *enc_len, const int64_t *txt_len, int B, int T,
                                        int U1, float *c, float *eb, float *el, void *stream) {
    if (B < 0 || T <= 0 || U1 <= 0) return ASRK_EINVAL;
    if (!fits31((int64_t)B * T * U1)) return ASRK_ESHAPE;
    if (B == 0) return ASRK_OK;
    if (!lpb || !lpl || !alpha || !beta || !nll || !enc_len || !txt_len || !c || !eb || !el) return ASRK_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int M = B * T * U1;
    asrk_prof_begin_(PROF_ROWOPS, s);
    hipLaunchKernelGGL(rnnt_simple_occ_kernel, dim3(asrk_div_up(M, 256)), dim3(256), 0, s, lpb, lpl, alpha, beta, nll,
                       enc_len, txt_len, T, U1, M, c, eb, el);
    asrk_prof_end_(PROF_ROWOPS, s);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}

extern "C" int asrk_rnnt_simple_grad_f32(const float *am, int64_t lda, const float *lm, int64_t ldl, const int64_t *txt,
                                         int64_t txt_stride, const int64_t *enc_len, const int64_t *txt_len, int B, int T,
                                         int U1, int V, int blank, const float *lse, const float *c, const float *eb,
                                         const float *el, const float *gscale, float *dam, int64_t lddam, float *dlm,
                                         int64_t lddlm, void *stream) {
    const int rc = simple_check(lda, ldl, txt_stride, B, T, U1, V, blank);
    if (rc != ASRK_OK) return rc;
    if (lddam < V || lddlm < V) return ASRK_EINVAL;
    if (B == 0) return ASRK_OK;
    if (!am || !lm || !enc_len || !txt_len || !lse || !c || !eb || !el || !gscale || !dam || !dlm || (U1 > 1 && !txt))
        return ASRK_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const SimpleArgs p{am, lda, lm, ldl, txt, txt_stride, enc_len, txt_len, B, T, U1, V, blank};
    const int gv = asrk_div_up(V, 256);
    asrk_prof_begin_(PROF_ROWOPS, s);
    hipLaunchKernelGGL((rnnt_simple_grad_kernel<false>), dim3(gv, asrk_div_up(T, SG_R), B), dim3(256), 0, s, p, lse, c, eb,
                       el, gscale, dam, lddam);
    hipLaunchKernelGGL((rnnt_simple_grad_kernel<true>), dim3(gv, asrk_div_up(U1, SG_R), B), dim3(256), 0, s, p, lse, c, eb,
                       el, gscale, dlm, lddlm);
    asrk_prof_end_(PROF_ROWOPS, s);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}

extern "C" int asrk_rnnt_prune_ranges_f32(const float *occ, const int64_t *enc_len, const int64_t *txt_len, int B, int T,
                                          int U1, int S, int32_t *s_out, void *stream) {
    if (B < 0 || T <= 0 || U1 <= 0 || S < 1 || S > PRUNE_MAX_S) return ASRK_EINVAL;
    if (!fits31((int64_t)B * T * U1)) return ASRK_ESHAPE;
    if (B == 0) return ASRK_OK;
    if (!occ || !enc_len || !txt_len || !s_out) return ASRK_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    asrk_prof_begin_(PROF_CTC, s);
    hipLaunchKernelGGL(rnnt_prune_ranges_kernel, dim3(B), dim3(64), 0, s, occ, enc_len, txt_len, T, U1, S, s_out);
    asrk_prof_end_(PROF_CTC, s);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}

extern "C" int asrk_rnnt_joint_band_f32(const float *E, int64_t lde, const float *P, int64_t ldp, const int32_t *s_band,
                                        int B, int T, int S, int U1, int J, float *H, int64_t ldh, void *stream) {
    if (B < 0 || T <= 0 || U1 <= 0 || J <= 0 || S < 1 || S > PRUNE_MAX_S || lde < J || ldp < J || ldh < J)
        return ASRK_EINVAL;
    if (B == 0) return ASRK_OK;
    if (!E || !P || !s_band || !H) return ASRK_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const bool vec = al16(E) && al16(P) && al16(H) && J % 4 == 0 && lde % 4 == 0 && ldp % 4 == 0 && ldh % 4 == 0;
    const int64_t total = (int64_t)B * T * S * (vec ? J / 4 : J);
    asrk_prof_begin_(PROF_ROWOPS, s);
    if (vec)
        hipLaunchKernelGGL((rnnt_joint_band_kernel<true>), dim3(grid_for64(total, 256)), dim3(256), 0, s, E, lde, P, ldp,
                           s_band, T, S, U1, J, H, ldh, total);
    else
        hipLaunchKernelGGL((rnnt_joint_band_kernel<false>), dim3(grid_for64(total, 256)), dim3(256), 0, s, E, lde, P, ldp,
                           s_band, T, S, U1, J, H, ldh, total);
    asrk_prof_end_(PROF_ROWOPS, s);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}

extern "C" int asrk_rnnt_joint_band_bwd_f32(const float *H, int64_t ldh, const float *dH, int64_t lddh,
                                            const int32_t *s_band, int B, int T, int S, int U1, int J, float *dE,
                                            int64_t ldde, float *dP, int64_t lddp, void *stream) {
    if (B < 0 || T <= 0 || U1 <= 0 || J <= 0 || S < 1 || S > PRUNE_MAX_S || ldh < J || lddh < J || ldde < J || lddp < J)
        return ASRK_EINVAL;
    if (B == 0) return ASRK_OK;
    if (!H || !dH || !s_band || !dE || !dP) return ASRK_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int64_t nE = (int64_t)B * T * J, nP = (int64_t)B * U1 * J;
    asrk_prof_begin_(PROF_ROWOPS, s);
    hipLaunchKernelGGL(rnnt_joint_band_bwd_e_kernel, dim3(grid_for64(nE, 256)), dim3(256), 0, s, H, ldh, dH, lddh, S, J, dE,
                       ldde, nE);
    hipLaunchKernelGGL(rnnt_joint_band_bwd_p_kernel, dim3(grid_for64(nP, 256)), dim3(256), 0, s, H, ldh, dH, lddh, s_band,
                       T, S, U1, J, dP, lddp, nP);
    asrk_prof_end_(PROF_ROWOPS, s);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}

extern "C" int asrk_rnnt_rows_band_f32(const float *z, int64_t ldz, const int64_t *txt, int64_t txt_stride,
                                       const int64_t *enc_len, const int64_t *txt_len, const int32_t *s_band, int B, int T,
                                       int S, int U1, int V, int blank, float *lse, float *lpb, float *lpl, void *stream) {
    const int rc = band_check(ldz, txt_stride, B, T, S, U1, V, blank);
    if (rc != ASRK_OK) return rc;
    if (B == 0) return ASRK_OK;
    if (!z || !enc_len || !txt_len || !s_band || !lse || !lpb || !lpl || (U1 > 1 && !txt)) return ASRK_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int M = B * T * S;
    const BandArgs p{txt, txt_stride, enc_len, txt_len, s_band, B, T, S, U1, V, blank};
    const bool vec = al16(z) && (ldz % 4 == 0);
    asrk_prof_begin_(PROF_ROWOPS, s);
    if (V >= RNNT_WG_MIN_V) {
        if (vec)
            hipLaunchKernelGGL((rnnt_rows_band_kernel<true, true>), dim3(M), dim3(256), 0, s, z, ldz, p, M, lse, lpb, lpl);
        else
            hipLaunchKernelGGL((rnnt_rows_band_kernel<false, true>), dim3(M), dim3(256), 0, s, z, ldz, p, M, lse, lpb, lpl);
    } else {
        const unsigned grid = (unsigned)asrk_div_up(M, 4);
        if (vec)
            hipLaunchKernelGGL((rnnt_rows_band_kernel<true, false>), dim3(grid), dim3(256), 0, s, z, ldz, p, M, lse, lpb,
                               lpl);
        else
            hipLaunchKernelGGL((rnnt_rows_band_kernel<false, false>), dim3(grid), dim3(256), 0, s, z, ldz, p, M, lse, lpb,
                               lpl);
    }
    asrk_prof_end_(PROF_ROWOPS, s);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}

extern "C" int asrk_rnnt_band_scatter_f32(const float *lpb_band, const float *lpl_band, const int32_t *s_band,
                                          const int64_t *enc_len, const int64_t *txt_len, int B, int T, int S, int U1,
                                          float *lpb, float *lpl, void *stream) {
    if (B < 0 || T <= 0 || U1 <= 0 || S < 1 || S > PRUNE_MAX_S) return ASRK_EINVAL;
    if (!fits31((int64_t)B * T * S) || !fits31((int64_t)B * T * U1)) return ASRK_ESHAPE;
    if (B == 0) return ASRK_OK;
    if (!lpb_band || !lpl_band || !s_band || !enc_len || !txt_len || !lpb || !lpl) return ASRK_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int M = B * T * U1;
    asrk_prof_begin_(PROF_ROWOPS, s);
    hipLaunchKernelGGL(rnnt_band_scatter_kernel, dim3(asrk_div_up(M, 256)), dim3(256), 0, s, lpb_band, lpl_band, s_band,
                       enc_len, txt_len, T, S, U1, M, lpb, lpl);
    asrk_prof_end_(PROF_ROWOPS, s);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}

extern "C" int asrk_rnnt_grad_band_f32(const float *z, int64_t ldz, const int64_t *txt, int64_t txt_stride,
                                       const int64_t *enc_len, const int64_t *txt_len, const int32_t *s_band, int B, int T,
                                       int S, int U1, int V, int blank, const float *lse, const float *lpb,
                                       const float *lpl, const float *alpha, const float *beta, const float *nll,
                                       const float *gscale, float *dz, int64_t lddz, void *stream) {
    const int rc = band_check(ldz, txt_stride, B, T, S, U1, V, blank);
    if (rc != ASRK_OK) return rc;
    if (lddz < V) return ASRK_EINVAL;
    if (B == 0) return ASRK_OK;
    if (!z || !enc_len || !txt_len || !s_band || !lse || !lpb || !lpl || !alpha || !beta || !nll || !gscale || !dz ||
        (U1 > 1 && !txt))
        return ASRK_EINVAL;
    if (dz == z && lddz != ldz) return ASRK_EINVAL;   // in place means element for element
    hipStream_t s = (hipStream_t)stream;
    const int M = B * T * S;
    const BandArgs p{txt, txt_stride, enc_len, txt_len, s_band, B, T, S, U1, V, blank};
    const BandGradArgs a{lse, lpb, lpl, alpha, beta, nll, gscale};
    const bool vec = al16(z) && al16(dz) && (ldz % 4 == 0) && (lddz % 4 == 0);
    asrk_prof_begin_(PROF_ROWOPS, s);
    if (V >= RNNT_WG_MIN_V) {
        if (vec)
            hipLaunchKernelGGL((rnnt_grad_band_kernel<true, true>), dim3(M), dim3(256), 0, s, z, ldz, p, a, M, dz, lddz);
        else
            hipLaunchKernelGGL((rnnt_grad_band_kernel<false, true>), dim3(M), dim3(256), 0, s, z, ldz, p, a, M, dz, lddz);
    } else {
        const unsigned grid = (unsigned)asrk_div_up(M, 4);
        if (vec)
            hipLaunchKernelGGL((rnnt_grad_band_kernel<true, false>), dim3(grid), dim3(256), 0, s, z, ldz, p, a, M, dz,
                               lddz);
        else
            hipLaunchKernelGGL((rnnt_grad_band_kernel<false, false>), dim3(grid), dim3(256), 0, s, z, ldz, p, a, M, dz,
                               lddz);
    }
    asrk_prof_end_(PROF_ROWOPS, s);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}
