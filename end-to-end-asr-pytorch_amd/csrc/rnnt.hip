// RNN-transducer head for gfx950 (src/transducer.py): joint network, fused loss, greedy decoding step.
//
//   asrk_rnnt_joint_f32        H[b,t,u,:] = tanh(E[b,t,:] + P[b,u,:]); with t_idx the decode form, one frame per row b.
//   asrk_rnnt_joint_bwd_f32    dE = sum_u dH (1 - H^2), dP = sum_t dH (1 - H^2): every sum inside one thread, in index order.
//   asrk_rnnt_rows_f32         first read of the [B*T*(U+1), V] logits: per row the log-sum-exp and the log-probabilities
//                              of blank and of the row's label (txt[b, u]); rows outside the lattice are never read.
//   asrk_rnnt_lattice_f32      alpha and beta over anti-diagonals, one workgroup per utterance, both directions in one
//                              launch (as ctc.hip); the previous diagonal stays in LDS.  The walk itself: rnnt.inc.
//   asrk_rnnt_grad_f32         second and last read of the logits: the closed-form gradient, in place or out of place.
//   asrk_rnnt_greedy_step_f32  argmax per row and the device-resident bookkeeping of the lock-step greedy search.
//
// The logits are read twice and written once; no [M, V] log_softmax exists at any time.  wave64, no float atomics:
// every result is a pure function of its inputs, reproducible bit for bit.
#include "rnnt_rows.h"

namespace {

constexpr int RNNT_LAT_THREADS = 128;   // lanes per direction of the lattice walk
constexpr int RNNT_MAX_U1 = 2048;       // 4 diagonals of U1 floats in LDS: 32 KiB

// row m = (b * T + t) * U1 + u of utterance b; false: the cell lies outside the utterance's lattice
struct RowArgs {
    const int64_t *txt;      // [B, txt_stride]
    int64_t txt_stride;
    const int64_t *enc_len;  // [B]
    const int64_t *txt_len;  // [B]
    int B, T, U1, V, blank;
};

__device__ __forceinline__ bool row_cell(const RowArgs &p, int row, int &b, int &t, int &u, int &Tb, int &Ub) {
    const int tu = p.T * p.U1;
    b = row / tu;
    const int r = row - b * tu;
    t = r / p.U1;
    u = r - t * p.U1;
    Tb = rnnt_clamp_T(p.enc_len[b], p.T);
    Ub = rnnt_clamp_U(p.txt_len[b], p.U1);
    return t < Tb && u <= Ub;
}

// WG = false: one wave per row, 4 rows per workgroup; WG = true: one 256-thread workgroup per row
template <bool VEC, bool WG>
__global__ __launch_bounds__(256) void rnnt_rows_kernel(const float *__restrict__ z, int64_t ldz, RowArgs p, int M,
                                                        float *__restrict__ lse_out, float *__restrict__ lpb,
                                                        float *__restrict__ lpl) {
    __shared__ float sm_m[4], sm_s[4];
    const int row = WG ? (int)blockIdx.x : (int)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tid = WG ? (int)threadIdx.x : (int)(threadIdx.x & 63);
    if (row >= M) return;
    int b, t, u, Tb, Ub;
    if (!row_cell(p, row, b, t, u, Tb, Ub)) {   // uniform over the row's threads; the row is never read
        if (tid == 0) {
            lse_out[row] = 0.f;
            lpb[row] = 0.f;
            lpl[row] = 0.f;
        }
        return;
    }
    const float *zr = z + (size_t)row * ldz;
    MaxSum r = ms_wave(ms_row<VEC>(zr, p.V, tid, WG ? 256 : 64));
    if (WG) {
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
    }
    if (tid == 0) {
        const float lse = r.m + logf(r.s);
        lse_out[row] = lse;
        lpb[row] = zr[p.blank] - lse;
        float l = 0.f;                 // u == U_b: no label
        if (u < Ub) {
            const int64_t y = p.txt[(int64_t)b * p.txt_stride + u];
            l = (y < 0 || y >= p.V) ? __builtin_nanf("") : zr[y] - lse;   // a bad label: NaN, nothing read
        }
        lpl[row] = l;
    }
}

// ---------------------------------------------------------------------------------------------
// lattice

struct BlockSync {
    __device__ __forceinline__ void operator()() const { __syncthreads(); }
};

// blockDim.x = 128 (alpha only) or 256 (threads 128.. walk beta)
__global__ __launch_bounds__(2 * RNNT_LAT_THREADS) void rnnt_lattice_kernel(
    const float *__restrict__ lpb, const float *__restrict__ lpl, const int64_t *__restrict__ enc_len,
    const int64_t *__restrict__ txt_len, int T, int U1, float *__restrict__ alpha, float *__restrict__ beta,
    float *__restrict__ nll) {
    extern __shared__ float diag[];   // [2 directions][2][U1]
    const int b = blockIdx.x;
    const int dir = __builtin_amdgcn_readfirstlane(threadIdx.x >= RNNT_LAT_THREADS ? 1 : 0);
    const int tid = threadIdx.x - dir * RNNT_LAT_THREADS;
    const int Tb = rnnt_clamp_T(enc_len[b], T), Ub = rnnt_clamp_U(txt_len[b], U1);
    const size_t off = (size_t)b * T * U1;
    rnnt_walk(dir, tid, RNNT_LAT_THREADS, Tb, Ub, U1, lpb + off, lpl + off, (dir ? beta : alpha) + off,
              diag + (size_t)dir * 2 * U1, nll + b, BlockSync());
}

// ---------------------------------------------------------------------------------------------
// gradient

struct GradArgs {
    const float *lse, *lpb, *lpl, *alpha, *beta, *nll, *gscale;
};

// z and dz may be the same memory: a thread reads an element (or a 16-byte group) and then writes that very element;
// the blank's and the label's log-probabilities come from the row pass, never from the row being overwritten
template <bool VEC, bool WG>
__global__ __launch_bounds__(256) void rnnt_grad_kernel(const float *z, int64_t ldz, RowArgs p, GradArgs a, int M,
                                                        float *dz, int64_t lddz) {
    const int row = WG ? (int)blockIdx.x : (int)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tid = WG ? (int)threadIdx.x : (int)(threadIdx.x & 63);
    constexpr int NT = WG ? 256 : 64;
    if (row >= M) return;
    const int V = p.V;
    float *dr = dz + (size_t)row * lddz;
    int b, t, u, Tb, Ub;
    if (!row_cell(p, row, b, t, u, Tb, Ub)) {   // a padded cell: exact zeros are WRITTEN, z is never read
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
        if (y >= 0 && y < V) lab = (int)y;   // a bad label made the forward NaN; k.el is NaN then and goes nowhere
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

// ---------------------------------------------------------------------------------------------
// joint network

// one thread per output element (VEC: per 16-byte group); row r = (b * To + to) * U1 + u, To = 1 with t_idx
template <bool VEC>
__global__ __launch_bounds__(256) void rnnt_joint_kernel(const float *__restrict__ E, int64_t lde,
                                                         const float *__restrict__ P, int64_t ldp,
                                                         const int32_t *__restrict__ t_idx, int T, int To, int U1, int J,
                                                         float *__restrict__ H, int64_t ldh, int64_t total) {
    const int per_row = VEC ? (J >> 2) : J;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / per_row;
        const int j = (int)(i - r * per_row);
        const int u = (int)(r % U1);
        const int64_t bt = r / U1;
        const int b = (int)(bt / To);
        int t = (int)(bt - (int64_t)b * To);
        if (t_idx) {
            t = t_idx[b];
            t = t < 0 ? 0 : (t > T - 1 ? T - 1 : t);   // a finished row points one past its last frame
        }
        const float *e = E + ((int64_t)b * T + t) * lde;
        const float *q = P + ((int64_t)b * U1 + u) * ldp;
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

// OVER_T = false: dE[b,t,:] = sum over u; true: dP[b,u,:] = sum over t.  One thread owns an output element (VEC: four)
// and adds its n terms in ascending index order.
template <bool VEC, bool OVER_T>
__global__ __launch_bounds__(256) void rnnt_joint_bwd_kernel(const float *__restrict__ H, int64_t ldh,
                                                             const float *__restrict__ dH, int64_t lddh, int T, int U1,
                                                             int J, float *__restrict__ out, int64_t ldo,
                                                             int64_t total) {
    const int per_row = VEC ? (J >> 2) : J;
    const int rows_per_b = OVER_T ? U1 : T;
    const int n = OVER_T ? T : U1;
    const int64_t step = OVER_T ? U1 : 1;   // in rows of H
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / per_row;       // b * rows_per_b + (t or u)
        const int j = (int)(i - r * per_row);
        const int64_t b = r / rows_per_b;
        const int64_t k = r - b * rows_per_b;
        const int64_t row0 = OVER_T ? b * T * U1 + k : (b * T + k) * U1;
        if (VEC) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            for (int s = 0; s < n; ++s) {
                const int64_t row = row0 + s * step;
                const f32x4 h = reinterpret_cast<const f32x4 *>(H + row * ldh)[j];
                const f32x4 g = reinterpret_cast<const f32x4 *>(dH + row * lddh)[j];
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[c] += g[c] * (1.f - h[c] * h[c]);
            }
            reinterpret_cast<f32x4 *>(out + r * ldo)[j] = acc;
        } else {
            float acc = 0.f;
            for (int s = 0; s < n; ++s) {
                const int64_t row = row0 + s * step;
                const float h = H[row * ldh + j];
                acc += dH[row * lddh + j] * (1.f - h * h);
            }
            out[r * ldo + j] = acc;
        }
    }
}

static inline unsigned grid_for64(int64_t n, int block) {
    const int64_t g = (n + block - 1) / block;
    return (unsigned)(g > 65536 ? 65536 : (g < 1 ? 1 : g));
}

// ---------------------------------------------------------------------------------------------
// greedy step: one wave per row, 4 rows per workgroup

__global__ __launch_bounds__(256) void rnnt_greedy_step_kernel(const float *__restrict__ x, int64_t ldx,
                                                               const int64_t *__restrict__ enc_len, int B, int T, int V,
                                                               int blank, int max_symbols, int max_len,
                                                               int32_t *__restrict__ t_ptr, int32_t *__restrict__ n_sym,
                                                               int32_t *__restrict__ n_tok, int64_t *__restrict__ tokens,
                                                               int64_t tok_stride, int64_t *__restrict__ last_tok,
                                                               int32_t *__restrict__ emit, int32_t *__restrict__ done) {
    const int b = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (b >= B) return;
    if (done[b]) {                       // a finished row: nothing is read, nothing moves
        if (lane == 0) emit[b] = 0;
        return;
    }
    const float *xr = x + (size_t)b * ldx;
    float best = -INFINITY;
    int arg = V;                         // a lane without a candidate loses every comparison
    for (int i = lane; i < V; i += 64) {
        const float v = xr[i];
        if (v > best || arg == V) {      // ascending i inside a lane: the first of equal values stays
            best = v;
            arg = i;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oa = __shfl_xor(arg, o, 64);
        if (oa < V && (arg == V || ov > best || (ov == best && oa < arg))) {
            best = ov;
            arg = oa;
        }
    }
    if (lane != 0) return;
    const int Tb = rnnt_clamp_T(enc_len[b], T);
    const int ns = n_sym[b], nt = n_tok[b];
    if (arg == blank || ns >= max_symbols || nt >= max_len || nt < 0) {   // (nt < 0: damaged state writes nothing)
        const int t = t_ptr[b] + 1;
        t_ptr[b] = t;
        n_sym[b] = 0;
        emit[b] = 0;
        if (t >= Tb) done[b] = 1;
    } else {
        tokens[(int64_t)b * tok_stride + nt] = arg;
        n_tok[b] = nt + 1;
        n_sym[b] = ns + 1;
        last_tok[b] = arg;
        emit[b] = 1;
    }
}

static inline bool rows_fit(int B, int T, int U1) { return (int64_t)B * T * U1 <= (int64_t)INT32_MAX; }

}  // namespace

extern "C" int asrk_rnnt_joint_f32(const float *E, int64_t lde, const float *P, int64_t ldp, const int32_t *t_idx, int B,
                                   int T, int U1, int J, float *H, int64_t ldh, void *stream) {
    if (B < 0 || T <= 0 || U1 <= 0 || J <= 0 || lde < J || ldp < J || ldh < J) return ASRK_EINVAL;
    if (B == 0) return ASRK_OK;
    if (!E || !P || !H) return ASRK_EINVAL;
    const int To = t_idx ? 1 : T;
    hipStream_t s = (hipStream_t)stream;
    const bool vec = al16(E) && al16(P) && al16(H) && J % 4 == 0 && lde % 4 == 0 && ldp % 4 == 0 && ldh % 4 == 0;
    const int64_t total = (int64_t)B * To * U1 * (vec ? J / 4 : J);
    asrk_prof_begin_(PROF_ROWOPS, s);
    if (vec)
        hipLaunchKernelGGL((rnnt_joint_kernel<true>), dim3(grid_for64(total, 256)), dim3(256), 0, s, E, lde, P, ldp,
                           t_idx, T, To, U1, J, H, ldh, total);
    else
        hipLaunchKernelGGL((rnnt_joint_kernel<false>), dim3(grid_for64(total, 256)), dim3(256), 0, s, E, lde, P, ldp,
                           t_idx, T, To, U1, J, H, ldh, total);
    asrk_prof_end_(PROF_ROWOPS, s);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}

extern "C" int asrk_rnnt_joint_bwd_f32(const float *H, int64_t ldh, const float *dH, int64_t lddh, int B, int T, int U1,
                                       int J, float *dE, int64_t ldde, float *dP, int64_t lddp, void *stream) {
    if (B < 0 || T <= 0 || U1 <= 0 || J <= 0 || ldh < J || lddh < J || ldde < J || lddp < J) return ASRK_EINVAL;
    if (B == 0) return ASRK_OK;
    if (!H || !dH || !dE || !dP) return ASRK_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const bool vec = al16(H) && al16(dH) && al16(dE) && al16(dP) && J % 4 == 0 && ldh % 4 == 0 && lddh % 4 == 0 &&
                     ldde % 4 == 0 && lddp % 4 == 0;
    const int per_row = vec ? J / 4 : J;
    const int64_t nE = (int64_t)B * T * per_row, nP = (int64_t)B * U1 * per_row;
    asrk_prof_begin_(PROF_ROWOPS, s);
    if (vec) {
        hipLaunchKernelGGL((rnnt_joint_bwd_kernel<true, false>), dim3(grid_for64(nE, 256)), dim3(256), 0, s, H, ldh, dH,
                           lddh, T, U1, J, dE, ldde, nE);
        hipLaunchKernelGGL((rnnt_joint_bwd_kernel<true, true>), dim3(grid_for64(nP, 256)), dim3(256), 0, s, H, ldh, dH,
                           lddh, T, U1, J, dP, lddp, nP);
    } else {
        hipLaunchKernelGGL((rnnt_joint_bwd_kernel<false, false>), dim3(grid_for64(nE, 256)), dim3(256), 0, s, H, ldh, dH,
                           lddh, T, U1, J, dE, ldde, nE);
        hipLaunchKernelGGL((rnnt_joint_bwd_kernel<false, true>), dim3(grid_for64(nP, 256)), dim3(256), 0, s, H, ldh, dH,
                           lddh, T, U1, J, dP, lddp, nP);
    }
    asrk_prof_end_(PROF_ROWOPS, s);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}

static int rnnt_shape_check(int64_t ldz, int64_t txt_stride, int B, int T, int U1, int V, int blank) {
    if (B < 0 || T <= 0 || U1 <= 0 || V <= 0 || ldz < V || blank < 0 || blank >= V) return ASRK_EINVAL;
    if (txt_stride < U1 - 1) return ASRK_EINVAL;
    if (!rows_fit(B, T, U1)) return ASRK_ESHAPE;
    return ASRK_OK;
}

extern "C" int asrk_rnnt_rows_f32(const float *z, int64_t ldz, const int64_t *txt, int64_t txt_stride,
                                  const int64_t *enc_len, const int64_t *txt_len, int B, int T, int U1, int V, int blank,
                                  float *lse, float *lpb, float *lpl, void *stream) {
    const int rc = rnnt_shape_check(ldz, txt_stride, B, T, U1, V, blank);
    if (rc != ASRK_OK) return rc;
    if (B == 0) return ASRK_OK;
    if (!z || !enc_len || !txt_len || !lse || !lpb || !lpl || (U1 > 1 && !txt)) return ASRK_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int M = B * T * U1;
    const RowArgs p{txt, txt_stride, enc_len, txt_len, B, T, U1, V, blank};
    const bool vec = al16(z) && (ldz % 4 == 0);
    asrk_prof_begin_(PROF_ROWOPS, s);
    if (V >= RNNT_WG_MIN_V) {
        if (vec)
            hipLaunchKernelGGL((rnnt_rows_kernel<true, true>), dim3(M), dim3(256), 0, s, z, ldz, p, M, lse, lpb, lpl);
        else
            hipLaunchKernelGGL((rnnt_rows_kernel<false, true>), dim3(M), dim3(256), 0, s, z, ldz, p, M, lse, lpb, lpl);
    } else {
        const unsigned grid = (unsigned)asrk_div_up(M, 4);
        if (vec)
            hipLaunchKernelGGL((rnnt_rows_kernel<true, false>), dim3(grid), dim3(256), 0, s, z, ldz, p, M, lse, lpb,
                               lpl);
        else
            hipLaunchKernelGGL((rnnt_rows_kernel<false, false>), dim3(grid), dim3(256), 0, s, z, ldz, p, M, lse, lpb,
                               lpl);
    }
    asrk_prof_end_(PROF_ROWOPS, s);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}

extern "C" int asrk_rnnt_lattice_f32(const float *lpb, const float *lpl, const int64_t *enc_len, const int64_t *txt_len,
                                     int B, int T, int U1, float *alpha, float *beta, float *nll, void *stream) {
    if (B < 0 || T <= 0 || U1 <= 0) return ASRK_EINVAL;
    if (!rows_fit(B, T, U1) || U1 > RNNT_MAX_U1) return ASRK_ESHAPE;
    if (B == 0) return ASRK_OK;
    if (!lpb || !lpl || !enc_len || !txt_len || !alpha || !nll) return ASRK_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const size_t lds = 4 * (size_t)U1 * sizeof(float);
    asrk_prof_begin_(PROF_CTC, s);   // the lattice family
    hipLaunchKernelGGL(rnnt_lattice_kernel, dim3(B), dim3(beta ? 2 * RNNT_LAT_THREADS : RNNT_LAT_THREADS), lds, s, lpb,
                       lpl, enc_len, txt_len, T, U1, alpha, beta, nll);
    asrk_prof_end_(PROF_CTC, s);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}

extern "C" int asrk_rnnt_grad_f32(const float *z, int64_t ldz, const int64_t *txt, int64_t txt_stride,
                                  const int64_t *enc_len, const int64_t *txt_len, int B, int T, int U1, int V, int blank,
                                  const float *lse, const float *lpb, const float *lpl, const float *alpha,
                                  const float *beta, const float *nll, const float *gscale, float *dz, int64_t lddz,
                                  void *stream) {
    const int rc = rnnt_shape_check(ldz, txt_stride, B, T, U1, V, blank);
    if (rc != ASRK_OK) return rc;
    if (lddz < V) return ASRK_EINVAL;
    if (B == 0) return ASRK_OK;
    if (!z || !enc_len || !txt_len || !lse || !lpb || !lpl || !alpha || !beta || !nll || !gscale || !dz ||
        (U1 > 1 && !txt))
        return ASRK_EINVAL;
    if (dz == z && lddz != ldz) return ASRK_EINVAL;   // in place means element for element
    hipStream_t s = (hipStream_t)stream;
    const int M = B * T * U1;
    const RowArgs p{txt, txt_stride, enc_len, txt_len, B, T, U1, V, blank};
    const GradArgs a{lse, lpb, lpl, alpha, beta, nll, gscale};
    const bool vec = al16(z) && al16(dz) && (ldz % 4 == 0) && (lddz % 4 == 0);
    asrk_prof_begin_(PROF_ROWOPS, s);
    if (V >= RNNT_WG_MIN_V) {
        if (vec)
            hipLaunchKernelGGL((rnnt_grad_kernel<true, true>), dim3(M), dim3(256), 0, s, z, ldz, p, a, M, dz, lddz);
        else
            hipLaunchKernelGGL((rnnt_grad_kernel<false, true>), dim3(M), dim3(256), 0, s, z, ldz, p, a, M, dz, lddz);
    } else {
        const unsigned grid = (unsigned)asrk_div_up(M, 4);
        if (vec)
            hipLaunchKernelGGL((rnnt_grad_kernel<true, false>), dim3(grid), dim3(256), 0, s, z, ldz, p, a, M, dz, lddz);
        else
            hipLaunchKernelGGL((rnnt_grad_kernel<false, false>), dim3(grid), dim3(256), 0, s, z, ldz, p, a, M, dz,
                               lddz);
    }
    asrk_prof_end_(PROF_ROWOPS, s);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}

extern "C" int asrk_rnnt_greedy_step_f32(const float *logits, int64_t ld, const int64_t *enc_len, int B, int T, int V,
                                         int blank, int max_symbols, int max_len, int32_t *t_ptr, int32_t *n_sym,
                                         int32_t *n_tok, int64_t *tokens, int64_t tok_stride, int64_t *last_tok,
                                         int32_t *emit, int32_t *done, void *stream) {
    if (B < 0 || T <= 0 || V <= 0 || ld < V || blank < 0 || blank >= V || max_symbols < 0 || max_len < 0 ||
        tok_stride < max_len)
        return ASRK_EINVAL;
    if (B == 0) return ASRK_OK;
    if (!logits || !enc_len || !t_ptr || !n_sym || !n_tok || !last_tok || !emit || !done || (max_len > 0 && !tokens))
        return ASRK_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    asrk_prof_begin_(PROF_ROWOPS, s);
    hipLaunchKernelGGL(rnnt_greedy_step_kernel, dim3(asrk_div_up(B, 4)), dim3(256), 0, s, logits, ld, enc_len, B, T, V,
                       blank, max_symbols, max_len, t_ptr, n_sym, n_tok, tokens, tok_stride, last_tok, emit, done);
    asrk_prof_end_(PROF_ROWOPS, s);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}
