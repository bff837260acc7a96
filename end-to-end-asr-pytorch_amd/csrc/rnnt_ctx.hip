// Stateless prediction network of the transducer head (Ghodsi et al. 2020) for gfx950 (src/transducer.py): a causal
// depthwise convolution over the last C label embeddings and a ReLU, no recurrence.
//
//   asrk_rnnt_ctx_fwd_f32     Y[b,u,d] = relu(sum_j w[d,0,j] X[b, u-(C-1)+j, d]), one streaming pass over [B*U1, D].
//   asrk_rnnt_ctx_bwd_f32     dX per element; dw in two launches: partial sums per block of CTX_DW_ROWS rows, then the
//                             blocks in ascending order.  No float atomics: two runs are bit-equal.
//   asrk_rnnt_ctx_step_f32    the decode form: the last C labels of every search row are gathered straight from the
//                             embedding matrix, the sum is the forward kernel's (ctx_tap below is the one place it is
//                             written), so a step equals the matching row of the forward bit for bit.
//
// w is [D, 1, C], the layout of a depthwise Conv1d weight; tap C-1 multiplies the current label.  wave64, 256-thread
// workgroups, a thread owns one output element (four with 16-byte accesses).
#include "common.h"

namespace {

constexpr int CTX_MAX_C = 8;
constexpr int CTX_DW_ROWS = 32;   // rows of [B*U1] that one partial sum of dw covers

static inline bool al16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static inline unsigned grid_for64(int64_t n, int block) {
    const int64_t g = (n + block - 1) / block;
    return (unsigned)(g > 65536 ? 65536 : (g < 1 ? 1 : g));
}

// the one multiply-add of the context sum: forward and decode step share it, so their bits agree
__device__ __forceinline__ float ctx_tap(float w, float x, float acc) { return __fmaf_rn(w, x, acc); }

template <bool VEC>
__global__ __launch_bounds__(256) void rnnt_ctx_fwd_kernel(const float *__restrict__ X, int64_t ldx,
                                                           const float *__restrict__ w, int U1, int D, int C,
                                                           float *__restrict__ Y, int64_t ldy, int64_t total) {
    const int per_row = VEC ? (D >> 2) : D;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / per_row;          // b * U1 + u
        const int g = (int)(i - row * per_row);
        const int u = (int)(row % U1);
        const int j0 = u >= C - 1 ? 0 : C - 1 - u;   // taps below j0 look before the sequence: they contribute zero
        if (VEC) {
            const int d = g << 2;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            for (int j = j0; j < C; ++j) {
                const f32x4 x = reinterpret_cast<const f32x4 *>(X + (row - (C - 1) + j) * ldx)[g];
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[c] = ctx_tap(w[(int64_t)(d + c) * C + j], x[c], acc[c]);
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c] = acc[c] > 0.f ? acc[c] : (acc[c] != acc[c] ? acc[c] : 0.f);
            reinterpret_cast<f32x4 *>(Y + row * ldy)[g] = acc;
        } else {
            float acc = 0.f;
            for (int j = j0; j < C; ++j) acc = ctx_tap(w[(int64_t)g * C + j], X[(row - (C - 1) + j) * ldx + g], acc);
            Y[row * ldy + g] = acc > 0.f ? acc : (acc != acc ? acc : 0.f);   // NaN stays NaN
        }
    }
}

// dX[b,u,d] = sum_j w[d,0,j] dYm[b, u+(C-1)-j, d] over the j with u+(C-1)-j < U1, ascending j; dYm = dY (Y > 0)
template <bool VEC>
__global__ __launch_bounds__(256) void rnnt_ctx_dx_kernel(const float *__restrict__ w, const float *__restrict__ Y,
                                                          const float *__restrict__ dY, int U1, int D, int C,
                                                          float *__restrict__ dX, int64_t total) {
    const int per_row = VEC ? (D >> 2) : D;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / per_row;
        const int g = (int)(i - row * per_row);
        const int u = (int)(row % U1);
        const int j0 = u + C - 1 < U1 ? 0 : u + C - U1;   // first j with u + (C-1) - j <= U1 - 1
        if (VEC) {
            const int d = g << 2;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            for (int j = j0; j < C; ++j) {
                const int64_t r = (row + (C - 1) - j) * D;
                const f32x4 y = reinterpret_cast<const f32x4 *>(Y + r)[g];
                const f32x4 gy = reinterpret_cast<const f32x4 *>(dY + r)[g];
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[c] = __fmaf_rn(w[(int64_t)(d + c) * C + j], y[c] > 0.f ? gy[c] : 0.f, acc[c]);
            }
            reinterpret_cast<f32x4 *>(dX + row * D)[g] = acc;
        } else {
            float acc = 0.f;
            for (int j = j0; j < C; ++j) {
                const int64_t r = (row + (C - 1) - j) * D + g;
                acc = __fmaf_rn(w[(int64_t)g * C + j], Y[r] > 0.f ? dY[r] : 0.f, acc);
            }
            dX[row * D + g] = acc;
        }
    }
}

// part[k, j, d] = sum over the rows r of block k (r = k * CTX_DW_ROWS .., ascending) of dYm[r, d] X[r - (C-1) + j, d]
// (the terms that look before the row's own sequence left out).  Lanes run along d: every access is coalesced.
__global__ __launch_bounds__(256) void rnnt_ctx_dw_part_kernel(const float *__restrict__ X, const float *__restrict__ Y,
                                                               const float *__restrict__ dY, int64_t N, int U1, int D,
                                                               int C, float *__restrict__ part) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= D) return;
    const int64_t k = blockIdx.y;
    const int64_t r0 = k * CTX_DW_ROWS;
    const int64_t r1 = r0 + CTX_DW_ROWS < N ? r0 + CTX_DW_ROWS : N;
    float acc[CTX_MAX_C];
#pragma unroll
    for (int j = 0; j < CTX_MAX_C; ++j) acc[j] = 0.f;
    int u = (int)(r0 % U1);
    for (int64_t r = r0; r < r1; ++r) {
        const float y = Y[r * D + d];
        const float g = y > 0.f ? dY[r * D + d] : 0.f;
#pragma unroll
        for (int j = 0; j < CTX_MAX_C; ++j) {
            const int back = C - 1 - j;            // the tap reads `back` rows behind r
            if (j < C && back <= u) acc[j] = __fmaf_rn(g, X[(r - back) * D + d], acc[j]);
        }
        if (++u == U1) u = 0;
    }
#pragma unroll
    for (int j = 0; j < CTX_MAX_C; ++j)
        if (j < C) part[(k * C + j) * D + d] = acc[j];
}

// dw[d, 0, j] = sum_k part[k, j, d], k ascending
__global__ __launch_bounds__(256) void rnnt_ctx_dw_sum_kernel(const float *__restrict__ part, int64_t nblk, int D, int C,
                                                              float *__restrict__ dw) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;   // j * D + d: coalesced reads of part
    if (i >= C * D) return;
    const int j = i / D, d = i - j * D;
    float acc = 0.f;
    for (int64_t k = 0; k < nblk; ++k) acc += part[(k * C + j) * D + d];
    dw[(int64_t)d * C + j] = acc;
}

// TOK = int32_t (beam state) or int64_t (greedy state)
template <bool VEC, typename TOK>
__global__ __launch_bounds__(256) void rnnt_ctx_step_kernel(const TOK *__restrict__ tokens, int64_t ldt,
                                                            const int32_t *__restrict__ n_tok, int Lc,
                                                            const float *__restrict__ emb, int V, int D,
                                                            const float *__restrict__ w, int C, float *__restrict__ Y,
                                                            int64_t ldy, int64_t total) {
    const int per_row = VEC ? (D >> 2) : D;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / per_row;
        const int g = (int)(i - r * per_row);
        int n = n_tok[r];
        n = n < 0 ? 0 : (n > Lc ? Lc : n);
        // tap j reads position n - C + j of the row's labels; -1 is <sos> = 0, anything before it contributes zero
        const int j0 = n >= C - 1 ? 0 : C - 1 - n;
        int64_t lab[CTX_MAX_C];
        bool bad = false;
#pragma unroll
        for (int j = 0; j < CTX_MAX_C; ++j) {
            lab[j] = 0;
            if (j >= j0 && j < C) {
                const int p = n - C + j;
                const int64_t y = p < 0 ? 0 : (int64_t)tokens[r * ldt + p];
                if (y < 0 || y >= V) bad = true;
                else lab[j] = y;                      // a bad label is never used as an index
            }
        }
        const float qnan = __builtin_nanf("");
        if (VEC) {
            const int d = g << 2;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < CTX_MAX_C; ++j) {
                if (j >= j0 && j < C) {
                    const f32x4 x = reinterpret_cast<const f32x4 *>(emb + lab[j] * D)[g];
#pragma unroll
                    for (int c = 0; c < 4; ++c) acc[c] = ctx_tap(w[(int64_t)(d + c) * C + j], x[c], acc[c]);
                }
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c] = bad ? qnan : (acc[c] > 0.f ? acc[c] : (acc[c] != acc[c] ? acc[c] : 0.f));
            reinterpret_cast<f32x4 *>(Y + r * ldy)[g] = acc;
        } else {
            float acc = 0.f;
#pragma unroll
            for (int j = 0; j < CTX_MAX_C; ++j)
                if (j >= j0 && j < C) acc = ctx_tap(w[(int64_t)g * C + j], emb[lab[j] * D + g], acc);
            Y[r * ldy + g] = bad ? qnan : (acc > 0.f ? acc : (acc != acc ? acc : 0.f));
        }
    }
}

static inline int64_t dw_blocks(int64_t N) { return (N + CTX_DW_ROWS - 1) / CTX_DW_ROWS; }

static inline bool ctx_sizes_ok(int B, int U1, int D, int C) { return B >= 0 && U1 > 0 && D > 0; }

}  // namespace

extern "C" int asrk_rnnt_ctx_fwd_f32(const float *X, int64_t ldx, const float *w, int B, int U1, int D, int C, float *Y,
                                     int64_t ldy, void *stream) {
    if (!ctx_sizes_ok(B, U1, D, C) || ldx < D || ldy < D) return ASRK_EINVAL;
    if (C < 1 || C > CTX_MAX_C || (int64_t)B * U1 > (int64_t)INT32_MAX) return ASRK_ESHAPE;
    if (B == 0) return ASRK_OK;
    if (!X || !w || !Y) return ASRK_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const bool vec = al16(X) && al16(Y) && D % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0;
    const int64_t total = (int64_t)B * U1 * (vec ? D / 4 : D);
    asrk_prof_begin_(PROF_ROWOPS, s);
    if (vec)
        hipLaunchKernelGGL((rnnt_ctx_fwd_kernel<true>), dim3(grid_for64(total, 256)), dim3(256), 0, s, X, ldx, w, U1, D, C,
                           Y, ldy, total);
    else
        hipLaunchKernelGGL((rnnt_ctx_fwd_kernel<false>), dim3(grid_for64(total, 256)), dim3(256), 0, s, X, ldx, w, U1, D,
                           C, Y, ldy, total);
    asrk_prof_end_(PROF_ROWOPS, s);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}

extern "C" size_t asrk_rnnt_ctx_bwd_ws_bytes(int B, int U1, int D, int C) {
    if (B <= 0 || U1 <= 0 || D <= 0 || C < 1 || C > CTX_MAX_C) return 0;
    return (size_t)dw_blocks((int64_t)B * U1) * (size_t)C * (size_t)D * sizeof(float);
}

extern "C" int asrk_rnnt_ctx_bwd_f32(const float *X, const float *w, const float *Y, const float *dY, int B, int U1, int D,
                                     int C, float *dX, float *dw, void *ws, size_t ws_bytes, void *stream) {
    if (!ctx_sizes_ok(B, U1, D, C)) return ASRK_EINVAL;
    if (C < 1 || C > CTX_MAX_C || (int64_t)B * U1 > (int64_t)INT32_MAX) return ASRK_ESHAPE;
    if (B == 0) return ASRK_OK;
    if (!X || !w || !Y || !dY || !dX || !dw) return ASRK_EINVAL;
    if (!ws || (reinterpret_cast<uintptr_t>(ws) & 3) || ws_bytes < asrk_rnnt_ctx_bwd_ws_bytes(B, U1, D, C))
        return ASRK_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int64_t N = (int64_t)B * U1;
    const int64_t nblk = dw_blocks(N);
    if (nblk > 65535) return ASRK_ESHAPE;   // gridDim.y
    const bool vec = al16(Y) && al16(dY) && al16(dX) && D % 4 == 0;
    const int64_t total = N * (vec ? D / 4 : D);
    float *part = static_cast<float *>(ws);
    asrk_prof_begin_(PROF_ROWOPS, s);
    if (vec)
        hipLaunchKernelGGL((rnnt_ctx_dx_kernel<true>), dim3(grid_for64(total, 256)), dim3(256), 0, s, w, Y, dY, U1, D, C,
                           dX, total);
    else
        hipLaunchKernelGGL((rnnt_ctx_dx_kernel<false>), dim3(grid_for64(total, 256)), dim3(256), 0, s, w, Y, dY, U1, D, C,
                           dX, total);
    hipLaunchKernelGGL(rnnt_ctx_dw_part_kernel, dim3((D + 255) / 256, (unsigned)nblk), dim3(256), 0, s, X, Y, dY, N, U1,
                       D, C, part);
    hipLaunchKernelGGL(rnnt_ctx_dw_sum_kernel, dim3((C * D + 255) / 256), dim3(256), 0, s, part, nblk, D, C, dw);
    asrk_prof_end_(PROF_ROWOPS, s);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}

extern "C" int asrk_rnnt_ctx_step_f32(const void *tokens, int tok_bytes, int64_t ldt, const int32_t *n_tok, int R, int Lc,
                                      const float *emb, int V, int D, const float *w, int C, float *Y, int64_t ldy,
                                      void *stream) {
    if (R < 0 || Lc <= 0 || V <= 0 || D <= 0 || ldt < Lc || ldy < D) return ASRK_EINVAL;
    if (C < 1 || C > CTX_MAX_C || (tok_bytes != 4 && tok_bytes != 8)) return ASRK_ESHAPE;
    if (R == 0) return ASRK_OK;
    if (!tokens || !n_tok || !emb || !w || !Y) return ASRK_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const bool vec = al16(emb) && al16(Y) && D % 4 == 0 && ldy % 4 == 0;
    const int64_t total = (int64_t)R * (vec ? D / 4 : D);
    const unsigned grid = grid_for64(total, 256);
    asrk_prof_begin_(PROF_ROWOPS, s);
    if (tok_bytes == 4) {
        const int32_t *t = static_cast<const int32_t *>(tokens);
        if (vec)
            hipLaunchKernelGGL((rnnt_ctx_step_kernel<true, int32_t>), dim3(grid), dim3(256), 0, s, t, ldt, n_tok, Lc, emb,
                               V, D, w, C, Y, ldy, total);
        else
            hipLaunchKernelGGL((rnnt_ctx_step_kernel<false, int32_t>), dim3(grid), dim3(256), 0, s, t, ldt, n_tok, Lc,
                               emb, V, D, w, C, Y, ldy, total);
    } else {
        const int64_t *t = static_cast<const int64_t *>(tokens);
        if (vec)
            hipLaunchKernelGGL((rnnt_ctx_step_kernel<true, int64_t>), dim3(grid), dim3(256), 0, s, t, ldt, n_tok, Lc, emb,
                               V, D, w, C, Y, ldy, total);
        else
            hipLaunchKernelGGL((rnnt_ctx_step_kernel<false, int64_t>), dim3(grid), dim3(256), 0, s, t, ldt, n_tok, Lc,
                               emb, V, D, w, C, Y, ldy, total);
    }
    asrk_prof_end_(PROF_ROWOPS, s);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}
