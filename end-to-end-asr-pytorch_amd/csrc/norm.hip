// Per-frame regularisers of the encoder / decoder stacks (src/module.py:116-119,135-138;
// src/asr.py:36,162,219,226): LayerNorm over the feature axis and inverted dropout.
// Both are one-pass HBM streaming kernels (wave64 per row / 16-B lanes).  Dropout keeps NO mask in
// memory: the keep-decision of element i is bit (Philox4x32-10(counter = i/4, key = seed))[i%4],
// so backward re-derives the same mask from (seed, offset) instead of reading 1 byte/element.
#include "common.h"
#include "knobs.h"
#include "philox.h"
#include "rowops_plan.h"
#include <algorithm>

namespace {

// ---------------------------------------------------------------- LayerNorm
// one wave per row; biased variance, eps inside the sqrt (torch.nn.LayerNorm semantics)
__global__ __launch_bounds__(256) void ln_fwd_kernel(const float *__restrict__ x,
                                                     const float *__restrict__ w,
                                                     const float *__restrict__ b,
                                                     float *__restrict__ y,
                                                     float *__restrict__ mean_out,
                                                     float *__restrict__ rstd_out, int rows, int cols,
                                                     float eps) {
    const int row = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float *xr = x + (size_t)row * cols;
    float *yr = y + (size_t)row * cols;
    float s = 0.f;
    for (int i = lane; i < cols; i += 64) s += xr[i];
    const float mean = wave_sum(s) / (float)cols;
    float v = 0.f;
    for (int i = lane; i < cols; i += 64) {
        const float d = xr[i] - mean;
        v += d * d;
    }
    const float rstd = 1.0f / sqrtf(wave_sum(v) / (float)cols + eps);
    for (int i = lane; i < cols; i += 64) yr[i] = (xr[i] - mean) * rstd * w[i] + b[i];
    if (lane == 0) {
        mean_out[row] = mean;
        rstd_out[row] = rstd;
    }
}

// dx_r = rstd * (g*w - mean_c(g*w) - xhat * mean_c(g*w*xhat))
__global__ __launch_bounds__(256) void ln_bwd_data_kernel(const float *__restrict__ x,
                                                          const float *__restrict__ w,
                                                          const float *__restrict__ dy,
                                                          const float *__restrict__ mean_in,
                                                          const float *__restrict__ rstd_in,
                                                          float *__restrict__ dx, int rows, int cols) {
    const int row = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float *xr = x + (size_t)row * cols;
    const float *gr = dy + (size_t)row * cols;
    float *dr = dx + (size_t)row * cols;
    const float mean = mean_in[row], rstd = rstd_in[row];
    float s1 = 0.f, s2 = 0.f;
    for (int i = lane; i < cols; i += 64) {
        const float gw = gr[i] * w[i];
        s1 += gw;
        s2 += gw * (xr[i] - mean) * rstd;
    }
    s1 = wave_sum(s1) / (float)cols;
    s2 = wave_sum(s2) / (float)cols;
    for (int i = lane; i < cols; i += 64) {
        const float xh = (xr[i] - mean) * rstd;
        dr[i] = rstd * (gr[i] * w[i] - s1 - xh * s2);
    }
}

// dw_c = sum_r dy*xhat, db_c = sum_r dy : 64 columns x 4 row-lanes per block, row chunks on
// grid.y, atomics combine the chunks (outputs pre-zeroed by the launcher)
__global__ __launch_bounds__(256) void ln_bwd_param_kernel(const float *__restrict__ x,
                                                           const float *__restrict__ dy,
                                                           const float *__restrict__ mean_in,
                                                           const float *__restrict__ rstd_in,
                                                           float *__restrict__ dw,
                                                           float *__restrict__ db, int rows, int cols,
                                                           int rows_per_chunk) {
    __shared__ float pw[4][64], pb[4][64];
    const int l = threadIdx.x & 63;
    const int c = blockIdx.x * 64 + l;
    const int rl = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r0 = blockIdx.y * rows_per_chunk;
    const int r1 = min(rows, r0 + rows_per_chunk);
    float sw = 0.f, sb = 0.f;
    if (c < cols) {
        for (int r = r0 + rl; r < r1; r += 4) {
            const float g = dy[(size_t)r * cols + c];
            sw += g * (x[(size_t)r * cols + c] - mean_in[r]) * rstd_in[r];
            sb += g;
        }
    }
    pw[rl][l] = sw;
    pb[rl][l] = sb;
    __syncthreads();
    if (rl == 0 && c < cols) {
        unsafeAtomicAdd(dw + c, pw[0][l] + pw[1][l] + pw[2][l] + pw[3][l]);
        unsafeAtomicAdd(db + c, pb[0][l] + pb[1][l] + pb[2][l] + pb[3][l]);
    }
}

// ---------------------------------------------------------------- dropout (Philox4x32-10)
// y[i] = keep(i) ? x[i] * scale : 0, keep(i) <=> (u32 >> 8) >= thresh24  (thresh24 = round(p*2^24))
template <bool VEC>
__global__ __launch_bounds__(256) void dropout_kernel(const float *__restrict__ x,
                                                      float *__restrict__ y, int64_t n,
                                                      uint32_t thresh24, float scale, uint64_t seed,
                                                      uint64_t offset) {
    const int64_t nq = (n + 3) >> 2;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq;
         q += (int64_t)gridDim.x * blockDim.x) {
        uint32_t r[4];
        philox4x32_10((uint64_t)q, offset, seed, r);
        if (VEC) {
            f32x4 v = reinterpret_cast<const f32x4 *>(x)[q];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = ((r[j] >> 8) >= thresh24) ? v[j] * scale : 0.f;
            reinterpret_cast<f32x4 *>(y)[q] = v;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t i = q * 4 + j;
                if (i < n) y[i] = ((r[j] >> 8) >= thresh24) ? x[i] * scale : 0.f;
            }
        }
    }
}

}  // namespace

extern "C" int asrk_layer_norm_fwd_f32(const float *x, const float *weight, const float *bias,
                                       float *y, float *mean, float *rstd, int rows, int cols,
                                       float eps, void *stream) {
    if (rows < 0 || cols <= 0 || !(eps >= 0.f)) return ASRK_EINVAL;
    if (rows == 0) return ASRK_OK;
    if (!x || !weight || !bias || !y || !mean || !rstd) return ASRK_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    asrk_prof_begin_(PROF_ROWOPS, s);
    hipLaunchKernelGGL(ln_fwd_kernel, dim3((unsigned)asrk_div_up(rows, 4)), dim3(256), 0, s, x,
                       weight, bias, y, mean, rstd, rows, cols, eps);
    asrk_prof_end_(PROF_ROWOPS, s);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}

extern "C" int asrk_layer_norm_bwd_f32(const float *x, const float *weight, const float *dy,
                                       const float *mean, const float *rstd, float *dx, float *dweight,
                                       float *dbias, int rows, int cols, void *stream) {
    if (rows < 0 || cols <= 0) return ASRK_EINVAL;
    if (!dweight != !dbias) return ASRK_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (dweight) {
        ASRK_HIP(hipMemsetAsync(dweight, 0, sizeof(float) * cols, s));
        ASRK_HIP(hipMemsetAsync(dbias, 0, sizeof(float) * cols, s));
    }
    if (rows == 0) return ASRK_OK;
    if (!x || !weight || !dy || !mean || !rstd) return ASRK_EINVAL;
    asrk_prof_begin_(PROF_ROWOPS, s);
    if (dx)
        hipLaunchKernelGGL(ln_bwd_data_kernel, dim3((unsigned)asrk_div_up(rows, 4)), dim3(256), 0, s,
                           x, weight, dy, mean, rstd, dx, rows, cols);
    if (dweight) {
        const rowops_plan::LnParamPlan pl = rowops_plan::ln_param_plan(rows, cols);
        hipLaunchKernelGGL(ln_bwd_param_kernel, dim3(pl.gx, pl.gy), dim3(256), 0, s, x, dy, mean, rstd, dweight, dbias,
                           rows, cols, pl.rpc);
    }
    asrk_prof_end_(PROF_ROWOPS, s);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}

extern "C" int asrk_dropout_f32(const float *x, float *y, int64_t n, float p, uint64_t seed,
                                uint64_t offset, void *stream) {
    if (n < 0 || !(p >= 0.f) || !(p < 1.f)) return ASRK_EINVAL;
    if (n == 0) return ASRK_OK;
    if (!x || !y) return ASRK_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t thresh24 = (uint32_t)llrintf(p * 16777216.0f);
    const float scale = 1.0f / (1.0f - p);
    const rowops_plan::DropoutPlan pl = rowops_plan::dropout_plan(x, y, n);
    const unsigned grid = pl.grid;
    asrk_prof_begin_(PROF_ROWOPS, s);
    if (pl.variant == 1)
        hipLaunchKernelGGL((dropout_kernel<true>), dim3(grid), dim3(256), 0, s, x, y, n, thresh24,
                           scale, (uint64_t)seed, (uint64_t)offset);
    else
        hipLaunchKernelGGL((dropout_kernel<false>), dim3(grid), dim3(256), 0, s, x, y, n, thresh24,
                           scale, (uint64_t)seed, (uint64_t)offset);
    asrk_prof_end_(PROF_ROWOPS, s);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}
