// Minimum word error rate training on n-best lists (src/mwer.py) - the two kernels beside asrk_seq_logp_lse_f32
// (rescore.hip) that make the sequence scores trainable:
//
//   asrk_seq_logp_bwd_f32   dx[m, v] = w_m * (1[v == target[m]] - exp(x[m, v] - lse[m])), w_m the float64 gradient of the
//                           sequence row m belongs to, rounded to f32 once.  ce_bwd_kernel (rowops.hip) with a weight
//                           per row instead of one scalar: reads x once, writes dx once, HBM bound.
//   asrk_mwer_loss_f64      softmax over the n-best scores of one utterance, expected errors, the mean-subtracted loss
//                           and its closed-form derivative; one wave per utterance, float64 throughout.
//
// wave64, no float atomics: every result is reproducible bit for bit.
#include "common.h"

namespace {

constexpr int BWD_WG_MIN_V = 2048;   // the case split of seq_logp (rescore.hip): a workgroup per row from here on
constexpr int MWER_MAX_N = 32;       // the beam search's own limit

// The weight of row m: gseq[r] of the segment [seg_off[r], seg_off[r+1]) that holds m (seg_off [R+1], non-decreasing),
// found by bisection - the last r in [0, R] with seg_off[r] <= m.  false: m lies in no segment.
__device__ __forceinline__ bool row_weight(const int64_t *__restrict__ seg_off, const double *__restrict__ gseq, int R,
                                           int m, float &w) {
    if (R <= 0 || seg_off[0] > m || seg_off[R] <= m) return false;
    int lo = 0, hi = R;              // seg_off[lo] <= m < seg_off[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (seg_off[mid] <= m) lo = mid;
        else hi = mid;
    }
    w = (float)gseq[lo];
    return true;
}

__device__ __forceinline__ float bwd_value(float x, float lse, float w, bool hit) {
    return w * ((hit ? 1.f : 0.f) - expf(x - lse));
}

// WG = false: one wave per row, 4 rows per workgroup; WG = true: one 256-thread workgroup per row.  x and dx may be the
// same memory: a thread reads an element (or a 16-byte group) and then writes that very element, nothing else.
template <bool VEC, bool WG>
__global__ __launch_bounds__(256) void seq_logp_bwd_kernel(const float *x, int64_t ldx,
                                                           const int64_t *__restrict__ target,
                                                           const float *__restrict__ lse,
                                                           const int64_t *__restrict__ seg_off,
                                                           const double *__restrict__ gseq, int M, int V, int R,
                                                           float *dx, int64_t lddx) {
    const int row = WG ? (int)blockIdx.x : (int)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tid = WG ? (int)threadIdx.x : (int)(threadIdx.x & 63);
    constexpr int NT = WG ? 256 : 64;
    if (row >= M) return;
    float *dr = dx + (size_t)row * lddx;
    const int64_t tg = target[row];
    float w = 0.f;
    // (every thread bisects for itself: row is wave-uniform, so these are log2(R) scalar loads per wave, far below the
    // cost of a row, and no [M] weight array has to be built and read)
    const bool counted = tg >= 0 && row_weight(seg_off, gseq, R, row, w);
    if (!counted || tg >= V) {
        // skipped row or no segment: zeros are WRITTEN, x is never read.  A label >= V inside a segment made the
        // forward's score NaN (tok_value, rescore.hip): its gradient is NaN too, as autograd would hand on
        const float fill = counted ? __builtin_nanf("") : 0.f;
        if (VEC) {
            const int nv = V >> 2;
            const f32x4 z = {fill, fill, fill, fill};
            for (int i = tid; i < nv; i += NT) reinterpret_cast<f32x4 *>(dr)[i] = z;
            for (int i = (nv << 2) + tid; i < V; i += NT) dr[i] = fill;
        } else {
            for (int i = tid; i < V; i += NT) dr[i] = fill;
        }
        return;
    }
    const float *xr = x + (size_t)row * ldx;
    const float l = lse[row];
    const int t = (int)tg;
    if (VEC) {
        const int nv = V >> 2;
#pragma unroll 4
        for (int i = tid; i < nv; i += NT) {
            const f32x4 v = reinterpret_cast<const f32x4 *>(xr)[i];
            const int c = i << 2;
            f32x4 o;
            o[0] = bwd_value(v[0], l, w, c == t);
            o[1] = bwd_value(v[1], l, w, c + 1 == t);
            o[2] = bwd_value(v[2], l, w, c + 2 == t);
            o[3] = bwd_value(v[3], l, w, c + 3 == t);
            reinterpret_cast<f32x4 *>(dr)[i] = o;
        }
        for (int i = (nv << 2) + tid; i < V; i += NT) dr[i] = bwd_value(xr[i], l, w, i == t);
    } else {
#pragma unroll 4
        for (int i = tid; i < V; i += NT) dr[i] = bwd_value(xr[i], l, w, i == t);
    }
}

__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// one wave per utterance (4 per workgroup); lane n < N holds hypothesis n, whose row is n * U + u
__global__ __launch_bounds__(256) void mwer_loss_kernel(const double *__restrict__ s, const int32_t *__restrict__ err,
                                                        const int32_t *__restrict__ count, int N, int U,
                                                        double *__restrict__ loss_u, double *__restrict__ exp_err_u,
                                                        double *__restrict__ g) {
    const int u = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (u >= U) return;
    int cnt = count[u];
    cnt = cnt < 0 ? 0 : (cnt > N ? N : cnt);
    const bool valid = lane < cnt;
    const size_t idx = (size_t)lane * U + u;
    const double sv = valid ? s[idx] : -INFINITY;
    const double ev = valid ? (double)err[idx] : 0.0;
    const double mx = wave_max_f64(sv);
    const double ex = valid ? exp(sv - mx) : 0.0;     // the largest score contributes exp(0) = 1: Z >= 1
    const double Z = wave_sum_f64(ex);
    const double p = valid ? ex / Z : 0.0;
    const double ebar = cnt > 0 ? wave_sum_f64(ev) / (double)cnt : 0.0;
    const double ee = wave_sum_f64(p * ev);
    const double loss = wave_sum_f64(p * (ev - ebar));
    if (lane < N) g[idx] = valid ? p * (ev - ee) : 0.0;
    if (lane == 0) {
        loss_u[u] = cnt > 0 ? loss : 0.0;
        exp_err_u[u] = cnt > 0 ? ee : 0.0;
    }
}

static inline bool al16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int asrk_seq_logp_bwd_f32(const float *x, int64_t ldx, const int64_t *target, const float *lse,
                                     const int64_t *seg_off, const double *gseq, int M, int V, int R, float *dx,
                                     int64_t lddx, void *stream) {
    if (M < 0 || V <= 0 || R < 0 || ldx < V || lddx < V) return ASRK_EINVAL;
    if (M == 0) return ASRK_OK;
    if (!x || !target || !lse || !dx) return ASRK_EINVAL;
    if (R > 0 && (!seg_off || !gseq)) return ASRK_EINVAL;
    if (dx == x && lddx != ldx) return ASRK_EINVAL;   // in place means element for element
    hipStream_t s = (hipStream_t)stream;
    const bool vec = al16(x) && al16(dx) && (ldx % 4 == 0) && (lddx % 4 == 0);
    asrk_prof_begin_(PROF_ROWOPS, s);   // the row-kernel family, where seq_logp and the cross-entropy kernels count
    if (V >= BWD_WG_MIN_V) {
        if (vec)
            hipLaunchKernelGGL((seq_logp_bwd_kernel<true, true>), dim3(M), dim3(256), 0, s, x, ldx, target, lse,
                               seg_off, gseq, M, V, R, dx, lddx);
        else
            hipLaunchKernelGGL((seq_logp_bwd_kernel<false, true>), dim3(M), dim3(256), 0, s, x, ldx, target, lse,
                               seg_off, gseq, M, V, R, dx, lddx);
    } else {
        const unsigned grid = (unsigned)asrk_div_up(M, 4);
        if (vec)
            hipLaunchKernelGGL((seq_logp_bwd_kernel<true, false>), dim3(grid), dim3(256), 0, s, x, ldx, target, lse,
                               seg_off, gseq, M, V, R, dx, lddx);
        else
            hipLaunchKernelGGL((seq_logp_bwd_kernel<false, false>), dim3(grid), dim3(256), 0, s, x, ldx, target, lse,
                               seg_off, gseq, M, V, R, dx, lddx);
    }
    asrk_prof_end_(PROF_ROWOPS, s);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}

extern "C" int asrk_mwer_loss_f64(const double *s, const int32_t *err, const int32_t *count, int N, int U,
                                  double *loss_u, double *exp_err_u, double *g, void *stream) {
    if (N < 0 || U < 0) return ASRK_EINVAL;
    if (N > MWER_MAX_N) return ASRK_ESHAPE;
    if (U == 0) return ASRK_OK;
    if (!count || !loss_u || !exp_err_u) return ASRK_EINVAL;
    if (N > 0 && (!s || !err || !g)) return ASRK_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    asrk_prof_begin_(PROF_ROWOPS, st);
    hipLaunchKernelGGL(mwer_loss_kernel, dim3(asrk_div_up(U, 4)), dim3(256), 0, st, s, err, count, N, U, loss_u,
                       exp_err_u, g);
    asrk_prof_end_(PROF_ROWOPS, st);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}
