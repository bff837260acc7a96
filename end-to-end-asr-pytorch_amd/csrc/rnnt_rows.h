// Row arithmetic shared by the transducer loss kernels (rnnt.hip: the dense lattice; rnnt_prune.hip: the pruned band):
// the one-pass log-sum-exp of a row of logits and the value of one gradient element.  Device code only.
#pragma once
#include "common.h"

#define RNNT_HD __device__
#include "rnnt.inc"

namespace {

constexpr int RNNT_WG_MIN_V = 2048;     // the case split of seq_logp (rescore.hip): a workgroup per row from here on

static inline bool al16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---------------------------------------------------------------------------------------------
// row reductions: running (max, sum of exp(x - max)) per lane, the arithmetic of seq_logp (rescore.hip)

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

__device__ __forceinline__ MaxSum ms_wave(MaxSum a) {
    const float M = wave_max(a.m);
    const float s = (a.m == -INFINITY) ? 0.f : a.s * expf(a.m - M);
    return MaxSum{M, wave_sum(s)};
}

template <bool VEC>
__device__ __forceinline__ MaxSum ms_row(const float *__restrict__ xr, int V, int tid, int nthreads) {
    MaxSum a{-INFINITY, 0.f};
    if (VEC) {
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

// d nll / d z of one element: k from rnnt_coef, gs the utterance's scale
__device__ __forceinline__ float grad_value(float x, float lse, const RnntCoef &k, float gs, bool isb, bool isl) {
    float g = expf((x - lse) + k.c);
    if (isb) g -= k.eb;
    if (isl) g -= k.el;
    return gs * g;
}

}  // namespace
