// SpecAugment on a padded feature batch (time warp along the frames, frequency masks, time masks) in one pass over
// HBM: x [B, T, ld] -> y [B, T, ld].  Everything random is decided on the host (src/audio.py:SpecAugment.sample) and
// arrives as one int32 row per utterance; the kernel is a pure function of (x, lens, params).
//
// One workgroup = one utterance x SA_TILE output frames.  Prologue: the parameter row goes to LDS once; thread f < tile
// works out frame f's two source frames and blend weight (the only 64-bit divisions of the kernel: one per frame, not
// per element), every thread marks its share of the C*D columns as frequency-masked or not.  Body: the tile's
// frames x columns, 16 B per lane when the rows allow it, one element per lane otherwise.
#include "common.h"

#define SA_THREADS 256
#define SA_TILE 32
#define SA_MAX_MASKS 8
#define SA_MAX_COLS 16384                      // column mask bytes in LDS
#define SA_MAX_P (2 + 4 * SA_MAX_MASKS)
// LDS: s_i, s_j, s_a [SA_TILE], the parameter row [SA_MAX_P], then (16-byte aligned) one mask byte per column
#define SA_HDR_BYTES (((3 * SA_TILE + SA_MAX_P) * 4 + 15) & ~15)

// frame codes in s_i / s_j
#define SA_FRAME_FILL (-1)                     // s_i: time-masked frame
#define SA_FRAME_PAD (-1)                      // s_j: frame beyond the utterance, copied as it is (no frequency mask)

template <bool VEC> struct SaElem;
template <> struct SaElem<true> {
    typedef f32x4 T;
    typedef uint32_t M;
    static __device__ __forceinline__ T splat(float v) { return T{v, v, v, v}; }
    static __device__ __forceinline__ T masked(T v, M m, float fill) {
        if (m & 0x000000ffu) v.x = fill;
        if (m & 0x0000ff00u) v.y = fill;
        if (m & 0x00ff0000u) v.z = fill;
        if (m & 0xff000000u) v.w = fill;
        return v;
    }
};
template <> struct SaElem<false> {
    typedef float T;
    typedef uint8_t M;
    static __device__ __forceinline__ T splat(float v) { return v; }
    static __device__ __forceinline__ T masked(T v, M m, float fill) { return m ? fill : v; }
};

// source of output frame t of an utterance of n frames: i, j = min(i + 1, n - 1), a = r / den (0 <=> r == 0)
__device__ __forceinline__ void sa_warp_source(int t, int n, int c, int w, int &i, int &j, float &a) {
    i = t, j = t, a = 0.0f;
    const int64_t d = (int64_t)c + w;
    if (!(w != 0 && c > 0 && c < n - 1 && d > 0 && d < n - 1)) return;
    int64_t num, den;
    if (t <= d) {
        num = (int64_t)t * c, den = d;
    } else {
        num = (int64_t)c * (n - 1 - d) + (t - d) * (int64_t)(n - 1 - c), den = n - 1 - d;
    }
    int64_t q, r;
    if (((uint64_t)num | (uint64_t)den) >> 32) {
        q = num / den, r = num % den;
    } else {                                   // every realistic length: 32-bit hardware-assisted division
        const uint32_t n32 = (uint32_t)num, d32 = (uint32_t)den;
        q = n32 / d32, r = n32 % d32;
    }
    // the map is increasing and fixes 0 and n - 1; the clamps hold whatever a miscomputed table would do to it
    i = (int)(q < 0 ? 0 : (q > n - 1 ? n - 1 : q));
    j = i + 1 < n ? i + 1 : n - 1;
    a = r == 0 ? 0.0f : (float)r / (float)den;
}

template <bool VEC>
__global__ __launch_bounds__(SA_THREADS) void spec_augment_kernel(const float *__restrict__ x, float *__restrict__ y,
                                                                  int T, int ld, int D, int CD, int tiles,
                                                                  const int64_t *__restrict__ lens,
                                                                  const int32_t *__restrict__ params, int n_fmask,
                                                                  int n_tmask, float fill) {
    typedef typename SaElem<VEC>::T ET;
    typedef typename SaElem<VEC>::M MT;
    extern __shared__ __attribute__((aligned(16))) unsigned char sa_smem[];
    int *s_i = reinterpret_cast<int *>(sa_smem);
    int *s_j = s_i + SA_TILE;
    float *s_a = reinterpret_cast<float *>(s_j + SA_TILE);
    int *s_par = reinterpret_cast<int *>(s_a + SA_TILE);
    uint8_t *s_cm = sa_smem + SA_HDR_BYTES;

    const int tid = threadIdx.x;
    const int b = blockIdx.x / tiles, t0 = (blockIdx.x - b * tiles) * SA_TILE;
    const int nt = min(SA_TILE, T - t0);
    const int P = 2 + 2 * n_fmask + 2 * n_tmask;
    if (tid < P) s_par[tid] = params[(size_t)b * P + tid];
    const int64_t len = lens[b];
    const int n = (int)(len < 0 ? 0 : (len > T ? T : len));
    __syncthreads();

    if (tid < nt) {
        const int t = t0 + tid;
        int i = t, j = SA_FRAME_PAD;
        float a = 0.0f;
        if (t < n) {
            bool hit = false;
            const int *tm = s_par + 2 + 2 * n_fmask;
            for (int k = 0; k < n_tmask; ++k) {
                const int64_t m0 = tm[2 * k], mw = tm[2 * k + 1];
                hit = hit || (mw > 0 && t >= m0 && t < m0 + mw);
            }
            if (hit) i = SA_FRAME_FILL, j = 0;
            else sa_warp_source(t, n, s_par[0], s_par[1], i, j, a);
        }
        s_i[tid] = i, s_j[tid] = j, s_a[tid] = a;
    }
    for (int col = tid; col < CD; col += SA_THREADS) {
        const int d = col % D;
        bool hit = false;
        for (int k = 0; k < n_fmask; ++k) {
            const int64_t m0 = s_par[2 + 2 * k], mw = s_par[3 + 2 * k];
            hit = hit || (mw > 0 && d >= m0 && d < m0 + mw);
        }
        s_cm[col] = hit ? 1 : 0;
    }
    __syncthreads();

    // body: units = 4-column vectors (VEC) or columns; (f, u) walks the tile in steps of SA_THREADS units
    const int units = VEC ? CD / 4 : CD;
    const int df = SA_THREADS / units, du = SA_THREADS - df * units;
    int f = tid / units, u = tid - f * units;
    const ET *xb = reinterpret_cast<const ET *>(x + (size_t)b * T * ld);
    ET *yb = reinterpret_cast<ET *>(y + (size_t)b * T * ld);
    const size_t row = VEC ? ld / 4 : ld;
    const MT *cm = reinterpret_cast<const MT *>(s_cm);
    for (; f < nt; f += df, u += du) {
        if (u >= units) {
            u -= units;
            if (++f >= nt) break;
        }
        const int i = s_i[f], j = s_j[f];
        ET out;
        if (i == SA_FRAME_FILL) {
            out = SaElem<VEC>::splat(fill);
        } else {
            const float a = s_a[f];
            out = xb[(size_t)i * row + u];
            if (a != 0.0f) {
                const ET xj = xb[(size_t)j * row + u];
                out = (1.0f - a) * out + a * xj;
            }
            if (j != SA_FRAME_PAD) out = SaElem<VEC>::masked(out, cm[u], fill);
        }
        yb[(size_t)(t0 + f) * row + u] = out;
    }
}

extern "C" int asrk_spec_augment_f32(const float *x, float *y, int B, int T, int ld, int D, int C,
                                     const int64_t *lens, const int32_t *params, int n_fmask, int n_tmask, float fill,
                                     void *stream) {
    if (B < 0 || T < 0 || ld < 0 || D < 0 || C < 0) return ASRK_ESHAPE;
    const int64_t cd = (int64_t)C * D;
    if (ld < cd || cd > SA_MAX_COLS) return ASRK_ESHAPE;
    if (n_fmask < 0 || n_fmask > SA_MAX_MASKS || n_tmask < 0 || n_tmask > SA_MAX_MASKS) return ASRK_ESHAPE;
    if (x && x == y) return ASRK_ESHAPE;                                // the warp reads frames other workgroups write
    if ((int64_t)B * T == 0) return ASRK_OK;
    if (!x || !y || !lens || !params) return ASRK_ESHAPE;
    if (cd == 0) return ASRK_OK;                                        // no column belongs to the features
    const int tiles = (int)asrk_div_up64(T, SA_TILE);
    if ((int64_t)B * tiles > 0x7fffffff) return ASRK_ESHAPE;
    hipStream_t s = (hipStream_t)stream;
    const bool vec = ld % 4 == 0 && cd % 4 == 0 && (((uintptr_t)x | (uintptr_t)y) & 15) == 0;
    const size_t lds = SA_HDR_BYTES + (size_t)((cd + 3) & ~3);
    const dim3 grid((unsigned)(B * tiles)), block(SA_THREADS);
    asrk_prof_begin_(PROF_FBANK, s);
    if (vec)
        hipLaunchKernelGGL(spec_augment_kernel<true>, grid, block, lds, s, x, y, T, ld, D, (int)cd, tiles, lens, params,
                           n_fmask, n_tmask, fill);
    else
        hipLaunchKernelGGL(spec_augment_kernel<false>, grid, block, lds, s, x, y, T, ld, D, (int)cd, tiles, lens,
                           params, n_fmask, n_tmask, fill);
    asrk_prof_end_(PROF_FBANK, s);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}
