// Reverberation and additive noise on the padded PCM batch: every row convolved with its own room impulse response
// (direct-form FIR of up to 8192 taps, output shifted by the response's peak so the row keeps its length), level
// restored to the dry signal's, a circularly tiled noise row added at a requested signal-to-noise ratio
// (semantics: include/asrk.h, asrk_reverb_mix_f32).  x [B, ld_in] (int16 or f32) -> out [B, ld_out] f32, two launches:
//
//   1. reverb_conv_kernel: one workgroup = one row x one tile of RM_TILE outputs.  The taps are walked in chunks of
//      RM_KC, last chunk first (so every output is summed in DESCENDING k: the small late taps first).  Per chunk the
//      taps go to LDS reversed and the matching window of s = x * scale (RM_TILE + RM_KC samples, zero outside the row)
//      is converted once.  A lane owns RM_PER = 8 consecutive outputs in registers and slides a 12-sample window over
//      LDS: per 4 taps one 16-byte read of s, one 16-byte broadcast read of h, 32 FMAs (0.25 LDS words per FMA).  Lanes
//      read s at a stride of 8 words; rm_phys() skews every 64-word line by 4 words so that the 16 lanes of a
//      ds_read_b128 group cover all 64 banks.  The tile's sums of s^2, y^2 and v^2 leave in float64 as one partial each
//      (ws [B][tiles][3]); y is written to out.
//   2. reverb_mix_kernel: adds a row's partials in tile order (every workgroup of the row does the same additions),
//      a = sqrt(Ps / Py), g = sqrt(Ps / (Pv * snr)), out = a * out + g * v in place.  Rows with a == 1 and g == 0 are
//      left as launch 1 wrote them; the launch is skipped when no row has a response or noise.
//
// No atomics: a row's bits depend on nothing but the row.
#include <float.h>
#include "common.h"

#define RM_THREADS 256
#define RM_PER 8                               // consecutive outputs per lane
#define RM_TILE (RM_THREADS * RM_PER)          // outputs per workgroup
#define RM_KC 384                              // taps per chunk: a multiple of 12 (the register window turns in 3 steps of 4)
#define RM_MAX_TAPS 8192
#define RM_SX (RM_TILE + RM_KC)                // window of s per chunk (the last word is read, never used)
#define RM_SX_WORDS (RM_SX + (RM_SX / 64) * 4)
#define RM_USE_RIR 1
#define RM_USE_NOISE 2

__device__ __forceinline__ int rm_phys(int j) { return j + ((j >> 6) << 2); }       // word j of the window in LDS
__device__ __forceinline__ int rm_quad(int j4) { return j4 + (j4 >> 4); }           // = rm_phys(4 * j4) / 4

__device__ __forceinline__ double rm_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// acc[r] += h[u] * w[r + u] over the 12-sample window (a, b, c), u ascending
__device__ __forceinline__ void rm_fma(float (&acc)[RM_PER], const f32x4 a, const f32x4 b, const f32x4 c,
                                       const f32x4 h) {
    const float w[12] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3], c[0], c[1], c[2], c[3]};
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int r = 0; r < RM_PER; ++r) acc[r] = fmaf(h[u], w[r + u], acc[r]);
}

struct RmRow {                                 // a row's clamped view of the device copies
    int64_t n, m;
    int r, K, p;
};

__device__ __forceinline__ RmRow rm_row(int b, const int64_t *n_rows, const int64_t *m_rows, const int32_t *rir_idx,
                                        const int32_t *rir_len, const int32_t *rir_peak, int R, int64_t ld_in,
                                        int64_t ld_out, int64_t ld_v, int64_t ld_r, int tiles, int use) {
    RmRow w;
    int64_t n = n_rows[b];                     // the host checked its copies; these are not trusted
    const int64_t cap = ld_in < ld_out ? ld_in : ld_out;
    n = n < 0 ? 0 : (n > cap ? cap : n);
    if (n > (int64_t)tiles * RM_TILE) n = (int64_t)tiles * RM_TILE;
    w.n = n;
    int64_t m = (use & RM_USE_NOISE) ? m_rows[b] : 0;
    w.m = m < 0 ? 0 : (m > ld_v ? ld_v : m);
    int r = (use & RM_USE_RIR) ? rir_idx[b] : -1;
    if (r < 0 || r >= R) r = -1;
    w.r = r, w.K = 1, w.p = 0;
    if (r >= 0) {
        int K = rir_len[r], p = rir_peak[r];
        const int kcap = ld_r < RM_MAX_TAPS ? (int)ld_r : RM_MAX_TAPS;
        K = K < 1 ? 1 : (K > kcap ? kcap : K);
        w.K = K, w.p = p < 0 ? 0 : (p > K - 1 ? K - 1 : p);
        if (kcap < 1) w.r = -1;
    }
    return w;
}

template <typename T, bool VEC>
__global__ __launch_bounds__(RM_THREADS) void reverb_conv_kernel(
    const T *__restrict__ x, int64_t ld_in, const T *__restrict__ v, int64_t ld_v, float *__restrict__ out,
    int64_t ld_out, const float *__restrict__ rir, int64_t ld_r, const int64_t *__restrict__ n_rows,
    const int64_t *__restrict__ m_rows, const int32_t *__restrict__ rir_idx, const int32_t *__restrict__ rir_len,
    const int32_t *__restrict__ rir_peak, int R, int tiles, float scale, int use, double *__restrict__ ws) {
    __shared__ f32x4 s_h4[RM_KC / 4];          // read 16 bytes at a time (typed so: the compiler then emits ds_read_b128),
    __shared__ f32x4 s_x4[RM_SX_WORDS / 4];    // written a word at a time through s_h / s_x
    float *s_h = reinterpret_cast<float *>(s_h4), *s_x = reinterpret_cast<float *>(s_x4);
    __shared__ double s_red[RM_THREADS / 64][3];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
    const RmRow w = rm_row(b, n_rows, m_rows, rir_idx, rir_len, rir_peak, R, ld_in, ld_out, ld_v, ld_r, tiles, use);
    const int64_t n = w.n, i0 = (int64_t)tile * RM_TILE;
    if (i0 >= n) return;
    const int nt = (int)(n - i0 < RM_TILE ? n - i0 : RM_TILE);
    const T *xb = x + (size_t)b * ld_in;
    float *ob = out + (size_t)b * ld_out + i0;
    const int o = tid * RM_PER, o4 = tid * (RM_PER / 4);

    float acc[RM_PER];
    if (w.r < 0) {                             // not filtered: y = x * scale, bit for bit
#pragma unroll
        for (int r = 0; r < RM_PER; ++r) acc[r] = o + r < nt ? (float)xb[i0 + o + r] * scale : 0.0f;
    } else {
#pragma unroll
        for (int r = 0; r < RM_PER; ++r) acc[r] = 0.0f;
        const float *h = rir + (size_t)w.r * ld_r;
        const int K = w.K;
        for (int c = (K - 1) / RM_KC; c >= 0; --c) {
            const int k0 = c * RM_KC;
            __syncthreads();                   // the previous chunk has been read
            for (int q = tid; q < RM_KC; q += RM_THREADS) {
                const int k = k0 + RM_KC - 1 - q;
                s_h[q] = k < K ? h[k] : 0.0f;
            }
            const int64_t base = i0 + w.p - k0 - (RM_KC - 1);
            for (int j = tid; j < RM_SX; j += RM_THREADS) {
                const int64_t idx = base + j;
                s_x[rm_phys(j)] = (idx >= 0 && idx < n) ? (float)xb[idx] * scale : 0.0f;
            }
            __syncthreads();
            const int valid = K - k0 < RM_KC ? K - k0 : RM_KC;
            int q4 = ((RM_KC - valid) / 12) * 3;          // the chunk's zero taps lie at its low end: skip whole turns
            f32x4 wa = s_x4[rm_quad(o4 + q4)], wb = s_x4[rm_quad(o4 + q4 + 1)], wc;
            for (; q4 < RM_KC / 4; q4 += 3) {  // in words every index stays under RM_SX: o + q + 19 <= 2040 + 372 + 19
                wc = s_x4[rm_quad(o4 + q4 + 2)];
                rm_fma(acc, wa, wb, wc, s_h4[q4]);
                wa = s_x4[rm_quad(o4 + q4 + 3)];
                rm_fma(acc, wb, wc, wa, s_h4[q4 + 1]);
                wb = s_x4[rm_quad(o4 + q4 + 4)];
                rm_fma(acc, wc, wa, wb, s_h4[q4 + 2]);
            }
        }
    }

    // the tile's share of Ps, Py, Pv in float64: lane order, then wave order
    double ps = 0.0, py = 0.0, pv = 0.0;
    const T *vb = v + (size_t)b * ld_v;
    unsigned vc = 0;
    const unsigned m = (unsigned)w.m;
    if (m > 0 && o < nt) vc = (unsigned)((uint64_t)(i0 + o) % m);
#pragma unroll
    for (int r = 0; r < RM_PER; ++r) {
        if (o + r < nt) {
            const float s = w.r < 0 ? acc[r] : (float)xb[i0 + o + r] * scale;
            ps += (double)s * (double)s;
            py += (double)acc[r] * (double)acc[r];
            if (m > 0) {
                const float vv = (float)vb[vc] * scale;
                pv += (double)vv * (double)vv;
                if (++vc == m) vc = 0;
            }
        }
    }
    if (VEC && o + RM_PER <= nt) {
        *reinterpret_cast<f32x4 *>(ob + o) = f32x4{acc[0], acc[1], acc[2], acc[3]};
        *reinterpret_cast<f32x4 *>(ob + o + 4) = f32x4{acc[4], acc[5], acc[6], acc[7]};
    } else {
#pragma unroll
        for (int r = 0; r < RM_PER; ++r)
            if (o + r < nt) ob[o + r] = acc[r];
    }
    ps = rm_wave_sum(ps), py = rm_wave_sum(py), pv = rm_wave_sum(pv);
    if ((tid & 63) == 0) s_red[tid >> 6][0] = ps, s_red[tid >> 6][1] = py, s_red[tid >> 6][2] = pv;
    __syncthreads();
    if (tid < 3) {
        double t = s_red[0][tid];
#pragma unroll
        for (int q = 1; q < RM_THREADS / 64; ++q) t += s_red[q][tid];
        ws[((size_t)b * tiles + tile) * 3 + tid] = t;
    }
}

template <typename T, bool VEC>
__global__ __launch_bounds__(RM_THREADS) void reverb_mix_kernel(
    const T *__restrict__ v, int64_t ld_v, float *__restrict__ out, int64_t ld_out, int64_t ld_in, int64_t ld_r,
    const int64_t *__restrict__ n_rows, const int64_t *__restrict__ m_rows, const int32_t *__restrict__ rir_idx,
    const int32_t *__restrict__ rir_len, const int32_t *__restrict__ rir_peak, int R,
    const float *__restrict__ snr_lin, int tiles, float scale, int use, const double *__restrict__ ws) {
    __shared__ double s_p[3];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
    const RmRow w = rm_row(b, n_rows, m_rows, rir_idx, rir_len, rir_peak, R, ld_in, ld_out, ld_v, ld_r, tiles, use);
    const int64_t n = w.n, i0 = (int64_t)tile * RM_TILE;
    if (i0 >= n) return;
    if (w.r < 0 && w.m == 0) return;
    if (tid < 3) {                             // the row's sums: its tiles' partials in tile order
        const int nt_row = (int)((n + RM_TILE - 1) / RM_TILE);
        const double *p = ws + (size_t)b * tiles * 3 + tid;
        double t = 0.0;
        for (int q = 0; q < nt_row; ++q) t += p[(size_t)q * 3];
        s_p[tid] = t;
    }
    __syncthreads();
    const double Ps = s_p[0], Py = s_p[1], Pv = s_p[2];
    float a = 1.0f, g = 0.0f;
    if (w.r >= 0 && Py > 0.0) a = (float)fmin(sqrt(Ps / Py), (double)FLT_MAX);
    if (w.m > 0 && Pv > 0.0 && Ps > 0.0) {
        const double snr = (double)snr_lin[b];
        if (snr > 0.0 && snr <= (double)FLT_MAX) g = (float)fmin(sqrt(Ps / (Pv * snr)), (double)FLT_MAX);
    }
    if (a == 1.0f && g == 0.0f) return;
    const int nt = (int)(n - i0 < RM_TILE ? n - i0 : RM_TILE);
    float *ob = out + (size_t)b * ld_out + i0;
    const T *vb = v + (size_t)b * ld_v;
    const unsigned m = g != 0.0f ? (unsigned)w.m : 0u;
    for (int e = tid * 4; e < nt; e += RM_THREADS * 4) {
        unsigned vc = m > 0 ? (unsigned)((uint64_t)(i0 + e) % m) : 0u;
        float y[4];
        const bool full = VEC && e + 4 <= nt;
        if (full) {
            const f32x4 t = *reinterpret_cast<const f32x4 *>(ob + e);
            y[0] = t[0], y[1] = t[1], y[2] = t[2], y[3] = t[3];
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) y[q] = e + q < nt ? ob[e + q] : 0.0f;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float t = a * y[q];
            if (m > 0 && e + q < nt) {
                t = t + g * ((float)vb[vc] * scale);
                if (++vc == m) vc = 0;
            }
            y[q] = t;
        }
        if (full) {
            *reinterpret_cast<f32x4 *>(ob + e) = f32x4{y[0], y[1], y[2], y[3]};
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (e + q < nt) ob[e + q] = y[q];
        }
    }
}

static inline int64_t rm_tiles(int64_t n_max) { return n_max <= 0 ? 0 : asrk_div_up64(n_max, RM_TILE); }

extern "C" size_t asrk_reverb_mix_ws_bytes(int B, int64_t n_max) {
    if (B <= 0 || n_max <= 0) return 0;
    return (size_t)B * (size_t)rm_tiles(n_max) * 3 * sizeof(double);
}

static bool rm_overlap(const void *a, size_t abytes, const void *b, size_t bbytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a && b && a0 < b0 + bbytes && b0 < a0 + abytes;
}

extern "C" int asrk_reverb_mix_f32(const void *x, int sample_bytes, int64_t ld_in, const int64_t *n_host,
                                   const int64_t *n_dev, const float *rir, int64_t ld_r, const int32_t *rir_len_host,
                                   const int32_t *rir_len_dev, const int32_t *rir_peak_host,
                                   const int32_t *rir_peak_dev, int R, const int32_t *rir_idx_host,
                                   const int32_t *rir_idx_dev, const void *v, int64_t ld_v, const int64_t *m_host,
                                   const int64_t *m_dev, const float *snr_lin_dev, int B, float *out, int64_t ld_out,
                                   float scale, void *ws, size_t ws_bytes, void *stream) {
    if (B < 0 || R < 0 || ld_in < 0 || ld_out < 0 || ld_v < 0 || ld_r < 0) return ASRK_ESHAPE;
    if (ld_in > 0x7fffffff || ld_out > 0x7fffffff || ld_v > 0x7fffffff) return ASRK_ESHAPE;
    if (sample_bytes != 2 && sample_bytes != 4) return ASRK_ESHAPE;
    if (R > 0 && (!rir_len_host || !rir_peak_host)) return ASRK_ESHAPE;
    for (int r = 0; r < R; ++r) {
        const int K = rir_len_host[r], p = rir_peak_host[r];
        if (K < 1 || K > RM_MAX_TAPS || K > ld_r || p < 0 || p > K - 1) return ASRK_ESHAPE;
    }
    if (B == 0) return ASRK_OK;
    if (!n_host || !rir_idx_host || !m_host) return ASRK_ESHAPE;
    int64_t n_max = 0, work = 0;
    int use = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t n = n_host[b], m = m_host[b];
        const int r = rir_idx_host[b];
        if (n < 0 || n > ld_in || n > ld_out || m < 0 || m > ld_v || r < -1 || r >= R) return ASRK_ESHAPE;
        n_max = n > n_max ? n : n_max;
        work += n;
        if (n > 0 && r >= 0) use |= RM_USE_RIR;
        if (n > 0 && m > 0) use |= RM_USE_NOISE;
    }
    if (out && (rm_overlap(out, (size_t)B * ld_out * sizeof(float), x, (size_t)B * ld_in * sample_bytes) ||
                rm_overlap(out, (size_t)B * ld_out * sizeof(float), v, (size_t)B * ld_v * sample_bytes)))
        return ASRK_ESHAPE;
    if (work == 0) return ASRK_OK;
    if (!x || !out || !n_dev || !rir_idx_dev || !m_dev) return ASRK_ESHAPE;
    if ((use & RM_USE_RIR) && (!rir || !rir_len_dev || !rir_peak_dev)) return ASRK_ESHAPE;
    if ((use & RM_USE_NOISE) && (!v || !snr_lin_dev)) return ASRK_ESHAPE;
    const int64_t tiles = rm_tiles(n_max);
    if ((int64_t)B * tiles > 0x7fffffff) return ASRK_ESHAPE;
    if (!ws || ws_bytes < asrk_reverb_mix_ws_bytes(B, n_max)) return ASRK_EWORKSPACE;
    if ((uintptr_t)ws & 7) return ASRK_ESHAPE;
    hipStream_t s = (hipStream_t)stream;
    const bool vec = ld_out % 4 == 0 && ((uintptr_t)out & 15) == 0;
    const dim3 grid((unsigned)(B * tiles)), block(RM_THREADS);
    double *wsd = reinterpret_cast<double *>(ws);
    asrk_prof_begin_(PROF_FBANK, s);
#define ASRK_RM_CONV(T_, V_)                                                                                           \
    hipLaunchKernelGGL((reverb_conv_kernel<T_, V_>), grid, block, 0, s, reinterpret_cast<const T_ *>(x), ld_in,        \
                       reinterpret_cast<const T_ *>(v), ld_v, out, ld_out, rir, ld_r, n_dev, m_dev, rir_idx_dev,       \
                       rir_len_dev, rir_peak_dev, R, (int)tiles, scale, use, wsd)
#define ASRK_RM_MIX(T_, V_)                                                                                            \
    hipLaunchKernelGGL((reverb_mix_kernel<T_, V_>), grid, block, 0, s, reinterpret_cast<const T_ *>(v), ld_v, out,     \
                       ld_out, ld_in, ld_r, n_dev, m_dev, rir_idx_dev, rir_len_dev, rir_peak_dev, R, snr_lin_dev,      \
                       (int)tiles, scale, use, wsd)
    if (sample_bytes == 2) {
        if (vec) ASRK_RM_CONV(int16_t, true);
        else ASRK_RM_CONV(int16_t, false);
    } else {
        if (vec) ASRK_RM_CONV(float, true);
        else ASRK_RM_CONV(float, false);
    }
    if (use) {                                 // no response and no noise anywhere: launch 1 wrote the result
        if (sample_bytes == 2) {
            if (vec) ASRK_RM_MIX(int16_t, true);
            else ASRK_RM_MIX(int16_t, false);
        } else {
            if (vec) ASRK_RM_MIX(float, true);
            else ASRK_RM_MIX(float, false);
        }
    }
#undef ASRK_RM_CONV
#undef ASRK_RM_MIX
    asrk_prof_end_(PROF_FBANK, s);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}
