// Speed perturbation on the padded PCM batch: polyphase windowed-sinc resampling of every row by its own rational
// ratio, x [B, ld_in] (int16 or f32) -> y [B, ld_out] f32, in one pass over HBM (semantics: include/asrk.h,
// asrk_resample_rows_f32).  The tap tables are the caller's (src/audio.py builds them in float64); the kernel is a pure
// function of (x, n, ratio index, tables).
//
// One workgroup = one row x one tile of `it` input steps = it * new consecutive outputs (it is a multiple of 4 chosen so
// that a tile holds about RS_TILE_OUT outputs: every tile starts on a 16-byte boundary of its row).  Prologue: the
// ratio's whole tap table goes to LDS (row stride padded to an odd number of floats), then the tile's input span plus
// halo, converted to f32 and scaled ONCE, zero outside the row.  Body: a thread owns 4 consecutive outputs; when they
// share their input step (the common case: new >= 4) each input sample is read from LDS once for the four.  16-byte
// stores when the rows allow it, one element per store otherwise and at a row's ragged end.  Rows of ratio 1:1 take no
// filter: their tiles are a scaled copy.
#include "common.h"

#define RS_THREADS 256
#define RS_TILE_OUT 2048                       // outputs per tile, about (exactly for 1:1 rows)
#define RS_MAX_RATIOS 8
#define RS_MAX_TERM 100                        // orig, new <= 100
#define RS_LOWPASS_WIDTH 6
#define RS_MAX_LDS (64 * 1024)

struct RsRatios {                              // by value: the kernel's view of the (at most 8) ratios of a call
    const float *h[RS_MAX_RATIOS];             // taps [nw][taps], NULL for 1:1
    int orig[RS_MAX_RATIOS], nw[RS_MAX_RATIOS], width[RS_MAX_RATIOS], it[RS_MAX_RATIOS];
    int count;
};

static inline int rs_tile_steps(int nw) {      // input steps per tile: a multiple of 4, >= 4
    const int it = (RS_TILE_OUT / nw) & ~3;
    return it < 4 ? 4 : it;
}

// width = ceil(W * orig / (min(orig, new) * 0.99)) in integers: ceil(100 * W * orig / (99 * min))
static inline int rs_width(int orig, int nw) {
    const int mn = orig < nw ? orig : nw;
    return (100 * RS_LOWPASS_WIDTH * orig + 99 * mn - 1) / (99 * mn);
}

template <typename T, bool VEC>
__global__ __launch_bounds__(RS_THREADS) void resample_rows_kernel(const T *__restrict__ x, int64_t ld_in,
                                                                   float *__restrict__ y, int64_t ld_out,
                                                                   const int64_t *__restrict__ n_rows,
                                                                   const int32_t *__restrict__ ratio_idx, int tiles,
                                                                   float scale, RsRatios R) {
    extern __shared__ __attribute__((aligned(16))) float rs_smem[];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
    const int r = ratio_idx[b];
    if (r < 0 || r >= R.count) return;         // the host checked its copy of the indices; this one is not trusted
    int64_t n = n_rows[b];
    n = n < 0 ? 0 : (n > ld_in ? ld_in : n);
    const int orig = R.orig[r], nw = R.nw[r];
    int64_t n_out = ((int64_t)nw * n + orig - 1) / orig;
    if (n_out > ld_out) n_out = ld_out;
    const T *xb = x + (size_t)b * ld_in;
    float *yb = y + (size_t)b * ld_out;

    if (orig == 1 && nw == 1) {                // not filtered: y = x * scale, bit for bit
        const int64_t o0 = (int64_t)tile * RS_TILE_OUT;
        const int nt = n_out <= o0 ? 0 : (int)(n_out - o0 < RS_TILE_OUT ? n_out - o0 : RS_TILE_OUT);
        for (int g = tid * 4; g < nt; g += RS_THREADS * 4) {
            const T *xp = xb + o0 + g;
            if (VEC && g + 4 <= nt) {
                *reinterpret_cast<f32x4 *>(yb + o0 + g) =
                    f32x4{(float)xp[0] * scale, (float)xp[1] * scale, (float)xp[2] * scale, (float)xp[3] * scale};
            } else {
                for (int q = 0; q < 4 && g + q < nt; ++q) yb[o0 + g + q] = (float)xp[q] * scale;
            }
        }
        return;
    }

    const int it = R.it[r], width = R.width[r];
    const int64_t i0 = (int64_t)tile * it, o0 = i0 * nw;
    if (o0 >= n_out) return;
    const int nt = (int)(n_out - o0 < (int64_t)it * nw ? n_out - o0 : (int64_t)it * nw);
    const int taps = 2 * width + orig, hs = taps | 1;
    float *s_h = rs_smem;                                       // [nw][hs]
    float *s_x = rs_smem + ((nw * hs + 3) & ~3);                // [(it - 1) * orig + taps]
    const float *h = R.h[r];
    for (int e = tid; e < nw * taps; e += RS_THREADS) {
        const int j = e / taps;
        s_h[j * hs + (e - j * taps)] = h[e];
    }
    const int span = (it - 1) * orig + taps;
    const int64_t x0 = i0 * orig - width;
    for (int s = tid; s < span; s += RS_THREADS) {
        const int64_t idx = x0 + s;
        s_x[s] = (idx >= 0 && idx < n) ? (float)xb[idx] * scale : 0.0f;
    }
    __syncthreads();

    // it * nw is a multiple of 4, so the four outputs of a group all lie inside the tile's it steps (whether the row
    // still has them or not): every LDS index below stays inside s_h / s_x
    for (int g = tid * 4; g < nt; g += RS_THREADS * 4) {
        int i = g / nw, j = g - i * nw;
        int xo[4], ho[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            xo[q] = i * orig, ho[q] = j * hs;
            if (++j == nw) j = 0, ++i;
        }
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
        const float *h0 = s_h + ho[0], *h1 = s_h + ho[1], *h2 = s_h + ho[2], *h3 = s_h + ho[3];
        if (xo[0] == xo[3]) {
            const float *xp = s_x + xo[0];
#pragma unroll 4
            for (int k = 0; k < taps; ++k) {
                const float xv = xp[k];
                a0 = fmaf(h0[k], xv, a0);
                a1 = fmaf(h1[k], xv, a1);
                a2 = fmaf(h2[k], xv, a2);
                a3 = fmaf(h3[k], xv, a3);
            }
        } else {
            const float *x0p = s_x + xo[0], *x1p = s_x + xo[1], *x2p = s_x + xo[2], *x3p = s_x + xo[3];
#pragma unroll 4
            for (int k = 0; k < taps; ++k) {
                a0 = fmaf(h0[k], x0p[k], a0);
                a1 = fmaf(h1[k], x1p[k], a1);
                a2 = fmaf(h2[k], x2p[k], a2);
                a3 = fmaf(h3[k], x3p[k], a3);
            }
        }
        float *yp = yb + o0 + g;
        if (VEC && g + 4 <= nt) {
            *reinterpret_cast<f32x4 *>(yp) = f32x4{a0, a1, a2, a3};
        } else {
            const float a[4] = {a0, a1, a2, a3};
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (g + q < nt) yp[q] = a[q];
        }
    }
}

extern "C" int asrk_resample_rows_f32(const void *x, int sample_bytes, int64_t ld_in, const int64_t *n_host,
                                      const int64_t *n_dev, const int32_t *ratio_idx_host,
                                      const int32_t *ratio_idx_dev, int B, const int32_t *ratios_host,
                                      const float *const *taps_host, int n_ratios, float *y, int64_t ld_out,
                                      float scale, void *stream) {
    if (B < 0 || ld_in < 0 || ld_out < 0 || n_ratios < 0 || n_ratios > RS_MAX_RATIOS) return ASRK_ESHAPE;
    if (sample_bytes != 2 && sample_bytes != 4) return ASRK_ESHAPE;
    if (x && x == (const void *)y) return ASRK_ESHAPE;
    if (B == 0) return ASRK_OK;
    if (!n_host || !ratio_idx_host || !ratios_host || !taps_host) return ASRK_ESHAPE;
    RsRatios R;
    R.count = n_ratios;
    size_t lds = 0;
    for (int r = 0; r < RS_MAX_RATIOS; ++r) {
        R.h[r] = nullptr, R.orig[r] = R.nw[r] = 1, R.width[r] = 0, R.it[r] = RS_TILE_OUT;
        if (r >= n_ratios) continue;
        const int orig = ratios_host[2 * r], nw = ratios_host[2 * r + 1];
        if (orig < 1 || nw < 1 || orig > RS_MAX_TERM || nw > RS_MAX_TERM || orig > 2 * nw || nw > 2 * orig)
            return ASRK_ESHAPE;
        for (int a = orig, c = nw; c != 0;) {                   // coprime
            const int t = a % c;
            a = c, c = t;
            if (c == 0 && a != 1) return ASRK_ESHAPE;
        }
        R.orig[r] = orig, R.nw[r] = nw;
        if (orig == 1 && nw == 1) continue;
        R.h[r] = taps_host[r], R.width[r] = rs_width(orig, nw), R.it[r] = rs_tile_steps(nw);
        const int taps = 2 * R.width[r] + orig;
        const size_t need = (size_t)(((nw * (taps | 1) + 3) & ~3) + (R.it[r] - 1) * orig + taps) * sizeof(float);
        if (need > lds) lds = need;
    }
    if (lds > RS_MAX_LDS) return ASRK_ESHAPE;                   // cannot happen inside the limits above
    int64_t tiles = 0, work = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t n = n_host[b];
        const int r = ratio_idx_host[b];
        if (n < 0 || n > ld_in || r < 0 || r >= n_ratios) return ASRK_ESHAPE;
        const int64_t n_out = ((int64_t)R.nw[r] * n + R.orig[r] - 1) / R.orig[r];
        if (n_out > ld_out) return ASRK_ESHAPE;
        if (n_out > 0 && !(R.orig[r] == 1 && R.nw[r] == 1) && !R.h[r]) return ASRK_ESHAPE;
        const int64_t t = asrk_div_up64(n_out, (int64_t)R.it[r] * R.nw[r]);
        tiles = t > tiles ? t : tiles;
        work += n_out;
    }
    if (work == 0) return ASRK_OK;
    if (!x || !y || !n_dev || !ratio_idx_dev) return ASRK_ESHAPE;
    if ((int64_t)B * tiles > 0x7fffffff) return ASRK_ESHAPE;
    hipStream_t s = (hipStream_t)stream;
    const bool vec = ld_out % 4 == 0 && ((uintptr_t)y & 15) == 0;
    const dim3 grid((unsigned)(B * tiles)), block(RS_THREADS);
    asrk_prof_begin_(PROF_FBANK, s);
#define ASRK_RS_LAUNCH(T_, V_)                                                                                     \
    hipLaunchKernelGGL((resample_rows_kernel<T_, V_>), grid, block, lds, s, reinterpret_cast<const T_ *>(x), ld_in, y, \
                       ld_out, n_dev, ratio_idx_dev, (int)tiles, scale, R)
    if (sample_bytes == 2) {
        if (vec) ASRK_RS_LAUNCH(int16_t, true);
        else ASRK_RS_LAUNCH(int16_t, false);
    } else {
        if (vec) ASRK_RS_LAUNCH(float, true);
        else ASRK_RS_LAUNCH(float, false);
    }
#undef ASRK_RS_LAUNCH
    asrk_prof_end_(PROF_FBANK, s);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}
