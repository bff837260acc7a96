// Philox4x32-10 (Salmon et al., "Parallel Random Numbers: As Easy as 1, 2, 3", SC'11) as a stateless device function,
// and the pure noise function of the dithered filterbank front end built on it.  One copy for the dropout mask
// (norm.hip) and the dither (audio.hip); oracle/regularizer_oracle.py restates the rounds in numpy and checks them
// against the paper's known-answer vectors.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ __forceinline__ void philox_round(uint32_t &c0, uint32_t &c1, uint32_t &c2, uint32_t &c3,
                                             uint32_t k0, uint32_t k1) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
}

// counter words (ctr lo, ctr hi, offset lo, offset hi), key words (seed lo, seed hi)
__device__ __forceinline__ void philox4x32_10(uint64_t ctr, uint64_t offset, uint64_t seed,
                                              uint32_t out[4]) {
    uint32_t c0 = (uint32_t)ctr, c1 = (uint32_t)(ctr >> 32);
    uint32_t c2 = (uint32_t)offset, c3 = (uint32_t)(offset >> 32);
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        philox_round(c0, c1, c2, c3, k0, k1);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// The dither noise z(key, f, j) of include/asrk.h for the four positions j = 4 g .. 4 g + 3 of frame f: the words of
// Philox4x32-10(counter = (g, f, 0, 0), key) as two Box-Muller pairs.  u1 lies in (0, 1] and u2 in [0, 1), both exact
// in f32; sincospif takes 2 u2 (exact) so that no rounded 2 pi enters the angle.  |z| <= sqrt(48 ln 2).
__device__ __forceinline__ void dither_normals(uint64_t key, uint32_t f, uint32_t g, float z[4]) {
    uint32_t r[4];
    philox4x32_10((uint64_t)g | ((uint64_t)f << 32), 0, key, r);
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const float u1 = (float)((r[2 * p] >> 8) + 1u) * 0x1p-24f;
        const float u2 = (float)(r[2 * p + 1] >> 8) * 0x1p-24f;
        const float rad = sqrtf(-2.0f * logf(u1));
        float s, c;
        sincospif(2.0f * u2, &s, &c);
        z[2 * p] = rad * c;
        z[2 * p + 1] = rad * s;
    }
}
