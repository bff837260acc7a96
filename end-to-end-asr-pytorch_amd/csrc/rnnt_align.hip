// RNN-transducer forced alignment for gfx950 (ops.rnnt_align, TransducerHead.align): the best (Viterbi) path of every
// utterance through its lattice, found and traced back on the device in one launch.
//
//   asrk_rnnt_align_ws_bytes   the workspace of a call: the backpointers on the global route, 0 on the LDS route.
//   asrk_rnnt_align_f32        lattice, backtrace and per-token outputs.
//
// Recurrence (rnnt_align.inc, the source the host build of the tests compiles too), on the lpb / lpl [B,T,U1] arrays
// of asrk_rnnt_rows_f32, lengths clamped as everywhere in the transducer kernels:
//   delta(0,0) = 0;  a = delta(t-1,u) + lpb(t-1,u);  b = delta(t,u-1) + lpl(t,u-1)   (-inf where the arc does not exist)
//   the label arc is taken iff (b > a) or (b != b);  delta(t,u) = taken ? b : a;  score = delta(T_b-1,U_b) + lpb(T_b-1,U_b)
// plain f32, one add per arc and one compare per cell: a host f32 computation in this order gives the same bits.
// Tie rule: the blank arc, so among equal-scoring paths every label is emitted as early as possible.  A NaN on either
// arc reaches the score.
// Walk: one 128-lane workgroup per utterance over the T_b + U_b anti-diagonals (rnnt_walk's order), the previous
// diagonal in LDS, one barrier per diagonal.  Lane l of a wave owns the cells u = 64 k + l, so the backpointers - one
// bit per cell - are one __ballot per wave: the 64-bit word (d, u >> 6) of (T + U1 - 1) * ceil(U1 / 64) words, written
// by the wave's lane 0.
// Routes (flags = ASRK_ALIGN_BP_*): LDS holds the words behind the two diagonals when they fit RA_LDS_BP_BUDGET =
// 128 KiB (the diagonals add at most 16 KiB; a CU has 160 KiB); GLOBAL keeps them in the caller's workspace; AUTO takes
// LDS where it fits.
// Backtrace, same launch: lane 0 follows the bits back from (T_b-1, U_b), one dependent 8-byte read per step, and
// stores frames / labels_done; after a barrier all lanes gather tok_logp, compute tok_post (rnnt_coef's el at the
// emitting cell) and write the padding.  Cells outside an utterance's lattice are never read.
// Errors, all before any device call: ASRK_EINVAL for a NULL pointer, a negative B, T or U1 <= 0, unknown flags, only
// some of alpha / beta / nll (or those without tok_post), a NULL, misaligned or short workspace on the global route;
// ASRK_ESHAPE for U1 > 2048, B*T*U1 > INT32_MAX or a forced LDS route that does not fit.  B == 0: ASRK_OK, no launch.
// wave64, no float atomics: every output is a pure function of the inputs, reproducible bit for bit.
#include "rnnt_rows.h"
#include "rnnt_align.inc"

namespace {

constexpr int RA_THREADS = 128;                      // two waves: the lanes of one direction of the loss lattice
constexpr int RA_MAX_U1 = 2048;                      // as asrk_rnnt_lattice_f32
constexpr size_t RA_LDS_BP_BUDGET = 128 * 1024;      // bytes of LDS backpointers per utterance

struct RaArgs {
    const float *lpb, *lpl;           // [B, T, U1]
    const int64_t *enc_len, *txt_len;
    int T, U1;
    const float *alpha, *beta, *nll;  // all three or none
    int32_t *frames;                  // [B, U1 - 1]
    int32_t *labels_done;             // [B, T]
    float *tok_logp, *tok_post;       // [B, U1 - 1]
    float *score;                     // [B]
    unsigned long long *bp;           // global route: [B, T + U1 - 1, nslot]
    int64_t *stamps;                  // optional [B, 4]: wall_clock64 at start / lattice done / backtrace done / end
};

struct RaSync {
    __device__ __forceinline__ void operator()() const { __syncthreads(); }
};

// every lane of the wave calls it (rnnt_align_diag); lane 0 stores the wave's word
struct RaBallotPut {
    unsigned long long *bp;
    int nslot;
    __device__ __forceinline__ void operator()(int d, int u, bool taken) const {
        const unsigned long long w = __ballot(taken);
        if ((threadIdx.x & 63) == 0) bp[(size_t)d * nslot + (u >> 6)] = w;
    }
};

static inline size_t ra_rows_bytes(int U1) { return ((size_t)2 * U1 * sizeof(float) + 15) & ~(size_t)15; }
// host side of rnnt_align_nslot: (T + U1 - 1) diagonals of ceil(U1 / 64) words
static inline size_t ra_bp_words(int T, int U1) { return (size_t)(T + U1 - 1) * (size_t)((U1 + 63) >> 6); }

template <bool BP_LDS>
__global__ __launch_bounds__(RA_THREADS) void rnnt_align_kernel(RaArgs a, int rows_bytes) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ float s_score;
    float *diag = reinterpret_cast<float *>(smem);   // [2][U1]
    const int b = blockIdx.x, tid = threadIdx.x;
    const int T = a.T, U1 = a.U1;
    const int Tb = rnnt_clamp_T(a.enc_len[b], T), Ub = rnnt_clamp_U(a.txt_len[b], U1);
    const int nslot = rnnt_align_nslot(U1);
    const size_t off = (size_t)b * T * U1;
    const float *lpb = a.lpb + off, *lpl = a.lpl + off;
    unsigned long long *bp = BP_LDS ? reinterpret_cast<unsigned long long *>(smem + rows_bytes)
                                    : a.bp + (size_t)b * (T + U1 - 1) * nslot;
    int64_t *stamp = a.stamps ? a.stamps + (size_t)b * 4 : nullptr;
    if (stamp && tid == 0) stamp[0] = (int64_t)wall_clock64();

    rnnt_align_walk(tid, RA_THREADS, Tb, Ub, U1, lpb, lpl, diag, &s_score, RaSync(), RaBallotPut{bp, nslot});
    const float score = s_score;       // written on the last diagonal, before its barrier
    if (stamp && tid == 0) stamp[1] = (int64_t)wall_clock64();

    // a path exists only behind a score above -inf (false for NaN)
    const bool ok = score > -INFINITY;
    int32_t *frames = a.frames + (size_t)b * (U1 - 1);
    int32_t *done = a.labels_done + (size_t)b * T;
    if (ok && tid == 0) rnnt_align_backtrace(Tb, Ub, U1, bp, frames, done);
    __syncthreads();                   // what lane 0 stored is visible to the workgroup
    if (stamp && tid == 0) stamp[2] = (int64_t)wall_clock64();

    rnnt_align_tokens(tid, RA_THREADS, ok, T, Tb, Ub, U1, lpb, lpl, a.alpha ? a.alpha + off : nullptr,
                      a.alpha ? a.beta + off : nullptr, a.alpha ? a.nll[b] : 0.f, frames, done,
                      a.tok_logp + (size_t)b * (U1 - 1), a.alpha ? a.tok_post + (size_t)b * (U1 - 1) : nullptr);
    if (tid == 0) {
        a.score[b] = score;
        if (stamp) stamp[3] = (int64_t)wall_clock64();
    }
}

// 0 = bad flags / a forced LDS route that does not fit, else ASRK_ALIGN_BP_LDS or ASRK_ALIGN_BP_GLOBAL
static int ra_route(int T, int U1, int flags) {
    const bool fits = ra_bp_words(T, U1) * sizeof(unsigned long long) <= RA_LDS_BP_BUDGET;
    if (flags == ASRK_ALIGN_BP_AUTO) return fits ? ASRK_ALIGN_BP_LDS : ASRK_ALIGN_BP_GLOBAL;
    if (flags == ASRK_ALIGN_BP_LDS) return fits ? ASRK_ALIGN_BP_LDS : 0;
    return flags == ASRK_ALIGN_BP_GLOBAL ? ASRK_ALIGN_BP_GLOBAL : 0;
}

static inline bool ra_shape_ok(int B, int T, int U1) {
    return B > 0 && T > 0 && U1 > 0 && U1 <= RA_MAX_U1 && (int64_t)B * T * U1 <= (int64_t)INT32_MAX;
}

}  // namespace

extern "C" size_t asrk_rnnt_align_ws_bytes(int B, int T, int U1, int flags) {
    if (!ra_shape_ok(B, T, U1)) return 0;
    if (ra_route(T, U1, flags) != ASRK_ALIGN_BP_GLOBAL) return 0;
    return (size_t)B * ra_bp_words(T, U1) * sizeof(unsigned long long);
}

extern "C" int asrk_rnnt_align_f32(const float *lpb, const float *lpl, const int64_t *enc_len, const int64_t *txt_len,
                                   int B, int T, int U1, int flags, const float *alpha, const float *beta,
                                   const float *nll, int32_t *frames, int32_t *labels_done, float *tok_logp,
                                   float *tok_post, float *score, int64_t *stamps, void *ws, size_t ws_bytes,
                                   void *stream) {
    if (B < 0 || T <= 0 || U1 <= 0) return ASRK_EINVAL;
    if (flags != ASRK_ALIGN_BP_AUTO && flags != ASRK_ALIGN_BP_LDS && flags != ASRK_ALIGN_BP_GLOBAL)
        return ASRK_EINVAL;
    if (U1 > RA_MAX_U1 || (int64_t)B * T * U1 > (int64_t)INT32_MAX) return ASRK_ESHAPE;
    if (B == 0) return ASRK_OK;
    if (!lpb || !lpl || !enc_len || !txt_len || !labels_done || !score) return ASRK_EINVAL;
    if (U1 > 1 && (!frames || !tok_logp)) return ASRK_EINVAL;
    const int n_lat = (alpha != nullptr) + (beta != nullptr) + (nll != nullptr);
    if (n_lat != 0 && n_lat != 3) return ASRK_EINVAL;
    if (n_lat == 3 && U1 > 1 && !tok_post) return ASRK_EINVAL;
    const int route = ra_route(T, U1, flags);
    if (!route) return ASRK_ESHAPE;       // a forced LDS route whose backpointers do not fit the budget
    const size_t need = route == ASRK_ALIGN_BP_GLOBAL ? (size_t)B * ra_bp_words(T, U1) * sizeof(unsigned long long) : 0;
    if (need > 0 && (!ws || ((uintptr_t)ws & 15) || ws_bytes < need)) return ASRK_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    RaArgs a{};
    a.lpb = lpb, a.lpl = lpl, a.enc_len = enc_len, a.txt_len = txt_len, a.T = T, a.U1 = U1;
    if (n_lat == 3) a.alpha = alpha, a.beta = beta, a.nll = nll, a.tok_post = tok_post;
    a.frames = frames, a.labels_done = labels_done, a.tok_logp = tok_logp, a.score = score;
    a.bp = need ? static_cast<unsigned long long *>(ws) : nullptr;
    a.stamps = stamps;
    const size_t rows = ra_rows_bytes(U1);
    asrk_prof_begin_(PROF_CTC, s);   // the lattice family
    if (route == ASRK_ALIGN_BP_LDS) {
        static AsrkLdsLatch latch;
        ASRK_HIP(asrk_max_lds_once(latch, reinterpret_cast<const void *>(rnnt_align_kernel<true>),
                                   (int)(ra_rows_bytes(RA_MAX_U1) + RA_LDS_BP_BUDGET)));
        const size_t lds = rows + ra_bp_words(T, U1) * sizeof(unsigned long long);
        hipLaunchKernelGGL((rnnt_align_kernel<true>), dim3(B), dim3(RA_THREADS), lds, s, a, (int)rows);
    } else {
        hipLaunchKernelGGL((rnnt_align_kernel<false>), dim3(B), dim3(RA_THREADS), rows, s, a, (int)rows);
    }
    asrk_prof_end_(PROF_CTC, s);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}
