// Back-off n-gram LM step for shallow fusion (src/ngram.py: NGramLM): one workgroup per row.
//
// Thread 0 walks the trie (ngram.inc: advance the row's state by its token, collect the back-off chain of the new
// state - a few dependent loads), then all threads expand the row in place in global memory: the unigram level
// shifted by the whole chain's back-off sum (16-byte loads and stores where the row allows them), and, context by
// context from the shortest to the longest with a workgroup barrier in between, the explicit entries on top - so
// the longest context that holds a word decides its value.  The row is NOT staged in LDS: the fill is a pure
// stream (R * V * 4 bytes written once) and the overwrites touch a few hundred words of lines this workgroup has
// just written; a staged row would need V * 4 bytes of LDS per workgroup (64 KB at V = 16000: two workgroups per
// CU) and a size limit with a second variant behind it.  One variant, no size limit.
// A row's result depends on the image and its own (state, token) only: no atomics, one fixed order of f32 adds.
#include "common.h"

#define NG_HD __device__
#include "ngram.inc"

#define NG_THREADS 256

template <typename PT>
__global__ __launch_bounds__(NG_THREADS) void ngram_step_kernel(NGImage g, const int *__restrict__ state_in,
                                                                int n_state, const long long *__restrict__ token,
                                                                const PT *__restrict__ parent, int *__restrict__ state_out,
                                                                float *__restrict__ out, long long ld) {
    __shared__ int s_c[NG_MAX_ORDER];
    __shared__ float s_B[NG_MAX_ORDER];
    __shared__ int s_d;
    const int r = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) {
        int s = 0;
        if (state_in) {
            const long long p = parent ? (long long)parent[r] : (long long)r;
            if (p >= 0 && p < n_state) s = state_in[p];
        }
        s = ng_advance(g, s, token[r]);
        state_out[r] = s;
        s_d = ng_chain(g, s, s_c, s_B);
    }
    __syncthreads();
    const int d = s_d, V = g.V;
    float *row = out + (long long)r * ld;
    const float Bd = s_B[d];
    if (((((uintptr_t)row) | ((uintptr_t)g.uni_logp)) & 15) == 0) {
        const f32x4 *u4 = reinterpret_cast<const f32x4 *>(g.uni_logp);
        f32x4 *r4 = reinterpret_cast<f32x4 *>(row);
        const int n4 = V >> 2;
        for (int i = tid; i < n4; i += NG_THREADS) {
            f32x4 u = u4[i];
            u.x = Bd + u.x; u.y = Bd + u.y; u.z = Bd + u.z; u.w = Bd + u.w;
            r4[i] = u;
        }
        for (int v = (n4 << 2) + tid; v < V; v += NG_THREADS) row[v] = Bd + g.uni_logp[v];
    } else {
        for (int v = tid; v < V; v += NG_THREADS) row[v] = Bd + g.uni_logp[v];
    }
    for (int k = d - 1; k >= 0; --k) {
        __syncthreads();                                   // the level below is in place: this one overwrites it
        const int c = s_c[k];
        const float Bk = s_B[k];
        int lo = g.child_off[c], hi = g.child_off[c + 1];
        if (lo < 0) lo = 0;
        if (hi > g.n_entries) hi = g.n_entries;
        for (int e = lo + tid; e < hi; e += NG_THREADS) {
            const int w = g.word[e];
            if (w >= 0 && w < V) row[w] = Bk + g.logp[e];
        }
    }
}

extern "C" int asrk_ngram_step_f32(int order, int V, int n_nodes, int n_entries, const float *uni_logp,
                                   const int32_t *uni_next, const float *bo, const int32_t *fail,
                                   const int32_t *child_off, const int32_t *word, const float *logp,
                                   const int32_t *next, const int32_t *state_in, int n_state, const int64_t *token,
                                   const void *parent, int parent_is_i64, int32_t *state_out, float *out,
                                   int64_t row_stride, int R, void *stream) {
    if (order < 1 || order > NG_MAX_ORDER || V <= 0 || n_nodes < 1 || n_entries < 0 || R < 0 || n_state < 0)
        return ASRK_EINVAL;
    if (!uni_logp || !uni_next || !bo || !fail || !child_off) return ASRK_EINVAL;
    if (n_entries > 0 && (!word || !logp || !next)) return ASRK_EINVAL;
    if (row_stride < V) return ASRK_EINVAL;
    if (R == 0) return ASRK_OK;
    if (!token || !state_out || !out || (const void *)state_out == (const void *)state_in) return ASRK_EINVAL;
    if (state_in && n_state == 0) return ASRK_EINVAL;
    NGImage g{order, V, n_nodes, n_entries, uni_logp, uni_next, bo, fail, child_off, word, logp, next};
    hipStream_t s = (hipStream_t)stream;
    const long long *tok = reinterpret_cast<const long long *>(token);
    if (parent && parent_is_i64)
        hipLaunchKernelGGL(ngram_step_kernel<long long>, dim3(R), dim3(NG_THREADS), 0, s, g, state_in, n_state, tok,
                           reinterpret_cast<const long long *>(parent), state_out, out, (long long)row_stride);
    else
        hipLaunchKernelGGL(ngram_step_kernel<int>, dim3(R), dim3(NG_THREADS), 0, s, g, state_in, n_state, tok,
                           reinterpret_cast<const int *>(parent), state_out, out, (long long)row_stride);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}
