// Contextual biasing (phrase boosting) for the three beam searches (src/bias.py: ContextBias, BiasedNGram): one
// workgroup per row, as the n-gram step (ngram.hip) and for its reasons: the row is a pure stream written once
// (R * V * 4 bytes) followed by a few overwrites of lines this workgroup has just written, so it is NOT staged in LDS
// (no size limit, one variant).
//
// asrk_bias_step_f32: thread 0 resolves the row's parent, advances the automaton state by the row's token (ctx_bias.inc:
// one binary search + one table read) and publishes phi of the new state; all threads stream row[v] = root_arrive[v] -
// phi (16-byte accesses where the row and the table allow them); after a barrier the new state's merged entries
// overwrite their words with ext_arrive[e] - phi.  Every value is ONE f32 subtraction of two stored f32 values.
//
// asrk_ngram_bias_step_f32: the same launch walks the n-gram trie (ngram.inc) and the automaton and writes the row
// once: fill (Bd + uni[v]) + (root_arrive[v] - phi); the n-gram's levels, shortest context first, overwrite with
// (Bk + logp[e]) + (root_arrive[w] - phi); after a barrier each merged entry of the automaton state - one lane per
// word - looks its word up in the n-gram chain (longest context first: the value L(w) asrk_ngram_step_f32 writes) and
// stores L(w) + (ext_arrive[e] - phi).  No multiply in the row, no atomics, one fixed order.
//
// asrk_bias_walk: one lane per token sequence, for the residual correction of finished hypotheses.
#include "common.h"

#define NG_HD __device__
#include "ngram.inc"
#define CB_HD __device__
#include "ctx_bias.inc"

#define CB_THREADS 256

template <typename PT>
__global__ __launch_bounds__(CB_THREADS) void bias_step_kernel(CBImage b, const int *__restrict__ state_in, int n_state,
                                                               const long long *__restrict__ token,
                                                               const PT *__restrict__ parent, int *__restrict__ state_out,
                                                               float *__restrict__ out, long long ld) {
    __shared__ int s_s;
    __shared__ float s_phi;
    const int r = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) {
        int s = 0;
        if (state_in) {
            const long long p = parent ? (long long)parent[r] : (long long)r;
            if (p >= 0 && p < n_state) s = state_in[p];
        }
        float a;
        s = cb_goto(b, s, token[r], &a);
        state_out[r] = s;
        s_s = s;
        s_phi = b.phi[s];
    }
    __syncthreads();
    const int V = b.V, s = s_s;
    const float phi = s_phi;
    float *row = out + (long long)r * ld;
    if (((((uintptr_t)row) | ((uintptr_t)b.root_arrive)) & 15) == 0) {
        const f32x4 *a4 = reinterpret_cast<const f32x4 *>(b.root_arrive);
        f32x4 *r4 = reinterpret_cast<f32x4 *>(row);
        const int n4 = V >> 2;
        for (int i = tid; i < n4; i += CB_THREADS) {
            f32x4 a = a4[i];
            a.x = a.x - phi; a.y = a.y - phi; a.z = a.z - phi; a.w = a.w - phi;
            r4[i] = a;
        }
        for (int v = (n4 << 2) + tid; v < V; v += CB_THREADS) row[v] = b.root_arrive[v] - phi;
    } else {
        for (int v = tid; v < V; v += CB_THREADS) row[v] = b.root_arrive[v] - phi;
    }
    if (s == 0) return;                                    // uniform: the root has no entries
    __syncthreads();                                       // the fill is in place: the entries overwrite it
    int lo, hi;
    cb_range(b, s, &lo, &hi);
    for (int e = lo + tid; e < hi; e += CB_THREADS) {
        const int w = b.ext_word[e];
        if (w >= 0 && w < V) row[w] = b.ext_arrive[e] - phi;
    }
}

template <typename PT>
__global__ __launch_bounds__(CB_THREADS) void ngram_bias_step_kernel(NGImage g, CBImage b,
                                                                     const int *__restrict__ state_in, int n_state,
                                                                     const long long *__restrict__ token,
                                                                     const PT *__restrict__ parent,
                                                                     int *__restrict__ state_out, float *__restrict__ out,
                                                                     long long ld) {
    __shared__ int s_c[NG_MAX_ORDER];
    __shared__ float s_B[NG_MAX_ORDER];
    __shared__ int s_d, s_s;
    __shared__ float s_phi;
    const int r = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) {
        int sn = 0, sb = 0;                                // state rows are (n-gram node, automaton node) pairs
        if (state_in) {
            const long long p = parent ? (long long)parent[r] : (long long)r;
            if (p >= 0 && p < n_state) {
                sn = state_in[2 * p];
                sb = state_in[2 * p + 1];
            }
        }
        const long long tok = token[r];
        sn = ng_advance(g, sn, tok);
        float a;
        sb = cb_goto(b, sb, tok, &a);
        state_out[2 * (long long)r] = sn;
        state_out[2 * (long long)r + 1] = sb;
        s_d = ng_chain(g, sn, s_c, s_B);
        s_s = sb;
        s_phi = b.phi[sb];
    }
    __syncthreads();
    const int d = s_d, V = g.V, sb = s_s;
    const float phi = s_phi, Bd = s_B[d];
    float *row = out + (long long)r * ld;
    if (((((uintptr_t)row) | ((uintptr_t)g.uni_logp) | ((uintptr_t)b.root_arrive)) & 15) == 0) {
        const f32x4 *u4 = reinterpret_cast<const f32x4 *>(g.uni_logp);
        const f32x4 *a4 = reinterpret_cast<const f32x4 *>(b.root_arrive);
        f32x4 *r4 = reinterpret_cast<f32x4 *>(row);
        const int n4 = V >> 2;
        for (int i = tid; i < n4; i += CB_THREADS) {
            f32x4 u = u4[i];
            const f32x4 a = a4[i];
            u.x = (Bd + u.x) + (a.x - phi); u.y = (Bd + u.y) + (a.y - phi);
            u.z = (Bd + u.z) + (a.z - phi); u.w = (Bd + u.w) + (a.w - phi);
            r4[i] = u;
        }
        for (int v = (n4 << 2) + tid; v < V; v += CB_THREADS) row[v] = (Bd + g.uni_logp[v]) + (b.root_arrive[v] - phi);
    } else {
        for (int v = tid; v < V; v += CB_THREADS) row[v] = (Bd + g.uni_logp[v]) + (b.root_arrive[v] - phi);
    }
    for (int k = d - 1; k >= 0; --k) {
        __syncthreads();                                   // the level below is in place: this one overwrites it
        const int c = s_c[k];
        const float Bk = s_B[k];
        int lo = g.child_off[c], hi = g.child_off[c + 1];
        if (lo < 0) lo = 0;
        if (hi > g.n_entries) hi = g.n_entries;
        for (int e = lo + tid; e < hi; e += CB_THREADS) {
            const int w = g.word[e];
            if (w >= 0 && w < V) row[w] = (Bk + g.logp[e]) + (b.root_arrive[w] - phi);
        }
    }
    if (sb == 0) return;                                   // uniform: the root has no entries
    __syncthreads();                                       // every n-gram level is in place
    int lo, hi;
    cb_range(b, sb, &lo, &hi);
    for (int e = lo + tid; e < hi; e += CB_THREADS) {      // words ascend strictly inside a node: one lane per word
        const int w = b.ext_word[e];
        if (w < 0 || w >= V) continue;
        float L = Bd + g.uni_logp[w];
        for (int k = 0; k < d; ++k) {                      // the longest context that holds w decides
            const int hit = ng_find(g, s_c[k], w);
            if (hit >= 0) {
                L = s_B[k] + g.logp[hit];
                break;
            }
        }
        row[w] = L + (b.ext_arrive[e] - phi);
    }
}

__global__ __launch_bounds__(CB_THREADS) void bias_walk_kernel(CBImage b, const long long *__restrict__ tokens,
                                                               long long ld, const int *__restrict__ n_tok, int Lmax,
                                                               int H, int *__restrict__ state, float *__restrict__ total,
                                                               float *__restrict__ residual) {
    const int h = blockIdx.x * CB_THREADS + threadIdx.x;
    if (h >= H) return;
    int n = n_tok[h];
    if (n < 0) n = 0;
    if (n > Lmax) n = Lmax;
    const long long *seq = tokens + (long long)h * ld;
    int s = 0;
    float tot = 0.0f;
    for (int i = 0; i < n; ++i) {
        float a;
        const int nxt = cb_goto(b, s, seq[i], &a);
        const float delta = a - b.phi[s];
        tot = tot + delta;
        s = nxt;
    }
    state[h] = s;
    total[h] = tot;
    residual[h] = b.phi[s];
}

static bool cb_image_ok(int V, int n_nodes, int n_entries, const float *phi, const float *root_arrive,
                        const int32_t *root_next, const int32_t *ext_off, const int32_t *ext_word,
                        const float *ext_arrive, const int32_t *ext_next) {
    if (V <= 0 || n_nodes < 1 || n_entries < 0) return false;
    if (!phi || !root_arrive || !root_next || !ext_off) return false;
    if (n_entries > 0 && (!ext_word || !ext_arrive || !ext_next)) return false;
    return true;
}

extern "C" int asrk_bias_step_f32(int V, int n_nodes, int n_entries, const float *phi, const float *root_arrive,
                                  const int32_t *root_next, const int32_t *ext_off, const int32_t *ext_word,
                                  const float *ext_arrive, const int32_t *ext_next, const int32_t *state_in,
                                  int n_state, const int64_t *token, const void *parent, int parent_is_i64,
                                  int32_t *state_out, float *out, int64_t row_stride, int R, void *stream) {
    if (!cb_image_ok(V, n_nodes, n_entries, phi, root_arrive, root_next, ext_off, ext_word, ext_arrive, ext_next))
        return ASRK_EINVAL;
    if (R < 0 || n_state < 0 || row_stride < V) return ASRK_EINVAL;
    if (R == 0) return ASRK_OK;
    if (!token || !state_out || !out || (const void *)state_out == (const void *)state_in) return ASRK_EINVAL;
    if (state_in && n_state == 0) return ASRK_EINVAL;
    CBImage b{V, n_nodes, n_entries, phi, root_arrive, root_next, ext_off, ext_word, ext_arrive, ext_next};
    hipStream_t s = (hipStream_t)stream;
    const long long *tok = reinterpret_cast<const long long *>(token);
    if (parent && parent_is_i64)
        hipLaunchKernelGGL(bias_step_kernel<long long>, dim3(R), dim3(CB_THREADS), 0, s, b, state_in, n_state, tok,
                           reinterpret_cast<const long long *>(parent), state_out, out, (long long)row_stride);
    else
        hipLaunchKernelGGL(bias_step_kernel<int>, dim3(R), dim3(CB_THREADS), 0, s, b, state_in, n_state, tok,
                           reinterpret_cast<const int *>(parent), state_out, out, (long long)row_stride);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}

extern "C" int asrk_ngram_bias_step_f32(int order, int V, int n_nodes, int n_entries, const float *uni_logp,
                                        const int32_t *uni_next, const float *bo, const int32_t *fail,
                                        const int32_t *child_off, const int32_t *word, const float *logp,
                                        const int32_t *next, int b_nodes, int b_entries, const float *phi,
                                        const float *root_arrive, const int32_t *root_next, const int32_t *ext_off,
                                        const int32_t *ext_word, const float *ext_arrive, const int32_t *ext_next,
                                        const int32_t *state_in, int n_state, const int64_t *token, const void *parent,
                                        int parent_is_i64, int32_t *state_out, float *out, int64_t row_stride, int R,
                                        void *stream) {
    if (order < 1 || order > NG_MAX_ORDER || V <= 0 || n_nodes < 1 || n_entries < 0 || R < 0 || n_state < 0)
        return ASRK_EINVAL;
    if (!uni_logp || !uni_next || !bo || !fail || !child_off) return ASRK_EINVAL;
    if (n_entries > 0 && (!word || !logp || !next)) return ASRK_EINVAL;
    if (!cb_image_ok(V, b_nodes, b_entries, phi, root_arrive, root_next, ext_off, ext_word, ext_arrive, ext_next))
        return ASRK_EINVAL;
    if (row_stride < V) return ASRK_EINVAL;
    if (R == 0) return ASRK_OK;
    if (!token || !state_out || !out || (const void *)state_out == (const void *)state_in) return ASRK_EINVAL;
    if (state_in && n_state == 0) return ASRK_EINVAL;
    NGImage g{order, V, n_nodes, n_entries, uni_logp, uni_next, bo, fail, child_off, word, logp, next};
    CBImage b{V, b_nodes, b_entries, phi, root_arrive, root_next, ext_off, ext_word, ext_arrive, ext_next};
    hipStream_t s = (hipStream_t)stream;
    const long long *tok = reinterpret_cast<const long long *>(token);
    if (parent && parent_is_i64)
        hipLaunchKernelGGL(ngram_bias_step_kernel<long long>, dim3(R), dim3(CB_THREADS), 0, s, g, b, state_in, n_state,
                           tok, reinterpret_cast<const long long *>(parent), state_out, out, (long long)row_stride);
    else
        hipLaunchKernelGGL(ngram_bias_step_kernel<int>, dim3(R), dim3(CB_THREADS), 0, s, g, b, state_in, n_state, tok,
                           reinterpret_cast<const int *>(parent), state_out, out, (long long)row_stride);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}

extern "C" int asrk_bias_walk(int V, int n_nodes, int n_entries, const float *phi, const float *root_arrive,
                              const int32_t *root_next, const int32_t *ext_off, const int32_t *ext_word,
                              const float *ext_arrive, const int32_t *ext_next, const int64_t *tokens,
                              int64_t token_stride, const int32_t *n_tok, int L, int H, int32_t *state, float *total,
                              float *residual, void *stream) {
    if (!cb_image_ok(V, n_nodes, n_entries, phi, root_arrive, root_next, ext_off, ext_word, ext_arrive, ext_next))
        return ASRK_EINVAL;
    if (H < 0 || L < 0 || token_stride < L) return ASRK_EINVAL;
    if (H == 0) return ASRK_OK;
    if (!n_tok || !state || !total || !residual || (L > 0 && !tokens)) return ASRK_EINVAL;
    CBImage b{V, n_nodes, n_entries, phi, root_arrive, root_next, ext_off, ext_word, ext_arrive, ext_next};
    hipLaunchKernelGGL(bias_walk_kernel, dim3((H + CB_THREADS - 1) / CB_THREADS), dim3(CB_THREADS), 0,
                       (hipStream_t)stream, b, reinterpret_cast<const long long *>(tokens), (long long)token_stride,
                       n_tok, L, H, state, total, residual);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}
