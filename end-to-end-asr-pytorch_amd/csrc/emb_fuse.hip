// Word-embedding plug-in kernels (reference: src/plugin.py EmbeddingRegularizer): the fused decoder / embedding
// distribution (forward + backward), the cosine embedding loss with the target row gathered in the kernel, the NLL
// loss over log-probabilities and the row L2 normalisation.  All f32, labels int64.
//
// Every reduction here has a fixed order (wave shuffle tree, then the four waves of a workgroup in LDS, then one
// workgroup over the per-row / per-chunk partials): no float atomics, so results are bit-reproducible.
#include "common.h"

namespace {

inline bool al16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// sum / max over the 256 threads of a workgroup; every thread gets the result.  `red` holds 4 floats; the leading
// barrier makes back-to-back calls on the same buffer safe.
__device__ __forceinline__ float block_sum(float v, float *red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
__device__ __forceinline__ float block_max(float v, float *red) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// element v of a parameter vector of length 1 or V
__device__ __forceinline__ float par_at(const float *p, int len, int v) { return len == 1 ? p[0] : p[v]; }
__device__ __forceinline__ float mix_of(float lam, int is_logit) { return is_logit ? sigmoidf_acc(lam) : lam; }
// log(f + eps) for a probability f.  Near f = 1 (a confident row; every row of a one-word vocabulary) f + eps rounds
// back to f in float32 and the logarithm's relative accuracy goes with it: f - 1 is exact there, log1p keeps it.
__device__ __forceinline__ float log_prob(float f, float eps) {
    return f > 0.5f ? log1pf((f - 1.f) + eps) : logf(f + eps);
}

// ------------------------------------------------------------------------------------------------ fused distribution
// one workgroup of 256 threads per row.  The row is read three times (maxima, sums, output); a [V] f32 row is at most
// 64 KB at the shipped vocabulary, so the second and third reads come from the L2.  VEC: 16-byte accesses, legal only
// when V % 4 == 0, ld % 4 == 0 and every base pointer is 16-byte aligned (checked by the launcher); else scalar.
template <bool VEC>
__global__ __launch_bounds__(256) void fuse_fwd_kernel(const float *__restrict__ d, int ld,
                                                       const float *__restrict__ e,
                                                       const float *__restrict__ temp, int temp_len,
                                                       const float *__restrict__ lam, int lam_len, int lam_is_logit,
                                                       float eps, int V, float *__restrict__ y,
                                                       float *__restrict__ stats) {
    __shared__ float red[4];
    const int row = blockIdx.x;
    const int tid = threadIdx.x;
    const float *dr = d + (size_t)row * ld;
    const float *er = e + (size_t)row * V;
    float *yr = y + (size_t)row * V;
    const int nv = VEC ? (V >> 2) : 0;

    float md = -INFINITY, ma = -INFINITY;
    if (VEC) {
        for (int i = tid; i < nv; i += 256) {
            const f32x4 dv = reinterpret_cast<const f32x4 *>(dr)[i];
            const f32x4 ev = reinterpret_cast<const f32x4 *>(er)[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                md = fmaxf(md, dv[j]);
                ma = fmaxf(ma, fmaxf(par_at(temp, temp_len, 4 * i + j), 0.f) * ev[j]);
            }
        }
    } else {
        for (int i = tid; i < V; i += 256) {
            md = fmaxf(md, dr[i]);
            ma = fmaxf(ma, fmaxf(par_at(temp, temp_len, i), 0.f) * er[i]);
        }
    }
    md = block_max(md, red);
    ma = block_max(ma, red);

    float sd = 0.f, sa = 0.f;
    if (VEC) {
        for (int i = tid; i < nv; i += 256) {
            const f32x4 dv = reinterpret_cast<const f32x4 *>(dr)[i];
            const f32x4 ev = reinterpret_cast<const f32x4 *>(er)[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                sd += expf(dv[j] - md);
                sa += expf(fmaxf(par_at(temp, temp_len, 4 * i + j), 0.f) * ev[j] - ma);
            }
        }
    } else {
        for (int i = tid; i < V; i += 256) {
            sd += expf(dr[i] - md);
            sa += expf(fmaxf(par_at(temp, temp_len, i), 0.f) * er[i] - ma);
        }
    }
    sd = block_sum(sd, red);
    sa = block_sum(sa, red);
    if (tid == 0) {
        stats[(size_t)row * 4 + 0] = md;
        stats[(size_t)row * 4 + 1] = sd;
        stats[(size_t)row * 4 + 2] = ma;
        stats[(size_t)row * 4 + 3] = sa;
    }
    const float rd = 1.f / sd, ra = 1.f / sa;
    const float s1 = lam_len == 1 ? mix_of(lam[0], lam_is_logit) : 0.f;
    if (VEC) {
        for (int i = tid; i < nv; i += 256) {
            const f32x4 dv = reinterpret_cast<const f32x4 *>(dr)[i];
            const f32x4 ev = reinterpret_cast<const f32x4 *>(er)[i];
            f32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int v = 4 * i + j;
                const float pd = expf(dv[j] - md) * rd;
                const float pe = expf(fmaxf(par_at(temp, temp_len, v), 0.f) * ev[j] - ma) * ra;
                const float s = lam_len == 1 ? s1 : mix_of(lam[v], lam_is_logit);
                o[j] = log_prob((1.f - s) * pd + s * pe, eps);
            }
            reinterpret_cast<f32x4 *>(yr)[i] = o;
        }
    } else {
        for (int i = tid; i < V; i += 256) {
            const float pd = expf(dr[i] - md) * rd;
            const float pe = expf(fmaxf(par_at(temp, temp_len, i), 0.f) * er[i] - ma) * ra;
            const float s = lam_len == 1 ? s1 : mix_of(lam[i], lam_is_logit);
            yr[i] = log_prob((1.f - s) * pd + s * pe, eps);
        }
    }
}

// everything the backward needs of element v of a row, recomputed from the saved row statistics
struct FuseElem {
    float pd, pe, s, df, tpos;
};
__device__ __forceinline__ FuseElem fuse_elem(float dv, float ev, float gv, float tv, float sv, float md, float rd,
                                              float ma, float ra, float eps) {
    FuseElem r;
    r.tpos = fmaxf(tv, 0.f);
    r.pd = expf(dv - md) * rd;
    r.pe = expf(r.tpos * ev - ma) * ra;
    r.s = sv;
    r.df = gv / ((1.f - sv) * r.pd + sv * r.pe + eps);
    return r;
}

// backward, one workgroup per row: pass 1 forms the two softmax dot products, pass 2 writes d_dec / d_emb and, for a
// SCALAR temp / lam parameter, this row's contribution (row_par[row*2 + {0,1}]).  dots[row*2 + {0,1}] are kept for the
// column pass of per-vocabulary parameters.
template <bool VEC>
__global__ __launch_bounds__(256) void fuse_bwd_kernel(const float *__restrict__ g, const float *__restrict__ d, int ld,
                                                       const float *__restrict__ e,
                                                       const float *__restrict__ temp, int temp_len,
                                                       const float *__restrict__ lam, int lam_len, int lam_is_logit,
                                                       float eps, const float *__restrict__ stats, int V,
                                                       float *__restrict__ dd, float *__restrict__ de,
                                                       float *__restrict__ dots, float *__restrict__ row_par) {
    __shared__ float red[4];
    const int row = blockIdx.x;
    const int tid = threadIdx.x;
    const float *gr = g + (size_t)row * V;
    const float *dr = d + (size_t)row * ld;
    const float *er = e + (size_t)row * V;
    float *ddr = dd + (size_t)row * V;
    float *der = de + (size_t)row * V;
    const float md = stats[(size_t)row * 4 + 0], rd = 1.f / stats[(size_t)row * 4 + 1];
    const float ma = stats[(size_t)row * 4 + 2], ra = 1.f / stats[(size_t)row * 4 + 3];
    const float s1 = lam_len == 1 ? mix_of(lam[0], lam_is_logit) : 0.f;
    const int nv = VEC ? (V >> 2) : 0;

    float ad = 0.f, ae = 0.f;
    if (VEC) {
        for (int i = tid; i < nv; i += 256) {
            const f32x4 gv = reinterpret_cast<const f32x4 *>(gr)[i];
            const f32x4 dv = reinterpret_cast<const f32x4 *>(dr)[i];
            const f32x4 ev = reinterpret_cast<const f32x4 *>(er)[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int v = 4 * i + j;
                const float sv = lam_len == 1 ? s1 : mix_of(lam[v], lam_is_logit);
                const FuseElem q = fuse_elem(dv[j], ev[j], gv[j], par_at(temp, temp_len, v), sv, md, rd, ma, ra, eps);
                ad += q.pd * ((1.f - q.s) * q.df);
                ae += q.pe * (q.s * q.df);
            }
        }
    } else {
        for (int i = tid; i < V; i += 256) {
            const float sv = lam_len == 1 ? s1 : mix_of(lam[i], lam_is_logit);
            const FuseElem q = fuse_elem(dr[i], er[i], gr[i], par_at(temp, temp_len, i), sv, md, rd, ma, ra, eps);
            ad += q.pd * ((1.f - q.s) * q.df);
            ae += q.pe * (q.s * q.df);
        }
    }
    ad = block_sum(ad, red);
    ae = block_sum(ae, red);
    if (tid == 0) {
        dots[(size_t)row * 2 + 0] = ad;
        dots[(size_t)row * 2 + 1] = ae;
    }

    float pt = 0.f, pl = 0.f;
    if (VEC) {
        for (int i = tid; i < nv; i += 256) {
            const f32x4 gv = reinterpret_cast<const f32x4 *>(gr)[i];
            const f32x4 dv = reinterpret_cast<const f32x4 *>(dr)[i];
            const f32x4 ev = reinterpret_cast<const f32x4 *>(er)[i];
            f32x4 od, oe;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int v = 4 * i + j;
                const float tv = par_at(temp, temp_len, v);
                const float sv = lam_len == 1 ? s1 : mix_of(lam[v], lam_is_logit);
                const FuseElem q = fuse_elem(dv[j], ev[j], gv[j], tv, sv, md, rd, ma, ra, eps);
                const float da = q.pe * (q.s * q.df - ae);
                od[j] = q.pd * ((1.f - q.s) * q.df - ad);
                oe[j] = q.tpos * da;
                pt += tv > 0.f ? ev[j] * da : 0.f;
                pl += (q.pe - q.pd) * q.df * (lam_is_logit ? q.s * (1.f - q.s) : 1.f);
            }
            reinterpret_cast<f32x4 *>(ddr)[i] = od;
            reinterpret_cast<f32x4 *>(der)[i] = oe;
        }
    } else {
        for (int i = tid; i < V; i += 256) {
            const float tv = par_at(temp, temp_len, i);
            const float sv = lam_len == 1 ? s1 : mix_of(lam[i], lam_is_logit);
            const FuseElem q = fuse_elem(dr[i], er[i], gr[i], tv, sv, md, rd, ma, ra, eps);
            const float da = q.pe * (q.s * q.df - ae);
            ddr[i] = q.pd * ((1.f - q.s) * q.df - ad);
            der[i] = q.tpos * da;
            pt += tv > 0.f ? er[i] * da : 0.f;
            pl += (q.pe - q.pd) * q.df * (lam_is_logit ? q.s * (1.f - q.s) : 1.f);
        }
    }
    if (row_par) {      // wave-uniform: a kernel argument
        pt = block_sum(pt, red);
        pl = block_sum(pl, red);
        if (tid == 0) {
            row_par[(size_t)row * 2 + 0] = pt;
            row_par[(size_t)row * 2 + 1] = pl;
        }
    }
}

// scalar parameter gradients: one workgroup adds the per-row contributions in a fixed order
__global__ __launch_bounds__(256) void fuse_scalar_sum_kernel(const float *__restrict__ row_par, int N,
                                                              float *__restrict__ dtemp, float *__restrict__ dlam) {
    __shared__ float red[4];
    float a = 0.f, b = 0.f;
    for (int r = threadIdx.x; r < N; r += 256) {
        a += row_par[(size_t)r * 2 + 0];
        b += row_par[(size_t)r * 2 + 1];
    }
    a = block_sum(a, red);
    b = block_sum(b, red);
    if (threadIdx.x == 0) {
        if (dtemp) dtemp[0] = a;
        if (dlam) dlam[0] = b;
    }
}

// per-vocabulary parameter gradients, first pass: thread = one column, workgroup (x, c) = columns [256x, 256x + 256) of
// the rows [c * rpc, (c + 1) * rpc); part_t / part_l [chunks, V] (either may be null)
__global__ __launch_bounds__(256) void fuse_col_kernel(const float *__restrict__ g, const float *__restrict__ d, int ld,
                                                       const float *__restrict__ e,
                                                       const float *__restrict__ temp, int temp_len,
                                                       const float *__restrict__ lam, int lam_len, int lam_is_logit,
                                                       float eps, const float *__restrict__ stats,
                                                       const float *__restrict__ dots, int N, int V, int rpc,
                                                       float *__restrict__ part_t, float *__restrict__ part_l) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const int r0 = blockIdx.y * rpc;
    const int r1 = min(N, r0 + rpc);
    const float tv = par_at(temp, temp_len, v);
    const float sv = mix_of(par_at(lam, lam_len, v), lam_is_logit);
    const float ls = lam_is_logit ? sv * (1.f - sv) : 1.f;
    float pt = 0.f, pl = 0.f;
    for (int r = r0; r < r1; ++r) {
        const float md = stats[(size_t)r * 4 + 0], rd = 1.f / stats[(size_t)r * 4 + 1];
        const float ma = stats[(size_t)r * 4 + 2], ra = 1.f / stats[(size_t)r * 4 + 3];
        const float ev = e[(size_t)r * V + v];
        const FuseElem q = fuse_elem(d[(size_t)r * ld + v], ev, g[(size_t)r * V + v], tv, sv, md, rd, ma, ra, eps);
        const float da = q.pe * (q.s * q.df - dots[(size_t)r * 2 + 1]);
        pt += tv > 0.f ? ev * da : 0.f;
        pl += (q.pe - q.pd) * q.df * ls;
    }
    if (part_t) part_t[(size_t)blockIdx.y * V + v] = pt;
    if (part_l) part_l[(size_t)blockIdx.y * V + v] = pl;
}

// second pass: out[v] = sum over chunks, in chunk order
__global__ __launch_bounds__(256) void fuse_col_sum_kernel(const float *__restrict__ part, int chunks, int V,
                                                           float *__restrict__ out) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    float a = 0.f;
    for (int c = 0; c < chunks; ++c) a += part[(size_t)c * V + v];
    out[v] = a;
}

// ------------------------------------------------------------------------------------------------ cosine embedding loss
// one wave per row, 4 rows per workgroup.  y = table[label] is read in place.  A label outside [0, rows of the table)
// is treated like the pad label: the row contributes nothing and gets a zero gradient.
// The row arithmetic is float64: the gradient y |x|^2 - (x.y) x cancels as x turns parallel to y - the state the
// regulariser trains towards - and in float32 the difference is rounding noise well before that (at E = 1 always).
// The rows are [N,E] with E a few hundred, so the wider arithmetic costs nothing next to the [N,V] kernels.
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__global__ __launch_bounds__(256) void cos_fwd_kernel(const float *__restrict__ x, const float *__restrict__ table,
                                                      int64_t table_rows, const int64_t *__restrict__ label, int N,
                                                      int E, float *__restrict__ row_loss) {
    const int row = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= N) return;
    const int64_t t = label[row];
    if (t <= 0 || t >= table_rows) {
        if (lane == 0) row_loss[row] = 0.f;
        return;
    }
    const float *xr = x + (size_t)row * E;
    const float *yr = table + (size_t)t * E;
    double xy = 0., xx = 0., yy = 0.;
    for (int i = lane; i < E; i += 64) {
        const double a = xr[i], b = yr[i];
        xy += a * b;
        xx += a * a;
        yy += b * b;
    }
    xy = wave_sum_f64(xy);
    xx = wave_sum_f64(xx);
    yy = wave_sum_f64(yy);
    if (lane == 0) row_loss[row] = (float)(1. - xy / sqrt((xx + 1e-12) * (yy + 1e-12)));
}

// loss = mean_b( sum_t row_loss[b,t] / #{t: label[b,t] != 0} ): thread b adds its utterances' rows in order, then a
// fixed tree over the workgroup.  count[b] is kept for the backward.  An utterance without a label gives 0/0 = NaN.
__global__ __launch_bounds__(256) void cos_reduce_kernel(const float *__restrict__ row_loss,
                                                         const int64_t *__restrict__ label, int B, int L,
                                                         float *__restrict__ count, float *__restrict__ loss) {
    __shared__ float red[4];
    float acc = 0.f;
    for (int b = threadIdx.x; b < B; b += 256) {
        float s = 0.f, c = 0.f;
        for (int t = 0; t < L; ++t) {
            s += row_loss[(size_t)b * L + t];
            c += label[(size_t)b * L + t] != 0 ? 1.f : 0.f;
        }
        count[b] = c;
        acc += s / c;
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) loss[0] = acc / (float)B;
}

__global__ __launch_bounds__(256) void cos_bwd_kernel(const float *__restrict__ x, const float *__restrict__ table,
                                                      int64_t table_rows, const int64_t *__restrict__ label, int N,
                                                      int L, int E, float inv_b, const float *__restrict__ count,
                                                      const float *__restrict__ gout, float *__restrict__ dx,
                                                      float *__restrict__ dy) {
    const int row = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= N) return;
    const int64_t t = label[row];
    float *dxr = dx + (size_t)row * E;
    float *dyr = dy ? dy + (size_t)row * E : nullptr;
    if (t <= 0 || t >= table_rows) {
        for (int i = lane; i < E; i += 64) {
            dxr[i] = 0.f;
            if (dyr) dyr[i] = 0.f;
        }
        return;
    }
    const float *xr = x + (size_t)row * E;
    const float *yr = table + (size_t)t * E;
    double xy = 0., xx = 0., yy = 0.;
    for (int i = lane; i < E; i += 64) {
        const double a = xr[i], b = yr[i];
        xy += a * b;
        xx += a * a;
        yy += b * b;
    }
    xy = wave_sum_f64(xy);
    xx = wave_sum_f64(xx) + 1e-12;
    yy = wave_sum_f64(yy) + 1e-12;
    const double den = sqrt(xx * yy);
    // d(1 - cos)/dx = -(y |x|^2 - (x.y) x) / (den |x|^2), likewise for y
    const double gl = (double)(gout[0] * inv_b / count[row / L]);
    const double kx = -gl / (den * xx), ky = -gl / (den * yy);
    for (int i = lane; i < E; i += 64) {
        const double a = xr[i], b = yr[i];
        dxr[i] = (float)(kx * (b * xx - xy * a));
        if (dyr) dyr[i] = (float)(ky * (a * yy - xy * b));
    }
}

// Gradient of a trainable table from the gathered rows' gradients dy [N,E]: dtable[v] = sum of dy[n] over the rows with
// label[n] == v, added in row order - no atomics, so repeated labels give the same bits every run.  One wave per row n;
// the wave of the FIRST row that carries a label owns that label's table row (a wave that finds its label earlier in
// the list leaves) and adds the later occurrences as it meets them.  Labels are scanned 64 at a time (one per lane, a
// ballot marks the matches); N is B*L, a few thousand, so the N^2/64 label reads are nothing next to one [N,V] pass.
// dtable is zeroed by the launcher; rows no label names, and the pad row 0, stay zero.
__global__ __launch_bounds__(256) void cos_table_grad_kernel(const float *__restrict__ dy,
                                                             const int64_t *__restrict__ label, int N, int E,
                                                             int64_t table_rows, float *__restrict__ dtable) {
    const int row = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= N) return;
    const int64_t t = label[row];
    if (t <= 0 || t >= table_rows) return;
    for (int base = 0; base < row; base += 64) {          // an earlier occurrence owns the label
        const int n = base + lane;
        if (__ballot(n < row && label[n] == t) != 0ull) return;
    }
    float *out = dtable + (size_t)t * E;
    for (int c0 = 0; c0 < E; c0 += 64) {
        const int c = c0 + lane;
        float acc = c < E ? dy[(size_t)row * E + c] : 0.f;
        for (int base = row + 1; base < N; base += 64) {
            const int n = base + lane;
            unsigned long long m = __ballot(n < N && label[n] == t);
            while (m) {                                    // wave-uniform: matches in ascending row order
                const int k = __builtin_ctzll(m);
                m &= m - 1;
                if (c < E) acc += dy[(size_t)(base + k) * E + c];
            }
        }
        if (c < E) out[c] = acc;
    }
}

// ------------------------------------------------------------------------------------------------ NLL over log-probs
// sums[0] = sum over counted rows of -logp[r, t_r], sums[1] = their number; one workgroup, fixed order
__global__ __launch_bounds__(256) void nll_fwd_kernel(const float *__restrict__ logp, int rows, int V, int ld,
                                                      const int64_t *__restrict__ tgt, int ignore_index,
                                                      float *__restrict__ sums) {
    __shared__ float red[4];
    float a = 0.f, c = 0.f;
    for (int r = threadIdx.x; r < rows; r += 256) {
        const int64_t t = tgt[r];
        if (t != ignore_index && t >= 0 && t < V) {
            a -= logp[(size_t)r * ld + t];
            c += 1.f;
        }
    }
    a = block_sum(a, red);
    c = block_sum(c, red);
    if (threadIdx.x == 0) {
        sums[0] = a;
        sums[1] = c;
    }
}

// dlogp[r, :] = 0 except dlogp[r, t_r] = -gscale for counted rows; one workgroup per row
__global__ __launch_bounds__(256) void nll_bwd_kernel(int V, int ld, const int64_t *__restrict__ tgt, int ignore_index,
                                                      const float *__restrict__ gscale, float *__restrict__ dlogp) {
    const int row = blockIdx.x;
    const int64_t t = tgt[row];
    const bool live = t != ignore_index && t >= 0 && t < V;
    const float gneg = live ? -gscale[0] : 0.f;
    float *dr = dlogp + (size_t)row * ld;
    for (int i = threadIdx.x; i < V; i += 256) dr[i] = (live && i == (int)t) ? gneg : 0.f;
}

// ------------------------------------------------------------------------------------------------ row L2 normalisation
// y = x / max(|x|, eps) (torch.nn.functional.normalize); one wave per row
__global__ __launch_bounds__(256) void l2norm_fwd_kernel(const float *__restrict__ x, float *__restrict__ y,
                                                         float *__restrict__ norm, int rows, int D, float eps) {
    const int row = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float *xr = x + (size_t)row * D;
    float *yr = y + (size_t)row * D;
    float ss = 0.f;
    for (int i = lane; i < D; i += 64) ss += xr[i] * xr[i];
    const float nrm = sqrtf(wave_sum(ss));
    if (lane == 0) norm[row] = nrm;
    const float den = fmaxf(nrm, eps);
    for (int i = lane; i < D; i += 64) yr[i] = xr[i] / den;
}

// dx = (dy - y * (y . dy)) / |x| where |x| > eps; below the clamp the divisor is the constant eps: dx = dy / eps
__global__ __launch_bounds__(256) void l2norm_bwd_kernel(const float *__restrict__ y, const float *__restrict__ dy,
                                                         const float *__restrict__ norm, float *__restrict__ dx,
                                                         int rows, int D, float eps) {
    const int row = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float *yr = y + (size_t)row * D;
    const float *gr = dy + (size_t)row * D;
    float *dr = dx + (size_t)row * D;
    const float nrm = norm[row];
    if (!(nrm >= eps)) {
        for (int i = lane; i < D; i += 64) dr[i] = gr[i] / eps;
        return;
    }
    float dot = 0.f;
    for (int i = lane; i < D; i += 64) dot += yr[i] * gr[i];
    dot = wave_sum(dot);
    for (int i = lane; i < D; i += 64) dr[i] = (gr[i] - yr[i] * dot) / nrm;
}

// workspace layout of the fused backward, in floats: dots [2N], row_par [2N], part_t [chunks * V], part_l [chunks * V]
struct FuseWs {
    int chunks, rpc;
    size_t dots, row_par, part_t, part_l, total;
};
FuseWs fuse_ws(int N, int V, int temp_len, int lam_len, int want_dtemp, int want_dlam) {
    FuseWs w{};
    const bool col_t = want_dtemp && temp_len != 1, col_l = want_dlam && lam_len != 1;
    const int gx = asrk_div_up(V, 256);
    int chunks = asrk_div_up(1024, gx);
    if (chunks > asrk_div_up(N, 16)) chunks = asrk_div_up(N, 16);
    if (chunks < 1) chunks = 1;
    w.rpc = asrk_div_up(N, chunks);
    if (w.rpc < 1) w.rpc = 1;
    w.chunks = asrk_div_up(N, w.rpc);
    if (w.chunks < 1) w.chunks = 1;
    w.dots = 0;
    w.row_par = w.dots + (size_t)2 * N;
    w.part_t = w.row_par + (size_t)2 * N;
    w.part_l = w.part_t + (col_t ? (size_t)w.chunks * V : 0);
    w.total = w.part_l + (col_l ? (size_t)w.chunks * V : 0);
    return w;
}

bool fuse_args_ok(int N, int V, int ld, int temp_len, int lam_len) {
    return N >= 0 && V > 0 && ld >= V && (temp_len == 1 || temp_len == V) && (lam_len == 1 || lam_len == V);
}

}  // namespace

extern "C" size_t asrk_emb_fuse_bwd_ws_bytes(int N, int V, int temp_len, int lam_len, int want_dtemp, int want_dlam) {
    if (!fuse_args_ok(N, V, V, temp_len, lam_len)) return 0;
    return fuse_ws(N, V, temp_len, lam_len, want_dtemp, want_dlam).total * sizeof(float);
}

extern "C" int asrk_emb_fuse_fwd_f32(const float *dec_logit, int ld, const float *emb_logit, const float *temp,
                                     int temp_len, const float *lam, int lam_len, int lam_is_logit, float eps, int N,
                                     int V, float *y, float *stats, void *stream) {
    if (!fuse_args_ok(N, V, ld, temp_len, lam_len) || !(eps >= 0.f)) return ASRK_EINVAL;
    if (!dec_logit || !emb_logit || !temp || !lam || !y || !stats) return ASRK_EINVAL;
    if (N == 0) return ASRK_OK;
    hipStream_t s = (hipStream_t)stream;
    const bool vec = V % 4 == 0 && ld % 4 == 0 && al16(dec_logit) && al16(emb_logit) && al16(y);
    asrk_prof_begin_(PROF_ROWOPS, s);
    if (vec)
        hipLaunchKernelGGL((fuse_fwd_kernel<true>), dim3((unsigned)N), dim3(256), 0, s, dec_logit, ld, emb_logit, temp,
                           temp_len, lam, lam_len, lam_is_logit ? 1 : 0, eps, V, y, stats);
    else
        hipLaunchKernelGGL((fuse_fwd_kernel<false>), dim3((unsigned)N), dim3(256), 0, s, dec_logit, ld, emb_logit, temp,
                           temp_len, lam, lam_len, lam_is_logit ? 1 : 0, eps, V, y, stats);
    asrk_prof_end_(PROF_ROWOPS, s);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}

extern "C" int asrk_emb_fuse_bwd_f32(const float *g, const float *dec_logit, int ld, const float *emb_logit,
                                     const float *temp, int temp_len, const float *lam, int lam_len, int lam_is_logit,
                                     float eps, const float *stats, int N, int V, float *d_dec, float *d_emb,
                                     float *dtemp, float *dlam, void *ws, size_t ws_bytes, void *stream) {
    if (!fuse_args_ok(N, V, ld, temp_len, lam_len) || !(eps >= 0.f)) return ASRK_EINVAL;
    if (!g || !dec_logit || !emb_logit || !temp || !lam || !stats || !d_dec || !d_emb) return ASRK_EINVAL;
    const FuseWs w = fuse_ws(N, V, temp_len, lam_len, dtemp != nullptr, dlam != nullptr);
    if (!ws || ws_bytes < w.total * sizeof(float)) return ASRK_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    if (N == 0) {       // no rows: the parameter gradients are sums over nothing
        if (dtemp) ASRK_HIP(hipMemsetAsync(dtemp, 0, (size_t)temp_len * 4, s));
        if (dlam) ASRK_HIP(hipMemsetAsync(dlam, 0, (size_t)lam_len * 4, s));
        return ASRK_OK;
    }
    float *wf = (float *)ws;
    const bool sc_t = dtemp && temp_len == 1, sc_l = dlam && lam_len == 1;
    const bool col_t = dtemp && temp_len != 1, col_l = dlam && lam_len != 1;
    float *row_par = (sc_t || sc_l) ? wf + w.row_par : nullptr;
    const bool vec = V % 4 == 0 && ld % 4 == 0 && al16(g) && al16(dec_logit) && al16(emb_logit) && al16(d_dec) &&
                     al16(d_emb);
    const int il = lam_is_logit ? 1 : 0;
    asrk_prof_begin_(PROF_ROWOPS, s);
    if (vec)
        hipLaunchKernelGGL((fuse_bwd_kernel<true>), dim3((unsigned)N), dim3(256), 0, s, g, dec_logit, ld, emb_logit, temp,
                           temp_len, lam, lam_len, il, eps, stats, V, d_dec, d_emb, wf + w.dots, row_par);
    else
        hipLaunchKernelGGL((fuse_bwd_kernel<false>), dim3((unsigned)N), dim3(256), 0, s, g, dec_logit, ld, emb_logit, temp,
                           temp_len, lam, lam_len, il, eps, stats, V, d_dec, d_emb, wf + w.dots, row_par);
    if (row_par)
        hipLaunchKernelGGL(fuse_scalar_sum_kernel, dim3(1), dim3(256), 0, s, row_par, N, sc_t ? dtemp : nullptr,
                           sc_l ? dlam : nullptr);
    if (col_t || col_l) {
        const unsigned gx = (unsigned)asrk_div_up(V, 256);
        float *pt = col_t ? wf + w.part_t : nullptr, *pl = col_l ? wf + w.part_l : nullptr;
        hipLaunchKernelGGL(fuse_col_kernel, dim3(gx, (unsigned)w.chunks), dim3(256), 0, s, g, dec_logit, ld, emb_logit,
                           temp, temp_len, lam, lam_len, il, eps, stats, wf + w.dots, N, V, w.rpc, pt, pl);
        if (col_t) hipLaunchKernelGGL(fuse_col_sum_kernel, dim3(gx), dim3(256), 0, s, pt, w.chunks, V, dtemp);
        if (col_l) hipLaunchKernelGGL(fuse_col_sum_kernel, dim3(gx), dim3(256), 0, s, pl, w.chunks, V, dlam);
    }
    asrk_prof_end_(PROF_ROWOPS, s);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}

extern "C" int asrk_cos_emb_loss_fwd_f32(const float *x, const float *table, int64_t table_rows, const int64_t *label,
                                         int B, int L, int E, float *row_loss, float *count, float *loss,
                                         void *stream) {
    if (B <= 0 || L <= 0 || E <= 0 || table_rows <= 0 || (int64_t)B * L > INT32_MAX) return ASRK_EINVAL;
    if (!x || !table || !label || !row_loss || !count || !loss) return ASRK_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int N = B * L;
    asrk_prof_begin_(PROF_ROWOPS, s);
    hipLaunchKernelGGL(cos_fwd_kernel, dim3((unsigned)asrk_div_up(N, 4)), dim3(256), 0, s, x, table, table_rows, label,
                       N, E, row_loss);
    hipLaunchKernelGGL(cos_reduce_kernel, dim3(1), dim3(256), 0, s, row_loss, label, B, L, count, loss);
    asrk_prof_end_(PROF_ROWOPS, s);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}

extern "C" int asrk_cos_emb_loss_bwd_f32(const float *x, const float *table, int64_t table_rows, const int64_t *label,
                                         int B, int L, int E, const float *count, const float *gout, float *dx,
                                         float *dy, void *stream) {
    if (B <= 0 || L <= 0 || E <= 0 || table_rows <= 0 || (int64_t)B * L > INT32_MAX) return ASRK_EINVAL;
    if (!x || !table || !label || !count || !gout || !dx) return ASRK_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int N = B * L;
    asrk_prof_begin_(PROF_ROWOPS, s);
    hipLaunchKernelGGL(cos_bwd_kernel, dim3((unsigned)asrk_div_up(N, 4)), dim3(256), 0, s, x, table, table_rows, label,
                       N, L, E, 1.f / (float)B, count, gout, dx, dy);
    asrk_prof_end_(PROF_ROWOPS, s);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}

extern "C" int asrk_cos_emb_table_grad_f32(const float *dy, const int64_t *label, int N, int E, int64_t table_rows,
                                           float *dtable, void *stream) {
    if (N < 0 || E <= 0 || table_rows <= 0) return ASRK_EINVAL;
    if (!dtable || (N > 0 && (!dy || !label))) return ASRK_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    ASRK_HIP(hipMemsetAsync(dtable, 0, (size_t)table_rows * E * sizeof(float), s));
    if (N == 0) return ASRK_OK;
    asrk_prof_begin_(PROF_ROWOPS, s);
    hipLaunchKernelGGL(cos_table_grad_kernel, dim3((unsigned)asrk_div_up(N, 4)), dim3(256), 0, s, dy, label, N, E,
                       table_rows, dtable);
    asrk_prof_end_(PROF_ROWOPS, s);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}

extern "C" int asrk_nll_loss_fwd_f32(const float *logp, int rows, int V, int ld, const int64_t *targets,
                                     int ignore_index, float *sums, void *stream) {
    if (rows < 0 || V <= 0 || ld < V) return ASRK_EINVAL;
    if (!sums || (rows > 0 && (!logp || !targets))) return ASRK_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    asrk_prof_begin_(PROF_ROWOPS, s);
    hipLaunchKernelGGL(nll_fwd_kernel, dim3(1), dim3(256), 0, s, logp, rows, V, ld, targets, ignore_index, sums);
    asrk_prof_end_(PROF_ROWOPS, s);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}

extern "C" int asrk_nll_loss_bwd_f32(int rows, int V, int ld, const int64_t *targets, int ignore_index,
                                     const float *gscale, float *dlogp, void *stream) {
    if (rows < 0 || V <= 0 || ld < V) return ASRK_EINVAL;
    if (rows == 0) return ASRK_OK;
    if (!targets || !gscale || !dlogp) return ASRK_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    asrk_prof_begin_(PROF_ROWOPS, s);
    hipLaunchKernelGGL(nll_bwd_kernel, dim3((unsigned)rows), dim3(256), 0, s, V, ld, targets, ignore_index, gscale,
                       dlogp);
    asrk_prof_end_(PROF_ROWOPS, s);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}

extern "C" int asrk_l2norm_fwd_f32(const float *x, float *y, float *norm, int rows, int D, float eps, void *stream) {
    if (rows < 0 || D <= 0 || !(eps > 0.f)) return ASRK_EINVAL;
    if (rows == 0) return ASRK_OK;
    if (!x || !y || !norm) return ASRK_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    asrk_prof_begin_(PROF_ROWOPS, s);
    hipLaunchKernelGGL(l2norm_fwd_kernel, dim3((unsigned)asrk_div_up(rows, 4)), dim3(256), 0, s, x, y, norm, rows, D,
                       eps);
    asrk_prof_end_(PROF_ROWOPS, s);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}

extern "C" int asrk_l2norm_bwd_f32(const float *y, const float *dy, const float *norm, float *dx, int rows, int D,
                                   float eps, void *stream) {
    if (rows < 0 || D <= 0 || !(eps > 0.f)) return ASRK_EINVAL;
    if (rows == 0) return ASRK_OK;
    if (!y || !dy || !norm || !dx) return ASRK_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    asrk_prof_begin_(PROF_ROWOPS, s);
    hipLaunchKernelGGL(l2norm_bwd_kernel, dim3((unsigned)asrk_div_up(rows, 4)), dim3(256), 0, s, y, dy, norm, dx, rows,
                       D, eps);
    asrk_prof_end_(PROF_ROWOPS, s);
    ASRK_LAUNCH_CHECK();
    return ASRK_OK;
}
