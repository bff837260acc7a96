// Alignment-length-synchronous transducer beam search (Saon et al. 2020), one iteration of one utterance: the
// candidates of the [W, K+1] table, the merge of equal label sequences, the cut to W and the finished list, as
// data-parallel phases over flat arrays.  Shared by the gfx950 kernel (rnnt_beam.hip, one workgroup per utterance) and
// the host build of the tests (tests/native/rnnt_beam_host.cpp); the float64 reference of the tests
// (tests/rnnt_beam_reference.py) implements the same rules.  Plain C++: no HIP call, no atomics.
//
// Required before inclusion: RB_HD (function qualifier), RB_FOR(i, n) { ... } (the workgroup's strided loop; a plain
// loop on the host), RB_SYNC() (workgroup barrier; nothing on the host).  Optional: RB_HHD, the qualifier of the
// argument check, which the host side of the device build calls too (default: RB_HD).  Inside one phase no lane reads
// what another lane writes, so the single-threaded host build runs the very same phases.
//
// A live hypothesis of iteration i is (tokens y, frame t, symbols emitted at this frame n_sym, score s) with
// t + len(y) = i, and the live rows of a beam spell pairwise different sequences (they are the merged survivors of the
// iteration before).  Candidate e = h * (K + 1) + c of slot h: c = 0 the blank extension (y, t + 1, 0, s + lpb[h]),
// c = 1..K the label extension (y + lab[h][c-1], t, n_sym + 1, s + val[h][c-1]) - present only while
// n_sym < max_symbols and len(y) < max_len and lab >= 0.  Candidate order = ascending e.
// Two candidates spell the same sequence only as blank(h) and label(g, k) with y_h = y_g + k (equal lengths force
// equal frames); the pair becomes one candidate at the position of the earlier of the two with the float64 logaddexp of
// the two scores and every other field of the better one (the earlier on a tie).
#pragma once
#include <stdint.h>

#ifndef RB_HHD
#define RB_HHD RB_HD
#endif
#define RB_MAX_BEAM 32
#define RB_MAX_ENTRIES (RB_MAX_BEAM * (RB_MAX_BEAM + 1))

// logaddexp in float64 from +, -, *, / alone, in one fixed order: the host build, the kernel and the reference agree to
// the bit (no libm call whose last bit differs between implementations).  |error| < 1e-15 + 4e-18.
RB_HD inline double rb_lae(double a, double b) {
    const double m = a > b ? a : b;
    if (m == -INFINITY) return m;
    const double t = a > b ? a - b : b - a;          // >= 0, +inf when one side is -inf
    if (!(t < 40.0)) return m;                       // exp(-40) = 4e-18
    // u = exp(-t) = 2^-n exp(x), |x| <= 0.35
    const double nf = floor(t * 1.4426950408889634 + 0.5);
    const double x = -((t - nf * 0.693147180369123816490) - nf * 1.90821492927058770002e-10);
    double p = 1.0;
    for (int j = 14; j >= 1; --j) p = 1.0 + (x / (double)j) * p;
    double sc = 1.0, hf = 0.5;
    for (int n = (int)nf; n > 0; n >>= 1) {
        if (n & 1) sc = sc * hf;
        hf = hf * hf;
    }
    const double u = p * sc;
    // log1p(u) = 2 atanh(u / (2 + u)), 0 < u <= 1
    const double s = u / (2.0 + u), s2 = s * s;
    double q = 0.0;
    for (int j = 19; j >= 0; --j) q = 1.0 / (double)(2 * j + 1) + s2 * q;
    return m + (2.0 * s) * q;
}

struct RBState {                    // one utterance; every pointer is this utterance's slice
    int W, K, Tb, max_symbols, max_len;
    int64_t tok_stride;             // ints between two token rows (>= max_len)
    int64_t row0, rows;             // first global row of the utterance (b * W) and B * W
    // the table of the row pass
    const float *lpb;               // [W]
    const float *val;               // [W][K]
    const int32_t *lab;             // [W][K]
    // current beam (read) and next beam (written)
    const int32_t *c_live, *c_t, *c_sym, *c_len, *c_tok;
    const double *c_score;
    int32_t *n_live, *n_t, *n_sym, *n_len, *n_tok;
    double *n_score;
    // finished list: current (read) and next (written), sorted by score descending
    const int32_t *cf_n, *cf_len, *cf_tok;
    const double *cf_score;
    int32_t *nf_n, *nf_len, *nf_tok;
    double *nf_score;
    // what drives the state gathers of the caller, per row of the NEXT beam
    int64_t *parent;                // global row of the hypothesis the row continues
    int64_t *last_tok;              // the label it appended (0 without one)
    int32_t *emit;                  // 1: it appended a label
    int64_t *sel;                   // own global row + emit * rows: index into cat([kept, stepped])
    int64_t *lm_sel;                // emit ? rows + own global row : parent: index into cat([kept LM rows, stepped LM rows])
    // scratch (LDS on the device)
    double *e_sc;                   // [RB_MAX_ENTRIES]
    int32_t *e_src;                 // [RB_MAX_ENTRIES] candidate whose fields the entry carries
    unsigned char *e_alive;         // [RB_MAX_ENTRIES]
    int32_t *order;                 // [W] candidate of rank r, -1 beyond the last
    int32_t *r_fin;                 // [W] survivor r leaves for the finished list
    double *f_sc;                   // [2W] scores of the finished list followed by the new finishers
};

RB_HD inline bool rb_expands(const RBState &s, int h) {
    return s.c_sym[h] < s.max_symbols && s.c_len[h] < s.max_len && s.c_len[h] >= 0;
}

// token `pos` of the sequence candidate e spells (pos < its length)
RB_HD inline int32_t rb_cand_tok(const RBState &s, int e, int pos) {
    const int h = e / (s.K + 1), c = e % (s.K + 1);
    return pos < s.c_len[h] ? s.c_tok[(int64_t)h * s.tok_stride + pos] : s.lab[h * s.K + c - 1];
}

RB_HD inline void rb_select(const RBState &s) {
    const int W = s.W, K = s.K, K1 = K + 1;
    int nl = s.c_live[0];
    nl = nl < 0 ? 0 : (nl > W ? W : nl);
    const int N = nl * K1;

    // ---- P1: the candidates
    RB_FOR(e, N) {
        const int h = e / K1, c = e % K1;
        bool alive = true;
        double sc = s.c_score[h];
        if (c == 0) {
            sc += (double)s.lpb[h];
        } else {
            const int32_t k = s.lab[h * K + c - 1];
            alive = rb_expands(s, h) && k >= 0;
            sc += (double)s.val[h * K + c - 1];
        }
        s.e_sc[e] = sc;
        s.e_src[e] = e;
        s.e_alive[e] = alive ? 1 : 0;
    }
    RB_FOR(r, W) s.order[r] = -1;
    RB_SYNC();

    // ---- P2: merge blank(h) with label(g, k) where y_h = y_g + k.  A blank pairs with at most one label entry and a
    // label entry with at most one blank (the rows of a beam differ), so no two lanes touch the same entry.
    RB_FOR(p, nl * nl) {
        const int h = p / nl, g = p % nl;
        const int lh = s.c_len[h], lg = s.c_len[g];
        if (h != g && lg >= 0 && lh == lg + 1 && lh <= s.max_len && rb_expands(s, g)) {
            const int32_t k = s.c_tok[(int64_t)h * s.tok_stride + lg];
            int c = -1;
            for (int q = 0; q < K; ++q)
                if (s.lab[g * K + q] == k && k >= 0) {
                    c = q;
                    break;
                }
            bool same = c >= 0;
            for (int pos = 0; same && pos < lg; ++pos)
                same = s.c_tok[(int64_t)h * s.tok_stride + pos] == s.c_tok[(int64_t)g * s.tok_stride + pos];
            if (same) {
                const int e1 = h * K1, e2 = g * K1 + 1 + c;
                const int first = e1 < e2 ? e1 : e2, second = e1 < e2 ? e2 : e1;
                const double a = s.e_sc[first], b = s.e_sc[second];
                s.e_sc[first] = rb_lae(a, b);
                s.e_src[first] = a >= b ? first : second;
                s.e_alive[second] = 0;
            }
        }
    }
    RB_SYNC();

    // ---- P3: rank by score, ties in candidate order; ranks are dense, the first W stay
    RB_FOR(e, N) {
        if (s.e_alive[e]) {
            const double v = s.e_sc[e];
            int r = 0;
            for (int f = 0; f < e; ++f) r += (s.e_alive[f] && s.e_sc[f] >= v) ? 1 : 0;
            for (int f = e + 1; f < N; ++f) r += (s.e_alive[f] && s.e_sc[f] > v) ? 1 : 0;
            if (r < W) s.order[r] = e;
        }
    }
    RB_SYNC();

    // ---- P4: which survivors finish; the candidates of the finished list
    const int nfc = s.cf_n[0] < 0 ? 0 : (s.cf_n[0] > W ? W : s.cf_n[0]);
    RB_FOR(r, W) {
        const int e = s.order[r];
        int fin = 0;
        if (e >= 0) {
            const int src = s.e_src[e], par = src / K1;
            fin = (s.c_t[par] + (src % K1 == 0 ? 1 : 0)) >= s.Tb ? 1 : 0;
        }
        s.r_fin[r] = fin;
        if (r < nfc) s.f_sc[r] = s.cf_score[r];
    }
    RB_SYNC();
    RB_FOR(r, W) {                  // new finishers follow the list, in rank order
        if (s.r_fin[r]) {
            int j = nfc;
            for (int q = 0; q < r; ++q) j += s.r_fin[q];
            s.f_sc[j] = s.e_sc[s.order[r]];
        }
    }
    RB_SYNC();

    // ---- P5: the next beam (live survivors, packed in rank order) and the next finished list
    int n_new = 0, n_finish = 0;
    for (int q = 0; q < W; ++q) {
        if (s.order[q] >= 0 && !s.r_fin[q]) ++n_new;
        n_finish += s.r_fin[q];
    }
    const int nu = nfc + n_finish;                  // entries of the union, <= 2W
    RB_FOR(r, W) {
        const int e = s.order[r];
        if (e >= 0) {
            const int src = s.e_src[e], par = src / K1, c = src % K1;
            const int em = c > 0 ? 1 : 0;
            const int len = s.c_len[e / K1] + (e % K1 > 0 ? 1 : 0);
            if (!s.r_fin[r]) {
                int li = 0;
                for (int q = 0; q < r; ++q) li += (s.order[q] >= 0 && !s.r_fin[q]) ? 1 : 0;
                s.n_t[li] = s.c_t[par] + (em ? 0 : 1);
                s.n_sym[li] = em ? s.c_sym[par] + 1 : 0;
                s.n_len[li] = len;
                s.n_score[li] = s.e_sc[e];
                s.parent[li] = s.row0 + par;
                s.last_tok[li] = em ? (int64_t)s.lab[par * K + c - 1] : 0;
                s.emit[li] = em;
                s.sel[li] = s.row0 + li + (em ? s.rows : 0);
                s.lm_sel[li] = em ? s.rows + s.row0 + li : s.row0 + par;
            }
        }
        if (r >= n_new) {           // a dead row: identity indices, nothing emitted
            s.n_t[r] = 0; s.n_sym[r] = 0; s.n_len[r] = 0; s.n_score[r] = 0.0;
            s.parent[r] = s.row0 + r; s.last_tok[r] = 0; s.emit[r] = 0;
            s.sel[r] = s.row0 + r; s.lm_sel[r] = s.row0 + r;
        }
    }
    if (s.max_len > 0) {
        RB_FOR(z, W * s.max_len) {
            const int r = z / s.max_len, pos = z % s.max_len;
            const int e = s.order[r];
            if (e >= 0 && !s.r_fin[r]) {
                int li = 0;
                for (int q = 0; q < r; ++q) li += (s.order[q] >= 0 && !s.r_fin[q]) ? 1 : 0;
                const int len = s.c_len[e / K1] + (e % K1 > 0 ? 1 : 0);
                if (pos < len) s.n_tok[(int64_t)li * s.tok_stride + pos] = rb_cand_tok(s, e, pos);
            }
        }
    }
    // union entry j: j < nfc an entry of the list, else finisher number j - nfc; earlier entries win ties
    RB_FOR(j, nu) {
        const double v = s.f_sc[j];
        int rank = 0;
        for (int q = 0; q < j; ++q) rank += s.f_sc[q] >= v ? 1 : 0;
        for (int q = j + 1; q < nu; ++q) rank += s.f_sc[q] > v ? 1 : 0;
        if (rank < W) {
            int len;
            if (j < nfc) {
                len = s.cf_len[j];
            } else {
                int r = 0, seen = nfc;
                for (; r < W; ++r)
                    if (s.r_fin[r] && seen++ == j) break;
                const int e = s.order[r];
                len = s.c_len[e / K1] + (e % K1 > 0 ? 1 : 0);
            }
            s.nf_len[rank] = len;
            s.nf_score[rank] = v;
        }
    }
    if (s.max_len > 0) {
        RB_FOR(z, nu * s.max_len) {
            const int j = z / s.max_len, pos = z % s.max_len;
            const double v = s.f_sc[j];
            int rank = 0;
            for (int q = 0; q < j; ++q) rank += s.f_sc[q] >= v ? 1 : 0;
            for (int q = j + 1; q < nu; ++q) rank += s.f_sc[q] > v ? 1 : 0;
            if (rank < W) {
                if (j < nfc) {
                    if (pos < s.cf_len[j])
                        s.nf_tok[(int64_t)rank * s.tok_stride + pos] = s.cf_tok[(int64_t)j * s.tok_stride + pos];
                } else {
                    int r = 0, seen = nfc;
                    for (; r < W; ++r)
                        if (s.r_fin[r] && seen++ == j) break;
                    const int e = s.order[r];
                    const int len = s.c_len[e / K1] + (e % K1 > 0 ? 1 : 0);
                    if (pos < len) s.nf_tok[(int64_t)rank * s.tok_stride + pos] = rb_cand_tok(s, e, pos);
                }
            }
        }
    }
    RB_FOR(one, 1) {
        s.n_live[0] = n_new;
        s.nf_n[0] = nu < W ? nu : W;
    }
}

// The batch: every state array is [2, B, ...] (beam buffer `cur` is read, the other written); the table and the gather
// outputs are [B * W, ...].  rb_bind points an RBState at utterance b (the scratch stays the caller's).
struct RBArgs {
    const float *lpb, *val;
    const int32_t *lab;
    const int64_t *enc_len;
    int B, T, W, K, max_symbols, max_len, cur;
    int64_t tok_stride;
    int32_t *n_live, *t_ptr, *n_sym, *n_tok, *tokens;
    double *score;
    int32_t *fin_n, *fin_len, *fin_tok;
    double *fin_score;
    int64_t *parent, *last_tok, *sel, *lm_sel;
    int32_t *emit;
};

RB_HD inline void rb_bind(const RBArgs &a, int b, RBState &s) {
    const int W = a.W;
    const int64_t B = a.B, c = a.cur ? 1 : 0, n = 1 - c;
    const int64_t u = b, rc = (c * B + u) * W, rn = (n * B + u) * W;
    const long long el = a.enc_len[b];
    s.W = W; s.K = a.K; s.max_symbols = a.max_symbols; s.max_len = a.max_len; s.tok_stride = a.tok_stride;
    s.Tb = el < 1 ? 1 : (el > a.T ? a.T : (int)el);
    s.row0 = u * W; s.rows = B * W;
    s.lpb = a.lpb + u * W; s.val = a.val + u * W * a.K; s.lab = a.lab + u * W * a.K;
    s.c_live = a.n_live + c * B + u; s.n_live = a.n_live + n * B + u;
    s.c_t = a.t_ptr + rc; s.n_t = a.t_ptr + rn;
    s.c_sym = a.n_sym + rc; s.n_sym = a.n_sym + rn;
    s.c_len = a.n_tok + rc; s.n_len = a.n_tok + rn;
    s.c_score = a.score + rc; s.n_score = a.score + rn;
    s.c_tok = a.tokens + rc * a.tok_stride; s.n_tok = a.tokens + rn * a.tok_stride;
    s.cf_n = a.fin_n + c * B + u; s.nf_n = a.fin_n + n * B + u;
    s.cf_len = a.fin_len + rc; s.nf_len = a.fin_len + rn;
    s.cf_score = a.fin_score + rc; s.nf_score = a.fin_score + rn;
    s.cf_tok = a.fin_tok + rc * a.tok_stride; s.nf_tok = a.fin_tok + rn * a.tok_stride;
    s.parent = a.parent + u * W; s.last_tok = a.last_tok + u * W; s.emit = a.emit + u * W;
    s.sel = a.sel + u * W; s.lm_sel = a.lm_sel + u * W;
}

// argument errors of the select step, shared by both builds (0 = fine)
RB_HHD inline int rb_args_bad(const RBArgs &a) {
    return a.B < 0 || a.T <= 0 || a.W < 1 || a.W > RB_MAX_BEAM || a.K < 1 || a.K > a.W || a.max_symbols < 0 ||
           a.max_len < 0 || a.tok_stride < a.max_len || a.tok_stride < 1 || (a.cur != 0 && a.cur != 1);
}
