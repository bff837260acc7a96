// Pure-CTC prefix beam search, one frame of it, as data-parallel phases over flat arrays.
//
// Restates the per-frame body of the reference's CTCBeamDecoder.forward (src/ctc.py:262-350, Graves 2014
// Algo. 1 with the reference's bookkeeping) without Python objects, deep copies or string sorts:
//   * a hypothesis is a row of the beam tables: tokens, the decimal string of the tokens (the reference
//     orders and de-duplicates the expanded beam by sorting on ''.join(str(s) for s in y), src/ctc.py:144-146,
//     320-329 - a sort key that different sequences can share, e.g. [1,23] and [12,3]; reproducing its ORDER is
//     what makes the kept / dropped hypotheses identical), Pr-(y,t), Pr+(y,t) in float64;
//   * an expanded entry is (parent row, appended token or none): its string is parent string + digits, so two
//     entries compare in O(1) from PAIR TABLES over the <= W parent rows: length of the longest common string
//     prefix, the sign of the first differing character, the next characters of the longer string when one
//     parent's string is a prefix of the other's, and whether one token sequence is a prefix of the other;
//   * the pair tables of the NEXT beam follow from this frame's tables and the chosen (parent, token) entries in
//     O(1) per pair as well (a child's string is its parent's plus <= 5 digits) - no O(length) loop anywhere;
//   * "stable sort" = rank by counting (entries x entries), run boundaries = adjacent sequence inequality,
//     winners = first maximum of a run, pruning = rank by score.
// The arithmetic follows the reference under numpy >= 2 promotion rules (python floats are weak): CTC and LM
// log-probs are float32, `lm_w * lm[k]` and `ctc[k] + lm_w * lm[k]` round to float32, everything accumulated
// into a hypothesis is float64 (np.logaddexp on float64).
//
// This file is compiled twice: into the device kernel (prefix_beam.hip, one workgroup per utterance, PB_FOR =
// workgroup-strided loop, PB_SYNC = __syncthreads) and - by tests/ only - into a single-threaded host library
// that checks the ALGORITHM against the reference's golden hypotheses without a GPU (the product never calls
// the host build).
//
// Required before inclusion: PB_HD (function qualifier), PB_FOR(i, n) { ... }, PB_SYNC(), PB_TID0 (true for the
// one thread that publishes scalars), pb_exp(double), pb_log1p(double), PB_STAMP(k) (phase time stamp; may be empty;
// it may refer to pb_frame's template argument PB_WG0: 1 = the launch has several workgroups, stamp from the first).
#pragma once
#include <stdint.h>

#define PB_LOG_ZERO (-10000000.0)           /* src/ctc.py:9 */
#define PB_MAX_ENTRIES 1024
#define PB_MAX_BEAM 32
#define PB_PAIRS (PB_MAX_BEAM * PB_MAX_BEAM)

struct PBBeam {                             // one of the two beam buffers (global memory, kept between launches)
    int *len, *slen;                        // [W] tokens / characters of the decimal string
    int *tok;                               // [W][Lcap]
    unsigned char *str;                     // [W][Scap]
    double *pb, *pnb;                       // [W] Pr-(y,t), Pr+(y,t)
    int *upd;                               // [W] CTCHypothesis.updated_lm
    // pair tables, [PB_PAIRS] indexed i * PB_MAX_BEAM + j
    int *lcp;                               // longest common prefix of the strings of rows i and j
    signed char *dif;                       // lcp < both lengths: sign of str_i[lcp] - str_j[lcp]
    unsigned char *pre;                     // tokens of row i are a prefix of the tokens of row j
    unsigned long long *tail;               // str_i is a prefix of str_j: the next <= 6 characters of str_j (count + chars)
};

struct PBState {
    int W, C, V, Lcap, Scap;
    PBBeam beam[2];
    int *nb;                                // [2] live rows of each buffer
    // per-frame scratch (LDS on the device)
    int *e_par, *e_tok, *sorted, *m_list, *order, *off, *fin, *cand;   // cand [W][C]
    int *r_len, *r_slen, *r_last;           // [W] copies of the current rows' lengths / last token
    int *t_lcp;                             // [PB_PAIRS] this frame's pair tables (copies of the beam's)
    signed char *t_dif;
    unsigned char *t_pre;
    unsigned long long *t_tail;
    unsigned long long *t_tkey;             // [PB_PAIRS] t_tail as a left-aligned big-endian key (+ count in the low byte)
    unsigned long long *e_lk;               // [PB_MAX_ENTRIES] an entry's digits as a left-aligned big-endian key
    double *e_pb, *e_pnb, *e_sc, *key, *s_pb1, *s_pnb1, *s_same, *s_diff;   // key [PB_MAX_ENTRIES]: P5 sort keys
    unsigned long long *e_dig;
    unsigned char *bnd;
    int *scal;                              // [4]: N, m, nb_new
    double *w_key;                          // device only: [8 waves][W] stage-1 survivors of the score selection
    int *w_pos;
    // outputs for the LM bookkeeping of the caller ([W] each, valid after a frame)
    int *out_parent, *out_last, *out_gidx;
};

PB_HD inline double pb_lae(double x, double y) {          // np.logaddexp (npy_logaddexp)
    if (x == y) return x + 0.693147180559945309417232121458176568;
    const double t = x - y;
    if (t > 0) return x + pb_log1p(pb_exp(-t));
    if (t <= 0) return y + pb_log1p(pb_exp(t));
    return t;
}

// packed short strings: byte 0 = count (<= 7), bytes 1.. = characters
PB_HD inline unsigned long long pb_digits(int k) {        // str(k)
    if (k < 0) return 0ull;
    unsigned char d[12];
    int n = 0;
    unsigned v = (unsigned)k;
    do { d[n++] = (unsigned char)('0' + v % 10u); v /= 10u; } while (v && n < 7);
    unsigned long long r = (unsigned long long)n;
    for (int i = 0; i < n; ++i) r |= (unsigned long long)d[n - 1 - i] << (8 * (i + 1));
    return r;
}
// the characters of a packed short string as a big-endian integer, first character in the top byte: for strings
// without zero bytes, lexicographic order (a proper prefix sorts first) == integer order of these keys
PB_HD inline unsigned long long pb_left_key(unsigned long long pk) {
    const int n = (int)(pk & 0xff);
    unsigned long long k = 0ull;
    for (int c = 0; c < n && c < 7; ++c) k |= ((pk >> (8 * (c + 1))) & 0xffull) << (8 * (7 - c));
    return k;
}
// first six characters of (tail characters ++ digits) as a key: tkey = left-aligned tail (count in the low byte)
PB_HD inline unsigned long long pb_rem_key(unsigned long long tkey, unsigned long long lk) {
    const int cnt = (int)(tkey & 0xff);
    const unsigned long long t = tkey & ~0xffull;
    return (cnt >= 6 ? t : (t | (lk >> (8 * cnt)))) & 0xffffffffffff0000ull;
}
PB_HD inline int pb_pk_at(unsigned long long pk, int d) {   // character d of a packed string, -1 beyond its end
    return (d >= 0 && d < (int)(pk & 0xff)) ? (int)((pk >> (8 * (d + 1))) & 0xff) : -1;
}

// Character `pos` (>= l) of the string of an expanded entry (parent row i + digits dg) while it is compared with
// an entry of parent row j, where l = lcp(str_i, str_j) = min(len_i, len_j) (one parent string is a prefix of the
// other).  Inside the parent: only reachable when str_j is the shorter one, from tail[j][i].
PB_HD inline int pb_entry_char(int pos, int li, int lj, unsigned long long tail_ji, unsigned long long dg) {
    if (pos < li) return pb_pk_at(tail_ji, pos - lj);
    return pb_pk_at(dg, pos - li);
}

// Compare the strings (parent i + d1) and (parent j + d2): result in `sign` (-1 / 0 / +1), `lcp_out` = length of
// their common prefix.  li, lj parent string lengths; l, dif, tail_ij, tail_ji from the pair tables (i != j) or
// l = li for i == j.  O(1): at most 7 characters are looked at.
PB_HD inline void pb_cmp_ext(int li, int lj, int l, int dif, unsigned long long tail_ij, unsigned long long tail_ji,
                             unsigned long long d1, unsigned long long d2, int &sign, int &lcp_out) {
    const int mn = li < lj ? li : lj;
    if (l < mn) { sign = dif; lcp_out = l; return; }
    int pos = l;
    for (int it = 0; it < 7; ++it, ++pos) {
        const int ca = pb_entry_char(pos, li, lj, tail_ji, d1), cb = pb_entry_char(pos, lj, li, tail_ij, d2);
        if (ca != cb) { sign = ca < cb ? -1 : 1; lcp_out = pos; return; }
        if (ca < 0) { sign = 0; lcp_out = pos; return; }
    }
    sign = 0; lcp_out = pos;                      // unreachable: an entry adds at most 5 characters
}

PB_HD inline int pb_cmp_str(const PBState &s, int e1, int e2) {
    const int i = s.e_par[e1], j = s.e_par[e2], p = i * PB_MAX_BEAM + j, q = j * PB_MAX_BEAM + i;
    int sign, l;
    pb_cmp_ext(s.r_slen[i], s.r_slen[j], i == j ? s.r_slen[i] : s.t_lcp[p], s.t_dif[p], s.t_tail[p], s.t_tail[q],
               s.e_dig[e1], s.e_dig[e2], sign, l);
    return sign;
}

// tokens of (row i + k1) are a prefix of the tokens of (row j + k2)?  (k < 0: the row itself)
PB_HD inline bool pb_pre_ext(const PBState &s, const PBBeam &b, int i, int k1, int j, int k2) {
    const int li = s.r_len[i], lj = s.r_len[j];
    const int la = li + (k1 >= 0 ? 1 : 0), lb = lj + (k2 >= 0 ? 1 : 0);
    if (la > lb) return false;
    const bool pij = i == j || s.t_pre[i * PB_MAX_BEAM + j];
    if (k1 < 0) {
        if (li <= lj) return pij;
        // li == lj + 1 (only possible with k2 >= 0): y_i == y_j + [k2]
        return (s.t_pre[j * PB_MAX_BEAM + i] != 0) && s.r_last[i] == k2;
    }
    if (li == lj) return pij && k2 >= 0 && k1 == k2;                   // equal-length parents: same appended token
    // li < lj: y_i + [k1] must be a prefix of y_j itself
    return pij && b.tok[(size_t)j * s.Lcap + li] == k1;
}

// do two expanded entries spell the same token sequence (CTCHypothesis.check_same)?
PB_HD inline bool pb_same_seq(const PBState &s, const PBBeam &b, int e1, int e2) {
    const int i = s.e_par[e1], j = s.e_par[e2], k1 = s.e_tok[e1], k2 = s.e_tok[e2];
    const int la = s.r_len[i] + (k1 >= 0 ? 1 : 0), lb = s.r_len[j] + (k2 >= 0 ? 1 : 0);
    return la == lb && pb_pre_ext(s, b, i, k1, j, k2);
}

// One frame.  x = ctc log-probs of the frame [V] (float32); lm = per-row RNN-LM log-probs [W][V] or null
// (lw = float32(lm_weight)); s.cand [nb][C] = this frame's candidate symbols per row (filled by the caller's
// ranking phase); last_frame selects the length-normalised final score; lm_step_follows = an LM update will be
// run after this frame (t < T - 1) so out_gidx / upd are set accordingly.
template <int PB_WG0 = 0>
PB_HD inline void pb_frame(const PBState &s, int cur, const float *x, const float *lm, float lw, int last_frame,
                           int lm_step_follows) {
    const PBBeam &b = s.beam[cur];
    const PBBeam &n = s.beam[1 - cur];
    const int nb = s.nb[cur], C = s.C, W = s.W;

    // ---- P0: this frame's row / pair tables into the scratch
    PB_FOR(i, nb) {
        const int li = b.len[i];
        s.r_len[i] = li; s.r_slen[i] = b.slen[i];
        s.r_last[i] = li > 0 ? b.tok[(size_t)i * s.Lcap + li - 1] : -1;
    }
    PB_FOR(p, nb * nb) {
        const int q = (p / nb) * PB_MAX_BEAM + p % nb;
        s.t_lcp[q] = b.lcp[q]; s.t_dif[q] = b.dif[q]; s.t_pre[q] = b.pre[q]; s.t_tail[q] = b.tail[q];
        s.t_tkey[q] = pb_left_key(b.tail[q]) | (b.tail[q] & 0xffull);
    }
    PB_SYNC();
    PB_STAMP(1);

    // ---- P1: per row: Pr+ / Pr- of the row itself at this frame, the two bases its children use
    PB_FOR(i, nb) {
        const int li = s.r_len[i], last = s.r_last[i];
        const int fin = li > 0 && last == 1;         // <eos> = 1: finished, copied through unchanged
        const double pbo = b.pb[i], pnbo = b.pnb[i];
        double pnb1 = pnbo, pb1 = pbo;
        if (!fin) {
            if (li > 0) {
                pnb1 = pnbo + (double)x[last];                                   // update_Pr_nblank
                for (int j = 0; j < nb; ++j)                                     // first other row spelling y[:-1]
                    if (j != i && s.r_len[j] == li - 1 && s.t_pre[j * PB_MAX_BEAM + i]) {
                        const float lmp = lm ? lw * lm[(size_t)j * s.V + last] : 0.f;
                        const float cl = x[last] + lmp;
                        const bool rep = li >= 2 && last == b.tok[(size_t)i * s.Lcap + li - 2];
                        const double base = rep ? b.pb[j] : pb_lae(b.pb[j], b.pnb[j]);
                        pnb1 = pb_lae(pnb1, (double)cl + base);                   // update_Pr_nblank_prefix
                        break;
                    }
            }
            pb1 = pb_lae(pnbo, pbo) + (double)x[0];                              // update_Pr_blank (blank = 0)
        }
        s.fin[i] = fin;
        s.s_pb1[i] = pb1; s.s_pnb1[i] = pnb1;
        s.s_same[i] = pbo;                            // child repeats the last token: only Pr-
        s.s_diff[i] = pb_lae(pbo, pnbo);
        int off = 0;
        for (int q = 0; q < i; ++q) off += (s.r_len[q] > 0 && s.r_last[q] == 1) ? 1 : C + 1;
        s.off[i] = off;
        if (i == nb - 1) s.scal[0] = off + (fin ? 1 : C + 1);
    }
    PB_SYNC();
    PB_STAMP(2);

    // ---- P2: the expanded beam in the reference's order: per row its C children, then the row itself
    PB_FOR(q, nb * (C + 1)) {
        const int i = q / (C + 1), c = q % (C + 1);
        if (s.fin[i]) {
            if (c == 0) {
                const int e = s.off[i];
                s.e_par[e] = i; s.e_tok[e] = -1; s.e_dig[e] = 0ull;
                s.e_pb[e] = b.pb[i]; s.e_pnb[e] = b.pnb[i];
                s.e_sc[e] = pb_lae(b.pb[i], b.pnb[i]);
            }
        } else {
            const int e = s.off[i] + c;
            s.e_par[e] = i;
            if (c < C) {
                const int k = s.cand[i * C + c];
                const float lmp = lm ? lw * lm[(size_t)i * s.V + k] : 0.f;
                const float cl = x[k] + lmp;
                s.e_tok[e] = k; s.e_dig[e] = pb_digits(k);
                s.e_pb[e] = PB_LOG_ZERO;
                s.e_pnb[e] = (double)cl + (s.r_last[i] == k ? s.s_same[i] : s.s_diff[i]);   // add_token
                s.e_sc[e] = pb_lae(PB_LOG_ZERO, s.e_pnb[e]);
            } else {
                s.e_tok[e] = -1; s.e_dig[e] = 0ull;
                s.e_pb[e] = s.s_pb1[i]; s.e_pnb[e] = s.s_pnb1[i];
                s.e_sc[e] = pb_lae(s.s_pb1[i], s.s_pnb1[i]);
            }
        }
    }
    PB_SYNC();
    PB_STAMP(3);
    const int N = s.scal[0];
    PB_FOR(e, N) s.e_lk[e] = pb_left_key(s.e_dig[e]);
    PB_SYNC();

    // ---- P3: sorted(B_new, key=get_string) - stable: rank = entries that sort strictly before
    // (the entries of a parent whose string differs from this entry's parent string inside both strings all
    // fall on the same side - decided by one table look-up; only entries of the same or of a prefix-related
    // parent are compared one by one: ~W + a few x (C + 1) comparisons per entry instead of W x (C + 1))
    PB_FOR(e, N) {
        const int i = s.e_par[e], li = s.r_slen[i];
        int r = 0;
        for (int j = 0; j < nb; ++j) {
            const int f0 = s.off[j], cnt = s.fin[j] ? 1 : C + 1, lj = s.r_slen[j];
            const int l = s.t_lcp[j * PB_MAX_BEAM + i];
            if (j != i && l < (li < lj ? li : lj)) {
                r += s.t_dif[j * PB_MAX_BEAM + i] < 0 ? cnt : 0;
                continue;
            }
            // same or prefix-related parent: what differs starts at position l; at most six characters decide
            // (an entry adds <= 5), so each side is one 64-bit key and the comparison one integer compare
            const unsigned long long ke = s.e_lk[e];
            if (j == i) {
                for (int f = f0; f < f0 + cnt; ++f) {
                    const unsigned long long kf = s.e_lk[f];
                    r += (f != e && (kf < ke || (kf == ke && f < e))) ? 1 : 0;
                }
            } else if (lj <= li) {                 // str_j is a prefix of (or equal to) str_i
                const unsigned long long kE = pb_rem_key(s.t_tkey[j * PB_MAX_BEAM + i], ke);
                for (int f = f0; f < f0 + cnt; ++f) {
                    const unsigned long long kf = s.e_lk[f] & 0xffffffffffff0000ull;
                    r += (kf < kE || (kf == kE && f < e)) ? 1 : 0;
                }
            } else {                               // str_i is a proper prefix of str_j
                const unsigned long long tk = s.t_tkey[i * PB_MAX_BEAM + j], kE = ke & 0xffffffffffff0000ull;
                for (int f = f0; f < f0 + cnt; ++f) {
                    const unsigned long long kf = pb_rem_key(tk, s.e_lk[f]);
                    r += (kf < kE || (kf == kE && f < e)) ? 1 : 0;
                }
            }
        }
        s.sorted[r] = e;
    }
    PB_SYNC();
    PB_STAMP(4);

    // ---- P4: runs of equal sequences; the survivor of a run is its first maximum (strict > replaces)
    PB_FOR(r, N) s.bnd[r] = r == 0 || !pb_same_seq(s, b, s.sorted[r - 1], s.sorted[r]);
    PB_SYNC();
    PB_STAMP(5);
    PB_FOR(r, N) {
        if (s.bnd[r]) {
            int best = s.sorted[r];
            for (int q = r + 1; q < N && !s.bnd[q]; ++q)
                if (s.e_sc[s.sorted[q]] > s.e_sc[best]) best = s.sorted[q];
            int idx = 0;
            const unsigned *bw = reinterpret_cast<const unsigned *>(s.bnd);     // flags are 0 / 1 bytes: 4 per word
            for (int q = 0; q < (r >> 2); ++q) idx += (int)((bw[q] * 0x01010101u) >> 24);
            for (int q = r & ~3; q < r; ++q) idx += s.bnd[q];
            s.m_list[idx] = best;
        }
        if (r == N - 1) {
            int m = 0;
            const unsigned *bw = reinterpret_cast<const unsigned *>(s.bnd);
            for (int q = 0; q < (N >> 2); ++q) m += (int)((bw[q] * 0x01010101u) >> 24);
            for (int q = N & ~3; q < N; ++q) m += s.bnd[q];
            s.scal[1] = m;
        }
    }
    PB_SYNC();
    PB_STAMP(6);
    const int m = s.scal[1];

    // ---- P5: sorted(B, reverse=True, key=score) - stable - and the cut to W rows (keys computed once)
    PB_FOR(a, m) {
        const int ea = s.m_list[a];
        const int la = s.r_len[s.e_par[ea]] + (s.e_tok[ea] >= 0 ? 1 : 0);
        s.key[a] = (last_frame && la > 0) ? s.e_sc[ea] / (double)la : s.e_sc[ea];
    }
    PB_SYNC();
    PB_STAMP(12);
#ifdef PB_TOPW
    PB_TOPW(s, m, W);                               // device: two-stage selection of the W best (same total order)
#else
    PB_FOR(a, m) {
        const double ka = s.key[a];
        int r = 0;
        for (int c = 0; c < a; ++c) r += (s.key[c] >= ka) ? 1 : 0;          // earlier entries win ties
        for (int c = a + 1; c < m; ++c) r += (s.key[c] > ka) ? 1 : 0;
        if (r < W) s.order[r] = s.m_list[a];
    }
    PB_SYNC();
#endif
    PB_STAMP(7);
    const int nbn = m < W ? m : W;

    // ---- P6: the new beam (other buffer): tokens, strings, probabilities, LM bookkeeping
    PB_FOR(z, nbn * s.Lcap) {
        const int r = z / s.Lcap, pos = z % s.Lcap;
        const int e = s.order[r], i = s.e_par[e], li = s.r_len[i];
        if (pos < li) n.tok[(size_t)r * s.Lcap + pos] = b.tok[(size_t)i * s.Lcap + pos];
        else if (pos == li && s.e_tok[e] >= 0) n.tok[(size_t)r * s.Lcap + pos] = s.e_tok[e];
    }
    PB_FOR(z, nbn * s.Scap) {
        const int r = z / s.Scap, pos = z % s.Scap;
        const int e = s.order[r], i = s.e_par[e], sl = s.r_slen[i];
        if (pos < sl) n.str[(size_t)r * s.Scap + pos] = b.str[(size_t)i * s.Scap + pos];
        else {
            const int c = pb_pk_at(s.e_dig[e], pos - sl);
            if (c >= 0) n.str[(size_t)r * s.Scap + pos] = (unsigned char)c;
        }
    }
    PB_FOR(r, W) {
        if (r < nbn) {
            const int e = s.order[r], i = s.e_par[e], k = s.e_tok[e];
            const int ln = s.r_len[i] + (k >= 0 ? 1 : 0);
            n.len[r] = ln;
            n.slen[r] = s.r_slen[i] + (int)(s.e_dig[e] & 0xff);
            n.pb[r] = s.e_pb[e]; n.pnb[r] = s.e_pnb[e];
            const int upd = k >= 0 ? 0 : b.upd[i];
            const int step = lm_step_follows && ln > 0 && !upd;       // src/ctc.py:342-350
            n.upd[r] = upd | step;
            s.out_parent[r] = i;
            s.out_last[r] = ln > 0 ? (k >= 0 ? k : s.r_last[i]) : 0;
            s.out_gidx[r] = step ? W + r : i;
        } else {
            s.out_parent[r] = 0; s.out_last[r] = 0; s.out_gidx[r] = 0;
        }
    }
    // pair tables of the new beam from this frame's tables, O(1) per pair
    PB_FOR(z, nbn * nbn) {
        const int ra = z / nbn, rb = z % nbn, q = ra * PB_MAX_BEAM + rb;
        const int ea = s.order[ra], eb = s.order[rb];
        const int i = s.e_par[ea], j = s.e_par[eb], k1 = s.e_tok[ea], k2 = s.e_tok[eb];
        const int p = i * PB_MAX_BEAM + j, pt = j * PB_MAX_BEAM + i;
        int sign, l;
        pb_cmp_ext(s.r_slen[i], s.r_slen[j], i == j ? s.r_slen[i] : s.t_lcp[p], s.t_dif[p], s.t_tail[p], s.t_tail[pt],
                   s.e_dig[ea], s.e_dig[eb], sign, l);
        n.lcp[q] = l;
        n.dif[q] = (signed char)sign;
        n.pre[q] = ra == rb ? 1 : (pb_pre_ext(s, b, i, k1, j, k2) ? 1 : 0);
    }
    PB_SYNC();
    PB_STAMP(8);
    // ... and the characters that follow a string which is a prefix of another row's string (read back from the
    // rows just written: <= 6 bytes per such pair)
    PB_FOR(z, nbn * nbn) {
        const int ra = z / nbn, rb = z % nbn, q = ra * PB_MAX_BEAM + rb;
        const int la = n.slen[ra], lb = n.slen[rb];
        unsigned long long t = 0ull;
        if (ra != rb && n.lcp[q] == la && la <= lb) {
            const unsigned char *S = n.str + (size_t)rb * s.Scap;
            int cnt = lb - la < 6 ? lb - la : 6;
            t = (unsigned long long)cnt;
            for (int c = 0; c < cnt; ++c) t |= (unsigned long long)S[la + c] << (8 * (c + 1));
        }
        n.tail[q] = t;
    }
    PB_SYNC();
    PB_STAMP(9);
    if (PB_TID0) { s.nb[1 - cur] = nbn; s.scal[2] = nbn; }
    PB_SYNC();
    PB_STAMP(10);
}

// Lock-step search of U utterances (one LM batch of U * W rows, rows u*W .. u*W+W-1 = utterance u): the LM
// bookkeeping pb_frame left for the rows of beam buffer `buf` of utterance u, as GLOBAL row indices.  parent /
// gidx index cat([old rows, stepped rows]) of the U * W row batch: a row that inherits its state names its parent's
// old row, a row whose LM is stepped names its own row in the stepped half.  Dead rows keep their own state
// (identity) and feed token 0, so the batched LM step sees valid indices in every row.
PB_HD inline void pb_export_rows(const PBState &s, int buf, int u, int U, int *parent, int *last, int *gidx) {
    const int W = s.W, base = u * W, nbn = s.nb[buf];
    PB_FOR(r, W) {
        if (r < nbn) {
            const int g = s.out_gidx[r];
            parent[base + r] = base + s.out_parent[r];
            last[base + r] = s.out_last[r];
            gidx[base + r] = g >= W ? U * W + base + (g - W) : base + g;
        } else {
            parent[base + r] = base + r; last[base + r] = 0; gidx[base + r] = base + r;
        }
    }
}
