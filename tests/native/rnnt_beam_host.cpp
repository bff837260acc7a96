// TEST INFRASTRUCTURE ONLY: the select step of the transducer beam search
// (end-to-end-asr-pytorch_amd/csrc/rnnt_beam.inc, the very source the gfx950 kernel is built from) compiled for the host,
// so that tests/test_rnnt_beam_cpu.py can check it against the float64 reference without a GPU.
// The product never links or calls this file.  Built by the test with g++ -O2 -ffp-contract=off.
//
// With -DRNNT_BEAM_HOST_MAIN it is a stand-alone program for a sanitizer build (g++ -fsanitize=address,undefined): it
// runs whole searches on generated tables with exactly sized heap buffers and checks the invariants of the state
// (t + n_tok = iteration for every live row, live rows pairwise different, the finished list sorted, nothing live after
// the last iteration).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define RB_HD
#define RB_FOR(i, n) for (int i = 0; i < (n); ++i)
#define RB_SYNC() \
    do {          \
    } while (0)
#include "../../end-to-end-asr-pytorch_amd/csrc/rnnt_beam.inc"

extern "C" double rnntb_lae(double a, double b) { return rb_lae(a, b); }

// the arguments of asrk_rnnt_beam_select, host arrays; -1: an argument error
extern "C" int rnntb_select(const float *lpb, const float *val, const int32_t *lab, const int64_t *enc_len, int B, int T,
                            int W, int K, int max_symbols, int max_len, int64_t tok_stride, int cur, int32_t *n_live,
                            int32_t *t_ptr, int32_t *n_sym, int32_t *n_tok, double *score, int32_t *tokens,
                            int32_t *fin_n, int32_t *fin_len, double *fin_score, int32_t *fin_tok, int64_t *parent,
                            int64_t *last_tok, int32_t *emit, int64_t *sel, int64_t *lm_sel) {
    const RBArgs a{lpb,     val,    lab,     enc_len,   B,      T,      W,     K,       max_symbols,
                   max_len, cur,    tok_stride, n_live, t_ptr,  n_sym,  n_tok, tokens,  score,
                   fin_n,   fin_len, fin_tok, fin_score, parent, last_tok, sel,  lm_sel,  emit};
    if (rb_args_bad(a)) return -1;
    // exactly sized scratch: an index outside is a sanitizer report
    std::vector<double> e_sc((size_t)W * (K + 1)), f_sc(2 * (size_t)W);
    std::vector<int32_t> e_src((size_t)W * (K + 1)), order(W), r_fin(W);
    std::vector<unsigned char> e_alive((size_t)W * (K + 1));
    for (int b = 0; b < B; ++b) {
        RBState s;
        rb_bind(a, b, s);
        s.e_sc = e_sc.data();
        s.f_sc = f_sc.data();
        s.e_src = e_src.data();
        s.order = order.data();
        s.r_fin = r_fin.data();
        s.e_alive = e_alive.data();
        rb_select(s);
    }
    return 0;
}

#ifdef RNNT_BEAM_HOST_MAIN
int main() {
    unsigned seed = 2024;
    auto rnd = [&seed]() {
        seed = seed * 1664525u + 1013904223u;
        return (float)(seed >> 8) / (float)(1u << 24);
    };
    int bad = 0;
    const int shapes[][5] = {{1, 4, 3, 2, 5}, {2, 5, 4, 1, 3}, {3, 7, 3, 2, 0}, {8, 6, 5, 3, 6}, {32, 5, 40, 2, 4}};
    for (const auto &sh : shapes) {
        const int W = sh[0], T = sh[1], V = sh[2], max_symbols = sh[3], max_len = sh[4], B = 3;
        const int K = W < V - 1 ? W : V - 1;
        const int64_t Lc = max_len > 0 ? max_len : 1;
        const size_t bw = (size_t)B * W;
        std::vector<float> lpb(bw), val(bw * K);
        std::vector<int32_t> lab(bw * K), n_live(2 * B, 0), t_ptr(2 * bw, 0), n_sym(2 * bw, 0), n_tok(2 * bw, 0),
            tokens(2 * bw * Lc, 0), fin_n(2 * B, 0), fin_len(2 * bw, 0), fin_tok(2 * bw * Lc, 0), emit(bw);
        std::vector<double> score(2 * bw, 0.0), fin_score(2 * bw, 0.0);
        std::vector<int64_t> parent(bw), last_tok(bw), sel(bw), lm_sel(bw), enc_len(B);
        for (int b = 0; b < B; ++b) {
            enc_len[b] = 1 + (b * 2) % T;
            n_live[b] = 1;
        }
        for (int i = 0; i < T + max_len; ++i) {
            const int cur = i & 1;
            for (size_t r = 0; r < bw; ++r) {
                lpb[r] = std::log(0.05f + 0.9f * rnd());
                // labels: a rotation of 1..V-1, values descending on a coarse grid (ties), sometimes a short row
                const int rot = (int)(rnd() * (V - 1)), nk = rnd() < 0.8f ? K : (int)(rnd() * (K + 1));
                float v = -0.25f * (float)(int)(rnd() * 4);
                for (int c = 0; c < K; ++c) {
                    lab[r * K + c] = c < nk ? 1 + (rot + c) % (V - 1) : -1;
                    val[r * K + c] = c < nk ? v : -INFINITY;
                    v -= 0.25f * (float)(int)(rnd() * 3);
                }
            }
            if (rnntb_select(lpb.data(), val.data(), lab.data(), enc_len.data(), B, T, W, K, max_symbols, max_len, Lc,
                             cur, n_live.data(), t_ptr.data(), n_sym.data(), n_tok.data(), score.data(), tokens.data(),
                             fin_n.data(), fin_len.data(), fin_score.data(), fin_tok.data(), parent.data(),
                             last_tok.data(), emit.data(), sel.data(), lm_sel.data()) != 0) {
                std::printf("W %d: argument error\n", W);
                ++bad;
                break;
            }
            const size_t nb = (size_t)(1 - cur);
            for (int b = 0; b < B; ++b) {
                const size_t base = (nb * B + b) * W;
                const int nl = n_live[nb * B + b];
                if (nl < 0 || nl > W) ++bad;
                for (int h = 0; h < nl && h < W; ++h) {
                    if (t_ptr[base + h] + n_tok[base + h] != i + 1 || t_ptr[base + h] >= enc_len[b] ||
                        n_tok[base + h] > max_len) {
                        std::printf("W %d it %d utt %d row %d: t %d n_tok %d\n", W, i, b, h, t_ptr[base + h],
                                    n_tok[base + h]);
                        ++bad;
                    }
                    for (int g = 0; g < h; ++g) {
                        bool same = n_tok[base + g] == n_tok[base + h];
                        for (int q = 0; same && q < n_tok[base + h]; ++q)
                            same = tokens[(base + g) * Lc + q] == tokens[(base + h) * Lc + q];
                        if (same) {
                            std::printf("W %d it %d utt %d: rows %d and %d are equal\n", W, i, b, g, h);
                            ++bad;
                        }
                    }
                }
                for (int j = 1; j < fin_n[nb * B + b]; ++j)
                    if (!(fin_score[base + j - 1] >= fin_score[base + j])) ++bad;
            }
        }
        const size_t last = (size_t)((T + max_len) & 1);
        for (int b = 0; b < B; ++b)
            if (n_live[last * B + b] != 0 || fin_n[last * B + b] < 1) {
                std::printf("W %d utt %d: live %d finished %d at the end\n", W, b, n_live[last * B + b],
                            fin_n[last * B + b]);
                ++bad;
            }
    }
    std::printf("%d failures\n", bad);
    return bad ? 1 : 0;
}
#endif
