// TEST INFRASTRUCTURE ONLY: the transducer forced-alignment cell rule, walk, backtrace and token outputs
// (end-to-end-asr-pytorch_amd/csrc/rnnt_align.inc, the very source the gfx950 kernel is built from) compiled for the
// host, so that tests/test_rnnt_align_cpu.py can check them against the numpy reference without a GPU.
// The product never links or calls this file.  Built by the test with g++ -O2 -ffp-contract=off.
//
// With -DRNNT_ALIGN_HOST_MAIN it is a stand-alone program for a sanitizer build (g++ -fsanitize=address,undefined): it
// aligns a set of lattice shapes on generated log-probabilities with exactly sized buffers and checks that the path is
// a path (frames non-decreasing, labels_done consistent with them) and that the score is the sum along it.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define RNNT_HD
#include "../../end-to-end-asr-pytorch_amd/csrc/rnnt.inc"
#include "../../end-to-end-asr-pytorch_amd/csrc/rnnt_align.inc"

namespace {
struct NoSync {
    void operator()() const {}
};
// one lane at a time: the lane's bit of the word, where the kernel stores a wave's ballot
struct BitPut {
    unsigned long long *bp;
    int nslot;
    void operator()(int d, int u, bool taken) const {
        unsigned long long &w = bp[(size_t)d * nslot + (u >> 6)];
        const unsigned long long bit = 1ull << (u & 63);
        w = taken ? (w | bit) : (w & ~bit);
    }
};
}  // namespace

// B utterances of padded shape [T, U1].  nthr: lanes of the walk (1, or a multiple of 64 as on the device), run one
// after the other in reverse order inside a diagonal: the result may not depend on it.  alpha, beta, nll, tok_post:
// all NULL or all given.  The backpointer words start out as garbage, as device memory does.
extern "C" void rnnth_align(const float *lpb, const float *lpl, const long long *enc_len, const long long *txt_len, int B,
                            int T, int U1, int nthr, const float *alpha, const float *beta, const float *nll,
                            int *frames, int *labels_done, float *tok_logp, float *tok_post, float *score) {
    const int nslot = rnnt_align_nslot(U1);
    std::vector<float> diag(2 * (size_t)U1);
    std::vector<unsigned long long> bp((size_t)(T + U1 - 1) * nslot);
    for (int b = 0; b < B; ++b) {
        const int Tb = rnnt_clamp_T(enc_len[b], T), Ub = rnnt_clamp_U(txt_len[b], U1);
        const size_t off = (size_t)b * T * U1;
        for (auto &w : bp) w = 0xA5A5A5A5A5A5A5A5ull;
        const BitPut put{bp.data(), nslot};
        float sc = 0.f;
        if (nthr == 1) {
            rnnt_align_walk(0, 1, Tb, Ub, U1, lpb + off, lpl + off, diag.data(), &sc, NoSync(), put);
        } else {
            for (int d = 0; d < Tb + Ub; ++d)      // one diagonal at a time: what the barrier of the kernel enforces
                for (int tid = nthr - 1; tid >= 0; --tid)
                    rnnt_align_diag(d, tid, nthr, Tb, Ub, U1, lpb + off, lpl + off, diag.data(), &sc, put);
        }
        const bool ok = sc > -INFINITY;
        int *fr = frames + (size_t)b * (U1 - 1), *ld = labels_done + (size_t)b * T;
        if (ok) rnnt_align_backtrace(Tb, Ub, U1, bp.data(), fr, ld);
        for (int tid = nthr - 1; tid >= 0; --tid)
            rnnt_align_tokens(tid, nthr, ok, T, Tb, Ub, U1, lpb + off, lpl + off, alpha ? alpha + off : nullptr,
                              alpha ? beta + off : nullptr, alpha ? nll[b] : 0.f, fr, ld,
                              tok_logp + (size_t)b * (U1 - 1), alpha ? tok_post + (size_t)b * (U1 - 1) : nullptr);
        score[b] = sc;
    }
}

#ifdef RNNT_ALIGN_HOST_MAIN
int main() {
    const int shapes[][2] = {{1, 0}, {1, 1}, {1, 5}, {5, 0}, {2, 1}, {7, 3}, {3, 7}, {64, 63}, {65, 64}, {9, 300},
                             {130, 100}};
    unsigned seed = 12345;
    auto rnd = [&seed]() {
        seed = seed * 1664525u + 1013904223u;
        return (float)(seed >> 8) / (float)(1u << 24);
    };
    int bad = 0;
    for (const auto &s : shapes) {
        const int T = s[0], U = s[1], U1 = U + 1;
        const size_t n = (size_t)T * U1;
        // exactly sized heap buffers: an index outside them is a sanitizer report
        std::vector<float> lpb(n), lpl(n), tok_logp(U);
        std::vector<int> frames(U), done(T);
        for (size_t i = 0; i < n; ++i) {
            const float p = 0.05f + 0.9f * rnd();
            lpb[i] = std::log(p);
            lpl[i] = std::log((1.f - p) * (0.05f + 0.9f * rnd()));
        }
        for (int nthr : {1, 128}) {
            const long long el = T, tl = U;
            float score = 0.f;
            rnnth_align(lpb.data(), lpl.data(), &el, &tl, 1, T, U1, nthr, nullptr, nullptr, nullptr, frames.data(),
                        done.data(), tok_logp.data(), nullptr, &score);
            double sum = 0.0;
            int u = 0, ok = 1;
            for (int t = 0; t < T; ++t) {          // replay the path: labels emitted at frame t, then its blank
                while (u < U && frames[u] == t) sum += lpl[(size_t)t * U1 + u], ++u;
                if (done[t] != u) ok = 0;
                sum += lpb[(size_t)t * U1 + u];
            }
            if (u != U) ok = 0;
            if (!ok || !(std::fabs(sum - score) <= 1e-5 * (T + U) * (1.0 + std::fabs(sum)))) {
                std::printf("T %d U %d lanes %d: path %s, score %g, sum along the path %g\n", T, U, nthr,
                            ok ? "ok" : "broken", score, sum);
                ++bad;
            }
        }
    }
    std::printf("%d failures\n", bad);
    return bad ? 1 : 0;
}
#endif
