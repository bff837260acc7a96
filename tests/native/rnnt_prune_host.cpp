// TEST INFRASTRUCTURE ONLY: the pruning rule of pruned transducer training
// (end-to-end-asr-pytorch_amd/csrc/rnnt_prune.inc, the very source the gfx950 kernel is built from) compiled for the
// host, so that tests/test_rnnt_prune_cpu.py can check it against the numpy mirror without a GPU.
// The product never links or calls this file.  Built by the test with g++ -O2 -ffp-contract=off.
//
// With -DRNNT_PRUNE_HOST_MAIN it is a stand-alone program for a sanitizer build (g++ -fsanitize=address,undefined): it
// runs the rule on generated occupations with exactly sized buffers and checks the four invariants of the result.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define RNNT_HD
#include "../../end-to-end-asr-pytorch_amd/csrc/rnnt.inc"
#include "../../end-to-end-asr-pytorch_amd/csrc/rnnt_prune.inc"

// occ [B, T, U1] -> s [B, T].  nthr = 1: one thread per utterance (rnntp_ranges_one); otherwise the kernel's split of
// the band starts of a frame over nthr lanes, the lanes' candidates merged in reverse order (the result may not depend
// on the order).
extern "C" void rnntph_ranges(const float *occ, const long long *enc_len, const long long *txt_len, int B, int T, int U1,
                              int S, int nthr, int *s_out) {
    for (int b = 0; b < B; ++b) {
        const int Tb = rnnt_clamp_T(enc_len[b], T), Ub = rnnt_clamp_U(txt_len[b], U1);
        const float *ob = occ + (size_t)b * T * U1;
        int *sb = s_out + (size_t)b * T;
        if (nthr == 1) {
            rnntp_ranges_one(ob, T, U1, Tb, Ub, S, sb);
            continue;
        }
        const int E = rnntp_last_start(Ub, S);
        int sp = 0, last = 0;
        for (int t = 0; t < T; ++t) {
            if (t < Tb) {
                float best = -INFINITY;
                int arg = -1;
                for (int lane = nthr - 1; lane >= 0; --lane) {
                    float lb = -INFINITY;
                    int la = -1;
                    for (int s = lane; s <= E; s += nthr) rnntp_better(rnntp_window(ob + (size_t)t * U1, s, S, Ub), s, &lb, &la);
                    if (la >= 0) rnntp_better(lb, la, &best, &arg);
                }
                last = rnntp_step(arg < 0 ? 0 : arg, &sp, t, Tb, Ub, S);
            }
            sb[t] = last;
        }
    }
}

extern "C" int rnntph_feasible(int Tb, int Ub, int S) { return rnntp_feasible(Tb, Ub, S) ? 1 : 0; }

#ifdef RNNT_PRUNE_HOST_MAIN
int main() {
    unsigned seed = 2022;
    auto rnd = [&seed]() {
        seed = seed * 1664525u + 1013904223u;
        return (float)(seed >> 8) / (float)(1u << 24);
    };
    int bad = 0;
    for (int it = 0; it < 400; ++it) {
        const int T = 1 + (int)(rnd() * 12), U1 = 1 + (int)(rnd() * 40), S = 2 + (int)(rnd() * 6);
        const long long Tb = 1 + (long long)(rnd() * T), Ub = (long long)(rnd() * U1);
        // exactly sized heap buffers: an index outside them is a sanitizer report
        std::vector<float> occ((size_t)T * U1);
        for (auto &v : occ) v = rnd();
        for (int nthr : {1, 64}) {
            std::vector<int> s(T, -7);
            rnntph_ranges(occ.data(), &Tb, &Ub, 1, T, U1, S, nthr, s.data());
            const int tb = rnnt_clamp_T(Tb, T), ub = rnnt_clamp_U(Ub, U1), E = rnntp_last_start(ub, S);
            bool ok = s[tb - 1] == E && ((s[0] == 0) == rnntp_feasible(tb, ub, S));
            for (int t = 1; t < tb; ++t) ok = ok && s[t] >= s[t - 1] && s[t] - s[t - 1] <= S - 1;
            for (int t = tb; t < T; ++t) ok = ok && s[t] == s[tb - 1];
            if (!ok) {
                std::printf("T %d U1 %d S %d Tb %lld Ub %lld nthr %d: invariant broken\n", T, U1, S, Tb, Ub, nthr);
                ++bad;
            }
        }
    }
    std::printf("%d failures\n", bad);
    return bad ? 1 : 0;
}
#endif
