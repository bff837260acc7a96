// TEST INFRASTRUCTURE ONLY: the state walk and back-off chain of the n-gram LM step
// (end-to-end-asr-pytorch_amd/csrc/ngram.inc, the very source the gfx950 kernel is built from) compiled for the host,
// so that tests/test_ngram_cpu.py can check them against the numpy restatement without a GPU.
// The product never links or calls this file.  Built by the test with g++ -O2 -ffp-contract=off.
//
// With -DNGRAM_HOST_MAIN it is a stand-alone program for a sanitizer build (g++ -fsanitize=address,undefined):
//   ngram_host FILE     FILE = what `python tests/test_ngram_cpu.py --dump FILE` writes (image, walks, expected)
// It runs every walk and compares states, depths, chains and sums with the expected ones bit for bit.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#define NG_HD
#include "../../end-to-end-asr-pytorch_amd/csrc/ngram.inc"

// n walks: state_out[i] = advance(state_in[i], token[i]); depth[i], chain[i][8] and sums[i][8] of the new state
extern "C" void ngh_walk(int order, int V, int n_nodes, int n_entries, const float *uni_logp, const int *uni_next,
                         const float *bo, const int *fail, const int *child_off, const int *word, const float *logp,
                         const int *next, int n, const int *state_in, const long long *token, int *state_out,
                         int *depth, int *chain, float *sums) {
    const NGImage g{order, V, n_nodes, n_entries, uni_logp, uni_next, bo, fail, child_off, word, logp, next};
    for (int i = 0; i < n; ++i) {
        int c[NG_MAX_ORDER] = {0};
        float B[NG_MAX_ORDER] = {0.0f};
        state_out[i] = ng_advance(g, state_in[i], token[i]);
        depth[i] = ng_chain(g, state_out[i], c, B);
        std::memcpy(chain + (size_t)i * NG_MAX_ORDER, c, sizeof(c));
        std::memcpy(sums + (size_t)i * NG_MAX_ORDER, B, sizeof(B));
    }
}

#ifdef NGRAM_HOST_MAIN
namespace {
bool read(FILE *f, void *p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; }
}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s FILE\n", argv[0]); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    int hdr[5];                                            // order, V, n_nodes, n_entries, n walks
    if (!read(f, hdr, sizeof(hdr))) return 2;
    const int order = hdr[0], V = hdr[1], N = hdr[2], E = hdr[3], n = hdr[4];
    if (V <= 0 || N <= 0 || E < 0 || n < 0) return 2;
    std::vector<float> uni_logp(V), bo(N), logp(E), sums((size_t)n * NG_MAX_ORDER), want_sums(sums.size());
    std::vector<int> uni_next(V), fail(N), child_off(N + 1), word(E), next(E), state_in(n), state_out(n), depth(n),
        chain((size_t)n * NG_MAX_ORDER), want_state(n), want_depth(n), want_chain(chain.size());
    std::vector<long long> token(n);
    bool ok = read(f, uni_logp.data(), 4u * V) && read(f, uni_next.data(), 4u * V) && read(f, bo.data(), 4u * N) &&
              read(f, fail.data(), 4u * N) && read(f, child_off.data(), 4u * (N + 1)) && read(f, word.data(), 4u * E) &&
              read(f, logp.data(), 4u * E) && read(f, next.data(), 4u * E) && read(f, state_in.data(), 4u * n) &&
              read(f, token.data(), 8u * n) && read(f, want_state.data(), 4u * n) && read(f, want_depth.data(), 4u * n) &&
              read(f, want_chain.data(), 4u * chain.size()) && read(f, want_sums.data(), 4u * sums.size());
    std::fclose(f);
    if (!ok) { std::fprintf(stderr, "short file\n"); return 2; }
    ngh_walk(order, V, N, E, uni_logp.data(), uni_next.data(), bo.data(), fail.data(), child_off.data(), word.data(),
             logp.data(), next.data(), n, state_in.data(), token.data(), state_out.data(), depth.data(), chain.data(),
             sums.data());
    int bad = 0;
    for (int i = 0; i < n; ++i) {
        bool same = state_out[i] == want_state[i] && depth[i] == want_depth[i];
        for (int k = 0; same && k <= depth[i]; ++k)
            same = chain[(size_t)i * NG_MAX_ORDER + k] == want_chain[(size_t)i * NG_MAX_ORDER + k] &&
                   std::memcmp(&sums[(size_t)i * NG_MAX_ORDER + k], &want_sums[(size_t)i * NG_MAX_ORDER + k], 4) == 0;
        bad += !same;
    }
    std::printf("%d walks, %d differ\n", n, bad);
    return bad ? 1 : 0;
}
#endif
