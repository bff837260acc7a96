// Back-off n-gram LM step: the state walk and the back-off chain, shared by the gfx950 kernel (ngram.hip) and the
// host build of the tests (tests/native/ngram_host.cpp).  The includer defines NG_HD (`__device__` or nothing).
// Plain C++: no HIP call, no float atomics, f32 adds in one fixed order.
//
// Image (src/ngram.py: build_image): node 0 is the empty context.  uni_logp / uni_next [V] are the dense unigram
// level (a word without a unigram: ln(10) * -99, next state 0); per node bo, fail (the context without its oldest
// token; fail[0] = 0, fail[s] < s) and the children child_off[s] .. child_off[s + 1]; per child word (ascending
// inside a node), logp and next (the state after consuming the word there, resolved by the builder).
#define NG_MAX_ORDER 8

struct NGImage {
    int order, V, n_nodes, n_entries;
    const float *uni_logp;
    const int *uni_next;
    const float *bo;
    const int *fail;
    const int *child_off;
    const int *word;
    const float *logp;
    const int *next;
};

// child entry of node s for token `tok`, or -1
NG_HD inline int ng_find(const NGImage &g, int s, int tok) {
    int lo = g.child_off[s], hi = g.child_off[s + 1];
    if (lo < 0) lo = 0;                                           // a damaged image must not lead outside itself
    if (hi > g.n_entries) hi = g.n_entries;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        const int w = g.word[mid];
        if (w == tok) return mid;
        if (w < tok) lo = mid + 1; else hi = mid;
    }
    return -1;
}

// the state after feeding `tok` in state s: the entry of the longest context that has one, else the unigram's;
// a token outside [0, V) (and, through uni_next, one without a unigram) leads to the empty context
NG_HD inline int ng_advance(const NGImage &g, int s, long long tok) {
    if (tok < 0 || tok >= g.V) return 0;
    if (s < 0 || s >= g.n_nodes) s = 0;
    for (int hop = 0; hop < NG_MAX_ORDER && s != 0; ++hop) {      // at most order - 1 contexts above node 0
        const int e = ng_find(g, s, (int)tok);
        if (e >= 0) return g.next[e];
        s = g.fail[s];
        if (s < 0 || s >= g.n_nodes) s = 0;
    }
    return g.uni_next[tok];
}

// the back-off chain of state s: c[0] = s, c[k] = fail[c[k - 1]], ..., c[d] = 0 and the running back-off sums
// B[0] = +0, B[k] = fl(B[k - 1] + bo[c[k - 1]]); returns d <= NG_MAX_ORDER - 1.  c and B hold NG_MAX_ORDER values.
NG_HD inline int ng_chain(const NGImage &g, int s, int *c, float *B) {
    if (s < 0 || s >= g.n_nodes) s = 0;
    int d = 0;
    c[0] = s;
    B[0] = 0.0f;
    while (c[d] != 0 && d < NG_MAX_ORDER - 1) {
        B[d + 1] = B[d] + g.bo[c[d]];
        c[d + 1] = g.fail[c[d]];
        if (c[d + 1] < 0 || c[d + 1] >= g.n_nodes) c[d + 1] = 0;
        ++d;
    }
    c[d] = 0;                                                     // a valid image ends here by itself
    return d;
}
