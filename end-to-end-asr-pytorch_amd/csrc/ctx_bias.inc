// Contextual biasing (phrase boosting): the automaton walk, shared by the gfx950 kernels (ctx_bias.hip) and any host
// build.  The includer defines CB_HD (`__device__` or nothing).  Plain C++: no HIP call, no float atomics.
//
// Image (src/bias.py: build_image): an Aho-Corasick automaton over the model's tokens, node 0 = the root.  phi [N] is
// the pending (not yet banked) bonus of a node; root_arrive / root_next [V] are the dense transitions of the root
// (arrive[goto(0, v)], goto(0, v)); per node n >= 1 a CSR list ext_off[n] .. ext_off[n + 1] of (ext_word ascending,
// ext_arrive, ext_next): the children of every node on n's fail chain except the root, merged by the builder so that
// the deepest node wins.  goto(s, v) is therefore one binary search plus one table read: no chain is followed here
// and no phrase length is limited.  The step's value is delta(s, v) = arrive[goto(s, v)] - phi[s], one f32 subtraction.
struct CBImage {
    int V, n_nodes, n_entries;
    const float *phi;
    const float *root_arrive;
    const int *root_next;
    const int *ext_off;
    const int *ext_word;
    const float *ext_arrive;
    const int *ext_next;
};

// the entry range of node s, clamped: a damaged image must not lead outside itself
CB_HD inline void cb_range(const CBImage &b, int s, int *lo, int *hi) {
    int l = b.ext_off[s], h = b.ext_off[s + 1];
    if (l < 0) l = 0;
    if (h > b.n_entries) h = b.n_entries;
    *lo = l;
    *hi = h;
}

// merged entry of node s for token `tok`, or -1
CB_HD inline int cb_find(const CBImage &b, int s, int tok) {
    int lo, hi;
    cb_range(b, s, &lo, &hi);
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        const int w = b.ext_word[mid];
        if (w == tok) return mid;
        if (w < tok) lo = mid + 1; else hi = mid;
    }
    return -1;
}

// goto(s, tok) and arrive[goto(s, tok)]; a token outside [0, V) leads to the root (arrive 0)
CB_HD inline int cb_goto(const CBImage &b, int s, long long tok, float *arrive) {
    *arrive = 0.0f;
    if (tok < 0 || tok >= b.V) return 0;
    if (s < 0 || s >= b.n_nodes) s = 0;
    int nxt;
    if (s != 0) {
        const int e = cb_find(b, s, (int)tok);
        if (e >= 0) {
            nxt = b.ext_next[e];
            if (nxt < 0 || nxt >= b.n_nodes) return 0;
            *arrive = b.ext_arrive[e];
            return nxt;
        }
    }
    nxt = b.root_next[tok];
    if (nxt < 0 || nxt >= b.n_nodes) return 0;
    *arrive = b.root_arrive[tok];
    return nxt;
}
