// Launch plans of the streaming helpers (rowops.hip: copy3d, colsum; norm.hip: dropout, the LayerNorm parameter
// gradient; optim.hip: the single-tensor Adadelta step).  Each entry point takes kernel, grid and chunking from the
// function below and from nowhere else; asrk_rowops_plan_info (rowops.hip) reports the same record, so a test can
// hold a shape to the kernel it is meant to reach.  Host only: pointers are looked at for alignment, never read.
#pragma once
#include "common.h"
#include "knobs.h"
#include <algorithm>

namespace rowops_plan {

inline bool al16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---- copy3d: variant bit 0 = accumulate; 0/1 generic scalar, 2/3 generic 16-byte, 4/5 wide-row kernel
struct Copy3dPlan {
    int variant;
    bool vec, rows_kernel;
    unsigned gx, gy;
    int rpb;          // rows kernel: rows per workgroup (0 otherwise)
    int rows, per_row;
    int64_t total;    // work items of the generic kernel: elements or 16-byte pieces
};

inline Copy3dPlan copy3d_plan(const void *src, const void *dst, int n0, int n1, int n2, int64_t ss0, int64_t ss1,
                              int64_t ds0, int64_t ds1, int accumulate) {
    Copy3dPlan pl{};
    pl.vec = al16(src) && al16(dst) && (n2 % 4 == 0) && (ss0 % 4 == 0) && (ss1 % 4 == 0) && (ds0 % 4 == 0) &&
             (ds1 % 4 == 0);
    pl.total = (int64_t)n0 * n1 * (pl.vec ? n2 / 4 : n2);
    int64_t g = asrk_div_up64(pl.total, 256);
    if (g > 256 * 16) g = 256 * 16;  // grid-stride beyond ~16 blocks/CU
    if (g < 1) g = 1;
    pl.gx = (unsigned)g;
    pl.gy = 1;
    const int64_t rows64 = (int64_t)n0 * n1;
    if (pl.vec && n2 / 4 >= 64 && rows64 < (1ll << 30)) {
        const int rows = (int)rows64, per_row = n2 / 4;
        const int gx = asrk_div_up(per_row, 256);
        int rpb = 16;                                   // rows per block: >= ~2k blocks when possible
        while (rpb > 4 && (int64_t)gx * asrk_div_up(rows, rpb) < 2048) rpb >>= 1;
        if (asrk_div_up(rows, rpb) > 65535) rpb = asrk_div_up(rows, 65535);
        if ((unsigned)asrk_div_up(rows, rpb) <= 65535u) {
            pl.rows_kernel = true;
            pl.gx = (unsigned)gx;
            pl.gy = (unsigned)asrk_div_up(rows, rpb);
            pl.rpb = rpb;
            pl.rows = rows;
            pl.per_row = per_row;
        }
    }
    pl.variant = (pl.rows_kernel ? 4 : pl.vec ? 2 : 0) + (accumulate ? 1 : 0);
    return pl;
}

// ---- colsum: variant 0 scalar, 1 16-byte columns, 2 narrow contiguous stream
struct ColsumPlan {
    int variant;
    unsigned gx, gy;
    int chunks;            // workgroups that add into one out[c]: row chunks (grid y), or the narrow kernel's blocks
    int rpc;               // rows per chunk (scalar / vector kernel)
    int64_t per_block;     // narrow kernel: 16-byte pieces per block (a multiple of 2048)
    int64_t total4;
};

inline ColsumPlan colsum_plan(const void *X, int M, int N, int ldx) {
    ColsumPlan pl{};
    const bool det = asrk_knobs_().get(asrk_knobs_().deterministic, 0) != 0;
    const bool vec = al16(X) && (N % 4 == 0) && (ldx % 4 == 0);
    if (vec && ldx == N && N <= 128 && 256 % (N / 4) == 0 && M >= 4096) {
        pl.variant = 2;
        pl.total4 = (int64_t)M * (N / 4);
        // out[c] takes one atomic per block: 2048 blocks on 64 addresses took longer than the 131-MB read itself
        const int blocks = det ? 1 : 512;
        pl.per_block = asrk_div_up64(asrk_div_up64(pl.total4, blocks), 2048) * 2048;
        pl.chunks = (int)asrk_div_up64(pl.total4, pl.per_block);
        pl.gx = (unsigned)pl.chunks;
        pl.gy = 1;
        return pl;
    }
    pl.variant = vec ? 1 : 0;
    const int gx = asrk_div_up(N, vec ? 256 : 64);
    int chunks = asrk_div_up(vec ? 2048 : 1024, gx);
    if (chunks > asrk_div_up(M, 32)) chunks = asrk_div_up(M, 32);
    // deterministic: ONE row chunk per column block - the block's fixed-order sum is the only value added to out[c]
    if (chunks < 1 || det) chunks = 1;
    pl.rpc = asrk_div_up(M, chunks);
    pl.chunks = asrk_div_up(M, pl.rpc);
    pl.gx = (unsigned)gx;
    pl.gy = (unsigned)pl.chunks;
    return pl;
}

// ---- dropout: variant 0 scalar, 1 16-byte
struct DropoutPlan {
    int variant;
    unsigned grid;
    int64_t nq;            // Philox counters = quads of elements
};

inline DropoutPlan dropout_plan(const void *x, const void *y, int64_t n) {
    DropoutPlan pl{};
    pl.variant = (al16(x) && al16(y) && (n % 4 == 0)) ? 1 : 0;
    pl.nq = (n + 3) / 4;
    pl.grid = (unsigned)std::min<int64_t>(8192, asrk_div_up64(pl.nq, 256));
    return pl;
}

// ---- single-tensor Adadelta step: variant 0 scalar, 1 16-byte
struct AdadeltaPlan {
    int variant;
    unsigned grid;
    int64_t items;         // elements, or 16-byte pieces
};

inline unsigned optim_grid_for(int64_t n) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(asrk_div_up64(n, 256), 4096));
}

inline AdadeltaPlan adadelta_plan(const void *param, const void *grad, const void *sq, const void *acc, int64_t n) {
    AdadeltaPlan pl{};
    pl.variant = (al16(param) && al16(grad) && al16(sq) && al16(acc) && (n % 4 == 0)) ? 1 : 0;
    pl.items = pl.variant ? n / 4 : n;
    pl.grid = optim_grid_for(pl.items);
    return pl;
}

// ---- LayerNorm parameter gradient: row chunks whose sums meet in float atomics
struct LnParamPlan {
    unsigned gx, gy;
    int rpc;               // rows per chunk, a multiple of 4
};

inline LnParamPlan ln_param_plan(int rows, int cols) {
    LnParamPlan pl{};
    // ASRK_DETERMINISTIC: one row chunk - a column's fixed-order block sum is the only value added to dw / db
    const int chunks = asrk_knobs_().get(asrk_knobs_().deterministic, 0)
                           ? 1 : std::max(1, std::min(asrk_div_up(rows, 64), 256));
    pl.rpc = asrk_div_up(asrk_div_up(rows, chunks), 4) * 4;
    pl.gx = (unsigned)asrk_div_up(cols, 64);
    pl.gy = (unsigned)asrk_div_up(rows, pl.rpc);
    return pl;
}

}  // namespace rowops_plan
