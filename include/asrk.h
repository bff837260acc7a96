/*
 * asrk.h — C ABI of libasrk.so: the MI355X (gfx950 / CDNA4) kernels underneath the
 * LAS/CTC training + decode hot path of Alexander-H-Liu/End-to-end-ASR-Pytorch.
 *
 * The reference has NO FFI of its own (pure Python over torch/ATen); each entry
 * point below therefore cites the reference call site (file:line under /root/reference) whose
 * third-party arithmetic it replaces.  INTEGRATION.md shows the ctypes binding a maintainer adds.
 *
 * Conventions
 *  - plain C, raw device pointers, explicit sizes/strides in ELEMENTS (floats) unless stated;
 *  - `stream` is a hipStream_t passed as void*; every call only ENQUEUES work (no device sync);
 *  - the library never allocates/frees device memory: outputs + workspaces are caller-owned
 *    (every entry point that needs scratch has a *_bytes query next to it);
 *  - no mutable mode state: arithmetic / launch variants are `flags` ARGUMENTS of the calls they affect;
 *    the ASRK_* tuning environment variables are read ONCE, at the first asrk_init();
 *    the only process-wide state is the cached device query and the optional profiling hooks below;
 *  - return 0 on success, negative ASRK_E* for argument errors, positive = hipError_t;
 *  - no C++ exceptions cross the boundary, no abort().
 */
#ifndef ASRK_H
#define ASRK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ASRK_OK 0
#define ASRK_EINVAL (-1)   /* bad argument (null pointer, negative size, unsupported combo) */
#define ASRK_ESHAPE (-2)   /* shape not supported by the persistent kernels (see message)   */
#define ASRK_EWORKSPACE (-3) /* workspace too small                                          */
#define ASRK_EDEVICE (-4)  /* device lacks the CUs/LDS the persistent kernel needs            */
#define ASRK_ETIMEOUT (-5) /* in-kernel grid sync gave up (reported by asrk_lstm_check_error) */

int asrk_version(void);
const char *asrk_strerror(int rc);
/* Query + cache device properties (CU count, LDS/CU). Call once per device before persistent
 * kernels; returns the CU count (>0) or a negative error. */
int asrk_init(int device);

/* ---- optional per-kernel hipEvent timing (bench.py roofline) --------------------------- */
void asrk_profile_enable(int on);
/* Families (bit id = ASRK_PROF_* id) that record events while profiling is on; default all.  An event pair costs ~3 us of
 * stream time (a marker packet waits for the kernel in front of it), so a timed region that only needs the dominant
 * kernel's durations enables that family alone. */
void asrk_profile_families(unsigned mask);
void asrk_profile_reset(void);
/* Resolves pending events (synchronises them) and returns total ms + launch count for a
 * kernel family id (see ASRK_PROF_*). */
int asrk_profile_get(int id, double *total_ms, int64_t *launches);
/* Algorithmic work the family was asked to do while profiling was on: flops for the GEMM families (2*M*N*K per
 * call), HBM bytes for the streaming families (CTC: dense gradient read + write; SPLIT: 4 B read + 6 B written per
 * element; OPTIM: 28 B per parameter for the update + 4 B per gradient element for the norm). */
int asrk_profile_get_work(int id, double *flops);
#define ASRK_PROF_GEMM 0
#define ASRK_PROF_LSTM_FWD 1
#define ASRK_PROF_LSTM_BWD 2
#define ASRK_PROF_CTC 3
#define ASRK_PROF_ROWOPS 4
#define ASRK_PROF_ATTN 5
#define ASRK_PROF_CELL 6
#define ASRK_PROF_FBANK 7
#define ASRK_PROF_GEMM_BG 8 /* asrk_gemm_f32 calls whose flags carry ASRK_GEMM_LDS_HINT(> 80) */
#define ASRK_PROF_SPELLER 9 /* asrk_speller_* (one event pair per call; launches = kernels enqueued) */
#define ASRK_PROF_CONV 10   /* prenet convolutions: im2col / col2im / ReLU / max-pool (their GEMMs count as GEMM) */
#define ASRK_PROF_SPLIT 11  /* split passes of the bf16x6 GEMM path (their time is ALSO inside ASRK_PROF_GEMM) */
#define ASRK_PROF_OPTIM 12  /* fused optimiser steps and gradient-norm passes */

/* ---- dense f32 GEMM on v_mfma_f32_32x32x2_f32 (exact f32) ------------------------------
 * C[M,N] = alpha * op(A) * op(B) + beta * C + bias[n] + bias2[n]     (row-major, ld in floats)
 *   transA=0: A stored [M,K] (lda>=K);  transA=1: A stored [K,M] (lda>=M)
 *   transB=0: B stored [K,N] (ldb>=N);  transB=1: B stored [N,K] (ldb>=K)
 * Supported: NT (0,1), NN (0,0), TN (1,0).  bias/bias2 may be NULL.
 * splitk<=0 -> heuristic; splitk>1 accumulates partials with f32 atomics (beta must be 0 or 1).
 * Replaces: torch Linear / the LSTM input projection inside nn.LSTM (src/module.py:131,
 * src/asr.py:96,220,280,290) and their autograd GEMMs. */
int asrk_gemm_f32(int transA, int transB, int M, int N, int K, float alpha,
                  const float *A, int lda, const float *B, int ldb, float beta,
                  float *C, int ldc, const float *bias, const float *bias2, int splitk,
                  int flags, void *ws, size_t ws_bytes, void *stream);

/* `flags` of asrk_gemm_f32 / asrk_gemm_ws_bytes / asrk_gemm_takes_split (per CALL - the library keeps no
 * mode state):
 *  bits 0-1  arithmetic of large contractions.  They run on the bf16 matrix cores by EXACT operand splitting
 *            (csrc/gemm_split.hip): every f32 operand is the exact sum of three bf16 numbers; the six partial
 *            products down to 2^-24 of the full product are accumulated in f32 (the three dropped ones are each
 *            below one f32 rounding of the product), so the result has f32-GEMM accuracy (checked against
 *            float64 in the tests) at 6/16 of the f32-MFMA cost.
 *              ASRK_GEMM_SPLIT_AUTO   when it pays (both output extents and K large) - the default (0)
 *              ASRK_GEMM_SPLIT_OFF    never: always v_mfma_f32_32x32x2_f32
 *              ASRK_GEMM_SPLIT_ALWAYS whenever the shape allows (K >= 8)
 *  bits 8-15 ASRK_GEMM_LDS_HINT(kib): request at least `kib` KiB of LDS per workgroup of the f32 tiled kernel
 *            (> 80 = one workgroup per CU instead of two), for GEMMs launched in the background of
 *            latency-critical kernels on another stream; 0 = no hint.
 * Workspace: a call that takes the split path writes the bf16 panels of both operands into `ws`
 * (caller-owned device memory, 16-byte aligned, at least asrk_gemm_ws_bytes(M, N, K, flags) bytes, private to
 * the call until the stream has passed it); other calls ignore ws (NULL / 0 allowed).  ASRK_EWORKSPACE if
 * it is missing or too small.  Replaces nothing in the reference by itself: it is the arithmetic behind the
 * same ATen GEMMs (src/module.py:131, src/asr.py:96,220 and their autograd contractions). */
#define ASRK_GEMM_SPLIT_AUTO 0
#define ASRK_GEMM_SPLIT_OFF 1
#define ASRK_GEMM_SPLIT_ALWAYS 2
#define ASRK_GEMM_LDS_HINT(kib) (((kib) & 0xff) << 8)
size_t asrk_gemm_ws_bytes(int M, int N, int K, int flags);
/* 1 if asrk_gemm_f32 runs an M x N x K contraction on the split path under `flags` */
int asrk_gemm_takes_split(int M, int N, int K, int flags);

/* Which kernel asrk_gemm_f32 runs for these arguments, from the very planner the launch uses (knobs included).
 * `align`: bit 0 = A is 16-byte aligned, bit 1 = B is (the query takes no pointers).  Host only when ncu > 0: plan
 * for a device of `ncu` compute units, no device call; ncu == 0: the current device's count (256 without one, as
 * the launch assumes).  Returns what the launch would for the same arguments: ASRK_EINVAL for a negative size or
 * flags, TT, a leading dimension below the extent (and for NULL info / ncu < 0); M == 0 or N == 0 is ASRK_OK with
 * launches = 0.
 * info[ASRK_GEMM_PLAN_INFO_LEN]:
 *   [0] path: 0 skinny NT, 1 skinny NN, 2 bf16x6 split, 3 fast tiled, 4 generic tiled
 *   [1] a_kc, [2] b_kc (operand stored K-contiguous)   [3] vec (16-byte global loads)
 *   [4] K ranges (splitk after clamping)   [5] k per range   [6..8] grid x / y / z (0 on the split path)
 *   [9] pre-pass establishing beta*C: 0 none, 1 memset, 2 scale_rows
 *   [10] store form of the epilogue: 0 overwrite, 1 read-modify-write with beta, 2 +=, 3 atomics
 *   [11] dynamic LDS bytes   [12] launches: the kernel, the pre-pass, on the split path the two split passes and the
 *        panel GEMM (3; its optional 128x128 tail launch is not counted)   [13] the CU count used */
#define ASRK_GEMM_PLAN_INFO_LEN 16
int asrk_gemm_plan_info(int transA, int transB, int M, int N, int K, int lda, int ldb, int ldc, int align,
                        float beta, int splitk, int flags, int ncu, int *info);

/* Split panels as operands of their own: split an operand ONCE, multiply it several times (the weight
 * gradients dW_ih = dG^T X and dW_hh = dG^T H_prev of an LSTM layer share dG^T; autograd of nn.LSTM,
 * src/module.py:131).  A panel holds the three bf16 planes of a logical [rows][K] operand (K = contraction
 * index); `trans` != 0: src is stored [K][rows] (ld >= rows), else [rows][K] (ld >= K).  The buffer is the
 * caller's (asrk_split_panel_bytes bytes, 16-byte aligned).
 * asrk_gemm_panels_f32: C[M,N] = alpha * A[a_row0 .. a_row0+M, a_k0 .. a_k0+K] * B[b_row0 .. b_row0+N,
 * b_k0 .. b_k0+K]^T + beta * C + bias + bias2 with A, B given as panels of the stated full extents
 * (a_rows x a_K, b_rows x b_K).  Row offsets must be multiples of 128, k offsets multiples of 8; K must be a
 * multiple of 32 unless the range ends at the end of one of the panels (ASRK_ESHAPE otherwise).  `flags`: reserved,
 * must be 0. */
size_t asrk_split_panel_bytes(int rows, int K, int flags);
int asrk_split_panel_f32(const float *src, int ld, int rows, int K, int trans, void *panel, int flags, void *stream);
int asrk_gemm_panels_f32(int M, int N, int K, float alpha, const void *A_panel, int a_rows, int a_K,
                         int a_row0, int a_k0, const void *B_panel, int b_rows, int b_K, int b_row0, int b_k0,
                         float beta, float *C, int ldc, const float *bias, const float *bias2, int flags,
                         void *stream);
/* The same product with a fixed-order split-K, for outputs of few 128 x 128 tiles under a deep K (dW_ih = dG^T X of an
 * LSTM layer with a narrow input, 8H x 80 x tokens: autograd of src/module.py:131; ops.py: LSTMLayerFn.backward,
 * ops.gemm_panels(splitk=...)).  The k-tiles (32 k) are cut into `splitk` contiguous slices (more slices than k-tiles:
 * clamped), each slice's raw accumulators go to ws[slice][M][round_up(N, 4)] and a second kernel adds the slices in index
 * order and applies alpha, beta and the biases: bit-reproducible, no atomics.  splitk = 1 is asrk_gemm_panels_f32's
 * launch; splitk = 0 lets the library choose (the smallest count with a workgroup per CU while a slice keeps >= 64
 * k-tiles; 1 for N >= 512).  ws: caller-owned device memory, 16-byte aligned (ASRK_EINVAL if NULL or misaligned), at
 * least asrk_gemm_panels_splitk_ws_bytes(M, N, splitk) bytes (ASRK_EWORKSPACE otherwise; for splitk = 0 that is the
 * bound over every K).  ASRK_EINVAL for splitk < 0. */
size_t asrk_gemm_panels_splitk_ws_bytes(int M, int N, int splitk);
int asrk_gemm_panels_splitk_f32(int M, int N, int K, float alpha, const void *A_panel, int a_rows, int a_K,
                                int a_row0, int a_k0, const void *B_panel, int b_rows, int b_K, int b_row0, int b_k0,
                                float beta, float *C, int ldc, const float *bias, const float *bias2, int splitk,
                                void *ws, size_t ws_bytes, int flags, void *stream);

/* ---- strided 3-D copy: dst[i0][i1][0:n2] = src[i0][i1][0:n2] (strides in floats) ------
 * Used for [B,T,D]<->[T,B,D] and the pyramid 'concat'/'drop' time reduction
 * (src/module.py:141-153). accumulate!=0 -> dst += src. */
int asrk_copy3d_f32(const float *src, float *dst, int n0, int n1, int n2,
                    int64_t s_stride0, int64_t s_stride1, int64_t d_stride0, int64_t d_stride1,
                    int accumulate, void *stream);

/* out[n] (+)= sum_m X[m, n]   (X row-major [M,N], ldx floats); bias gradients. */
int asrk_colsum_f32(const float *X, int M, int N, int ldx, float *out, int accumulate,
                    void *stream);

/* What asrk_copy3d_f32, asrk_colsum_f32, asrk_dropout_f32, asrk_adadelta_step_f32 and the parameter-gradient launch of
 * asrk_layer_norm_bwd_f32 would launch for their arguments, from the plan functions the entries themselves call
 * (csrc/rowops_plan.h); host only, no device call, runs without a GPU.  Pointers are looked at for their alignment and
 * never read.  ptrs / args per op:
 *   COPY3D    ptrs {src, dst}                      args {n0, n1, n2, s_stride0, s_stride1, d_stride0, d_stride1, accumulate}
 *   COLSUM    ptrs {X, out}                        args {M, N, ldx, accumulate}
 *   DROPOUT   ptrs {x, y}                          args {n}
 *   ADADELTA  ptrs {param, grad, square_avg, acc}  args {n}
 *   LN_PARAM  ptrs unused (may be NULL)            args {rows, cols}
 * ASRK_EINVAL: info == NULL, n < ASRK_ROWOPS_PLAN_INFO_LEN, an unknown op, and whatever the entry itself refuses (a
 * negative size, ldx < N, a NULL pointer it would read); info[0..n) is zeroed first whenever info and n are valid.
 * Otherwise ASRK_OK and
 *   [0] variant.  copy3d: 0 / 1 generic kernel, 4-byte lanes, copy / accumulate; 2 / 3 generic kernel, 16-byte lanes;
 *       4 / 5 wide-row kernel (16-byte lanes, rows of >= 64 of them).  colsum: 0 scalar, 1 16-byte columns, 2 narrow
 *       contiguous stream (ldx == N in {4, 8, 16, 32, 64, 128}, M >= 4096).  dropout, adadelta: 0 scalar, 1 16-byte.
 *   [1] kernel launches (0: an empty problem; every other field but [7] is 0 then)
 *   [2], [3] grid x, y
 *   [4] copy3d wide-row kernel: rows per workgroup; colsum: rows per chunk (narrow: 16-byte pieces per workgroup, a
 *       multiple of 2048); LN_PARAM: rows per chunk, a multiple of 4
 *   [5] colsum, LN_PARAM: the workgroups whose sums meet in one output element (1 under ASRK_DETERMINISTIC)
 *   [6] work items: copy3d elements or 16-byte pieces (generic kernel), colsum narrow 16-byte pieces, dropout quads,
 *       adadelta elements or 16-byte pieces
 *   [7] colsum: 1 = out is zeroed first (accumulate == 0) */
#define ASRK_ROWOPS_PLAN_INFO_LEN 8
#define ASRK_ROWOPS_PLAN_COPY3D 0
#define ASRK_ROWOPS_PLAN_COLSUM 1
#define ASRK_ROWOPS_PLAN_DROPOUT 2
#define ASRK_ROWOPS_PLAN_ADADELTA 3
#define ASRK_ROWOPS_PLAN_LN_PARAM 4
int asrk_rowops_plan_info(int op, const void *const *ptrs, const int64_t *args, int64_t *info, int n);

/* elementwise helpers (activation epilogues that are not fused into a GEMM) */
int asrk_tanh_fwd_f32(const float *x, float *y, int64_t n, void *stream);
/* dx = dy * (1 - y^2) */
int asrk_tanh_bwd_f32(const float *y, const float *dy, float *dx, int64_t n, void *stream);

/* ---- row log-softmax (src/asr.py:96, src/decode.py:93,121) -----------------------------
 * y[r,:] = x[r,:] - logsumexp(x[r,:]); in-place allowed (y==x). */
int asrk_log_softmax_fwd_f32(const float *x, float *y, int rows, int cols, int ld,
                             void *stream);
/* dx[r,:] = dy[r,:] - exp(y[r,:]) * sum(dy[r,:]); in-place allowed (dx==dy). */
int asrk_log_softmax_bwd_f32(const float *y, const float *dy, float *dx, int rows, int cols,
                             int ld, void *stream);

/* ---- row top-k / arg-max (src/asr.py:136-142 greedy feedback, src/decode.py:124,150 beam
 * pruning, bin/test_asr.py:118-120): values [rows,k] descending, indices [rows,k] int64; ties
 * resolve to the smaller index (k = 1 is the first arg-max).  NaNs are never selected. */
int asrk_topk_f32(const float *x, int rows, int cols, int ld, int k, float *values,
                  int64_t *indices, void *stream);

/* ---- validation read-out (bin/train_asr.py:169-217 -> src/util.py:113-127 cal_er) -------------------------
 * token_crop: the rule every reference text encoder's decode() applies to a row of (arg-max) token ids
 * (src/text.py:61-71): stop at the first eos_idx, drop pad_idx, and with ignore_repeat != 0 drop an id equal
 * to the RAW previous element (CTC repeat merging).  ids [B, ld] int64 (T used per row) -> out [B, ld_out]
 * compacted in place order, out_len [B] int32.  One wave per row.
 * edit_distance: unit-cost Levenshtein distance of B independent pairs of int64 symbol sequences
 * (a [B, lda] with a_len, b [B, ldb] with b_len <= max_b_len <= 4096) -> dist [B] int32; replaces
 * editdistance.eval at src/util.py:126 (third-party, absent: the classic dynamic programme).  Symbols are
 * whatever the caller interned (token ids for token-level rates, word ids for WER). */
int asrk_token_crop_i64(const int64_t *ids, int64_t ld, int B, int T, int64_t pad_idx, int64_t eos_idx,
                        int ignore_repeat, int64_t *out, int64_t ld_out, int32_t *out_len, void *stream);
int asrk_edit_distance_i64(const int64_t *a, int64_t lda, const int32_t *a_len, const int64_t *b, int64_t ldb,
                           const int32_t *b_len, int B, int max_b_len, int32_t *dist, void *stream);

/* ---- fused softmax cross-entropy (bin/train_asr.py:47,130-131: CrossEntropyLoss(ignore_index=0))
 * fwd: row_lse[r] = logsumexp(logits[r,:]); sums[0] = sum over counted rows of (lse - logit[tgt]),
 *      sums[1] = number of counted rows (targets != ignore_index).  mean loss = sums[0]/sums[1].
 * bwd: dlogits[r,:] = (softmax(logits[r,:]) - onehot(tgt[r])) * gscale[0]  (0 for ignored rows);
 *      gscale is a DEVICE scalar (grad_out / count) so no host sync is needed. */
int asrk_cross_entropy_fwd_f32(const float *logits, int rows, int V, int ld,
                               const int64_t *targets, int ignore_index, float *row_lse,
                               float *sums, void *stream);
int asrk_cross_entropy_bwd_f32(const float *logits, int rows, int V, int ld,
                               const int64_t *targets, int ignore_index, const float *row_lse,
                               const float *gscale, float *dlogits, void *stream);

/* ---- label-smoothed cross entropy: torch.nn.functional.cross_entropy(ignore_index, label_smoothing=eps), uniform
 * smoothing, no class weights.  Per counted row (tgt != ignore_index and 0 <= tgt < V), lse = logsumexp(logits[r,:]):
 *     loss_r = (1 - eps) * (lse - logit[tgt]) + eps * (lse - mean(logits[r,:]))
 * fwd reads the logits as often as asrk_cross_entropy_fwd_f32 and does not take eps: sums[0] and sums[1] as above,
 *      sums[2] = sum over counted rows of (lse - mean); mean loss = ((1-eps)*sums[0] + eps*sums[2]) / sums[1].
 *      row_lse[r] and row_smooth[r] = lse - mean are written for every row (row_smooth is what the fixed-order
 *      reduction under ASRK_DETERMINISTIC=1 adds up).
 * bwd: dlogits[r,:] = (softmax(logits[r,:]) - (1-eps)*onehot(tgt[r]) - eps/V) * gscale[0], exactly 0 for ignored rows;
 *      gscale is a device scalar.  ASRK_EINVAL for label_smoothing outside [0, 1) (NaN included).
 * Both: ASRK_EINVAL for a NULL pointer, checked before any device call. */
int asrk_cross_entropy_ls_fwd_f32(const float *logits, int rows, int V, int ld, const int64_t *targets,
                                  int ignore_index, float *row_lse, float *row_smooth, float *sums, void *stream);
int asrk_cross_entropy_ls_bwd_f32(const float *logits, int rows, int V, int ld, const int64_t *targets,
                                  int ignore_index, float label_smoothing, const float *row_lse, const float *gscale,
                                  float *dlogits, void *stream);

/* ---- bidirectional LSTM recurrence, persistent kernels (src/module.py:131 -> ATen lstm) ----
 * Time-major layout.  G: [T*B, ldg] with ldg = ndir*4H, column = dir*4H + gate*H + unit
 * (gate order i,f,g,o as torch).  On entry G holds X*W_ih^T + b_ih + b_hh; on exit the
 * ACTIVATED gates (saved for backward).  Y,C: [T*B, ndir*H] hidden / cell states.
 * whh_f/whh_r: [4H,H] torch layout (whh_r ignored when ndir==1).  Zero initial state
 * (module.py:131 passes none).  ws: asrk_lstm_ws_bytes() bytes of device scratch
 * (error word). */
size_t asrk_lstm_ws_bytes(void);
/* `flags` of every recurrence entry point and of the two plan queries below (the queries must be asked with
 * the flags of the launch they size): ASRK_REC_F32_MFMA = form the recurrent products with
 * v_mfma_f32_16x16x4_f32 instead of the exact bf16x6 operand split (wide layers, H = 512 / 1024, use the
 * split by default; results agree to f32 rounding).  0 = default. */
#define ASRK_REC_F32_MFMA 1
/* ASRK_REC_REARM: the launch hands `xchg` back ARMED - every byte 0xFF again once the stream gets past this call -
 * so the NEXT launch of the same shape and flags on this buffer may pass xchg_prefilled = 1 and no fill pass ever
 * runs in front of a recurrence (the workgroups refill the region of step s - 2 while they compute step s; a small
 * fill behind the kernel covers the last two steps).  A launch that ends in ASRK_ETIMEOUT (asrk_lstm_check_error)
 * leaves the buffer in an undefined state: fill or drop it. */
#define ASRK_REC_REARM 2
/* ASRK_REC_BWD_NO_DG (asrk_lstm_rec_bwd_pyr_panel_f32 only; every other entry point ignores it): the BPTT kernel does
 * NOT store the f32 dG over `gates` - the caller takes dG from the panels alone (dX = dG W_ih from dg_panel, the weight
 * gradients from dgt_panel, the bias gradient from `db`).  On return `gates` still holds the activated gates.  Saves four
 * 4-byte stores per cell and step (ops.py: LSTMLayerFn.backward sets it when every consumer of dG takes a panel). */
#define ASRK_REC_BWD_NO_DG 4
/* Bytes of the inter-workgroup EXCHANGE buffer a launch needs (fragment-ordered h_t / dG_t of
 * every step; the kernels pre-fill it with a NaN sentinel and poll the data itself). 0 = shape
 * unsupported. backward: 0 for rec_fwd, 1 for rec_bwd. */
size_t asrk_lstm_xchg_bytes(int T, int B, int H, int ndir, int backward, int flags);
/* Workgroups (= CUs, one each) a launch of the persistent kernel occupies for this shape; 0 = shape
 * unsupported.  Lets a caller decide what may usefully run beside it on another stream. */
int asrk_lstm_plan_workgroups(int T, int B, int H, int ndir, int backward, int flags);
/* Which kernel a launch of this shape and these flags runs, from the very planner the launches use (tuning knobs
 * included).  Host only when ncu > 0: plan for a device of `ncu` compute units, no device call; ncu == 0: the current
 * device's count.  Returns what the launch would: ASRK_EINVAL (bad flags / shape arguments, NULL info), ASRK_ESHAPE
 * (H % 4 != 0, or no plan), ASRK_EDEVICE (ncu == 0 and no device); T == 0 is ASRK_OK with launches = 0.
 * info[ASRK_LSTM_PLAN_INFO_LEN]:
 *   [0] family: 0 = f32 MFMA kernel, 1 = bf16x6 kernel
 *   [1] forward MT (16-row gate tiles per workgroup; units = 4*MT)   | backward UB (units per workgroup)
 *   [2] NT (16-row batch tiles per workgroup)
 *   [3] forward KGW (k-groups per wave: 4, 8, 16; bf16x6 kernel: its KSW = H / 128) | backward RK (register-resident
 *       k-groups: 0, 32; bf16x6 kernel: 0)
 *   [4] forward db (1 = partial sums double-buffered by step parity) | backward 0
 *   [5] launches   [6] directions per launch   [7] batch groups per launch   [8] workgroups per (direction, group)
 *   [9] batch groups in all   [10] dynamic LDS bytes   [11] workgroups per launch (= asrk_lstm_plan_workgroups)
 *   [12], [13] exchange-buffer bytes, low 31 bits and the rest (= asrk_lstm_xchg_bytes)   [14] the CU count used
 * asrk_lstm_plan_workgroups, asrk_lstm_plan_is_bf and asrk_lstm_xchg_bytes are views of this record at ncu == 0. */
#define ASRK_LSTM_PLAN_INFO_LEN 16
int asrk_lstm_plan_info(int T, int B, int H, int ndir, int backward, int flags, int ncu, int *info);
/* xchg_prefilled != 0: the caller has already set every byte of `xchg` to 0xFF (e.g. on another
 * stream, off the critical path) since its last use; otherwise the launch fills it first. */
int asrk_lstm_rec_fwd_f32(float *G, const float *whh_f, const float *whh_r, float *Y, float *C,
                          int T, int B, int H, int ndir, void *xchg, int xchg_prefilled, void *ws,
                          int flags, void *stream);
/* The same with the time reduction that follows the layer (src/module.py:141-153) fused into the
 * output store: besides Y the kernel writes Y2, the tensor the NEXT layer reads.
 *   pyr_mode 1 ('concat'): Y2 [T/r, B, r*ndir*H], Y2[t/r][b][(t%r)*ndir*H + col] = Y[t][b][col] for
 *                          t < (T/r)*r (trailing frames dropped);
 *   pyr_mode 2 ('drop')  : Y2 [ceil(T/r), B, ndir*H] = Y[0::r];      pyr_mode 0: Y2 unused.
 * The backward variant reads dY in that layout (the gradient w.r.t. Y2; frames that were dropped
 * get zero), so neither direction needs a separate strided-copy pass.  When the reduced tensor is EMPTY
 * ('concat' with T < r) Y2 / dY may be NULL. */
int asrk_lstm_rec_fwd_pyr_f32(float *G, const float *whh_f, const float *whh_r, float *Y, float *C,
                              int T, int B, int H, int ndir, void *xchg, int xchg_prefilled, void *ws,
                              float *Y2, int pyr_mode, int pyr_rate, int flags, void *stream);
int asrk_lstm_rec_bwd_pyr_f32(float *gates, const float *whh_f, const float *whh_r, const float *C,
                              const float *dY, int T, int B, int H, int ndir, void *xchg,
                              int xchg_prefilled, void *ws, float *db, int pyr_mode, int pyr_rate,
                              int flags, void *stream);
/* Panels written by their producers (round 5).  The forward variant ALSO stores the layer's output as the row-major
 * split panel (asrk_split_panel_bytes(rows, K, 0) bytes, ZERO-initialised by the caller once: the kernel overwrites the
 * real extent, the padding stays zero) of the tensor the next layer multiplies - rows (t / r, b), K = r * ndir * H for
 * pyr_mode 1, rows (t, b), K = ndir * H for pyr_mode 0 - so that layer's input projection (asrk_gemm_panels_f32) needs no
 * split pass over it; the BPTT variant stores dG [T*B, ndir*4H] as the panel of dX = dG W_ih likewise (dg_panel,
 * may be NULL) and, in dgt_panel (may be NULL; needs B % 16 == 0, ASRK_ESHAPE otherwise), the TRANSPOSED panel dG^T
 * [ndir*4H rows, K = T*B tokens] (asrk_split_panel_bytes(ndir*4H, T*B, 0) bytes, zero-initialised once) that the
 * layer's weight gradients dW_ih = dG^T X, dW_hh = dG^T H_prev take row / k ranges of.  Only the
 * bf16x6 kernels emit panels (asrk_lstm_plan_is_bf; ASRK_ESHAPE otherwise; no 'drop' reduction, no GRU). */
int asrk_lstm_plan_is_bf(int T, int B, int H, int ndir, int backward, int flags);
int asrk_lstm_rec_fwd_pyr_panel_f32(float *G, const float *whh_f, const float *whh_r, float *Y, float *C,
                                    int T, int B, int H, int ndir, void *xchg, int xchg_prefilled, void *ws,
                                    float *Y2, int pyr_mode, int pyr_rate, void *x2_panel, int flags, void *stream);
int asrk_lstm_rec_bwd_pyr_panel_f32(float *gates, const float *whh_f, const float *whh_r, const float *C,
                                    const float *dY, int T, int B, int H, int ndir, void *xchg,
                                    int xchg_prefilled, void *ws, float *db, int pyr_mode, int pyr_rate,
                                    void *dg_panel, void *dgt_panel, int flags, void *stream);
/* Inference form with PER-ROW sequence lengths `lens` [B] (int64, device): row b runs steps s < lens[b] only and the
 * reverse direction starts at ITS last frame - what nn.LSTM computes when the reference encodes that utterance alone
 * and unpadded, which is how it decodes (bin/test_asr.py:163-167, src/decode.py:64,88: batch 1).  This lets U
 * utterances of different lengths share one encoder pass with results equal to U batch-1 passes.  Frames
 * t >= lens[b] of Y / Y2 / G / C are NOT written: zero-fill Y / Y2 first.  'concat' reduction trims lens[b] % r
 * frames of every row by itself.  No backward counterpart (decoding only). */
int asrk_lstm_rec_fwd_len_f32(float *G, const float *whh_f, const float *whh_r, float *Y, float *C,
                              const int64_t *lens, int T, int B, int H, int ndir, void *xchg,
                              int xchg_prefilled, void *ws, float *Y2, int pyr_mode, int pyr_rate, int flags,
                              void *stream);
/* torch.nn.GRU layers (module 'GRU' of src/module.py:112-113,131 and src/lm.py:20; gate order r, z, n)
 * in the same persistent kernels.  G [T*B, ndir*4H], per direction four H-wide blocks:
 *   in : x W_ir^T + b_ir + b_hr | x W_iz^T + b_iz + b_hz | x W_in^T + b_in | b_hn (every row)
 *   out: r | z | n | W_hn h_{t-1} + b_hn            whh_*: [3H, H] (nn.GRU weight_hh layout)
 * The BPTT entry point reads those blocks plus Y (the forward outputs, = h_{t-1} of the next step) and
 * leaves  dr | dz | dn | dn*r  in `gates`: blocks 0..2 are the input-side gate gradients (dX, dW_ih,
 * db_ih), blocks 0, 1, 3 the hidden-side ones (dW_hh, db_hh); db [ndir*4H] = their column sums.
 * xchg / ws / pyr_* exactly as for the LSTM entry points (same plans: asrk_lstm_xchg_bytes). */
int asrk_gru_rec_fwd_f32(float *G, const float *whh_f, const float *whh_r, float *Y, int T, int B, int H,
                         int ndir, void *xchg, int xchg_prefilled, void *ws, float *Y2, int pyr_mode,
                         int pyr_rate, int flags, void *stream);
int asrk_gru_rec_bwd_f32(float *gates, const float *whh_f, const float *whh_r, const float *Y,
                         const float *dY, int T, int B, int H, int ndir, void *xchg, int xchg_prefilled,
                         void *ws, float *db, int pyr_mode, int pyr_rate, int flags, void *stream);
/* Backward through time.  gates = activated gates from fwd (overwritten IN PLACE with the
 * pre-activation gradients dG, same layout); dY: [T*B, ndir*H] gradient w.r.t. Y (read only).
 * db (optional, [ndir*4H]): the bias gradient colsum(dG), accumulated by the kernel while it produces
 * dG (every workgroup sees all T steps of its units), so no extra pass over dG is needed.
 * Afterwards: dX = dG*W_ih, dW_ih = dG^T*X, dW_hh = dG^T*Y(t-1). */
int asrk_lstm_rec_bwd_f32(float *gates, const float *whh_f, const float *whh_r, const float *C,
                          const float *dY, int T, int B, int H, int ndir, void *xchg,
                          int xchg_prefilled, void *ws, float *db, int flags, void *stream);
/* Copies the in-kernel error word to host after synchronising `stream`; 0 or ASRK_ETIMEOUT. */
int asrk_lstm_check_error(void *ws, void *stream);

/* ---- pure-CTC prefix beam search on the device (CTCBeamDecoder.forward, src/ctc.py:241-352) ---------------
 * Graves-2014 prefix search with the reference's bookkeeping (expansion order, de-duplication by a stable sort
 * on the decimal string of the tokens, first-maximum survivors, stable score sort, length-normalised final
 * ranking) as ONE workgroup per utterance; hypotheses are identical to the reference's.
 *   ctc [T, V]: the log-probabilities the reference hands to its loop (log_softmax applied twice, src/ctc.py:250);
 *   allowed [V] bytes: 1 for members of vocab_range (ascending id order = the reference's tie order);
 *   beam <= 32, beam * (cand + 1) <= 1024, V <= 99999;
 *   lm: NULL, or [beam, V] RNN-LM log-probabilities of the CURRENT beam rows (row i = hypothesis i), weight
 *       lm_weight; with an LM exactly one frame per call (t1 == t0 + 1): after the call the caller steps the LM
 *       for the rows whose gather index is >= beam (new state row = index - beam; otherwise the state of old
 *       row `index` is inherited) - parent row / last token / gather index per new row are in the workspace;
 *   frames [t0, t1) of T are processed (the caller skips leading frames whose arg-max is blank, src/ctc.py:265);
 *   init != 0 resets the beam to the single empty hypothesis first; cur_buf says which of the two beam buffers
 *   holds the beam at t0 (it alternates every frame: after the call it is cur_buf ^ ((t1 - t0) & 1));
 *   lm_step_follows: t < T - 1 and an LM is fused (src/ctc.py:342).
 * ws: asrk_ctc_prefix_beam_ws_bytes(beam, T) bytes, 16-byte aligned, kept between calls of one utterance;
 * asrk_ctc_prefix_beam_ws_offsets gives the byte offsets of the results (all int32): live-row count, lengths
 * [beam], tokens [beam][T + 1] of buffer `buf`, and parent / last-token / gather-index [beam]. */
size_t asrk_ctc_prefix_beam_ws_bytes(int beam, int T);
int asrk_ctc_prefix_beam_ws_offsets(int beam, int T, int buf, int64_t *nb_off, int64_t *len_off, int64_t *tok_off,
                                    int64_t *parent_off, int64_t *last_off, int64_t *gidx_off);
int asrk_ctc_prefix_beam_f32(const float *ctc, int T, int V, const unsigned char *allowed, int beam, int cand,
                             const float *lm, float lm_weight, int t0, int t1, int cur_buf, int init,
                             int lm_step_follows, void *ws, size_t ws_bytes, void *stream);
/* The same search for U utterances in LOCK-STEP with RNN-LM fusion: one launch of U workgroups per step j, then the
 * caller steps the LM ONCE for all U * beam rows.  Workgroup u searches frame t_start[u] + j of utterance u with the
 * phases, scratch and arithmetic of the single-utterance kernel, so its hypotheses do not depend on the batch.
 *   ctc [U, Tmax, V]: frame t of utterance u at ctc + (u * Tmax + t) * ctc_row_stride floats (ctc_row_stride >= V);
 *   allowed [V]: as above, shared by all utterances;
 *   lm [U * beam, V] (required): rows u*beam .. u*beam + beam - 1 are the current beam rows of utterance u;
 *   frames [U], t_start [U] (int32, device): frame count T_u (clamped to Tmax) and the first frame whose arg-max
 *       is not blank; t_start[u] < 0 = all blank, the utterance never runs;
 *   j >= 0: the lock-step index.  Utterance u runs frame t = t_start[u] + j while t < T_u: init = (j == 0), the
 *       current beam buffer is j & 1, lm_step_follows = (t < T_u - 1), last frame = (t == T_u - 1) - its final
 *       beam is in buffer (T_u - t_start[u]) & 1.  A workgroup with nothing to do leaves its slab untouched;
 *   out_parent / out_last / out_gidx [U * beam] (int32, device): per LM row, as GLOBAL row indices - the row
 *       whose LM state it continues (u*beam + i), the token to feed, and the index into cat([old rows, stepped
 *       rows]) of its next state: u*beam + i = inherit old row, U*beam + u*beam + r = stepped row r.  Dead rows
 *       and utterances that did not run export their own row (identity) and token 0 / the token already there:
 *       one index_select per LM tensor, valid indices in every row.
 *   ws: asrk_ctc_prefix_beam_multi_ws_bytes(U, beam, Tmax, &slab) bytes, 16-byte aligned, kept between the calls
 *       of one batch: U slabs of `slab` bytes, each laid out as asrk_ctc_prefix_beam_ws_offsets(beam, Tmax, ...)
 *       describes.  Limits as above (beam <= 32, beam * (cand + 1) <= 1024, V <= 16384), 1 <= U <= 2^20 (the
 *       global row indices are int32). */
size_t asrk_ctc_prefix_beam_multi_ws_bytes(int U, int beam, int Tmax, size_t *slab_stride);
int asrk_ctc_prefix_beam_multi_f32(const float *ctc, int64_t ctc_row_stride, int U, int Tmax, int V,
                                   const unsigned char *allowed, int beam, int cand, const float *lm, float lm_weight,
                                   const int *frames, const int *t_start, int j, int *out_parent, int *out_last,
                                   int *out_gidx, void *ws, size_t ws_bytes, void *stream);

/* ---- back-off n-gram LM step for shallow fusion (no counterpart in the reference, which fuses an RNN-LM only) ----
 * One decode position of an ARPA back-off model for R rows: row r continues the state state_in[parent ? parent[r] : r]
 * (state_in == NULL: the empty context), consumes token[r], writes its new state (one int32: a context node) to
 * state_out[r] and ln p(v | new context) for every v to out[r * row_stride + v], v < V (columns V .. row_stride - 1
 * are not touched).  One workgroup per row, the row written in place (no staging, no limit on V).
 *   image (device memory, built by src/ngram.py: build_image; node 0 = the empty context):
 *     uni_logp [V] f32, uni_next [V] int32: the unigram level, dense - ln(10) * -99 and state 0 for a word without
 *       a unigram; bo [n_nodes] f32, fail [n_nodes] int32 (the context without its oldest token, fail[0] = 0),
 *       child_off [n_nodes + 1] int32 (CSR; node 0 has no entries); word (ascending inside a node), logp, next
 *       [n_entries]: the explicit n-grams above the unigram level, next = the state after the word (resolved by the
 *       builder, for top-order entries too).  word / logp / next may be NULL when n_entries == 0 (a unigram model).
 *   advance: binary-search token[r] among the children of the state, follow fail on a miss, uni_next at node 0; a
 *       token outside [0, V) leads to the empty context.
 *   scores: with the chain c_0 = new state, c_k = fail[c_k-1], c_d = 0 and B_0 = +0, B_k = fl(B_k-1 + bo[c_k-1]):
 *       out[v] = fl(B_d + uni_logp[v]), then for k = d - 1 .. 0 out[word[e]] = fl(B_k + logp[e]) over the entries of
 *       c_k (the longest context wins).  f32 adds in exactly this order, no atomics: a row's result depends on the
 *       image and its own (state, token) only, not on R, its position or the launch.
 *   token [R] int64; parent [R] int32, or int64 when parent_is_i64 != 0, or NULL; n_state = rows of state_in (a
 *       parent outside [0, n_state) reads the empty context); state_out must not be state_in.
 * ASRK_EINVAL, checked before any device call: order outside 1..8, V <= 0, n_nodes < 1, a negative count, a NULL
 * image array, row_stride < V; for R > 0 also a NULL token / state_out / out.  R == 0 is ASRK_OK. */
int asrk_ngram_step_f32(int order, int V, int n_nodes, int n_entries, const float *uni_logp,
                        const int32_t *uni_next, const float *bo, const int32_t *fail, const int32_t *child_off,
                        const int32_t *word, const float *logp, const int32_t *next, const int32_t *state_in,
                        int n_state, const int64_t *token, const void *parent, int parent_is_i64, int32_t *state_out,
                        float *out, int64_t row_stride, int R, void *stream);

/* ---- contextual biasing: a phrase-boosting automaton behind the same row contract (no counterpart in the reference) ----
 * An Aho-Corasick automaton over the model's tokens, built by src/bias.py: build_image (node 0 = the root):
 *     phi [n_nodes] f32: the pending (not yet banked) bonus of a node, phi[0] = 0;
 *     root_arrive [V] f32, root_next [V] int32: arrive[goto(0, v)] and goto(0, v), dense;
 *     ext_off [n_nodes + 1] int32 (CSR; node 0 has no entries); ext_word (strictly ascending inside a node), ext_arrive,
 *     ext_next [n_entries]: for node n >= 1 the children of every node on its fail chain except the root, merged so
 *     that the deepest node wins.  The three ext_* arrays may be NULL when n_entries == 0.
 *   goto(s, v): the entry of s that holds v, else (root_next[v], root_arrive[v]); a token outside [0, V) leads to the
 *     root with arrive 0.  delta(s, v) = fl(arrive[goto(s, v)] - phi[s]): one f32 subtraction of two stored values.
 * asrk_bias_step_f32: row r continues state_in[parent ? parent[r] : r] (state_in == NULL or a parent outside
 *   [0, n_state): the root), consumes token[r], writes its new state s' to state_out[r] and delta(s', v) to
 *   out[r * row_stride + v] for v < V (columns V .. row_stride - 1 are not touched).  One workgroup per row.
 * asrk_ngram_bias_step_f32: the n-gram step of asrk_ngram_step_f32 and the biasing step in one launch that writes the
 *   row once.  States are int32 pairs (n-gram node, automaton node): state_in [n_state, 2], state_out [R, 2].
 *   out[v] = fl(L(v) + delta(s', v)) with L(v) bit for bit what asrk_ngram_step_f32 writes: one f32 add, no multiply.
 * asrk_bias_walk: sequence h = tokens[h * token_stride + i], i < min(max(n_tok[h], 0), L), walked from the root:
 *   state[h] = the final node, total[h] = the f32 sum of its deltas in token order, residual[h] = phi[state[h]].
 * token(s) int64; parent [R] int32, or int64 when parent_is_i64 != 0, or NULL; state_out must not be state_in.
 * ASRK_EINVAL, checked before any device call: V <= 0, n_nodes < 1, a negative count, a NULL image array (ext_* only
 * when n_entries > 0), row_stride < V, token_stride < L, the n-gram conditions of asrk_ngram_step_f32; for R > 0 (H > 0)
 * also a NULL token / state / output array and state_out == state_in.  R == 0 (H == 0) is ASRK_OK. */
int asrk_bias_step_f32(int V, int n_nodes, int n_entries, const float *phi, const float *root_arrive,
                       const int32_t *root_next, const int32_t *ext_off, const int32_t *ext_word,
                       const float *ext_arrive, const int32_t *ext_next, const int32_t *state_in, int n_state,
                       const int64_t *token, const void *parent, int parent_is_i64, int32_t *state_out, float *out,
                       int64_t row_stride, int R, void *stream);
int asrk_ngram_bias_step_f32(int order, int V, int n_nodes, int n_entries, const float *uni_logp,
                             const int32_t *uni_next, const float *bo, const int32_t *fail, const int32_t *child_off,
                             const int32_t *word, const float *logp, const int32_t *next, int b_nodes, int b_entries,
                             const float *phi, const float *root_arrive, const int32_t *root_next,
                             const int32_t *ext_off, const int32_t *ext_word, const float *ext_arrive,
                             const int32_t *ext_next, const int32_t *state_in, int n_state, const int64_t *token,
                             const void *parent, int parent_is_i64, int32_t *state_out, float *out, int64_t row_stride,
                             int R, void *stream);
int asrk_bias_walk(int V, int n_nodes, int n_entries, const float *phi, const float *root_arrive,
                   const int32_t *root_next, const int32_t *ext_off, const int32_t *ext_word, const float *ext_arrive,
                   const int32_t *ext_next, const int64_t *tokens, int64_t token_stride, const int32_t *n_tok, int L,
                   int H, int32_t *state, float *total, float *residual, void *stream);

/* ---- attention decoder step (src/module.py:179-258, src/asr.py:277-313) -------------------
 * BN = B*num_head rows ordered (b, head).  All tensors contiguous f32; lens int64 [B].
 * loc_conv:  c[b,t,k] = sum_{n,j} prev_att[b,n,t+j-ks] * Wc[k,n,j]   (Conv1d(N,K,2ks+1,pad ks))
 * energy:    loc=1: e = we . tanh(key + q + tanh(Wp c)) + be ; loc=0: e = key . q
 *            attn = softmax(e / temperature) over t < lens[b], 0 beyond (masked_fill(-inf)).
 *            e_scratch: [BN,T] floats of scratch for the scaled energies.
 * context:   ctx[bn,:] = sum_t attn[bn,t] * value[bn,t,:]  (row stride ctx_stride, so it can be
 *            written straight into the decoder's [emb | ctx] input buffer).
 * Backward kernels ACCUMULATE (+=) into *_acc buffers owned by the caller (zeroed once per
 * sequence): dkey_acc [BN,T,A], dWc_acc, dWp_acc, dwe_acc, dbe_acc.  dq/dattn/dprev_att/dc are
 * per-step outputs (dc is scratch [B,T,K], zeroed inside). */
int asrk_loc_conv_fwd_f32(const float *prev_att, const float *Wc, float *c, int B, int N, int T,
                          int K, int ks, void *stream);
int asrk_loc_conv_bwd_f32(const float *dc, const float *prev_att, const float *Wc,
                          float *dprev_att, float *dWc_acc, int B, int N, int T, int K, int ks,
                          void *stream);
int asrk_attn_energy_fwd_f32(int loc, const float *key, const float *q, const float *c,
                             const float *Wp, const float *we, const float *be,
                             const int64_t *lens, float *attn, float *e_scratch, int B, int N, int T,
                             int A, int K, float temperature, void *stream);
int asrk_attn_energy_bwd_f32(int loc, const float *key, const float *q, const float *c,
                             const float *Wp, const float *we, const int64_t *lens,
                             const float *attn, const float *dattn, float *dkey_acc, float *dq,
                             float *dc, float *dWp_acc, float *dwe_acc, float *dbe_acc, int B,
                             int N, int T, int A, int K, float temperature, void *stream);
/* The launch geometry asrk_attn_energy_fwd_f32 (bwd == 0) / asrk_attn_energy_bwd_f32 (bwd != 0) use for BN = B*N rows,
 * from the one host function both launchers call; host only (no device call, runs without a GPU;
 * tests/test_attention_plan_cpu.py holds the attention case table to it).  K is ignored when loc == 0.
 *   *tpb: frames per workgroup (the backward halves it, down to 8, while its LDS exceeds 150 KB)
 *   *chunks: workgroups per row = ceil(T / tpb) (grid = BN x chunks)   *lds_bytes: dynamic LDS of the launch
 * The status is the launcher's for the same sizes: ASRK_EINVAL for BN < 0, T <= 0, A <= 0, loc with K <= 0 (or a NULL
 * output pointer here); ASRK_ESHAPE for loc && bwd && K > 16 and for LDS over 150 KB; BN == 0 is ASRK_OK.  The three
 * outputs are 0 unless a launch would happen. */
int asrk_attn_energy_plan(int loc, int bwd, int BN, int T, int A, int K, int *tpb, int *chunks,
                          int64_t *lds_bytes);
int asrk_attn_context_fwd_f32(const float *attn, const float *value, float *ctx, int BN, int T,
                              int Dv, int64_t ctx_stride, void *stream);
int asrk_attn_context_bwd_f32(const float *dctx, const float *value, float *dattn, int BN, int T,
                              int Dv, int64_t dctx_stride, void *stream);

/* ---- one LSTM cell step (src/asr.py:218 decoder nn.LSTM on a length-1 sequence) ----------
 * gates [B,4H] = x W_ih^T + h W_hh^T + b (i,f,g,o) -> activated in place; c = f*c_prev + i*g;
 * h = o*tanh(c).  bwd: gates (activated) -> pre-activation grads in place; dh/dc_in may be NULL. */
int asrk_lstm_cell_fwd_f32(float *gates, const float *c_prev, float *c, float *h, int B, int H,
                           void *stream);
int asrk_lstm_cell_bwd_f32(float *gates, const float *c_prev, const float *c, const float *dh,
                           const float *dc_in, float *dc_prev, int B, int H, void *stream);

/* ---- GRU cell, one step (module: 'GRU' of src/module.py:112-113, src/asr.py:175-176, src/lm.py:20-21)
 * gi = x W_ih^T + b_ih, gh = h W_hh^T + b_hh: rows of 3H (gate order r, z, n; row strides ldi/ldh).
 * fwd: h_new = (1-z) n + z h_prev; r, z, n are written over gi (gh keeps gh_n).  h_prev NULL = zeros.
 * bwd: the gradient of h' is dh + dh2 (either may be NULL; dh2 is contiguous [B,H]: the carried
 *      recurrent gradient); gi/gh (as left by fwd) are overwritten with dL/dgi and dL/dgh; dh_prev = dh * z (the caller
 * adds dgh W_hh).  Then dx = dgi W_ih, dW_ih = dgi^T x, dW_hh = dgh^T h_prev, db = column sums. */
int asrk_gru_cell_fwd_f32(float *gi, const float *gh, int64_t ldi, int64_t ldh, const float *h_prev,
                          int64_t ldp, float *h_new, int64_t ldn, int B, int H, void *stream);
int asrk_gru_cell_bwd_f32(float *gi, float *gh, int64_t ldi, int64_t ldh, const float *h_prev,
                          int64_t ldp, const float *dh, int64_t ldd, const float *dh2, float *dh_prev,
                          int64_t ldo, int B, int H, void *stream);

/* ---- embedding gather / scatter-add (src/asr.py:103-109,134,142: nn.Embedding) ------------ */
int asrk_embedding_fwd_f32(const int64_t *idx, const float *W, float *out, int64_t n, int D, int V,
                           void *stream);
int asrk_embedding_bwd_f32(const int64_t *idx, const float *dout, float *dW_acc, int64_t n, int D,
                           int V, void *stream);

/* ---- word-embedding plug-in (src/plugin.py:7-160 EmbeddingRegularizer; csrc/emb_fuse.hip) ---------------------
 * Rows n = 0..N-1 (N = B*L in training, the live beam rows at a decode position), vocabulary V, embedding width E.
 * None of these kernels uses a float atomic: every sum has a fixed order, so results are bit-reproducible.
 *
 * Fused distribution (src/plugin.py:103-123): with a_v = max(temp_v, 0) * emb_logit[n,v], pd = softmax(dec_logit[n,:]),
 * pe = softmax(a), s_v = sigmoid(lam_v) (lam_is_logit != 0) or lam_v,
 *     y[n,v] = log((1 - s_v) * pd_v + s_v * pe_v + eps).
 * dec_logit has leading dimension ld >= V; emb_logit, y and every gradient are dense [N,V].  temp and lam hold 1 or V
 * floats (temp_len / lam_len; anything else: ASRK_EINVAL).  stats [N,4] receives the row maximum and the sum of
 * exponentials of both softmaxes; the backward recomputes pd / pe from them.
 * bwd: g = dL/dy [N,V] -> d_dec, d_emb [N,V]; dtemp [temp_len] / dlam [lam_len] when not NULL (summed over rows, and
 *      over v for a scalar; dlam is with respect to the logit when lam_is_logit).  ws: asrk_emb_fuse_bwd_ws_bytes
 *      (want_* = the matching pointer is not NULL) bytes of device scratch, 4-byte aligned; ASRK_EWORKSPACE if smaller.
 * Both: ASRK_EINVAL for a NULL pointer, V <= 0, ld < V or a bad length, checked before any device call. */
size_t asrk_emb_fuse_bwd_ws_bytes(int N, int V, int temp_len, int lam_len, int want_dtemp, int want_dlam);
int asrk_emb_fuse_fwd_f32(const float *dec_logit, int ld, const float *emb_logit, const float *temp, int temp_len,
                          const float *lam, int lam_len, int lam_is_logit, float eps, int N, int V, float *y,
                          float *stats, void *stream);
int asrk_emb_fuse_bwd_f32(const float *g, const float *dec_logit, int ld, const float *emb_logit, const float *temp,
                          int temp_len, const float *lam, int lam_len, int lam_is_logit, float eps, const float *stats,
                          int N, int V, float *d_dec, float *d_emb, float *dtemp, float *dlam, void *ws,
                          size_t ws_bytes, void *stream);
/* Cosine embedding loss against table[label] (src/plugin.py:137-155; nn.CosineEmbeddingLoss(reduction='none'), target
 * +1): row_loss[n] = 1 - x.y / sqrt((|x|^2 + 1e-12)(|y|^2 + 1e-12)) with y = table[label[n]] read in place, 0 where
 * label[n] == 0 (or outside the table); loss[0] = mean_b(sum_t row_loss[b,t] / count[b]), count[b] = #{t: label != 0}
 * (an utterance without labels gives NaN, as in the reference).  x [B*L,E], table [table_rows,E], label [B,L].
 * bwd: gout = dL/dloss (device scalar) -> dx [B*L,E] and, when not NULL, dy [B*L,E] = the gradient of the gathered
 *      rows; for a trainable table asrk_cos_emb_table_grad_f32 turns it into dtable [table_rows,E] (zeroed first):
 *      dtable[v] = sum of dy[n] over label[n] == v in row order - a fixed order, unlike the atomic scatter of
 *      asrk_embedding_bwd_f32, so repeated labels give the same bits every run. */
int asrk_cos_emb_loss_fwd_f32(const float *x, const float *table, int64_t table_rows, const int64_t *label, int B,
                              int L, int E, float *row_loss, float *count, float *loss, void *stream);
int asrk_cos_emb_loss_bwd_f32(const float *x, const float *table, int64_t table_rows, const int64_t *label, int B,
                              int L, int E, const float *count, const float *gout, float *dx, float *dy,
                              void *stream);
/* NLLLoss(ignore_index) over log-probabilities (bin/train_asr.py:62): sums[0] = sum of -logp[r, t_r] over the rows
 * with t_r != ignore_index, sums[1] = their number (mean = sums[0] / sums[1]; no such row: 0/0).
 * bwd: dlogp[r,:] = 0 except dlogp[r, t_r] = -gscale[0] on counted rows; gscale is a device scalar. */
int asrk_cos_emb_table_grad_f32(const float *dy, const int64_t *label, int N, int E, int64_t table_rows,
                                float *dtable, void *stream);
int asrk_nll_loss_fwd_f32(const float *logp, int rows, int V, int ld, const int64_t *targets, int ignore_index,
                          float *sums, void *stream);
int asrk_nll_loss_bwd_f32(int rows, int V, int ld, const int64_t *targets, int ignore_index, const float *gscale,
                          float *dlogp, void *stream);
/* Row L2 normalisation (src/plugin.py:107-108; F.normalize): y = x / max(|x|, eps), norm[r] = |x_r|.
 * bwd: dx = (dy - y (y.dy)) / |x| where |x| >= eps, dy / eps below the clamp. */
int asrk_l2norm_fwd_f32(const float *x, float *y, float *norm, int rows, int D, float eps, void *stream);
int asrk_l2norm_bwd_f32(const float *y, const float *dy, const float *norm, float *dx, int rows, int D, float eps,
                        void *stream);

/* ---- the attention-decoder ("speller") loop as one call per direction ---------------------------
 * Replaces the teacher-forced decode loop of ASR.forward (src/asr.py:112-148 with tf_rate == 1) and
 * the autograd graph under it: per step Attention.forward (src/asr.py:277-313) ->
 * LocationAwareAttention.forward (src/module.py:234-258) -> Decoder.forward (src/asr.py:214-221).
 * Single head, location-aware attention, single-layer LSTM (or, `cell` = 1, GRU) decoder.  All buffers are caller-owned;
 * "tape" buffers written by the forward call are read by the backward call.
 *
 *   dims     B batch, Te encoder frames, A attention dim, Dv encoder feature dim, K/ks location
 *            kernels / half width (2ks+1 taps), H decoder dim, E embedding dim, L decode steps
 *   memory   key [B,Te,A] = tanh(proj_k(enc)), value [B,Te,Dv] = enc, lens [B]
 *   weights  Wq [A,H], bq [A]; Wc [K,1,2ks+1]; Wp [A,K]; we [A]; be [1]; W_ih [4H,E+Dv]; W_hh [4H,H];
 *            b_ih, b_hh [4H] (only read by asrk_speller_step_f32)
 *   eproj    [L,B,4H] = emb_t W_ih[:, :E]^T + b_ih + b_hh for the known (teacher) inputs of all steps
 *   tape     q [L,B,A]; conv [L,B,Te,K]; attn: row (b, step t) at attn + b*attn_ld + t*attn_step
 *            (att_seq [B,1,L,Te]: attn_ld = L*Te, attn_step = Te); ctx [L,B,Dv]; gates [L,B,4H]
 *            (activated i,f,g,o; the backward call turns them into pre-activation gradients in
 *            place); h, c [L+1,B,H] (slot 0 = initial state, written by the caller);
 *            states [B,L,H] = h_1..h_L batch-major (optional); e_scratch [B,Te];
 *            prev0 [B,Te] = the uniform attention that feeds step 0 (src/module.py:239-242). */
typedef struct asrk_speller {
    int B, Te, A, Dv, K, ks, H, E, L;
    float temperature;
    int shared_kv;   /* != 0 (asrk_speller_step_f32 only): key [1,Te,A], value [1,Te,Dv], lens [1] are one
                        utterance shared by all B rows (the live hypotheses of a beam search) */
    const float *key, *value;
    const int64_t *lens;
    const float *Wq, *bq, *Wc, *Wp, *we, *be, *W_ih, *W_hh, *b_ih, *b_hh;
    const float *eproj;
    float *q, *conv, *attn;
    int64_t attn_ld, attn_step;
    float *ctx, *gates, *h, *c, *states, *e_scratch;
    const float *prev0;
    const int *row_mem;   /* optional (asrk_speller_step_f32 only): batch row b attends over memory row row_mem[b] of
                             key [U,Te,A] / value [U,Te,Dv] / lens [U] - the beams of U utterances decoded together
                             (reference fan-out over utterances: bin/test_asr.py:163-167); NULL: row b / shared_kv */
    int cell;             /* 0: LSTM decoder cell (gates i,f,g,o).  1: GRU cell (src/asr.py:172 with module 'GRU')
                             in the SAME four-rows-per-unit layout:
                             rows [0,H) r, [H,2H) z, [2H,3H) n_x = W_in x + b_in, [3H,4H) n_h = W_hn h + b_hn, i.e.
                             W_ih = [W_ir; W_iz; W_in; 0], W_hh = [W_hr; W_hz; 0; W_hn] (the caller stacks them);
                             h' = (1 - z) tanh(n_x + r n_h) + z h.  The gates tape holds r, z, n, n_h; c is not used */
    /* stacked LSTM decoder (nn.LSTM(num_layers = nlayer), src/asr.py:175-176; round 6): nlayer 0 / 1 = one layer (the
       fields above), up to ASRK_SPELLER_MAX_LAYERS.  Upper layer l = 1.. uses slot l - 1 of: Wu_ih [4H,H], Wu_hh
       [4H,H], bu_ih / bu_hh [4H] (read by the forward call), tapes hu / cu [L+1,B,H] (slot 0 = initial state) and gu
       [L,B,4H] (activated gates; pre-activation gradients after the backward call).  Wq is then [A, nlayer*H] (the
       query reads the layer-concatenated state, src/asr.py:207-212), `states` receives the TOP layer's outputs and W_ih
       / W_hh / h / c / gates are layer 0's.  LSTM cells only (cell == 0); asrk_speller_step_f32 takes one layer. */
    int nlayer;
    const float *Wu_ih[2], *Wu_hh[2], *bu_ih[2], *bu_hh[2];
    float *hu[2], *cu[2], *gu[2];
    /* attention variants of the loop (round 6; asrk_speller_step_f32 takes neither).  att_mode 0: location-aware (all of
       the above); 1: ScaleDotAttention (src/module.py:198-212): e = q . key / temperature, no Wc / Wp / we / be / conv /
       prev0 (K = ks = 0 allowed).  nhead N > 1 (dot only; the location-aware form convolves ACROSS the heads' previous
       alignments, src/module.py:221,244): key [B*N,Te,A], value [B*N,Te,Dv] and lens [B] as src/asr.py:294-304 builds
       them (row b*N + n; heads of an utterance share lens[b]); Wq [N*A, nlayer*H]; the tapes q [L,B,N*A], attn (rows
       b*N + n, same attn_ld / attn_step addressing) and e_scratch [B*N,Te] hold B*N rows; ctxh [L,B,N*Dv] receives the
       heads' contexts and ctx = ctxh Wm^T + bm (merge_head, Wm [Dv, N*Dv], src/asr.py:308-311). */
    int att_mode, nhead;
    const float *Wm, *bm;
    float *ctxh;
    /* asrk_speller_step_f32 with row_mem only: RG > 1 = the batch rows [g*RG, (g+1)*RG) all attend over memory
       row_mem[g*RG] (the beam of one utterance in consecutive rows, B % RG == 0, RG <= 32): the context kernel then reads
       an utterance's value memory once per utterance instead of once per row.  0 / 1: no such promise. */
    int row_group;
} asrk_speller_t;
#define ASRK_SPELLER_MAX_LAYERS 3

/* backward-only buffers.  dstates [B,L,H] = dLoss/dh_t (batch-major, from the vocabulary projection);
 * dattn_seq = gradient of att_seq (same addressing as attn) or NULL; WT [(Dv+H),4H] =
 * [W_ih[:,E:] | W_hh]^T and WqT [H,A] = Wq^T (asrk_transpose_ld_f32).
 * Accumulated (+=, zero them first): dkey [B,Te,A]; per-workgroup partial sums dwe_part [B*tc,A],
 * dWp_part [B*tc,A*K], dbe_part [B*tc], dWc_part [B,K*(2ks+1)] (reduce over the leading axis
 * afterwards); tc from asrk_speller_plan.  Written: dxh [L,B,Dv+H] (dctx_t | dh via W_hh),
 * dq_pre [L,B,A] = dq_t (1 - q_t^2).  Scratch: dattn, dprev [B,Te]; dconv [B,Te,K];
 * dq_part [B*tc,A]; dc [B,H].  After the call `gates` holds dG [L,B,4H]; the weight gradients are
 * whole-sequence GEMMs over the tape (dW_ih = dG^T [emb|ctx], dW_hh = dG^T h_{0..L-1},
 * dWq = dq_pre^T h_{0..L-1}, dvalue[b] = attn[b]^T dctx[b], demb = dG W_ih[:, :E]). */
typedef struct asrk_speller_bwd {
    const float *dstates, *dattn_seq, *WT, *WqT;
    float *dkey, *dxh, *dq_pre, *dattn, *dprev, *dconv, *dq_part, *dwe_part, *dWp_part, *dbe_part,
        *dWc_part, *dc;
    int tc;
    /* stacked decoder, upper layer l = 1.. in slot l - 1: WuT [2H,4H] = [W_ih_l | W_hh_l]^T; dxu [L,B,2H] written
       (d h of the layer below at the same step | d h of layer l's previous step); dcu [B,H] scratch.  WqT is
       [nlayer*H, A]; the upper layers' weight gradients are dW_ih_l = dG_l^T h_{l-1}[1..L], dW_hh_l = dG_l^T h_l[0..L-1]. */
    const float *WuT[2];
    float *dxu[2], *dcu[2];
    /* nhead > 1: WmT [N*Dv, Dv] = Wm^T; dctxh [L,B,N*Dv] written (gradient of the heads' contexts: dvalue's operand, and
       dWm = dctx^T ctxh).  With several heads dkey is [B*N,Te,A], dq_pre [L,B,N*A], dattn [B*N,Te], dq_part [B*N*tc,A];
       the location-only buffers (dprev, dconv, dwe_part, dWp_part, dbe_part, dWc_part) may be NULL for att_mode 1. */
    const float *WmT;
    float *dctxh;
} asrk_speller_bwd_t;

/* number of frame chunks (workgroups per utterance) the energy kernels will use: sizes the
 * per-workgroup partial buffers above */
int asrk_speller_plan(const asrk_speller_t *dims, int *tc_fwd, int *tc_bwd);
/* read-only report of the kernel variants the same plan selects (host only, nothing is launched):
 * info[8] = {ae2_na, ae2_km, eb3_na, eb3_km, tpb_f, tpb_b, KP, ctx_vec}.  ae2 / eb3 = the <NA, KM> instantiation of
 * the one-round-trip forward / backward energy kernel, NA == 0: the staged kernel runs; tpb = frames per
 * workgroup; KP = padded row pitch of Wp in LDS; ctx_vec = Dv % 4 == 0 (vector softmax/context kernel, given a
 * 16-byte aligned value).  Dot-product plans (att_mode 1) report 0 in the first four slots. */
int asrk_speller_plan_info(const asrk_speller_t *dims, int *info);
/* read-only report of the softmax/context kernel a step of this descriptor launches for slot 0, from the function the
 * launch itself calls (host only, nothing is launched): *variant = 0 per-row kernel with scalar loads, 1 per-row kernel
 * with 16-byte loads (Dv % 4 == 0, aligned value), 2 the row-grouped kernel (row_group = RG in 2..32, B % RG == 0, one
 * head, no shared_kv, RG * round4(Te) floats <= 64 KiB, (B / RG) * ceil(Dv / 256) >= 64 workgroups).  Alignment is read
 * from the descriptor's value / ctx pointers; a null pointer counts as aligned. */
int asrk_speller_ctx_variant(const asrk_speller_t *dims, int *variant);
int asrk_speller_fwd_f32(const asrk_speller_t *p, void *stream);
int asrk_speller_bwd_f32(const asrk_speller_t *p, const asrk_speller_bwd_t *g, void *stream);
/* one attention + decoder-cell step outside the training loop (greedy / beam decoding,
 * src/decode.py:110-121): tape slot `slot` (h, c slots slot -> slot+1), previous attention rows at
 * prev_att + b*prev_ld, embedded previous tokens emb [B,E]; eproj is not read (the embedding goes
 * through W_ih[:, :E] inside the step, plus b_ih + b_hh).  emb == NULL: the attention half only (query from h slot
 * `slot`, energies, alignment, context) - the caller runs the decoder cell itself (W_ih, W_hh, b_*, c not read; with many
 * rows the host layer uses bf16x6 panel GEMMs against weight panels split once per decode).  In that form Wq == NULL
 * means that q slot `slot` already holds the query tanh(h Wq^T + bq) (the same host route). */
int asrk_speller_step_f32(const asrk_speller_t *p, int slot, const float *prev_att, int64_t prev_ld,
                          const float *emb, void *stream);
/* dvalue[b,t',d] = sum_l attn(b, l)[t'] * dxh[l*step_ld + b*row_ld + d]  (overwritten): the gradient of
 * the encoder memory `value` over a whole decode loop from the tape (attn addressing as above, dctx_l
 * = the first Dv columns of dxh's step-l rows). */
int asrk_speller_dvalue_f32(const float *attn, int64_t attn_ld, int64_t attn_step, const float *dxh,
                            int64_t step_ld, int64_t row_ld, float *dvalue, int B, int L, int Te, int Dv,
                            void *stream);
/* joint token scores of one beam-search step (src/decode.py:123-148), rows = live hypotheses:
 *   out = (1 - ctc_weight) * att_logp + ctc_weight * hack,  hack[r, cand[r,c]] = psi[r,c] - prev_ctc[r],
 *   LOG_ZERO elsewhere;  out[:, 0] = LOG_ZERO;  out += lm_weight * lm_logp
 * cand NULL = no CTC term; lm_logp NULL = no LM term; out must not alias att_logp. */
int asrk_joint_score_f32(const float *att_logp, const int64_t *cand, const float *psi,
                         const float *prev_ctc, const float *lm_logp, float *out, int n, int V, int C,
                         double ctc_weight, double lm_weight, double logzero, void *stream);
/* one nn.LSTM step on a length-1 sequence, input projection, recurrent projection and cell update in
 * ONE kernel (decoder / RNN-LM steps of the beam search, src/decode.py:113,143-146, src/lm.py:38):
 * gates = x W_ih^T + h W_hh^T + b_ih + b_hh (x rows at x + m*ldx, In features), then c', h'.
 * Out-of-place: h_out / c_out must not alias h / c. */
int asrk_lstm_cell_fused_f32(const float *x, int64_t ldx, int In, const float *h, const float *c,
                             const float *W_ih, const float *W_hh, const float *b_ih,
                             const float *b_hh, float *h_out, float *c_out, int B, int H, void *stream);
/* out[c*ldo + r] = in[r*ldi + c] */
int asrk_transpose_ld_f32(const float *in, int64_t ldi, float *out, int64_t ldo, int rows, int cols,
                          void *stream);

/* ---- per-frame regularisers (src/module.py:116-119,135-138; src/asr.py:36,162) --------------
 * layer_norm: torch.nn.LayerNorm(cols) over contiguous rows [rows, cols]: biased variance, eps
 *   inside the sqrt; fwd also returns mean/rstd [rows] for the backward.  bwd: dx (may be NULL),
 *   dweight/dbias [cols] (both or neither; overwritten).
 * dropout: inverted dropout y = keep ? x/(1-p) : 0.  keep(i) is a pure function of
 *   (seed, offset, i): word i%4 of Philox4x32-10(counter = (i/4, offset), key = seed), kept when
 *   (word >> 8) >= round(p * 2^24).  No mask is stored: the backward is the same call on dy. */
int asrk_layer_norm_fwd_f32(const float *x, const float *weight, const float *bias, float *y,
                            float *mean, float *rstd, int rows, int cols, float eps, void *stream);
int asrk_layer_norm_bwd_f32(const float *x, const float *weight, const float *dy, const float *mean,
                            const float *rstd, float *dx, float *dweight, float *dbias, int rows,
                            int cols, void *stream);
int asrk_dropout_f32(const float *x, float *y, int64_t n, float p, uint64_t seed, uint64_t offset,
                     void *stream);

/* ---- device-side beam bookkeeping of the joint CTC-attention(-LM) search (src/decode.py:150-167, 209-239) ----------
 * One decode position t of U utterances at once, no read-back.  Utterance u owns the row slots [u*B, (u+1)*B); at
 * position t every live row (alive[row] != 0) is a hypothesis of t labels with score sum ssum[row] (float64: the
 * reference's Python floats).  Inputs: the position's top-B scores / labels of every row (topv / topi [U*B, B]) and, with
 * CTC (C > 0), the C candidates' labels and prefix scores (cand / psi [U*B, C]).  Per utterance the B*B continuations are
 * taken in the reference's record order (hypothesis-major, rank-minor), <eos> (label 1) and labels missing from `cand`
 * are dropped, and the B best by AVERAGE score (ssum + score) / (t + 1), ties in record order, go to the utterance's
 * slots in rank order:  prev_token / parent (row of position t) / col (candidate column) / pctc (psi of that column) /
 * ssum / alive, and row t of the back-pointer history hist_tok / hist_sc / hist_par [lmax][U*B].
 * Finished hypotheses are appended to the utterance's log (fin_* [U][fcap], fin_count [U]): kind 0 = row fin_row of
 * position fin_t followed by <eos> with score fin_term (a row whose top-B holds <eos>, once t >= min_len[u]; the LAST
 * <eos> among its top-B); kind 1 = the continuation in slot fin_row of position fin_t that was alive when the utterance
 * ended (no continuation left, t + 1 >= max_len[u], or B == 1 after its first finished hypothesis - then no kind-1
 * entries).  An ended utterance sets utt_done[u], clears its rows and decrements *live_utts.
 * B <= 32, C <= 48 (ASRK_ESHAPE).  All pointers are device memory. */
int asrk_beam_select_f32(const float *topv, const int64_t *topi, const float *psi, const int64_t *cand, int U, int B, int C,
                         int t, int lmax, int fcap, const int *min_len, const int *max_len, int *alive, double *ssum,
                         int *utt_done, int64_t *prev_token, int64_t *parent, int64_t *col, float *pctc, int *hist_tok,
                         float *hist_sc, int *hist_par, int *fin_count, int *fin_kind, int *fin_t, int *fin_row,
                         float *fin_term, double *fin_ssum, int *live_utts, void *stream);

/* The survivors' states for the next decode position in ONE launch: for segment s < nseg (<= 8) and row i < n
 *   dst[s][i, :] = src[s][parent[i] * mul[s] + (use_col[s] ? col[i] : 0), :]      rows of row_floats[s] floats
 * (decoder h / c and the previous alignment: mul 1; the CTC prefix state r [rows, C, Te, 2]: mul = C, use_col = 1, rows of
 * 2*Te floats; LM state layers: one segment each).  src / dst / row_floats / mul / use_col are HOST arrays of nseg entries;
 * parent / col device int64 [n].  Sources and destinations must not overlap. */
int asrk_gather_rows_multi_f32(int nseg, const float *const *src, float *const *dst, const int *row_floats, const int *mul,
                               const int *use_col, const int64_t *parent, const int64_t *col, int n, void *stream);

/* ---- convolutional prenets (src/module.py:7-90: VGGExtractor / CNNExtractor) -----------------
 * Activations are channels-last [B, H(time), W(freq), C].  A convolution is im2col -> asrk_gemm_f32
 * against weight.view(Cout, Cin*KH*KW) (+bias) -> [B*Ho*Wo, Cout] = the next channels-last tensor.
 * im2col: col[(b,ho,wo), (cin*KH+kh)*KW+kw] = x[b*sb + (ho*SH+kh-PH)*sh + (wo*SW+kw-PW)*sw + cin*sc]
 *         (0 outside the input); Ho/Wo = asrk_conv_out_size(extent, k, stride, pad) (0 = invalid).
 * col2im: the adjoint (gather form, overwrites dx at the same strides).
 * relu_fwd is in place; relu_bwd: dx = y > 0 ? dy : 0.
 * maxpool2x2: stride 2, floor mode, x contiguous [B,H,W,C]; y / dy addressed with explicit output
 *         strides (osb, osh, osw, osc) so the last pool can emit [B, T/4, C*F/4] directly
 *         (src/module.py:62-65); idx [B,H/2,W/2,C] keeps the arg-max (0..3) for the backward, which
 *         writes every element of the contiguous dx. */
int asrk_conv_out_size(int in, int k, int stride, int pad);
int asrk_im2col_f32(const float *x, float *col, int B, int H, int W, int C, int KH, int KW, int SH, int SW,
                    int PH, int PW, int64_t sb, int64_t sh, int64_t sw, int64_t sc, void *stream);
int asrk_col2im_f32(const float *dcol, float *dx, int B, int H, int W, int C, int KH, int KW, int SH,
                    int SW, int PH, int PW, int64_t sb, int64_t sh, int64_t sw, int64_t sc, void *stream);
/* im2col with patch rows ldcol >= C*KH*KW floats apart, columns C*KH*KW .. ldcol-1 written as zeros: a K that is not a
 * multiple of 4 (the first VGG layer: 1-3 channels x 9 taps) padded up so that the GEMMs over the patches take their
 * 16-byte paths (against a weight padded with zero columns; the extra dW columns are dropped). */
int asrk_im2col_ld_f32(const float *x, float *col, int ldcol, int B, int H, int W, int C, int KH, int KW, int SH, int SW,
                       int PH, int PW, int64_t sb, int64_t sh, int64_t sw, int64_t sc, void *stream);
/* The same pair with the K axis ordered (kh, kw, cin) - col[(b,ho,wo), (kh*KW+kw)*C + cin] - for inputs whose channels
 * are contiguous (sc == 1, C % 4 == 0, sb / sh / sw multiples of 4, 16-byte aligned pointers; ASRK_ESHAPE otherwise):
 * both become strided copies in whole 16-byte pieces.  The GEMM then multiplies against the weight re-ordered by
 * asrk_conv_weight_reorder_f32 (weight.view(Cout, Cin, KH*KW) -> [Cout][KH*KW][Cin]; inverse != 0: back, for dW). */
int asrk_im2col_cl_f32(const float *x, float *col, int B, int H, int W, int C, int KH, int KW, int SH, int SW,
                       int PH, int PW, int64_t sb, int64_t sh, int64_t sw, int64_t sc, void *stream);
int asrk_col2im_cl_f32(const float *dcol, float *dx, int B, int H, int W, int C, int KH, int KW, int SH,
                       int SW, int PH, int PW, int64_t sb, int64_t sh, int64_t sw, int64_t sc, void *stream);
int asrk_conv_weight_reorder_f32(const float *src, float *dst, int Cout, int Cin, int KK, int inverse, void *stream);
/* 3x3 / stride 1 / pad 1 convolutions WITHOUT a patch matrix (the VGG prenet's layers with 64 or 128 input channels,
 * src/module.py:21-33: Conv2d(64,64,3,padding=1), Conv2d(64,128,...), Conv2d(128,128,...)): implicit GEMMs on the f32-input
 * matrix cores over contiguous channels-last activations x [B,H,W,C] -> y [B,H,W,Cout].  Same arithmetic as im2col +
 * asrk_gemm_f32 (exact f32 products, f32 accumulation; the summation order differs).
 *   asrk_conv3x3_supported: 1 when the shape has a kernel (C, Cout in {64, 128}, W <= 128), else 0 - callers keep the
 *       im2col path for everything else (the first layer, the CNN prenet).
 *   asrk_conv3x3_weight_f32: the parameter w[Cout][Cin][3][3] in the kernels' fragment order (9*Cin*Cout floats).
 *       transpose == 0: the forward weight; != 0: the data gradient's (cin <-> cout, taps flipped).
 *   asrk_conv3x3_f32: y = conv(x where xmask > 0, wf) + bias, optionally max(., 0).  xmask (shape of x) and bias may be
 *       NULL.  The data gradient is this entry on dy: x = dy, xmask = the layer's ReLU output (or NULL), wf = the
 *       transposed weight, C = the layer's Cout, Cout = the layer's Cin, no bias, no ReLU.
 *   asrk_conv3x3_wgrad_f32: dw[Cout][Cin][3][3] (parameter layout) = sum over positions of (dy where ymask > 0) x patches
 *       of x; db[Cout] = column sums of the same masked dy.  Either output may be NULL; ymask may be NULL.  Deterministic
 *       (per-workgroup partial sums in `ws`, added in a fixed order).  ws: asrk_conv3x3_wgrad_ws_bytes bytes, 16-byte
 *       aligned (ASRK_EWORKSPACE if smaller).
 * ASRK_ESHAPE: unsupported shape or a pointer that is not 16-byte aligned. */
int asrk_conv3x3_supported(int H, int W, int C, int Cout);
/* What the 3x3 launches do for a shape, from the planners the launches themselves use; host only (no device call, runs
 * without a GPU; tests/test_conv_plan_cpu.py holds the convolution case table to it).
 * kind: 0 asrk_conv3x3_f32 / _len_f32 (forward; the data gradient is kind 0 with C and Cout exchanged),
 *       1 asrk_conv3x3_wgrad_f32, 2 asrk_conv3x3_first_f32 / _first_len_f32, 3 asrk_conv3x3_first_wgrad_f32.
 * ASRK_EINVAL: out == NULL, n < ASRK_CONV3X3_PLAN_INFO_LEN, kind outside 0..3, B < 0 or a size <= 0 (as the launches);
 * out[0..n) is zeroed first whenever out and n are valid.  Otherwise ASRK_OK and
 *   [0] supported: what asrk_conv3x3_supported / asrk_conv3x3_first_supported and the launches' own size limits say;
 *       0 leaves every other field 0 (the callers keep the im2col route)
 *   [1] TH: the most image rows one tile can touch   [2] tiles per image   [3] tiles in all (B x [2])
 *   [4] workgroups (grid x)   [5] grid y (kind 1: Cin/64 x Cout/64 splits; kinds 2, 3: 64-column blocks; kind 0: 1)
 *   [6] the most and [7] the fewest tiles any workgroup walks (1 and 1 for the forward kinds)
 *   [8] dynamic LDS bytes   [9] workspace bytes (= the *_wgrad_ws_bytes functions; 0 for the forward kinds; INT_MAX if larger)
 *   [10] kind 1: thmax, the largest TH the LDS budget allows - the cost model chose a smaller one where [1] < [10];
 *        other kinds: [1]
 * B == 0 launches nothing: [4..7] and [9] are 0. */
#define ASRK_CONV3X3_PLAN_INFO_LEN 12
int asrk_conv3x3_plan_info(int kind, int B, int H, int W, int C, int Cout, int *out, int n);
int asrk_conv3x3_weight_f32(const float *w, float *wf, int Cout, int Cin, int transpose, void *stream);
int asrk_conv3x3_f32(const float *x, const float *xmask, const float *wf, const float *bias, float *y, int B, int H, int W,
                     int C, int Cout, int relu, void *stream);
size_t asrk_conv3x3_wgrad_ws_bytes(int B, int H, int W, int C, int Cout);
int asrk_conv3x3_wgrad_f32(const float *x, const float *dy, const float *ymask, float *dw, float *db, int B, int H, int W,
                           int C, int Cout, void *ws, size_t ws_bytes, void *stream);
/* The FIRST VGG layer (Conv2d(in_channel, 64, 3, padding=1), in_channel = 1..3 delta-feature planes, src/module.py:21;
 * view_input, 44-57, is folded into the element strides: x[b*sb + h*sh + w*sw + c*sc]): 9*C <= 27 fits one MFMA tile, so
 * forward = one kernel (bias and ReLU fused) writing y [B,H,W,Cout], and the weight + bias gradients = one kernel over dy
 * (gated by ymask > 0 when given) plus a fixed-order reduction of per-workgroup partial sums in `ws`
 * (asrk_conv3x3_first_wgrad_ws_bytes bytes, 16-byte aligned).  w / dw: the parameter's [Cout][C][3][3] layout.
 * C <= 3, Cout a multiple of 64, W <= 128 (asrk_conv3x3_first_supported; ASRK_ESHAPE otherwise).  The gradient with
 * respect to the features is not part of this pair (callers that need it keep the im2col path for that one product). */
int asrk_conv3x3_first_supported(int H, int W, int C, int Cout);
int asrk_conv3x3_first_f32(const float *x, const float *w, const float *bias, float *y, int B, int H, int W, int C, int Cout,
                           int64_t sb, int64_t sh, int64_t sw, int64_t sc, int relu, void *stream);
size_t asrk_conv3x3_first_wgrad_ws_bytes(int B, int H, int W, int C, int Cout);
int asrk_conv3x3_first_wgrad_f32(const float *x, const float *dy, const float *ymask, float *dw, float *db, int B, int H,
                                 int W, int C, int Cout, int64_t sb, int64_t sh, int64_t sw, int64_t sc, void *ws,
                                 size_t ws_bytes, void *stream);
/* Length-aware FORWARD entries (inference over a zero- or garbage-padded batch: several utterances encoded together,
 * each as if it were alone).  hlen: B int64 values on the DEVICE (the convention of asrk_lstm_rec_fwd_len_f32's `lens`),
 * read by the kernels - no host synchronisation.  Image b is Hv = min(H, max(0, hlen[b])) rows high:
 *   - an input element (b, h, w) counts only if 0 <= h < Hv; every other one reads as exactly 0 (a select - the rows
 *     beyond Hv may hold anything, NaN included), so the row h = Hv is the zero padding a batch-1 run of that image sees;
 *   - asrk_conv3x3_len_f32 / asrk_conv3x3_first_len_f32 (same shapes, layouts and support predicates as
 *     asrk_conv3x3_f32 without xmask / asrk_conv3x3_first_f32; y 16-byte aligned) write output rows h >= Hv as exactly 0
 *     (no bias, no ReLU of it), and a workgroup whose whole tile lies there writes its zeros without staging its halo or
 *     issuing an MFMA: the padded tail of a batch costs a store.  Every valid output element is summed in the order of
 *     the plain entries, which depends on neither the tile position nor B: bit-identical to the batch-1 result;
 *   - asrk_im2col_ld_len_f32 / asrk_im2col_cl_len_f32 (arguments of asrk_im2col_ld_f32 / asrk_im2col_cl_f32 plus hlen)
 *     gather with the same select; patch rows whose output row lies beyond the image's own output extent are whatever
 *     that yields (bias after the GEMM) - asrk_conv_zero_tail_f32 clears them;
 *   - asrk_conv_zero_tail_f32: y [B, H, row] contiguous, y[b, h, :] = 0 for h >= hlen[b].
 * ASRK_EINVAL for a NULL hlen or any other NULL pointer, ASRK_ESHAPE as the plain entries.  No backward. */
int asrk_conv3x3_len_f32(const float *x, const float *wf, const float *bias, float *y, const int64_t *hlen, int B, int H,
                         int W, int C, int Cout, int relu, void *stream);
int asrk_conv3x3_first_len_f32(const float *x, const float *w, const float *bias, float *y, const int64_t *hlen, int B, int H,
                               int W, int C, int Cout, int64_t sb, int64_t sh, int64_t sw, int64_t sc, int relu,
                               void *stream);
int asrk_im2col_ld_len_f32(const float *x, float *col, const int64_t *hlen, int ldcol, int B, int H, int W, int C, int KH,
                           int KW, int SH, int SW, int PH, int PW, int64_t sb, int64_t sh, int64_t sw, int64_t sc,
                           void *stream);
int asrk_im2col_cl_len_f32(const float *x, float *col, const int64_t *hlen, int B, int H, int W, int C, int KH, int KW,
                           int SH, int SW, int PH, int PW, int64_t sb, int64_t sh, int64_t sw, int64_t sc, void *stream);
int asrk_conv_zero_tail_f32(float *y, const int64_t *hlen, int B, int H, int64_t row, void *stream);
int asrk_relu_fwd_f32(float *x, int64_t n, void *stream);
int asrk_relu_bwd_f32(const float *y, const float *dy, float *dx, int64_t n, void *stream);
int asrk_maxpool2x2_fwd_f32(const float *x, float *y, uint8_t *idx, int B, int H, int W, int C,
                            int64_t osb, int64_t osh, int64_t osw, int64_t osc, void *stream);
int asrk_maxpool2x2_bwd_f32(const float *dy, const uint8_t *idx, float *dx, int B, int H, int W, int C,
                            int64_t osb, int64_t osh, int64_t osw, int64_t osc, void *stream);

/* ---- fused optimiser updates (src/solver.py:76-91: clip_grad_norm_ + torch.optim step) --------
 * One streaming pass per parameter tensor (n elements).  clip_coef: DEVICE scalar holding
 * max_norm / (total_norm + 1e-6) (clamped to <= 1 inside), or NULL for no clipping; the gradient is
 * read-only (the clipped gradient is never written back).
 * adadelta: torch.optim.Adadelta(lr, rho, eps, weight_decay=0) state (square_avg, acc_delta).
 * adam:     torch.optim.Adam(lr, betas, eps, weight_decay=0, amsgrad=False) state (exp_avg,
 *           exp_avg_sq); `step` is the 1-based step count used for the bias corrections.
 * Hyper-parameters are doubles (as Python floats): 1-rho, 1-beta and the bias corrections are formed
 * in double before rounding to f32, as torch does. */
int asrk_adadelta_step_f32(float *param, const float *grad, float *square_avg, float *acc_delta,
                           int64_t n, double lr, double rho, double eps, const float *clip_coef,
                           void *stream);
int asrk_adam_step_f32(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n,
                       double lr, double beta1, double beta2, double eps, int64_t step,
                       const float *clip_coef, void *stream);
/* Multi-tensor forms: `count` parameter tensors in one call (HOST arrays of device pointers and
 * element counts; one kernel launch per 24 tensors, the table travels in the kernel arguments).
 * Element-wise identical to the single-tensor calls above; all tensors share the hyper-parameters
 * (one torch param_group) and, for adam, the step count. */
int asrk_adadelta_multi_f32(int count, float *const *params, const float *const *grads,
                            float *const *square_avg, float *const *acc_delta, const int64_t *numel,
                            double lr, double rho, double eps, const float *clip_coef, void *stream);
int asrk_adam_multi_f32(int count, float *const *params, const float *const *grads,
                        float *const *exp_avg, float *const *exp_avg_sq, const int64_t *numel,
                        double lr, double beta1, double beta2, double eps, int64_t step,
                        const float *clip_coef, void *stream);
/* Extended multi-tensor forms: the step above plus weight decay and a running average of the weights in the same
 * pass.  weight_decay: HOST array [count] of per-tensor lambda_t >= 0, or NULL (no decay).  decay_mode 0 ignores it;
 * 1 = L2 as torch.optim.Adadelta / Adam(weight_decay=) define it (g' = min(coef, 1) * g + lambda_t * p, the decay
 * added after clipping); 2 = decoupled as torch.optim.AdamW (p *= 1 - lr * lambda_t before the update, lr the call's
 * learning rate; adam only).  avg: HOST array [count] of device pointers e_t or NULL; a NULL entry is a tensor without
 * an average.  After the new p is stored: e += avg_weight * (p - e), avg_weight in [0, 1].  A NaN clip_coef leaves p,
 * both states and e untouched.  With decay_mode 0 (or lambda_t = 0 everywhere) and no average the result is the plain
 * call's bit for bit.
 * asrk_avg_multi_f32: the same e update as a launch of its own (optimisers that are not fused), the same bits and the
 * same NaN skip.  asrk_swap_multi_f32: exchange the tensors of two lists in place, one launch per 24 tensors.
 * ASRK_EINVAL before any device call: count or numel < 0, NULL table, NULL pointer of a non-empty tensor (avg entries
 * of the step calls excepted), lambda_t < 0 or not finite, avg_weight outside [0, 1] or not finite, decay_mode outside
 * 0..2, decay_mode 2 with adadelta. */
int asrk_adadelta_multi_ext_f32(int count, float *const *params, const float *const *grads,
                                float *const *square_avg, float *const *acc_delta, const int64_t *numel,
                                double lr, double rho, double eps, const float *clip_coef,
                                const float *weight_decay, int decay_mode, float *const *avg, double avg_weight,
                                void *stream);
int asrk_adam_multi_ext_f32(int count, float *const *params, const float *const *grads, float *const *exp_avg,
                            float *const *exp_avg_sq, const int64_t *numel, double lr, double beta1, double beta2,
                            double eps, int64_t step, const float *clip_coef, const float *weight_decay,
                            int decay_mode, float *const *avg, double avg_weight, void *stream);
int asrk_avg_multi_f32(int count, float *const *avg, const float *const *params, const int64_t *numel,
                       double avg_weight, const float *clip_coef, void *stream);
int asrk_swap_multi_f32(int count, float *const *a, float *const *b, const int64_t *numel, void *stream);

/* Global 2-norm of a list of gradient tensors and the clipping coefficient of clip_grad_norm_(params, max_norm)
 * (src/solver.py:84): norm_out[0] = sqrt(sum_t sum_i g_t[i]^2), coef_out[0] = max_norm / (norm + 1e-6) (either may be
 * NULL), both on the device so that nothing is read back before the optimiser step.  Two deterministic stages
 * (per-block partial sums, one block adds them in a fixed order): bit-reproducible.  ws: asrk_grad_norm_ws_bytes
 * bytes of device scratch, 8-byte aligned.  asrk_fill_f32: x[0:n] = value. */
size_t asrk_grad_norm_ws_bytes(int count, const int64_t *numel);
int asrk_grad_norm_multi_f32(int count, const float *const *grads, const int64_t *numel, float max_norm,
                             float *norm_out, float *coef_out, void *ws, size_t ws_bytes, void *stream);
int asrk_fill_f32(float *x, int64_t n, float value, void *stream);

/* ---- audio front end (src/audio.py:7-133; fbank = torchaudio.compliance.kaldi.fbank) ------
 * frames:  wave [n_samples] f32 -> frames [m, ldf]: snip_edges framing (frame i = samples
 *          [i*shift, i*shift+win)), optional per-frame DC removal, pre-emphasis with replicate
 *          padding, multiplication by `window` [win] (povey); columns >= win are zero.
 * The spectrum is frames x (cos|sin basis) through asrk_gemm_f32; power: spec [m, 2*nb] = [re|im]
 * -> power [m, nb]; mel energies = power x melT through asrk_gemm_f32; log_floor: x =
 * log(max(x, eps)) in place.
 * delta:   x [D,T] -> y [C,D,T], y[c,d,t] = sum_j filters[c,j] * x[d, t+j-(L-1)/2], zero padded
 *          (src/audio.py:48-54; L odd).  cmvn: rows [R,T] -> (x-mean)/(eps+std_unbiased) over T
 *          (src/audio.py:24-27).  transpose: [rows, cols] -> [cols, rows] (Postprocess 85-89). */
int asrk_fbank_frames_f32(const float *wave, int64_t n_samples, const float *window, float *frames,
                          int m, int win, int shift, int ldf, float preemph, int remove_dc,
                          void *stream);
int asrk_power_spectrum_f32(const float *spec, float *power, int64_t m, int nb, void *stream);
int asrk_log_floor_f32(float *x, int64_t n, float eps, void *stream);
int asrk_delta_f32(const float *x, const float *filters, float *y, int C, int D, int T, int L,
                   void *stream);
int asrk_cmvn_f32(const float *x, float *y, int rows, int T, float eps, void *stream);
int asrk_transpose_f32(const float *x, float *y, int rows, int cols, void *stream);
/* The same front end for a whole padded batch (collate: src/data.py:14-43 extracts one file at a time in
 * DataLoader workers and pads afterwards; here the padded PCM of the batch is the input):
 * frames_batch: wave [B, ld_wave] of int16 PCM (sample_bytes 2; scale = 1/32768 reproduces torchaudio.load's
 *          float conversion exactly) or f32 (sample_bytes 4); utterance b owns rows frame_off[b] ..
 *          frame_off[b+1] of frames [total_m, ldf] (frame_off [B+1] int64 on the device, max_m = the longest
 *          utterance's frame count; n_samples_host: optional HOST array [B] checked against ld_wave).
 *          The spectrum / mel / log steps then run once over all total_m rows.
 * delta_cmvn_batch: mel [total_m, D] -> out [B, Tmax, C*D], zero beyond each utterance's frames:
 *          Delta (C = order + 1 filters of L <= 16 odd taps, zero padded at the utterance edges), CMVN over the
 *          utterance's own frames (apply_cmvn != 0; unbiased std, eps added to std), Postprocess's
 *          [T, c*D + d] layout and pad_sequence's zero padding in one kernel. */
int asrk_fbank_frames_batch_f32(const void *wave, int sample_bytes, int64_t ld_wave, const int64_t *n_samples_host,
                                const int64_t *frame_off, int B, int max_m, const float *window, float *frames,
                                int win, int shift, int ldf, float scale, float preemph, int remove_dc,
                                void *stream);
int asrk_delta_cmvn_batch_f32(const float *mel, const int64_t *frame_off, int B, int D, const float *filters, int C,
                              int L, int apply_cmvn, float eps, float *out, int Tmax, void *stream);
/* asrk_fbank_logmel_batch_f32 (round 6): torchaudio.compliance.kaldi.fbank for a whole padded PCM batch in ONE kernel
 * (reference call site src/audio.py:104-108): frame f of utterance b -> row frame_off[b] + f of mel [sum m, nmel] =
 * log(max(mel energies, eps)).  One wave per frame: framing exactly as asrk_fbank_frames_batch_f32 (same arguments),
 * the zero-padded 2^log2n-point real DFT as a 2^(log2n-1)-point complex FFT in LDS, power spectrum, triangular mel
 * weights.  Tables are the caller's: window [win]; tw_fft [2^(log2n-1)] (re, im) pairs of e^{-2 pi i k / 2^(log2n-1)};
 * tw_unpack [2^(log2n-1) + 1] pairs of e^{-2 pi i k / 2^log2n}; melT [>= 2^(log2n-1) + 1 rows][ld_mel] the dense mel
 * weights (row = FFT bin); mel_range [nmel][2] (int32) = first / one-past-last FFT bin with a non-zero weight.
 * log2n in 8..11 and win <= 2^log2n, else ASRK_ESHAPE. */
int asrk_fbank_logmel_batch_f32(const void *wave, int sample_bytes, int64_t ld_wave, const int64_t *n_samples_host,
                                const int64_t *frame_off, int B, int max_m, const float *window, const float *tw_fft,
                                const float *tw_unpack, const float *melT, const int *mel_range, int nmel, int ld_mel,
                                float *mel, int win, int shift, int log2n, float scale, float preemph, int remove_dc,
                                float eps, void *stream);

/* ---- Dither (the reference's `audio.dither` key, forwarded to torchaudio.compliance.kaldi.fbank / mfcc, whose
 * _get_window adds randn(strided_input.shape) * dither to the strided frame matrix BEFORE DC removal) ------------------
 * The three framing entries above, with x replaced by
 *     v[f][j] = x[f*shift + j] + dither * z(key, f, j),        f = frame within the utterance, j = 0..win-1,
 * x the sample after `scale`; product and sum are two f32 operations (not fused).  Everything behind is the plain
 * entry's arithmetic on v: mean over the frame, pre-emphasis with the replicated v[f][0], window, ...  The noise is per
 * (frame, position), not per waveform sample: two overlapping frames see different noise on one sample.  `dither` is in
 * the units of the [-1, 1) waveform: 1/32768 = 3.05e-5 is Kaldi's int16-scale default of 1.0.
 * z is a pure function, the same in every batch composition, launch and run:
 *     (r0, r1, r2, r3) = Philox4x32-10(counter words (j >> 2, f, 0, 0), key words (key & 0xffffffff, key >> 32))
 *     u1 = ((r0 >> 8) + 1) * 2^-24,  u2 = (r1 >> 8) * 2^-24      (u1 in (0, 1], u2 in [0, 1), exact in f32)
 *     z0 = sqrt(-2 ln u1) * cos(2 pi u2),  z1 = sqrt(-2 ln u1) * sin(2 pi u2);   z2, z3 likewise from r2, r3
 *     z(key, f, j) = z[j & 3];   |z| <= sqrt(48 ln 2) = 5.77
 * evaluated in f32 with the accurate logf / sqrtf / sincospif (tests/dither_reference.py restates it in float64).
 * key: one per utterance; the per-file entry takes it by value, the batch entries as keys [B] (uint64, DEVICE).
 * Arguments, results and refusals are the plain entries'; in addition ASRK_EINVAL for a negative or non-finite dither
 * (checked with the sizes) and for keys == NULL (checked with the other pointers).  dither = 0 is taken: v = x. */
int asrk_fbank_frames_dither_f32(const float *wave, int64_t n_samples, const float *window, float *frames, int m,
                                 int win, int shift, int ldf, float preemph, int remove_dc, float dither, uint64_t key,
                                 void *stream);
int asrk_fbank_frames_batch_dither_f32(const void *wave, int sample_bytes, int64_t ld_wave,
                                       const int64_t *n_samples_host, const int64_t *frame_off, int B, int max_m,
                                       const float *window, float *frames, int win, int shift, int ldf, float scale,
                                       float preemph, int remove_dc, float dither, const uint64_t *keys, void *stream);
int asrk_fbank_logmel_batch_dither_f32(const void *wave, int sample_bytes, int64_t ld_wave,
                                       const int64_t *n_samples_host, const int64_t *frame_off, int B, int max_m,
                                       const float *window, const float *tw_fft, const float *tw_unpack,
                                       const float *melT, const int *mel_range, int nmel, int ld_mel, float *mel,
                                       int win, int shift, int log2n, float scale, float preemph, int remove_dc,
                                       float eps, float dither, const uint64_t *keys, void *stream);

/* ---- SpecAugment on the padded feature batch (training input augmentation; the reference keeps the SpecAugment
 * learning-rate schedules, src/optim.py:65-82, and augments nothing: the call sits between fetch_data and the model
 * call of bin/train_asr.py:99-105) -----------------------------------------------------------------------------------
 * x, y [B, T, ld] (x != y), ld >= C*D; column c*D + d = mel bin d of channel c (static / delta / delta-delta: the
 * layout of Postprocess and asrk_delta_cmvn_batch_f32).  lens [B] int64 (device): n = valid frames of utterance b
 * (clamped to 0..T).  params [B, P] int32 (device), P = 2 + 2*n_fmask + 2*n_tmask, row = c, w, f0_0, fw_0, ..,
 * t0_0, tw_0, ..  (sampled on the host: src/audio.py SpecAugment.sample).
 * Output frame t < n.  Time warp, active only when w != 0, 0 < c < n-1 and 0 < d = c+w < n-1 (else source = frame t):
 *     t <= d: num = t*c, den = d;   t > d: num = c*(n-1-d) + (t-d)*(n-1-c), den = n-1-d   (64-bit integers)
 *     i = num / den, r = num % den, j = min(i+1, n-1), a = (float)r / (float)den,
 *     y[t] = (1-a)*x[i] + a*x[j], and y[t] = x[i] bit for bit when r == 0.
 * The map is increasing, fixes frames 0 and n-1 and sends d to c; i and j are clamped to 0..n-1 whatever the row holds.
 * Masks, after the warp, in output coordinates: mel bin d in any [f0_k, f0_k+fw_k) -> `fill` in every channel; frame t
 * in any [t0_k, t0_k+tw_k) (t < n) -> `fill` in all C*D columns; zero or negative widths mask nothing.
 * Frames t >= n are copied from x unchanged; columns >= C*D of y are not written.  One launch, no atomics.
 * ASRK_ESHAPE: a negative size, ld < C*D, C*D > 16384, n_fmask / n_tmask outside 0..8, x == y, a NULL pointer with
 * B*T > 0 (all checked before any device call); B*T == 0 returns 0 without a launch. */
int asrk_spec_augment_f32(const float *x, float *y, int B, int T, int ld, int D, int C, const int64_t *lens,
                          const int32_t *params, int n_fmask, int n_tmask, float fill, void *stream);

/* ---- Speed perturbation on the padded PCM batch (training input augmentation; sits between the PCM upload and
 * asrk_fbank_*_batch_f32, which then take y with sample_bytes = 4, scale = 1) ------------------------------------------
 * x [B, ld_in] of int16 (sample_bytes 2) or f32 (sample_bytes 4), `scale` as in asrk_fbank_frames_batch_f32; row b
 * holds n[b] samples.  y [B, ld_out] f32 (x != y).  ratios_host [n_ratios][2] int32 (HOST) = (orig, new), coprime
 * positive integers; row b uses ratio ratio_idx[b].  Speed = orig / new: the row is taken as sampled at orig/new times
 * the rate and converted to the rate (torchaudio's sinc_interp_hann resampler, lowpass_filter_width W = 6, rolloff 0.99):
 *     base = min(orig, new) * 0.99, width = ceil(W * orig / base) taken exactly = ceil(100 W orig / (99 min(orig, new))),
 *     taps = 2*width + orig;  table h [new][taps] f32 (device; the caller builds it in float64 and rounds once):
 *     t = clamp((-j/new + (k - width)/orig) * base, -W, W),  h[j][k] = sinc(pi t) * cos^2(pi t / (2W)) * base/orig;
 *     n_out = (new*n + orig - 1) / orig  (integers);  for o = i*new + j < n_out:
 *     y[o] = sum_k h[j][k] * (x[i*orig + k - width] * scale),  x = 0 outside 0..n-1,
 *     accumulated in f32 with fused multiply-adds in ascending k, starting from 0.
 * Ratio (1, 1) is not filtered: y[o] = x[o] * scale bit for bit (its table pointer is not read and may be NULL).
 * taps_host [n_ratios] (HOST) holds the DEVICE pointers of the tables.  Columns o >= n_out[b] of y are not written.
 * n and ratio_idx are passed twice: the HOST arrays are checked and size the launch; the DEVICE copies are what the
 * kernel reads (clamped there to the buffers: a copy that disagrees cannot make it leave x or y).  One launch, no atomics;
 * 16-byte stores when y is 16-byte aligned and ld_out is a multiple of 4, element stores otherwise.
 * Limits: orig, new <= 100 and 1/2 <= orig/new <= 2 (speeds with two decimals in [0.5, 2.0]); n_ratios <= 8.
 * ASRK_ESHAPE, all checked before any device call: a negative size, sample_bytes not 2 or 4, x == y, n_ratios > 8, a
 * ratio outside the limits or not coprime, n[b] outside 0..ld_in, ratio_idx[b] outside 0..n_ratios-1, ld_out < n_out[b],
 * a NULL pointer with work to do (any host array with B > 0; x, y, a device copy or a used table with an output sample
 * to compute).  B == 0, or no output sample at all, returns 0 without a launch. */
int asrk_resample_rows_f32(const void *x, int sample_bytes, int64_t ld_in, const int64_t *n_host, const int64_t *n_dev,
                           const int32_t *ratio_idx_host, const int32_t *ratio_idx_dev, int B,
                           const int32_t *ratios_host, const float *const *taps_host, int n_ratios, float *y,
                           int64_t ld_out, float scale, void *stream);

/* ---- Reverberation and additive noise on the padded PCM batch (training input augmentation; sits behind
 * asrk_resample_rows_f32 and in front of asrk_fbank_*_batch_f32, which then take out with sample_bytes = 4, scale = 1) ---
 * x [B, ld_in] of int16 (sample_bytes 2) or f32 (sample_bytes 4), `scale` as in asrk_resample_rows_f32; row b holds n[b]
 * samples: s[i] = x[b][i] * scale (one f32 rounding), s = 0 outside 0..n-1.  out [B, ld_out] f32.
 * Impulse responses: rir [R, ld_r] f32 (device); response r has rir_len[r] = K taps, 1 <= K <= 8192, and
 * rir_peak[r] = p, the first index of its largest |h| (the caller finds it).  rir_idx[b] in -1..R-1; -1 = no response,
 * then y[i] = s[i] bit for bit; otherwise, for 0 <= i < n,
 *     y[i] = sum_{k < K} h[k] * s[i + p - k]         (f32, fused multiply-adds in DESCENDING k, starting from 0):
 * the direct sound stays where it was and the row keeps its length.
 * Level: Ps = sum s[i]^2, Py = sum y[i]^2, Pv = sum v_i^2, each over i < n, each square and sum in float64 (of the f32
 * values), through one partial per tile of 2048 samples in ws, added in tile order.  a = sqrt(Ps / Py) when
 * rir_idx[b] >= 0 and Py > 0, else 1.
 * Noise: v [B, ld_v], sample type and scale of x; row b holds m[b] samples, v_i = v[b][i mod m[b]] * scale (tiled
 * circularly); m[b] == 0 = no noise.  snr_lin [B] f32 (device) = 10^(snr_dB / 10).  g = sqrt(Ps / (Pv * snr_lin)) when
 * m > 0, Pv > 0, Ps > 0 and snr_lin is positive and finite, else 0.  a and g are computed in float64, rounded to f32
 * (and kept at or under FLT_MAX).
 *     out[b][i] = a * y[i] + g * v_i   for i < n   (f32: two products, one sum; no noise term when g == 0).
 * Columns i >= n[b] of out are not written.  A row with neither a response nor noise is s bit for bit; a silent row
 * stays exactly zero; no input of finite samples gives NaN or Inf.  A row's bits depend on that row alone (not on B,
 * not on the other rows, not on ld_out), and two calls give the same bits: no atomics.
 * n, m, rir_idx, rir_len and rir_peak are passed twice: the HOST arrays are checked and size the launch; the DEVICE
 * copies are what the kernels read (clamped there to the buffers: a copy that disagrees cannot make them leave x, v, rir
 * or out).  Two launches (convolution + partial sums; scale + mix), one when no row has a response or noise.
 * ws: caller-owned device memory, 8-byte aligned, at least asrk_reverb_mix_ws_bytes(B, max_b n[b]) bytes
 * (ASRK_EWORKSPACE if NULL or smaller), private to the call until the stream has passed it.
 * ASRK_ESHAPE, all checked before any device call: a negative size, a leading dimension above 2^31 - 1, sample_bytes not
 * 2 or 4, rir_len[r] outside 1..min(8192, ld_r), rir_peak[r] outside 0..rir_len[r]-1, rir_idx[b] outside -1..R-1,
 * n[b] outside 0..min(ld_in, ld_out), m[b] outside 0..ld_v, out overlapping x or v, a misaligned ws, a NULL pointer with
 * work to do (any host array it has to read; x, out, the device copies with a sample to compute; rir and its arrays
 * with a response in use; v and snr_lin with noise in use).  B == 0, or no sample at all, returns 0 without a launch. */
size_t asrk_reverb_mix_ws_bytes(int B, int64_t n_max);
int asrk_reverb_mix_f32(const void *x, int sample_bytes, int64_t ld_in, const int64_t *n_host, const int64_t *n_dev,
                        const float *rir, int64_t ld_r, const int32_t *rir_len_host, const int32_t *rir_len_dev,
                        const int32_t *rir_peak_host, const int32_t *rir_peak_dev, int R, const int32_t *rir_idx_host,
                        const int32_t *rir_idx_dev, const void *v, int64_t ld_v, const int64_t *m_host,
                        const int64_t *m_dev, const float *snr_lin_dev, int B, float *out, int64_t ld_out, float scale,
                        void *ws, size_t ws_bytes, void *stream);

/* ---- CTC loss (bin/train_asr.py:49,123-124 -> torch.nn.CTCLoss(blank=0)) ---------------
 * log_probs element (t,b,c) at lp[t*stride_t + b*stride_b + c]; targets [B,L] int64 (row stride
 * tgt_stride) zero-padded; input_lengths/target_lengths int64 [B].
 * alpha/beta: [B, T, S] scratch/saved, S = 2*Lmax+1; nll: [B] per-utterance -log p.
 * The scalar reduction (mean over b of nll/len) is done by the caller (host glue). */
int asrk_ctc_loss_fwd_f32(const float *lp, int64_t stride_t, int64_t stride_b, int T, int B,
                          int V, const int64_t *targets, int64_t tgt_stride, int Lmax,
                          const int64_t *input_lengths, const int64_t *target_lengths,
                          int blank, float *alpha, float *beta, float *lpg, float *nll,
                          void *stream);
/* fwd also needs lpg [B, T, S] (scratch: the gathered log-probs lp[t,b,ext_b[s]]) and, when `beta`
 * is non-NULL, computes the beta lattice concurrently with alpha (training: pass it, then bwd is
 * only the gradient assembly; inference: NULL).
 * grad[t,b,c] = (exp(lp) - exp(logsum_{s:ext[s]=c}(alpha+beta) + nll_b - lp)) * gscale[b]
 * for t < input_length[b], else 0  (== ATen ctc_loss backward; gscale folds grad_out and the
 * 'mean' normaliser).  grad uses the same (stride_t, stride_b) addressing as given. */
int asrk_ctc_loss_bwd_f32(const float *lp, int64_t stride_t, int64_t stride_b, int T, int B,
                          int V, const int64_t *targets, int64_t tgt_stride, int Lmax,
                          const int64_t *input_lengths, const int64_t *target_lengths,
                          int blank, const float *alpha, const float *beta, const float *lpg,
                          const float *nll, const float *gscale, float *grad, int64_t g_stride_t,
                          int64_t g_stride_b, void *stream);

/* An utterance whose nll is NaN (a target outside [0,V), flagged by the forward without reading out of bounds) gets, from
 * both bwd entry points and with any flags: NaN in every gradient element of its frames t < input_length[b], 0 beyond,
 * and nothing written outside its own rows - its labels are never used as a column index.  The gradient norm of the
 * batch is then NaN, which is what a solver's non-finite-gradient guard tests.
 *
 * What the two loss calls launch for a shape, from the planner the launchers themselves use; host only (no device call,
 * runs without a GPU; tests/test_loss_plan_cpu.py holds the CTC case table of tests/loss_reference.py to it).
 * ASRK_EINVAL: info == NULL, n < ASRK_CTC_LOSS_PLAN_INFO_LEN or a negative size; ASRK_ESHAPE: Lmax > 1023 (as the
 * launches); info[0..n) is zeroed first whenever info and n are valid.  Otherwise ASRK_OK and
 *   [0] the lattice kernel's states-per-lane template: 4 (up to 256 states), 16 (up to 1024) or 32
 *   [1] its FAST flag: 1 = hardware exp / log (template 4 and T <= 512), 0 = library expf / logf
 *   [2] spl = ceil((2*Lmax+1) / 64), the states each lane holds
 *   [3] the gather grid's y = ceil(T / 8) (0: B == 0 or T == 0, no gather launch)
 *   [4] the gradient kernel's t_per_block (frames per workgroup, a multiple of 4) and [5] its chunk count (grid y);
 *       [4] x [5] >= T > [4] x ([5] - 1); both 0 where the backward launches nothing (B == 0 or T == 0)
 *   [6] the dense gradient grid = ceil(T*B / 4)   [7] 2*Lmax+1 */
#define ASRK_CTC_LOSS_PLAN_INFO_LEN 8
int asrk_ctc_loss_plan_info(int T, int B, int Lmax, int *info, int n);

/* The same two calls with flags; asrk_ctc_loss_{fwd,bwd}_f32 are these with flags = 0 (loss, n_infeasible NULL).
 * ASRK_CTC_ZERO_INFINITY = torch's zero_infinity=True.  An utterance whose targets have no path through its frames
 * has nll[b] = +inf, and nll keeps that value: it is the marker the backward tests.
 *   fwd: loss[b] ([B], may be NULL without the flag, required with it) = 0 for those utterances, nll[b] otherwise;
 *        *n_infeasible (device int32, may be NULL) = how many were zeroed (0 without the flag).
 *   bwd: every gradient element of those utterances is written as exactly 0, label columns included.
 * A NaN nll (targets outside [0,V)) stays NaN either way.  The caller's 'mean' still divides by all B utterances.
 * ASRK_EINVAL for unknown flag bits. */
#define ASRK_CTC_ZERO_INFINITY 1
int asrk_ctc_loss_fwd_ex_f32(const float *lp, int64_t stride_t, int64_t stride_b, int T, int B, int V,
                             const int64_t *targets, int64_t tgt_stride, int Lmax, const int64_t *input_lengths,
                             const int64_t *target_lengths, int blank, float *alpha, float *beta, float *lpg,
                             float *nll, int flags, float *loss, int32_t *n_infeasible, void *stream);
int asrk_ctc_loss_bwd_ex_f32(const float *lp, int64_t stride_t, int64_t stride_b, int T, int B, int V,
                             const int64_t *targets, int64_t tgt_stride, int Lmax, const int64_t *input_lengths,
                             const int64_t *target_lengths, int blank, const float *alpha, const float *beta,
                             const float *lpg, const float *nll, const float *gscale, float *grad,
                             int64_t g_stride_t, int64_t g_stride_b, int flags, void *stream);

/* ---- CTC forced alignment: the best (Viterbi) path of every utterance, found and traced back on the device ----------
 * lp / strides / targets / lengths / blank as asrk_ctc_loss_fwd_f32 (so a [B,T,V]-backed transposed view needs no
 * copy).  Over the blank-extended labels ext (S_b = 2*L_b + 1 states), frames t < T_b = min(input_lengths[b], T):
 *     delta_0[s] = lp_0[ext[s]] for s <= 1 (else -inf)
 *     delta_t[s] = max(delta_{t-1}[s], delta_{t-1}[s-1], delta_{t-1}[s-2] if s odd and ext[s] != ext[s-2]) + lp_t[ext[s]]
 * in plain f32 (compares and one add: a host f32 computation in this order gives the same bits).  Tie rule: among equal
 * maxima the smallest jump wins (a candidate replaces the best only if strictly greater, tried in the order s, s-1,
 * s-2); the path ends in state S_b-1 unless delta[S_b-2] is strictly greater.
 * Outputs (device): states [B,T] int32 = extended state of every frame; tokens [B,T] = ext[state] (blank or target
 * token); both -1 for t >= T_b.  spans [B,Lmax,2] = first frame and last frame + 1 of target token l, -1 for l >= L_b.
 * score [B] = delta of the final state = log-probability of the best path (0 for T_b <= 0 and L_b == 0).
 * An utterance without a path of non-zero probability (T_b < L_b + number of adjacent repeats, T_b <= 0 < L_b, or
 * -inf log-probs on every path) gets score -inf and -1 everywhere; a target outside [0,V) gives a NaN score (the
 * loss's convention; nothing is read out of bounds) and -1 everywhere.
 * `flags` (per call) picks where the 2-bit backpointers (jump 0..2 per state and frame) live until the backtrace, which
 * runs in the same launch (nothing returns to the host):
 *     ASRK_ALIGN_BP_LDS     in LDS, as bit planes: per frame 4*ceil((2*Lmax+1)/64) 32-bit words (2 bits per state,
 *                           states rounded up to whole 64-lane slots); needs T * that many words <= 128 KiB,
 *                           ASRK_ESHAPE otherwise
 *     ASRK_ALIGN_BP_GLOBAL  in the caller's workspace (any T)
 *     ASRK_ALIGN_BP_AUTO    LDS when it fits those 128 KiB, else the workspace - the default (0)
 * ws: caller-owned device memory, 16-byte aligned, at least asrk_ctc_align_ws_bytes(B, T, Lmax, flags) bytes (the
 * gathered log-probs [B,T,2*Lmax+1] and, on the global route, the backpointers), private to the call until the stream
 * has passed it; ASRK_EWORKSPACE if smaller.  asrk_ctc_align_ws_bytes returns 0 when the call needs no workspace
 * (B == 0 or T == 0) and for arguments the call rejects.
 * stamps: optional (NULL allowed) [B,4] int64, device wall-clock ticks of utterance b's wave at its start, after the
 * lattice, after the backtrace and at its end (for tools/ctc_align_bench.py).
 * ASRK_EINVAL: a NULL pointer, negative size, blank outside [0,V) or unknown flags; ASRK_ESHAPE: 2*Lmax+1 > 2048 or
 * a forced LDS route that does not fit - all checked before any device call.  One wave per utterance. */
#define ASRK_ALIGN_BP_AUTO 0
#define ASRK_ALIGN_BP_LDS 1
#define ASRK_ALIGN_BP_GLOBAL 2
size_t asrk_ctc_align_ws_bytes(int B, int T, int Lmax, int flags);
int asrk_ctc_align_f32(const float *lp, int64_t stride_t, int64_t stride_b, int T, int B, int V,
                       const int64_t *targets, int64_t tgt_stride, int Lmax, const int64_t *input_lengths,
                       const int64_t *target_lengths, int blank, int flags, int32_t *states, int32_t *tokens,
                       int32_t *spans, float *score, int64_t *stamps, void *ws, size_t ws_bytes, void *stream);

/* ---- second-pass scoring (n-best rescoring; csrc/rescore.hip).  The gradient: asrk_seq_logp_bwd_f32 below. ---------
 * Token and sequence log-probabilities from logits, without a [M,V] log_softmax tensor:
 *   x [M,V] f32, row stride ldx >= V; target [M] int64;
 *   tok_logp[m] = x[m, target[m]] - logsumexp(x[m, :])  (one pass over the row: running max and sum per lane,
 *   max-subtracted, f32), or x[m, target[m]] alone with ASRK_SEQ_LOGP_NORMALIZED (x already holds log-probabilities).
 *   target[m] < 0: the row is skipped - tok_logp[m] = 0 and the row is never read; target[m] >= V: NaN, nothing read.
 *   seq_logp[r] (float64, r < R) = sum of (double)tok_logp[m] for m in [seg_off[r], seg_off[r+1]) (seg_off [R+1] int64,
 *   clipped to [0, M]), added one after the other in ascending m: reproducible bit for bit; an empty segment gives 0.
 *   seg_off and seq_logp may both be NULL (no sums; R is ignored then).
 * Rows shorter than 2048 take one wave each (4 rows per workgroup), longer ones a 256-thread workgroup each; loads are
 * 16 bytes wide when x is 16-byte aligned and ldx % 4 == 0, scalar otherwise.  No float atomics.
 * ASRK_EINVAL, before any device call: a NULL pointer with M > 0, only one of seg_off / seq_logp, a negative size,
 * V <= 0, ldx < V, unknown flags.  M == 0 (and R == 0) is ASRK_OK without a launch. */
#define ASRK_SEQ_LOGP_NORMALIZED 1
int asrk_seq_logp_f32(const float *x, int64_t ldx, const int64_t *target, const int64_t *seg_off, int M, int V, int R,
                      int flags, float *tok_logp, double *seq_logp, void *stream);

/* asrk_seq_logp_f32 with one more output, lse[m] = logsumexp(x[m, :]) (f32 [M]; 0 for a skipped row, for
 * target[m] >= V and with ASRK_SEQ_LOGP_NORMALIZED): the same kernels and the same arithmetic, so tok_logp and seq_logp
 * equal asrk_seq_logp_f32's bit for bit.  lse NULL with M > 0 is ASRK_EINVAL. */
int asrk_seq_logp_lse_f32(const float *x, int64_t ldx, const int64_t *target, const int64_t *seg_off, int M, int V,
                          int R, int flags, float *tok_logp, float *lse, double *seq_logp, void *stream);

/* ---- minimum word error rate training (csrc/mwer.hip; src/mwer.py) --------------------------------------------------
 * Gradient of seq_logp with respect to the logits:
 *   dx[m, v] = w_m * (1[v == target[m]] - exp(x[m, v] - lse[m])),  w_m = (float)gseq[r] for the segment r with
 *   seg_off[r] <= m < seg_off[r+1] (seg_off [R+1] int64, non-decreasing; gseq [R] float64; lse [M] as
 *   asrk_seq_logp_lse_f32 wrote it).  A row with target < 0, and a row in no segment, gets a row of zeros WRITTEN (dx
 *   may be uninitialised memory) and is not read; a row with target >= V inside a segment (its forward value is NaN)
 *   gets a row of NaN, not read either.  dx has its own row stride lddx >= V; dx == x (in place,
 *   then lddx == ldx) is allowed: every element is read once, before it is written.  x is read once and dx written
 *   once; the case split is asrk_seq_logp_f32's (one wave per row below 2048 columns, a workgroup per row above; 16-byte
 *   accesses when x and dx are 16-byte aligned and both strides are multiples of 4).  No atomics.
 * ASRK_EINVAL, before any device call: a NULL pointer with M > 0 (seg_off / gseq only when R > 0), a negative size,
 * V <= 0, ldx < V, lddx < V, in place with lddx != ldx.  M == 0 is ASRK_OK without a launch. */
int asrk_seq_logp_bwd_f32(const float *x, int64_t ldx, const int64_t *target, const float *lse, const int64_t *seg_off,
                          const double *gseq, int M, int V, int R, float *dx, int64_t lddx, void *stream);

/* MWER loss of U utterances over n-best lists of at most N hypotheses: s [N,U] float64 scores and err [N,U] int32 error
 * counts, hypothesis n of utterance u at n*U + u; only n < count[u] is valid (count [U] int32, clipped to [0,N]).
 *   p = softmax over the valid scores (max-subtracted);  exp_err_u[u] = sum p e;  loss_u[u] = sum p (e - mean e);
 *   g[n,u] = d loss_u / d s[n,u] = p (e - exp_err_u[u]), 0 on invalid slots.  count[u] == 0: loss 0, g = 0.
 * All outputs float64; one wave per utterance, sums by a fixed butterfly: reproducible bit for bit.
 * ASRK_ESHAPE: N > 32; ASRK_EINVAL: a NULL pointer or a negative size; U == 0 is ASRK_OK without a launch. */
int asrk_mwer_loss_f64(const double *s, const int32_t *err, const int32_t *count, int N, int U, double *loss_u,
                       double *exp_err_u, double *g, void *stream);

/* CTC log-likelihood of R hypotheses against the posteriors of U utterances (usually U < R): row r scores
 * targets[r, :tgt_len[r]] against the mem_len[row_mem[r]] frames of utterance row_mem[r]; frame t of utterance u at
 * lp + u*stride_u + t*stride_t (log-probabilities, V per frame).  mem_len [U], row_mem [R], tgt_len [R], targets
 * [R, tgt_stride] are int64 device arrays; row_mem need not be sorted; frames >= mem_len[u] are never read (lengths are
 * clipped to [0, Tmax] and [0, Lmax]).
 *   score[r] = log p_ctc: -inf when the target does not fit the frames (or there is no frame and tgt_len > 0), the sum
 *   of the blank log-probabilities for tgt_len == 0 (0 without frames), NaN for a label outside [0,V) or a row_mem
 *   outside [0,U) - neither reads out of bounds.
 * Alpha only, one wave per row, no lattice is stored; the arithmetic is asrk_ctc_loss_fwd_f32's (hardware exp/log for
 * 2*Lmax+1 <= 256 and Tmax <= 512, the library functions beyond), so score[r] = -nll of the same row.
 * ws: caller-owned device memory, 16-byte aligned, at least asrk_ctc_score_rows_ws_bytes(R, Tmax, Lmax) bytes (the
 * gathered log-probs [R, Tmax, 2*Lmax+1]); the size function returns 0 for arguments without work or that the call
 * rejects.  ASRK_EINVAL, before any device call: a NULL pointer, a negative size or stride, tgt_stride < Lmax, blank
 * outside [0,V), a NULL / misaligned / short workspace; ASRK_ESHAPE: 2*Lmax+1 > 2048.  R == 0 is ASRK_OK. */
size_t asrk_ctc_score_rows_ws_bytes(int R, int Tmax, int Lmax);
int asrk_ctc_score_rows_f32(const float *lp, int64_t stride_u, int64_t stride_t, int U, int Tmax, int V,
                            const int64_t *mem_len, const int64_t *row_mem, const int64_t *targets, int64_t tgt_stride,
                            int Lmax, const int64_t *tgt_len, int R, int blank, float *score, void *ws, size_t ws_bytes,
                            void *stream);

/* ---- RNN-transducer head (csrc/rnnt.hip, csrc/rnnt.inc; src/transducer.py) --------------------------------------------
 * Shapes: B utterances, T encoder frames, U1 = U + 1 prediction rows (U = padded label count), V outputs, J joint
 * width.  Cell (b, t, u) is row (b*T + t)*U1 + u of every [B,T,U1,...] array.  enc_len, txt_len [B] and txt
 * [B, txt_stride] (txt_stride >= U; the labels y_1..y_U of utterance b are txt[b, 0..U_b-1]) are int64 device arrays;
 * the kernels clamp the lengths to 1 <= T_b <= T and 0 <= U_b <= U, so a bad length never indexes outside a buffer.
 * All values f32.  No float atomics: every result is a pure function of its inputs, reproducible bit for bit.
 * 16-byte accesses when every base is 16-byte aligned and every row stride (and J) is a multiple of 4, scalar otherwise.
 * ASRK_EINVAL, before any device call: a NULL pointer with B > 0, a negative size, T, U1, V or J <= 0, a row stride
 * below the row length, blank outside [0,V), txt_stride < U.  ASRK_ESHAPE: B*T*U1 > INT32_MAX.  B == 0: ASRK_OK.
 *
 * Joint network: H[b,t,u,:] = tanh(E[b,t,:] + P[b,u,:]); E [B,T,J] row stride lde, P [B,U1,J] row stride ldp,
 * H [B,T,U1,J] row stride ldh.  With t_idx (int32 [B], clamped to [0,T-1]) the decode form: H [B,U1,J] from frame
 * t_idx[b] of utterance b alone (U1 = 1 in the greedy search).  Call site: ops.RNNTJointFn, ops.rnnt_joint_step. */
int asrk_rnnt_joint_f32(const float *E, int64_t lde, const float *P, int64_t ldp, const int32_t *t_idx, int B, int T,
                        int U1, int J, float *H, int64_t ldh, void *stream);
/* dE[b,t,:] = sum_u dH[b,t,u,:] * (1 - H^2), dP[b,u,:] = sum_t dH[b,t,u,:] * (1 - H^2): one thread owns an output
 * element and adds its terms in ascending u (t).  Padded cells need no mask: their dH is zero as asrk_rnnt_grad_f32
 * writes it.  H and dH are read twice (once per output).  Call site: ops.RNNTJointFn.backward. */
int asrk_rnnt_joint_bwd_f32(const float *H, int64_t ldh, const float *dH, int64_t lddh, int B, int T, int U1, int J,
                            float *dE, int64_t ldde, float *dP, int64_t lddp, void *stream);
/* Row pass, the first of two reads of the logits z [B*T*U1, V] (row stride ldz): per cell inside the lattice
 *   lse = logsumexp(z[row, :]) (one pass: running max and sum per lane, as asrk_seq_logp_f32),
 *   lpb = z[row, blank] - lse,  lpl = z[row, txt[b, u]] - lse for u < U_b (0 at u = U_b; NaN for a label outside [0,V),
 *   nothing read).  A cell outside the lattice (t >= T_b or u > U_b) gets three zeros and its row is never read.
 * One wave per row below V = 2048 (4 rows per workgroup), a 256-thread workgroup per row from there on.
 * Call site: ops.RNNTLossFn.forward. */
int asrk_rnnt_rows_f32(const float *z, int64_t ldz, const int64_t *txt, int64_t txt_stride, const int64_t *enc_len,
                       const int64_t *txt_len, int B, int T, int U1, int V, int blank, float *lse, float *lpb,
                       float *lpl, void *stream);
/* Lattice: alpha(0,0) = 0, alpha(t,u) = logaddexp(alpha(t-1,u) + lpb(t-1,u), alpha(t,u-1) + lpl(t,u-1));
 * beta(T_b-1,U_b) = lpb, beta(t,u) = logaddexp(lpb(t,u) + beta(t+1,u), lpl(t,u) + beta(t,u+1));
 * nll[b] = -(alpha(T_b-1,U_b) + lpb(T_b-1,U_b)).  One workgroup per utterance walks the T_b + U_b anti-diagonals, 128
 * lanes per direction (a lane loop when U1 > 128), alpha and beta concurrently in the same launch, the previous
 * diagonal in LDS.  alpha, beta [B,T,U1]: cells outside the lattice are not written.  beta == NULL: alpha alone (no
 * gradient wanted).  ASRK_ESHAPE: U1 > 2048.  Call site: ops.RNNTLossFn.forward. */
int asrk_rnnt_lattice_f32(const float *lpb, const float *lpl, const int64_t *enc_len, const int64_t *txt_len, int B,
                          int T, int U1, float *alpha, float *beta, float *nll, void *stream);
/* Gradient pass, the second and last read of the logits:
 *   dz[b,t,u,v] = gscale[b] * (exp(alpha + beta - lnP) * softmax_v - [v == blank] exp(alpha + lpb + beta(t+1,u) - lnP)
 *                              - [v == y_{u+1}] exp(alpha + lpl + beta(t,u+1) - lnP)),
 * beta(T_b,U_b) := 0 and every other beta outside the lattice -inf.  Cells outside the lattice get exact zeros WRITTEN
 * (dz may be uninitialised) and are not read.  dz has its own row stride lddz >= V; dz == z (in place, then
 * lddz == ldz) is allowed: every element is read once, before it is written, and lpb / lpl come from the row pass.
 * The case split is asrk_rnnt_rows_f32's.  Call site: ops.RNNTLossFn.backward. */
int asrk_rnnt_grad_f32(const float *z, int64_t ldz, const int64_t *txt, int64_t txt_stride, const int64_t *enc_len,
                       const int64_t *txt_len, int B, int T, int U1, int V, int blank, const float *lse,
                       const float *lpb, const float *lpl, const float *alpha, const float *beta, const float *nll,
                       const float *gscale, float *dz, int64_t lddz, void *stream);
/* One iteration of the lock-step greedy search: k = argmax of logits[b, :V] (row stride ld; the lowest index among
 * equal values), then per row with done[b] == 0:
 *   k == blank, or n_sym[b] >= max_symbols, or n_tok[b] >= max_len: t_ptr[b] += 1, n_sym[b] = 0, emit[b] = 0, and
 *   done[b] = 1 once t_ptr[b] >= T_b (nothing is emitted);
 *   otherwise tokens[b, n_tok[b]] = k, n_tok[b] += 1, n_sym[b] += 1, last_tok[b] = k, emit[b] = 1.
 * A row with done[b] != 0 is not read; only emit[b] = 0 is written.  t_ptr, n_sym, n_tok, emit, done: int32 [B];
 * tokens int64 [B, tok_stride] (tok_stride >= max_len), last_tok int64 [B]; all device-resident, nothing is read back.
 * One wave per row.  Call site: ops.rnnt_greedy_step. */
int asrk_rnnt_greedy_step_f32(const float *logits, int64_t ld, const int64_t *enc_len, int B, int T, int V, int blank,
                              int max_symbols, int max_len, int32_t *t_ptr, int32_t *n_sym, int32_t *n_tok,
                              int64_t *tokens, int64_t tok_stride, int64_t *last_tok, int32_t *emit, int32_t *done,
                              void *stream);

/* ---- pruned transducer training (csrc/rnnt_prune.hip, csrc/rnnt_prune.inc; TransducerHead.forward_pruned) ---------------
 * Kuang et al. 2022: an additive joiner am[b,t,v] + lm[b,u,v] on the whole lattice tells which S consecutive label
 * positions per frame carry the mass; the joint network and the loss then run on that band, [B,T,S,..] arrays whose cell
 * (b,t,k) stands for u = s[b,t] + k (s int32 [B,T], clamped to [0, U1-1] by every kernel).  Lengths, txt and the lattice
 * conventions are those of the section above; 1 <= S <= 32.
 *
 * Simple-joiner row pass: am [B,T,V] row stride lda, lm [B,U1,V] row stride ldl.  Per cell inside the lattice
 *   lse = logsumexp_v(am[b,t,v] + lm[b,u,v]) (summed directly, one pass, the arithmetic of asrk_rnnt_rows_f32),
 *   lpb = (am[t,blank] + lm[u,blank]) - lse,  lpl = (am[t,y] + lm[u,y]) - lse with y = txt[b,u], 0 at u = U_b.
 * A workgroup owns 16 x 16 cells and streams V through LDS 64 columns at a time.  Cells outside the lattice get three
 * zeros; rows t >= T_b of am and u > U_b of lm are never read.  asrk_rnnt_lattice_f32 runs on lpb / lpl unchanged.
 * Call site: ops.RNNTSimpleLossFn.forward. */
int asrk_rnnt_simple_rows_f32(const float *am, int64_t lda, const float *lm, int64_t ldl, const int64_t *txt,
                              int64_t txt_stride, const int64_t *enc_len, const int64_t *txt_len, int B, int T, int U1,
                              int V, int blank, float *lse, float *lpb, float *lpl, void *stream);
/* Occupation, [B,T,U1] each, zeros outside the lattice: c = exp(alpha + beta - lnP), eb = exp(alpha + lpb + beta(t+1,u)
 * - lnP), el = exp(alpha + lpl + beta(t,u+1) - lnP), with beta(T_b,U_b) := 0 and -inf elsewhere outside the lattice
 * (asrk_rnnt_grad_f32's conventions).  Call site: ops.RNNTSimpleLossFn.forward. */
int asrk_rnnt_simple_occ_f32(const float *lpb, const float *lpl, const float *alpha, const float *beta, const float *nll,
                             const int64_t *enc_len, const int64_t *txt_len, int B, int T, int U1, float *c, float *eb,
                             float *el, void *stream);
/* Gradient of sum_b gscale[b] nll_b of the simple joiner, two launches:
 *   dam[b,t,v] = gscale[b] (sum_u c(t,u) exp(am[t,v] + lm[u,v] - lse(t,u)) - [v == blank] sum_u eb(t,u)
 *                           - sum_u [v == y_{u+1}] el(t,u)),   dlm[b,u,v] the same summed over t.
 * A thread owns its output elements and adds the terms in ascending u (t): no atomics, bit-reproducible.  Padded rows
 * (t >= T_b of dam, u > U_b of dlm) are written as exact zeros and not read.  Call site: ops.RNNTSimpleLossFn.backward. */
int asrk_rnnt_simple_grad_f32(const float *am, int64_t lda, const float *lm, int64_t ldl, const int64_t *txt,
                              int64_t txt_stride, const int64_t *enc_len, const int64_t *txt_len, int B, int T, int U1,
                              int V, int blank, const float *lse, const float *c, const float *eb, const float *el,
                              const float *gscale, float *dam, int64_t lddam, float *dlm, int64_t lddlm, void *stream);
/* Pruning bounds s int32 [B,T] from occ [B,T,U1] (= eb + el), one wave per utterance.  With E_b = max(0, U_b + 1 - S):
 *   raw(t) = argmax_{0 <= s <= E_b} sum_{u=s}^{min(s+S-1, U_b)} occ(t,u), the lowest s among equal sums;
 *   s'(0) = 0, s'(t) = clamp(raw(t), s'(t-1), s'(t-1) + S - 1);  s(t) = max(s'(t), E_b - (T_b-1-t)(S-1)) for t < T_b,
 *   s(t) = s(T_b-1) for padded frames.  s is non-decreasing, moves at most S-1 per frame, ends at E_b and starts at 0
 * exactly when (T_b-1)(S-1) >= E_b; otherwise the utterance has no path inside its band.
 * Call site: ops.rnnt_prune_ranges. */
int asrk_rnnt_prune_ranges_f32(const float *occ, const int64_t *enc_len, const int64_t *txt_len, int B, int T, int U1,
                               int S, int32_t *s, void *stream);
/* Band joint: H[b,t,k,:] = tanh(E[b,t,:] + P[b, min(s[b,t]+k, U1-1), :]); H [B,T,S,J] row stride ldh.  16-byte accesses
 * under the rule of asrk_rnnt_joint_f32.  Call site: ops.RNNTJointBandFn.forward. */
int asrk_rnnt_joint_band_f32(const float *E, int64_t lde, const float *P, int64_t ldp, const int32_t *s, int B, int T,
                             int S, int U1, int J, float *H, int64_t ldh, void *stream);
/* dE[b,t,:] = sum_k dH (1 - H^2) in ascending k; dP[b,u,:] = the sum over the (t,k) with min(s[b,t]+k, U1-1) == u, in
 * ascending t, then k.  One thread per output element, no atomics.  Call site: ops.RNNTJointBandFn.backward. */
int asrk_rnnt_joint_band_bwd_f32(const float *H, int64_t ldh, const float *dH, int64_t lddh, const int32_t *s, int B,
                                 int T, int S, int U1, int J, float *dE, int64_t ldde, float *dP, int64_t lddp,
                                 void *stream);
/* Row pass of the band loss on logits z [B*T*S, V]: asrk_rnnt_rows_f32 with cell (t,k) standing for u = s[b,t] + k
 * (inside the lattice iff t < T_b and u <= U_b; label txt[b,u]); lse, lpb, lpl [B,T,S], zeros outside, rows outside
 * never read.  The same one-pass log-sum-exp and the same case split at V = 2048.  Call site: ops.RNNTBandLossFn. */
int asrk_rnnt_rows_band_f32(const float *z, int64_t ldz, const int64_t *txt, int64_t txt_stride, const int64_t *enc_len,
                            const int64_t *txt_len, const int32_t *s, int B, int T, int S, int U1, int V, int blank,
                            float *lse, float *lpb, float *lpl, void *stream);
/* Band lpb / lpl [B,T,S] -> dense [B,T,U1] arrays holding -inf at every cell outside the band (or the lattice): the
 * band loss is the dense loss on these, so asrk_rnnt_lattice_f32 computes alpha, beta and nll (+inf when the band
 * holds no path).  Call site: ops.RNNTBandLossFn.forward. */
int asrk_rnnt_band_scatter_f32(const float *lpb_band, const float *lpl_band, const int32_t *s, const int64_t *enc_len,
                               const int64_t *txt_len, int B, int T, int S, int U1, float *lpb, float *lpl,
                               void *stream);
/* Gradient pass of the band loss: asrk_rnnt_grad_f32 per band cell; lse [B,T,S] from the row pass, lpb, lpl, alpha, beta
 * the dense [B,T,U1] arrays.  Cells outside the lattice, and every cell of an utterance whose nll is +inf, get exact
 * zeros written and are not read.  dz == z (then lddz == ldz) is allowed.  Call site: ops.RNNTBandLossFn.backward. */
int asrk_rnnt_grad_band_f32(const float *z, int64_t ldz, const int64_t *txt, int64_t txt_stride, const int64_t *enc_len,
                            const int64_t *txt_len, const int32_t *s, int B, int T, int S, int U1, int V, int blank,
                            const float *lse, const float *lpb, const float *lpl, const float *alpha, const float *beta,
                            const float *nll, const float *gscale, float *dz, int64_t lddz, void *stream);

/* ---- stateless prediction network (csrc/rnnt_ctx.hip; TransducerHead with pred.module = stateless) ----------------------
 * Ghodsi et al. 2020: the prediction network is a causal depthwise convolution over the embeddings of the last C labels
 * and a ReLU.  X [B,U1,D] is the embedded input <sos>, y_1 .. y_U; w [D,1,C] has the layout of a depthwise Conv1d weight
 * (tap C-1 multiplies the current label); 1 <= C <= 8.
 *   Y[b,u,d] = relu(sum_{j=0}^{C-1} w[d,0,j] * X[b, u-(C-1)+j, d]),
 * positions < 0 contribute zero, the sum runs over ascending j as a chain of f32 fused multiply-adds.  All values f32, no
 * float atomics: every result is a pure function of its inputs, reproducible bit for bit.
 * ASRK_EINVAL, before any device call: a NULL pointer with B > 0 (R > 0), B < 0 (R < 0), any other size <= 0, a row
 * stride below the row length.  ASRK_ESHAPE: C outside 1..8, tok_bytes not 4 or 8, B*U1 > INT32_MAX.  B == 0 (R == 0):
 * ASRK_OK without a launch.
 *
 * Forward: X and Y are [B*U1] rows of D floats with row strides ldx, ldy >= D.  One pass; 16-byte accesses when X and Y
 * are 16-byte aligned and D, ldx, ldy are multiples of 4, scalar otherwise.  Call site: ops.RNNTContextFn.forward. */
int asrk_rnnt_ctx_fwd_f32(const float *X, int64_t ldx, const float *w, int B, int U1, int D, int C, float *Y, int64_t ldy,
                          void *stream);
/* Backward, contiguous arrays: with dYm = dY * (Y > 0) (the derivative at a pre-activation of exactly 0 is 0)
 *   dX[b,u,d] = sum_j w[d,0,j] * dYm[b, u+(C-1)-j, d] over the j with u+(C-1)-j < U1, ascending j;
 *   dw[d,0,j] = sum_{b,u} dYm[b,u,d] * X[b, u-(C-1)+j, d]: partial sums over blocks of 32 consecutive rows of [B*U1] (rows
 *   ascending) into ws, then the blocks in ascending order.
 * ws: caller-owned device scratch, 4-byte aligned, at least asrk_rnnt_ctx_bwd_ws_bytes(B, U1, D, C) bytes, private to the
 * call until the stream has passed it; ASRK_EWORKSPACE if NULL, misaligned or smaller.  ASRK_ESHAPE above 65535 * 32 rows.
 * Three launches.  Call site: ops.RNNTContextFn.backward. */
size_t asrk_rnnt_ctx_bwd_ws_bytes(int B, int U1, int D, int C);
int asrk_rnnt_ctx_bwd_f32(const float *X, const float *w, const float *Y, const float *dY, int B, int U1, int D, int C,
                          float *dX, float *dw, void *ws, size_t ws_bytes, void *stream);
/* Decode step on the search state: tokens [R, ldt] (ldt >= Lc >= 1) of int32 (tok_bytes = 4, the beam state) or int64
 * (tok_bytes = 8, the greedy state), n_tok int32 [R].  Row r at n = clamp(n_tok[r], 0, Lc) is position n of the sequence
 * <sos>, tokens[r, 0..n-1]: tap j reads the label at n - C + j (the stored label for an index >= 0, <sos> = 0 for -1,
 * nothing before that), gathers its row straight from emb [V, D] (no [R,C,D] intermediate) and adds in the forward's
 * order with the forward's arithmetic, so Y[r, :] equals row n of the forward on the same labels bit for bit.  A label
 * outside [0, V) among those the row reads makes the whole row NaN and is never used as an index (dead beam slots carry
 * arbitrary labels).  Y [R, D] row stride ldy.  One launch.  Call site: ops.rnnt_ctx_step. */
int asrk_rnnt_ctx_step_f32(const void *tokens, int tok_bytes, int64_t ldt, const int32_t *n_tok, int R, int Lc,
                           const float *emb, int V, int D, const float *w, int C, float *Y, int64_t ldy, void *stream);

/* ---- transducer beam search (csrc/rnnt_beam.hip, csrc/rnnt_beam.inc; TransducerHead.beam_search) -----------------------
 * Alignment-length-synchronous search, B utterances in lock-step with W <= 32 slots each; row r = b*W + w of every
 * [B*W, ...] array.  The beam state is double buffered: arrays [2, B, ...], buffer `cur` is read and the other written.
 *
 * Joint step with several slots per utterance: H[r,:] = tanh(E[r / W, t_ptr[r], :] + P[r,:]); E [B,T,J] is not repeated
 * per slot, t_ptr int32 [B*W] is clamped to [0, T-1].  Call site: ops.rnnt_joint_slots. */
int asrk_rnnt_joint_slots_f32(const float *E, int64_t lde, const float *P, int64_t ldp, const int32_t *t_ptr, int B,
                              int T, int W, int J, float *H, int64_t ldh, void *stream);
/* Row pass over the logits z [B*W, V] (row stride ldz) and, with lm != NULL, the LM log-probabilities [B*W, V] (row
 * stride ldlm): per row lse = logsumexp(z), lpb = z[blank] - lse and the K <= min(32, V-1) best labels k != blank by
 * z[k] + lm_weight*lm[k] (the lower k among equal values), written as lab [B*W, K] int32 and
 * val = (z[k] - lse) + lm_weight*lm[k] (z[k] - lse without an LM), descending.  A label whose ranking value is -inf or
 * NaN is no candidate; missing entries are lab = -1, val = -inf.  The row is read once and held in registers: one wave
 * per row below V = 2048, a 256-thread workgroup from there on, 16-byte loads when bases and strides allow;
 * ASRK_ESHAPE above V = 16384.  Row w of utterance b with w >= n_live[b] (n_live int32 [B]; NULL: every row is live)
 * is not read: lse = lpb = 0 and K padded entries.  Call site: ops.rnnt_beam_rows. */
int asrk_rnnt_beam_rows_f32(const float *z, int64_t ldz, const float *lm, int64_t ldlm, float lm_weight,
                            const int32_t *n_live, int B, int W, int V, int K, int blank, float *lse, float *lpb,
                            float *val, int32_t *lab, void *stream);
/* Select, one workgroup per utterance (rules and phases: csrc/rnnt_beam.inc): from the [W, K+1] table of the row pass
 * and beam buffer `cur` it forms the candidates (blank first, then the labels of a slot with n_sym < max_symbols and
 * n_tok < max_len), merges equal sequences (float64 logaddexp), keeps the W best, moves survivors with t_ptr == T_b to
 * the finished list (capacity W, sorted by score, the earlier entry first on ties) and writes the other buffer:
 * n_live int32 [2,B]; t_ptr, n_sym, n_tok int32 [2,B,W]; score float64 [2,B,W]; tokens int32 [2,B,W,tok_stride]
 * (tok_stride >= max(max_len, 1)); fin_n int32 [2,B]; fin_len int32, fin_score float64 [2,B,W]; fin_tok as tokens.
 * Live rows are packed in rank order.  Per row of the next beam it also writes what drives the caller's gathers:
 * parent int64 (global row continued), last_tok int64 (label appended, else 0), emit int32, sel int64 = r + emit*B*W and
 * lm_sel int64 = emit ? B*W + r : parent (dead rows: identity).  Nothing is read back.  Call site: ops.rnnt_beam_select. */
int asrk_rnnt_beam_select(const float *lpb, const float *val, const int32_t *lab, const int64_t *enc_len, int B, int T,
                          int W, int K, int max_symbols, int max_len, int64_t tok_stride, int cur, int32_t *n_live,
                          int32_t *t_ptr, int32_t *n_sym, int32_t *n_tok, double *score, int32_t *tokens,
                          int32_t *fin_n, int32_t *fin_len, double *fin_score, int32_t *fin_tok, int64_t *parent,
                          int64_t *last_tok, int32_t *emit, int64_t *sel, int64_t *lm_sel, void *stream);

/* ---- transducer forced alignment (csrc/rnnt_align.hip, csrc/rnnt_align.inc; TransducerHead.align) ----------------------
 * The best (Viterbi) path of every utterance through its lattice, on the lpb / lpl [B,T,U1] arrays of
 * asrk_rnnt_rows_f32 (lengths clamped as there; cells outside an utterance's lattice are never read):
 *   delta(0,0) = 0;  a = delta(t-1,u) + lpb(t-1,u) (t > 0, else -inf);  b = delta(t,u-1) + lpl(t,u-1) (u > 0, else -inf);
 *   the label arc is taken iff (b > a) or (b != b);  delta(t,u) = taken ? b : a;
 *   score[b] = delta(T_b-1,U_b) + lpb(T_b-1,U_b),
 * in plain f32 (one add per arc, one compare per cell: a host f32 computation in this order gives the same bits).  Ties
 * go to the blank arc: among equal-scoring paths every label is emitted as early as possible.  A NaN on an arc (lpl of
 * a label outside [0,V)) reaches the score.
 * Outputs (device): frames int32 [B,U1-1] = the frame at which y_{u+1} was emitted, -1 for u >= U_b; labels_done int32
 * [B,T] = the number of labels emitted through frame t (the u at which frame t's blank was taken), -1 for t >= T_b;
 * tok_logp [B,U1-1] = lpl at the emitting cell, 0 beyond U_b; score [B] = the best path's log-probability.  With alpha,
 * beta, nll (asrk_rnnt_lattice_f32's, on the same lpb / lpl; all three or none) also tok_post [B,U1-1] = the posterior
 * exp(((alpha + lpl) + beta(t,u+1)) + nll) of the chosen emission arc, 0 beyond U_b; without them tok_post is not
 * touched.  An utterance whose score is -inf or NaN gets -1 in frames and labels_done and 0 in tok_logp and tok_post.
 * One 128-lane workgroup per utterance walks the T_b + U_b anti-diagonals with the previous diagonal in LDS; lattice,
 * backtrace and outputs run in one launch, nothing returns to the host.  Backpointers are one bit per cell, stored as
 * one 64-bit ballot word per (diagonal, 64-label slot): (T + U1 - 1) * ceil(U1 / 64) words per utterance.  `flags`
 * (ASRK_ALIGN_BP_*, above) picks where they live: _LDS in LDS when those words fit 128 KiB (beside at most 16 KiB of
 * diagonals), ASRK_ESHAPE otherwise; _GLOBAL in the caller's workspace; _AUTO (0) LDS where it fits.
 * ws: caller-owned device memory, 16-byte aligned, at least asrk_rnnt_align_ws_bytes(B, T, U1, flags) bytes, private to
 * the call until the stream has passed it; the size is 0 on the LDS route (ws may be NULL) and for arguments the call
 * rejects.  stamps: optional (NULL allowed) int64 [B,4], device wall-clock ticks of utterance b's workgroup at its
 * start, after the lattice, after the backtrace and at its end (tools/rnnt_align_bench.py).
 * ASRK_EINVAL, before any device call: a NULL pointer (frames, tok_logp, tok_post may be NULL when U1 == 1), B < 0, T or
 * U1 <= 0, unknown flags, only some of alpha / beta / nll, a NULL, misaligned or short workspace.  ASRK_ESHAPE:
 * U1 > 2048, B*T*U1 > INT32_MAX, a forced LDS route that does not fit.  B == 0: ASRK_OK without a launch.
 * Call site: ops.rnnt_align. */
size_t asrk_rnnt_align_ws_bytes(int B, int T, int U1, int flags);
int asrk_rnnt_align_f32(const float *lpb, const float *lpl, const int64_t *enc_len, const int64_t *txt_len, int B, int T,
                        int U1, int flags, const float *alpha, const float *beta, const float *nll, int32_t *frames,
                        int32_t *labels_done, float *tok_logp, float *tok_post, float *score, int64_t *stamps, void *ws,
                        size_t ws_bytes, void *stream);

/* ---- CTC prefix scores for joint CTC-attention beam search (src/ctc.py:76-116) -----------
 * All (hypothesis h, candidate c) pairs of one beam step in one launch.  x [T,V] log-probs;
 * r_prev [n,T,2] (0 = non-blank, 1 = blank path) of each hypothesis' prefix g_h; prefix_len[h] =
 * |g_h|, last_char[h] = g_h[-1]; candidates [n,C] (int32).  Outputs psi [n,C] = log p_ctc(g_h+c,...)
 * and r_out [n,C,T,2], exactly CTCPrefixScore.cheap_compute (incl. phi = blank-only path when
 * c == g_h[-1], psi[<eos>] = logaddexp(r_prev[-1]), logzero = -1e8 initialisation). */
int asrk_ctc_prefix_score_f32(const float *x, const float *r_prev, const int *prefix_len,
                              const int *last_char, const int *candidates, float *psi,
                              float *r_out, int n, int C, int T, int V, int blank, int eos,
                              float logzero, void *stream);
/* the same for the beams of SEVERAL utterances in one launch: x [U,T,V] (zero-padded to the longest utterance),
 * hypothesis h belongs to utterance row_mem[h] whose log-probabilities have mem_len[row_mem[h]] frames; the
 * recursion of h runs over ITS frames only (r_out / r_prev keep the common stride T; entries beyond the
 * utterance's length stay `logzero` and are never read), psi[<eos>] looks at its last frame. */
int asrk_ctc_prefix_score_multi_f32(const float *x, const int *row_mem, const int *mem_len, const float *r_prev,
                                    const int *prefix_len, const int *last_char, const int *candidates,
                                    float *psi, float *r_out, int n, int C, int T, int V, int U, int blank,
                                    int eos, float logzero, void *stream);

/* ---- FLAC reader (host code; replaces torchaudio.load on LibriSpeech's .flac files, src/audio.py:102) --
 * info: STREAMINFO of the file (total_samples per channel, 0 = unknown; md5_16 = MD5 of the unencoded
 * audio, all zero = not set).  decode: interleaved samples [n, channels] as int32 (value range of the
 * file's bits_per_sample); frame header CRC-8 and frame CRC-16 are verified.  When the stream holds more
 * than capacity_samples the decode still runs to the end, *decoded_samples is the count the stream holds and
 * the call returns ASRK_EWORKSPACE (the caller retries with that capacity) - never a silent truncation. */
int asrk_flac_info(const char *path, int *sample_rate, int *channels, int *bits_per_sample,
                   int64_t *total_samples, uint8_t *md5_16);
int asrk_flac_decode_i32(const char *path, int32_t *out, int64_t capacity_samples,
                         int64_t *decoded_samples);

#ifdef __cplusplus
}
#endif
#endif /* ASRK_H */
