/*
 * nplda_hip.h — C ABI of libnplda_hip.so, the MI355X (gfx950) Neural-PLDA hot path.
 *
 * The reference (iiscleap/NeuralPlda) has no FFI: its boundary is the Python class
 * utils/models.py:348-461 (NeuralPlda), utils/models.py:571-665 (GaussianBackend), the batch
 * loaders utils/sv_trials_loaders.py:418-437 and the module-level script
 * utils/adaptive_score_normalization.py:20-84.  This header is the C boundary those Python
 * symbols bind to in neuralplda_amd/ (ctypes stub shown in INTEGRATION.md).  Each entry point
 * names the reference lines it replaces.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer on the current HIP device unless marked "host";
 *    row-major, innermost stride 1; float rows 16-byte aligned (ld % 4 == 0).
 *  - the caller owns every buffer, including workspaces; the library allocates nothing and
 *    never synchronises the device: kernels are enqueued on `stream` (a hipStream_t passed as
 *    void*; NULL = the legacy default stream).
 *  - return value: 0 = NPLDA_OK, negative = argument error (NPLDA_E*), positive = hipError_t of
 *    the failed launch.  Nothing throws, nothing exits.  B == 0 / N == 0 is a successful no-op.
 *  - "packed" is the MFMA-fragment-ordered image of the model parameters produced by
 *    nplda_pack_params_f32 (rebuilt whenever parameters change; 0.4-0.5 MB).
 */
#ifndef NPLDA_HIP_H
#define NPLDA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: the entry points declared between this push and the pop at the end of
 * the header are its whole dynamic symbol table (tests/test_c_abi_cpu.py checks `nm -D`). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define NPLDA_OK            0
#define NPLDA_EINVAL      (-22)  /* null pointer, negative size, misaligned row, bad ld      */
#define NPLDA_EUNSUPPORTED (-95) /* dimension outside the compiled kernel set (see _max_dim) */
#define NPLDA_ENOSPC      (-28)  /* caller-provided buffer / workspace too small             */

typedef void* nplda_stream_t;

/* Library ABI version (bumped on any signature change). */
int nplda_abi_version(void);
/* Largest layer1/layer2 dimension the compiled MFMA kernels accept (padded to 16). */
int nplda_max_dim(void);
/* Digest of the sources this library was built from (sha256 of csrc/ and this header, first 16 hex digits; "unknown" if
 * it was not built by neuralplda_amd/build.py).  Static storage. */
const char* nplda_build_id(void);
/* Human-readable text for a return code (host string, static storage). */
const char* nplda_strerror(int code);

/* ---- parameter image -------------------------------------------------------------------- */

/* Bytes of the packed parameter image for a D0 -> D1 -> D2 model. 0 if unsupported. */
size_t nplda_packed_bytes(int D0, int D1, int D2);

/* Pack nn.Linear-layout parameters (utils/models.py:351-354: centering_and_LDA.weight (D1,D0),
 * .bias (D1), centering_and_wccn_plda.weight (D2,D1), .bias (D2), P_sqrt (D2), Q (D2)) into the
 * fragment-ordered image; also folds P = P_sqrt*P_sqrt (utils/models.py:373). */
int nplda_pack_params_f32(const float* W1, const float* b1, const float* W2, const float* b2,
                          const float* P_sqrt, const float* Q, int D0, int D1, int D2,
                          void* packed, size_t packed_bytes, nplda_stream_t stream);

/* ---- scoring ---------------------------------------------------------------------------- */

/* NeuralPlda.forward(x1, x2) (utils/models.py:378-382 = :366-370 twice + :372-376), fused:
 * s[i] = sum_d Q_d (z1_id^2 + z2_id^2) + 2 sum_d P_d z1_id z2_id,
 * z = W2 * normalize(W1 x + b1) + b2.  x1, x2: (B, D0) with row stride ldx; s: (B). */
int nplda_score_pairs_f32(const float* x1, const float* x2, int64_t B, int64_t ldx,
                          const void* packed, int D0, int D1, int D2, float* s,
                          nplda_stream_t stream);

/* nplda_score_pairs_f32 on the pairs (table[rows1[i]], table[rows2[i]]) of a resident (N, ldt) x-vector table: the gather of
 * load_xvec_trials_from_numbatch (utils/sv_trials_loaders.py:418-426) — two passes over 2 B x 2 KB in validate()'s loop,
 * xvector_NeuralPlda_pytorch.py:60-66 — folded into the scoring kernel (the balanced-tile kernel reads its x fragments
 * through the indices).  rows1 / rows2: int64 device arrays, values clamped into [0, N).  Covers the batches
 * nplda_score_pairs_f32 itself gives to that kernel (D0 == 512, D1 and D2 in 145..176, B between the small-batch and the full
 * streaming sizes: same bits as gather + score); otherwise NPLDA_EUNSUPPORTED: gather with nplda_gather_rows_f32 and call
 * nplda_score_pairs_f32. */
int nplda_score_pairs_rows_f32(const float* table, int64_t N, int64_t ldt, const int64_t* rows1, const int64_t* rows2,
                               int64_t B, const void* packed, int D0, int D1, int D2, float* s, nplda_stream_t stream);
/* nplda_score_pairs_f32 on BFLOAT16 rows (x-vectors straight from an extractor that runs in bf16, BASELINE configs[4]):
 * ldx in elements, rows 8-byte aligned.  The rows are widened in registers by the streaming kernels — no fp32 copy of
 * the batch is made (2 x 1 M x 512: 4 GB of writes and reads) and the scores are those of nplda_score_pairs_f32 on the
 * widened rows, bit for bit.  NPLDA_EUNSUPPORTED below the streaming sizes (convert and call nplda_score_pairs_f32). */
int nplda_score_pairs_bf16rows_f32(const void* x1, const void* x2, int64_t B, int64_t ldx, const void* packed, int D0,
                                   int D1, int D2, float* s, nplda_stream_t stream);

/* Name of the kernel nplda_score_pairs_f32 launches for a batch of B pairs of a D0 -> D1 -> D2 model on the current
 * device (the batch decides between the small-batch, the balanced-tile and the streaming schedule); "" for B <= 0 or an
 * unsupported model.  Reporting only (bench.py labels its roofline object with it); static storage. */
const char* nplda_score_pairs_kernel_name(int64_t B, int D0, int D1, int D2);

/* NeuralPlda.extract_plda_embeddings(x) (utils/models.py:366-370) for N rows, plus the per-row
 * self term q[n] = sum_d Q_d z_nd^2 used by the indexed scorer.  z: (N, ldz) with
 * ldz >= nplda_padded_dim(D1, D2); columns D2..nplda_padded_dim-1 are written as 0.
 * q may be NULL. */
int nplda_embed_f32(const float* x, int64_t N, int64_t ldx, const void* packed, int D0, int D1,
                    int D2, float* z, int64_t ldz, float* q, nplda_stream_t stream);

/* extract_plda_embeddings of TWO tables in one launch: rows [0, Na) of z / q are xa's rows, rows [Na, Na + Nb) xb's (same
 * row stride ldx) — the enroll / test rows and the cohort of one adaptive-score-normalisation call
 * (utils/adaptive_score_normalization.py:27-36 needs both embedded; utils/models.py:366-370 per row).  Same values as two
 * nplda_embed_f32 calls; one launch where the balanced-tile kernel applies (D0 == 512, D1 and D2 in 145..176, a few tiles per
 * CU), two launches otherwise. */
int nplda_embed_pair_f32(const float* xa, int64_t Na, const float* xb, int64_t Nb, int64_t ldx, const void* packed, int D0,
                         int D1, int D2, float* z, int64_t ldz, float* q, nplda_stream_t stream);

/* extract_plda_embeddings of the rows rows[0 .. U) of a resident (N, ldt) x-vector table, the gather folded into the kernel:
 * z[u] = embed(table[rows[u]]) (indices clamped into [0, N)).  What validate() does per epoch
 * (xvector_NeuralPlda_pytorch.py:56-83 scores every trial through utils/sv_trials_loaders.py:418-426 + utils/models.py:378-382;
 * a trial list names each utterance many times, so the distinct utterances are embedded ONCE and the trials scored by index,
 * nplda_score_indexed_f32).  Returns NPLDA_EUNSUPPORTED where the balanced-tile kernel does not apply (the caller then
 * gathers, nplda_gather_rows_f32, and calls nplda_embed_f32: same values). */
int nplda_embed_rows_f32(const float* table, int64_t N, int64_t ldt, const int64_t* rows, int64_t U, const void* packed,
                         int D0, int D1, int D2, float* z, int64_t ldz, float* q, nplda_stream_t stream);

/* Row width (floats) the kernels use for layer outputs of a D1/D2 model: both layers are padded
 * to the same multiple of 16 (the compiled square kernel size). 0 if unsupported. */
int nplda_padded_dim(int D1, int D2);

/* ---- training: forward with saved activations, losses, backward ---------------------------- */

/* As nplda_score_pairs_f32, additionally saving what the backward needs: y (2B, ldz) = normalised
 * layer-1 outputs (rows [0,B) = x1 side, [B,2B) = x2 side), z (2B, ldz) = embeddings in the same
 * row order, rn (2B) = 1 / max(||u||, 1e-12).  ldz must equal nplda_padded_dim(D1, D2).
 * Replaces what autograd would save for utils/models.py:366-382. */
int nplda_forward_train_f32(const float* x1, const float* x2, int64_t B, int64_t ldx,
                            const void* packed, int D0, int D1, int D2, float* s, float* y, float* z,
                            float* rn, int64_t ldz, nplda_stream_t stream);

/* Number of fp64 batch sums the loss needs: kind 0 = SoftCdet over K thresholds (2 + 4K, K <= 4),
 * kind 1 = BCE ("crossentropy", 4), kind 2 = hard Cdet at the thresholds (utils/models.py:401-404;
 * same layout as kind 0, no gradient).  0 if unsupported. */
int nplda_loss_nsums(int K, int kind);

/* Pass 1 of the loss (utils/models.py:384-393): accumulate, in fp64, every batch-global sum the loss
 * and its gradient need into sums[nplda_loss_nsums] (zeroed here).  All entries are additive over
 * shards of a batch: under data parallelism all-reduce(sum) this vector before pass 2.
 * theta: HOST array of K device pointers (the Th{beta} / threshold_Xent parameters, 1 float each). */
int nplda_loss_sums_f32(const float* s, const float* t, int64_t B, const float* const* theta, int K,
                        float alpha, int kind, double* sums, nplda_stream_t stream);

/* Pass 2: loss (1 float), g[i] = dL/ds_i (B floats, may be NULL) and dL/dtheta (K floats, may be
 * NULL) from the sums.  beta: HOST array of K floats (utils/NpldaConf.py:38). */
int nplda_loss_finish_f32(const float* s, const float* t, int64_t B, const float* const* theta,
                          const float* beta, int K, float alpha, int kind, const double* sums,
                          float* loss, float* g, float* dtheta, nplda_stream_t stream);

/* Both passes in one call for a batch that is NOT sharded (no all-reduce of the sums in between): sums, loss, g and
 * dtheta as nplda_loss_sums_f32 followed by nplda_loss_finish_f32 would give them, bit for bit (all four outputs are
 * required; kinds 0 and 1).  A batch of <= 4096 16-byte aligned scores runs as ONE single-block launch — the training
 * step's loss (utils/models.py:384-393 + its autograd) in one graph node; anything else takes the two passes. */
int nplda_loss_fwd_bwd_f32(const float* s, const float* t, int64_t B, const float* const* theta, const float* beta,
                           int K, float alpha, int kind, double* sums, float* loss, float* g, float* dtheta,
                           nplda_stream_t stream);

/* Floats in the flat gradient [dW1 (D1,D0) | db1 (D1) | dW2 (D2,D1) | db2 (D2) | dP_sqrt (D2) | dQ (D2)]. */
size_t nplda_grad_floats(int D0, int D1, int D2);
/* Bytes of caller-provided workspace nplda_backward_f32 needs for a batch of B pairs. */
size_t nplda_backward_workspace_bytes(int64_t B, int D0, int D1, int D2);

/* Backward of s = NeuralPlda.forward(x1, x2) given g = dL/ds: the autograd of utils/models.py:366-382
 * hand-derived, three launches, deterministic summation order.
 * y, z, rn: as saved by nplda_forward_train_f32.  P_sqrt: the raw (D2) parameter (chain rule of
 * P = P_sqrt^2).  Writes grad_flat (nplda_grad_floats floats). */
int nplda_backward_f32(const float* x1, const float* x2, int64_t B, int64_t ldx, const void* packed,
                       int D0, int D1, int D2, const float* g, const float* y, const float* z,
                       const float* rn, int64_t ldz, const float* P_sqrt, void* ws, size_t ws_bytes,
                       float* grad_flat, nplda_stream_t stream);

/* nplda_backward_f32 plus the gradient w.r.t. the INPUTS: dx1, dx2 (B, D0) with row stride lddx, both or neither
 * NULL — dL/dx = du . W1, what autograd hands to an x-vector extractor trained jointly with the head (the E2E model,
 * utils/models.py:251-268, feeds extractor outputs through the same two layers).  One more MFMA GEMM on the `du` rows the
 * backward already holds (csrc/nplda_matmul.hip).  Workspace: nplda_backward_ex_workspace_bytes(2 B, ..., want_dx). */
size_t nplda_backward_ex_workspace_bytes(int64_t rows, int D0, int D1, int D2, int want_dx);
int nplda_backward_ex_f32(const float* x1, const float* x2, int64_t B, int64_t ldx, const void* packed,
                          int D0, int D1, int D2, const float* g, const float* y, const float* z,
                          const float* rn, int64_t ldz, const float* P_sqrt, void* ws, size_t ws_bytes,
                          float* grad_flat, float* dx1, float* dx2, int64_t lddx, nplda_stream_t stream);

/* NeuralPlda.extract_plda_embeddings (utils/models.py:366-370) with what ITS backward needs: z (N, ldz) as
 * nplda_embed_f32, y (N, ldz) = normalised layer-1 rows, rn (N) = 1 / max(||u||, 1e-12); ldz = nplda_padded_dim. */
int nplda_embed_train_f32(const float* x, int64_t N, int64_t ldx, const void* packed, int D0, int D1, int D2,
                          float* z, float* y, float* rn, int64_t ldz, nplda_stream_t stream);

/* Backward of z = extract_plda_embeddings(x) given gz = dL/dz (N, D2) with row stride ldgz (any stride >= D2):
 * grad_flat as nplda_backward_f32 lays it out (dP_sqrt = dQ = 0: z does not depend on them) and, when dx != NULL,
 * dL/dx (N, D0).  y, rn from nplda_embed_train_f32.  Workspace: nplda_backward_ex_workspace_bytes(N, ..., dx != NULL). */
int nplda_embed_backward_f32(const float* x, int64_t N, int64_t ldx, const void* packed, int D0, int D1, int D2,
                             const float* gz, int64_t ldgz, const float* y, const float* rn, int64_t ldz,
                             void* ws, size_t ws_bytes, float* grad_flat, float* dx, int64_t lddx,
                             nplda_stream_t stream);

/* Backward of s = NeuralPlda.forward_from_plda_embeddings(z1, z2) (utils/models.py:372-376) given g = dL/ds:
 * dz1 = 2 g (Q z1 + P z2), dz2 = 2 g (Q z2 + P z1) (either may be NULL), dQ = sum g (z1^2 + z2^2),
 * dP_sqrt = 4 P_sqrt sum g z1 z2 (either may be NULL); column sums in a fixed order (deterministic). */
size_t nplda_score_embeddings_bwd_workspace_bytes(int64_t B, int D2);
int nplda_score_embeddings_bwd_f32(const float* z1, int64_t ld1, const float* z2, int64_t ld2, int64_t B, int D2,
                                   const float* P_sqrt, const float* Q, const float* g, float* dz1, int64_t ldd1,
                                   float* dz2, int64_t ldd2, float* dP_sqrt, float* dQ, void* ws, size_t ws_bytes,
                                   nplda_stream_t stream);

/* ---- all-pairs training step on a batch of embeddings (csrc/nplda_allpairs.hip, design/k17_allpairs.md) ---------- */

/* Rows of z one block of the all-pairs kernel owns (tests place their ragged edges by it). */
#define NPLDA_ALLPAIRS_TILE 64

/* Bytes of caller-provided workspace nplda_allpairs_loss_f32 needs for N rows of D2 features and K thresholds (the padded
 * image of z, the self terms, the per-block partial sums).  0 for N < 0, N > 2^20, D2 above nplda_max_dim() or K outside
 * 1..4. */
size_t nplda_allpairs_workspace_bytes(int64_t N, int D2, int K);

/* The loss over ALL trials a batch of N embeddings implies, with every gradient: what the reference computes by listing
 * the pairs (utils/sv_trials_loaders.py:22-75, TrialSampler), scoring each (utils/models.py:372-376) and taking the loss
 * (utils/models.py:384-399) and its autograd, each utterance embedded once per pair it appears in.  Here
 *   T = {(i, j): i < j, and grp[i] == grp[j] when grp != NULL}, a trial is a target iff spk[i] == spk[j],
 *   s_ij = q_i + q_j + 2 sum_d P_d z_id z_jd,  q_i = sum_d Q_d z_id^2,  P = P_sqrt^2,
 *   sums (nplda_loss_nsums doubles), loss and dtheta as nplda_loss_fwd_bwd_f32 gives them on the scores of T (the BCE
 *   normaliser is |T|; N_t and N_n are counted exactly from the labels), and with g_ij = dL/ds_ij, G symmetric with
 *   G_ij = G_ji = g_ij on T and 0 elsewhere, r_i = sum_j G_ij, A_i = sum_j G_ij z_j:
 *   dz_i = 2 r_i (Q o z_i) + 2 P o A_i,  dQ_d = sum_i r_i z_id^2,  dP_sqrt_d = 2 P_sqrt_d sum_i z_id A_id
 *   (= 4 P_sqrt sum_{i<j} g z_i z_j, as nplda_score_embeddings_bwd_f32 defines it).
 * The N x N matrices are never written.  z: (N, ldz); spk, grp: N int32 (grp may be NULL: one group); theta: HOST array of K
 * device pointers, beta: HOST array of K floats (NULL for BCE), as for nplda_loss_fwd_bwd_f32; kind 0 = SoftCdet, 1 = BCE
 * (theta[0]).  dz (N, lddz), dP_sqrt (D2), dQ (D2) and dtheta (K) may each be NULL; with all three gradients NULL only the
 * tiles that hold a trial are walked.  Kernel launches on `stream` and nothing else (no allocation, no memset, no
 * synchronisation: capturable); bitwise repeatable (fixed summation orders, no floating-point atomics).  N < 2 or an empty T:
 * sums and gradients 0, loss 0 / 0.  NPLDA_EINVAL: a null required pointer, N < 0, D2 <= 0, K outside 1..4, kind outside
 * {0, 1}, z / dz / ws not 16-byte aligned or ldz / lddz not a multiple of 4 or below D2; NPLDA_EUNSUPPORTED: D2 above
 * nplda_max_dim() or N above 2^20; NPLDA_ENOSPC: ws_bytes below nplda_allpairs_workspace_bytes(N, D2, K). */
int nplda_allpairs_loss_f32(const float* z, int64_t ldz, int64_t N, int D2, const int32_t* spk, const int32_t* grp,
                            const float* P_sqrt, const float* Q, const float* const* theta, const float* beta, int K,
                            float alpha, int kind, double* sums, float* loss, float* dtheta, float* dz, int64_t lddz,
                            float* dP_sqrt, float* dQ, void* ws, size_t ws_bytes, nplda_stream_t stream);

/* ---- speaker-classification loss over a class table (csrc/nplda_classify.hip, design/k26_classify.md) ----------- */

/* Bytes of caller-provided workspace nplda_classify_loss_f32 needs for N rows, C classes and D features under the chunk
 * arguments it will be called with (0 = the plan's choice, a function of (N, C, D) alone): the padded images of X and W,
 * per-row and per-class vectors, and one partial of the gradients per chunk — nothing grows with N * C.  Never decreases
 * with N or C.  0 for N or C outside 0 .. 2^20, D outside 1 .. nplda_max_dim() or a negative chunk argument. */
size_t nplda_classify_workspace_bytes(int64_t N, int64_t C, int D, int class_chunks, int row_chunks);

/* Softmax (kind 0), AM-softmax / CosFace (kind 1) or AAM-softmax / ArcFace (kind 2) cross entropy of N embeddings
 * X (N, ldx) against a class table W (C, ldw) with optional bias b (C) and labels y (N int32), scale s > 0, margin m >= 0,
 * with every gradient; the N x C logits are never written.
 *   kind 0: u_ic = <x_i, w_c> (m must be 0);  kinds 1, 2: u_ic = <x^_i, w^_c>, x^_i = x_i / max(||x_i||, 1e-12), w^_c likewise
 *   a_ic = s u_ic + b_c (the inference logit);  l_ic = a_ic for c != y_i,  l_iy = s phi(u_iy) + b_y (the training logit)
 *   phi(u) = u (kind 0), u - m (kind 1); kind 2: v = clamp(u, -1, 1), sn = sqrt(max(1 - v^2, 2^-24)),
 *     v > -cos m: phi = v cos m - sn sin m, phi' = cos m + (v / sn) sin m;  otherwise phi = v - m sin m, phi' = 1
 *     (the clamp is the identity in the derivative)
 *   V = {i: 0 <= y_i < C}: y_i = -1 ignores row i; any other label outside 0 .. C - 1 is ignored too, and counted
 *   lse_i = log sum_c exp(l_ic);  rowloss_i = lse_i - l_iy on V, 0 elsewhere;  loss = sum_{i in V} rowloss_i / |V| (fp64 sum,
 *     rows in order; NaN for an empty V);  pred_i = argmax_c a_ic for every row (margin-free, the lowest index on ties)
 *   counts (3 int64) = |V|, #{i in V: pred_i = y_i}, #{i: y_i < -1 or y_i >= C}
 *   g_ic = (exp(l_ic - lse_i) - [c = y_i]) / |V| on V, 0 elsewhere;  db_c = sum_i g_ic;  h_ic = s g_ic, times phi'(u_iy) at c = y_i
 *   kind 0: dX = H W, dW = H^T X;  kinds 1, 2: A = H W^, dX_i = (A_i - <x^_i, A_i> x^_i) / max(||x_i||, 1e-12), and dW the
 *     same way from H^T X^.
 * rowloss (N), pred (N int32), dX (N, lddx), dW (C, lddw) and db (C) may each be NULL; without dX the rows-own gradient pass is
 * not launched, without dW and db the classes-own pass is not, without any of the three only the loss passes run.
 * class_chunks / row_chunks: into how many chunks the class tiles (of 16) / row tiles (of 16) are split over blocks; 0 = the
 * plan's choice, a positive value is used as given (at most one chunk per tile, at most 1024): the results agree to rounding,
 * pred and counts exactly away from ties in fp32.  Kernel launches on `stream` and nothing else (no allocation, no memset, no synchronisation:
 * capturable); bitwise repeatable for one (shape, chunk arguments): fixed summation orders, no floating-point atomics.
 * N == 0 or C == 0: nothing is launched, NPLDA_OK.  NPLDA_EINVAL: a null required pointer (X, W, y, loss, counts, ws), X / W /
 * dX / dW / ws not 16-byte aligned, ldx / ldw / lddx / lddw below D or not a multiple of 4, kind outside 0 .. 2, s <= 0, m < 0,
 * m != 0 under kind 0, m >= pi under kind 2, N, C or a chunk argument negative, D <= 0; NPLDA_EUNSUPPORTED: D above
 * nplda_max_dim(), N or C above 2^20; NPLDA_ENOSPC: ws_bytes below nplda_classify_workspace_bytes of the same arguments. */
int nplda_classify_loss_f32(const float* X, int64_t ldx, int64_t N, const float* W, int64_t ldw, int64_t C, int D,
                            const float* b, const int32_t* y, int kind, float s, float m, int class_chunks, int row_chunks,
                            float* loss, int64_t* counts, float* rowloss, int32_t* pred, float* dX, int64_t lddx, float* dW,
                            int64_t lddw, float* db, void* ws, size_t ws_bytes, nplda_stream_t stream);

/* ---- top-k search over an embedding table (csrc/nplda_topk.hip, design/k19_topk_search.md) ---------------------- */

/* Largest k of nplda_topk_scores_f32. */
#define NPLDA_TOPK_MAX_K 128

/* Bytes of caller-provided workspace nplda_topk_scores_f32 needs for R rows against M table rows (k composites per row and
 * column chunk of the table).  Never decreases with R, M or k.  0 for R outside 0 .. 2^24 - 1, M outside 0 .. 2^31 - 1, D2 above nplda_max_dim()
 * or k outside 1 .. NPLDA_TOPK_MAX_K.  The number of chunks is chosen to fill the chip; the environment variable
 * NPLDA_TOPK_MAX_CHUNKS, read at every call by this function and by nplda_topk_scores_f32 alike, can only lower its cap
 * (fewer, longer chunks and less workspace; the result does not depend on it). */
size_t nplda_topk_workspace_bytes(int64_t R, int64_t M, int D2, int k);

/* 1:N search: for each of R probe rows the k best-scoring of the M rows of a table, with their indices — what the
 * reference would do with forward_from_plda_embeddings (utils/models.py:372-376) on every pair, an R x M matrix and a sort;
 * the matrix is never written here.  s_rj = q_rows[r] + q_tab[j] + 2 sum_d P_d z_rows[r, d] z_tab[j, d], P = P_sqrt^2 from
 * `packed`; z_rows (R, ldz) / q_rows (R) and z_tab (M, ldz) / q_tab (M) come from nplda_embed_f32 (ldz >= nplda_padded_dim,
 * ldz % 4 == 0; columns D2 .. ldz may hold any FINITE values, they meet P = 0; buffer rows beyond R and M are never read).
 * Column j is ELIGIBLE for row r iff (grp_rows == NULL or grp_rows[r] == grp_tab[j]) and (self_rows == NULL or
 * self_rows[r] != j) and (mask_mode 0: always; 1: lab_rows[r] != lab_tab[j]; 2: lab_rows[r] == lab_tab[j]) — by index and
 * label only, never by value.  Labels and groups are int32 (lab_* may be NULL when mask_mode == 0; grp_rows / grp_tab are
 * given both or neither); self_rows is int64 (R) or NULL: row r IS table row self_rows[r] (any value outside 0 .. M - 1
 * excludes nothing).
 * Output: vals (R, k) float and idx (R, k) int64, per row the k largest (largest = 1) or smallest (largest = 0) eligible
 * scores, best first; equal fp32 scores (-0.0f counts as +0.0f) in ascending column order, inside the output and at the
 * rank-k boundary: the result of a stable sort of the row.  A row with fewer than k eligible columns has idx = -1 and
 * vals = -inf (largest) / +inf (smallest) in the remaining slots.  NaN scores are outside the ordering's contract.
 * The fp32 value of s_rj depends on (row, column, model) only — fp32-input MFMAs, a fixed feature order — never on R, M,
 * the chunking or the tile a column falls in, and so do vals and idx.  Two kernel launches on `stream` and nothing else (no
 * allocation, no memset, no atomics, no synchronisation: capturable; bitwise repeatable).
 * R == 0: a no-op.  M == 0: every slot is filled as for a short row.  NPLDA_EINVAL: a null required pointer, R or M < 0, k
 * outside 1 .. NPLDA_TOPK_MAX_K, largest outside {0, 1}, mask_mode outside 0 .. 2 or labels missing for it, one of grp_rows /
 * grp_tab without the other, z_rows / z_tab / packed / ws not 16-byte aligned, ldz not a multiple of 4 or below
 * nplda_padded_dim(D1, D2); NPLDA_EUNSUPPORTED: a model outside the compiled kernel set, R above 2^24 - 1 (search more rows in
 * several calls), M above 2^31 - 1;
 * NPLDA_ENOSPC: ws_bytes below nplda_topk_workspace_bytes(R, M, D2, k). */
int nplda_topk_scores_f32(const float* z_rows, const float* q_rows, int64_t R, const float* z_tab, const float* q_tab,
                          int64_t M, int64_t ldz, const void* packed, int D0, int D1, int D2, int k, int largest,
                          int mask_mode, const int32_t* lab_rows, const int32_t* lab_tab, const int32_t* grp_rows,
                          const int32_t* grp_tab, const int64_t* self_rows, float* vals, int64_t* idx, void* ws,
                          size_t ws_bytes, nplda_stream_t stream);

/* ---- small resident-matrix GEMM on row batches (input gradients; csrc/nplda_matmul.hip) ---------------------- */

/* MFMA-fragment image of a K x N matrix Wm (K <= 512, N % 4 == 0) for nplda_rows_matmul_f32.  mode 0: Wm = src (K, N)
 * row-major with stride ldw; 1: Wm = src^T (src is (N, K)); 2: Wm = src + src^T (K == N). */
size_t nplda_matrix_frag_bytes(int K, int N);
int nplda_pack_matrix_f32(const float* src, int64_t ldw, int K, int N, int mode, void* frag, size_t frag_bytes,
                          nplda_stream_t stream);
/* DPlda's quadratic form for the input-side backward, straight from logistic_regres.weight = [Wb | Ww | ws]
 * (utils/models.py:484-490): the fragment image of M + M^T, M = [[Ww, Wb], [Wb, Ww]] (2 D1 x 2 D1,
 * nplda_matrix_frag_bytes(2 D1, 2 D1) bytes) and v = [ws; ws] (2 D1 floats) in one launch — what
 * torch.cat x 3 + nplda_pack_matrix_f32(mode 2) produced. */
int nplda_dplda_quadform_f32(const float* wlr, int D1, void* frag, size_t frag_bytes, float* v, nplda_stream_t stream);
/* out[r, :] = rowscale[r] * (in[r, :K] . Wm + bias) for R rows; bias (N) and rowscale (R) may be NULL.  With
 * Wm = M + M^T, bias = v, rowscale = dL/ds this is the gradient of DPlda's quadratic form x^T M x + x^T v + c
 * (utils/models.py:484-495) w.r.t. the paired rows x = [y1; y2]. */
int nplda_rows_matmul_f32(const float* in, int64_t ldin, int64_t R, int K, const void* frag, int N,
                          const float* bias, const float* rowscale, float* out, int64_t ldout,
                          nplda_stream_t stream);
/* F.normalize backward on paired rows: du[h B + k, :] = (dy - y (y . dy)) * rn[h B + k], dy = dpaired[k, h D1 : (h+1) D1],
 * y = paired[k, h D1 : (h+1) D1]; du is (2 B, ldz) with zero padding columns (the layout nplda_backward's wgrad and
 * nplda_rows_matmul_f32 consume).  rn (2 B) from gb_score_pairs_ex_f32. */
int nplda_normalize_bwd_paired_f32(const float* dpaired, int64_t lddp, const float* paired, int64_t ldp,
                                   const float* rn, int64_t B, int D1, float* du, int64_t ldz,
                                   nplda_stream_t stream);
/* dW1 (D1, D0) and db1 (D1) of an LDA layer from du (2 B, ldz) and the inputs x1, x2 (B, D0): the wgrad half of
 * nplda_backward_f32 alone (DPlda / GaussianBackend heads have no second layer).  out: D1 * D0 + D1 floats. */
size_t nplda_lda_wgrad_workspace_bytes(int64_t B, int D0, int D1);
int nplda_lda_wgrad_f32(const float* x1, const float* x2, int64_t B, int64_t ldx, const float* du, int64_t ldz,
                        int D0, int D1, void* ws, size_t ws_bytes, float* out, nplda_stream_t stream);
/* dx1, dx2 (B, D0) = du . W1 for the same heads (W1 (D1, D0) row-major raw parameter; frag workspace inside ws). */
size_t nplda_lda_dgrad_workspace_bytes(int D0, int D1);
int nplda_lda_dgrad_f32(const float* du, int64_t ldz, int64_t B, const float* W1, int D0, int D1, void* ws,
                        size_t ws_bytes, float* dx1, float* dx2, int64_t lddx, nplda_stream_t stream);

/* ---- indexed scoring (embed each utterance once, then score index pairs) --------------------- */

/* utils/models.py:372-376 on rows of a pre-embedded table: s[p] = q[i1[p]] + q[i2[p]] +
 * 2 sum_d P_d z[i1[p], d] z[i2[p], d].  z: (N, ldz) and q: (N) from nplda_embed_f32; i1, i2: int64 (B).
 * The host gather of utils/sv_trials_loaders.py:418-426 disappears.  Out-of-range indices give NaN.
 * q may be NULL: the self terms q[i] = sum_d Q_d z[i, d]^2 (utils/models.py:374) are then formed inside the kernel from the
 * rows it reads anyway — two scattered 4-byte reads per pair less (4.6e9 -> 5.4e9 pairs/s over a 768 MB table). */
int nplda_score_indexed_f32(const float* z, int64_t ldz, const float* q, int64_t N, const int64_t* i1,
                            const int64_t* i2, int64_t B, const void* packed, int D0, int D1, int D2,
                            float* s, nplda_stream_t stream);

/* NeuralPlda.forward_from_plda_embeddings(z1, z2) (utils/models.py:372-376) on two explicit (B, D2)
 * tensors with arbitrary row strides; P_sqrt, Q are the raw (D2) parameters. */
int nplda_score_embeddings_f32(const float* z1, int64_t ld1, const float* z2, int64_t ld2, int64_t B,
                               int D2, const float* P_sqrt, const float* Q, float* s,
                               nplda_stream_t stream);

/* Device index-select out[r, :] = table[idx[r], :] from a resident (N, D0) x-vector matrix — the
 * device counterpart of load_xvec_trials_from_numbatch / _from_idbatch
 * (utils/sv_trials_loaders.py:418-437).  Out-of-range indices give NaN rows. */
int nplda_gather_rows_f32(const float* table, int64_t ldt, int64_t N, const int64_t* idx, int64_t B,
                          int D0, float* out, int64_t ldo, nplda_stream_t stream);

/* load_xvec_trials_from_numbatch (utils/sv_trials_loaders.py:418-426) on the device in ONE launch: the reference looks every
 * pair's two utterances up as mega_dict[num_to_id_dict[n]]; here `map` (nmap int64, built once per (mega_dict, num_to_id_dict))
 * takes a trial number to its row of the resident (N, ldt) x-vector table (negative: the utterance is not in the table) and
 * out1[r, :] = table[map[num1[r]], :], out2[r, :] = table[map[num2[r]], :] (B rows each, row stride ldo).  A number outside
 * [0, nmap) gives a NaN row and bad[0] |= 1, a number mapped to no row a NaN row and bad[0] |= 2: the caller reads the word
 * back and raises the reference's KeyError (the word is only ever OR-ed into, with a system-scope atomic: the caller clears
 * it, and may keep it in pinned host memory to read it after a stream synchronise without a copy). */
int nplda_gather_pairs_mapped_f32(const float* table, int64_t ldt, int64_t N, const int64_t* map, int64_t nmap,
                                  const int64_t* num1, const int64_t* num2, int64_t B, int D0, float* out1, float* out2,
                                  int64_t ldo, int32_t* bad, nplda_stream_t stream);

/* ---- adaptive score normalisation (utils/adaptive_score_normalization.py:27-73) ------------------ */

/* Recommended bytes of workspace: enough for the spilled cohort score matrix (whole matrix up to 4 GiB, else row
 * chunks, behind a 256-byte control block) and for the fused path's per-row candidate lists.  Any ws_bytes >= 256 + one
 * padded score row (4 * ceil(M / 4) * 4 bytes) is accepted by nplda_cohort_stats_f32; less gives NPLDA_ENOSPC. */
size_t nplda_cohort_workspace_bytes(int64_t R, int64_t M);

/* Smallest workspace with which nplda_cohort_stats_f32 takes its FUSED path for this shape (statistics formed in the
 * score GEMM's epilogue, no score matrix: csrc/nplda_cohort_fused.hip) — 0 when the shape is not eligible (M < 4096,
 * a top-N too large for the candidate lists).  With less workspace the spilling path is used; both are exact, they differ
 * in the last bits of the fp64 means (different summation orders). */
size_t nplda_cohort_fused_min_workspace_bytes(int64_t M, int topn, int D1, int D2);
/* Workspace for THIS call's parameters: the fused path's lists when the shape is eligible (a few KB per row), else the
 * spilled matrix as nplda_cohort_workspace_bytes. */
size_t nplda_cohort_workspace_bytes_ex(int64_t R, int64_t M, int topn, int D1, int D2);

/* Cohort score matrix + per-row statistics.  z_rows (R, ldz) / q_rows (R) and z_coh (M, ldz) / q_coh (M)
 * come from nplda_embed_f32.  For every row r: stats[4r..4r+3] = (mean, std, mean_top, std_top) of the M
 * cohort scores S[r, m] = NeuralPlda score of (row r, cohort m); std is the population std (ddof = 0);
 * "top" = the topn SMALLEST scores when select_lowest != 0 (the reference's behaviour:
 * adaptive_score_normalization.py:32-36 sorts ascending and keeps [:N]) or the topn largest otherwise.
 * The reference does not compute cohort scores at all (it reads a TSV, :27): this is new functionality.
 * Arithmetic of the fused path at D2 in 145 .. 176 (round 6): the GEMM takes each fp32 operand as three bf16 pieces and forms
 * a product from six bf16 MFMA passes with fp32 accumulation — the same fp32 products to rounding (dropped terms < 2^-26 of a
 * product); the environment variable NPLDA_COHORT_SPLIT=0, read at every call, selects fp32-input MFMAs instead. */
int nplda_cohort_stats_f32(const float* z_rows, const float* q_rows, int64_t R, const float* z_coh,
                           const float* q_coh, int64_t M, int64_t ldz, const void* packed, int D0, int D1,
                           int D2, int topn, int select_lowest, double* stats, void* ws, size_t ws_bytes,
                           nplda_stream_t stream);

/* A PREPARED cohort.  One cohort serves every trial list scored against it (utils/adaptive_score_normalization.py:27-36 reads
 * ONE cohort score table for all its trials), but the part of nplda_cohort_stats_f32 that depends on the cohort only — its
 * second and first moments, folded with P into the covariance image the row thresholds are proposed from — is redone by
 * every call, and by every rank of a row-sharded call.  nplda_cohort_prepare_f32 leaves it in `state`
 * (nplda_cohort_state_bytes bytes, 256-byte aligned, caller-owned; 0 = this shape takes the spilling path, which has nothing
 * to prepare); nplda_cohort_stats_prepared_f32 is nplda_cohort_stats_f32 reading it from there: same statistics, bit for bit.
 * The state is valid for the (z_coh, q_coh, packed, topn) it was prepared with. */
size_t nplda_cohort_state_bytes(int64_t M, int topn, int D1, int D2);
int nplda_cohort_prepare_f32(const float* z_coh, const float* q_coh, int64_t M, int64_t ldz, const void* packed, int D0,
                             int D1, int D2, int topn, void* state, size_t state_bytes, nplda_stream_t stream);
int nplda_cohort_stats_prepared_f32(const float* z_rows, const float* q_rows, int64_t R, const float* z_coh,
                                    const float* q_coh, int64_t M, int64_t ldz, const void* packed, int D0, int D1,
                                    int D2, int topn, int select_lowest, double* stats, void* ws, size_t ws_bytes,
                                    const void* state, size_t state_bytes, nplda_stream_t stream);

/* The row-statistics half alone, on a caller-provided (R, lds) fp32 score matrix (e.g. cohort scores
 * parsed from the TSV the reference consumes, adaptive_score_normalization.py:27-36). */
int nplda_row_stats_f32(const float* S, int64_t lds, int64_t R, int64_t M, int topn, int select_lowest,
                        double* stats, nplda_stream_t stream);

/* Per trial i: out[4i..4i+3] = (znorm, tnorm, snorm, asnorm1) of raw[i] given the statistics rows ie[i]
 * (enroll) and it[i] (test) (adaptive_score_normalization.py:65-73).  fp64 like the reference script. */
int nplda_asnorm_apply_f64(const double* raw, const int64_t* ie, const int64_t* it, int64_t T,
                           const double* stats, int64_t R, double* out, nplda_stream_t stream);

/* ---- GaussianBackend (utils/models.py:571-601) ------------------------------------------------------ */

/* Bytes of the packed GaussianBackend image for a D0 -> D1 LDA (pair dimension 2 D1). 0 if unsupported. */
size_t gb_packed_bytes(int D0, int D1);

/* Pack centering_and_LDA.weight (D1, D0) / .bias (D1) and the paired statistics paired_mean_target (2 D1),
 * paired_cov_inv_target (2 D1, 2 D1), paired_mean_nontarget, paired_cov_inv_nontarget
 * (utils/models.py:574-580) into the fragment-ordered image; folds M = L_n - L_t, v, c (fp64). */
int gb_pack_params_f32(const float* W1, const float* b1, const float* mu_t, const float* Lam_t,
                       const float* mu_n, const float* Lam_n, int D0, int D1, void* packed,
                       size_t packed_bytes, nplda_stream_t stream);

/* Same image for an explicit quadratic form on x = [y1; y2]: S = x^T M x + x^T v + c with M (2 D1, 2 D1) row-major,
 * v (2 D1) or NULL, c a host scalar.  DPlda.forward (utils/models.py:484-495) is this form: its 2 D^2 + D outer-product
 * features times a single linear unit collapse to M = [[Ww, Wb], [Wb, Ww]], v = [ws; ws], c = bias — the 57 970
 * features per pair the reference materialises are never formed. */
int gb_pack_quadform_f32(const float* W1, const float* b1, const float* M, const float* v, float c, int D0, int D1,
                         void* packed, size_t packed_bytes, nplda_stream_t stream);

/* The same image straight from DPlda's parameters: wlr = logistic_regres.weight (1, 2 D1^2 + D1) laid out
 * [Wb | Ww | ws] as utils/models.py:484-490 concatenates the features, blr = logistic_regres.bias (1); both DEVICE
 * pointers (no host read of the bias, so a training loop stays asynchronous). */
int gb_pack_dplda_f32(const float* W1, const float* b1, const float* wlr, const float* blr, int D0, int D1,
                      void* packed, size_t packed_bytes, nplda_stream_t stream);

/* GaussianBackend.forward(x1, x2) -> s (B) (utils/models.py:584-593) and/or
 * GaussianBackend.forward_getpaired(x1, x2) -> paired (B, 2 D1) contiguous (utils/models.py:595-601).
 * Either output pointer may be NULL (not both). */
int gb_score_pairs_f32(const float* x1, const float* x2, int64_t B, int64_t ldx, const void* packed,
                       int D0, int D1, float* s, float* paired, nplda_stream_t stream);

/* gb_score_pairs_f32 that also returns rn (2 B) = 1 / max(||LDA x||, 1e-12) (x1 side rows, then x2 side): what a
 * backward through the LDA layer needs next to the paired rows.  rn may be NULL. */
int gb_score_pairs_ex_f32(const float* x1, const float* x2, int64_t B, int64_t ldx, const void* packed,
                          int D0, int D1, float* s, float* paired, float* rn, nplda_stream_t stream);

/* The same score WITHOUT the normalisation step: rows of y1/y2 are used as layer-1 inputs as they are, i.e.
 * s = x^T M x + x^T v + c with x = [W1 y1 + b1; W1 y2 + b1].  With W1 = I (D0 = padded D1), b1 = 0 this is
 * DPlda.forward_from_plda_embeddings (utils/models.py:484-490) on already-extracted embeddings. */
int gb_score_rows_f32(const float* y1, const float* y2, int64_t B, int64_t ldy, const void* packed, int D0, int D1,
                      float* s, nplda_stream_t stream);

/* ---- weighted moments of paired rows (Gaussian-backend statistics, DPlda weight gradient) ---------------------- */

/* For c in {0, 1} (w1 may be NULL -> only c = 0):
 *     cnt[c] = sum_k w_c[k],  sum[c][i] = sum_k w_c[k] x[k][i],  sq[c][i][j] = sum_k w_c[k] x[k][i] x[k][j]
 * over the B rows of x (B, ldx), n valid columns.  Replaces the per-batch `x[mask].sum(0)` / `x[mask].t() @ x[mask]`
 * accumulation of xvector_GaussianBackend_pytorch.py:40-52 (w_0 = [t > 0.5], w_1 = [t < 0.5]; accumulate = 1 adds
 * into the outputs so batches can be streamed) and, with w_0 = dL/ds, yields the gradient of DPlda's linear unit
 * (utils/models.py:484-490) without the 2 D^2 + D features.  Products in exact fp32 on MFMA, reduction over the
 * row groups in fp64; outputs are DEVICE doubles: cnt (2), sum (2, n), sq (2, n, n) [first half only if w1 == NULL].
 * Requires n % 4 == 0, n <= 2 * nplda_max_dim(), ldx % 4 == 0, x 16-byte aligned. */
size_t nplda_moments_workspace_bytes(int64_t B, int n);
int nplda_weighted_moments_f32(const float* x, int64_t B, int64_t ldx, int n, const float* w0, const float* w1,
                               double* cnt, double* sum, double* sq, int accumulate, void* workspace,
                               size_t workspace_bytes, nplda_stream_t stream);
/* Gradient of DPlda's linear unit from the paired rows x_k = [y1 | y2] (B, ld >= 2 D1) and g = dL/ds:
 * dw (2 D1^2 + D1) = [G12 + G21 | G11 + G22 | s1 + s2], db (1) = sum g, G = sum_k g_k x_k x_k^T  (utils/models.py:484-490;
 * xvector_DPlda_pytorch.py:140-152 trains exactly these).  Same bits as nplda_weighted_moments_f32 followed by the fold in
 * fp64 and one rounding; workspace: nplda_moments_workspace_bytes(B, 2 D1). */
int nplda_dplda_grad_f32(const float* paired, int64_t B, int64_t ld, int D1, const float* g, float* dw, float* db,
                         void* workspace, size_t workspace_bytes, nplda_stream_t stream);

/* The tail of the recipe step xvector_DPlda_pytorch.py:35-43 runs (DPlda.forward -> loss -> backward -> Adam on
 * logistic_regres, the LDA frozen, :140-147) in TWO launches: the weighted moments of the paired rows, then per element of
 * [logistic_regres.weight | .bias] the gradient fold of nplda_dplda_grad_f32, torch.optim.Adam's update (the arithmetic of
 * nplda_adam_step_f32; exp_avg / exp_avg_sq: 2 D1^2 + D1 + 1 + K floats each, [weight | bias | thresholds]; step[0] counts
 * the steps, incremented here) and the store of the new value into the parameter AND into `image`, the quadratic-form image
 * of gb_pack_dplda_f32 the next forward scores with (NULL: not kept).  K thresholds (SoftCdet; dtheta from the loss call)
 * take their Adam step in the same launch.  grad_out (optional, 2 D1^2 + D1 + 1): the applied gradient.
 * loss / loss_sum (optional, ABI 4): loss_sum[0] += loss[0], the device-side running sum behind the progress line of
 * xvector_DPlda_pytorch.py:44-50 (mean of the losses since the previous line) — one launch less per step than adding it
 * from the host side. */
int nplda_dplda_update_f32(const float* paired, int64_t B, int64_t ld, int D1, const float* g, float* wlr, float* blr,
                           float* exp_avg, float* exp_avg_sq, float* const* thetas, const float* dtheta, int K, float* step,
                           float lr, float beta1, float beta2, float eps, float weight_decay, void* image, int D0,
                           float* grad_out, const float* loss, double* loss_sum, void* workspace, size_t workspace_bytes,
                           nplda_stream_t stream);

/* nplda_dplda_update_f32 with the LOSS inside its first launch (round 6): the weights of the moments are dL/ds_i of
 * utils/models.py:384-399's loss (kind 0 = SoftCdet with loss_K thresholds `loss_theta` and HOST betas, 1 = BCE with
 * loss_theta[0]), formed by the moments blocks from (s, t) with the device functions of nplda_loss_fwd_bwd_f32, and ONE more
 * block of that launch is the loss kernel itself: `sums` (nplda_loss_nsums doubles), `loss`, `dtheta` (and dL/ds into g_out
 * when it is not NULL) come out exactly as nplda_loss_fwd_bwd_f32 gives them.  The step xvector_DPlda_pytorch.py:35-43 runs
 * is then THREE launches: score | moments + loss | fold + Adam.  B <= 4096, s / t 16-byte aligned (else
 * NPLDA_EUNSUPPORTED: run the two calls).  `thetas` (K, may be 0): the thresholds that take their Adam step from `dtheta`. */
int nplda_dplda_update_loss_f32(const float* paired, int64_t B, int64_t ld, int D1, const float* s, const float* t, int kind,
                                const float* const* loss_theta, const float* beta, int loss_K, float alpha, double* sums,
                                float* loss, float* dtheta, float* g_out, float* wlr, float* blr, float* exp_avg,
                                float* exp_avg_sq, float* const* thetas, int K, float* step, float lr, float beta1, float beta2,
                                float eps, float weight_decay, void* image, int D0, float* grad_out, double* loss_sum,
                                void* workspace, size_t workspace_bytes, nplda_stream_t stream);

/* ---- detection-cost sweep (validation metrics) -------------------------------------------------------------------- */

/* NeuralPlda.minc (utils/models.py:406-436) for N scores / labels and K <= 8 betas (HOST array), replacing its
 * O(N_tgt * N) Python loop by a device sort + prefix scan + one sweep kernel.
 *   exact = 0: the reference's semantics bit for bit — thresholds swept over the target scores only, counts through
 *              arr2val (:23-27: count - 1, or 1.0 when the set is empty), float32 arithmetic in the reference's order;
 *              minc[k] = min_i P_miss_i + beta_k P_fa_i, thr[k] = the target score attaining it (first occurrence),
 *              minc_avg = sum(minc) / K.
 *   exact = 1: the true minimum of P_miss(th) + beta P_fa(th) over every distinct score and +inf ("target" iff
 *              s >= th), in fp64; eer (optional) = the equal error rate by linear interpolation at the crossing.
 * Labels: target iff t > 0.5, non-target iff t < 0.5 (as :407-408).  With exact = 0 the rates are divided by sum t and
 * sum (1 - t) over ALL labels (as :411,413; exact for labels that are multiples of 2^-24), with exact = 1 by the class
 * counts.  A trial whose score is NaN is in neither class (its label still enters the two sums).
 * minc, thr (K), minc_avg (1), eer (1 or NULL)
 * are DEVICE floats.  N < 2^31.  The workspace size needs no device: for the sort and the scan it reserves
 * max(N, 1) * 14 bytes + 4 MiB from N alone, and the call returns NPLDA_ENOSPC if the sort library asks for more.
 * nplda_detcost_workspace_bytes returns 0 when N is out of range. */
size_t nplda_detcost_workspace_bytes(int64_t N);
int nplda_detcost_sweep_f32(const float* scores, const float* target, int64_t N, const float* betas, int K, int exact,
                            float* minc, float* thr, float* minc_avg, float* eer, void* workspace,
                            size_t workspace_bytes, nplda_stream_t stream);

/* ---- score calibration and fusion (csrc/nplda_calib.hip; counterpart of utils/score_calibration.py) ---------------- */

/* Notation: X (N, K) scores of K <= 8 systems, fp32 (_f32) or fp64 (_f64), row stride ldx >= K elements; target (N)
 * fp32, target iff t > 0.5, non-target iff t < 0.5, neither: the trial is ignored; theta = (a_1 .. a_K, b), K + 1 DEVICE
 * doubles; tau = logit(p_target); z_i = sum_k a_k X_ik + b + tau; w_i = p_target / N_tgt on targets and
 * (1 - p_target) / N_non on non-targets.  All arithmetic is fp64; every sum over trials is a fixed-order tree (no
 * floating-point atomics: the same input gives the same bits) and a plain sum over trials.
 * Every entry point checks its arguments before anything is enqueued: K outside 1 .. 8 or N >= 2^31 ->
 * NPLDA_EUNSUPPORTED; a null pointer, N < 2 (fits, pass) / N < 1 (costs) / N < 0 (apply), ldx < K, p_target outside
 * (0, 1), l2 < 0, a workspace that is null or not 16-byte aligned -> NPLDA_EINVAL; a workspace smaller than
 * nplda_calib_workspace_bytes(N, K) -> NPLDA_ENOSPC.  nplda_calib_workspace_bytes returns 0 for an unsupported size
 * (N < 2, N >= 2^31, K outside 1 .. 8); it does not decrease with N.  gauss_fit and costs take the workspace of K = 1. */
size_t nplda_calib_workspace_bytes(int64_t N, int K);
/* Rows one full sweep of the reduction grid covers (blocks x threads): above it a lane sums more than one trial. */
int nplda_calib_sweep_rows(void);

/* One pass of the prior-weighted logistic objective at theta.  out (DEVICE doubles, 2 + 1 + (K + 1) + (K + 1)(K + 2) / 2):
 *   N_tgt, N_non,
 *   J = sum_i w_i softplus(-z_i | target, +z_i | non-target) + (l2 / 2) sum_k a_k^2,
 *   g = sum_i w_i (sigma(z_i) - t_i) [X_i, 1] + l2 [a, 0]                                   (K + 1),
 *   H = sum_i w_i sigma_i (1 - sigma_i) [X_i, 1][X_i, 1]^T + l2 diag(1 .. 1, 0), upper triangle by rows.
 * softplus and sigma are evaluated in their overflow-safe forms. */
int nplda_calib_logreg_pass_f32(const float* X, int64_t N, int64_t ldx, int K, const float* target, const double* theta,
                                double p_target, double l2, double* out, void* workspace, size_t workspace_bytes,
                                nplda_stream_t stream);
int nplda_calib_logreg_pass_f64(const double* X, int64_t N, int64_t ldx, int K, const float* target, const double* theta,
                                double p_target, double l2, double* out, void* workspace, size_t workspace_bytes,
                                nplda_stream_t stream);

/* Damped Newton fit: enqueues a FIXED budget of max_passes (1 .. 256) pairs of launches (pass | finish + step) on the
 * stream with no host synchronisation; the step solves H d = g by Cholesky, accepts theta - alpha d if J did not
 * increase (beyond 8 ulp of J, the rounding of the sum) and halves alpha otherwise, at most 20 times in a row.  Once a
 * stop flag is set the remaining launches return at once.  theta (in: the start, out: ALWAYS the last accepted value).
 * resume = 0 starts a fit; resume = 1 continues the fit whose state is in `workspace` with another budget (so that a
 * caller can enqueue the budget in pieces and look at the flags in between).  report (10 DEVICE doubles): J and
 * max |g_k| at theta, iterations (accepted Newton directions), passes, converged (max |g_k| <= tol), not_finite (J, g or H
 * not finite, an empty class, or the Cholesky failed), stalled (20 halvings did not lower J), N_tgt, N_non, last alpha. */
int nplda_calib_logreg_fit_f32(const float* X, int64_t N, int64_t ldx, int K, const float* target, double* theta,
                               double p_target, double l2, int max_passes, double tol, int resume, double* report,
                               void* workspace, size_t workspace_bytes, nplda_stream_t stream);
int nplda_calib_logreg_fit_f64(const double* X, int64_t N, int64_t ldx, int K, const float* target, double* theta,
                               double p_target, double l2, int max_passes, double tol, int resume, double* report,
                               void* workspace, size_t workspace_bytes, nplda_stream_t stream);

/* One Gaussian per class (utils/score_calibration.py:14-24).  out (6 DEVICE doubles): count, mean and POPULATION
 * standard deviation (ddof = 0, np.std) of the targets, then of the non-targets; two passes (sums, then squared
 * deviations about the means), an empty class gives NaN. */
int nplda_calib_gauss_fit_f32(const float* scores, const float* target, int64_t N, double* out, void* workspace,
                              size_t workspace_bytes, nplda_stream_t stream);
int nplda_calib_gauss_fit_f64(const double* scores, const float* target, int64_t N, double* out, void* workspace,
                              size_t workspace_bytes, nplda_stream_t stream);

/* out_i = sum_k a_k X_ik + b (one fma chain from b); out: N floats (out_f64 = 0) or doubles (out_f64 = 1). */
int nplda_calib_apply_linear_f32(const float* X, int64_t N, int64_t ldx, int K, const double* theta, void* out,
                                 int out_f64, nplda_stream_t stream);
int nplda_calib_apply_linear_f64(const double* X, int64_t N, int64_t ldx, int K, const double* theta, void* out,
                                 int out_f64, nplda_stream_t stream);

/* out_i = log std_imp - log std_tgt - (s - mu_tgt)^2 / (2 std_tgt^2) + (s - mu_imp)^2 / (2 std_imp^2), in this form
 * (utils/score_calibration.py:26-28: the difference of two normal log densities).  Standard deviations that are not
 * positive and finite, or a mean that is not finite -> NPLDA_EINVAL. */
int nplda_calib_apply_gauss_f32(const float* scores, int64_t N, double mu_tgt, double std_tgt, double mu_imp,
                                double std_imp, void* out, int out_f64, nplda_stream_t stream);
int nplda_calib_apply_gauss_f64(const double* scores, int64_t N, double mu_tgt, double std_tgt, double mu_imp,
                                double std_imp, void* out, int out_f64, nplda_stream_t stream);

/* Calibration-sensitive costs of N log-likelihood ratios at nth <= 8 thresholds (HOST doubles, +-inf allowed, NaN ->
 * NPLDA_EINVAL).  counts (2 + 2 nth DEVICE int64): N_tgt, N_non, misses (llr < th on a target) per threshold, false
 * alarms (llr >= th on a non-target) per threshold — the decision rule of nplda_detcost_sweep_f32's exact mode.
 * sums (2 DEVICE doubles): sum_tgt log2(1 + exp(-llr)), sum_non log2(1 + exp(llr)) — Cllr = (sums[0] / N_tgt +
 * sums[1] / N_non) / 2. */
int nplda_calib_costs_f32(const float* llr, const float* target, int64_t N, const double* thresholds, int nth,
                          int64_t* counts, double* sums, void* workspace, size_t workspace_bytes, nplda_stream_t stream);
int nplda_calib_costs_f64(const double* llr, const float* target, int64_t N, const double* thresholds, int nth,
                          int64_t* counts, double* sums, void* workspace, size_t workspace_bytes, nplda_stream_t stream);

/* ---- PAV / ROC convex hull: min Cllr, ROCCH EER, isotonic calibration (csrc/nplda_pav.hip) ----------------------- */

/* The isotonic regression of the labels on the scores, as the strict lower convex hull of the cumulative (trials,
 * targets) diagram of the score bins (design/k18_pav_rocch.md).  scores: N fp32 (_f32) or fp64 (_f64); target as above
 * (neither class: the trial is excluded); a trial whose score is NaN is excluded too, +-inf are scores.  Equal scores
 * (==) form one bin.  laplace != 0 adds a bin (n = 2, t = 1) at -inf and one at +inf before the hull.
 * Block table, DEVICE arrays of `cap` >= 1 entries: lo, hi (first and last score of the block's real bins; a block made
 * of a dummy bin alone has lo = hi = -+inf), n, t (trials and targets, dummy trials included) and
 * llr = log(t / (n - t)) - log(N_t' / N_n') with N' the class counts (+ 2 each under the Laplace rule).
 * summary, 8 DEVICE doubles: N_t, N_n (real trials kept), M (bins), nb (blocks: always the true number), min Cllr and
 * the ROCCH equal error rate of THIS block table (NaN when a class is empty), an overflow flag (nb > cap: the blocks
 * beyond cap were not written), 0.
 * Everything is enqueued on `stream`; nothing is read back and the number of launches depends on N only; the result is
 * bitwise repeatable (integer hull decisions, fixed-order fp64 sums).
 * A null pointer, a pointer that is not aligned to its type (workspace: 16 bytes), N < 2 or cap < 1 -> NPLDA_EINVAL;
 * N >= 2^31 -> NPLDA_EUNSUPPORTED; workspace_bytes < nplda_pav_workspace_bytes(N, is_f64) -> NPLDA_ENOSPC; all before
 * anything is enqueued.  nplda_pav_workspace_bytes needs no device, returns 0 for N < 2 or N >= 2^31 and does not
 * decrease with N. */
int nplda_pav_chunk(void); /* points one thread scans at level 0 of the hull: tests straddle its multiples */
size_t nplda_pav_workspace_bytes(int64_t N, int is_f64);
int nplda_pav_fit_f32(const float* scores, const float* target, int64_t N, int laplace, double* lo, double* hi, int64_t* n,
                      int64_t* t, double* llr, int64_t cap, double* summary, void* workspace, size_t workspace_bytes,
                      nplda_stream_t stream);
int nplda_pav_fit_f64(const double* scores, const float* target, int64_t N, int laplace, double* lo, double* hi, int64_t* n,
                      int64_t* t, double* llr, int64_t cap, double* summary, void* workspace, size_t workspace_bytes,
                      nplda_stream_t stream);

/* For stage timing (tools/bench_pav.py): nplda_pav_fit_f32 cut short after the sort and scan (stop_after = 1), the
 * binning (2) or the hull (3); 0 runs everything.  Outputs are written by the full run only. */
int nplda_pav_fit_stages_f32(const float* scores, const float* target, int64_t N, int laplace, double* lo, double* hi,
                             int64_t* n, int64_t* t, double* llr, int64_t cap, double* summary, void* workspace,
                             size_t workspace_bytes, int stop_after, nplda_stream_t stream);

/* out_i = the table's llr at scores_i: llr_b inside a block (lo_b <= s <= hi_b, the first such block), the first / last
 * block's beyond the ends, linear in s across a gap with two finite ends (clamped to [llr_b, llr_b+1]; an infinite llr
 * at either end of the gap is taken as it is, the left one first), the llr of the block on the infinite side of a gap
 * with one infinite end, NaN for NaN.  lo, hi, llr: nb >= 1 DEVICE doubles; out: N floats (out_f64 = 0) or doubles.
 * N < 0, nb < 1, a null or misaligned pointer -> NPLDA_EINVAL; N or nb >= 2^31 -> NPLDA_EUNSUPPORTED; N = 0 does
 * nothing. */
int nplda_pav_apply_f32(const float* scores, int64_t N, const double* lo, const double* hi, const double* llr, int64_t nb,
                        void* out, int out_f64, nplda_stream_t stream);
int nplda_pav_apply_f64(const double* scores, int64_t N, const double* lo, const double* hi, const double* llr, int64_t nb,
                        void* out, int out_f64, nplda_stream_t stream);

/* ---- group bootstrap of EER, min cost, actual cost and Cllr (csrc/nplda_bootstrap.hip) -------------------------------- */

/* B bootstrap replicates of the detection metrics over ONE sorted trial list (design/k20_bootstrap.md).  scores, target:
 * N fp32 (target as above; a trial with a NaN score is excluded); g1, g2: N int32 group ids of the two trial sides in
 * [0, G1) and [0, G2); g2 = NULL with G2 = 0 resamples side 1 alone.  Replicate b = 1 .. B draws G1 (and G2) groups with
 * replacement from the counter-based generator of the design note (splitmix64 finaliser, keyed by seed, b and the side);
 * a trial weighs the product of the draw counts of its two groups.  Row 0 is the point estimate (all weights 1).
 * out: (B + 1) x ncol DEVICE doubles, ncol = K + 1 + (is_llr ? K + 1 : 0): min cost at betas[0 .. K) (every distinct
 * score and +inf as threshold, target iff s >= th), the interpolated EER of nplda_detcost_sweep_f32's exact mode, then
 * with is_llr P_miss + beta P_fa at the threshold log(beta) and Cllr in bits.  totals: (B + 1) x 2 DEVICE int64, the
 * weighted N_tgt, N_non.  A replicate with an empty class has NaN in every column; nothing else produces a NaN.
 * betas: K HOST doubles.  After the call the first 16 bytes of the workspace hold two DEVICE int64 flags: the number of
 * trials whose group id was out of range (such a trial is excluded, never used as an index) and the number of draw
 * counts above 255 (stored saturated: the result is then not the bootstrap's).
 * Everything is enqueued on `stream`; nothing is read back, the number of launches depends on (N, B, G1, G2) only and
 * the result is bitwise repeatable (integer atomics and counts, fixed-order fp64 sums).
 * Limits: 2 <= N < 2^31, 1 <= G1 <= 2^20, G2 <= 2^20, 1 <= B <= 2^20, 1 <= K <= 8.  Before anything is enqueued: a null
 * pointer (other than g2 with G2 = 0; g2 given with G2 = 0 as well), a pointer not aligned to its type (workspace: 16
 * bytes), N < 2, B < 1, G1 < 1, G2 < 0, K < 1, a beta that is not positive and finite -> NPLDA_EINVAL; a size past the
 * limits -> NPLDA_EUNSUPPORTED; workspace_bytes < nplda_bootstrap_workspace_bytes(N, G1, G2, B) -> NPLDA_ENOSPC.
 * nplda_bootstrap_workspace_bytes needs no device, returns 0 outside the limits, does not decrease with N and does not
 * depend on B inside them (the replicates are processed in tiles that reuse one table and one set of partials). */
size_t nplda_bootstrap_workspace_bytes(int64_t N, int64_t G1, int64_t G2, int B);
int nplda_bootstrap_run(void);  /* sorted positions one wave walks (per-run partials): tests straddle its multiples */
int nplda_bootstrap_tile(void); /* replicates per tile, row 0 included: tests straddle its multiples */
int nplda_bootstrap_f32(const float* scores, const float* target, const int32_t* g1, const int32_t* g2, int64_t N, int64_t G1,
                        int64_t G2, int B, uint64_t seed, const double* betas, int K, int is_llr, double* out,
                        int64_t* totals, void* workspace, size_t workspace_bytes, nplda_stream_t stream);

/* ---- host-side text I/O of the trial-list path (no device work; plain host pointers) ------------------------------ */

/* Rows and columns of a whitespace-separated table held in memory, with np.genfromtxt(dtype=str) semantics (the
 * reader of utils/scorefile_generator.py:26,45 and utils/sv_trials_loaders.py:377,400): any run of blanks separates
 * columns, '#' starts a comment, blank lines are skipped.  Returns the number of data rows (>= 0) and their column
 * count in *ncols, or NPLDA_EINVAL when rows have different column counts (genfromtxt raises there). */
int64_t nplda_text_scan(const char* text, size_t len, int* ncols);

/* Resolve columns 0 and 1 of every data row after the first skip_rows to numbers through an id table, replacing the
 * per-trial Python loops of utils/sv_trials_loaders.py:379-383 / :402-406 (dict look-ups, float(label)) and :432-433
 * (basename / splitext per id).  mode1 / mode2: 0 = id as written, 1 = os.path.splitext(id)[0],
 * 2 = os.path.splitext(os.path.basename(id))[0], 3 = id.replace('.sph', '') (utils/adaptive_score_normalization.py:25).
 * ids: n_ids ids separated by single '\n' bytes, id i =
 * ids[id_off[i] .. id_off[i+1] - 1) (id_off has n_ids + 1 entries); a repeated id resolves to its last occurrence
 * (dict semantics).  id_num (n_ids) maps a table position to the number stored (NULL: the position itself).
 * label_col >= 0: that column is parsed like Python's float() into label.  Rows with an unknown id, an unparsable
 * label or too few columns are skipped, as the reference's bare `except: pass` does; *first_bad_row (optional) gets
 * the first such row (relative to skip_rows) or -1, so that a caller with KeyError semantics (:433) can raise.
 * Outputs have room for every data row; *n_kept rows are written; row_of (optional) = source row of each. */
int nplda_text_lookup(const char* text, size_t len, int64_t skip_rows, int mode1, int mode2, int label_col,
                      const char* ids, const int64_t* id_off, const int64_t* id_num, int64_t n_ids, int64_t* i1,
                      int64_t* i2, float* label, int64_t* row_of, int64_t* n_kept, int64_t* first_bad_row);

/* Write a score file: optional header line, then for each of the first n data rows after skip_rows its first
 * keep_cols columns joined by tabs, a tab, and the score formatted as str(np.float32) (scores_f64 = 0, float array)
 * or str(np.float64) (scores_f64 = 1, double array) — byte for byte what
 * np.savetxt(np.c_[trials, scores.astype(str)], fmt='%s', delimiter='\t') writes at
 * utils/scorefile_generator.py:38 (keep_cols = all columns, header = columns + "\tLLR"), :55 (keep_cols = 2) and
 * utils/adaptive_score_normalization.py:81-84 (doubles, keep_cols = all but the last, header "# " + columns). */
int nplda_scores_write(const char* path, const char* text, size_t len, int64_t skip_rows, int keep_cols,
                       const char* header, const void* scores, int scores_f64, int64_t n);

/* str(np.float32(v)) / str(np.float64(v)) into out (>= 32 bytes, NUL-terminated); returns the length. */
int nplda_format_f32(float v, char* out);
int nplda_format_f64(double v, char* out);

/* One column (col < 0 counts from the end: -1 = last) of the n data rows after skip_rows parsed like Python's
 * float(): the `.astype(float)` of utils/adaptive_score_normalization.py:24,32.  NPLDA_EINVAL if a token does not
 * parse or the table has fewer / more rows than n. */
int nplda_text_column_f64(const char* text, size_t len, int64_t skip_rows, int col, double* out, int64_t n);

/* Number of distinct tokens in a column: len(np.unique(tab[:, col])) of utils/adaptive_score_normalization.py:28. */
int nplda_text_count_unique(const char* text, size_t len, int64_t skip_rows, int col, int64_t* n_unique);

/* Byte spans (start offset into text, length) of column col in rows skip_rows + k * stride, k = 0..n-1: the row ids
 * of the reshaped cohort table, utils/adaptive_score_normalization.py:38. */
int nplda_text_column_spans(const char* text, size_t len, int64_t skip_rows, int col, int64_t stride, int64_t* start,
                            int64_t* length, int64_t n);

/* ---- optimiser ----------------------------------------------------------------------------------------- */

/* torch.optim.Adam's update (xvector_NeuralPlda_pytorch.py:139: lr, weight_decay = 1e-5 as L2 term, no amsgrad)
 * applied to nseg <= 12 (param, grad, exp_avg, exp_avg_sq) segments in one launch.  The four pointer arrays and
 * numel are HOST arrays of nseg entries (device pointers / element counts).  step: DEVICE buffer of TWO 4-byte words,
 * zero-initialised by the caller: step[0] is the number of steps taken so far as a float (incremented by the launch,
 * the new value is the one used for the bias correction), step[1] is scratch of the launch (an arrival counter, zero
 * between launches).  Graph-replay safe: nothing about the step lives on the host.  A segment of numel == 0 may carry
 * null pointers (a tensor without storage has none); a launch whose segments are all empty only counts the step. */
int nplda_adam_step_f32(float* const* params, const float* const* grads, float* const* exp_avg,
                        float* const* exp_avg_sq, const int64_t* numel, int nseg, float* step, float lr,
                        float beta1, float beta2, float eps, float weight_decay, nplda_stream_t stream);

/* One whole optimisation step on B <= 16384 pairs in THREE launches: forward + loss + data gradients in one kernel (dL/ds
 * of a pair needs its own score / target and the batch counts only) -> weight-gradient slabs ->
 * slab sums + Adam + refreshed fragment image + loss / dL/dtheta / threshold update.  What the reference spends
 * `loss.backward(); optimizer.step()` on (xvector_NeuralPlda_pytorch.py:66-75: ~250 ATen launches).  Same arithmetic as
 * nplda_pack_params_f32 -> nplda_forward_train_f32 -> nplda_loss_fwd_bwd_f32 -> nplda_backward_f32 ->
 * nplda_adam_step_f32; the loss sums are formed per block of 16 pairs (fp64, fixed order).
 *   params:  HOST array of the 6 DEVICE tensors W1 (D1, D0), b1, W2 (D2, D1), b2, P_sqrt, Q — updated in place;
 *   thetas:  HOST array of K device scalars (the thresholds; kind 1 = BCE uses thetas[0]), updated in place;
 *   betas:   HOST array of K floats (kind 0 = SoftCdet);  exp_avg / exp_avg_sq: nplda_grad_floats + K floats each, in
 *            flat-gradient order followed by the thresholds;  step: as nplda_adam_step_f32;
 *   packed:  IN the image of the current parameters (nplda_pack_params_f32), OUT the image of the updated ones — the
 *            caller re-packs only when the parameters were changed by something else;
 *   loss:    device scalar;  grad_out: optional nplda_grad_floats + K floats (the gradient that was applied);
 *   loss_sum: optional device double, loss_sum[0] += loss — the training log prints the MEAN of the losses since its
 *            previous line (xvector_NeuralPlda_pytorch.py:41-47), which a replayed step cannot collect one by one: its
 *            loss lives at one address.  The caller zeroes it when it reads it.
 * NPLDA_EUNSUPPORTED for B > 16384 or the hard cost (kind 2): use the separate entry points. */
size_t nplda_train_step_workspace_bytes(int64_t B, int D0, int D1, int D2);
/* The same step on the pairs (table[rows1[i]], table[rows2[i]]) of a resident (N, ldt) x-vector matrix — the form of the
 * reference's training loop, which looks every pair's two utterances up in mega_xvec_dict (utils/sv_trials_loaders.py:418-437):
 * the first kernel gathers the rows itself (and leaves them in the workspace for the weight gradients), so no gather
 * launch and no (B, D0) staging tensors.  rows1 / rows2: B int64 device indices in [0, N) (the loaders check them; the
 * kernel clamps).  D0 % 16 == 0 (else NPLDA_EUNSUPPORTED: gather with nplda_gather_rows_f32 and call nplda_train_step_f32). */
size_t nplda_train_step_rows_workspace_bytes(int64_t B, int D0, int D1, int D2);
int nplda_train_step_rows_f32(const float* table, int64_t N, int64_t ldt, const int64_t* rows1, const int64_t* rows2,
                              int64_t B, const float* target, float* const* params, int D0, int D1, int D2,
                              float* const* thetas, const float* betas, int K, float alpha, int kind, float* exp_avg,
                              float* exp_avg_sq, float* step, float lr, float beta1, float beta2, float eps,
                              float weight_decay, void* packed, void* ws, size_t ws_bytes, float* loss, double* loss_sum,
                              float* grad_out, nplda_stream_t stream);
/* The same step for a device-resident epoch of batches.  A record is [rows1 (B int64) | rows2 (B int64) | labels (B float32)],
 * 20 B bytes, records back to back (TrialLoader.device_epoch lays an epoch out this way).  The step trains on the record in
 * `stage` (device, 20 B bytes, 16-byte aligned) and its last kernel copies the epoch's NEXT record there: `cursor` is a
 * DEVICE array of three int64 — [0] the address of record 0, [1] the index of the next record to stage, [2] the record
 * count; the first kernel counts cursor[1] up, the update kernel stages record cursor[1] while cursor[1] < cursor[2].  The
 * caller stages record 0 and sets cursor = {base, 0, count} once per epoch; a captured graph of this call then walks the
 * epoch replay by replay with no copy launch and no host write per step (the reference's loop moves three host tensors to
 * the device per batch, xvector_NeuralPlda_pytorch.py:38).  B % 4 == 0 and D0 % 16 == 0 (else NPLDA_EUNSUPPORTED).
 * Workspace: as nplda_train_step_rows_f32. */
int nplda_train_step_records_f32(const float* table, int64_t N, int64_t ldt, int64_t* cursor, void* stage, int64_t B,
                                 float* const* params, int D0, int D1, int D2, float* const* thetas, const float* betas,
                                 int K, float alpha, int kind, float* exp_avg, float* exp_avg_sq, float* step, float lr,
                                 float beta1, float beta2, float eps, float weight_decay, void* packed, void* ws,
                                 size_t ws_bytes, float* loss, double* loss_sum, float* grad_out, nplda_stream_t stream);
int nplda_train_step_f32(const float* x1, const float* x2, int64_t B, int64_t ldx, const float* target,
                         float* const* params, int D0, int D1, int D2, float* const* thetas, const float* betas, int K,
                         float alpha, int kind, float* exp_avg, float* exp_avg_sq, float* step, float lr, float beta1,
                         float beta2, float eps, float weight_decay, void* packed, void* ws, size_t ws_bytes, float* loss,
                         double* loss_sum, float* grad_out, nplda_stream_t stream);

/* The data-parallel form of nplda_train_step_f32: ONE collective per step.  dL/ds_i of SoftCdet / BCE needs the pair's own
 * score and target and the GLOBAL batch's counts N_t, N_n only (utils/models.py:384-399), and a rank that slices its shard
 * out of the global minibatch knows those from the labels — so no collective has to precede the backward:
 *   nplda_train_step_grad_f32   forward + loss terms + data gradients + weight-gradient slabs of this rank's B pairs (the
 *                               same three launches), stopping at flat[0 .. nplda_train_step_flat_floats): the flat
 *                               gradient (nplda_grad_floats order) followed by the rank's fp64 loss sums as 4 x 18 floats
 *                               (four 16-bit fixed-point limbs each: integer-valued floats whose fp32 sum over <= 256
 *                               ranks is exact, so the summed loss sums come back to 2^-41 absolute).  global_counts: device [N_t, N_n] doubles of the global
 *                               batch (NULL: this rank's own counts, i.e. a single rank).  Counts Adam's step; updates nothing
 *                               else.  Workspace: nplda_train_step_workspace_bytes(B, ...).
 *   -- SUM all-reduce of flat (fp32) across the ranks --
 *   nplda_train_step_apply_f32  one launch: Adam on the parameters from flat, the refreshed parameter image, loss and
 *                               dL/dtheta from the summed loss sums, Adam on the thresholds, loss_sum[0] += loss.
 * On one rank the two calls give nplda_train_step_f32's parameters (the same slab sums and update arithmetic; the loss
 * sums pass through the limbs, 2^-41 absolute).  B <= 16384 per rank, <= 256 ranks. */
size_t nplda_train_step_flat_floats(int D0, int D1, int D2);
int nplda_train_step_grad_f32(const float* x1, const float* x2, int64_t B, int64_t ldx, const float* target,
                              const double* global_counts, float* const* params, int D0, int D1, int D2,
                              float* const* thetas, const float* betas, int K, float alpha, int kind, float* step,
                              void* packed, void* ws, size_t ws_bytes, float* flat, nplda_stream_t stream);
/* (the gradient phase on the pairs (table[rows1], table[rows2]) of a resident x-vector matrix, as nplda_train_step_rows_f32;
 * workspace: nplda_train_step_rows_workspace_bytes) */
int nplda_train_step_grad_rows_f32(const float* table, int64_t N, int64_t ldt, const int64_t* rows1, const int64_t* rows2,
                                   int64_t B, const float* target, const double* global_counts, float* const* params, int D0,
                                   int D1, int D2, float* const* thetas, const float* betas, int K, float alpha, int kind,
                                   float* step, void* packed, void* ws, size_t ws_bytes, float* flat, nplda_stream_t stream);
/* (the gradient phase of the head's end-to-end step, as nplda_train_step_dx_f32: x1 / x2 and dx1 / dx2 float32 or, with
 * io_bf16, bfloat16; dL/dx of this rank's rows is complete after this call — it depends on the other ranks through the global
 * counts only; workspace: nplda_train_step_dx_workspace_bytes) */
int nplda_train_step_grad_dx_f32(const void* x1, const void* x2, int64_t B, int64_t ldx, int io_bf16, const float* target,
                                 const double* global_counts, float* const* params, int D0, int D1, int D2,
                                 float* const* thetas, const float* betas, int K, float alpha, int kind, float* step,
                                 void* packed, void* ws, size_t ws_bytes, float* flat, void* dx1, void* dx2, int64_t lddx,
                                 nplda_stream_t stream);
int nplda_train_step_apply_f32(const float* flat, float* const* params, int D0, int D1, int D2, float* const* thetas,
                               const float* betas, int K, float alpha, int kind, float* exp_avg, float* exp_avg_sq,
                               float* step, float lr, float beta1, float beta2, float eps, float weight_decay, void* packed,
                               float* loss, double* loss_sum, nplda_stream_t stream);

/* The head's step of an end-to-end fine-tune (BASELINE configs[4]; the reference chains an x-vector extractor into this head:
 * Etdnn_Xvec_NeuralPlda, utils/models.py:251-268, and autograd hands dL/dx back to it): nplda_train_step_f32 that also returns
 * dx1, dx2 (B, lddx) = dL/dx1, dL/dx2 = du . W1 with the weights the forward used — four launches: forward + loss + data
 * gradients, weight-gradient slabs, the input-gradient product, update.  io_bf16 != 0: x1, x2 are bfloat16 rows (ldx in
 * elements) and dx1, dx2 are written in bfloat16 (round to nearest even) — the dtype a bf16 extractor works in; the head's own
 * arithmetic stays fp32 (the rows are widened exactly).  io_bf16 needs D0 == 512 and D1, D2 in 145..192.  B <= 16384.
 * Workspace: nplda_train_step_dx_workspace_bytes. */
size_t nplda_train_step_dx_workspace_bytes(int64_t B, int D0, int D1, int D2, int io_bf16);
int nplda_train_step_dx_f32(const void* x1, const void* x2, int64_t B, int64_t ldx, int io_bf16, const float* target,
                            float* const* params, int D0, int D1, int D2, float* const* thetas, const float* betas, int K,
                            float alpha, int kind, float* exp_avg, float* exp_avg_sq, float* step, float lr, float beta1,
                            float beta2, float eps, float weight_decay, void* packed, void* ws, size_t ws_bytes, float* loss,
                            double* loss_sum, float* grad_out, void* dx1, void* dx2, int64_t lddx, nplda_stream_t stream);

/* ---- split-bf16 scoring (opt-in) --------------------------------------------------------------------------- */

/* Same functions as nplda_pack_params_f32 / nplda_score_pairs_f32 / nplda_embed_f32 computed on the bf16 matrix
 * pipe with every fp32 operand split into three bf16 pieces and six MFMA passes per product (csrc/nplda_fwd_bf16x3.h):
 * fp32-class accuracy (the dropped cross terms are <= 2^-23 relative; scores within the same 2e-5 + 1e-5 |s| tolerance
 * of the fp64 oracle), ~1.5x the throughput of the exact-fp32 kernels.  Uses its own packed image. */
size_t nplda_bf16x3_packed_bytes(int D0, int D1, int D2);
int nplda_pack_params_bf16x3(const float* W1, const float* b1, const float* W2, const float* b2,
                             const float* P_sqrt, const float* Q, int D0, int D1, int D2, void* packed,
                             size_t packed_bytes, nplda_stream_t stream);
int nplda_score_pairs_bf16x3(const float* x1, const float* x2, int64_t B, int64_t ldx, const void* packed,
                             int D0, int D1, int D2, float* s, nplda_stream_t stream);
int nplda_embed_bf16x3(const float* x, int64_t N, int64_t ldx, const void* packed, int D0, int D1, int D2,
                       float* z, int64_t ldz, float* q, nplda_stream_t stream);

/* ---- E-TDNN x-vector extractor (utils/models.py:29-214) ------------------------------------------------------ */

/* XVectorNet_ETDNN_12Layer.extract (utils/models.py:170-186): MFCC frames -> 512-d x-vectors, exact fp32 MFMA
 * (csrc/nplda_xvec.hip).  tdnn1..tdnn10 (unfold c frames at dilation d, nn.Linear, ReLU, eval-mode
 * BatchNorm1d(affine=False)), statistics pooling [mean | unbiased std or var] over time, lin11 (affine only).
 * An utterance of T frames yields T - 22 pooled frames; T = 23 gives NaN std / var, as the reference does. */
#define NPLDA_XVEC_LAYOUT_ROWS 0  /* x: (total_frames, 30) rows with row stride ld_in >= 30                    */
#define NPLDA_XVEC_LAYOUT_BCT  1  /* x: the reference's (n_utts, 30, T) contiguous, T = total_frames / n_utts  */
#define NPLDA_XVEC_POOL_STD    0  /* pooling_function = torch.std (default)                                  */
#define NPLDA_XVEC_POOL_VAR    1  /* pooling_function = torch.var (E2EConf pooling_function = var)           */

/* Bytes of the packed extractor image (fixed architecture, 24.5 MB). */
size_t nplda_xvec_packed_bytes(void);
/* Pack the extractor's parameters.  W, b: HOST arrays of 11 device pointers, tdnn1..tdnn10 kernel.weight (Dout,
 * c * Din) / kernel.bias, then lin11.weight (512, 3000) / lin11.bias; running_mean, running_var: host arrays of 10
 * device pointers (tdnn<i>.bn); eps: host array of 10 floats.  Batch norm is folded as (mean, 1 / sqrt(var + eps)). */
int nplda_xvec_pack_f32(const float* const* W, const float* const* b, const float* const* running_mean,
                        const float* const* running_var, const float* eps, void* packed, size_t packed_bytes,
                        nplda_stream_t stream);
/* Workspace of one nplda_xvec_extract_f32 call over total_frames frames of n_utts utterances (8 KB per frame plus
 * 12 KB per utterance, rounded to whole tiles). */
size_t nplda_xvec_workspace_bytes(int64_t total_frames, int64_t n_utts);
/* out[u, 0:512] = extract(utterance u) for u < n_utts.  offsets: int64 device array of n_utts + 1 frame offsets
 * (utterance u is frames [offsets[u], offsets[u+1]), each at least 23 frames long for a finite result; for LAYOUT_BCT
 * offsets[u] = u T).  out: (n_utts, ldx), ldx >= 512, ldx % 4 == 0.  Every layer runs over all frames in one launch; an
 * utterance's result does not depend on the rest of the batch (bit for bit).  The caller's x is read only inside its
 * total_frames rows. */
int nplda_xvec_extract_f32(const float* x, int layout, int64_t ld_in, const int64_t* offsets, int64_t n_utts,
                           int64_t total_frames, int pooling, const void* packed, float* out, int64_t ldx, void* ws,
                           size_t ws_bytes, nplda_stream_t stream);

/* Sliding-window extraction (design/k23_sliding_windows.md): x-vectors of n_windows row ranges of ONE dense pass over
 * x, for diarization.  Workspace of one call: the dense buffers of total_frames frames plus 3008 floats per window,
 * rounded to whole tiles (the same formula as nplda_xvec_workspace_bytes(total_frames, n_windows)). */
size_t nplda_xvec_windows_workspace_bytes(int64_t total_frames, int64_t n_windows);
/* out[w, 0:512] = extract(rows [win_begin[w], win_end[w]) of x as one utterance) for w < n_windows, bit for bit what
 * nplda_xvec_extract_f32 gives for a copy of those rows.  x: (total_frames, ld_in) rows (NPLDA_XVEC_LAYOUT_ROWS only);
 * win_begin, win_end: int64 device arrays of row indices into x.  The caller promises that the rows of a window are
 * consecutive frames of one recording; windows may overlap, repeat and come in any order.  tdnn1..tdnn10 run ONCE over
 * the total_frames rows, whatever the windows cover; a pooling kernel then takes, per window, the dense tdnn10 rows
 * [begin, end - 22): fp64 sum in row order, mean, fp64 sum of squared deviations in row order, unbiased std or var (NaN
 * at one pooled row), as the utterance pooling does; lin11 runs over the n_windows pooled rows.  Indices are clamped to
 * [0, total_frames]; a window with end - begin <= 22 after clamping yields NaN pooled values (a NaN x-vector) and reads
 * no row.  out: (n_windows, ldx), ldx >= 512, ldx % 4 == 0.  n_windows == 0 returns NPLDA_OK and touches nothing. */
int nplda_xvec_extract_windows_f32(const float* x, int64_t ld_in, int64_t total_frames, const int64_t* win_begin,
                                   const int64_t* win_end, int64_t n_windows, int pooling, const void* packed, float* out,
                                   int64_t ldx, void* ws, size_t ws_bytes, nplda_stream_t stream);

/* Training forward and backward of the same extractor (csrc/nplda_xvec_bwd.hip), for fine-tuning it end to end under
 * Etdnn_Xvec_NeuralPlda.train1() (utils/models.py:238-249: the tdnn batch norms on their running statistics).  Bytes of
 * the `saved` buffer of one nplda_xvec_extract_train_f32 call: the padded input image, every tdnn layer's normalised
 * output and ReLU-mask bytes, a per-row index and the pooled rows (about 30 KB per frame, 12 KB per utterance). */
size_t nplda_xvec_train_saved_bytes(int64_t total_frames, int64_t n_utts);
/* utils/models.py:170-186 as nplda_xvec_extract_f32 (same arguments; out is bit for bit the same), keeping in `saved`
 * what nplda_xvec_backward_f32 reads.  One call covers the whole batch (no chunking). */
int nplda_xvec_extract_train_f32(const float* x, int layout, int64_t ld_in, const int64_t* offsets, int64_t n_utts,
                                 int64_t total_frames, int pooling, const void* packed, float* out, int64_t ldx,
                                 void* saved, size_t saved_bytes, nplda_stream_t stream);
/* Bytes of the transposed weight image the data gradient reads (tdnn2..tdnn10 and lin11, W per context tap transposed). */
size_t nplda_xvec_packed_t_bytes(void);
/* Pack it from W: the host array of 11 device pointers of nplda_xvec_pack_f32 (W[0], tdnn1, is not read). */
int nplda_xvec_pack_t_f32(const float* const* W, void* packed_t, size_t packed_t_bytes, nplda_stream_t stream);
/* Floats of the flat gradient: for tdnn1..tdnn10 then lin11, dW in torch layout (Dout, c * Din) followed by db (Dout). */
size_t nplda_xvec_grad_floats(void);
/* Workspace of one nplda_xvec_backward_f32 call (about 10 KB per frame plus the split-K partials, 40 MB at most). */
size_t nplda_xvec_backward_workspace_bytes(int64_t total_frames, int64_t n_utts);
/* The autograd backward of utils/models.py:170-186 (unfold, nn.Linear, ReLU, eval BatchNorm1d, torch.std / torch.var
 * pooling, lin11) with respect to the 22 weights and biases: grad (nplda_xvec_grad_floats() floats) = dL/dparams given
 * dxvec (n_utts, lddx) = dL/dx-vectors, from the `saved` buffer of the nplda_xvec_extract_train_f32 call with the same
 * offsets, n_utts, total_frames, pooling and packed image; packed_t from the same weights.  grad is overwritten, not
 * accumulated.  Deterministic: fixed split-K partition and summation order, no atomics. */
int nplda_xvec_backward_f32(const void* saved, size_t saved_bytes, const int64_t* offsets, int64_t n_utts,
                            int64_t total_frames, int pooling, const float* dxvec, int64_t lddx, const void* packed,
                            const void* packed_t, float* grad, void* ws, size_t ws_bytes, nplda_stream_t stream);

/* The same extractor trained with batch-statistics batch norm (csrc/nplda_xvec_bn.hip, design/k27_xvec_batch_stats.md):
 * XVectorNet_ETDNN_12Layer.extract under a plain model.train() (utils/models.py:90-93: unfold, Linear, ReLU, then
 * nn.BatchNorm1d(affine=False) on the statistics of the batch).  For tdnn layer l the statistics run over V_l, the rows
 * whose index inside their utterance is < T_u - ctx_l (ctx = 4, 4, 8, 8, 14, 14, 22, 22, 22, 22), over all utterances
 * of the call: mu_l the mean, v_l the biased variance (fp64 sums in a fixed order), O_l = (ReLU(.) - mu_l) / sqrt(v_l + eps_l).
 * These four calls mirror the four above.  Every utterance must be longer than 22 frames, and total_frames - 22 n_utts
 * (the valid rows of tdnn7..tdnn10) must be 2 at least: otherwise NPLDA_EINVAL, and nothing is launched.
 * Bytes of `saved`: what nplda_xvec_train_saved_bytes counts, plus mu_l and 1 / sqrt(v_l + eps_l) of every layer and the
 * partial sums of the statistics. */
size_t nplda_xvec_train_bn_saved_bytes(int64_t total_frames, int64_t n_utts);
/* Bytes of the statistics table nplda_xvec_extract_train_bn_f32 fills: for l = 0..9 the batch mean (ld_l floats) then
 * the UNBIASED batch variance v_l n_l / (n_l - 1) (ld_l floats), ld_l = 512 (tdnn10: 1504, the first 1500 used), then
 * ten int64 n_l.  What torch's running_mean / running_var update takes. */
size_t nplda_xvec_bn_stats_bytes(void);
/* Where layer `layer` (0..9) keeps its ReLU-mask bytes inside `saved`: mask[row, col] (1 = the pre-activation was > 0
 * and the row lies in V_l) is the byte at *offset + row * *row_stride + col.  For tests and tools. */
int nplda_xvec_bn_mask_layout(int64_t total_frames, int64_t n_utts, int layer, size_t* offset, int64_t* row_stride);
/* Arguments as nplda_xvec_extract_train_f32; the packed image's running statistics are not read.  eps: HOST array of
 * ten floats (tdnn<i>.bn.eps).  stats: device table of nplda_xvec_bn_stats_bytes() bytes, 16-byte aligned. */
int nplda_xvec_extract_train_bn_f32(const float* x, int layout, int64_t ld_in, const int64_t* offsets, int64_t n_utts,
                                    int64_t total_frames, int pooling, const void* packed, const float* eps, float* out,
                                    int64_t ldx, void* saved, size_t saved_bytes, void* stats, size_t stats_bytes,
                                    nplda_stream_t stream);
/* Workspace of one nplda_xvec_backward_bn_f32 call (that of nplda_xvec_backward_f32 plus the partial column sums). */
size_t nplda_xvec_backward_bn_workspace_bytes(int64_t total_frames, int64_t n_utts);
/* The autograd backward of the batch-statistics forward with respect to the 22 weights and biases, arguments as
 * nplda_xvec_backward_f32.  With G_l = dL/dO_l, a_l = mean over V_l of G_l and c_l = mean over V_l of G_l O_l (fp64 sums
 * in a fixed order, rows outside V_l excluded by their index, not by value): dL/dR_l = (G_l - a_l - O_l c_l) / sqrt(v_l +
 * eps_l) on V_l, then the ReLU mask, then the data-gradient and weight-gradient kernels of the running-statistics path.
 * grad is overwritten.  Deterministic, no atomics. */
int nplda_xvec_backward_bn_f32(const void* saved, size_t saved_bytes, const int64_t* offsets, int64_t n_utts,
                               int64_t total_frames, int pooling, const float* dxvec, int64_t lddx, const void* packed,
                               const void* packed_t, float* grad, void* ws, size_t ws_bytes, nplda_stream_t stream);

/* ---- feature front end of the extractor (Kaldi feature archives -> its input rows) ------------------------------ */

/* csrc/nplda_feat.hip: what the x-vector recipe runs in front of nnet3-xvector-compute, `apply-cmvn-sliding
 * --norm-vars=false --center=true --cmn-window=300 | select-voiced-frames` over feats.scp and vad.scp (or
 * compute-vad-energy with the options of vad.conf), on matrix bodies copied from the archive as they are
 * (neuralplda_amd/kaldi_format.py load_feature_scp).  design/k13_feature_frontend.md. */
#define NPLDA_FEAT_DIM 30  /* columns of every matrix (the extractor's input dimension) */
#define NPLDA_FEAT_FM  0   /* float32 rows                                                         */
#define NPLDA_FEAT_DM  1   /* float64 rows                                                         */
#define NPLDA_FEAT_CM  2   /* Kaldi CompressedMatrix, one byte per value, column-major, per-column headers */
#define NPLDA_FEAT_CM2 3   /* uint16 per value, row-major                                          */
#define NPLDA_FEAT_CM3 4   /* uint8 per value, row-major                                           */
/* One matrix of the payload.  Offsets are bytes from the start of the payload; data_off is a multiple of the element size
 * (4 FM, 8 DM, 2 CM2), hdr_off (CM only: cols x four uint16 percentiles) is even.  min_value / range: CM, CM2, CM3. */
typedef struct nplda_feat_desc {
    int32_t format, rows, cols;
    float min_value, range;
    int32_t reserved;
    int64_t hdr_off, data_off;
} nplda_feat_desc;

/* frames (total_frames, 30) float32 = the n_utts matrices of `desc` (device array of nplda_feat_desc) decoded from `payload`
 * (device bytes, 8-byte aligned), one launch.  offsets: int64 device array of n_utts + 1 frame offsets, offsets[u + 1] -
 * offsets[u] == desc[u].rows, offsets[n_utts] == total_frames.  An entry whose body does not lie inside payload_bytes, is
 * misaligned, has cols != 30 or an unknown format decodes to NaN rows (nothing outside the payload is read). */
int nplda_feat_decode_f32(const void* payload, size_t payload_bytes, const void* desc, const int64_t* offsets, int64_t n_utts,
                          int64_t total_frames, float* frames, nplda_stream_t stream);
/* compute-vad-energy on column 0: thr_u = energy_threshold + energy_mean_scale * mean_t frames[u][t][0] (fp64, fixed order);
 * mask[t] = 1 iff, over t2 in [t - frames_context, t + frames_context] clipped to the utterance, the number of frames
 * with c0 > thr_u is >= (number of t2) * proportion_threshold.  mask: (total_frames) bytes. */
int nplda_feat_vad_energy_f32(const float* frames, const int64_t* offsets, int64_t n_utts, int64_t total_frames,
                              double energy_threshold, double energy_mean_scale, double proportion_threshold,
                              int frames_context, uint8_t* mask, nplda_stream_t stream);
/* Workspace of one nplda_feat_cmn_select_f32 call (fp64 prefix sums: 240 bytes per frame and per utterance). */
size_t nplda_feat_workspace_bytes(int64_t total_frames, int64_t n_utts);
/* Sliding-window mean subtraction, then selection of the voiced frames, in that order.  Frame t of a T-frame utterance
 * loses the mean of frames [s, e): s = t - cmn_window / 2, e = s + cmn_window, shifted into [0, T) and cut to it (fp64
 * prefix sums in a fixed order); cmn_window == 0: no subtraction.  mask: (total_frames) bytes, non-zero = keep; NULL keeps
 * every frame.  counts[u] (int32, n_utts) = kept frames of utterance u.  Utterances with counts[u] >= min_frames are
 * written to `out` one after the other, their kept frames in order ((sum of those counts, 30) float32, at most
 * total_frames rows); the others are left out.  Same bits on every call; an utterance's rows do not depend on the batch. */
int nplda_feat_cmn_select_f32(const float* frames, const int64_t* offsets, int64_t n_utts, int64_t total_frames,
                              const uint8_t* mask, int cmn_window, int min_frames, float* out, int32_t* counts, void* ws,
                              size_t ws_bytes, nplda_stream_t stream);

/* ---- MFCCs from 16-bit audio (compute-mfcc-feats with --dither=0) ------------------------------------------------ */

/* csrc/nplda_mfcc.hip, design/k14_mfcc.md: samples -> frames -> mean removal, energy, pre-emphasis, window -> real DFT as
 * a matrix product -> power -> mel banks -> log -> DCT and lifter, one kernel.  The three tables are built by the caller
 * (neuralplda_amd/mfcc.py MfccPlan) in float64, rounded once and laid out in MFMA fragment order, lane = 0 .. 63,
 * i = 0 .. 3, KB = ceil(N / 16), NBW = P / 128, MB = 2 if B <= 32 else 4, zero outside the matrices:
 *   dft [kb][w][u][lane][i]   = t(n = 16 kb + 4 (lane >> 4) + i, bin = 16 (w NBW + u % NBW) + (lane & 15)), w = 0 .. 3,
 *                               u = 0 .. 2 NBW - 1: t = cos(2 pi n bin / P) for u < NBW, sin for the others
 *   bank[bb][mb][lane][i]     = weight of FFT bin 16 bb + 4 (lane >> 4) + i in mel bin 16 mb + (lane & 15), bb < P / 32
 *   dct [kb][cb][lane][i]     = lifter(c) D(c, b) for c = 16 cb + (lane & 15), b = 16 kb + 4 (lane >> 4) + i, kb, cb < MB */
#define NPLDA_MFCC_TILE 32         /* output frames per block */
#define NPLDA_MFCC_REMOVE_DC  1    /* flags */
#define NPLDA_MFCC_USE_ENERGY 2
#define NPLDA_MFCC_RAW_ENERGY 4
typedef struct nplda_mfcc_geometry {
    int32_t N, P, S;        /* samples per frame, padded (power of two) frame, samples per shift */
    int32_t snip_edges;     /* non-zero: frame f starts at f S; zero: at f S + S / 2 - N / 2, indices reflected into the utterance */
    int32_t B, C;           /* mel bins, cepstra */
    int32_t flags;
    float preemph;          /* pre-emphasis coefficient */
    float energy_floor;     /* > 0: log energy >= log of it */
} nplda_mfcc_geometry;

/* Bytes of image `which` (0 dft, 1 bank, 2 dct) for a supported geometry, 0 otherwise. */
size_t nplda_mfcc_image_bytes(const nplda_mfcc_geometry* geometry, int which);
/* out (total_frames, C) float32 = the MFCCs of n_utts utterances, one launch whatever their lengths.  samples: DEVICE int16,
 * utterance u at [sample_offsets[u], sample_offsets[u + 1]); frame_offsets: its rows of `out` (both DEVICE int64 arrays of
 * n_utts + 1; the caller computes the frame counts on the host, so nothing is read back).  geometry: HOST pointer.  window:
 * N floats; images: 16-byte aligned.  Supported: N % 4 == 0, N <= 512, P in {256, 512}, N <= P, B <= 64, C <= B — anything
 * else returns NPLDA_EUNSUPPORTED before any launch.  total_frames == 0 is a no-op.  Nothing outside an utterance's own
 * samples is read; same bits on every call; a frame's row does not depend on the batch. */
int nplda_mfcc_frames_f32(const int16_t* samples, const int64_t* sample_offsets, const int64_t* frame_offsets, int64_t n_utts,
                          int64_t total_frames, const nplda_mfcc_geometry* geometry, const float* window, const void* dft_image,
                          const void* bank_image, const void* dct_image, float* out, nplda_stream_t stream);

/* ---- class scatter of x-vector rows (LDA / PLDA estimation, neuralplda_amd/backend.py) ------------------------ */

/* With x_k = table[rows[k]][0:n] - pivot (rows == NULL: row k itself; pivot == NULL: 0) for the N positions k, of which
 * offs[s] .. offs[s + 1] belong to class s (offs: S + 1 DEVICE int64, non-decreasing, offs[0] = 0, offs[S] = N):
 *     sum[i] = sum_k x_k[i],   scatter[i][j] = sum_k x_k[i] x_k[j],   class_sum[s][i] = sum_{k in s} x_k[i]
 * — what ivector-mean, ivector-compute-lda and ivector-compute-plda accumulate.  Outputs are DEVICE doubles: sum (n),
 * scatter (n, n), class_sum (S, n).  accumulate != 0 adds into sum and scatter (training sets can be streamed); class_sum is
 * always overwritten, an empty class gives a zero row.  Products are exact fp32 on MFMA, summed in fp32 over row groups of
 * 1024 and in fp64, in a fixed order, across them: no atomics, the same bits on every call, scatter exactly symmetric.  The
 * pivot is subtracted BEFORE the product: pass an estimate of the mean, so that data far from the origin does not cancel in
 * fp32.  Row indices are clamped into [0, table_rows) as in nplda_embed_rows_f32 (callers validate them).
 * Requires n % 4 == 0, n <= 512 (else NPLDA_EUNSUPPORTED), ldt % 4 == 0, ldt >= n, table / pivot / ws 16-byte aligned
 * (else NPLDA_EINVAL); nothing is launched then.  N == 0: zeros (sum and scatter untouched under accumulate).
 * ws: nplda_class_scatter_workspace_bytes(N, S, n) bytes (0 for an unsupported n).  The environment variable
 * NPLDA_SCATTER_MAX_CHUNKS (read by both functions at every call) lowers the number of fp64 slabs the GEMM keeps: less
 * workspace, the same result to the last bit. */
size_t nplda_class_scatter_workspace_bytes(int64_t N, int64_t S, int n);
int nplda_class_scatter_f32(const float* table, int64_t table_rows, int64_t ldt, const int64_t* rows, int64_t N,
                            const int64_t* offs, int64_t S, int n, const float* pivot, double* sum, double* scatter,
                            double* class_sum, int accumulate, void* ws, size_t ws_bytes, nplda_stream_t stream);

/* ---- dense score matrix of a set against itself, and its agglomerative clustering ---------------------------- */

/* csrc/nplda_ahc.hip, design/k21_ahc.md.  One call handles P independent PROBLEMS: problem p owns the contiguous rows
 * offsets[p] .. offsets[p + 1] of an embedding table (z, q from nplda_embed_f32, row stride ldz); n_p = 0 and 1 are legal;
 * row indices in every output are local to the problem.  `offsets_host` (P + 1 int64, offsets_host[0] == 0, non-decreasing)
 * is read by the host during the call only: it sizes the launch and is what the argument checks see; `offsets` is the same
 * array in DEVICE memory.  The matrices of the problems lie one after the other, problem p's n_p x n_p floats (row stride
 * n_p) at element sum_{r < p} n_r^2.  Caller-owned workspace, nothing allocated, no host synchronisation, capturable, the same
 * bits on every call, no floating-point atomics; every output word is written by the call (no memset), nothing is read back.
 * P == 0 or an empty table is a no-op; every error is a status code before any launch. */
typedef struct nplda_ahc_merge {
    int32_t a, b;       /* the clusters merged, named by their smallest member rows, a < b; b is absorbed into a */
    double value;       /* the linkage value of the pair */
    int32_t size_after; /* members of a after the merge */
    int32_t reserved;   /* written as 0 */
} nplda_ahc_merge;
#define NPLDA_AHC_AVERAGE  0  /* S(A, B) / (|A| |B|): fp64 sums of member-pair scores, ONE addition per surviving cluster and merge */
#define NPLDA_AHC_COMPLETE 1  /* the minimum member-pair score */
#define NPLDA_AHC_SINGLE   2  /* the maximum member-pair score */
int nplda_ahc_max_n(void);  /* the largest n_p (16384: the fp64 numerators of a problem take 8 n_p^2 bytes) */
int nplda_ahc_block(void);  /* threads of the clustering workgroup (one workgroup per problem) */
int nplda_ahc_small_n(void); /* problems above this many rows scan a row again with the whole workgroup, the others with one wave */
/* Bytes of the matrices / workspace bytes of the clustering for these problems; 0 where the offsets are not acceptable
 * (the workspace of acceptable offsets is never 0). */
size_t nplda_score_matrix_bytes(const int64_t* offsets_host, int64_t P);
size_t nplda_ahc_workspace_bytes(const int64_t* offsets_host, int64_t P);
/* out = the score matrices s_ij = q_i + q_j + 2 sum_d P_d z_id z_jd of the problems.  Only 16 x 16 pieces that hold some
 * i < j are formed, with the lower index as the row operand and the products and feature order of nplda_topk_scores_f32,
 * so that for i < j the bits are what that call returns for (row i, column j); entry (j, i) is a copy of (i, j) and the
 * diagonal is +0.0f.  Rows of another problem are never read; pad columns D2 .. ldz meet P = 0. */
int nplda_score_matrix_f32(const float* z, int64_t ldz, const float* q, const int64_t* offsets_host, const int64_t* offsets,
                           int64_t P, const void* packed, int D0, int D1, int D2, float* out, nplda_stream_t stream);
/* Agglomerative clustering of every problem under its matrix in S (the layout above; only the strict upper triangle is
 * read; NaN scores are outside the contract).  Each step merges the pair of live clusters (a, b), a < b, with the LARGEST
 * linkage value, the lexicographically lowest (a, b) among equal values, and stops before the first merge whose value is
 * < threshold or when min_clusters clusters remain.  merges: sum of max(n_p - 1, 0) records, problem by problem, the ones not
 * executed (-1, -1, NaN, 0); n_merges, n_clusters: P int32; labels: one int32 per table row, the dense rank of the row's
 * cluster in order of the clusters' smallest members.  A NaN threshold, min_clusters < 1 or an unknown linkage is
 * NPLDA_EINVAL, n_p above nplda_ahc_max_n() NPLDA_EUNSUPPORTED, a short workspace NPLDA_ENOSPC.  ws: 16-byte aligned. */
int nplda_ahc_f32(const float* S, const int64_t* offsets_host, const int64_t* offsets, int64_t P, int linkage, double threshold,
                  int min_clusters, nplda_ahc_merge* merges, int32_t* n_merges, int32_t* n_clusters, int32_t* labels, void* ws,
                  size_t ws_bytes, nplda_stream_t stream);

/* ---- VB-HMM resegmentation of clustered embeddings (VBx) ----------------------------------------------------- */

/* csrc/nplda_vbhmm.hip, design/k22_vbhmm.md.  One call handles P independent PROBLEMS (recordings) with the conventions of
 * nplda_ahc_f32: problem p owns the rows offsets[p] .. offsets[p + 1] of z IN TIME ORDER (T_p of them) and the speaker slots
 * spk_offsets[p] .. spk_offsets[p + 1] (S_p of them); both offset arrays are given on the host (read during the call only:
 * checks and sizes) and on the device.  z is what nplda_embed_f32 wrote (fp32, 16-byte aligned, row stride ldz >= D2, a
 * multiple of 4): rows in the space where the within-class covariance is I and the between-class covariance diag(psi);
 * columns D2 .. ldz and rows of another problem are never read.  psi: D2 float64 on the device, >= 0.
 *
 * Per problem, in float64 throughout, iteration i = 0, 1, ...: speaker models from the posteriors (N_s, invL_sd, alpha_sd),
 * emissions l_ts, a forward-backward pass over the HMM with transition loop_prob [i = j] + (1 - loop_prob) pi_j (normalised
 * at every step; speakers with pi_s == 0 stay exactly dead), ELBO_i, the update of pi; for i >= 1 it stops after the
 * iteration whose ELBO gain is < epsilon (-inf: never), else after max_iters.  Initial posteriors: gamma_init (the layout of
 * gamma), or from labels_init (one int32 per table row, local to the problem): softmax_s(init_smoothing [s = label]), a
 * label outside 0 .. S_p - 1 gives the uniform row.  EXACTLY ONE of the two is non-null.  pi_init (the layout of pi) may be
 * null: 1 / S_p.
 *
 * Outputs, every word written by the call: gamma (float64, problem p's T_p x S_p block at element sum_{r < p} T_r S_r),
 * pi (float64, at spk_offsets[p]), elbo (P x max_iters float64, NaN where not executed), n_iters (P int32), labels (one
 * int32 per table row: argmax_s gamma_ts, the lowest s among equal values, renumbered to the dense rank of the speakers
 * that own a row, in order of s), n_speakers (P int32).  T_p == 0 writes n_iters = 0, n_speakers = 0 and a NaN elbo row
 * only.  Rows with NaN are outside the contract.
 *
 * NPLDA_EINVAL: NaN epsilon, Fa or Fb not > 0 (or not finite), loop_prob outside [0, 1), init_smoothing < 0 or NaN,
 * max_iters < 1, bad offsets, S_p == 0 with T_p > 0, a null or misaligned pointer, both or neither initialiser.
 * NPLDA_EUNSUPPORTED: S_p above nplda_vbhmm_max_speakers(), max_iters above nplda_vbhmm_max_iters(), T_p above
 * nplda_ahc_max_n(), D2 above nplda_max_dim().  NPLDA_ENOSPC: a short workspace.  ws: 16-byte aligned.  Caller-owned
 * workspace, nothing allocated, no host synchronisation, capturable, the same bits on every call, no floating-point
 * atomics, no memset, nothing read back; P == 0 is a no-op; every error is a status code before any launch. */
int nplda_vbhmm_max_speakers(void); /* 64: a speaker per lane of one wave in the recursions */
int nplda_vbhmm_max_iters(void);    /* 256 */
int nplda_vbhmm_block(void);        /* threads of the workgroup (one workgroup per problem) */
/* 0 where the arguments are not acceptable, never 0 for acceptable ones, a multiple of 256 */
size_t nplda_vbhmm_workspace_bytes(const int64_t* offsets_host, const int64_t* spk_offsets_host, int64_t P, int D2);
int nplda_vbhmm_f64(const float* z, int64_t ldz, const int64_t* offsets_host, const int64_t* offsets,
                    const int64_t* spk_offsets_host, const int64_t* spk_offsets, int64_t P, int D2, const double* psi,
                    const int32_t* labels_init, const double* gamma_init, const double* pi_init, double Fa, double Fb,
                    double loop_prob, double epsilon, double init_smoothing, int max_iters, double* gamma, double* pi,
                    double* elbo, int32_t* n_iters, int32_t* labels, int32_t* n_speakers, void* ws, size_t ws_bytes,
                    nplda_stream_t stream);

/* ---- diarization error rate with the optimal speaker mapping -------------------------------------------------- */

/* csrc/nplda_der.hip, design/k24_der.md.  One call scores P PROBLEMS against Rn RECORDINGS; a problem names a recording
 * (prob_reco) and holds one hypothesis for it, and many problems may share a recording: the reference side is prepared once
 * per recording.  Everything counts in integer frames and every output is an exact integer; there is no floating point.
 *
 * Recording r has T_r = frame_offsets[r + 1] - frame_offsets[r] frames.  A TURN is three int32 (begin, end, speaker) with
 * 0 <= begin <= end <= T_r and a speaker local to the recording and to its side, in [0, n_ref_speakers) for the reference
 * and [0, n_hyp_speakers) for a hypothesis (both at most nplda_der_max_speakers()).  Turns may overlap, on both sides, and
 * the turns of one speaker are taken as given.  The reference turns of recording r are the rows ref_offsets[r] ..
 * ref_offsets[r + 1] of ref_turns.  On the device the bounds of a turn are clamped to [0, T_r]; a turn whose end lies before
 * its begin, or whose speaker is outside the limit, does not exist (it has no collar either).
 *
 * SCORED frames of a recording: the frames inside its UEM regions (rows uem_offsets[r] .. uem_offsets[r + 1] of uem, two
 * int32 (begin, end) each; uem_offsets == NULL: [0, T_r) for every recording; a recording without a region has no scored
 * frame), less every frame f with b - collar <= f < b + collar or e - collar <= f < e + collar for a reference turn [b, e),
 * less, with skip_overlap != 0, every frame with more than one reference speaker.
 *
 * HYPOTHESES, exactly one of two forms per call (the other form's pointers all NULL):
 *   turns:          hyp_offsets (P + 1) into hyp_turns, the rows of a problem as for the reference;
 *   labelled items: frame_item holds one int32 per frame of every RECORDING (at frame_offsets[r] + f), the index of the item
 *                   (window) that owns the frame or -1; item_offsets (P + 1) into item_labels, one int32 label per item of
 *                   the PROBLEM in [0, n_hyp_speakers) or -1 for no speaker.  An item index outside the problem's items and a
 *                   label outside the limit count as -1.
 *
 * With R(t), H(t) the sets of active reference and hypothesis speakers at a scored frame t, per problem:
 *   counts[6] (int64): scored = the number of scored frames, total = sum |R|, miss = sum max(0, |R| - |H|),
 *                      fa = sum max(0, |H| - |R|), summin = sum min(|R|, |H|), matched = max over one-to-one partial
 *                      mappings m of sum_i C[i][m(i)], where C[i][j] = scored frames with i in R(t) and j in H(t);
 *                      speaker confusion is summin - matched and DER = (miss + fa + summin - matched) / total;
 *   map_ref[64] (int32): the hypothesis speaker of each reference speaker under one optimal mapping, -1 for a speaker that
 *                      is unmapped or shares no scored frame with its partner.  Ties between optimal mappings are broken by a
 *                      fixed rule (rows enter the shortest-augmenting-path search in increasing order, the lowest column
 *                      among equal smallest slacks is taken), so the mapping is a function of C alone;
 *   C[64 * 64] (int32, row = reference speaker), or C == NULL.
 * A problem of an empty recording gets zeros and -1.
 *
 * The offset tables and prob_reco are given on the host (read during the call only: checks and sizes) and on the device.
 * NPLDA_EINVAL: a negative count, collar or speaker limit, offsets that do not start at 0 or decrease, prob_reco_host
 * outside [0, Rn), both or neither hypothesis form, a null or misaligned pointer (int64 tables and counts 8 bytes, int32
 * tables 4, ws 16).  NPLDA_EUNSUPPORTED: a speaker limit above nplda_der_max_speakers(), T_r above 2^31 - 1, more than 2^40
 * frames, Rn or P above 2^24.  NPLDA_ENOSPC: ws_bytes below nplda_der_workspace_bytes(frame_offsets_host, Rn) (0 where the
 * offsets are not acceptable, else a positive multiple of 256: 12 bytes per frame).  Caller-owned workspace, nothing
 * allocated, no host synchronisation, capturable, the same bits on every call, integer atomics only (OR on the frame
 * masks, ADD on C in LDS: order-free), nothing read back; P == 0 is a no-op; every error is a status code before any launch. */
int nplda_der_max_speakers(void); /* 64: a speaker per bit of a frame's mask and per lane in the assignment */
int nplda_der_block(void);        /* threads of the counting workgroup (one workgroup per problem) */
size_t nplda_der_workspace_bytes(const int64_t* frame_offsets_host, int64_t Rn);
int nplda_der_i64(const int64_t* frame_offsets_host, const int64_t* frame_offsets, int64_t Rn, const int64_t* ref_offsets_host,
                  const int64_t* ref_offsets, const int32_t* ref_turns, const int64_t* uem_offsets_host, const int64_t* uem_offsets,
                  const int32_t* uem, int collar, int skip_overlap, int n_ref_speakers, int n_hyp_speakers,
                  const int32_t* prob_reco_host, const int32_t* prob_reco, int64_t P, const int64_t* hyp_offsets_host,
                  const int64_t* hyp_offsets, const int32_t* hyp_turns, const int32_t* frame_item, const int64_t* item_offsets_host,
                  const int64_t* item_offsets, const int32_t* item_labels, int64_t* counts, int32_t* map_ref, int32_t* C, void* ws,
                  size_t ws_bytes, nplda_stream_t stream);

/* ---- spectral clustering with an auto-tuned neighbour count (NME-SC) ------------------------------------------ */

/* csrc/nplda_spectral.hip, design/k25_spectral.md.  One call handles P independent PROBLEMS with the conventions of
 * nplda_ahc_f32: S is the ragged block-diagonal fp32 score matrix of nplda_score_matrix_f32 (problem p's n_p x n_p floats at
 * element sum_{r < p} n_r^2); only off-diagonal entries are read, -0.0f counts as +0.0f, NaN is outside the contract.
 * `neighbours` is a HOST table of C candidate neighbour counts, 1 <= C <= 16, positive and strictly increasing.  A CELL is a
 * (problem, candidate) pair, cell number p C + candidate index.  For a cell with n rows and candidate c, m = min(c, n - 1):
 *   1. graph: B[i][j] = 1 for the m columns j != i with the largest s_ij, equal scores by ascending j, 0 elsewhere;
 *      A = (B + B^T) / 2, d_i = sum_j A_ij, L = diag(d) - A: every entry a multiple of 1/2, formed without rounding.
 *   2. spectrum: all eigenvalues l_1 <= ... <= l_n of L (cyclic Jacobi in float64, round-robin ordering, a rotation skipped
 *      where |a_pq| <= ||L||_F 2^-53 / (n rounded up to even), at most nplda_spectral_max_sweeps() sweeps, stopping after a
 *      sweep without a rotation), equal computed values ordered by their position on the diagonal, and the eigenvectors of
 *      the K + 1 smallest, K = min(max_clusters, n - 1), scaled to unit length.
 *   3. count: gap_k = l_{k+1} - l_k for min_clusters <= k <= K; k* the k of the largest gap, the lowest among equals;
 *      g = gap_{k*} / l_n; r = c / g (c, not m), each quotient one correctly rounded division.  Where n <= 1, no k is in
 *      range, l_n <= 0 or g <= 0: k* = min(min_clusters, max(n, 1)) and r = +inf.
 *   4. per problem the cell with the smallest r is chosen, the lowest candidate index among equals (so a candidate that
 *      repeats another after the clip to n - 1 never wins: its g is the same and its c larger).
 *   5. partition: k = min(k*, n); k-means on the rows of the n x k matrix E of the chosen cell's k smallest eigenvectors.
 *      Centres: row 0, then each time the row with the largest minimum squared distance to the centres so far (the lowest
 *      row among equals).  An iteration assigns each row to the nearest centre (the lowest among equals), and, unless that
 *      assignment repeats the previous iteration's, sets each centre to the mean of its rows (a centre without rows keeps
 *      its place); it ends at a repeated assignment or after max_iters iterations; n_kmeans_iters counts the assignments made.
 *      Squared distances (in column order) and centre sums (in row order) are float64, one subtraction, multiplication and
 *      addition at a time, never contracted; a mean is one division.  Labels: the dense rank of the row's cluster in order
 *      of the clusters' smallest members; n_clusters: the clusters that own a row.
 * Outputs, every word written by the call: per cell eigenvalues[max_clusters + 2] (slots 0 .. K the K + 1 smallest, the
 * last slot l_n, NaN elsewhere and for n = 0), kstar, ratio, n_sweeps, converged (0: the sweep limit was reached; the cell
 * still takes part); per problem chosen (candidate index), n_clusters, n_kmeans_iters; labels (one int32 per table row).
 * Optional (NULL: not wanted): embedding (rows x max_clusters doubles; problem p's E, row-major n_p x k, compact at element
 * offsets[p] max_clusters), degrees (rows x C doubles; cell (p, c)'s d at offsets[p] C + c n_p), vectors (per cell
 * min(max_clusters + 1, n_p) x n_p doubles, the eigenvectors as ROWS in eigenvalue order, cell after cell).
 * P == 0 is a no-op; with an empty table only the per-cell and per-problem words are written.
 * NPLDA_EINVAL: a bad candidate table, min_clusters < 1, max_clusters < min_clusters or > nplda_spectral_max_k(),
 * max_iters < 1, bad offsets, a null or misaligned pointer.  NPLDA_EUNSUPPORTED: n_p above nplda_spectral_max_n(), P >= 2^22.
 * NPLDA_ENOSPC: ws_bytes below nplda_spectral_workspace_bytes (0 where the arguments are not acceptable, else a positive
 * multiple of 256: about 16 n_p^2 bytes per cell).  ws: 16-byte aligned.  Three launches whatever the problems; caller-owned
 * workspace, nothing allocated, no host synchronisation, capturable, the same bits on every call, no floating-point atomics,
 * no memset, nothing read back; every error is a status code before any launch. */
int nplda_spectral_max_n(void);          /* 2048 */
int nplda_spectral_max_k(void);          /* 64: the speaker slots of the VB-HMM and the DER */
int nplda_spectral_max_candidates(void); /* 16 */
int nplda_spectral_max_sweeps(void);     /* 30 */
int nplda_spectral_block(void);          /* threads of the eigensolver's workgroup (one workgroup per cell) ... */
int nplda_spectral_small_n(void);        /* ... unless no problem of the call has more rows than this: then ... */
int nplda_spectral_small_block(void);    /* ... this many */
size_t nplda_spectral_workspace_bytes(const int64_t* offsets_host, int64_t P, int n_candidates);
int nplda_spectral_f32(const float* S, const int64_t* offsets_host, const int64_t* offsets, int64_t P, const int32_t* neighbours,
                       int n_candidates, int min_clusters, int max_clusters, int max_iters, double* eigenvalues, int32_t* kstar,
                       double* ratio, int32_t* n_sweeps, int32_t* converged, int32_t* chosen, int32_t* n_clusters,
                       int32_t* n_kmeans_iters, int32_t* labels, double* embedding, double* degrees, double* vectors, void* ws,
                       size_t ws_bytes, nplda_stream_t stream);
/* Step 5 alone on caller-given rows: E is (rows, dim) float64, row-major, problem p's rows offsets[p] .. offsets[p + 1];
 * every problem is partitioned into min(k, n_p) clusters.  1 <= dim, k <= nplda_spectral_max_k(); the other conventions,
 * limits and status codes as above (workspace: 8 bytes per row). */
size_t nplda_spectral_kmeans_workspace_bytes(const int64_t* offsets_host, int64_t P);
int nplda_spectral_kmeans_f64(const double* E, const int64_t* offsets_host, const int64_t* offsets, int64_t P, int dim, int k,
                              int max_iters, int32_t* n_clusters, int32_t* n_iters, int32_t* labels, void* ws, size_t ws_bytes,
                              nplda_stream_t stream);

/* ---- augmentation of 16-bit audio: reverberation and additive noise ------------------------------------------- */

/* csrc/nplda_augment.hip, design/k28_augment.md: x -> x * h (uniformly partitioned overlap-save, block 256, transform 512,
 * both transforms exact fp32 MFMA products against constant tables) -> + s noise -> gain -> float32 or int16.  A block's
 * spectrum is 512 floats: [0, 256) the real parts of bins 0 .. 255, [256] the (real) Nyquist bin, [256 + k] the imaginary
 * part of bin k = 1 .. 255.  The two tables are built by the caller (neuralplda_amd/augment.py) in float64, rounded once
 * and laid out in MFMA fragment order, kb = 0 .. 31, w = 0 .. 3, lane = 0 .. 63, i = 0 .. 3:
 *   forward [kb][w][u][lane][i], u < 8 = F(o = 16 (8 w + u) + (lane & 15), n = 16 kb + 4 (lane >> 4) + i):
 *            F(o, n) = cos(2 pi o n / 512) for o < 256, (-1)^n for o = 256, -sin(2 pi (o - 256) n / 512) above
 *   inverse [kb][w][u][lane][i], u < 4 = G(t = 16 (4 w + u) + (lane & 15), o = 16 kb + 4 (lane >> 4) + i), output
 *            sample 256 + t of the inverse transform: G(t, 0) = 1 / 512, G(t, 256) = (-1)^t / 512,
 *            G(t, o) = 2 cos(2 pi o (256 + t) / 512) / 512 for 0 < o < 256, -2 sin(2 pi (o - 256) (256 + t) / 512) / 512 above */
#define NPLDA_AUGMENT_BLOCK 256       /* samples per block of the convolution (the transform has twice as many) */
#define NPLDA_AUGMENT_TILE 32         /* blocks per thread block of the transform kernels */
#define NPLDA_AUGMENT_GROUP 8         /* consecutive blocks of one utterance per thread block of the multiply-accumulate */
#define NPLDA_AUGMENT_CHUNK 2048      /* samples per thread block of the element-wise kernels */
#define NPLDA_AUGMENT_MAX_RIR 32768   /* taps: 128 partitions */

typedef struct nplda_augment_utt {    /* one utterance of a call, 64 bytes */
    int64_t in_off;                   /* its first sample in `samples` */
    int64_t out_off;                  /* its first sample in `out` */
    int64_t y_off;                    /* 256 times its first block: where x * h starts in the workspace (with a RIR) */
    int32_t n, n_out;                 /* samples in, samples out */
    int32_t shift;                    /* out[t] = (x * h)[shift + t]: the RIR's peak with shift_output, else 0 */
    int32_t rir;                      /* index of the impulse response, -1: none */
    int32_t ent_begin, ent_count;     /* its additive entries */
    int32_t n_early;                  /* n + (b - a) - 1, the length of x * h[a:b] (with a RIR) */
    int32_t normalize;                /* non-zero: gain sqrt(P_in / P_mix) unless volume > 0 */
    float volume;                     /* > 0: the gain */
    int32_t reserved;
} nplda_augment_utt;

typedef struct nplda_augment_entry {  /* one additive entry, 32 bytes */
    int64_t noise_off;                /* the item's first sample in `noise` */
    int32_t len, start, item, repeat; /* the item's length, the first output sample, the item, non-zero: periodic */
    double ratio;                     /* 10^(-snr_db / 10), computed on the host */
} nplda_augment_entry;

typedef struct nplda_augment_call {   /* HOST struct; every pointer in it is a DEVICE pointer */
    const int16_t* samples;
    const nplda_augment_utt* utts;    /* n_utts */
    const nplda_augment_entry* entries; /* n_entries */
    const int64_t* in_off;            /* n_utts + 1 sample offsets */
    const int32_t* in_len;            /* n_utts */
    const int32_t* in_chunk_off;      /* n_utts + 1: cumulative ceil(n / CHUNK) */
    const int32_t* out_chunk_off;     /* n_utts + 1: cumulative ceil(n_out / CHUNK) */
    const int32_t* blk_off;           /* n_utts + 1: cumulative ceil((n + L - 1) / BLOCK), 0 blocks without a RIR */
    const int32_t* grp_off;           /* n_utts + 1: cumulative ceil(blocks / GROUP) */
    const int32_t* rir_of;            /* n_utts: nplda_augment_utt.rir */
    const int32_t* early_len;         /* n_utts: nplda_augment_utt.n_early */
    const float* rir_spectra;         /* nplda_augment_spectra_f32 of every RIR and of its early window */
    const int32_t* rir_parts;         /* per RIR: first partition, partitions, the early window's first, its partitions */
    const int16_t* noise;
    const int64_t* noise_sums;        /* per noise item: nplda_augment_power_i64 */
    const void* forward_table;        /* 1 MiB, 16-byte aligned */
    const void* inverse_table;        /* 512 KiB, 16-byte aligned */
    void* out;                        /* float32 or int16, sum of n_out */
    int32_t* clipped;                 /* n_utts: saturated samples (int16 output; zeroed otherwise) */
    int64_t n_utts, n_entries, total_blocks, total_groups, total_in_chunks, total_out_chunks;
    int64_t max_conv_len;             /* the largest n + L - 1 of the call */
    int32_t max_rir_len;              /* the largest L in use */
    int32_t out_i16;                  /* non-zero: int16 by round-half-to-even with saturation */
} nplda_augment_call;

/* Bytes of table `which` (0 forward, 1 inverse), 0 otherwise. */
size_t nplda_augment_table_bytes(int which);
/* spectra[b] (512 floats each) = the forward transform of partition b of every filter: filter f is src_len[f] >= 1 floats at
 * src + src_off[f] and takes blocks blk_off[f] .. blk_off[f + 1] = blk_off[f] + ceil(src_len[f] / 256) (DEVICE arrays; the
 * caller gives the smallest and the largest length from the host).  min_len < 1: NPLDA_EINVAL; max_len >
 * NPLDA_AUGMENT_MAX_RIR: NPLDA_EUNSUPPORTED, before any launch. */
int nplda_augment_spectra_f32(const float* src, const int64_t* src_off, const int32_t* src_len, const int32_t* blk_off,
                              int64_t n_filters, int64_t total_blocks, int32_t min_len, int32_t max_len,
                              const void* forward_table, float* spectra, nplda_stream_t stream);
/* sums[i] = the exact sum of squares of item i (samples[item_off[i]] .. samples[item_off[i + 1]]), chunk_off its cumulative
 * ceil(length / NPLDA_AUGMENT_CHUNK); all DEVICE arrays.  Integer atomics only: the same value on every call. */
int nplda_augment_power_i64(const int16_t* samples, const int64_t* item_off, const int32_t* chunk_off, int64_t n_items,
                            int64_t total_chunks, int64_t* sums, nplda_stream_t stream);
/* Host arithmetic: the workspace of a call (20 bytes per sample of x * h, 8 per block and per output chunk, 16 per utterance, 4 per entry). */
size_t nplda_augment_workspace_bytes(int64_t n_utts, int64_t n_entries, int64_t total_blocks, int64_t total_out_chunks);
/* One augmentation call (design/k28_augment.md gives the arithmetic).  The launch count depends on the struct's counts only
 * (no transform launches when total_blocks == 0), nothing is read back, and the call can be captured in a graph.
 * NPLDA_EUNSUPPORTED before any launch: max_rir_len > NPLDA_AUGMENT_MAX_RIR, or max_conv_len / the block and chunk counts
 * beyond the int32 indexing.  NPLDA_ENOSPC: ws_bytes below nplda_augment_workspace_bytes.  n_utts == 0 is a no-op.  No
 * floating-point atomics: same bits on every call, and an utterance's result does not depend on the batch. */
int nplda_augment_batch(const nplda_augment_call* call, void* ws, size_t ws_bytes, nplda_stream_t stream);

/* ---- resampling and speed perturbation of 16-bit audio ---------------------------------------------------------- */

/* csrc/nplda_resample.hip, design/k29_resample.md: a rational-ratio polyphase windowed-sinc resampler over a ragged batch.
 * With g = gcd(rin, rout), iu = rin / g, ou = rout / g, an utterance of n samples gives m = ceil(n ou / iu) samples
 *   y[k] = gain * sum_{t < taps} w[t][k mod ou] * x[(k div ou) iu + first[k mod ou] + t],   x = 0 outside [0, n),
 * one chain of float32 fused multiply-adds per output in increasing t, times gain in float32, stored as float32 or as int16
 * by round-half-to-even with saturation.  The caller (neuralplda_amd/resample.py) builds first[] and w[] in float64 from the
 * integer tick distance i ou - k iu and rounds the weights once; a phase with fewer weights is padded with zeros at its end,
 * and `taps` is padded with zero weights to a multiple of 4 (a ratio whose taps is not is skipped); first[] must not
 * decrease with the phase and first[ou - 1] <= first[0] + iu. */
#define NPLDA_RESAMPLE_CHUNK 1024         /* output samples per thread block */
#define NPLDA_RESAMPLE_MAX_UNITS 1024     /* iu and ou */
#define NPLDA_RESAMPLE_MAX_TAPS 128
#define NPLDA_RESAMPLE_MAX_LDS_BYTES 65536 /* of a chunk's input span as float32 */

typedef struct nplda_resample_utt {   /* one utterance of a call, 32 bytes */
    int64_t in_off;                   /* its first sample in `samples` */
    int64_t out_off;                  /* its first sample in `out` */
    int32_t n, m;                     /* samples in, samples out (m == n for a copy) */
    int32_t ratio;                    /* its row of `ratios`, -1: a copy times the gain, no filter */
    float gain;
} nplda_resample_utt;

typedef struct nplda_resample_ratio { /* one ratio of a call, 32 bytes */
    int32_t iu, ou, taps, reserved;
    int64_t first_off;                /* its ou first-input offsets in `first` */
    int64_t weight_off;               /* its taps x ou weights in `weights`, [tap][phase] */
} nplda_resample_ratio;

typedef struct nplda_resample_call {  /* HOST struct; every pointer in it is a DEVICE pointer */
    const int16_t* samples;           /* 16-byte aligned */
    const nplda_resample_utt* utts;   /* n_utts */
    const nplda_resample_ratio* ratios; /* n_ratios */
    const int32_t* first;
    const float* weights;
    const int32_t* chunks;            /* total_chunks x 2: nplda_resample_chunk_table */
    void* out;                        /* float32 or int16, sum of m */
    int32_t* clipped;                 /* n_utts: the samples that saturated (set to zero by the call first) */
    int64_t n_utts, n_ratios, total_chunks;
    int32_t max_iu, max_ou, max_taps; /* the largest of `ratios`, from the host */
    int32_t max_span;                 /* the largest nplda_resample_span_floats of `ratios` */
    int32_t out_i16;                  /* non-zero: int16 */
    int32_t reserved;
} nplda_resample_call;

/* NPLDA_RESAMPLE_CHUNK. */
int nplda_resample_chunk(void);
/* Host arithmetic: the float32 slots of LDS a chunk of this ratio stages, 0 for a ratio beyond the limits. */
size_t nplda_resample_span_floats(int32_t iu, int32_t ou, int32_t taps);
/* Host arithmetic on HOST arrays: out_off holds n_utts + 1 non-decreasing output offsets starting at 0; returns the number
 * of chunks (ceil(m / NPLDA_RESAMPLE_CHUNK) per utterance) and, if table != NULL, writes (utterance, chunk of the utterance)
 * per chunk, in order.  A negative status instead: NPLDA_EINVAL for a malformed table, NPLDA_EUNSUPPORTED beyond the int32
 * indexing, NPLDA_ENOSPC if `capacity` chunks do not hold the table. */
int64_t nplda_resample_chunk_table(const int64_t* out_off, int64_t n_utts, int32_t* table, int64_t capacity);
/* One resampling call: utterances of different ratios, copies and empty ones in ONE launch (plus the launch that clears
 * `clipped`); the launch count depends on the struct's counts only, nothing is read back, there is no memset, and the call
 * can be captured in a graph.  NPLDA_EUNSUPPORTED before any launch: max_iu / max_ou > NPLDA_RESAMPLE_MAX_UNITS, max_taps >
 * NPLDA_RESAMPLE_MAX_TAPS, max_span beyond NPLDA_RESAMPLE_MAX_LDS_BYTES, counts beyond the int32 indexing; NPLDA_EINVAL: a
 * missing or misaligned pointer, a non-positive maximum.  n_utts == 0 is a no-op.  No floating-point atomics: the same bits
 * on every call, and an utterance's bits do not depend on the batch, the chunking or the order. */
int nplda_resample_batch(const nplda_resample_call* call, nplda_stream_t stream);

/* ---- measurement utility ------------------------------------------------------------------------------------- */

/* Shader-clock probe for bench.py (no reference counterpart): one wave that stays resident for window_us microseconds
 * on `stream` and writes out2[0] = shader cycles elapsed (s_memtime), out2[1] = ticks of the constant 100 MHz counter
 * (s_memrealtime) to DEVICE memory; MHz = 100 * out2[0] / out2[1].  Launched on a side stream next to the kernel under
 * test it reports the clock the chip actually holds under that kernel (the roofline peak assumes 2.4 GHz). */
int nplda_clock_probe(uint64_t* out2, unsigned window_us, nplda_stream_t stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* NPLDA_HIP_H */
