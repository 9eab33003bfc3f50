/*
 * gkg_hip.h — C ABI of libgkg_hip.so: the MI355X (gfx950) implementation of GKGNet's
 * Group-KNN graph-convolution hot path.
 *
 * The reference (jin-s13/GKGNet) has no native boundary: the path is a chain of ATen ops inside
 * DyGraphConv2d*.forward.  The operator boundary this library introduces sits exactly at the two
 * calls made there (paths relative to the reference tree):
 *
 *   self.dilated_knn_graph(x, y, relative_pos)        mmcls/models/backbones/vig_model/torch_vertex.py:203,226,247,272
 *        -> DenseDilatedKnnGraph.forward              .../vig_model/torch_edge.py:164-176   ==> gkg_knn_fwd
 *   GraphConv2d.forward(x, edge_index, y) / MRConv2d  .../vig_model/torch_vertex.py:47-54   ==> gkg_mr_fwd
 *        (batched_index_select x2 + max(x_j - x_i))   .../vig_model/torch_nn.py:84-105
 *   autograd of the above (max_backward, index_put_)  (ATen; SURVEY.md §8a "Backward contract")  ==> gkg_mr_bwd
 *
 * Conventions
 *   - All pointers are DEVICE pointers owned by the caller; tensors are contiguous, channel-major
 *     exactly like the reference's (B*G, c, N, 1) layout:   x[bg][ch][n].
 *   - Every call is asynchronous on `stream` (a hipStream_t passed as void*); the library never
 *     synchronises, allocates or frees, and keeps no mutable global state besides the last-error
 *     string (thread-local).  Workspace, when needed, is passed in by the caller.
 *   - Return value: 0 on success; >0 a hipError_t from a launch; <0 an argument error
 *     (GKG_ERR_*).  Nothing throws or exits.
 *   - dtype: element type of the feature tensors x / y / src / g / outputs (GKG_F32, GKG_BF16, GKG_F16).  Distances are
 *     always accumulated in fp32 (SURVEY.md §5 AMP row).
 *
 * Arithmetic contract of gkg_knn_fwd (restated bit-for-bit by oracle/gkg_oracle.c):
 *     s      = fma-chain_{ch} t[ch]^2            den = max(sqrt(s), 1e-12)       (GKG_KNN_NORMALIZE)
 *     th[ch] = t[ch] / den                       sq  = fma-chain_{ch} th[ch]^2
 *     dot    = fma-chain_{ch=0..c-1} yh[ch][m] * xh[ch][n]      (fp32 MFMA == ordered fmaf chain)
 *     dist   = ((sqx[n] + (-2*dot)) + sqy[m]) + relpos[n][m]    (reference op order, torch_edge.py:17-20,82)
 *     neighbours = the k*dilation smallest (dist, m) pairs in ascending lexicographic order
 *                  (tie rule: smaller key index first); ranks 0, d, 2d, ... are emitted.
 */
#ifndef GKG_HIP_H_
#define GKG_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GKG_ABI_VERSION 22

/* dtype codes */
#define GKG_F32 0
#define GKG_BF16 1
#define GKG_F16 2 /* the reference trains under fp16 AMP (configs/gkgnet/gkgnet_coco_576.py:146): inputs widened exactly */

/* gkg_knn_fwd flags */
#define GKG_KNN_NORMALIZE 1u /* L2-normalise tokens over the group's channels first (torch_edge.py:167-173) */
#define GKG_KNN_BF16_CONTRACT 2u /* x.y^T on the bf16 matrix cores.  For callers under bf16 autocast, where the reference computes
                                  * this product in bf16 and rounds it to bf16.  Token preparation is the contract's (s, den, th, sq
                                  * above; sq from the UNROUNDED fp32 th); the distance is
                                  *     dist = ( relpos[n][m] + sum_ch (-2 bf(xh[ch][n])) * bf(yh[ch][m]) ) + sqy[m]
                                  * bf = bf16 round-to-nearest-even of the fp32 th; the products are exact, the accumulator is fp32
                                  * and STARTS at relpos[n][m] (0 without a bias), sqy[m] is added last in fp32; the query's own
                                  * |x|^2 (one constant per query: no effect on the order) is left out.  Only the order of the c
                                  * additions inside the 16-deep matrix-core steps is the hardware's, so a distance lies within
                                  * (c + 2) 2^-24 (max|relpos| + 3.1) of its real value for normalised tokens
                                  * (tests/knn_bf16_ref.py).  Neighbour rule as above (ties: smaller key index first).  Outside the
                                  * bit-exact index contract; ignored for c < 9 (the call is then the fp32 contract).  Not with
                                  * GKG_KNN_X_PREPARED / GKG_KNN_Y_PREPARED or as knn_flags of a preparing producer
                                  * (GKG_ERR_UNSUPPORTED). */
#define GKG_KNN_SELECT_DIRECT 4u   /* force the direct sorted insert / the buffered selection of the tile kernel instead of */
#define GKG_KNN_SELECT_BUFFERED 8u /* the library's per-shape rule (measurement, tests): identical results either way */
#define GKG_KNN_NO_PREFILTER 16u   /* evaluate every distance with the contract's fp32 chain (knn_tile_kernel) instead of the
                                    * bf16 matrix-core prefilter + exact re-rank of the survivors (knn_pf_kernel): identical
                                    * results either way (measurement, tests) */
#define GKG_KNN_FORCE_PREFILTER 32u /* take the prefilter kernel wherever it is applicable (normalised tokens, un-split keys,
                                    * k*dilation <= 36, c >= 16), not only where the library's rule says it pays (tests) */
#define GKG_KNN_RELPOS_UNIT 64u     /* the caller guarantees |relative_pos| <= 1.125 everywhere (GKGNet's bias -2 PE PE^T / D lies
                                    * in [-1, 0], pos_embed.py:21-29; its bicubic resize for pooled keys, torch_vertex.py:311-315,
                                    * can overshoot by a fraction of a percent): precondition of the prefilter kernel's error
                                    * bound when a bias is given.  Without it a call with a bias always takes knn_tile_kernel (same results,
                                    * no range assumption) */

#define GKG_KNN_X_PREPARED 128u     /* token-major fp32 callers: the queries' normalised copies / norms (/ prefilter planes) are already
                                    * in `workspace`, left there by gkg_bn_apply_knn_prep called with the same problem — the call
                                    * launches no preparation for them (none at all for a self graph) */
#define GKG_KNN_Y_PREPARED 256u     /* likewise for the KEYS (gkg_bn_apply_knn_prep with as_keys: a label graph's keys, produced by the
                                    * Grapher in front of it) */
#define GKG_KNN_F16_CONTRACT 512u   /* x.y^T on the fp16 matrix cores (v_mfma_f32_32x32x16_f16: the bf16 form's rate), for callers under
                                    * 16-bit autocast who want fewer changed neighbours than GKG_KNN_BF16_CONTRACT gives: normalised
                                    * tokens lie in [-1, 1], where fp16 rounds 2^-12 relative against bf16's 2^-9.  Accepted by
                                    * gkg_knn_fwd, gkg_knn_fwd_tm, gkg_knn_fwd_tm16 and gkg_knn_workspace_bytes (the workspace plan is
                                    * the bf16 form's: planes of the same size).  Token preparation is the contract's (s, den, th, sq
                                    * above; sq from the UNROUNDED fp32 th); the planes hold h(th) = fp16 round-to-nearest-even of the
                                    * fp32 th, with a result of magnitude below 2^-14 (an fp16 subnormal) replaced by +0; the distance is
                                    *     dist = ( relpos[n][m] + sum_ch (-2 h(xh[ch][n])) * h(yh[ch][m]) ) + sqy[m]
                                    * The products are exact in fp32 (11 x 11 significand bits, exponents >= 2^-28), the accumulator
                                    * is fp32 and STARTS at relpos[n][m] (0 without a bias), sqy[m] is added last in fp32, the query's
                                    * own |x|^2 is left out.  Only the order of the c additions inside the 16-deep matrix-core steps
                                    * is the hardware's: a distance lies within (c + 2) 2^-24 (max|relpos| + 3.1) of its real value
                                    * (tests/knn_f16_ref.py).  Neighbours: the k d smallest (dist, m) pairs, smaller index first on
                                    * equal distance; ranks 0, d, 2d, ... are emitted.  The flush is a decision of this definition:
                                    * the result does not depend on what the matrix core does with subnormal inputs, and -2 h(x) is
                                    * an exact exponent step (a zero exponent field means zero).
                                    *   GKG_ERR_UNSUPPORTED, nothing launched: without GKG_KNN_NORMALIZE (raw tokens can overflow
                                    * fp16); together with GKG_KNN_BF16_CONTRACT; with GKG_KNN_X_PREPARED / GKG_KNN_Y_PREPARED; as
                                    * knn_flags of gkg_bn_apply_knn_prep[_sync], gkg_affine_knn_prep or gkg_linear_bf16_knn_prep;
                                    * through gkg_knn_mr_fwd_tm.  gkg_knn_mr_fused_supported and gkg_linear_bf16_knn_prep_supported
                                    * answer 0.  The prefilter is never taken.  Outside the bit-exact index contract; ignored for
                                    * c < 9 (the call is then the fp32 contract). */

/* argument errors */
#define GKG_ERR_NULL -1        /* required pointer is NULL */
#define GKG_ERR_SHAPE -2       /* non-positive / inconsistent sizes, k*dilation > M, ... */
#define GKG_ERR_UNSUPPORTED -3 /* dtype / size outside what this build supports */
#define GKG_ERR_WORKSPACE -4   /* workspace too small (gkg_linear_wgrad_x6_det: also NULL or not 16-byte aligned) */

/* ABI version of the loaded library (== GKG_ABI_VERSION it was built with). */
int gkg_version(void);
/* Identifier of the hipGraph capture `stream` is recording into; 0 when it is not capturing. */
unsigned long long gkg_stream_capture_id(void* stream);

/* Human-readable description of the last non-zero return on this thread ("" if none). */
const char* gkg_last_error_string(void);

/* Bytes of scratch gkg_knn_fwd needs for these sizes (normalised token copies, squared norms,
 * split-key partial lists).  Pure function of its arguments. */
size_t gkg_knn_workspace_bytes(int BG, int c, int N, int M, int k, int dilation, int dtype, unsigned flags);

/*
 * Dilated k-NN graph.  Replaces DenseDilatedKnnGraph.forward (torch_edge.py:164-176) including
 * dense_knn_matrix / xy_dense_knn_matrix (:54-106), pairwise distance (:9-51) and DenseDilated (:139-149).
 *   x        (BG, c, N)      query tokens
 *   y        (BG, c, M)      key tokens, or NULL for the self graph (then M must equal N)
 *   relpos   (N, M) fp32     positional bias shared by all BG problems, or NULL
 *   nn_idx   (BG, N, k) i64  out: neighbour index per query, ascending distance  (== edge_index[0])
 *   center   (BG, N, k) i64  out, optional (NULL to skip): centre index n         (== edge_index[1])
 */
int gkg_knn_fwd(const void* x, const void* y, const float* relpos, int64_t* nn_idx, int64_t* center,
                int BG, int c, int N, int M, int k, int dilation, int dtype, unsigned flags,
                void* workspace, size_t workspace_bytes, void* stream);

/*
 * Max-relative aggregation: m[bg][ch][n] = max_j ( src[bg][ch][nn_idx[bg][n][j]] - x[bg][ch][n] ).
 * Replaces batched_index_select x2 + torch.max(x_j - x_i, -1) (torch_vertex.py:49-54, torch_nn.py:84-105).
 *   src      (BG, c, M) or NULL (-> src = x, M = N)
 *   m_out    (BG, c, N)
 *   argmax   (BG, c, N) u8   out, optional: first j attaining the max (needed by gkg_mr_bwd)
 * An nn_idx entry outside [0, M) is clamped on its full 64-bit value (< 0 -> 0, >= M -> M - 1): never an out-of-bounds read.
 * The maximum follows torch.max: the first of equal values wins, a NaN difference is the maximum and the first NaN stays.
 */
int gkg_mr_fwd(const void* x, const void* src, const int64_t* nn_idx, void* m_out, uint8_t* argmax,
               int BG, int c, int N, int M, int k, int dtype, void* stream);

/*
 * Backward of gkg_mr_fwd for upstream gradient g (BG,c,N) on m:
 *     gx[bg][ch][n]                        = -g[bg][ch][n]
 *     gsrc[bg][ch][nn_idx[bg][n][argmax]] +=  g[bg][ch][n]
 *   gsrc == NULL  -> self graph: both terms are accumulated into gx (M must equal N).
 *   gx, gsrc are fully overwritten (no pre-zeroing needed).
 * The destination row is clamped exactly as the forward clamps its gathers: the slot as min(argmax, k - 1), then the entry it
 * names on its full 64-bit value (< 0 -> 0, >= M -> M - 1) — never an out-of-bounds access, whatever argmax and nn_idx hold.
 * The fan-in of a row is summed with fp32 atomics (in LDS; in global memory when one row of M accumulators exceeds the LDS
 * budget — fp32 tensors only there, GKG_ERR_UNSUPPORTED for bf16 / fp16): any summation order, so the last bits may differ
 * from run to run; |error| <= fan_in * 2^-24 * sum|addend| to first order (the self graph's -g counts as one addend), and a
 * bf16 / fp16 result is that fp32 sum rounded once.  Gradients whose partial sums are all exact in fp32 give the exact result.
 */
int gkg_mr_bwd(const void* g, const int64_t* nn_idx, const uint8_t* argmax, void* gx, void* gsrc,
               int BG, int c, int N, int M, int k, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * EdgeConv aggregation (Grapher(conv='edge'); reference torch_vertex.py:82-101 EdgeConv2d.forward + torch_nn.py:57-69
 * BasicConv).  The reference evaluates  max_k act(norm(Conv2d_1x1,groups=4(cat[x_i, x_j - x_i])))  on a (B, 2C, N, k)
 * tensor.  With the hard-coded groups = 4 the output channels of groups 2 and 3 depend on (x_j - x_i) only, and the
 * convolution is linear, so for them z[b][o][n][k] = Q[b][o][nn_idx[b][n][k]] - Qc[b][o][n] + bias[o] with the per-node
 * projections Q = W src, Qc = W x (ordinary GEMMs in the caller: k times less work, no (B, 2C, N, k) tensor).  These four
 * entry points are the gather side; channel-major fp32 (B, O, N) / (B, O, M), nn_idx (B, N, k) int64, k <= 255.  Out-of-range
 * nn_idx entries are clamped into [0, M) (all four: never an out-of-bounds read or atomic).
 *   gkg_edge_stats      sums[o] += sum (Q[j] - Qc), sums[O + o] += sum (Q[j] - Qc)^2 over all (b, n, k): the batch statistics
 *                       of train-mode BN (the bias shifts the mean only).  sums: 2*O doubles, zero on entry.
 *   gkg_edge_fwd        out = max_k act(a[o] (Q[j] - Qc) + c[o]); argmax (optional) = first maximising k.  The caller folds
 *                       norm and bias into a, c.  act: 0 none, 1 GELU (erf), 2 ReLU.
 *   gkg_edge_bwd_stats  sums[o] += sum_n g', sums[O + o] += sum_n g' zhat over the argmax elements, g' = g act'(.), zhat =
 *                       (z - mean0) invstd: dbeta, dgamma and (divided by B N k) the two means of the BN backward.
 *   gkg_edge_bwd        dz[n][k] = a (g' [k == argmax] - mg - zhat[n][k] mgz) for every edge; dqs[nn_idx] += dz (atomics; dqs
 *                       zero on entry), dqc[n] = -sum_k dz.  mg == NULL: statistics are constants, only the winning edge
 *                       carries gradient.
 *   qc == NULL (all four): Qc is zero, z = Q[nn_idx] + bias — GraphSAGE's nn1 applied to the gathered neighbours
 *                       (Grapher(conv='sage'); reference torch_vertex.py:116-131).  dqc may then be NULL (it is written
 *                       when given).  A non-NULL qc computes exactly what it did before. */
int gkg_edge_stats(const float* qs, const float* qc, const int64_t* nn_idx, double* sums, int B, int O, int N, int M, int k,
                   void* stream);
int gkg_edge_fwd(const float* qs, const float* qc, const int64_t* nn_idx, const float* a, const float* c, float* out,
                 uint8_t* argmax, int B, int O, int N, int M, int k, int act, void* stream);
int gkg_edge_bwd_stats(const float* g, const float* qs, const float* qc, const int64_t* nn_idx, const uint8_t* argmax,
                       const float* a, const float* c, const float* mean0, const float* invstd, double* sums, int B, int O,
                       int N, int M, int k, int act, void* stream);
int gkg_edge_bwd(const float* g, const float* qs, const float* qc, const int64_t* nn_idx, const uint8_t* argmax,
                 const float* a, const float* c, const float* mean0, const float* invstd, const float* mg, const float* mgz,
                 float* dqs, float* dqc, int B, int O, int N, int M, int k, int act, void* stream);

/* ------------------------------------------------------------------------------------------------
 * GIN and graph-attention aggregations (Grapher(conv='gin' / 'gat'); reference torch_vertex.py:134-150 GINConv2d and
 * :16-37 GraphAtten).  Channel-major fp32 x (B, C, N), src (B, C, M) or NULL (self graph: src = x, M == N), nn_idx (B, N, k)
 * int64 (== edge_index[0]; out-of-range entries are clamped into [0, M)).  The centre of every edge is the query itself
 * (edge_index[1][b][n][k] == n, as the k-NN produces it), so edge_index[1] is not an argument.  No (B, C, N, k) tensor is
 * formed, and every backward is bit-identical from run to run: the source gradients are gathers over the transposed graph
 * (built in the workspace, each key's edges in edge order), the parameter gradients fixed-order fp64 reductions.
 *   gkg_gconv_workspace_bytes  workspace the calls below need (0: invalid sizes).  ws: device memory whose base is aligned to 8
 *                 bytes (it holds int32, fp32 and, at 256-byte offsets, fp64 sections); its contents on entry do not matter (a
 *                 dirty buffer is fine: every section is written before it is read) and nothing in it outlives the call, so one
 *                 buffer of the largest size serves forward, backward and any smaller shape in turn.  ws_bytes below the
 *                 requirement returns GKG_ERR_WORKSPACE with nothing written.  Every launch of a call is a kernel (no memset
 *                 or copy nodes when the stream is being captured into a hipGraph).
 *   gkg_gin_fwd   h[b][c][n] = (1 + eps[0]) x[b][c][n] + sum_k src[b][c][nn_idx[b][n][k]]   (eps: 1 float in device memory)
 *   gkg_gin_bwd   gx = (1 + eps) gh; gsrc[j] += gh[n] over every edge (gsrc == NULL: into gx, self graph); geps (optional,
 *                 1 double) = sum gh x.  gx, gsrc, geps are fully overwritten.
 *   gkg_gat_fwd   a: 2C floats (the Conv2d(2C, 1, 1) weight), bias: 1 float or NULL.  t[n] = a[:C] . x[n] + bias,
 *                 s[m] = a[C:] . src[m], p[b][n][k] = softmax_k(t[n] + s[nn_idx]) (max-subtracted; (B, N, k) out, the
 *                 backward's input), agg[b][c][n] = sum_k p src[c][nn_idx].
 *   gkg_gat_bwd   g = d agg.  dp = g[n] . src[j], de = p (dp - sum_k p dp); gsrc[j] += p g[n] + de a[C:] (src and gsrc both
 *                 NULL: self graph, into gx); gx[n] += (sum_k de) a[:C]; da (optional, 2C doubles) = [sum (sum_k de) x[n],
 *                 sum de src[j]]; dbias (optional, 1 double) = sum de.  All outputs fully overwritten.  p is an input like any
 *                 other: any (B, N, k) floats are accepted and used as given (rows need not sum to 1, nothing is recomputed
 *                 from x, src and a), so the result is the formula above evaluated at that p. */
size_t gkg_gconv_workspace_bytes(int B, int C, int N, int M, int k);
int gkg_gin_fwd(const float* x, const float* src, const int64_t* nn_idx, const float* eps, float* h, int B, int C, int N, int M,
                int k, void* stream);
int gkg_gin_bwd(const float* gh, const float* x, const float* eps, const int64_t* nn_idx, float* gx, float* gsrc, double* geps,
                int B, int C, int N, int M, int k, void* ws, size_t ws_bytes, void* stream);
int gkg_gat_fwd(const float* x, const float* src, const int64_t* nn_idx, const float* a, const float* bias, float* agg, float* p,
                int B, int C, int N, int M, int k, void* ws, size_t ws_bytes, void* stream);
int gkg_gat_bwd(const float* g, const float* x, const float* src, const int64_t* nn_idx, const float* a, const float* p, float* gx,
                float* gsrc, double* da, double* dbias, int B, int C, int N, int M, int k, void* ws, size_t ws_bytes,
                void* stream);

/* ------------------------------------------------------------------------------------------------
 * Token-major variants used inside the fused Grapher block (activations (B, N, C), C = G*c, fp32).
 * Same arithmetic contracts as above; only the addressing differs.
 *   gkg_knn_fwd_tm : x (B,N,C), y (B,M,C) or NULL; nn_idx/center (B*G, N, k)
 *   gkg_mr_fwd_tm  : mode 0 -> out = m (B,N,C);
 *                    mode 1 -> out = XM (B*N, 2C): the grouped projection's operand buffer (see "XM layout" below);
 *                              needs C % 16 == 0
 *                    argmax (B,N,C) u8
 *   gkg_mr_bwd_tm  : mode 0: gin = g (B,N,C); mode 1: gin = dXM (B*N, 2C) in the XM layout (x chunks = gradient reaching x
 *                    directly, m chunks = gradient of m).  gx (B,N,C) and gsrc (B,M,C)|NULL fully overwritten.
 *                    Default for destination images of up to 512 rows (where it measured faster; with
 *                    GKG_MR_DETERMINISTIC wherever 8 channels of 64-bit accumulators per row fit the LDS): EXACT fixed-point
 *                    accumulation — every gradient becomes sign * (24-bit mantissa << shift) relative to the chunk's
 *                    largest magnitude, the fan-in is summed with 64-bit integer LDS atomics and rounded ONCE to fp32:
 *                    independent of the arrival order (bit-identical from run to run) and at least as accurate as an
 *                    fp32 sum; non-finite gradients fall back to fp32 atomics per chunk (inf / NaN propagate).
 *                    From 160 query rows per image the same accumulation runs in ONE sweep (round 5): the scale comes from
 *                    a strided sample of the chunk's rows plus 6 binary orders of headroom (the exact maximum when a thread's
 *                    first rows are the whole sweep); a gradient beyond the headroom makes that workgroup redo its chunk with
 *                    the exact two-sweep form.  Still order-independent and bit-identical from run to run.
 *                    flags & GKG_MR_FP32_ATOMICS: the round-1 fp32 LDS-atomic kernels (fan-in summed in arrival order);
 *                    flags & GKG_MR_DETERMINISTIC (shapes beyond the LDS budget): private accumulators, fixed order.
 *                    Destination rows: arg_kind 0 — the slot is clamped to min(argmax, k - 1) and the nn_idx entry it names on
 *                    its full 64-bit value (< 0 -> 0, >= M -> M - 1); arg_kind 1 — min(row, M - 1), nn_idx is not read and may
 *                    be NULL.  Every form clamps: no out-of-bounds access, whatever argmax and nn_idx hold.
 *                    gx = direct - g in fp32 (direct = 0 in mode 0); the self graph adds it to the row's sum as one more fp32
 *                    operation.  Order-independent (the same bits from run to run, whatever the order the lanes arrive in):
 *                    the fixed-point forms (two-sweep and streaming).  Fixed order, also the same bits from run to run: the
 *                    private-accumulator form and the ordered walk of GKG_MR_DETERMINISTIC (fp32 additions in query order).
 *                    Arrival order: the fp32-atomic forms — LDS images of more than 512 rows under fewer than 160 query rows,
 *                    images beyond the LDS budget (global atomics), GKG_MR_FP32_ATOMICS, and the chunk of a fixed-point
 *                    workgroup that meets an inf / NaN; there |error| <= fan_in * 2^-24 * sum|addend| to first order.
 *                    Exactness of the fixed-point forms: a row's sum is float32(the exact sum), rounded once, whenever no
 *                    addend loses bits and the integer total passes through a double unrounded, i.e. when every |g| of the
 *                    (image, channel chunk) lies within a factor 2^(SHMAX - 6) of the chunk's largest (SHMAX = 38 - bits(N); the
 *                    6 is the streaming form's headroom, the two-sweep form needs none) and 24 + s + bits(N) <= 53 for gradients
 *                    spread over s binary orders: e.g. any gradients spread over up to 8 binary orders, subnormal ones included,
 *                    at N <= 4095.  Smaller addends are truncated toward zero below 2^-SHMAX of the scale.
 *
 * XM layout (round 6) — the reference's MRConv2d interleaves [x_0, m_0, x_1, m_1, ...] (torch_vertex.py:57-61) and feeds
 * Conv2d(2C, 2C, 1, groups=4) (torch_nn.py:61): conv group q reads interleaved channels [q C/2, (q+1) C/2) = the x and m values
 * of original channels [q h, (q+1) h), h = C/4.  Nothing is interleaved here.  The grouped projection's operand is ONE buffer
 *     XM (T, 2C) fp32,   row t = [x_0 | m_0 | x_1 | m_1 | x_2 | m_2 | x_3 | m_3],   x_q = x[t][q h .. (q+1) h), m_q likewise,
 * i.e. group q's 2h inputs are contiguous with the x half first; the weight's input columns are reordered to match when its
 * bf16 planes are built (gkg_x6_prep_desc_fill kperm) and the weight gradient is permuted back where it is added to dW
 * (GkgWgradProblem.kperm) — the weight tensor keeps the reference's layout.  The PRODUCER of x (the Grapher's fc1 BN-apply:
 * gkg_bn_apply_train / gkg_affine_act with ochunk = h and ldo = 2C) writes x straight into the x chunks, the aggregation
 * (gkg_knn_mr_fwd_tm / gkg_mr_fwd_tm mode 1) fills the m chunks and, in the backward, the grouped input-gradient GEMM writes
 * dXM in the same layout (gkg_linear_dgrad_x6_sk ldx = 2C, x_bstride = 2h) for gkg_mr_bwd_tm mode 1: x is never copied.
 * Token-major fp32 inputs are therefore passed as VIEWS (pointer, row pitch ld, chunk): channel ch of token t sits at
 * p[t * ld + ch + (ch / chunk) * chunk] for chunk > 0 (chunk % 4 == 0, chunk | C, ld >= 2C: the x half of an XM buffer is
 * (XM, 2C, h)), at p[t * ld + ch] for chunk == 0; ld == 0 means ld = C.  A self graph gathers its neighbours through the same view.
 * When x passed to a mode-1 aggregation IS the output buffer's x half (x == out, ldx == 2C, xchunk == h) only m is written;
 * otherwise both halves are (a caller whose x lives elsewhere).
 */
int gkg_knn_fwd_tm(const void* x, int ldx, int xchunk, const void* y, const float* relpos, int64_t* nn_idx, int64_t* center,
                   int B, int G, int c, int N, int M, int k, int dilation, int dtype, unsigned flags,
                   void* workspace, size_t workspace_bytes, void* stream);
/* The Grapher's fc1 BN-apply and the k-NN's token preparation in ONE pass (round 6; reference torch_vertex.py:326 fc1's BN ->
 * torch_edge.py:167-173 F.normalize + |x|^2).  y (B N, C = G c) is fc1's pre-BN projection output whose train-mode batch
 * statistics lie in `sums` (gkg_linear_bn_fwd_x6 with train == 2; everything about sums / a / c / mean / invstd / running
 * statistics / zero_buf is gkg_bn_apply_train's contract with nb == 1, act == 0, no residual).  x = a y + c goes to `out` (row
 * pitch ldo floats, 0 = C; ochunk > 0: the x half of the grouped projection's operand buffer, "XM layout") and, from the same
 * registers, normalised into `knn_workspace`: the workspace of the k-NN call (gkg_knn_fwd_tm / gkg_knn_fwd_tm16 /
 * gkg_knn_mr_fwd_tm — fused_mr != 0 for the latter) with the SAME B, G, c, N, M, k, dilation, presence of y / relative_pos and
 * flags, which follows with GKG_KNN_X_PREPARED set and x = out.  Same operations in the same order per value as gkg_bn_apply_train
 * followed by that call's own preparation: bit-identical x, graphs and aggregation.
 * as_keys != 0 — the KEYS of the problem instead (a GrapherLabel's keys are the feature map a Grapher in front of it returns,
 * torch_vertex.py:331 -> :392-403): y (B M, C) is that Grapher's fc2 pre-BN output, res_tm (B M, C) or NULL its token-major
 * residual; a y + c + res_tm goes to `out` (B M, C) plain (the token-major companion the label block gathers its values from), to
 * out_nchw (B, C, M) or NULL (the block's channel-major result) and, normalised, into the keys' part of the label call's workspace;
 * that call then sets GKG_KNN_Y_PREPARED (and GKG_KNN_X_PREPARED when its own fc1 prepared the queries into the same workspace). */
int gkg_bn_apply_knn_prep(const float* y, const double* sums, const float* gamma, const float* beta, const float* bias,
                          float* running_mean, float* running_var, long long* num_batches_tracked, float* a, float* c_out,
                          float* mean, float* invstd, float* out, int ldo, int ochunk, int B, int G, int c, int N, int M, int k,
                          int dilation, int has_y, int has_relpos, unsigned knn_flags, int fused_mr, int as_keys, const float* res_tm,
                          float* out_nchw, void* knn_workspace, size_t knn_workspace_bytes, float momentum, float eps, double* zero_buf,
                          size_t zero_doubles, void* stream);
/* gkg_bn_apply_knn_prep behind a cross-rank exchange of the statistics (SyncBatchNorm): `sums` added up over the ranks, `count` /
 * `count_out` as in gkg_bn_apply_train_sync (B: this rank's images). */
int gkg_bn_apply_knn_prep_sync(const float* y, const double* sums, const float* gamma, const float* beta, const float* bias,
                               float* running_mean, float* running_var, long long* num_batches_tracked, float* a, float* c_out,
                               float* mean, float* invstd, float* out, int ldo, int ochunk, int B, int G, int c, int N, int M, int k,
                               int dilation, int has_y, int has_relpos, unsigned knn_flags, int fused_mr, int as_keys,
                               const float* res_tm, float* out_nchw, void* knn_workspace, size_t knn_workspace_bytes, float momentum,
                               float eps, double* zero_buf, size_t zero_doubles, const double* count, float* count_out, void* stream);
/* The eval-mode (frozen BatchNorm) counterpart of gkg_bn_apply_knn_prep: the caller passes the folded scale / shift a, c
 * (C = G c each; gkg_bn_eval_affine) instead of column sums.  out = fmaf(a, y, c) (+ res_tm for a keys producer) — the bits of
 * gkg_affine_act (queries: out / ldo / ochunk as above) or gkg_tm_affine_to_nchw_dual (as_keys: out (B M, C) plain, out_nchw
 * (B, C, M)) — and, from the same registers, the k-NN call's own token preparation into `knn_workspace`; the k-NN call with the
 * same problem follows with GKG_KNN_X_PREPARED (GKG_KNN_Y_PREPARED for as_keys).  Writes nothing but out, out_nchw and the
 * workspace: no saved statistics, no running statistics, no scratch buffer.  Every other argument as gkg_bn_apply_knn_prep. */
int gkg_affine_knn_prep(const float* y, const float* a, const float* c_in, float* out, int ldo, int ochunk, int B, int G, int c,
                        int N, int M, int k, int dilation, int has_y, int has_relpos, unsigned knn_flags, int fused_mr, int as_keys,
                        const float* res_tm, float* out_nchw, void* knn_workspace, size_t knn_workspace_bytes, void* stream);
/* Pooled key set of a Grapher with r > 1 (reference torch_vertex.py:194-196, F.avg_pool2d(x, r, r)) from a token-major map
 * x (B, H, W, C) given as a view -> out (B, H/r, W/r, C) plain fp32 (floor mode; window sum in (h, w) order, one division). */
int gkg_avgpool_tm(const float* x, int ldx, int xchunk, float* out, int B, int H, int W, int C, int r, void* stream);

/* Compact graph (round 5): gkg_knn_fwd_tm's neighbour lists as u16 rows, nn16 (B*G, N, k), INSTEAD of the int64 planes — for
 * callers that consume the graph on the device and do not hand it out (Grapher.forward discards it, reference
 * torch_vertex.py:330): no int64 index plane, no centre plane (GKGNet-576 stage 1: 24 MB written per launch instead of 191 MB).
 * Same contract, same neighbours in the same order as gkg_knn_fwd_tm; M <= 65536.  gkg_mr_fwd_tm16 / gkg_mr_linear_bf16_nn16
 * are gkg_mr_fwd_tm / gkg_mr_linear_bf16 reading these lists (same outputs, same bits). */
int gkg_knn_fwd_tm16(const void* x, int ldx, int xchunk, const void* y, const float* relpos, uint16_t* nn16, int B, int G, int c,
                     int N, int M, int k, int dilation, int dtype, unsigned flags, void* workspace, size_t workspace_bytes,
                     void* stream);
int gkg_mr_fwd_tm16(const float* x, int ldx, int xchunk, const float* src, const uint16_t* nn16, void* out /* out_dtype elements */,
                    uint8_t* argmax, int B, int G, int c, int N, int M, int k, int mode, int out_dtype, int arg_kind, void* stream);

/* Row g2 (round 5): the k-NN graph AND the max-relative aggregation over it in ONE kernel, for token-major fp32 callers — the
 * reference chain DenseDilatedKnnGraph.forward (torch_edge.py:164-176) -> MRConv2d.forward's two batched_index_select + max
 * (torch_vertex.py:49-61) without the (2, B*G, N, k) int64 edge_index in between.  x (B, N, C = G*c), y (B, M, C) or NULL (self
 * graph), relative_pos (N, M) or NULL; flags as gkg_knn_fwd (GKG_KNN_NORMALIZE ...).  The graph is the one gkg_knn_fwd_tm
 * builds (same contract, same bits); it is consumed by the workgroup that built it:
 *   xm_out  (B*N, 2C) fp32      the grouped projection's operand buffer (XM layout), exactly gkg_mr_fwd_tm(mode 1)'s output:
 *                                m into the m chunks, x into the x chunks unless x is that buffer's x half already
 *   arg_out (B, N, C)     u16   the winning neighbour ROW per channel, exactly gkg_mr_fwd_tm(arg_kind 1)'s argmax (the
 *                                backward gkg_mr_bwd_tm(arg_kind 1) scatters from it and needs no index tensor)
 *   nn16_out (B*G, N, k)  u16   the neighbour lists, or NULL (M <= 65536)
 *   nn_idx_out, center_out (B*G, N, k) int64   gkg_knn_fwd_tm's outputs, or NULL: only for callers that RETURN the graph
 *                                (GrapherLabel.forward, torch_vertex.py:403); a Grapher never materialises them
 * gkg_knn_mr_fused_supported: 1 when this shape takes the fused form — the fp32 tile kernel with merged per-wave lists (no
 * key splits, no prefilter, lists of <= 36 entries, k <= 18, c % 4 == 0, C % 16 == 0); otherwise call gkg_knn_fwd_tm and
 * gkg_mr_fwd_tm.  Workspace: gkg_knn_workspace_bytes. */
int gkg_knn_mr_fused_supported(int B, int G, int c, int N, int M, int k, int dilation, int has_y, int has_relpos, unsigned flags);
int gkg_knn_mr_fwd_tm(const float* x, int ldx, int xchunk, const float* y, const float* relative_pos, float* xm_out,
                      uint16_t* arg_out, uint16_t* nn16_out, int64_t* nn_idx_out, int64_t* center_out, int B, int G, int c, int N,
                      int M, int k, int dilation, unsigned flags, void* workspace, size_t workspace_bytes, void* stream);
/* arg_kind: what `argmax` holds — 0: (B,N,C) u8, the winning slot j (as gkg_mr_fwd); 1: (B,N,C) u16, the winning
 * neighbour's row index itself (M <= 65536), which lets the backward scatter without looking the index row up again.
 * An nn_idx entry outside [0, M) is clamped as in gkg_mr_fwd (int64 lists on the full 64-bit value; the u16 lists of
 * gkg_mr_fwd_tm16: >= M -> M - 1), and with arg_kind 1 the row stored is the CLAMPED one, always < M. */
int gkg_mr_fwd_tm(const float* x, int ldx, int xchunk, const float* src, const int64_t* nn_idx, void* out /* out_dtype elements */,
                  uint8_t* argmax, int B, int G, int c, int N, int M, int k, int mode, int out_dtype, int arg_kind,
                  void* stream);
#define GKG_MR_DETERMINISTIC 1u /* fixed summation order in the scatter: bit-identical results from run to run */
#define GKG_MR_FP32_ATOMICS 2u  /* keep the fp32 LDS-atomic scatter instead of the exact integer accumulation (measurement, tests) */
int gkg_mr_bwd_tm(const float* gin, const int64_t* nn_idx, const uint8_t* argmax, float* gx, float* gsrc,
                  int B, int G, int c, int N, int M, int k, int mode, int arg_kind, unsigned flags, void* stream);
/* gkg_mr_bwd_tm that is also the STATISTICS pass of the BN backward whose upstream gradient gx is (the layer x = BN(y) in front of
 * the aggregation; un-grouped, no activation): y (B*N, C), mean / invstd [C]; sums [2][C] fp64, ZERO on entry, receives sum gx
 * and sum gx * yhat with atomics, what gkg_bn_bwd_atomic's first launch would leave there — follow it with
 * gkg_bn_bwd_apply_from_sums.  gx / gsrc: the bits of gkg_mr_bwd_tm.  Returns GKG_ERR_UNSUPPORTED, with nothing launched, when
 * the shape or the flags select a scatter form that carries no statistics (mode 0, forced forms, fp32 atomics, destination images
 * beyond the LDS forms): run gkg_mr_bwd_tm and gkg_bn_bwd_atomic then. */
int gkg_mr_bwd_tm_bnstats(const float* gin, const int64_t* nn_idx, const uint8_t* argmax, float* gx, float* gsrc,
                          int B, int G, int c, int N, int M, int k, int mode, int arg_kind, unsigned flags,
                          const float* y, const float* mean, const float* invstd, double* sums, void* stream);
/* 1 when gkg_mr_bwd_tm_bnstats would run for these sizes and flags, 0 when it would return GKG_ERR_UNSUPPORTED (pure host code, the
 * call's own plan — csrc/gkg_mr_plan.h mr_bwd_tm_plan; for callers that book their scratch buffer before the call). */
int gkg_mr_bwd_tm_bnstats_supported(int B, int G, int c, int N, int M, int k, int mode, int arg_kind, int self_graph, unsigned flags);

/* ------------------------------------------------------------------------------------------------
 * SURVEY §8 row g1, inference: the aggregation as the OPERAND PRODUCER of the grouped 1x1 projection.
 * One launch replaces MRConv2d.forward's gather -> max(x_j - x_i) -> interleave -> BasicConv (Conv2d(2C, 2C, 1,
 * groups=4) + BN(eval) + GELU) chain (reference torch_vertex.py:47-62, torch_nn.py:57-69): the [x, m] tensor is built
 * tile by tile in LDS (bf16, round-to-nearest-even — the operand rounding of the reference's autocast convolution) and
 * consumed by v_mfma_f32_32x32x16_bf16 in place; it never exists in memory.
 *   x (B, N, C) fp32 token-major; src (B, M, C) fp32 or NULL (self graph); nn_idx (B*G, N, k) int64; C = G*c, C % 16 == 0
 *   wplanes: bf16 weight fragments [4][ci_pad/8][co_pad][8], ci = co = C/2, ci_pad = ci rounded up to 16, co_pad = co
 *            rounded up to 32: fragment (q, f, n) = W[q*co + n][8f .. 8f+7] (zero outside); gkg_mr_linear_planes_bytes(C)
 *   a, cshift (2C) fp32: out = act(a * conv + cshift) per output channel (eval-mode BN folded with the conv bias)
 *   out (B*N, ldo) bf16, columns [0, 2C) written (column q*co + n), ldo >= 2C, ldo % 8 == 0; act: 0 none, 1 GELU (erf)
 * The max-relative arithmetic is gkg_mr_fwd_tm's (bit-identical m before rounding), an nn_idx / nn16 entry outside [0, M)
 * included: it is clamped (< 0 -> 0, >= M -> M - 1). */
size_t gkg_mr_linear_planes_bytes(int C);
int gkg_mr_linear_bf16(const float* x, const float* src, const int64_t* nn_idx, const void* wplanes, const float* a,
                       const float* cshift, void* out, int ldo, int B, int G, int c, int N, int M, int k, int act,
                       void* stream);
int gkg_mr_linear_bf16_nn16(const float* x, const float* src, const uint16_t* nn16, const void* wplanes, const float* a,
                            const float* cshift, void* out, int ldo, int B, int G, int c, int N, int M, int k, int act,
                            void* stream);

/* ------------------------------------------------------------------------------------------------
 * Inference, bf16 operands: a dense 1x1 projection with its eval-mode BN, activation and residual as ONE launch
 * (csrc/gkg_linear_bf16.hip).  The layers are Conv2d(1x1) + BN of Grapher.fc1 / fc2 (reference torch_vertex.py:290-306), FFN.fc1 /
 * fc2 (gkgnet.py:46-72: fc1 + GELU, fc2 + shortcut) and the Conv2d + BN (+ GELU) of BasicConv (torch_nn.py:57-69), for callers under
 * bf16 autocast with gradients off.  Token-major rows:
 *   x (R, ldx) bf16, columns [0, cin) read
 *   wplanes: bf16 weight fragments [ci_pad/8][co_pad][8], fragment (f, n) = w[n][8f .. 8f+7] (zero outside cin / cout) — the
 *            gkg_mr_linear_bf16 layout with one group; ci_pad = cin rounded up to 16, co_pad = cout rounded up to 32;
 *            gkg_linear_bf16_planes_bytes(cin, cout) bytes (0: invalid sizes), the only place that encodes the paddings
 *   acc[r][n] = sum_k x[r][k] * w[n][k]         exact bf16 x bf16 products, fp32 accumulation on v_mfma_f32_32x32x16_bf16
 *   z = fmaf(a[n], acc, cshift[n])              a == NULL: z = acc + cshift[n] (a, cshift: [cout] fp32, e.g. gkg_bn_eval_affine)
 *   act == 1: z = GELU(z)                       the erf form all kernels of the library share (|erf error| <= 1.5e-7): the bits of
 *                                               gkg_affine_act's GELU
 *   res != NULL: z += res[r][n]                 res (R, ldr) fp32; an fp32 add AFTER the activation, the order of gkg_affine_act
 *   out_f32[r][n] = z (row pitch ldo32),  out_bf16[r][n] = round-to-nearest-even(z) (row pitch ldo16); at least one of the two is
 *   non-NULL, with both the bf16 output is the rounding of the fp32 one (gkg_affine_act_dual's pair).  Nothing outside columns
 *   [0, cout) of rows [0, R) of either output is written, nothing outside [0, cin) / [0, cout) of a row of x / res is read.
 * R, cin and cout need not be multiples of any tile; row offsets are 64-bit.  Preconditions, otherwise GKG_ERR_UNSUPPORTED with
 * nothing launched: R >= 1, cin % 8 == 0, cout % 8 == 0, ldx % 8 == 0, ldo16 % 8 == 0, ldo32 % 4 == 0, ldr % 4 == 0 (pitches of
 * absent operands are ignored), x / wplanes / res / out_f32 / out_bf16 16-byte aligned.  A pitch below its row's width is
 * GKG_ERR_SHAPE.  gkg_linear_bf16_supported: 1 when the sizes pass (pure host code; pitches and pointers are the call's to check). */
int gkg_linear_bf16_supported(int R, int cin, int cout, int has_res, int want_f32, int want_bf16, int act);
size_t gkg_linear_bf16_planes_bytes(int cin, int cout);
int gkg_linear_bf16(const void* x /* bf16 (R, ldx) */, int ldx, const void* wplanes,
                    const float* a /* [cout] or NULL = 1 */, const float* cshift /* [cout] */,
                    const float* res /* fp32 (R, ldr) or NULL */, int ldr,
                    float* out_f32 /* (R, ldo32) or NULL */, int ldo32,
                    void* out_bf16 /* (R, ldo16) or NULL */, int ldo16,
                    int R, int cin, int cout, int act /* 0 none, 1 GELU */, void* stream);
/* Grapher.fc1 under bf16 autocast with gradients off AND the token preparation of the k-NN call behind it, as ONE launch: the
 * projection above with R = B N rows, cout = G c, act == 0, no residual, fp32 result only, whose last workgroup per row tile also
 * prepares the rows it completes as the QUERIES of the k-NN problem (B, G, c, N, M, k, dilation, has_y, has_relpos, knn_flags,
 * fused_mr).  The arguments `out` .. `knn_workspace_bytes` are the producers' shared run of gkg_affine_knn_prep.  Bit for bit:
 *   out            = gkg_linear_bf16(x, ldx, wplanes, a, cshift, NULL, 0, out, ldo, NULL, 0, B N, cin, G c, 0, stream)
 *   knn_workspace  = what gkg_affine_knn_prep leaves there for the same problem, fed the raw accumulators with the same a / cshift:
 *                    the fp32 normalised channel-major copies with their zero pad channels, |t|^2 and, where that call's plan has
 *                    them, the bf16 hi / lo prefilter planes with their pad rows and the two |t|^2 channels
 * and the k-NN call with the same problem follows with GKG_KNN_X_PREPARED and x = out: it launches no preparation for the queries
 * (the keys of a problem with has_y are prepared by that call as always).
 * Scope, otherwise GKG_ERR_UNSUPPORTED with nothing launched: queries into plain rows only — ochunk == 0, as_keys == 0, res_tm ==
 * out_nchw == NULL, no GKG_KNN_BF16_CONTRACT / GKG_KNN_F16_CONTRACT in knn_flags; gkg_linear_bf16's preconditions (cin % 8, (G c) % 8, ldx % 8, ldo % 4,
 * 16-byte alignment; a pitch below its row's width is GKG_ERR_SHAPE) and c % 4 == 0; everything the k-NN plan itself refuses comes
 * back with that call's code.  ldo == 0 means G c.
 * scratch: gkg_linear_bf16_knn_prep_scratch_bytes(B N) bytes (one arrival counter per 128-row tile), caller-owned, 4-byte
 * aligned, ZERO on entry and left zero on exit: no memset per call, the launch can be captured in a graph.  Too small or NULL:
 * GKG_ERR_WORKSPACE.  gkg_linear_bf16_knn_prep_supported: 1 when sizes, flags and the k-NN plan pass (pure host code). */
size_t gkg_linear_bf16_knn_prep_scratch_bytes(int R);
int gkg_linear_bf16_knn_prep_supported(int cin, int B, int G, int c, int N, int M, int k, int dilation, int has_y, int has_relpos,
                                       unsigned knn_flags, int fused_mr);
int gkg_linear_bf16_knn_prep(const void* x /* bf16 (B N, ldx) */, int ldx, const void* wplanes, int cin,
                             const float* a /* [G c] or NULL */, const float* cshift /* [G c] */,
                             float* out, int ldo, int ochunk, int B, int G, int c, int N, int M, int k, int dilation,
                             int has_y, int has_relpos, unsigned knn_flags, int fused_mr, int as_keys,
                             const float* res_tm, float* out_nchw, void* knn_workspace, size_t knn_workspace_bytes,
                             void* scratch, size_t scratch_bytes, void* stream);
/* An FFN (reference gkgnet.py:46-72: fc1 + BN + GELU, fc2 + BN + shortcut) under bf16 autocast with gradients off as ONE launch
 * (csrc/gkg_ffn_bf16.hip): the (R, hid) hidden matrix stays on chip.  w1planes / w2planes are the gkg_linear_bf16 fragment arrays of
 * the cin -> hid and hid -> cout layers (gkg_linear_bf16_planes_bytes(cin, hid) / (hid, cout) bytes), a1 / c1 / a2 / c2 their BN
 * scale / shift vectors, act the activation ON THE HIDDEN.  Bit for bit, in every form, the outputs of the two launches
 *   gkg_linear_bf16(x, ldx, w1planes, a1, c1, NULL, 0, NULL, 0, h16, hid, R, cin, hid, act, stream)        h16 (R, hid) bf16
 *   gkg_linear_bf16(h16, hid, w2planes, a2, c2, res, ldr, out_f32, ldo32, out_bf16, ldo16, R, hid, cout, 0, stream)
 * (both contractions in the same order on v_mfma_f32_32x32x16_bf16, the hidden rounded to bf16 by the same helpers); h16 is never
 * written.  Every workgroup is independent (no counters, no flags).  Nothing outside columns [0, cout) of rows [0, R) of either
 * output is written, nothing outside [0, cin) / [0, cout) of a row of x / res or outside a1 / c1 [0, hid), a2 / c2 [0, cout) is read.
 * Envelope, otherwise GKG_ERR_UNSUPPORTED with nothing launched (the caller keeps the two launches): R >= 1, cin % 8 == hid % 8 ==
 * cout % 8 == 0, cin <= 192, cout <= 192 (any hid; cin != cout allowed), and gkg_linear_bf16's pitch multiples and 16-byte
 * alignment.  A null pointer is GKG_ERR_NULL, a pitch below its row's width GKG_ERR_SHAPE.  gkg_ffn_bf16_supported: 1 when the
 * sizes pass (pure host code; pitches and pointers are the call's to check). */
int gkg_ffn_bf16_supported(int R, int cin, int hid, int cout, int has_res, int want_f32, int want_bf16, int act);
int gkg_ffn_bf16(const void* x /* bf16 (R, ldx) */, int ldx,
                 const void* w1planes, const float* a1 /* [hid] or NULL = 1 */, const float* c1 /* [hid] */,
                 const void* w2planes, const float* a2 /* [cout] or NULL = 1 */, const float* c2 /* [cout] */,
                 const float* res /* fp32 (R, ldr) or NULL */, int ldr,
                 float* out_f32 /* (R, ldo32) or NULL */, int ldo32,
                 void* out_bf16 /* (R, ldo16) or NULL */, int ldo16,
                 int R, int cin, int hid, int cout, int act /* on the hidden: 0 none, 1 GELU */, void* stream);
/* The second half of a Grapher (reference torch_vertex.py:47-62 MRConv2d.forward + torch_nn.py:57-69 BasicConv, then
 * torch_vertex.py:325-333 fc2 + shortcut) under bf16 autocast with gradients off as ONE launch (csrc/gkg_mr_fc2_bf16.hip): gather,
 * max_k(x_j - x_i), [x, m] interleave, the grouped 1x1 projection (groups = 4) with eval-mode BN and the activation, AND the dense
 * 2C -> C projection behind it with its eval-mode BN, fp32 residual and both output precisions; the (B N, 2C) bf16 matrix between
 * the two projections stays on chip.  The arguments are gkg_mr_linear_bf16's operands — x (B, N, C) fp32, src (B, M, C) fp32 or
 * NULL (self graph, M == N), nn_idx (B*G, N, k) int64 | nn16 (B*G, N, k) u16 (M <= 65536), wplanes (gkg_mr_linear_planes_bytes(C)
 * bytes), a1 / c1 [2C], act ON THE HIDDEN — followed by gkg_linear_bf16's for the 2C -> C layer: w2planes
 * (gkg_linear_bf16_planes_bytes(2C, C) bytes), a2 [C] (NULL = 1), c2 [C], res fp32 (B N, ldr) or NULL, out_f32 / ldo32 and
 * out_bf16 / ldo16 (at least one non-NULL).  Bit for bit, in every form, the outputs of the two launches
 *   gkg_mr_linear_bf16[_nn16](x, src, idx, wplanes, a1, c1, h16, 2C, B, G, c, N, M, k, act, stream)          h16 (B N, 2C) bf16
 *   gkg_linear_bf16(h16, 2C, w2planes, a2, c2, res, ldr, out_f32, ldo32, out_bf16, ldo16, B N, 2C, C, 0, stream)
 * (one definition of the gather, the index clamp — < 0 -> 0, >= M -> M - 1 —, the maximum's tie rule, the GELU and the hidden's
 * rounding; both contractions on v_mfma_f32_32x32x16_bf16 over ascending steps of 16, no K-split; the second launch's epilogue:
 * fmaf(a2, acc, c2), + res in fp32, the bf16 output the rounding of the fp32 one); h16 is never written.  Every workgroup is
 * independent (no counters, no flags, no scratch buffer).  Nothing outside columns [0, C) of rows [0, B N) of either output is
 * written.  Envelope, otherwise GKG_ERR_UNSUPPORTED with nothing launched (the caller keeps the two launches): C = G c with
 * C % 16 == 0, c % 4 == 0, C <= 192, k <= 64, index rows that fit the LDS beside the tile (64 G k entries of 2 bytes where
 * M <= 65536, of 4 beyond; every shape of the models does), _nn16: M <= 65536, gkg_linear_bf16's pitch multiples (ldo16 % 8,
 * ldo32 % 4, ldr % 4; pitches of absent operands are ignored) and 16-byte alignment of x, src, the fragment arrays, res and the
 * outputs.  A null required pointer is GKG_ERR_NULL; non-positive sizes, a self graph with M != N and a pitch below its row's width
 * are GKG_ERR_SHAPE.  gkg_mr_fc2_bf16_supported: 1 when the sizes pass (pure host code; pitches and pointers are the call's to check). */
int gkg_mr_fc2_bf16_supported(int B, int G, int c, int N, int M, int k, int has_res, int want_f32, int want_bf16, int act);
int gkg_mr_fc2_bf16(const float* x, const float* src, const int64_t* nn_idx, const void* wplanes,
                    const float* a1 /* [2C] */, const float* c1 /* [2C] */,
                    const void* w2planes, const float* a2 /* [C] or NULL = 1 */, const float* c2 /* [C] */,
                    const float* res /* fp32 (B N, ldr) or NULL */, int ldr,
                    float* out_f32 /* (B N, ldo32) or NULL */, int ldo32,
                    void* out_bf16 /* (B N, ldo16) or NULL */, int ldo16,
                    int B, int G, int c, int N, int M, int k, int act /* on the hidden: 0 none, 1 GELU */, void* stream);
int gkg_mr_fc2_bf16_nn16(const float* x, const float* src, const uint16_t* nn16, const void* wplanes,
                         const float* a1 /* [2C] */, const float* c1 /* [2C] */,
                         const void* w2planes, const float* a2 /* [C] or NULL = 1 */, const float* c2 /* [C] */,
                         const float* res /* fp32 (B N, ldr) or NULL */, int ldr,
                         float* out_f32 /* (B N, ldo32) or NULL */, int ldo32,
                         void* out_bf16 /* (B N, ldo16) or NULL */, int ldo16,
                         int B, int G, int c, int N, int M, int k, int act /* on the hidden: 0 none, 1 GELU */, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Training under bf16 autocast (opt-in GKG_ENABLE=train_bf16): the three products of a dense 1x1 projection on bf16 operands with
 * fp32 accumulation, the operands read as the fp32 tensors training keeps and rounded (round-to-nearest-even) on their way into
 * LDS (csrc/gkg_linear_bf16.hip, csrc/gkg_linear_bf16_train.hip).  Reference layers as above, under mixed precision
 * (configs: fp16 = dict(loss_scale='dynamic')).
 *
 * gkg_linear_bf16_f32a: gkg_linear_bf16 with an fp32 A operand, x (R, ldx) fp32.  Bit for bit the result of gkg_linear_bf16 called
 * on the bf16 rounding of x, in every form (same contraction order and epilogue; the 64-column tile form at every shape, which
 * changes no bit).  cshift == NULL means zero (this entry point only).  Preconditions: gkg_linear_bf16's with ldx % 4 == 0
 * instead of ldx % 8 == 0; same error codes.  It serves
 *   the forward         Y = x W^T:            a = cshift = NULL, fp32 out (the conv bias stays in the BN passes)
 *   the input gradient  dx = dY W (+ dalias): x := dY, wplanes := the fragment array of W^T (contraction cout, output columns
 *                                             cin), res := dalias.
 * gkg_linear_bf16_f32a_supported: gkg_linear_bf16_supported's arguments and meaning for this entry point. */
int gkg_linear_bf16_f32a_supported(int R, int cin, int cout, int has_res, int want_f32, int want_bf16, int act);
int gkg_linear_bf16_f32a(const float* x /* fp32 (R, ldx) */, int ldx, const void* wplanes,
                         const float* a /* [cout] or NULL = 1 */, const float* cshift /* [cout] or NULL = 0 */,
                         const float* res /* fp32 (R, ldr) or NULL */, int ldr,
                         float* out_f32 /* (R, ldo32) or NULL */, int ldo32,
                         void* out_bf16 /* (R, ldo16) or NULL */, int ldo16,
                         int R, int cin, int cout, int act /* 0 none, 1 GELU */, void* stream);
/* The weight gradient: dw (cout, cin) += bf16(dy)^T bf16(x) over the R rows, dy (R, ldg) and x (R, ldx) fp32 in memory, exact
 * bf16 x bf16 products, fp32 accumulation on v_mfma_f32_32x32x16_bf16.  gkg_linear_wgrad_x6's accumulation contract: a workgroup
 * owns one dw tile and one slab of rows and ADDS its partial tile to dw (contiguous, row pitch cin) with fp32 atomics — the
 * caller zeroes dw, the summation order is run-dependent.  R, cin and cout need not be multiples of any tile; nothing outside
 * columns [0, cout) / [0, cin) of rows [0, R) of dy / x is read, nothing outside dw is written.  Preconditions, otherwise
 * GKG_ERR_UNSUPPORTED with nothing launched: cin % 8 == 0, cout % 8 == 0, ldg % 4 == 0, ldx % 4 == 0, ldg >= cout, ldx >= cin,
 * dy / x / dw 16-byte aligned, R <= INT_MAX - 32, a grid that fits; a size <= 0 is GKG_ERR_SHAPE, a null pointer GKG_ERR_NULL.
 * gkg_linear_wgrad_bf16_supported: 1 when the sizes pass (pure host code). */
int gkg_linear_wgrad_bf16_supported(int R, int cin, int cout);
int gkg_linear_wgrad_bf16(const float* dy /* (R, ldg) */, int ldg, const float* x /* (R, ldx) */, int ldx,
                          float* dw /* (cout, cin), += */, int R, int cin, int cout, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Training under fp16 autocast (opt-in GKG_ENABLE=train_f16; the reference's own recipe, configs/gkgnet/gkgnet_coco_576.py:146
 * fp16 = dict(loss_scale='dynamic')): the forward and the input gradient of a dense 1x1 projection on IEEE fp16 operands with
 * fp32 accumulation — the fp16 instantiation of the kernel above (csrc/gkg_linear_bf16.hip).  The weight gradient has no fp16
 * form: it stays on gkg_linear_wgrad_x6.
 *
 * gkg_linear_f16_f32a: gkg_linear_bf16_f32a's arguments and meaning (NULL a = 1, NULL cshift = 0, the same forward / input-gradient
 * uses), with
 *   x (R, ldx) fp32, each element rounded to fp16 on its way into LDS: round-to-nearest-even, overflow to +-inf, NaN stays NaN,
 *     subnormal results KEPT (under a loss scale small gradients are what must survive)
 *   wplanes_f16: fp16 weight fragments in gkg_linear_bf16's layout, [ci_pad/8][co_pad][8], fragment (f, n) = w[n][8f .. 8f+7], zero
 *     outside cin / cout; gkg_linear_f16_planes_bytes(cin, cout) bytes — the same paddings as the bf16 array, and like
 *     gkg_linear_bf16_planes_bytes the only place that encodes them
 *   acc[r][n] = sum_k f16(x[r][k]) * w[n][k]: the exact products of f16(x) and the fp16 fragments (an fp16 x fp16 product is exact
 *     in fp32; subnormal operands are not flushed), accumulated in fp32 on v_mfma_f32_32x32x16_f16 in the bf16 kernel's contraction
 *     order (ascending steps of 16, no K-split; the 64-column tile form at every shape)
 *   the a / cshift / act / res epilogue of gkg_linear_bf16, out_f32 as there, out_f16[r][n] = IEEE fp16 of the fp32 result
 *     (round-to-nearest-even; with both outputs the fp16 one is the rounding of the fp32 one).
 * Consequently the call on x and the call on the fp32 widening of x.to(fp16) give equal bits.  Preconditions, bounds and error
 * codes: gkg_linear_bf16_f32a's (cin % 8, cout % 8, ldx % 4, ldo16 % 8, ldo32 % 4, ldr % 4, 16-byte alignment).
 * gkg_linear_f16_f32a_supported: 1 when the sizes pass (pure host code; gkg_linear_bf16_f32a_supported's answer). */
size_t gkg_linear_f16_planes_bytes(int cin, int cout);
int gkg_linear_f16_f32a_supported(int R, int cin, int cout, int has_res, int want_f32, int want_f16, int act);
int gkg_linear_f16_f32a(const float* x /* fp32 (R, ldx) */, int ldx, const void* wplanes_f16,
                        const float* a /* [cout] or NULL = 1 */, const float* cshift /* [cout] or NULL = 0 */,
                        const float* res /* fp32 (R, ldr) or NULL */, int ldr,
                        float* out_f32 /* (R, ldo32) or NULL */, int ldo32,
                        void* out_f16 /* (R, ldo16) or NULL */, int ldo16,
                        int R, int cin, int cout, int act /* 0 none, 1 GELU */, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Training under 16-bit autocast, the GROUPED projection (opt-in GKG_ENABLE=train_grouped beside train_bf16 / train_f16): the forward
 * and the input gradient of BasicConv's Conv2d(2C -> 2C, 1x1, groups = 4) behind the max-relative aggregation (reference
 * torch_nn.py:57-69 behind torch_vertex.py:57-61) as ONE launch of the kernel above with a group dimension.
 *
 * gkg_linear_bf16_f32a_grouped / gkg_linear_f16_f32a_grouped: nb independent products
 *     out_q (R, cout) fp32 = kind(x_q) (R, cin) . kind(W_q)^T,   q = 0 .. nb - 1,   cin and cout PER GROUP,
 * group q's operands being x + q x_gs (row pitch ldx) and out + q out_gs (row pitch ldo), strides and pitches in floats, and the
 * q-th of nb fragment arrays that lie back to back in wplanes, each in gkg_linear_bf16's layout ([ci_pad/8][co_pad][8], fragment
 * (f, n) = W_q[n][8f .. 8f+7], zero outside cin / cout) and gkg_linear_bf16_planes_bytes(cin, cout) bytes long (fp16 elements for the
 * f16 entry point: gkg_linear_f16_planes_bytes, the same number).
 * BIT CONTRACT: group q's output is bit for bit what gkg_linear_bf16_f32a / gkg_linear_f16_f32a writes when called on group q's
 * views — x + q x_gs with ldx, wplanes + q planes_bytes, out + q out_gs with ldo, a = cshift = res = NULL, act = 0, the fp32 output
 * only — i.e. the same rounding of x on its way into LDS, the same contraction order (ascending steps of 16, no K-split, the
 * 64-column tile form) and store path.  Nothing outside rows [0, R) x columns [0, cin) of a group's x is read, nothing outside rows
 * [0, R) x columns [0, cout) of a group's out is written (pitch slack and the other groups' columns stay untouched); the CALLER
 * keeps the groups' output regions disjoint (they are written concurrently, in no order).  Workgroups are independent: no atomics,
 * no counters, run-independent bits.  The two layouts the library's own caller uses (XM (R, nb ci) the [x | m] operand buffer, Wg
 * (nb, co, ci) the grouped weight, Wp = its input columns in XM order [x chunk | m chunk]: fused._kperm_weight):
 *     product                            x                  ldx, x_gs     planes of                 out                  ldo, out_gs
 *     forward         Y_q = XM_q Wp_q^T    XM (R, nb ci)      nb ci, ci     Wp[q]   (co, ci)          Y (nb, R, co) stacked  co, R co
 *     input gradient  dXM_q = dY_q Wp_q    dY (nb, R, co)     co, R co      Wp[q]^T (ci, co)          dXM (R, nb ci) in place nb ci, ci
 * The column permutation lives in the fragment arrays, as it lives in the x6 planes (kperm): contraction columns in XM order for the
 * forward, output columns in XM order for the input gradient; no interleave and no re-layout copy exists at run time.
 * Preconditions, otherwise GKG_ERR_UNSUPPORTED with nothing launched: cin % 8 == 0, cout % 8 == 0 (each <= 2^24); ldx, ldo, x_gs,
 * out_gs multiples of 4; x, wplanes, out 16-byte aligned; 1 <= nb <= 64; nb x (row tiles x column tiles) <= 0x3fffffff.  R, cin or
 * cout <= 0, a negative group stride, ldx < cin or ldo < cout are GKG_ERR_SHAPE; a null pointer is GKG_ERR_NULL.
 * gkg_linear_bf16_f32a_grouped_supported: 1 when the sizes pass (pure host code; pitches, strides and pointers are the call's to
 * check); gkg_linear_f16_f32a_grouped_supported: the bf16 answer. */
int gkg_linear_bf16_f32a_grouped_supported(int R, int cin, int cout, int nb);
int gkg_linear_bf16_f32a_grouped(const float* x /* fp32, group q at x + q x_gs, (R, ldx) */, int ldx, long long x_gs,
                                 const void* wplanes /* nb fragment arrays back to back */,
                                 float* out /* fp32, group q at out + q out_gs, (R, ldo) */, int ldo, long long out_gs,
                                 int R, int cin, int cout, int nb, void* stream);
int gkg_linear_f16_f32a_grouped_supported(int R, int cin, int cout, int nb);
int gkg_linear_f16_f32a_grouped(const float* x /* fp32, group q at x + q x_gs, (R, ldx) */, int ldx, long long x_gs,
                                const void* wplanes /* nb fragment arrays back to back */,
                                float* out /* fp32, group q at out + q out_gs, (R, ldo) */, int ldo, long long out_gs,
                                int R, int cin, int cout, int nb, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Bandwidth kernels between the dense 1x1 projections (Conv2d 1x1 + SyncBN [+ GELU], reference
 * torch_vertex.py:290-306,334-360; torch_nn.py:57-69).  The projections themselves are plain GEMMs run by the
 * caller in the vendor library on token-major (rows = tokens) fp32 matrices.  `nb` stacks nb independent
 * (R, C) matrices (the 4 groups of the grouped projection) with parameters laid out [nb][C].
 */
/* (B,C,N) fp32 -> (B*N,C) in out_dtype (GKG_F32, or GKG_BF16 when the result only feeds a bf16 GEMM); img_scale (B) or
 * NULL multiplies image b (the backward of a stochastic-depth branch) */
int gkg_nchw_to_tm(const float* x, void* out, int B, int C, int N, int out_dtype, const float* img_scale, void* stream);
/* out(B,C,N) = (a[ch]*y[t][ch] + c[ch]) * img_scale[b] + res(B,C,N); a/c, img_scale and res optional (NULL).
 * img_scale is the reference's DropPath (torch_vertex.py:332, timm): per-image Bernoulli keep mask / keep probability. */
int gkg_tm_affine_to_nchw(const float* y, const float* a, const float* c, const float* res, float* out,
                          int B, int C, int N, const float* img_scale, void* stream);
/* Round 5: a block output handed out in BOTH layouts.  A Grapher that takes and returns NCHW (reference torch_vertex.py:325-333)
 * in front of a GrapherLabel (torch_vertex.py:392-403, which reads the feature map token-major as keys / values) used to pay a
 * layout pass in the label branch's forward and three in its backward (token-major gradient -> NCHW, + the other gradient,
 * -> token-major again).  gkg_tm_affine_to_nchw_dual: out(B,C,N) and out_tm(B*N,C) = a*y + c + res_tm, the residual given
 * token-major (the block's own token-major copy of its input).  gkg_nchw_to_tm_add: out(B*N,C) = x(B,C,N)^T + add_tm — the two
 * upstream gradients of such an output summed while the NCHW one is re-laid out. */
int gkg_tm_affine_to_nchw_dual(const float* y, const float* a, const float* c, const float* res_tm, float* out, float* out_tm,
                               int B, int C, int N, void* stream);
int gkg_nchw_to_tm_add(const float* x, const float* add_tm, float* out, int B, int C, int N, void* stream);
/* The same pass (add_tm may be NULL: gkg_nchw_to_tm's fp32 form) as the STATISTICS pass of the BN backward whose upstream
 * gradient it writes (un-grouped layer, no activation): y (B*N, C) that layer's pre-BN output, mean / invstd [C]; sums [2][C]
 * fp64, ZERO on entry, receives sum out and sum out * yhat with atomics — follow it with gkg_bn_bwd_apply_from_sums.  `out` has
 * the bits of gkg_nchw_to_tm_add / gkg_nchw_to_tm. */
int gkg_nchw_to_tm_add_bnstats(const float* x, const float* add_tm, float* out, const float* y, const float* mean,
                               const float* invstd, double* sums, int B, int C, int N, void* stream);
size_t gkg_bn_workspace_bytes(int R, int C, int nb);
/* Train-mode batch statistics of y (R,C) (conv bias NOT included in y; it is folded: it cancels in the output and
 * is added to running_mean).  Writes scale a, shift c (out = a*y + c), saved mean / invstd; updates running stats
 * (momentum, unbiased variance) when given.  Deterministic two-stage reduction. */
int gkg_bn_train_stats(const float* y, const float* gamma, const float* beta, const float* bias,
                       float* running_mean, float* running_var, float* a, float* c, float* mean, float* invstd,
                       int R, int C, int nb, float momentum, float eps, long long* num_batches_tracked /* += 1, or NULL */,
                       void* workspace, size_t workspace_bytes, void* stream);
/* Eval mode: a = gamma/sqrt(rv+eps), c = beta + a*(bias - rm) */
int gkg_bn_eval_affine(const float* gamma, const float* beta, const float* bias, const float* running_mean,
                       const float* running_var, float* a, float* c, int C, float eps, void* stream);
/* out = act(a*y + c) * row_scale[r / rows_per_scale] (+ res); act 0 = identity, 1 = GELU(erf); row_scale optional (NULL).
 * out[q] has row pitch ldo and batch stride out_bstride (both in elements of out_dtype: GKG_F32, or GKG_BF16 =
 * round-to-nearest-even of the fp32 result).  ochunk > 0: column ch is written at ch + (ch / ochunk) * ochunk — the x half of
 * an XM buffer (ldo >= 2C; see "XM layout") */
int gkg_affine_act(const float* y, const float* a, const float* c, const float* res, void* out, int R, int C,
                   int nb, int ldo, size_t out_bstride, int ochunk, int act, int out_dtype, const float* row_scale,
                   int rows_per_scale, void* stream);
/* gkg_affine_act for one batch of contiguous rows writing the result twice: fp32 (the residual stream) and its bf16
 * rounding (the next projection's operand in bf16 inference) — no stand-alone cast pass between blocks. */
int gkg_affine_act_dual(const float* y, const float* a, const float* c, const float* res, float* out_f32, void* out_bf16,
                        int R, int C, int act, const float* row_scale, int rows_per_scale, void* stream);

/* out = act(a * y + c) for a BF16 matrix y (R, C), C % 8 == 0: the output of a library convolution under bf16 autocast viewed
 * token-major (channels-last), eval-mode BN (+ conv bias) folded into a / c (reference gkgnet.py:79-118 in eval mode).  Writes
 * out_f32 (fp32: the residual stream) and / or out_bf16 (the next operand); at least one must be non-null.  act: 0 / 1 (GELU). */
int gkg_affine_act_bf16in(const void* y_bf16, const float* a, const float* c, float* out_f32, void* out_bf16, int R, int C,
                          int act, void* stream);
/* Backward of out = act(BN_train(y)): dy, dgamma, dbeta from dout (row pitch ldg, batch stride dout_bstride). */
int gkg_bn_bwd(const float* dout, const float* y, const float* a, const float* c, const float* mean,
               const float* invstd, float* dy, float* dgamma, float* dbeta, int R, int C, int nb, int ldg,
               size_t dout_bstride, int act, void* workspace, size_t workspace_bytes, void* stream);

/* Train-mode BN-apply straight from the projection kernel's fp64 column sums (gkg_linear_bn_fwd / gkg_linear_bn_fwd_x6 with
 * train == 2: statistics only): the consumer derives scale / shift itself — no finalize launch in between.  Every workgroup
 * computes the coefficients of the channels it applies (the token-major form: of its channel tile), exactly one per channel
 * also writes the saved a / c / mean / invstd [nb][C] and updates running_mean / running_var (conv `bias` folded), one
 * workgroup counts num_batches_tracked and clears `zero_buf` (`zero_doubles` doubles): the OTHER of the caller's two
 * alternating scratch buffers, i.e. what the previous projection accumulated into.
 * nchw_B == 0: token-major output like gkg_affine_act (fp32); nchw_B > 0: (nchw_B, C, R / nchw_B) channel-major output and
 * residual like gkg_tm_affine_to_nchw (nb == 1, act == 0, row_scale = one factor per image).  Same arithmetic as the
 * finalize + apply launches it replaces. */
int gkg_bn_apply_train(const float* y, const double* sums, const float* gamma, const float* beta, const float* bias,
                       float* running_mean, float* running_var, long long* num_batches_tracked, float* a, float* c,
                       float* mean, float* invstd, const float* res, float* out, int R, int C, int nb, int ldo,
                       size_t out_bstride, int ochunk /* as gkg_affine_act */, int act, int nchw_B, const float* row_scale,
                       int rows_per_scale, float momentum, float eps, double* zero_buf, size_t zero_doubles, void* stream);
/* gkg_bn_apply_train's channel-major form as gkg_tm_affine_to_nchw_dual: residual token-major, result in both layouts. */
int gkg_bn_apply_train_dual(const float* y, const double* sums, const float* gamma, const float* beta, const float* bias,
                            float* running_mean, float* running_var, long long* num_batches_tracked, float* a, float* c,
                            float* mean, float* invstd, const float* res_tm, float* out, float* out_tm, int B, int C, int N,
                            float momentum, float eps, double* zero_buf, size_t zero_doubles, void* stream);
/* gkg_bn_bwd in two launches instead of three: the statistics pass accumulates its column sums into `sums` (fp64,
 * 2 * nb * C doubles, ZERO on entry) with atomics, the apply pass reads them, writes dgamma / dbeta and clears `zero_buf`
 * (`zero_doubles` doubles; NULL / 0: nothing).  The caller alternates between two scratch buffers and passes the region the
 * previous call used as `zero_buf`, so every buffer is clean before its next use without a memset launch.  The sums are
 * run-dependent in their last fp64 bits (atomics); callers that need bit-reproducibility use gkg_bn_bwd. */
int gkg_bn_bwd_atomic(const float* dout, const float* y, const float* a, const float* c, const float* mean,
                      const float* invstd, float* dy, float* dgamma, float* dbeta, int R, int C, int nb, int ldg,
                      size_t dout_bstride, int act, double* sums, double* zero_buf, size_t zero_doubles, void* stream);


/* gkg_bn_bwd_atomic for a branch whose output was scaled per image (DropPath: torch_vertex.py:332,355,402): the incoming
 * gradient is multiplied by row_scale[row / rows_per_scale] inside both passes. */
int gkg_bn_bwd_atomic_scaled(const float* dout, const float* y, const float* a, const float* c, const float* mean,
                             const float* invstd, float* dy, float* dgamma, float* dbeta, int R, int C, int nb, int ldg,
                             size_t dout_bstride, int act, double* sums, double* zero_buf, size_t zero_doubles,
                             const float* row_scale, int rows_per_scale, void* stream);
/* Backward of out = act(a*y + c) for an EVAL-mode BN (running statistics; a, c from gkg_bn_eval_affine, y excludes the conv
 * bias): frozen-BatchNorm fine-tuning, input gradients of a model in eval().  No batch statistic stands between dout and dy,
 * so one sweep writes
 *   dy = a * dz,   dz = dout * row_scale[row / rows_per_scale] * act'(a*y + c)      (row_scale NULL: no scale; act 0 | 1 = GELU)
 * Operand forms as gkg_bn_bwd_atomic_scaled (y, dy (nb, R, C); dout with row pitch ldg and batch stride; C % 4 == 0).
 * dgamma / dbeta / dbias ([nb][C] each, any of them NULL = not wanted): the sweep also takes S0 = sum dz, S1 = sum dz*y per
 * column (fp64 from the first addition on) and a second, small launch finishes
 *   dbeta = S0,   dgamma = (S1 + (bias - running_mean) * S0) / sqrt(running_var + eps),   dbias = a * S0
 * (dbias: the gradient of the conv bias in front of the BN — not zero as in train mode).  All three NULL: ONE launch, a pure
 * elementwise pass (no atomics, no scratch; sums / workspace NULL); dy has the same bits in every form.
 * `sums` != NULL: fp64 atomics into it (2 * nb * C doubles, ZERO on entry), the finishing launch clears `zero_buf`
 * (`zero_doubles` doubles) — the alternating-pair protocol of gkg_bn_bwd_atomic; run-dependent in the last fp64 bits.
 * `sums` == NULL: bit-reproducible two-stage form through `workspace` (gkg_bn_workspace_bytes(R, C, nb)).
 * No host synchronisation (capturable). */
int gkg_bn_eval_bwd(const float* dout, const float* y, const float* a, const float* c, float* dy, int R, int C, int nb,
                    int ldg, size_t dout_bstride, int act, const float* row_scale, int rows_per_scale,
                    const float* running_mean, const float* running_var, const float* bias, float eps, float* dgamma,
                    float* dbeta, float* dbias, double* sums, double* zero_buf, size_t zero_doubles, void* workspace,
                    size_t workspace_bytes, void* stream);
/* Cross-rank batch statistics (the reference's SyncBatchNorm under DDP, torch_nn.py:37 / mmcv build_norm_layer):
 * gkg_bn_train_stats and gkg_bn_bwd split where the ranks exchange statistics.  Forward: gkg_bn_stats_sums ->
 * caller all-reduces `sums` [nb][2][C] (column sum, sum of squares) and the row count over the ranks ->
 * gkg_bn_finalize with the device scalar `count` (total rows).  Backward: gkg_bn_bwd_sums (also writes the LOCAL
 * dgamma/dbeta, like torch's batch_norm_backward_reduce, and parks dz in dy when act == 1) -> all-reduce `sums`
 * [nb][2][C] (sum dz, sum dz*yhat) -> gkg_bn_bwd_apply with the same `count`. */
int gkg_bn_stats_sums(const float* y, float* sums, int R, int C, int nb, void* workspace, size_t workspace_bytes,
                      void* stream);
int gkg_bn_finalize(const float* sums, const float* count, const float* gamma, const float* beta, const float* bias,
                    float* running_mean, float* running_var, float* a, float* c, float* mean, float* invstd, int C,
                    int nb, float momentum, float eps, long long* num_batches_tracked, void* stream);
int gkg_bn_bwd_sums(const float* dout, const float* y, const float* a, const float* c, const float* mean,
                    const float* invstd, float* dy, float* sums, float* dgamma, float* dbeta, int R, int C, int nb,
                    int ldg, size_t dout_bstride, int act, void* workspace, size_t workspace_bytes, void* stream);
int gkg_bn_bwd_apply(const float* dout, const float* y, const float* a, const float* c, const float* mean,
                     const float* invstd, const float* sums, const float* count, float* dy, int R, int C, int nb,
                     int ldg, size_t dout_bstride, int act, void* stream);
/* The same exchange for the layers whose statistics come out of the projection kernel as fp64 column sums (gkg_bn_apply_train /
 * gkg_bn_bwd_atomic): ONE fp64 all-reduce per direction, nothing rounded to fp32 before the derive.
 * Forward: the projection (train == 2) accumulates into `sums` [nb][2][C]; the caller stores its row count in a double behind
 * them and all-reduces the 2 nb C + 1 doubles; the _sync apply forms below are their local siblings with two more arguments:
 *   count      device scalar (never NULL): rows over ALL ranks.  Mean, biased variance and the unbiased factor of running_var use
 *              it where the sibling uses its host-side row count; R / B keep describing this rank's y and out.
 *   count_out  may be NULL: the first workgroup stores (float)*count there for gkg_bn_bwd_apply_sync (the scratch buffer `count`
 *              lives in is cleared by a later pass of the alternating-pair protocol).
 * Backward: gkg_bn_bwd_stats_f64 is gkg_bn_bwd_atomic[_scaled]'s statistics pass alone (sum dz, sum dz * yhat added to the
 * ZEROED `sums` with fp64 atomics; row_scale NULL: no scale; no apply pass, nothing else written); the caller keeps a copy of
 * this rank's sums, all-reduces the buffer and calls gkg_bn_bwd_apply_sync: dy from `sums_global` and `count`, dgamma / dbeta
 * from `sums_local` (like torch.nn.SyncBatchNorm and gkg_bn_bwd_sums: the data-parallel gradient exchange averages them), and
 * `zero_buf` cleared as by gkg_bn_bwd_atomic.  Both sums pointers 16-byte aligned.  Validation as the siblings': GKG_ERR_* and
 * nothing launched. */
int gkg_bn_apply_train_sync(const float* y, const double* sums, const float* gamma, const float* beta, const float* bias,
                            float* running_mean, float* running_var, long long* num_batches_tracked, float* a, float* c,
                            float* mean, float* invstd, const float* res, float* out, int R, int C, int nb, int ldo,
                            size_t out_bstride, int ochunk, int act, int nchw_B, const float* row_scale, int rows_per_scale,
                            float momentum, float eps, double* zero_buf, size_t zero_doubles, const double* count,
                            float* count_out, void* stream);
int gkg_bn_apply_train_dual_sync(const float* y, const double* sums, const float* gamma, const float* beta, const float* bias,
                                 float* running_mean, float* running_var, long long* num_batches_tracked, float* a, float* c,
                                 float* mean, float* invstd, const float* res_tm, float* out, float* out_tm, int B, int C, int N,
                                 float momentum, float eps, double* zero_buf, size_t zero_doubles, const double* count,
                                 float* count_out, void* stream);
int gkg_bn_bwd_stats_f64(const float* dout, const float* y, const float* a, const float* c, const float* mean,
                         const float* invstd, int R, int C, int nb, int ldg, size_t dout_bstride, int act, double* sums,
                         const float* row_scale, int rows_per_scale, void* stream);
int gkg_bn_bwd_apply_sync(const float* dout, const float* y, const float* a, const float* c, const float* mean,
                          const float* invstd, float* dy, float* dgamma, float* dbeta, int R, int C, int nb, int ldg,
                          size_t dout_bstride, int act, const double* sums_local, const double* sums_global, const float* count,
                          double* zero_buf, size_t zero_doubles, const float* row_scale, int rows_per_scale, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The dense 1x1 projections (reference torch_vertex.py:290-306 fc1 / fc2 = Conv2d(1x1) + BN, torch_nn.py:57-69 BasicConv =
 * Conv2d(1x1, groups=4) + BN + GELU behind the aggregation, torch_vertex.py:334-360 FFNLabel) with their input and weight
 * gradients, on the bf16 matrix cores at fp32 accuracy (csrc/gkg_gemm_x6.hip): every fp32 operand is split exactly into three
 * bf16 terms and six of the nine cross products are accumulated in fp32 (error vs fp64 measured 3-4x BELOW an fp32 fma chain
 * of the same length).  The WEIGHTS are split ahead of time into bf16 "planes", once per optimiser step and for all layers in
 * one launch; the activations are split inside the GEMM.  Token-major fp32: x (nb, R, cin), w (nb, cout, cin), y (nb, R, cout);
 * nb = 4 stacks the groups of the grouped projection.  (An fp32-MFMA forward kernel — rounds 1-5, csrc/gkg_gemm.hip — lost to
 * these at every shape and was removed in round 6.)
 *   gkg_linear_stats_doubles doubles of the fp64 column-sum scratch the statistics epilogue accumulates into
 *   gkg_x6_planes_bytes     bytes of one orientation's planes of a weight w (nb, cout, cin): dgrad = 0 forward, 1 dgrad
 *   gkg_x6_prep_desc_bytes  size of one descriptor of the batched split
 *   gkg_x6_prep_desc_fill   writes descriptor `index` into a HOST array (device pointers inside; one of the two plane
 *                           pointers may be NULL: that orientation is skipped); returns the running unit count to pass
 *                           as `unit_begin` of the next descriptor (-1: bad arguments)
 *   gkg_x6_prep_weights     ONE launch: every described weight -> its forward and dgrad planes.  `descs_dev`: the array
 *                           copied to device memory; total_units: the last gkg_x6_prep_desc_fill return value
 *   gkg_linear_bn_fwd_x6    y = x w^T with w given as `planes_fwd`; x has row pitch ldx and batch stride x_bstride (floats; a
 *                           column slice of a wider matrix is allowed).  train != 0: the train-mode BN statistics of y are
 *                           taken in the kernel's epilogue (per tile centred mean / M2 from the accumulator registers,
 *                           accumulated into fp64 column sums with atomics) and a small finalize kernel writes scale a, shift c
 *                           (out = a*y + c; the conv bias is folded: it cancels in the output and is added to running_mean),
 *                           saved mean / invstd and updates the running statistics.  `stats`: gkg_linear_stats_doubles()
 *                           doubles, zero on entry, zeroed again before the call's work completes (one buffer can serve every
 *                           layer on a stream).  train == 2: statistics only — the fp64 sums stay in `stats` for
 *                           gkg_bn_apply_train.  train == 0: plain projection.
 *   gkg_linear_dgrad_x6     dx (nb, R, cin) = dy (nb, R, cout; pitch ldg, batch stride g_bstride) w
 *   gkg_linear_wgrad_x6     dw (nb, cout, cin) += dy^T x (see below)
 * Rows must be 16-byte aligned (base pointer % 16 == 0, pitches % 4 == 0); each batch of x / dy below 4 GiB. */
int gkg_linear_stats_doubles(void);
size_t gkg_x6_planes_bytes(int cin, int cout, int nb, int dgrad);
int gkg_x6_prep_desc_bytes(void);
/* kperm != 0 (the grouped projection behind the aggregation, "XM layout"): the planes hold w's input columns as [even columns |
 * odd columns] per group — plane position p < cin/2 is column 2p (an x channel), p >= cin/2 column 2 (p - cin/2) + 1 (its m). */
long long gkg_x6_prep_desc_fill(void* host_descs, int index, const float* w, void* planes_fwd, void* planes_dgrad, int cin,
                                int cout, int nb, long long unit_begin, int kperm);
int gkg_x6_prep_weights(const void* descs_dev, int ndesc, long long total_units, void* stream);
/* The same launch also clearing up to two caller buffers (16-byte aligned, sizes multiples of 16; NULL / 0: none) — round 5: a
 * training step clears its flat gradient buffer and the fp64 BN scratch in front of the first projection anyway; riding in the
 * weight-split launch they cost no launch of their own. */
int gkg_x6_prep_weights_zero(const void* descs_dev, int ndesc, long long total_units, void* zero0, size_t zero0_bytes,
                             void* zero1, size_t zero1_bytes, void* stream);
int gkg_linear_bn_fwd_x6(const float* x, int ldx, size_t x_bstride, const void* planes_fwd, float* y, int R, int cin,
                         int cout, int nb, int train, const float* gamma, const float* beta, const float* bias,
                         float* running_mean, float* running_var, long long* num_batches_tracked, float* bn_a, float* bn_c,
                         float* bn_mean, float* bn_invstd, float momentum, float eps, double* stats, void* stream);
int gkg_linear_dgrad_x6(const float* dy, int ldg, size_t g_bstride, const void* planes_dgrad, float* dx, int R, int cin,
                        int cout, int nb, void* stream);
/* Split-K forms (round 5) for few rows under a long contraction (the label branch's 2 560-row matrices: 100 workgroups of 40
 * K-steps on 256 CUs): the same calls with a caller-owned workspace of gkg_x6_splitk_workspace_bytes() bytes (NULL: never
 * split) whose first 4 KiB (tile counters) are ZERO before the first use — every launch leaves them zero again.  The library cuts the contraction
 * into up to 8 ranges when that fills the chip (shapes it does not split run exactly as without the workspace); the last
 * workgroup to arrive at a tile adds the partial tiles in range order (run-to-run identical bits) and runs the normal
 * epilogue, BN statistics included.  gkg_linear_dgrad_x6_sk: `residual` (nb, R, cin) contiguous or NULL is added to dx in
 * the epilogue (the skip connection's gradient, reference torch_vertex.py:331,354,402). */
size_t gkg_x6_splitk_workspace_bytes(void);
/* With a workspace the _sk entry points run matrices of at most 4 096 rows on a body whose four waves split K inside the
 * workgroup (32-row x 64-column tiles, private LDS rings, B fragments straight from the weight planes, no barrier in the loop,
 * no cross-workgroup hand-off: csrc/gkg_gemm_x6.hip gemm_x6_ks_kernel) — the cross-workgroup split-K form above then only
 * serves what that body does not.  Taken for un-grouped projections of at most 640 output columns (where it measured faster:
 * a 32-row workgroup re-reads all of B).  `flags` (per call; measurement, tests): GKG_X6_NO_KS never takes it,
 * GKG_X6_FORCE_KS takes it for every short matrix. */
#define GKG_X6_NO_KS 1u
#define GKG_X6_FORCE_KS 2u
/* Round 11: a launch of the 128-row tile kernel (64-column tiles, un-split contraction; not the BN-backward statistics epilogue)
 * that needs exactly TWO rounds of resident workgroups (occupancy x CUs, queried per device) runs as one round of workgroups that
 * each WALK a static list of tiles, the next tile's first operand stages in flight under the epilogue (csrc/gkg_gemm_x6_tile.h,
 * gemm_x6_walk_kernel).  Same bits per output element.  Per call (measurement, tests): GKG_X6_NO_WALK never walks,
 * GKG_X6_FORCE_WALK walks whatever the size, and with it a non-zero cap field
 * c = (flags >> GKG_X6_WALK_CAP_SHIFT) & GKG_X6_WALK_CAP_MASK launches at most 8 c workgroups. */
#define GKG_X6_NO_WALK 4u
#define GKG_X6_FORCE_WALK 8u
#define GKG_X6_WALK_CAP_SHIFT 8
#define GKG_X6_WALK_CAP_MASK 255u
/* Workgroups of the walk launch that gkg_linear_bn_fwd_x6_sk takes for this shape, workspace (0 / 1) and flags on the current
 * device; 0: that launch does not walk (another kernel body, a split contraction, not two rounds, GKG_X6_NO_WALK); < 0: error. */
int gkg_x6_walk_workgroups(int R, int cin, int cout, int nb, int has_ws, unsigned flags);
int gkg_linear_bn_fwd_x6_sk(const float* x, int ldx, size_t x_bstride, const void* planes_fwd, float* y, int R, int cin,
                            int cout, int nb, int train, const float* gamma, const float* beta, const float* bias,
                            float* running_mean, float* running_var, long long* num_batches_tracked, float* bn_a, float* bn_c,
                            float* bn_mean, float* bn_invstd, float momentum, float eps, double* stats, void* splitk_ws,
                            size_t splitk_bytes, unsigned flags, void* stream);
/* ldx / x_bstride: row pitch and batch stride of dx in floats (ldx == 0: contiguous (nb, R, cin)); `residual` has dx's layout.
 * The grouped projection behind the aggregation writes dXM (R, 2C) directly: nb = 4, cin = C/2, ldx = 2C, x_bstride = C/2. */
int gkg_linear_dgrad_x6_sk(const float* dy, int ldg, size_t g_bstride, const void* planes_dgrad, float* dx, int R, int cin,
                           int cout, int nb, const float* residual, void* splitk_ws, size_t splitk_bytes, int ldx,
                           size_t x_bstride, unsigned flags, void* stream);
/* The un-grouped input gradient stored CHANNEL-MAJOR: dx (B, cin, N) = per image (dy w + residual)^T, R == B * N rows, residual
 * (R, cin) token-major or NULL — the bits of gkg_linear_dgrad_x6_sk + gkg_tm_affine_to_nchw in one launch.  The 128-row tile
 * kernel stores so itself when N % 4 == 0; a shape that takes another body (few rows with a split-K workspace, 80 columns,
 * N % 4 != 0) runs those two launches through dx_tm (R, cin; scratch, always required). */
int gkg_linear_dgrad_x6_nchw(const float* dy, int ldg, const void* planes_dgrad, float* dx, float* dx_tm, int R, int cin, int cout,
                             const float* residual, int B, int N, void* splitk_ws, size_t splitk_bytes, unsigned flags,
                             void* stream);
/* dw (nb, cout, cin) += dy^T x over the R rows (both operands split in registers; no LDS staging, each wave streams its own
 * rows).  dw must be ZERO on entry: slabs of rows are added with fp32 atomics (run-dependent summation order, like a
 * split-K GEMM).  x (nb, R, cin) with row pitch ldx / batch stride x_bstride (floats).  Any cin, cout >= 1. */
/* kperm != 0: x arrives with its columns as [x chunk | m chunk] per group (an XM buffer read with ldx = 2C, x_bstride = C/2):
 * operand column j is added to dw column 2j (j < cin/2) or 2 (j - cin/2) + 1 — dw keeps the reference's interleaved layout. */
int gkg_linear_wgrad_x6(const float* dy, int ldg, size_t g_bstride, const float* x, int ldx, size_t x_bstride, float* dw,
                        int R, int cin, int cout, int nb, int kperm, void* stream);
/* The weight gradients of SEVERAL layers in one launch (round 5).  Nothing downstream of a backward pass reads a dW, so the
 * host side may queue the weight gradients of every projection (reference torch_vertex.py:290-306, :334-360, torch_nn.py:57-69
 * backward) while the input gradients run and issue them together when the backward ends: at this path's sizes each of them
 * alone is a launch of 50-400 workgroups on 256 CUs.  Problem i is exactly gkg_linear_wgrad_x6(dy, ldg, g_bstride, x, ldx,
 * x_bstride, dw, R, cin, cout, nb): every dw ZERO on entry, accumulated with fp32 atomics.  At most 256 problems per call
 * (16 per launch); operands must stay valid until the launch has run.  units_per_slab: rows per workgroup in units of 128
 * (0: the library's default, 20). */
typedef struct GkgWgradProblem {
  const float* dy;
  const float* x;
  float* dw;
  size_t g_bstride, x_bstride;
  int ldg, ldx, R, cin, cout, nb;
  int kperm;
} GkgWgradProblem;
int gkg_linear_wgrad_x6_batch(const GkgWgradProblem* problems, int n, int units_per_slab, void* stream);
/* Run-independent forms of the two calls above (ABI 20): the same launches — the same tile shapes, row slabs, waves and
 * per-workgroup arithmetic, down to the LDS reduction — except that the workgroup of slab s STORES its fp32 partial tile into a
 * caller-owned workspace instead of adding it to dw with atomics, and one small launch behind them adds the partials in slab
 * order and writes dw.  No atomics, no memset node, no host synchronisation: every launch is a kernel, capturable in a hipGraph.
 *
 * Definition.  For every element of every group
 *     dw = (((0 + P_0) + P_1) + ... ) + P_{S-1}            all additions fp32, round to nearest
 * where P_s is the float32 partial the workgroup of slab s computes for that element exactly as in gkg_linear_wgrad_x6: each of
 * its four waves' acc + accs over its quarter of the slab's rows, the waves added (w0 + w1) + (w2 + w3).  Slab order: the main
 * launch's slabs (whole 128-row units, 16-byte aligned operands) in ascending row order, then the remainder launch's slabs
 * (ragged or unaligned rows) in ascending row order — what gkg_linear_wgrad_x6_det_slabs reports.  kperm is applied where the
 * element is stored.  dw is OVERWRITTEN: each of its nb * cout * cin elements is stored exactly once; it need not be zero on
 * entry and stale contents do not leak.  The result depends on the arguments only, never on the order in which workgroups run.
 *
 *   gkg_linear_wgrad_x6_det   slabs == 0: the library's slab rule (that of gkg_linear_wgrad_x6); slabs > 0 (tests,
 *                             measurements): exactly min(slabs, R / 128) balanced main slabs — with one slab over R rows the
 *                             call computes that slab's P.  `workspace`: at least gkg_linear_wgrad_x6_det_workspace_bytes()
 *                             bytes for the same sizes, 16-byte aligned, contents irrelevant on entry and undefined afterwards;
 *                             stream-ordered, so one buffer serves every call on a stream.
 *   ..._det_workspace_bytes   pure host code; an upper bound over operand alignments (slab images of nb * cout * cin floats); 0
 *                             where the call would fail on these arguments.
 *   ..._det_slabs             pure host code: the slab count S of the call with these sizes (`aligned` != 0: base pointers % 16
 *                             == 0 and batch strides % 4 == 0, which the sizes do not tell) and, for the first min(S, cap) slabs
 *                             in reduction order, first row and row count.  units_per_slab > 0: the plan of this problem
 *                             inside gkg_linear_wgrad_x6_batch_det called with that units_per_slab (`slabs` is ignored);
 *                             units_per_slab == 0: the plan of gkg_linear_wgrad_x6_det with `slabs`.  < 0: GKG_ERR_*.
 *   gkg_linear_wgrad_x6_batch_det   the problems of gkg_linear_wgrad_x6_batch (same struct, same plans, one launch per 16
 *                             problems) under the definition above, then one reduction launch per 16 problems; workspace of
 *                             gkg_linear_wgrad_x6_batch_det_workspace_bytes(problems, n, units_per_slab) bytes (pure host code,
 *                             exact for these pointers; 0 where the call would fail).
 * Errors: the argument errors of gkg_linear_wgrad_x6 / _batch; slabs outside 0 .. 4096 GKG_ERR_SHAPE; more than 2^31 elements
 * in a dw GKG_ERR_UNSUPPORTED; GKG_ERR_WORKSPACE for a workspace that is NULL, too small or not 16-byte aligned.  Every argument
 * of every problem is checked before the first launch: nothing is launched on any error. */
int gkg_linear_wgrad_x6_det(const float* dy, int ldg, size_t g_bstride, const float* x, int ldx, size_t x_bstride, float* dw,
                            int R, int cin, int cout, int nb, int kperm, int slabs, void* workspace, size_t workspace_bytes,
                            void* stream);
size_t gkg_linear_wgrad_x6_det_workspace_bytes(int R, int cin, int cout, int nb, int ldg, int ldx, int slabs);
int gkg_linear_wgrad_x6_det_slabs(int R, int cin, int cout, int nb, int ldg, int ldx, int aligned, int units_per_slab, int slabs,
                                  int* first_row, int* rows, int cap);
int gkg_linear_wgrad_x6_batch_det(const GkgWgradProblem* problems, int n, int units_per_slab, void* workspace,
                                  size_t workspace_bytes, void* stream);
size_t gkg_linear_wgrad_x6_batch_det_workspace_bytes(const GkgWgradProblem* problems, int n, int units_per_slab);

/*
 * Input gradient of a projection with the BACKWARD statistics of the layer in front of it in its epilogue (round 4).
 * dx (R, cin) = dy (R, cout; row pitch ldg) * w, weights as dgrad planes — like gkg_linear_dgrad_x6 with nb == 1 — where dx is
 * at the same time the upstream gradient g of the layer  h = act(BN_train(py))  that produced this projection's input
 * (reference: the chains fc1 -> BN -> GELU -> fc2 of FFN gkgnet.py:66-72 / FFNLabel torch_vertex.py:352-358 and
 * BasicConv -> fc2 of Grapher torch_vertex.py:329-330).  psums [pnb][2][pco] fp64 receives, with atomics, per channel
 *     sum_r dz   and   sum_r dz * yhat,     dz = g * act'(pa * py + pc),  yhat = (py - pmean) * pinvstd,
 * i.e. exactly what the statistics pass of gkg_bn_bwd_atomic would compute from g and py — which then runs as
 * gkg_bn_bwd_apply_from_sums (apply pass only).  py (pnb, R, pco) with cin == pnb * pco; column n of dx is group n / pco,
 * channel n % pco; pact 0 none / 1 GELU.
 */
int gkg_linear_dgrad_x6_bnbwd(const float* dy, int ldg, const void* planes_dgrad, float* dx, int R, int cin, int cout,
                              const float* py, const float* pa, const float* pc, const float* pmean, const float* pinvstd,
                              double* psums, int pnb, int pco, int pact, void* stream);
/* The same with gkg_linear_dgrad_x6_sk's choice of kernel body (round 9): with the split-K workspace the launch takes the
 * short-matrix body (whose epilogue then carries the statistics: one fp64 atomic pair per column and 32-row workgroup) or the
 * cross-workgroup split exactly where gkg_linear_dgrad_x6_sk does for the same shape and flags, so dx has that call's bits;
 * `residual` (R, cin) or NULL is added to dx in front of the statistics (the BN's upstream gradient is the sum).  The 128-row
 * body takes no residual here: gkg_linear_dgrad_x6_bnbwd_sk_supported() -> 1 / 0 tells beforehand, and an unsupported call
 * returns GKG_ERR_UNSUPPORTED with nothing launched. */
int gkg_linear_dgrad_x6_bnbwd_sk_supported(int R, int cin, int has_residual, int has_ws, unsigned flags);
int gkg_linear_dgrad_x6_bnbwd_sk(const float* dy, int ldg, const void* planes_dgrad, float* dx, int R, int cin, int cout,
                                 const float* residual, const float* py, const float* pa, const float* pc, const float* pmean,
                                 const float* pinvstd, double* psums, int pnb, int pco, int pact, void* splitk_ws,
                                 size_t splitk_bytes, unsigned flags, void* stream);
int gkg_bn_bwd_apply_from_sums(const float* dout, const float* y, const float* a, const float* c, const float* mean,
                               const float* invstd, float* dy, float* dgamma, float* dbeta, int R, int C, int nb, int ldg,
                               size_t dout_bstride, int act, const double* sums, double* zero_buf, size_t zero_doubles,
                               void* stream);

/* ------------------------------------------------------------------------------------------------
 * Block-level entry points (round 6; csrc/gkg_block.hip): ONE call runs the whole launch sequence of a Grapher / GrapherLabel
 * block's forward or backward (reference torch_vertex.py:325-333, :392-403 + FFNLabel :334-360) from a descriptor — the host side
 * allocates, fills the descriptor and calls.  Every launch inside is one of the entry points above, in the order and with the
 * arguments of the per-layer composition: bit-identical results.  Scope: fp32, train-mode BatchNorm with rank-local statistics
 * — or, with bn_frozen != 0, EVERY BatchNorm of the block in eval mode (running statistics) —, no DropPath scaling, un-pooled
 * keys (r == 1), C % 16 == 0, every projection on the split-bf16 kernels.
 * bn_frozen: per projection the forward is the GEMM without statistics (gkg_linear_bn_fwd_x6_sk, train == 0), gkg_bn_eval_affine
 * into the a | c slots of `bn`, and the apply (gkg_affine_act; gkg_affine_knn_prep where the train-mode form takes
 * gkg_bn_apply_knn_prep; gkg_tm_affine_to_nchw[_dual] for a Grapher's last layer); the backward is gkg_bn_eval_bwd (one launch
 * when dgamma, dbeta and dbias are all NULL, two otherwise — only then bsum / bzero are used) and the plain input-gradient
 * GEMMs.  running_mean / running_var are read, never written; nbt, momentum, fsum / fzero and the mean | invstd slots of `bn`
 * are unused; dgamma / dbeta / dbias may each be NULL (not wanted).
 * Every entry point validates the descriptor before its first launch: GKG_ERR_SHAPE for bad sizes (C % 16, the projections'
 * shapes, graph.G <= 0 or C % G != 0, keys_G likewise when keys_ws is set), GKG_ERR_NULL for a missing pointer (the saved
 * activations and projection buffers the backward reads included).  The library allocates
 * nothing and keeps no state: all buffers — including, per BN pass, the fp64 column-sum buffer to accumulate into and the region
 * of the OTHER buffer to clear (the caller's alternating pair, see gkg_bn_bwd_atomic) — come in the descriptor.
 *   GkgProjBN   one 1x1 projection + BatchNorm: weight as x6 planes (gkg_x6_prep_weights; the grouped projection behind the
 *               aggregation with kperm), BN parameters, what the forward saves for the backward (Y: pre-BN output (nb, R, cout);
 *               bn: [4][nb cout] = a, c, mean, invstd), the backward's outputs (dgamma, dbeta, with bn_frozen also dbias: the
 *               gradient of the conv bias, which is exactly zero in train mode; dw: where the weight-gradient problem it
 *               emits will add — zero on entry).
 *   GkgGraphOp  the k-NN + aggregation of the block: flags as gkg_knn_fwd (GKG_KNN_X_PREPARED: fc1's BN-apply prepares the
 *               queries — gkg_bn_apply_knn_prep; GKG_KNN_Y_PREPARED: the keys are already in knn_ws); fused_mr: one kernel
 *               (gkg_knn_mr_fused_supported), else k-NN + aggregation with u16 lists (nn16) or — a caller that returns the
 *               graph — int64 lists (nn_idx, center).  arg (B N, C) u16: the winning rows (saved for the backward).
 * Weight gradients: the backward calls FILL wq[] (3 / 5 problems, in backward order) for gkg_linear_wgrad_x6_batch; the caller
 * launches them at once or queues them with the rest of its backward pass (operands: dY buffers and saved activations must stay
 * valid until then). */
/* bwd_flags: the backward calls take the BN backward statistics of fc2 (Grapher) and fc1 inside the kernels that produce those
 * layers' upstream gradients (gkg_nchw_to_tm_add_bnstats, gkg_mr_bwd_tm_bnstats) and store a Grapher's dx from the GEMM
 * (gkg_linear_dgrad_x6_nchw); GKG_BLOCK_NO_BWD_FUSE keeps the stand-alone statistics and re-layout launches. */
#define GKG_BLOCK_NO_BWD_FUSE 1u
/* Round 9: the backward statistics of a layer whose upstream gradient an input-gradient GEMM writes — a block's grouped
 * projection (from fc2's input gradient) and a label block's FFN fc1 and fc2 (from the FFN fc2 / FFN fc1 input gradients) — are
 * taken in that GEMM's epilogue (gkg_linear_dgrad_x6_bnbwd_sk) and the layer runs its apply pass only: four launches fewer per
 * block pair.  GKG_BLOCK_NO_DGRAD_STATS keeps the stand-alone statistics launches (GKG_BLOCK_NO_BWD_FUSE implies it). */
#define GKG_BLOCK_NO_DGRAD_STATS 2u
/* Round 11: every projection launch of the call (forward calls included) with GKG_X6_NO_WALK — the one-tile form of the 128-row
 * tile kernel whatever the size. */
#define GKG_BLOCK_NO_X6_WALK 4u
typedef struct GkgProjBN {
  const void* planes_fwd; const void* planes_dgrad;
  const float* gamma; const float* beta; const float* bias;
  float* running_mean; float* running_var; long long* nbt;
  float momentum, eps;
  int cin, cout, nb;
  double* fsum; double* fzero; size_t fzero_n;      /* forward BN pass: accumulate into / clear */
  double* bsum; double* bzero; size_t bzero_n;      /* backward BN pass */
  float* Y; float* bn;
  float* dw; float* dgamma; float* dbeta;
  float* dbias;                                     /* bn_frozen only, may be NULL: the conv bias's gradient */
} GkgProjBN;
typedef struct GkgGraphOp {
  int G, k, d, fused_mr;
  const float* relpos; unsigned knn_flags, mr_flags;
  void* knn_ws; size_t knn_ws_bytes;
  uint16_t* arg; uint16_t* nn16; int64_t* nn_idx; int64_t* center;
} GkgGraphOp;
typedef struct GkgGrapherBlock {
  int B, C, H, W;
  const float* x; float* out; float* out_tm;                 /* out_tm (B N, C) or NULL: the token-major companion */
  float* xt; float* XM; float* A2;                            /* saved: (T, C), (T, 2C), (T, 2C) */
  GkgProjBN fc1, conv, fc2;
  GkgGraphOp graph;
  void* sk_ws; size_t sk_bytes;                               /* gkg_x6_splitk_workspace_bytes() */
  /* optional (with out_tm): the label graph behind this block — its keys are prepared by the last pass (gkg_bn_apply_knn_prep as_keys) */
  int keys_G, keys_L, keys_k, keys_d, keys_fused_mr; unsigned keys_flags; void* keys_ws; size_t keys_ws_bytes;
  /* backward */
  const float* dout; const float* dout_tm; float* dx;
  float* g3; float* dY3; float* dA2; float* dY2; float* dXM; float* gx1; float* dY1; float* dxt;
  unsigned bwd_flags;                                         /* GKG_BLOCK_* */
  int bn_frozen;                                              /* != 0: every BatchNorm in eval mode (see above); 0: train mode */
} GkgGrapherBlock;
typedef struct GkgLabelBlock {
  int B, C, L, M;
  const float* e; const float* ft; float* out;               /* e (B L, C), keys / values ft (B, M, C), out (B L, C) */
  float* XM; float* A2; float* h2; float* f1;                 /* saved: (T, 2C), (T, 2C), (T, C), (T, Cf) */
  GkgProjBN fc1, conv, fc2, ffn1, ffn2;
  GkgGraphOp graph;
  void* sk_ws; size_t sk_bytes;
  /* backward */
  const float* dout; float* de; float* dft;
  float* dY5; float* df1; float* dY4; float* dh2; float* dY3; float* dA2; float* dY2; float* dXM; float* gx1; float* dY1;
  unsigned bwd_flags;                                         /* GKG_BLOCK_* */
  int bn_frozen;
} GkgLabelBlock;
int gkg_grapher_fwd(const GkgGrapherBlock* b, void* stream);
int gkg_grapher_bwd(const GkgGrapherBlock* b, GkgWgradProblem* wq /* [3] */, void* stream);
int gkg_grapher_label_fwd(const GkgLabelBlock* b, void* stream);
int gkg_grapher_label_bwd(const GkgLabelBlock* b, GkgWgradProblem* wq /* [5] */, void* stream);

/*
 * The backbone's first stem convolution (reference gkgnet.py:79-81: Conv2d(3 -> C1/2, 3x3, stride 2, padding 1) on the image),
 * as a direct kernel — with 3 input channels the library's implicit-GEMM forms run at a few TFLOP/s — writing the
 * channels-last tensor the next convolution and the blocks' token-major kernels want; optionally the eval-mode BN (a, c:
 * gkg_bn_eval_affine, conv bias folded) and GELU behind it (gkgnet.py:81-83) in the epilogue.
 *   out (B, Ho, Wo, cout) = act(a * (conv(x) + bias) + c);  x (B, cin, H, W) fp32, w (cout, cin, 3, 3) fp32;
 *   a, c both NULL: the plain convolution (+ bias);  Ho = (H + 1) / 2, Wo = (W + 1) / 2;  out_dtype GKG_F32 / GKG_BF16.
 */
int gkg_stem_conv3x3s2_supported(int cin, int cout);
int gkg_stem_conv3x3s2_fwd(const float* x, const float* w, const float* bias, const float* a, const float* c, void* out, int B,
                           int cin, int H, int W, int cout, int act, int out_dtype, void* stream);

/*
 * Opt-in kernel timing (measurement only; off by default, nothing is recorded on the hot path when off).
 * When enabled, every kernel launch made by this library is bracketed by hipEventRecord on the SAME
 * stream it is launched on.  gkg_prof_read synchronises on the recorded events (so call it outside any
 * timed / captured region) and accumulates per kernel id.
 */
#define GKG_PROF_TOKEN_PREP 0
#define GKG_PROF_KNN_TILE 1
#define GKG_PROF_KNN_MERGE 2
#define GKG_PROF_MR_FWD 3
#define GKG_PROF_MR_BWD 4
#define GKG_PROF_GEMM_X6 5  /* gemm_x6_kernel (forward and dgrad launches) */
#define GKG_PROF_NUM 6
void gkg_prof_enable(int on);
void gkg_prof_reset(void);
/* total milliseconds and number of launches recorded for `kernel_id` since the last reset; 0 on success. */
int gkg_prof_read(int kernel_id, double* total_ms, long* launches);
/* Algorithmic work of the launches counted by gkg_prof_read since the last reset, for the kernels that report it:
 * GKG_PROF_GEMM_X6: flop, 2 R cin cout nb per launch; GKG_PROF_KNN_TILE: flop of the distance contraction, 2 BG c N M per
 * gkg_knn_fwd[_tm] call (SURVEY §8d flops_knn); GKG_PROF_MR_FWD / _BWD (token-major entry points): BYTES per SURVEY §8d —
 * fwd: x + keys (bipartite) + int64 indices + m + 1 B/element of argmax when saved; bwd: g + indices + argmax + gx + gsrc;
 * 0 otherwise. */
double gkg_prof_work(int kernel_id);

#ifdef __cplusplus
}
#endif
#endif /* GKG_HIP_H_ */
