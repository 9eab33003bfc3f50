// gkg_block.hip — block-level entry points (round 6, VERDICT r5 item 5 "a thin host"): ONE call runs the whole launch sequence of
// a Grapher / GrapherLabel block's forward or backward (reference torch_vertex.py:325-333 / :392-403 with FFNLabel :334-360) from a
// descriptor of pointers and sizes.  Nothing new is computed here: every launch is one of the library's own entry points
// (include/gkg_hip.h), called in the order and with the arguments the Python composition (gkgnet_amd/fused.py) uses for the same
// block — so the results are bit-identical to that composition (tests/test_hip_block_driver.py) — and the host side shrinks to
// "allocate, fill a descriptor, call".  Scope: the fp32 training form (train-mode BatchNorm with rank-local statistics, no
// DropPath scaling, un-pooled keys r == 1, every projection on the split-bf16 kernels) and its all-frozen form (bn_frozen: every
// BatchNorm of the block in eval mode — running statistics, nothing but gradients written back); everything else keeps the
// composition.
// The library still allocates nothing and keeps no state: the descriptor carries every buffer, including the fp64 column-sum
// scratch pair the caller alternates between BN passes.
//
// Structure: each entry point is ONE sequence of layer steps.  A step (the helpers below) picks the train or the frozen call itself
// from the Ctx it is handed, so the two modes cannot drift apart, and the part both blocks have — fc1 .. fc2's GEMM in the forward,
// the grouped projection .. fc1's BN backward in the backward — is written once (core_fwd / core_bwd, over the field names the two
// descriptors share).  The frozen backward is the train one with every "statistics ride in another kernel" question answered no.
// Because this file only calls other extern "C" entry points, its whole behaviour is a call trace:
// tests/test_block_driver_call_trace_host.py records it on the host over the cross product of the branches below.
#include "gkg_common.h"

using namespace gkg;

namespace {

#define GKG_TRY(call)              \
  do {                             \
    const int rc_ = (call);        \
    if (rc_ != 0) return rc_;      \
  } while (0)

// what every step of one block call shares: the BatchNorm mode, the split-K workspace, the stream
struct Ctx {
  bool frozen;
  void* sk_ws; size_t sk_bytes;
  void* st;
  unsigned x6_flags;                 // GKG_X6_* of every projection launch of the call
};
// the projections' per-call flags from a block's bwd_flags
unsigned x6_flags_of(unsigned bwd_flags) { return (bwd_flags & GKG_BLOCK_NO_X6_WALK) ? GKG_X6_NO_WALK : 0u; }

// ---- the layer steps ---------------------------------------------------------------------------------------------------------------
// GEMM step, y = x W^T.  Train: with the BN statistics into p.fsum.  Frozen: without, then (a, c) folded from the running
// statistics and the conv bias into p.bn's a | c slots.
int proj_gemm(const Ctx& c, const GkgProjBN& p, const float* x, int ldx, size_t x_bstride, int R) {
  GKG_TRY(gkg_linear_bn_fwd_x6_sk(x, ldx, x_bstride, p.planes_fwd, p.Y, R, p.cin, p.cout, p.nb, c.frozen ? 0 : 2, nullptr, nullptr, nullptr,
                                  nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, 0.f, c.frozen ? nullptr : p.fsum,
                                  c.sk_ws, c.sk_bytes, c.x6_flags, c.st));
  if (!c.frozen) return 0;
  const int n = p.nb * p.cout;
  return gkg_bn_eval_affine(p.gamma, p.beta, p.bias, p.running_mean, p.running_var, p.bn, p.bn + n, n, p.eps, c.st);
}
// Apply step, out = act(BN(y)) (+ res)
int proj_apply(const Ctx& c, const GkgProjBN& p, int R, const float* res, float* out, int ldo, size_t obs, int ochunk, int act, int nchw_B) {
  const int n = p.nb * p.cout;
  if (c.frozen) return gkg_affine_act(p.Y, p.bn, p.bn + n, res, out, R, p.cout, p.nb, ldo, obs, ochunk, act, GKG_F32, nullptr, 0, c.st);
  return gkg_bn_apply_train(p.Y, p.fsum, p.gamma, p.beta, p.bias, p.running_mean, p.running_var, p.nbt, p.bn, p.bn + n, p.bn + 2 * n,
                            p.bn + 3 * n, res, out, R, p.cout, p.nb, ldo, obs, ochunk, act, nchw_B, nullptr, 0, p.momentum, p.eps,
                            p.fzero, p.fzero_n, c.st);
}
// The apply step of an un-grouped layer as the token preparation of a k-NN problem (B, G, N queries, M keys, k, d; its flags and
// workspace): the queries form — out = the x half of the operand buffer — or (as_keys) the keys form — out + res token-major and
// channel-major (out_nchw).  The only place that spells these two argument lists.
int proj_apply_prep(const Ctx& c, const GkgProjBN& p, float* out, int ldo, int ochunk, int B, int G, int N, int M, int k, int d, int has_y,
                    int has_relpos, unsigned flags, int fused_mr, int as_keys, const float* res, float* out_nchw, void* ws, size_t ws_bytes) {
  const int n = p.cout;
  if (c.frozen)
    return gkg_affine_knn_prep(p.Y, p.bn, p.bn + n, out, ldo, ochunk, B, G, n / G, N, M, k, d, has_y, has_relpos, flags, fused_mr, as_keys, res,
                               out_nchw, ws, ws_bytes, c.st);
  return gkg_bn_apply_knn_prep(p.Y, p.fsum, p.gamma, p.beta, p.bias, p.running_mean, p.running_var, p.nbt, p.bn, p.bn + n, p.bn + 2 * n,
                               p.bn + 3 * n, out, ldo, ochunk, B, G, n / G, N, M, k, d, has_y, has_relpos, flags, fused_mr, as_keys, res, out_nchw,
                               ws, ws_bytes, p.momentum, p.eps, p.fzero, p.fzero_n, c.st);
}
// BN-backward step, dY of out = act(BN(Y)) for the upstream gradient g (row pitch ldg, batch stride gbs).  `have`: the statistics
// are already in p.bsum, left there by the kernel that produced g — the apply pass only.  Else train: statistics + apply; frozen:
// one sweep, and with a parameter gradient wanted two column sums into p.bsum and a small launch that finishes dgamma / dbeta /
// dbias (and clears p.bzero).
int proj_bn_bwd(const Ctx& c, const GkgProjBN& p, bool have, const float* g, int ldg, size_t gbs, int R, int act, float* dY) {
  const int n = p.nb * p.cout;
  if (have)
    return gkg_bn_bwd_apply_from_sums(g, p.Y, p.bn, p.bn + n, p.bn + 2 * n, p.bn + 3 * n, dY, p.dgamma, p.dbeta, R, p.cout, p.nb, ldg, gbs,
                                      act, p.bsum, p.bzero, p.bzero_n, c.st);
  if (!c.frozen)
    return gkg_bn_bwd_atomic(g, p.Y, p.bn, p.bn + n, p.bn + 2 * n, p.bn + 3 * n, dY, p.dgamma, p.dbeta, R, p.cout, p.nb, ldg, gbs, act,
                             p.bsum, p.bzero, p.bzero_n, c.st);
  const bool want = p.dgamma || p.dbeta || p.dbias;
  return gkg_bn_eval_bwd(g, p.Y, p.bn, p.bn + n, dY, R, p.cout, p.nb, ldg, gbs, act, nullptr, 0, p.running_mean, p.running_var, p.bias,
                         p.eps, p.dgamma, p.dbeta, p.dbias, want ? p.bsum : nullptr, want ? p.bzero : nullptr, want ? p.bzero_n : 0,
                         nullptr, 0, c.st);
}
// Input-gradient step, dx = dY W (+ residual; dx with row pitch ldx / batch stride x_bstride, 0: plain).  q: the layer IN FRONT
// (q's output, qact(BN(q.Y)), is this projection's input, so dx is q's upstream gradient) whose backward statistics the GEMM's
// epilogue takes into q->bsum; nullptr: none.
int proj_dgrad(const Ctx& c, const GkgProjBN& p, const GkgProjBN* q, int qact, const float* dY, int R, const float* residual, float* dx,
               int ldx, size_t x_bstride) {
  if (!q)
    return gkg_linear_dgrad_x6_sk(dY, p.cout, (size_t)R * p.cout, p.planes_dgrad, dx, R, p.cin, p.cout, p.nb, residual, c.sk_ws, c.sk_bytes,
                                  ldx, x_bstride, c.x6_flags, c.st);
  const int n = q->nb * q->cout;
  return gkg_linear_dgrad_x6_bnbwd_sk(dY, p.cout, p.planes_dgrad, dx, R, p.cin, p.cout, residual, q->Y, q->bn, q->bn + n, q->bn + 2 * n,
                                      q->bn + 3 * n, q->bsum, q->nb, q->cout, qact, c.sk_ws, c.sk_bytes, c.x6_flags, c.st);
}
// whether p's input-gradient GEMM can take the statistics of the layer in front (never in a frozen block: there are none)
bool dgrad_stats_ok(const Ctx& c, const GkgProjBN& p, unsigned bwd_flags, int R, bool residual) {
  return !c.frozen && !(bwd_flags & (GKG_BLOCK_NO_BWD_FUSE | GKG_BLOCK_NO_DGRAD_STATS)) && p.nb == 1 &&
         gkg_linear_dgrad_x6_bnbwd_sk_supported(R, p.cin, residual ? 1 : 0, c.sk_ws ? 1 : 0, c.x6_flags);
}
// A layer's backward: the BN-backward step (`have`: its statistics came with g), then the input-gradient step (`give`: with the
// statistics of the layer q in front)
int proj_bwd(const Ctx& c, const GkgProjBN& p, bool have, const GkgProjBN* q, bool give, int qact, const float* g, int ldg, size_t gbs,
             int R, int act, float* dY, const float* residual, float* dx, int ldx, size_t x_bstride) {
  GKG_TRY(proj_bn_bwd(c, p, have, g, ldg, gbs, R, act, dY));
  return proj_dgrad(c, p, give ? q : nullptr, qact, dY, R, residual, dx, ldx, x_bstride);
}
// The aggregation's backward (scatter) and fc1's BN backward.  `fuse`: fc1's statistics are taken inside the scatter and only the
// apply pass follows; a shape whose scatter form carries none answers GKG_ERR_UNSUPPORTED with nothing launched, and takes the
// plain pair like fuse off.
int mr_bwd_bn(const Ctx& c, const GkgProjBN& p, const GkgGraphOp& g, bool fuse, const float* dXM, float* gx1, float* gsrc, int B, int C,
              int N, int M, float* dY) {
  const uint8_t* arg = reinterpret_cast<const uint8_t*>(g.arg);
  const int T = B * N;
  bool have = false;
  if (fuse) {
    const int rc = gkg_mr_bwd_tm_bnstats(dXM, nullptr, arg, gx1, gsrc, B, g.G, C / g.G, N, M, g.k, 1, 1, g.mr_flags, p.Y, p.bn + 2 * p.cout,
                                         p.bn + 3 * p.cout, p.bsum, c.st);
    if (rc != 0 && rc != GKG_ERR_UNSUPPORTED) return rc;
    have = rc == 0;
  }
  if (!have) GKG_TRY(gkg_mr_bwd_tm(dXM, nullptr, arg, gx1, gsrc, B, g.G, C / g.G, N, M, g.k, 1, 1, g.mr_flags, c.st));
  return proj_bn_bwd(c, p, have, gx1, p.cout, 0, T, 0, dY);
}

void wgrad_entry(GkgWgradProblem& q, const GkgProjBN& p, const float* dY, const float* x, int ldx, size_t x_bstride, int R, int kperm) {
  q.dy = dY; q.x = x; q.dw = p.dw;
  q.g_bstride = (size_t)R * p.cout; q.x_bstride = x_bstride;
  q.ldg = p.cout; q.ldx = ldx; q.R = R; q.cin = p.cin; q.cout = p.cout; q.nb = p.nb; q.kperm = kperm;
}

// graph + aggregation of x (the x half of XM) over keys y (NULL: self graph): one fused launch or k-NN (u16 lists) + aggregation
int graph_fwd(const GkgGraphOp& g, float* XM, const float* y, int B, int C, int N, int M, void* st) {
  const int c = C / g.G;
  if (g.fused_mr)
    return gkg_knn_mr_fwd_tm(XM, 2 * C, C / 4, y, g.relpos, XM, g.arg, nullptr, g.nn_idx, g.center, B, g.G, c, N, M, g.k, g.d, g.knn_flags,
                             g.knn_ws, g.knn_ws_bytes, st);
  if (g.nn_idx) {                                  // the caller returns the graph (GrapherLabel): int64 lists
    GKG_TRY(gkg_knn_fwd_tm(XM, 2 * C, C / 4, y, g.relpos, g.nn_idx, g.center, B, g.G, c, N, M, g.k, g.d, GKG_F32, g.knn_flags, g.knn_ws,
                           g.knn_ws_bytes, st));
    return gkg_mr_fwd_tm(XM, 2 * C, C / 4, y, g.nn_idx, XM, reinterpret_cast<uint8_t*>(g.arg), B, g.G, c, N, M, g.k, 1, GKG_F32, 1, st);
  }
  GKG_TRY(gkg_knn_fwd_tm16(XM, 2 * C, C / 4, y, g.relpos, g.nn16, B, g.G, c, N, M, g.k, g.d, GKG_F32, g.knn_flags, g.knn_ws,
                           g.knn_ws_bytes, st));
  return gkg_mr_fwd_tm16(XM, 2 * C, C / 4, y, g.nn16, XM, reinterpret_cast<uint8_t*>(g.arg), B, g.G, c, N, M, g.k, 1, GKG_F32, 1, st);
}

// ---- the core both blocks share (Blk: GkgGrapherBlock / GkgLabelBlock — fc1, conv, fc2, graph, XM, A2 and the backward's
// temporaries carry the same names in both) ------------------------------------------------------------------------------------------
// Forward: fc1 GEMM on x (T, C) -> fc1's apply into the x half of the operand buffer, the same pass preparing the k-NN's queries
// when the graph op asks for it -> graph + aggregation over keys y (NULL: self graph) -> BasicConv on the operand buffer -> fc2 GEMM
template <class Blk>
int core_fwd(const Ctx& c, const Blk* b, const float* x, const float* y, int N, int M, int has_relpos) {
  const int B = b->B, C = b->C, T = B * N;
  const GkgGraphOp& g = b->graph;
  GKG_TRY(proj_gemm(c, b->fc1, x, C, (size_t)T * C, T));
  if (g.knn_flags & GKG_KNN_X_PREPARED)
    GKG_TRY(proj_apply_prep(c, b->fc1, b->XM, 2 * C, C / 4, B, g.G, N, M, g.k, g.d, y ? 1 : 0, has_relpos,
                            g.knn_flags & ~(GKG_KNN_X_PREPARED | GKG_KNN_Y_PREPARED), g.fused_mr, 0, nullptr, nullptr, g.knn_ws,
                            g.knn_ws_bytes));
  else
    GKG_TRY(proj_apply(c, b->fc1, T, nullptr, b->XM, 2 * C, 0, C / 4, 0, 0));
  GKG_TRY(graph_fwd(g, b->XM, y, B, C, N, M, c.st));
  GKG_TRY(proj_gemm(c, b->conv, b->XM, 2 * C, (size_t)(C / 2), T));
  GKG_TRY(proj_apply(c, b->conv, T, nullptr, b->A2, 2 * C, (size_t)(C / 2), 0, 1, 0));
  return proj_gemm(c, b->fc2, b->A2, 2 * C, (size_t)T * 2 * C, T);
}
// Backward, from dA2 (fc2's input gradient; `conv_stats`: that GEMM took the grouped projection's statistics): the grouped
// projection -> wq[0]; the scatter (gsrc: the keys' / values' gradient, NULL for a self graph) with fc1's BN backward -> wq[1],
// x (T, C) being fc1's input.  fc1's input gradient is the caller's.
template <class Blk>
int core_bwd(const Ctx& c, const Blk* b, GkgWgradProblem* wq, bool conv_stats, const float* x, float* gsrc, int N, int M) {
  const int B = b->B, C = b->C, T = B * N;
  GKG_TRY(proj_bwd(c, b->conv, conv_stats, nullptr, false, 0, b->dA2, 2 * C, (size_t)(C / 2), T, 1, b->dY2, nullptr, b->dXM, 2 * C,
                   (size_t)(C / 2)));
  wgrad_entry(wq[0], b->conv, b->dY2, b->XM, 2 * C, (size_t)(C / 2), T, 1);
  const bool fuse = !c.frozen && !(b->bwd_flags & GKG_BLOCK_NO_BWD_FUSE);
  GKG_TRY(mr_bwd_bn(c, b->fc1, b->graph, fuse, b->dXM, b->gx1, gsrc, B, C, N, M, b->dY1));
  wgrad_entry(wq[1], b->fc1, b->dY1, x, C, (size_t)T * C, T, 0);
  return 0;
}

// ---- descriptor validation, shared by the four entry points (before any launch) ---------------------------------------------------
int check_proj(const GkgProjBN& p, bool frozen, bool bwd, const char* who) {
  if (!p.planes_fwd || !p.planes_dgrad || !p.gamma || !p.beta || !p.Y || !p.bn) return gkg_fail(GKG_ERR_NULL, who);
  if (frozen ? (!p.running_mean || !p.running_var) : (!p.fsum || (bwd && !p.bsum))) return gkg_fail(GKG_ERR_NULL, who);
  if (bwd) {
    if (!p.dw) return gkg_fail(GKG_ERR_NULL, who);
    if (!frozen && (!p.dgamma || !p.dbeta)) return gkg_fail(GKG_ERR_NULL, who);
    if (frozen && (p.dgamma || p.dbeta || p.dbias) && !p.bsum) return gkg_fail(GKG_ERR_NULL, who);
    if (p.dbias && (!frozen || !p.bias)) return gkg_fail(GKG_ERR_SHAPE, who);
  }
  return 0;
}
// the sizes of the core — batch, C, the three projections (`own_bad`: the block's own sizes are not right) — then the graph op
template <class Blk>
int check_core_shapes(const Blk* b, bool own_bad, const char* who_null, const char* who_shape) {
  const int C = b->C;
  if (own_bad || b->B <= 0 || C <= 0 || (C & 15) || b->fc1.nb != 1 || b->conv.nb != 4 || b->fc2.nb != 1 || b->fc1.cin != C || b->fc1.cout != C ||
      b->conv.cin != C / 2 || b->conv.cout != C / 2 || b->fc2.cin != 2 * C || b->fc2.cout != C)
    return gkg_fail(GKG_ERR_SHAPE, who_shape);
  const GkgGraphOp& g = b->graph;
  if (g.G <= 0 || C % g.G || g.k <= 0 || g.d <= 0) return gkg_fail(GKG_ERR_SHAPE, who_shape);
  if (!g.arg || !g.knn_ws) return gkg_fail(GKG_ERR_NULL, who_null);
  return 0;
}
// what the forward writes and the backward reads: the saved activations (`own_missing`: one of the block's own is not there), then
// the core's projections
template <class Blk>
int check_core_ptrs(const Blk* b, bool own_missing, bool bwd, const char* who) {
  if (own_missing || !b->XM || !b->A2) return gkg_fail(GKG_ERR_NULL, who);
  const bool frozen = b->bn_frozen != 0;
  GKG_TRY(check_proj(b->fc1, frozen, bwd, who));
  GKG_TRY(check_proj(b->conv, frozen, bwd, who));
  return check_proj(b->fc2, frozen, bwd, who);
}
int check_grapher(const GkgGrapherBlock* b, const GkgWgradProblem* wq, bool bwd) {
  const char* nul = bwd ? "gkg_grapher_bwd: null pointer" : "gkg_grapher_fwd: null pointer";
  const char* shp = bwd ? "gkg_grapher_bwd: C % 16 == 0, G > 0, C % G == 0; fc1 C -> C, conv 4 x (C/2 -> C/2), fc2 2C -> C"
                        : "gkg_grapher_fwd: C % 16 == 0, G > 0, C % G == 0; fc1 C -> C, conv 4 x (C/2 -> C/2), fc2 2C -> C";
  if (!b || (bwd && !wq)) return gkg_fail(GKG_ERR_NULL, nul);
  GKG_TRY(check_core_shapes(b, b->H <= 0 || b->W <= 0, nul, shp));
  if (b->keys_ws && (b->keys_G <= 0 || b->C % b->keys_G)) return gkg_fail(GKG_ERR_SHAPE, shp);
  GKG_TRY(check_core_ptrs(b, !b->x || !b->xt, bwd, nul));
  if (!bwd) return b->out ? 0 : gkg_fail(GKG_ERR_NULL, nul);
  if (!b->dout || !b->dx || !b->g3 || !b->dY3 || !b->dA2 || !b->dY2 || !b->dXM || !b->gx1 || !b->dY1 || !b->dxt) return gkg_fail(GKG_ERR_NULL, nul);
  return 0;
}
int check_label(const GkgLabelBlock* b, const GkgWgradProblem* wq, bool bwd) {
  const char* nul = bwd ? "gkg_grapher_label_bwd: null pointer" : "gkg_grapher_label_fwd: null pointer";
  const char* shp = bwd ? "gkg_grapher_label_bwd: bad projection shapes (C % 16 == 0, G > 0, C % G == 0)"
                        : "gkg_grapher_label_fwd: bad projection shapes (C % 16 == 0, G > 0, C % G == 0)";
  if (!b || (bwd && !wq)) return gkg_fail(GKG_ERR_NULL, nul);
  GKG_TRY(check_core_shapes(b, b->L <= 0 || b->M <= 0 || b->ffn1.nb != 1 || b->ffn2.nb != 1 || b->ffn1.cin != b->C || b->ffn1.cout <= 0 ||
                                   b->ffn2.cout != b->C || b->ffn2.cin != b->ffn1.cout,
                            nul, shp));
  GKG_TRY(check_core_ptrs(b, !b->e || !b->ft || !b->h2 || !b->f1, bwd, nul));
  const bool frozen = b->bn_frozen != 0;
  GKG_TRY(check_proj(b->ffn1, frozen, bwd, nul));
  GKG_TRY(check_proj(b->ffn2, frozen, bwd, nul));
  if (!bwd) return b->out ? 0 : gkg_fail(GKG_ERR_NULL, nul);
  if (!b->dout || !b->de || !b->dft || !b->dY5 || !b->df1 || !b->dY4 || !b->dh2 || !b->dY3 || !b->dA2 || !b->dY2 || !b->dXM || !b->gx1 || !b->dY1)
    return gkg_fail(GKG_ERR_NULL, nul);
  return 0;
}

}  // namespace

// ---- Grapher (reference torch_vertex.py:325-333): x (B, C, H, W) -> out (B, C, H, W) [+ out_tm (B N, C)] ----------------------
extern "C" int gkg_grapher_fwd(const GkgGrapherBlock* b, void* st) {
  GKG_TRY(check_grapher(b, nullptr, false));
  const Ctx c{b->bn_frozen != 0, b->sk_ws, b->sk_bytes, st, x6_flags_of(b->bwd_flags)};
  const int B = b->B, C = b->C, N = b->H * b->W, T = B * N;
  // block entry: NCHW -> token-major; then the core on the self graph
  GKG_TRY(gkg_nchw_to_tm(b->x, b->xt, B, C, N, GKG_F32, nullptr, st));
  GKG_TRY(core_fwd(c, b, b->xt, nullptr, N, N, b->graph.relpos ? 1 : 0));
  // fc2's BN + residual -> NCHW: with the token-major companion and the keys of the label graph behind, with the companion, plain
  const GkgProjBN& p = b->fc2;
  if (b->out_tm && b->keys_ws)
    return proj_apply_prep(c, p, b->out_tm, 0, 0, B, b->keys_G, b->keys_L, N, b->keys_k, b->keys_d, 1, 0, b->keys_flags, b->keys_fused_mr, 1,
                           b->xt, b->out, b->keys_ws, b->keys_ws_bytes);
  if (b->out_tm)
    return c.frozen ? gkg_tm_affine_to_nchw_dual(p.Y, p.bn, p.bn + C, b->xt, b->out, b->out_tm, B, C, N, st)
                    : gkg_bn_apply_train_dual(p.Y, p.fsum, p.gamma, p.beta, p.bias, p.running_mean, p.running_var, p.nbt, p.bn, p.bn + C,
                                              p.bn + 2 * C, p.bn + 3 * C, b->xt, b->out, b->out_tm, B, C, N, p.momentum, p.eps, p.fzero,
                                              p.fzero_n, st);
  return c.frozen ? gkg_tm_affine_to_nchw(p.Y, p.bn, p.bn + C, b->x, b->out, B, C, N, nullptr, st)
                  : proj_apply(c, p, T, b->x, b->out, C, 0, 0, 0, B);
}

// Backward of the above: dout (B, C, H, W) [+ dout_tm (B N, C): the gradient of the token-major companion] -> dx (B, C, H, W), the
// BN parameter gradients, and the three weight-gradient PROBLEMS in wq[0..2] (for gkg_linear_wgrad_x6_batch: the caller launches
// them now or queues them with the rest of the backward pass).  Temporaries: g3, dY3 (T, C), dA2 (T, 2C), dY2 (4, T, C/2),
// dXM (T, 2C), gx1, dY1, dxt (T, C) — caller-owned; dY3 / dY2 / dY1 must stay valid until the weight gradients have run.
extern "C" int gkg_grapher_bwd(const GkgGrapherBlock* b, GkgWgradProblem* wq, void* st) {
  GKG_TRY(check_grapher(b, wq, true));
  const Ctx c{b->bn_frozen != 0, b->sk_ws, b->sk_bytes, st, x6_flags_of(b->bwd_flags)};
  const int B = b->B, C = b->C, N = b->H * b->W, T = B * N;
  // the output's gradient(s) token-major (g3); it is also the residual branch's gradient
  // (round 8, unless GKG_BLOCK_NO_BWD_FUSE or frozen: the re-layout pass takes fc2's BN backward statistics, the scatter takes fc1's
  // — three launches fewer; round 9, unless GKG_BLOCK_NO_DGRAD_STATS or frozen: fc2's input-gradient GEMM takes the grouped
  // projection's — one launch fewer)
  const bool nchw_dgrad = !(b->bwd_flags & GKG_BLOCK_NO_BWD_FUSE), fuse = nchw_dgrad && !c.frozen;
  const bool conv_stats = dgrad_stats_ok(c, b->fc2, b->bwd_flags, T, false);
  if (fuse) GKG_TRY(gkg_nchw_to_tm_add_bnstats(b->dout, b->dout_tm, b->g3, b->fc2.Y, b->fc2.bn + 2 * C, b->fc2.bn + 3 * C, b->fc2.bsum, B, C, N, st));
  else if (b->dout_tm) GKG_TRY(gkg_nchw_to_tm_add(b->dout, b->dout_tm, b->g3, B, C, N, st));
  else GKG_TRY(gkg_nchw_to_tm(b->dout, b->g3, B, C, N, GKG_F32, nullptr, st));
  GKG_TRY(proj_bwd(c, b->fc2, fuse, &b->conv, conv_stats, 1, b->g3, C, 0, T, 0, b->dY3, nullptr, b->dA2, 0, 0));
  wgrad_entry(wq[0], b->fc2, b->dY3, b->A2, 2 * C, (size_t)T * 2 * C, T, 0);
  GKG_TRY(core_bwd(c, b, wq + 1, conv_stats, b->xt, nullptr, N, N));
  // fc1's input gradient + the residual branch's (g3), channel-major: stored that way by the GEMM (round 8, in both modes), or
  // token-major and re-laid out
  if (nchw_dgrad)
    return gkg_linear_dgrad_x6_nchw(b->dY1, C, b->fc1.planes_dgrad, b->dx, b->dxt, T, C, C, b->g3, B, N, b->sk_ws, b->sk_bytes, c.x6_flags, st);
  GKG_TRY(proj_dgrad(c, b->fc1, nullptr, 0, b->dY1, T, b->g3, b->dxt, 0, 0));
  return gkg_tm_affine_to_nchw(b->dxt, nullptr, nullptr, nullptr, b->dx, B, C, N, nullptr, st);
}

// ---- GrapherLabel (reference torch_vertex.py:392-403 + FFNLabel :334-360): e (B L, C), keys / values ft (B, M, C) -> E' (B L, C) -----
extern "C" int gkg_grapher_label_fwd(const GkgLabelBlock* b, void* st) {
  GKG_TRY(check_label(b, nullptr, false));
  const Ctx c{b->bn_frozen != 0, b->sk_ws, b->sk_bytes, st, x6_flags_of(b->bwd_flags)};
  const int C = b->C, T = b->B * b->L, Cf = b->ffn1.cout;
  // the core on the graph from the labels to the image tokens (the train form has always announced "no positional bias" to the
  // query preparation, the frozen form what the graph op carries; a label graph has none)
  GKG_TRY(core_fwd(c, b, b->e, b->ft, b->L, b->M, c.frozen && b->graph.relpos ? 1 : 0));
  // fc2's BN + the block residual, then the FFN with its own
  GKG_TRY(proj_apply(c, b->fc2, T, b->e, b->h2, C, 0, 0, 0, 0));
  GKG_TRY(proj_gemm(c, b->ffn1, b->h2, C, (size_t)T * C, T));
  GKG_TRY(proj_apply(c, b->ffn1, T, nullptr, b->f1, Cf, 0, 0, 1, 0));
  GKG_TRY(proj_gemm(c, b->ffn2, b->f1, Cf, (size_t)T * Cf, T));
  return proj_apply(c, b->ffn2, T, b->h2, b->out, C, 0, 0, 0, 0);
}

// Backward: dout (B L, C) -> de (B L, C), dft (B, M, C) (the keys' / values' gradient), BN parameter gradients, wq[0..4].
// Temporaries: dY5 (T, C), df1 (T, Cf), dY4 (T, Cf), dh2 (T, C), dY3 (T, C), dA2 (T, 2C), dY2 (4, T, C/2), dXM (T, 2C), gx1, dY1 (T, C).
extern "C" int gkg_grapher_label_bwd(const GkgLabelBlock* b, GkgWgradProblem* wq, void* st) {
  GKG_TRY(check_label(b, wq, true));
  const Ctx c{b->bn_frozen != 0, b->sk_ws, b->sk_bytes, st, x6_flags_of(b->bwd_flags)};
  const int C = b->C, T = b->B * b->L, Cf = b->ffn1.cout;
  // (round 9, unless GKG_BLOCK_NO_DGRAD_STATS or frozen: each input-gradient GEMM of the chain ffn2 -> ffn1 -> fc2 -> conv takes the
  // backward statistics of the layer in front of it, whose BN backward is then its apply pass — three launches fewer)
  const bool s4 = dgrad_stats_ok(c, b->ffn2, b->bwd_flags, T, false), s3 = dgrad_stats_ok(c, b->ffn1, b->bwd_flags, T, true),
             s2 = dgrad_stats_ok(c, b->fc2, b->bwd_flags, T, false);
  GKG_TRY(proj_bwd(c, b->ffn2, false, &b->ffn1, s4, 1, b->dout, C, 0, T, 0, b->dY5, nullptr, b->df1, 0, 0));
  wgrad_entry(wq[0], b->ffn2, b->dY5, b->f1, Cf, (size_t)T * Cf, T, 0);
  GKG_TRY(proj_bwd(c, b->ffn1, s4, &b->fc2, s3, 0, b->df1, Cf, 0, T, 1, b->dY4, b->dout, b->dh2, 0, 0));   // + the FFN residual's gradient
  wgrad_entry(wq[1], b->ffn1, b->dY4, b->h2, C, (size_t)T * C, T, 0);
  GKG_TRY(proj_bwd(c, b->fc2, s3, &b->conv, s2, 1, b->dh2, C, 0, T, 0, b->dY3, nullptr, b->dA2, 0, 0));
  wgrad_entry(wq[2], b->fc2, b->dY3, b->A2, 2 * C, (size_t)T * 2 * C, T, 0);
  GKG_TRY(core_bwd(c, b, wq + 3, s2, b->e, b->dft, b->L, b->M));
  return proj_dgrad(c, b->fc1, nullptr, 0, b->dY1, T, b->dh2, b->de, 0, 0);                                  // + the block residual's gradient
}
