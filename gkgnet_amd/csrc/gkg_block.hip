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
#include "gkg_common.h"

using namespace gkg;

namespace {

#define GKG_TRY(call)              \
  do {                             \
    const int rc_ = (call);        \
    if (rc_ != 0) return rc_;      \
  } while (0)

// y = x W^T (statistics into p.fsum), then out = act(BN_train(y)) (+ res): the two launches of every projection layer
int proj_fwd(const GkgProjBN& p, const float* x, int ldx, size_t x_bstride, int R, void* sk_ws, size_t sk_bytes, void* st) {
  return gkg_linear_bn_fwd_x6_sk(x, ldx, x_bstride, p.planes_fwd, p.Y, R, p.cin, p.cout, p.nb, 2, nullptr, nullptr, nullptr, nullptr,
                                 nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, 0.f, p.fsum, sk_ws, sk_bytes, 0, st);
}
int proj_apply(const GkgProjBN& p, int R, const float* res, float* out, int ldo, size_t obs, int ochunk, int act, int nchw_B, void* st) {
  const int n = p.nb * p.cout;
  return gkg_bn_apply_train(p.Y, p.fsum, p.gamma, p.beta, p.bias, p.running_mean, p.running_var, p.nbt, p.bn, p.bn + n, p.bn + 2 * n,
                            p.bn + 3 * n, res, out, R, p.cout, p.nb, ldo, obs, ochunk, act, nchw_B, nullptr, 0, p.momentum, p.eps,
                            p.fzero, p.fzero_n, st);
}
// dY = BN backward of out = act(BN(Y)) for the upstream gradient g (row pitch ldg, batch stride gbs), then dx = dY W (+ residual)
int proj_bwd(const GkgProjBN& p, const float* g, int ldg, size_t gbs, int R, int act, float* dY, const float* residual, float* dx,
             int ldx, size_t x_bstride, void* sk_ws, size_t sk_bytes, void* st) {
  const int n = p.nb * p.cout;
  GKG_TRY(gkg_bn_bwd_atomic(g, p.Y, p.bn, p.bn + n, p.bn + 2 * n, p.bn + 3 * n, dY, p.dgamma, p.dbeta, R, p.cout, p.nb, ldg, gbs, act,
                            p.bsum, p.bzero, p.bzero_n, st));
  if (!dx) return 0;
  return gkg_linear_dgrad_x6_sk(dY, p.cout, (size_t)R * p.cout, p.planes_dgrad, dx, R, p.cin, p.cout, p.nb, residual, sk_ws, sk_bytes, ldx,
                                x_bstride, 0, st);
}
// The BN half of proj_bwd with the statistics ALREADY in p.bsum — left there by the kernel that produced g
// (gkg_nchw_to_tm_add_bnstats, gkg_mr_bwd_tm_bnstats; un-grouped layer, act == 0): the apply pass only.
int proj_bwd_apply(const GkgProjBN& p, const float* g, int R, float* dY, void* st) {
  const int n = p.cout;
  return gkg_bn_bwd_apply_from_sums(g, p.Y, p.bn, p.bn + n, p.bn + 2 * n, p.bn + 3 * n, dY, p.dgamma, p.dbeta, R, p.cout, 1, p.cout, 0, 0,
                                    p.bsum, p.bzero, p.bzero_n, st);
}
// Round 9.  proj_dgrad with the backward statistics of the layer q IN FRONT (q's output, act(BN(q.Y)), is this projection's input,
// so dx is q's upstream gradient) taken in the GEMM's epilogue into q.bsum, and the BN half of proj_bwd for such a layer: the
// apply pass only, in the layout proj_bwd gives it (grouped: row pitch ldg, batch stride gbs).
int proj_dgrad_stats(const GkgProjBN& p, const GkgProjBN& q, int qact, const float* dY, int R, const float* residual, float* dx,
                     void* sk_ws, size_t sk_bytes, void* st) {
  const int n = q.nb * q.cout;
  return gkg_linear_dgrad_x6_bnbwd_sk(dY, p.cout, p.planes_dgrad, dx, R, p.cin, p.cout, residual, q.Y, q.bn, q.bn + n, q.bn + 2 * n,
                                      q.bn + 3 * n, q.bsum, q.nb, q.cout, qact, sk_ws, sk_bytes, 0, st);
}
bool dgrad_stats_ok(const GkgProjBN& p, unsigned bwd_flags, int R, bool residual, const void* sk_ws) {
  return !(bwd_flags & (GKG_BLOCK_NO_BWD_FUSE | GKG_BLOCK_NO_DGRAD_STATS)) && p.nb == 1 &&
         gkg_linear_dgrad_x6_bnbwd_sk_supported(R, p.cin, residual ? 1 : 0, sk_ws ? 1 : 0, 0);
}
int proj_bwd_apply_at(const GkgProjBN& p, const float* g, int ldg, size_t gbs, int R, int act, float* dY, void* st) {
  const int n = p.nb * p.cout;
  return gkg_bn_bwd_apply_from_sums(g, p.Y, p.bn, p.bn + n, p.bn + 2 * n, p.bn + 3 * n, dY, p.dgamma, p.dbeta, R, p.cout, p.nb, ldg, gbs,
                                    act, p.bsum, p.bzero, p.bzero_n, st);
}
// proj_bwd of layer p whose statistics came with its upstream gradient (`have`) and whose own input gradient takes those of the
// layer q in front (`give`; q == nullptr: none)
int proj_bwd_chain(const GkgProjBN& p, bool have, const GkgProjBN* q, bool give, int qact, const float* g, int ldg, size_t gbs, int R,
                   int act, float* dY, const float* residual, float* dx, int ldx, size_t x_bstride, void* sk_ws, size_t sk_bytes,
                   void* st) {
  const int n = p.nb * p.cout;
  if (have) GKG_TRY(proj_bwd_apply_at(p, g, ldg, gbs, R, act, dY, st));
  else GKG_TRY(gkg_bn_bwd_atomic(g, p.Y, p.bn, p.bn + n, p.bn + 2 * n, p.bn + 3 * n, dY, p.dgamma, p.dbeta, R, p.cout, p.nb, ldg, gbs, act,
                                 p.bsum, p.bzero, p.bzero_n, st));
  if (give && q) return proj_dgrad_stats(p, *q, qact, dY, R, residual, dx, sk_ws, sk_bytes, st);
  return gkg_linear_dgrad_x6_sk(dY, p.cout, (size_t)R * p.cout, p.planes_dgrad, dx, R, p.cin, p.cout, p.nb, residual, sk_ws, sk_bytes, ldx,
                                x_bstride, 0, st);
}
int proj_dgrad(const GkgProjBN& p, const float* dY, int R, const float* residual, float* dx, void* sk_ws, size_t sk_bytes, void* st) {
  return gkg_linear_dgrad_x6_sk(dY, p.cout, (size_t)R * p.cout, p.planes_dgrad, dx, R, p.cin, p.cout, p.nb, residual, sk_ws, sk_bytes, 0, 0, 0, st);
}
// gkg_mr_bwd_tm with fc1's BN backward statistics taken inside the scatter (then only the apply pass follows), or — bwd_fuse off,
// or a shape whose scatter form carries none — the plain call and the two-launch BN backward
int mr_bwd_bn(const GkgProjBN& p, const GkgGraphOp& g, bool fuse, const float* dXM, float* gx1, float* gsrc, int B, int C, int N, int M,
              float* dY, void* st) {
  const uint8_t* arg = reinterpret_cast<const uint8_t*>(g.arg);
  const int T = B * N;
  if (fuse) {
    const int rc = gkg_mr_bwd_tm_bnstats(dXM, nullptr, arg, gx1, gsrc, B, g.G, C / g.G, N, M, g.k, 1, 1, g.mr_flags, p.Y, p.bn + 2 * p.cout,
                                         p.bn + 3 * p.cout, p.bsum, st);
    if (rc == 0) return proj_bwd_apply(p, gx1, T, dY, st);
    if (rc != GKG_ERR_UNSUPPORTED) return rc;
  }
  GKG_TRY(gkg_mr_bwd_tm(dXM, nullptr, arg, gx1, gsrc, B, g.G, C / g.G, N, M, g.k, 1, 1, g.mr_flags, st));
  return proj_bwd(p, gx1, p.cout, 0, T, 0, dY, nullptr, nullptr, 0, 0, nullptr, 0, st);
}
// ---- frozen (eval-mode) BatchNorm: the launches fused.py issues for a layer whose BN uses its running statistics ----------------
// y = x W^T without statistics, then (a, c) folded from the running statistics and the conv bias into p.bn's a | c slots
int proj_fwd_frozen(const GkgProjBN& p, const float* x, int ldx, size_t x_bstride, int R, void* sk_ws, size_t sk_bytes, void* st) {
  GKG_TRY(gkg_linear_bn_fwd_x6_sk(x, ldx, x_bstride, p.planes_fwd, p.Y, R, p.cin, p.cout, p.nb, 0, nullptr, nullptr, nullptr, nullptr,
                                  nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, 0.f, nullptr, sk_ws, sk_bytes, 0, st));
  const int n = p.nb * p.cout;
  return gkg_bn_eval_affine(p.gamma, p.beta, p.bias, p.running_mean, p.running_var, p.bn, p.bn + n, n, p.eps, st);
}
int proj_apply_frozen(const GkgProjBN& p, int R, const float* res, float* out, int ldo, size_t obs, int ochunk, int act, void* st) {
  return gkg_affine_act(p.Y, p.bn, p.bn + p.nb * p.cout, res, out, R, p.cout, p.nb, ldo, obs, ochunk, act, GKG_F32, nullptr, 0, st);
}
// fc1's apply: also the k-NN's token preparation when the graph op asks for prepared queries
int fc1_apply_frozen(const GkgProjBN& p, const GkgGraphOp& g, float* XM, int B, int C, int N, int M, int has_y, void* st) {
  if (g.knn_flags & GKG_KNN_X_PREPARED)
    return gkg_affine_knn_prep(p.Y, p.bn, p.bn + C, XM, 2 * C, C / 4, B, g.G, C / g.G, N, M, g.k, g.d, has_y, g.relpos ? 1 : 0,
                               g.knn_flags & ~(GKG_KNN_X_PREPARED | GKG_KNN_Y_PREPARED), g.fused_mr, 0, nullptr, nullptr, g.knn_ws,
                               g.knn_ws_bytes, st);
  return proj_apply_frozen(p, B * N, nullptr, XM, 2 * C, 0, C / 4, 0, st);
}
// dY of out = act(BN_eval(Y)): one sweep; with a parameter gradient wanted the sweep takes two column sums into p.bsum and a
// small second launch finishes dgamma / dbeta / dbias (and clears p.bzero)
int bn_bwd_frozen(const GkgProjBN& p, const float* g, int ldg, size_t gbs, int R, int act, float* dY, void* st) {
  const bool want = p.dgamma || p.dbeta || p.dbias;
  return gkg_bn_eval_bwd(g, p.Y, p.bn, p.bn + p.nb * p.cout, dY, R, p.cout, p.nb, ldg, gbs, act, nullptr, 0, p.running_mean,
                         p.running_var, p.bias, p.eps, p.dgamma, p.dbeta, p.dbias, want ? p.bsum : nullptr, want ? p.bzero : nullptr,
                         want ? p.bzero_n : 0, nullptr, 0, st);
}
int proj_bwd_frozen(const GkgProjBN& p, const float* g, int ldg, size_t gbs, int R, int act, float* dY, const float* residual, float* dx,
                    int ldx, size_t x_bstride, void* sk_ws, size_t sk_bytes, void* st) {
  GKG_TRY(bn_bwd_frozen(p, g, ldg, gbs, R, act, dY, st));
  return gkg_linear_dgrad_x6_sk(dY, p.cout, (size_t)R * p.cout, p.planes_dgrad, dx, R, p.cin, p.cout, p.nb, residual, sk_ws, sk_bytes, ldx,
                                x_bstride, 0, st);
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
int check_graph(const GkgGraphOp& g, int C, const char* who_null, const char* who_shape) {
  if (g.G <= 0 || C % g.G || g.k <= 0 || g.d <= 0) return gkg_fail(GKG_ERR_SHAPE, who_shape);
  if (!g.arg || !g.knn_ws) return gkg_fail(GKG_ERR_NULL, who_null);
  return 0;
}
int check_grapher(const GkgGrapherBlock* b, const GkgWgradProblem* wq, bool bwd) {
  const char* nul = bwd ? "gkg_grapher_bwd: null pointer" : "gkg_grapher_fwd: null pointer";
  const char* shp = bwd ? "gkg_grapher_bwd: C % 16 == 0, G > 0, C % G == 0; fc1 C -> C, conv 4 x (C/2 -> C/2), fc2 2C -> C"
                        : "gkg_grapher_fwd: C % 16 == 0, G > 0, C % G == 0; fc1 C -> C, conv 4 x (C/2 -> C/2), fc2 2C -> C";
  if (!b || (bwd && !wq)) return gkg_fail(GKG_ERR_NULL, nul);
  const int C = b->C;
  if (b->B <= 0 || b->H <= 0 || b->W <= 0 || C <= 0 || (C & 15) || b->fc1.nb != 1 || b->conv.nb != 4 || b->fc2.nb != 1 || b->fc1.cin != C ||
      b->fc1.cout != C || b->conv.cin != C / 2 || b->conv.cout != C / 2 || b->fc2.cin != 2 * C || b->fc2.cout != C)
    return gkg_fail(GKG_ERR_SHAPE, shp);
  GKG_TRY(check_graph(b->graph, C, nul, shp));
  if (b->keys_ws && (b->keys_G <= 0 || C % b->keys_G)) return gkg_fail(GKG_ERR_SHAPE, shp);
  // what the forward writes and the backward reads: the block's input, the saved activations, the projections
  if (!b->x || !b->xt || !b->XM || !b->A2) return gkg_fail(GKG_ERR_NULL, nul);
  const bool frozen = b->bn_frozen != 0;
  GKG_TRY(check_proj(b->fc1, frozen, bwd, nul));
  GKG_TRY(check_proj(b->conv, frozen, bwd, nul));
  GKG_TRY(check_proj(b->fc2, frozen, bwd, nul));
  if (!bwd) return b->out ? 0 : gkg_fail(GKG_ERR_NULL, nul);
  if (!b->dout || !b->dx || !b->g3 || !b->dY3 || !b->dA2 || !b->dY2 || !b->dXM || !b->gx1 || !b->dY1 || !b->dxt) return gkg_fail(GKG_ERR_NULL, nul);
  return 0;
}
int check_label(const GkgLabelBlock* b, const GkgWgradProblem* wq, bool bwd) {
  const char* nul = bwd ? "gkg_grapher_label_bwd: null pointer" : "gkg_grapher_label_fwd: null pointer";
  const char* shp = bwd ? "gkg_grapher_label_bwd: bad projection shapes (C % 16 == 0, G > 0, C % G == 0)"
                        : "gkg_grapher_label_fwd: bad projection shapes (C % 16 == 0, G > 0, C % G == 0)";
  if (!b || (bwd && !wq)) return gkg_fail(GKG_ERR_NULL, nul);
  const int C = b->C;
  if (b->B <= 0 || b->L <= 0 || b->M <= 0 || C <= 0 || (C & 15) || b->fc1.nb != 1 || b->conv.nb != 4 || b->fc2.nb != 1 || b->ffn1.nb != 1 ||
      b->ffn2.nb != 1 || b->fc1.cin != C || b->fc1.cout != C || b->conv.cin != C / 2 || b->conv.cout != C / 2 || b->fc2.cin != 2 * C ||
      b->fc2.cout != C || b->ffn1.cin != C || b->ffn1.cout <= 0 || b->ffn2.cout != C || b->ffn2.cin != b->ffn1.cout)
    return gkg_fail(GKG_ERR_SHAPE, shp);
  GKG_TRY(check_graph(b->graph, C, nul, shp));
  if (!b->e || !b->ft || !b->XM || !b->A2 || !b->h2 || !b->f1) return gkg_fail(GKG_ERR_NULL, nul);
  const bool frozen = b->bn_frozen != 0;
  GKG_TRY(check_proj(b->fc1, frozen, bwd, nul));
  GKG_TRY(check_proj(b->conv, frozen, bwd, nul));
  GKG_TRY(check_proj(b->fc2, frozen, bwd, nul));
  GKG_TRY(check_proj(b->ffn1, frozen, bwd, nul));
  GKG_TRY(check_proj(b->ffn2, frozen, bwd, nul));
  if (!bwd) return b->out ? 0 : gkg_fail(GKG_ERR_NULL, nul);
  if (!b->dout || !b->de || !b->dft || !b->dY5 || !b->df1 || !b->dY4 || !b->dh2 || !b->dY3 || !b->dA2 || !b->dY2 || !b->dXM || !b->gx1 || !b->dY1)
    return gkg_fail(GKG_ERR_NULL, nul);
  return 0;
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

}  // namespace

// ---- Grapher (reference torch_vertex.py:325-333): x (B, C, H, W) -> out (B, C, H, W) [+ out_tm (B N, C)] ----------------------
extern "C" int gkg_grapher_fwd(const GkgGrapherBlock* b, void* st) {
  GKG_TRY(check_grapher(b, nullptr, false));
  const int B = b->B, C = b->C, N = b->H * b->W, T = B * N;
  // block entry: NCHW -> token-major
  GKG_TRY(gkg_nchw_to_tm(b->x, b->xt, B, C, N, GKG_F32, nullptr, st));
  if (b->bn_frozen) {
    // every BatchNorm on its running statistics: projection without statistics, folded affine, apply — nothing else is written
    const GkgGraphOp& g = b->graph;
    GKG_TRY(proj_fwd_frozen(b->fc1, b->xt, C, (size_t)T * C, T, b->sk_ws, b->sk_bytes, st));
    GKG_TRY(fc1_apply_frozen(b->fc1, g, b->XM, B, C, N, N, 0, st));
    GKG_TRY(graph_fwd(g, b->XM, nullptr, B, C, N, N, st));
    GKG_TRY(proj_fwd_frozen(b->conv, b->XM, 2 * C, (size_t)(C / 2), T, b->sk_ws, b->sk_bytes, st));
    GKG_TRY(proj_apply_frozen(b->conv, T, nullptr, b->A2, 2 * C, (size_t)(C / 2), 0, 1, st));
    GKG_TRY(proj_fwd_frozen(b->fc2, b->A2, 2 * C, (size_t)T * 2 * C, T, b->sk_ws, b->sk_bytes, st));
    const GkgProjBN& p = b->fc2;
    if (b->out_tm && b->keys_ws)
      return gkg_affine_knn_prep(p.Y, p.bn, p.bn + C, b->out_tm, 0, 0, B, b->keys_G, C / b->keys_G, b->keys_L, N, b->keys_k, b->keys_d, 1, 0,
                                 b->keys_flags, b->keys_fused_mr, 1, b->xt, b->out, b->keys_ws, b->keys_ws_bytes, st);
    if (b->out_tm) return gkg_tm_affine_to_nchw_dual(p.Y, p.bn, p.bn + C, b->xt, b->out, b->out_tm, B, C, N, st);
    return gkg_tm_affine_to_nchw(p.Y, p.bn, p.bn + C, b->x, b->out, B, C, N, nullptr, st);
  }
  // fc1 + BN: x into the x half of the operand buffer; the same pass prepares the k-NN's queries when the graph op asks for it
  GKG_TRY(proj_fwd(b->fc1, b->xt, C, (size_t)T * C, T, b->sk_ws, b->sk_bytes, st));
  const GkgGraphOp& g = b->graph;
  if (g.knn_flags & GKG_KNN_X_PREPARED) {
    const int n = C;
    GKG_TRY(gkg_bn_apply_knn_prep(b->fc1.Y, b->fc1.fsum, b->fc1.gamma, b->fc1.beta, b->fc1.bias, b->fc1.running_mean, b->fc1.running_var,
                                  b->fc1.nbt, b->fc1.bn, b->fc1.bn + n, b->fc1.bn + 2 * n, b->fc1.bn + 3 * n, b->XM, 2 * C, C / 4, B, g.G,
                                  C / g.G, N, N, g.k, g.d, 0, g.relpos ? 1 : 0, g.knn_flags & ~(GKG_KNN_X_PREPARED | GKG_KNN_Y_PREPARED),
                                  g.fused_mr, 0, nullptr, nullptr, g.knn_ws, g.knn_ws_bytes, b->fc1.momentum, b->fc1.eps, b->fc1.fzero,
                                  b->fc1.fzero_n, st));
  } else {
    GKG_TRY(proj_apply(b->fc1, T, nullptr, b->XM, 2 * C, 0, C / 4, 0, 0, st));
  }
  // graph + aggregation (self graph), then BasicConv on the operand buffer
  GKG_TRY(graph_fwd(g, b->XM, nullptr, B, C, N, N, st));
  GKG_TRY(proj_fwd(b->conv, b->XM, 2 * C, (size_t)(C / 2), T, b->sk_ws, b->sk_bytes, st));
  GKG_TRY(proj_apply(b->conv, T, nullptr, b->A2, 2 * C, (size_t)(C / 2), 0, 1, 0, st));
  // fc2 + BN + residual -> NCHW (+ the token-major companion, + the keys of the label graph behind)
  GKG_TRY(proj_fwd(b->fc2, b->A2, 2 * C, (size_t)T * 2 * C, T, b->sk_ws, b->sk_bytes, st));
  const GkgProjBN& p = b->fc2;
  if (b->out_tm && b->keys_ws) {
    return gkg_bn_apply_knn_prep(p.Y, p.fsum, p.gamma, p.beta, p.bias, p.running_mean, p.running_var, p.nbt, p.bn, p.bn + C, p.bn + 2 * C,
                                 p.bn + 3 * C, b->out_tm, 0, 0, B, b->keys_G, C / b->keys_G, b->keys_L, N, b->keys_k, b->keys_d, 1, 0,
                                 b->keys_flags, b->keys_fused_mr, 1, b->xt, b->out, b->keys_ws, b->keys_ws_bytes, p.momentum, p.eps,
                                 p.fzero, p.fzero_n, st);
  }
  if (b->out_tm)
    return gkg_bn_apply_train_dual(p.Y, p.fsum, p.gamma, p.beta, p.bias, p.running_mean, p.running_var, p.nbt, p.bn, p.bn + C, p.bn + 2 * C,
                                   p.bn + 3 * C, b->xt, b->out, b->out_tm, B, C, N, p.momentum, p.eps, p.fzero, p.fzero_n, st);
  return proj_apply(p, T, b->x, b->out, C, 0, 0, 0, B, st);
}

// Backward of the above: dout (B, C, H, W) [+ dout_tm (B N, C): the gradient of the token-major companion] -> dx (B, C, H, W), the
// BN parameter gradients, and the three weight-gradient PROBLEMS in wq[0..2] (for gkg_linear_wgrad_x6_batch: the caller launches
// them now or queues them with the rest of the backward pass).  Temporaries: g3, dY3 (T, C), dA2 (T, 2C), dY2 (4, T, C/2),
// dXM (T, 2C), gx1, dY1, dxt (T, C) — caller-owned; dY3 / dY2 / dY1 must stay valid until the weight gradients have run.
extern "C" int gkg_grapher_bwd(const GkgGrapherBlock* b, GkgWgradProblem* wq, void* st) {
  GKG_TRY(check_grapher(b, wq, true));
  const int B = b->B, C = b->C, N = b->H * b->W, T = B * N;
  if (b->bn_frozen) {
    // running statistics: each BN backward is gkg_bn_eval_bwd (one sweep, + a finishing launch when a parameter gradient is
    // wanted) in front of the plain input-gradient GEMM; no statistics ride in another kernel
    if (b->dout_tm) GKG_TRY(gkg_nchw_to_tm_add(b->dout, b->dout_tm, b->g3, B, C, N, st));
    else GKG_TRY(gkg_nchw_to_tm(b->dout, b->g3, B, C, N, GKG_F32, nullptr, st));
    GKG_TRY(proj_bwd_frozen(b->fc2, b->g3, C, 0, T, 0, b->dY3, nullptr, b->dA2, 0, 0, b->sk_ws, b->sk_bytes, st));
    wgrad_entry(wq[0], b->fc2, b->dY3, b->A2, 2 * C, (size_t)T * 2 * C, T, 0);
    GKG_TRY(proj_bwd_frozen(b->conv, b->dA2, 2 * C, (size_t)(C / 2), T, 1, b->dY2, nullptr, b->dXM, 2 * C, (size_t)(C / 2), b->sk_ws,
                            b->sk_bytes, st));
    wgrad_entry(wq[1], b->conv, b->dY2, b->XM, 2 * C, (size_t)(C / 2), T, 1);
    const GkgGraphOp& g = b->graph;
    GKG_TRY(gkg_mr_bwd_tm(b->dXM, nullptr, reinterpret_cast<const uint8_t*>(g.arg), b->gx1, nullptr, B, g.G, C / g.G, N, N, g.k, 1, 1,
                          g.mr_flags, st));
    GKG_TRY(bn_bwd_frozen(b->fc1, b->gx1, C, 0, T, 0, b->dY1, st));
    wgrad_entry(wq[2], b->fc1, b->dY1, b->xt, C, (size_t)T * C, T, 0);
    if (!(b->bwd_flags & GKG_BLOCK_NO_BWD_FUSE))
      return gkg_linear_dgrad_x6_nchw(b->dY1, C, b->fc1.planes_dgrad, b->dx, b->dxt, T, C, C, b->g3, B, N, b->sk_ws, b->sk_bytes, 0, st);
    GKG_TRY(proj_dgrad(b->fc1, b->dY1, T, b->g3, b->dxt, b->sk_ws, b->sk_bytes, st));
    return gkg_tm_affine_to_nchw(b->dxt, nullptr, nullptr, nullptr, b->dx, B, C, N, nullptr, st);
  }
  // the output's gradient(s) token-major; it is also the residual branch's gradient
  // (round 8, unless GKG_BLOCK_NO_BWD_FUSE: the re-layout pass takes fc2's BN backward statistics, the scatter takes fc1's, and
  // fc1's input-gradient GEMM stores dx channel-major — four launches fewer)
  // (round 9, unless GKG_BLOCK_NO_DGRAD_STATS: fc2's input-gradient GEMM takes the grouped projection's — one launch fewer)
  const bool fuse = !(b->bwd_flags & GKG_BLOCK_NO_BWD_FUSE);
  const bool conv_stats = dgrad_stats_ok(b->fc2, b->bwd_flags, T, false, b->sk_ws);
  if (fuse) {
    GKG_TRY(gkg_nchw_to_tm_add_bnstats(b->dout, b->dout_tm, b->g3, b->fc2.Y, b->fc2.bn + 2 * C, b->fc2.bn + 3 * C, b->fc2.bsum, B, C, N, st));
    GKG_TRY(proj_bwd_apply(b->fc2, b->g3, T, b->dY3, st));
    if (conv_stats) GKG_TRY(proj_dgrad_stats(b->fc2, b->conv, 1, b->dY3, T, nullptr, b->dA2, b->sk_ws, b->sk_bytes, st));
    else GKG_TRY(proj_dgrad(b->fc2, b->dY3, T, nullptr, b->dA2, b->sk_ws, b->sk_bytes, st));
  } else {
    if (b->dout_tm) GKG_TRY(gkg_nchw_to_tm_add(b->dout, b->dout_tm, b->g3, B, C, N, st));
    else GKG_TRY(gkg_nchw_to_tm(b->dout, b->g3, B, C, N, GKG_F32, nullptr, st));
    GKG_TRY(proj_bwd(b->fc2, b->g3, C, 0, T, 0, b->dY3, nullptr, b->dA2, 0, 0, b->sk_ws, b->sk_bytes, st));
  }
  wgrad_entry(wq[0], b->fc2, b->dY3, b->A2, 2 * C, (size_t)T * 2 * C, T, 0);
  GKG_TRY(proj_bwd_chain(b->conv, conv_stats, nullptr, false, 0, b->dA2, 2 * C, (size_t)(C / 2), T, 1, b->dY2, nullptr, b->dXM, 2 * C,
                         (size_t)(C / 2), b->sk_ws, b->sk_bytes, st));
  wgrad_entry(wq[1], b->conv, b->dY2, b->XM, 2 * C, (size_t)(C / 2), T, 1);
  const GkgGraphOp& g = b->graph;
  GKG_TRY(mr_bwd_bn(b->fc1, g, fuse, b->dXM, b->gx1, nullptr, B, C, N, N, b->dY1, st));
  // fc1: its input gradient + the residual branch's (g3), channel-major (NCHW)
  wgrad_entry(wq[2], b->fc1, b->dY1, b->xt, C, (size_t)T * C, T, 0);
  if (fuse)
    return gkg_linear_dgrad_x6_nchw(b->dY1, C, b->fc1.planes_dgrad, b->dx, b->dxt, T, C, C, b->g3, B, N, b->sk_ws, b->sk_bytes, 0, st);
  GKG_TRY(proj_dgrad(b->fc1, b->dY1, T, b->g3, b->dxt, b->sk_ws, b->sk_bytes, st));
  return gkg_tm_affine_to_nchw(b->dxt, nullptr, nullptr, nullptr, b->dx, B, C, N, nullptr, st);
}

// ---- GrapherLabel (reference torch_vertex.py:392-403 + FFNLabel :334-360): e (B L, C), keys / values ft (B, M, C) -> E' (B L, C) -----
extern "C" int gkg_grapher_label_fwd(const GkgLabelBlock* b, void* st) {
  GKG_TRY(check_label(b, nullptr, false));
  const int B = b->B, C = b->C, L = b->L, M = b->M, T = B * L;
  const GkgGraphOp& g = b->graph;
  if (b->bn_frozen) {
    const int Cf = b->ffn1.cout;
    GKG_TRY(proj_fwd_frozen(b->fc1, b->e, C, (size_t)T * C, T, b->sk_ws, b->sk_bytes, st));
    GKG_TRY(fc1_apply_frozen(b->fc1, g, b->XM, B, C, L, M, 1, st));
    GKG_TRY(graph_fwd(g, b->XM, b->ft, B, C, L, M, st));
    GKG_TRY(proj_fwd_frozen(b->conv, b->XM, 2 * C, (size_t)(C / 2), T, b->sk_ws, b->sk_bytes, st));
    GKG_TRY(proj_apply_frozen(b->conv, T, nullptr, b->A2, 2 * C, (size_t)(C / 2), 0, 1, st));
    GKG_TRY(proj_fwd_frozen(b->fc2, b->A2, 2 * C, (size_t)T * 2 * C, T, b->sk_ws, b->sk_bytes, st));
    GKG_TRY(proj_apply_frozen(b->fc2, T, b->e, b->h2, C, 0, 0, 0, st));
    GKG_TRY(proj_fwd_frozen(b->ffn1, b->h2, C, (size_t)T * C, T, b->sk_ws, b->sk_bytes, st));
    GKG_TRY(proj_apply_frozen(b->ffn1, T, nullptr, b->f1, Cf, 0, 0, 1, st));
    GKG_TRY(proj_fwd_frozen(b->ffn2, b->f1, Cf, (size_t)T * Cf, T, b->sk_ws, b->sk_bytes, st));
    return proj_apply_frozen(b->ffn2, T, b->h2, b->out, C, 0, 0, 0, st);
  }
  GKG_TRY(proj_fwd(b->fc1, b->e, C, (size_t)T * C, T, b->sk_ws, b->sk_bytes, st));
  if (g.knn_flags & GKG_KNN_X_PREPARED) {
    const GkgProjBN& p = b->fc1;
    GKG_TRY(gkg_bn_apply_knn_prep(p.Y, p.fsum, p.gamma, p.beta, p.bias, p.running_mean, p.running_var, p.nbt, p.bn, p.bn + C, p.bn + 2 * C,
                                  p.bn + 3 * C, b->XM, 2 * C, C / 4, B, g.G, C / g.G, L, M, g.k, g.d, 1, 0,
                                  g.knn_flags & ~(GKG_KNN_X_PREPARED | GKG_KNN_Y_PREPARED), g.fused_mr, 0, nullptr, nullptr, g.knn_ws,
                                  g.knn_ws_bytes, p.momentum, p.eps, p.fzero, p.fzero_n, st));
  } else {
    GKG_TRY(proj_apply(b->fc1, T, nullptr, b->XM, 2 * C, 0, C / 4, 0, 0, st));
  }
  GKG_TRY(graph_fwd(g, b->XM, b->ft, B, C, L, M, st));
  GKG_TRY(proj_fwd(b->conv, b->XM, 2 * C, (size_t)(C / 2), T, b->sk_ws, b->sk_bytes, st));
  GKG_TRY(proj_apply(b->conv, T, nullptr, b->A2, 2 * C, (size_t)(C / 2), 0, 1, 0, st));
  GKG_TRY(proj_fwd(b->fc2, b->A2, 2 * C, (size_t)T * 2 * C, T, b->sk_ws, b->sk_bytes, st));
  GKG_TRY(proj_apply(b->fc2, T, b->e, b->h2, C, 0, 0, 0, 0, st));
  const int Cf = b->ffn1.cout;
  GKG_TRY(proj_fwd(b->ffn1, b->h2, C, (size_t)T * C, T, b->sk_ws, b->sk_bytes, st));
  GKG_TRY(proj_apply(b->ffn1, T, nullptr, b->f1, Cf, 0, 0, 1, 0, st));
  GKG_TRY(proj_fwd(b->ffn2, b->f1, Cf, (size_t)T * Cf, T, b->sk_ws, b->sk_bytes, st));
  return proj_apply(b->ffn2, T, b->h2, b->out, C, 0, 0, 0, 0, st);
}

// Backward: dout (B L, C) -> de (B L, C), dft (B, M, C) (the keys' / values' gradient), BN parameter gradients, wq[0..4].
// Temporaries: dY5 (T, C), df1 (T, Cf), dY4 (T, Cf), dh2 (T, C), dY3 (T, C), dA2 (T, 2C), dY2 (4, T, C/2), dXM (T, 2C), gx1, dY1 (T, C).
extern "C" int gkg_grapher_label_bwd(const GkgLabelBlock* b, GkgWgradProblem* wq, void* st) {
  GKG_TRY(check_label(b, wq, true));
  const int B = b->B, C = b->C, L = b->L, M = b->M, T = B * L, Cf = b->ffn1.cout;
  const GkgGraphOp& g = b->graph;
  if (b->bn_frozen) {
    GKG_TRY(proj_bwd_frozen(b->ffn2, b->dout, C, 0, T, 0, b->dY5, nullptr, b->df1, 0, 0, b->sk_ws, b->sk_bytes, st));
    wgrad_entry(wq[0], b->ffn2, b->dY5, b->f1, Cf, (size_t)T * Cf, T, 0);
    GKG_TRY(proj_bwd_frozen(b->ffn1, b->df1, Cf, 0, T, 1, b->dY4, b->dout, b->dh2, 0, 0, b->sk_ws, b->sk_bytes, st));   // + the FFN residual's gradient
    wgrad_entry(wq[1], b->ffn1, b->dY4, b->h2, C, (size_t)T * C, T, 0);
    GKG_TRY(proj_bwd_frozen(b->fc2, b->dh2, C, 0, T, 0, b->dY3, nullptr, b->dA2, 0, 0, b->sk_ws, b->sk_bytes, st));
    wgrad_entry(wq[2], b->fc2, b->dY3, b->A2, 2 * C, (size_t)T * 2 * C, T, 0);
    GKG_TRY(proj_bwd_frozen(b->conv, b->dA2, 2 * C, (size_t)(C / 2), T, 1, b->dY2, nullptr, b->dXM, 2 * C, (size_t)(C / 2), b->sk_ws,
                            b->sk_bytes, st));
    wgrad_entry(wq[3], b->conv, b->dY2, b->XM, 2 * C, (size_t)(C / 2), T, 1);
    GKG_TRY(gkg_mr_bwd_tm(b->dXM, nullptr, reinterpret_cast<const uint8_t*>(g.arg), b->gx1, b->dft, B, g.G, C / g.G, L, M, g.k, 1, 1,
                          g.mr_flags, st));
    GKG_TRY(bn_bwd_frozen(b->fc1, b->gx1, C, 0, T, 0, b->dY1, st));
    GKG_TRY(proj_dgrad(b->fc1, b->dY1, T, b->dh2, b->de, b->sk_ws, b->sk_bytes, st));                                 // + the block residual's gradient
    wgrad_entry(wq[4], b->fc1, b->dY1, b->e, C, (size_t)T * C, T, 0);
    return 0;
  }
  // (round 9, unless GKG_BLOCK_NO_DGRAD_STATS: each input-gradient GEMM of the chain ffn2 -> ffn1 -> fc2 -> conv takes the backward
  // statistics of the layer in front of it, whose BN backward is then its apply pass — three launches fewer)
  const bool s4 = dgrad_stats_ok(b->ffn2, b->bwd_flags, T, false, b->sk_ws), s3 = dgrad_stats_ok(b->ffn1, b->bwd_flags, T, true, b->sk_ws),
             s2 = dgrad_stats_ok(b->fc2, b->bwd_flags, T, false, b->sk_ws);
  GKG_TRY(proj_bwd_chain(b->ffn2, false, &b->ffn1, s4, 1, b->dout, C, 0, T, 0, b->dY5, nullptr, b->df1, 0, 0, b->sk_ws, b->sk_bytes, st));
  wgrad_entry(wq[0], b->ffn2, b->dY5, b->f1, Cf, (size_t)T * Cf, T, 0);
  GKG_TRY(proj_bwd_chain(b->ffn1, s4, &b->fc2, s3, 0, b->df1, Cf, 0, T, 1, b->dY4, b->dout, b->dh2, 0, 0, b->sk_ws, b->sk_bytes,
                         st));                                                                                     // + the FFN residual's gradient
  wgrad_entry(wq[1], b->ffn1, b->dY4, b->h2, C, (size_t)T * C, T, 0);
  GKG_TRY(proj_bwd_chain(b->fc2, s3, &b->conv, s2, 1, b->dh2, C, 0, T, 0, b->dY3, nullptr, b->dA2, 0, 0, b->sk_ws, b->sk_bytes, st));
  wgrad_entry(wq[2], b->fc2, b->dY3, b->A2, 2 * C, (size_t)T * 2 * C, T, 0);
  GKG_TRY(proj_bwd_chain(b->conv, s2, nullptr, false, 0, b->dA2, 2 * C, (size_t)(C / 2), T, 1, b->dY2, nullptr, b->dXM, 2 * C, (size_t)(C / 2),
                         b->sk_ws, b->sk_bytes, st));
  wgrad_entry(wq[3], b->conv, b->dY2, b->XM, 2 * C, (size_t)(C / 2), T, 1);
  GKG_TRY(mr_bwd_bn(b->fc1, g, !(b->bwd_flags & GKG_BLOCK_NO_BWD_FUSE), b->dXM, b->gx1, b->dft, B, C, L, M, b->dY1, st));
  GKG_TRY(proj_dgrad(b->fc1, b->dY1, T, b->dh2, b->de, b->sk_ws, b->sk_bytes, st));                                // + the block residual's gradient
  wgrad_entry(wq[4], b->fc1, b->dY1, b->e, C, (size_t)T * C, T, 0);
  return 0;
}
