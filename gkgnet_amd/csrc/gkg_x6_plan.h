// gkg_x6_plan.h — the launch plans of the split-bf16 ("x6") projection GEMMs and their weight gradients (gkg_gemm_x6.hip): everything
// a call decides from its sizes, pitches, flags and the device's resident-workgroup count, as pure host code (no HIP header, nothing
// __device__: tests/x6_plan/x6_plan_dump.cpp is built by a plain C++17 compiler).  The entry points fill a call, a plan function
// turns it into a plan (or a GKG_ERR_* code and the message gkg_fail gets), the launchers only read that plan and bind the pointers.
// The measurements behind every threshold are quoted where the threshold stands.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "gkg_hip.h"

namespace gkg {

// ------------------------------------------------------------------------------------------ constants and formulas, each once
constexpr int X6_NPAD = 128;             // plane rows are padded to this many n (covers NI = 2 and 4 column tiles)
constexpr int X6_STATS_DOUBLES = 2 * 4096 * 4;      // fp64 column-sum scratch of the BN-statistics epilogue (4 groups x 2 x 4096 channels)
// Split-K workspace (caller-owned, gkg_x6_splitk_workspace_bytes()): [1024 tile counters, zero between launches][partials].
constexpr size_t X6_SK_CNT_BYTES = 4096, X6_SK_MAX_WG = 512;
constexpr size_t X6_SK_BYTES = X6_SK_CNT_BYTES + X6_SK_MAX_WG * (size_t)(2 * 16 * 256 * 4);
// LDS of gemm_x6_kernel's operand rings: three 16-KiB A stages + two B stage images (+ slack: the unused lanes of a partial last
// block read past their image row); the walk form's statistics epilogue keeps its own [4 waves][BN][2] floats behind them (the
// one-tile form aliases the rings); the short-matrix body: 48 KiB of A rings (its 32 KiB of partials alias them)
constexpr int x6_ring_bytes(int NI, int BN) { return 3 * 4 * 4096 + 2 * 12 * BN * 16 + (BN != 32 * NI ? 512 : 0); }
constexpr int x6_walk_epi_bytes(bool stats, int BN) { return stats ? 4 * BN * 2 * 4 : 0; }
constexpr size_t X6_KS_LDS = 4 * 3 * 4096;
// weight-gradient LDS-DMA bodies: the rings + a zero-filled region for the lanes whose column lies outside the matrix
constexpr unsigned X6W_ZERO_BYTES = 4096;
constexpr size_t X6W_SH_DMA = (size_t)4 * 4 * 8192 + X6W_ZERO_BYTES, X6W_SH_WIDE = (size_t)4 * 3 * 16 * 192 * 4 + X6W_ZERO_BYTES;
constexpr int X6W_BATCH = 16;            // problems per batched launch (their descriptors travel in the kernel arguments)
constexpr int X6W_MAX_PROBLEMS = 256;    // per batch call

inline bool x6_bad_dim(int v) { return v <= 0 || (v & 3) != 0; }
// plane geometry of one orientation B[n][k]: n padded to X6_NPAD, k to 32 (KC chunks of 8), three planes per batch
constexpr int x6_plane_np(int n) { return (n + X6_NPAD - 1) / X6_NPAD * X6_NPAD; }
constexpr int x6_plane_kc(int k) { return (k + 31) / 32 * 4; }
inline size_t x6_plane_units(int n, int k, int nb) { return (size_t)nb * 3 * x6_plane_kc(k) * x6_plane_np(n); }      // uint4 units

enum { X6_STORE = 0, X6_BNSTATS = 1, X6_BNBWD = 2, X6_STORE_NCHW = 3 };      // the GEMM kernels' epilogues (template argument EPI)

// ------------------------------------------------------------------------------------------ forward / input-gradient GEMMs
// The rule for the short-matrix body (gemm_x6_ks_kernel; measured at x6_gemm_ladder) — ONE predicate for the launch and for the
// entry points that must know beforehand which body a shape takes.
inline bool x6_ks_form(int M, int N, int nb, bool has_ws, unsigned flags) {
  return has_ws && !(flags & GKG_X6_NO_KS) && M <= 4096 && (long long)((M + 31) / 32) * ((N + 63) / 64) * nb <= 65535 * 8 &&
         ((flags & GKG_X6_FORCE_KS) || (nb == 1 && N <= 640));
}

// The cross-workgroup split of the contraction for the 128-row tile kernel (x6_gemm_ladder): ranges per tile, < 2: none.
inline int x6_tile_ksplit(long long base2, int nk_total, bool has_ws) {
  if (!has_ws || base2 >= 320 || nk_total < 8) return 1;
  int ks = (int)(X6_SK_MAX_WG / base2);
  if (ks > nk_total / 4) ks = nk_total / 4;
  return ks > 8 ? 8 : ks;
}

// The launch rule of the walk form: the grid (workgroups) of the walk launch for `units` row blocks (batches folded in) of `ntiles`
// column tiles on `slots` resident workgroups, or 0: one tile per workgroup.  The longest XCD sequence (ceil(units / 8) row blocks)
// needs `rounds` rounds of the slots of one XCD.
//   * Walks when rounds == 2.  All workgroups of such a launch start together, so both workgroups of a CU are in their prologue
//     and in their epilogue at the same time, twice; walking, the second tile's first stages land under the first tile's
//     epilogue (cfg2's grouped 4 x (10 368 x 160 -> 160) products, 972 tiles: 26.7 -> 24.2 and 25.1 -> 21.4 us in the replayed
//     step, profiles/r11_bench_cfg2_graph_steps.txt).  From three rounds on the hardware dispatcher has de-phased the two
//     workgroups of a CU — one fills its rings while the other multiplies — and re-balances at every workgroup end, which a
//     static list cannot: walking everything made cfg2ref / stage3 / cfg4 0.9-2 % SLOWER (profiles/r11_x6_tile_walk_ab.txt).
//   * The sequence is cut into EQUAL shares: 123 entries on 64 slots are 62 workgroups of 2 (one of 1), not 64 + 59.
//   * GKG_X6_FORCE_WALK (tests, measurement): whatever the rounds; its cap field c > 0: at most 8 c workgroups.
inline int x6_walk_grid(long long units, int ntiles, int ksplit, int slots, unsigned flags) {
  if (ksplit > 1 || (flags & GKG_X6_NO_WALK)) return 0;
  const bool force = (flags & GKG_X6_FORCE_WALK) != 0;
  const long long seq = (units + 7) / 8 * ntiles, per_xcd = slots / 8;
  const long long rounds = (seq + per_xcd - 1) / per_xcd;
  if (!force && rounds != 2) return 0;
  long long w = (seq + rounds - 1) / rounds;
  const long long cap = (flags >> GKG_X6_WALK_CAP_SHIFT) & GKG_X6_WALK_CAP_MASK;
  if (force && cap > 0 && w > cap) w = cap;
  return (int)(w * 8);
}

enum X6Role {
  X6R_FWD,        // gkg_linear_bn_fwd_x6(_sk):      C (nb, M, N) = A (nb, M, K) W^T; train != 0: X6_BNSTATS, else X6_STORE
  X6R_DGRAD,      // gkg_linear_dgrad_x6(_sk):       the same product on the dgrad planes (+ residual), X6_STORE
  X6R_DGRAD_NCHW, // gkg_linear_dgrad_x6_nchw:       nb == 1, stored channel-major (X6_STORE_NCHW) or the two-launch form
  X6R_DGRAD_BNBWD // gkg_linear_dgrad_x6_bnbwd(_sk): nb == 1, the producer's BN-backward statistics in the epilogue (X6_BNBWD)
};
enum X6Body { X6_BODY_KS, X6_BODY_TILE, X6_BODY_WALK };      // gemm_x6_ks_kernel / gemm_x6_kernel / gemm_x6_walk_kernel

struct X6GemmCall {
  X6Role role;
  int M, N, K, nb;                 // rows, output columns, contraction (forward: R, cout, cin; input gradients: R, cin, cout)
  int lda; size_t a_bstride;       // the activation operand's row pitch and batch stride (floats)
  bool a_aligned;                  // ... and whether its pointer is 16-byte aligned
  int ldc; size_t c_bstride;       // X6R_DGRAD: dx's row pitch and batch stride (ldc == 0: contiguous)
  bool has_ws, ws_aligned; size_t ws_bytes;      // the split-K workspace
  unsigned flags;                  // GKG_X6_*
  bool has_residual;
  int train;                       // X6R_FWD: 0, 1, or 2 (the sums stay for a consumer that knows one copy)
  int nchw_b, nchw_n; bool dx_aligned;           // X6R_DGRAD_NCHW: M == nchw_b * nchw_n
  int pnb, pco, pact;              // X6R_DGRAD_BNBWD: the producer's BN groups / channels per group / activation
  // The device's resident-workgroup count of the walk form's kernel (workgroups per CU x CUs); 0: not known — the plan then names
  // the one-tile form and says in `walkable` whether the count would decide, and the caller asks the device and plans again.
  // QUIRK, kept: gkg_x6_walk_workgroups asks with the count of the X6_STORE walk instantiation at ring-only LDS, while the
  // training forward launches X6_BNSTATS with 2 KiB more.  Both are two workgroups per CU today; the plan itself gives equal
  // grids to equal `slots` whatever the role (tests/test_x6_plan_host.py).
  int slots;
};

struct X6GemmPlan {
  int epi;                         // X6_STORE ...
  X6Body body;
  int NI, BN;                      // gemm_x6(_walk)_kernel<NI, epi, BN>; short-matrix body: 64-column tiles (NI = 2)
  bool walkable;                   // the ladder came to the rung where call.slots decides between X6_BODY_TILE and X6_BODY_WALK
  size_t walk_lds;                 // walkable: the walk form's dynamic LDS — what the resident-workgroup count is asked with
  int mtiles, ntiles, ksplit, kper;
  unsigned grid_x, grid_y;         // 256 threads each
  size_t lds;                      // dynamic LDS bytes
  int NP, KC; size_t p_bstride;    // the planes' geometry
  int nslots;                      // X6_BNSTATS: copies of the sums the row tiles' atomics are spread over; else 0
  double work;                     // the profiler's flop
  bool two_launch;                 // X6R_DGRAD_NCHW: the plan is gkg_linear_dgrad_x6_sk's into dx_tm, gkg_tm_affine_to_nchw follows
};

// X6R_DGRAD_BNBWD: `residual` is added in front of the statistics by the short-matrix body only (= gkg_linear_dgrad_x6_bnbwd_sk_supported)
inline bool x6_bnbwd_takes_residual(int M, int N, bool has_ws, unsigned flags) { return x6_ks_form(M, N, 1, has_ws, flags); }

// X6R_DGRAD_NCHW: the shapes whose X6R_DGRAD launch is a kernel without the channel-major store (the short-matrix body, 80-column
// tiles) or whose store would not be 16-byte (nchw_n % 4, dx) keep gkg_linear_dgrad_x6_sk + gkg_tm_affine_to_nchw.
// `wide80` is a statement of its OWN, kept as the entry point had it, not the ladder's answer: it repeats the ladder's two constants
// — N == 80 (the 80-column rung) and base2 >= 160 (the 32-column rung's bound, nb == 1) — but reads neither the flags nor the
// split.  Under GKG_X6_FORCE_WALK with base2 < 160 the X6R_DGRAD ladder takes 80-column tiles and this says one launch; with a
// workspace, 160 <= base2 < 320 and a long contraction the ladder splits K on 64-column tiles and this says two launches.  dx has
// the same bits either way, so deriving it from the ladder would only move launches; whoever edits 80 or 160 in x6_gemm_ladder edits
// them here (tests/x6_plan/cases.txt has both disagreements and both sides of 160).
inline bool x6_nchw_two_launch(const X6GemmCall& q) {
  const bool wide80 = q.N == 80 && (long long)((q.M + 127) / 128) * ((q.N + 63) / 64) >= 160;
  return (q.nchw_n & 3) || x6_ks_form(q.M, q.N, 1, q.has_ws, q.flags) || wide80 || !q.dx_aligned;
}

// The launch ladder of a call whose sizes are valid: body, tile width, split, walk, grid, LDS.
inline void x6_gemm_ladder(const X6GemmCall& q, X6GemmPlan* p) {
  const int M = q.M, N = q.N, K = q.K, nb = q.nb;
  const int epi = q.role == X6R_FWD ? (q.train ? X6_BNSTATS : X6_STORE) : q.role == X6R_DGRAD ? X6_STORE
                  : q.role == X6R_DGRAD_NCHW ? X6_STORE_NCHW : X6_BNBWD;
  *p = X6GemmPlan{};
  p->epi = epi;
  p->work = 2.0 * M * N * K * nb;
  p->NP = x6_plane_np(N); p->KC = x6_plane_kc(K); p->p_bstride = (size_t)3 * p->KC * p->NP;
  p->ksplit = 1;
  if (epi == X6_BNSTATS) {
    // copies of the sums to spread the row tiles' atomics over (train == 2 leaves the sums for a consumer that knows one copy)
    const int fit = X6_STATS_DOUBLES / (nb * 2 * N), want = (M + 127) / 128 / 64;
    p->nslots = q.train == 2 ? 1 : (want < 1 ? 1 : (want > 16 ? 16 : want));
    if (p->nslots > fit) p->nslots = fit;
  }
  auto tile = [&](int NI, int BN) {
    p->body = X6_BODY_TILE; p->NI = NI; p->BN = BN;
    p->mtiles = (M + 127) / 128; p->ntiles = (N + BN - 1) / BN;
    p->grid_x = (unsigned)((p->mtiles + 7) / 8 * 8 * p->ntiles * p->ksplit); p->grid_y = (unsigned)nb;
    p->lds = (size_t)x6_ring_bytes(NI, BN);
  };
  // Few rows (<= 4 096: the label branch): the waves of a workgroup split K instead of M (gemm_x6_ks_kernel) — taken by the _sk
  // entry points, i.e. by callers that asked for the short-matrix forms.
  // Where it pays (measured inside the cfg2 step, same box, us, this body vs gemm_x6_kernel with cross-workgroup split-K:
  // profiles/r05_x6_ks_vs_tile_kernel.txt): 2 560 x 320 -> 320 11.0 vs 13.1 (input gradient + residual 11.7 vs 20.7), 640 -> 320
  // 15.2 vs 21.2, 1280 -> 320 24.3 vs 29.6 (input gradient of 320 -> 1280: 25.4 vs 36.5); a tie at 320 -> 640 (16.4); it LOSES
  // where every 32-row workgroup re-reads a wide B (320 -> 1280: 30.0 vs 22.4, its transpose 27.3 vs 21.3: 196 MB of plane
  // traffic) and on the grouped 4 x (160 -> 160) products (15.5 vs 13.5).  Rule: un-grouped, at most 640 output columns.
  // The caller's `flags` (GKG_X6_NO_KS / GKG_X6_FORCE_KS: measurement, tests) override the rule per call.
  // (X6_BNBWD comes here with a workspace only from gkg_linear_dgrad_x6_bnbwd_sk, which wants the body — and so the bits of dx —
  // that X6_STORE takes for the same shape.  64-row tiles — half the plane traffic, one wave per SIMD — measured no better on the
  // long contractions they were built for: 2 560 x 1280 -> 320 26.8 vs 24.3 us; what bounds those launches is the wave-serial K
  // loop, not the B planes.)
  if (epi != X6_STORE_NCHW && x6_ks_form(M, N, nb, q.has_ws, q.flags)) {
    p->body = X6_BODY_KS; p->NI = 2; p->BN = 64;
    p->mtiles = (M + 31) / 32; p->ntiles = (N + 63) / 64;
    p->grid_x = (unsigned)((p->mtiles + 7) / 8 * 8 * p->ntiles); p->grid_y = (unsigned)nb;
    p->lds = X6_KS_LDS;
    return;
  }
  // Few rows under a long contraction (the label branch: 2 560 x 1280 -> 320 is 100 workgroups of 40 K-steps on 256 CUs): the
  // contraction is cut into ksplit ranges so that the launch fills the chip's 512 workgroup slots, at least 4 K-steps each
  // (the pipeline's fill is worth about two).  The last arrival per tile sums the partials in split order (deterministic) and
  // runs the normal epilogue, BN statistics included.
  const long long base2 = (long long)((M + 127) / 128) * ((N + 63) / 64) * nb;
  const int nk_total = (K + 31) / 32;
  if (const int ks = x6_tile_ksplit(base2, nk_total, q.has_ws && q.ws_bytes >= X6_SK_BYTES); ks >= 2) {
    p->kper = (nk_total + ks - 1) / ks;
    p->ksplit = (nk_total + p->kper - 1) / p->kper;            // no empty range
    return tile(2, 64);
  }
  // Column-tile width (32 NI).  More columns per wave amortise the 44-instruction A split over more MFMAs (NI = 1 is
  // VALU-bound, NI = 2 about balanced) but leave fewer workgroups: NI = 2, and NI = 1 when that leaves the chip under-filled
  // (few rows: the label branch).  Measured cold-cache per shape with tools/bench_x6.py; NI = 5 (160 columns, one
  // workgroup per CU) was tried and is slower everywhere (cfg2 fc1 25.8 vs 22.9 us).
  if (base2 < 160 && !(q.flags & GKG_X6_FORCE_WALK)) return tile(1, 32);       // (the walk form exists for 64-column tiles: same bits)
  // 80 output columns on many rows (GKGNet-576 stage 1): ONE 80-column tile per row block instead of a full and a quarter
  // 64-column tile — 663 552 rows: 80 -> 80 171 -> 133 us, + statistics 208 -> 161, 320 -> 80 345 -> 279, dgrad 320 <- 80
  // 351 -> 279.  Wider outputs measured equal or slower on 80-column tiles (160: +-3 %, 320 / 400 / 640: 3-8 % slower:
  // profiles/r04_x6_80_column_tiles_ab.txt); the BN-backward epilogue's registers do not fit two waves per SIMD there.
  // Round 9 tried them for the grouped 4 x (160 -> 160) products of cfg2 (10 368 rows: 648 workgroups instead of 972, fewer
  // rounds of 512): the replayed step got 3-4 us SLOWER (profiles/r09_dgrad_stats_ab.txt) — not taken.
  if (N == 80 && (epi == X6_STORE || epi == X6_BNSTATS)) return tile(3, 80);
  tile(2, 64);
  // Two rounds of resident workgroups: the tile-walk form of the same kernel (x6_walk_grid; GKG_X6_NO_WALK / _FORCE_WALK).  Not with
  // the BN-backward statistics epilogue: its registers (the y prefetch beside the walk's state) leave the compiler 219 VGPRs and 69
  // spilled SGPRs for two waves per SIMD, and cfg2's 810-tile launch measured 44.0 -> 47.8 us walking — the flags do nothing there.
  if (epi == X6_BNBWD || (q.flags & GKG_X6_NO_WALK)) return;
  p->walkable = true;
  p->walk_lds = p->lds + (size_t)x6_walk_epi_bytes(epi == X6_BNSTATS, 64);
  if (q.slots <= 0) return;
  if (const int grid = x6_walk_grid((long long)nb * p->mtiles, p->ntiles, 1, q.slots, q.flags); grid > 0) {
    p->body = X6_BODY_WALK; p->grid_x = (unsigned)grid; p->grid_y = 1;
    p->lds = p->walk_lds;
  }
}

// The rejections of the four entry points (sizes, pitches, alignment, workspace), then the ladder.
inline int x6_gemm_plan(const X6GemmCall& q, X6GemmPlan* p, const char** msg) {
  auto fail = [&](int code, const char* m) { *msg = m; return code; };
  const bool bad_ws = q.has_ws && (q.ws_bytes < X6_SK_BYTES || !q.ws_aligned);
  const bool bad_a = q.lda < q.K || (q.lda & 3) || !q.a_aligned;
  const bool big = (size_t)q.M * q.lda * 4 > 0xffffffffull;
  switch (q.role) {
    case X6R_FWD:
      if (bad_ws) return fail(GKG_ERR_SHAPE, "gkg_linear_bn_fwd_x6_sk: need a 16-byte aligned workspace of gkg_x6_splitk_workspace_bytes() bytes (or NULL: no split)");
      if (q.M <= 0 || x6_bad_dim(q.K) || x6_bad_dim(q.N) || q.nb <= 0 || q.nb > 64 || bad_a || (q.a_bstride & 3))
        return fail(GKG_ERR_SHAPE, "gkg_linear_bn_fwd_x6: need R > 0, cin % 4 == 0, cout % 4 == 0, 1 <= nb <= 64, 16-byte aligned rows");
      if (big) return fail(GKG_ERR_UNSUPPORTED, "gkg_linear_bn_fwd_x6: operand larger than 4 GiB per batch");
      if (q.train && (size_t)q.nb * 2 * q.N > (size_t)X6_STATS_DOUBLES) return fail(GKG_ERR_UNSUPPORTED, "gkg_linear_bn_fwd_x6: nb * cout too large for the stats scratch");
      break;
    case X6R_DGRAD_NCHW:
      if (q.nchw_b <= 0 || q.nchw_n <= 0 || (long long)q.nchw_b * q.nchw_n != q.M) return fail(GKG_ERR_SHAPE, "gkg_linear_dgrad_x6_nchw: R == B * N");
      if (bad_ws) return fail(GKG_ERR_SHAPE, "gkg_linear_dgrad_x6_nchw: need a 16-byte aligned workspace of gkg_x6_splitk_workspace_bytes() bytes (or NULL: no split)");
      if (x6_nchw_two_launch(q)) {
        X6GemmCall d = q;                        // gkg_linear_dgrad_x6_sk into the token-major scratch, its own rejections
        d.role = X6R_DGRAD; d.ldc = 0; d.a_bstride = (size_t)q.M * q.K;
        const int rc = x6_gemm_plan(d, p, msg);
        p->two_launch = true;
        return rc;
      }
      if (q.M <= 0 || x6_bad_dim(q.N) || x6_bad_dim(q.K) || bad_a)
        return fail(GKG_ERR_SHAPE, "gkg_linear_dgrad_x6_nchw: need R > 0, cin % 4 == 0, cout % 4 == 0, 16-byte aligned rows");
      if (big) return fail(GKG_ERR_UNSUPPORTED, "gkg_linear_dgrad_x6_nchw: operand larger than 4 GiB");
      break;
    case X6R_DGRAD: {
      if (bad_ws) return fail(GKG_ERR_SHAPE, "gkg_linear_dgrad_x6_sk: need a 16-byte aligned workspace of gkg_x6_splitk_workspace_bytes() bytes (or NULL: no split)");
      const int ldc = q.ldc ? q.ldc : q.N;             // contiguous: the pitch is the width
      if (ldc < q.N || (ldc & 3) || (q.ldc && (q.c_bstride & 3))) return fail(GKG_ERR_SHAPE, "gkg_linear_dgrad_x6: bad dx pitch / batch stride");
      if (q.M <= 0 || x6_bad_dim(q.N) || x6_bad_dim(q.K) || q.nb <= 0 || q.nb > 64 || bad_a || (q.a_bstride & 3))
        return fail(GKG_ERR_SHAPE, "gkg_linear_dgrad_x6: need R > 0, cin % 4 == 0, cout % 4 == 0, 1 <= nb <= 64, 16-byte aligned rows");
      if (big) return fail(GKG_ERR_UNSUPPORTED, "gkg_linear_dgrad_x6: operand larger than 4 GiB per batch");
      break;
    }
    case X6R_DGRAD_BNBWD:
      if (bad_ws) return fail(GKG_ERR_SHAPE, "gkg_linear_dgrad_x6_bnbwd_sk: need a 16-byte aligned workspace of gkg_x6_splitk_workspace_bytes() bytes (or NULL: no split)");
      if (q.M <= 0 || x6_bad_dim(q.N) || x6_bad_dim(q.K) || bad_a || q.pnb <= 0 || q.pco <= 0 || (long long)q.pnb * q.pco != q.N ||
          (q.pact != 0 && q.pact != 1))
        return fail(GKG_ERR_SHAPE, "gkg_linear_dgrad_x6_bnbwd_sk: need R > 0, cin % 4 == 0, cout % 4 == 0, cin == pnb * pco, 16-byte aligned rows");
      if (big) return fail(GKG_ERR_UNSUPPORTED, "gkg_linear_dgrad_x6_bnbwd_sk: operand larger than 4 GiB");
      if (q.has_residual && !x6_bnbwd_takes_residual(q.M, q.N, q.has_ws, q.flags))
        return fail(GKG_ERR_UNSUPPORTED, "gkg_linear_dgrad_x6_bnbwd_sk: a residual needs the short-matrix body");
      break;
  }
  x6_gemm_ladder(q, p);
  return 0;
}

// ------------------------------------------------------------------------------------------ weight gradients
// dW (nb, cout, cin) = dY^T X over R rows.  Whole 128-row units go through an LDS-DMA kernel (64 x 64 tiles, or 64 x 128: `wide`)
// when the rows are 16-byte aligned; the ragged rest (and everything, when they are not) through the register-load kernel.
struct X6WgradCall {
  int R, cin, cout, nb;
  int ldg, ldx; size_t g_bstride, x_bstride;     // pitches / batch strides of dY and X (floats)
  bool aligned;                    // dY and X are 16-byte aligned pointers: the entry points look, the host-side queries pass the caller's word
  int batched;                     // > 0: the launch shares the chip with other problems (gkg_linear_wgrad_x6_batch) — slabs of
                                   // ~`batched` units whatever the tile count, few-slab problems spread over the XCDs by tiles
  int kperm;
  int force_slabs;                 // > 0 (gkg_linear_wgrad_x6_det): the caller's slab count, cut to the number of units
};

struct X6WgradPart {               // one launch: the size fields of its X6WgradArgs
  int rows, row0;                  // rows [row0, row0 + rows) of the operands; rows == 0: no launch
  int M, N;                        // the kernel's A / B widths (exchanged when the plan swaps)
  int mtiles, ntiles, splits, rows_per_split;
  int share, ubase, urem;          // LDS-DMA launch: x6w_map's tile sharing, slab s = ubase + (s < urem) units
  int grid_x;                      // workgroups per group (grid.y = nb)
};

struct X6WgradPlan {
  bool wide, swap;                 // 64 x 128 tiles; the 128-wide side is cout (operand roles exchanged, dW written transposed)
  X6WgradPart main, rest;          // LDS-DMA launch over the whole units, register-load launch over the remainder
  int kperm;
  // the deterministic form's slab images: main launch's slabs first, then the remainder's, both in ascending row order
  int main_slabs() const { return main.rows > 0 ? main.splits : 0; }
  int slabs() const { return main_slabs() + (rest.rows > 0 ? rest.splits : 0); }
  void slab_rows(int s, int* first_row, int* rows) const {
    if (s < main_slabs()) {
      *first_row = 128 * (s * main.ubase + (s < main.urem ? s : main.urem));
      *rows = 128 * (main.ubase + (s < main.urem ? 1 : 0));
    } else {
      const int off = (s - main_slabs()) * rest.rows_per_split, left = rest.rows - off;
      *first_row = rest.row0 + off;
      *rows = left < rest.rows_per_split ? left : rest.rows_per_split;
    }
  }
};

// elements of dw = floats of one slab image; the deterministic reduction's grid is counted in ints
inline bool x6_wdet_elems_ok(int cin, int cout, int nb) {
  return cin > 0 && cout > 0 && nb > 0 && (unsigned long long)nb * (unsigned long long)cout * (unsigned long long)cin <= (1ull << 31);
}

// The stand-alone slab rule: the slab count that minimises rounds x (units per slab + fixed cost) over an XCD's 32 CUs.  One
// workgroup per CU fits (128 / 144 KiB of LDS rings) and slab s runs with all its tiles on XCD s % 8 (its rows are fetched into
// that L2 once), so an XCD's 32 CUs work in rounds over tiles x ceil(slabs / 8) workgroups; the fixed cost (ring fill, LDS
// reduction, the tile's atomics) is worth about 6 units of streaming.  (Counting rounds over the whole chip instead put 36
// workgroups on two XCDs at 6 tiles x 42 slabs: 245 -> 393 us at 663 552 x 160 -> 80.)
inline int x6_wgrad_slabs_alone(int tiles, int units) {
  int sp_alone = 1;
  long long best = -1;
  for (int sp = 1; sp <= units && sp <= 4096; ++sp) {
    const long long per_xcd = (long long)tiles * ((sp + 7) / 8);
    const long long rounds = (per_xcd + 31) / 32;
    const long long cost = rounds * ((units + sp - 1) / sp + 6);
    if (best < 0 || cost < best) { best = cost; sp_alone = sp; }
  }
  return sp_alone;
}
// A problem that fills the chip on its own (GKGNet-576's stage-1 / stage-2 weight gradients: thousands of 128-row units) keeps its
// stand-alone slabs inside a batch too — ~20-unit slabs doubled its workgroup count (cfg4: 12.6 -> 13.3 ms of weight gradients per step)
inline bool x6_wgrad_fills_chip(int tiles, int sp_alone) { return (long long)tiles * sp_alone >= 512; }

inline int x6_wgrad_plan(const X6WgradCall& q, X6WgradPlan* pl, const char** msg) {
  auto fail = [&](int code, const char* m) { *msg = m; return code; };
  const int R = q.R, cin = q.cin, cout = q.cout, nb = q.nb, ldg = q.ldg, ldx = q.ldx;
  if (q.kperm && (cin & 1)) return fail(GKG_ERR_SHAPE, "gkg_linear_wgrad_x6: kperm needs an even cin");
  if (R <= 0 || cin <= 0 || cout <= 0 || nb <= 0 || nb > 64 || ldg < cout || ldx < cin)
    return fail(GKG_ERR_SHAPE, "gkg_linear_wgrad_x6: need R, cin, cout > 0, 1 <= nb <= 64, pitches >= widths");
  if ((size_t)ldg * 4 * 16 > 0x7fffffffull || (size_t)ldx * 4 * 16 > 0x7fffffffull) return fail(GKG_ERR_UNSUPPORTED, "gkg_linear_wgrad_x6: row pitch too large");
  *pl = X6WgradPlan{};
  pl->kperm = q.kperm ? 1 : 0;
  const int mtiles = (cout + 63) / 64, ntiles = (cin + 63) / 64;
  const bool aligned = (cin & 3) == 0 && (cout & 3) == 0 && (ldg & 3) == 0 && (ldx & 3) == 0 && q.aligned && (q.g_bstride & 3) == 0 &&
                       (q.x_bstride & 3) == 0 && (size_t)R * ldg * 4 < 0xffffffffull && (size_t)R * ldx * 4 < 0xffffffffull;
  // 64 x 128 tiles (wgrad_x6_wide_kernel) when one of the two widths pads to 128 at no more than a tenth of extra work
  // (measured in the cfg2 step, wide vs 64 x 64: 640 -> 320 42.6 -> 35.6 us, 1280 -> 320 37.9 -> 30.9, but 320 -> 320 at
  // 20 % padding 22.3 -> 24.3); the 128-wide side is cin, or — roles of the operands exchanged, dW written transposed — cout
  const int nwide = (cin + 127) / 128, mwide = (cout + 127) / 128;
  const long long padn = (long long)nwide * 128 * 100 / ((long long)ntiles * 64);
  const long long padm = (long long)mwide * 128 * 100 / ((long long)mtiles * 64);
  bool wide = aligned && (padn <= 110 || padm <= 110);
  bool swap = wide && padm < padn;
  int batched = q.batched;
  if (batched > 0 && aligned) {
    // inside a batched launch the tile count of ONE problem no longer decides how well the chip is filled, only the matrix
    // time does: per MFMA the 64 x 64 loop carries 7.7 vector instructions and the 64 x 128 loop 5.8 (compiled counts, at the
    // bodies), so a 64 x 64 tile (24 MFMAs per step) is charged 36 and a wide tile 48 — padding up to 128 pays until it costs
    // that much (160 x 160: 3 x 2 wide tiles against 3 x 3; 320 x 320: 5 x 3 against 5 x 5)
    const long long c64 = (long long)mtiles * ntiles * 36;
    const long long cwn = (long long)mtiles * nwide * 48, cwm = (long long)ntiles * mwide * 48;
    wide = (cwn < cwm ? cwn : cwm) <= c64;
    swap = wide && cwm < cwn;
  }
  const int main_mtiles = swap ? ntiles : mtiles;
  const int main_ntiles = !wide ? ntiles : (swap ? mwide : nwide);
  const int tiles = main_mtiles * main_ntiles * nb, units = R / 128;
  const int sp_alone = x6_wgrad_slabs_alone(tiles, units);
  if (batched && x6_wgrad_fills_chip(tiles, sp_alone)) batched = 0;
  int splits = 1, share = 0;
  if (batched) {
    // ~`batched` (default 20) units of 128 rows per workgroup (its fixed cost — ring fill, LDS reduction, the tile's atomics — is
    // worth about 6): 1 / 2 / 4 slabs shared by 8 / 4 / 2 XCDs each, or a multiple of 8 slabs on one XCD each
    const int want = (units + batched - 1) / batched;
    if (want <= 1) splits = 1;
    else if (want <= 2) splits = 2;
    else if (want <= 5) splits = 4;
    else splits = (want + 7) / 8 * 8;
    if (splits > units) splits = units > 0 ? units : 1;
    if (splits < 8) { while (8 % splits) --splits; share = 8 / splits; }
  } else {
    splits = q.force_slabs > 0 ? q.force_slabs : sp_alone;       // slabs of whole 128-row units (4 waves x 2 steps x 16 rows)
  }
  const int rows_per_split = units > 0 ? (units + splits - 1) / splits * 128 : 128;
  pl->wide = wide; pl->swap = swap;
  const int main_rows = aligned ? units * 128 : 0;
  if (main_rows > 0) {
    X6WgradPart& m = pl->main;
    m.rows = main_rows; m.rows_per_split = rows_per_split;
    m.M = swap ? cin : cout; m.N = swap ? cout : cin;     // swap: the kernel's "A" (64-wide side) is x, its "B" (128-wide side) dy
    m.mtiles = main_mtiles; m.ntiles = main_ntiles;
    m.splits = splits < units ? splits : units;
    m.ubase = units / m.splits; m.urem = units % m.splits;
    if (share > 1 && m.splits * share == 8) {
      m.share = share;
      m.grid_x = (m.mtiles * m.ntiles + share - 1) / share * 8;
    } else {
      m.grid_x = (m.splits + 7) / 8 * 8 * m.mtiles * m.ntiles;
    }
  }
  if (const int rest = R - main_rows; rest > 0) {
    X6WgradPart& t = pl->rest;
    t.rows = rest; t.row0 = main_rows;
    t.M = cout; t.N = cin; t.mtiles = mtiles; t.ntiles = ntiles;
    const int tunits = (rest + 127) / 128, ts = splits > tunits ? tunits : splits;
    t.rows_per_split = (tunits + ts - 1) / ts * 128;
    t.splits = (rest + t.rows_per_split - 1) / t.rows_per_split;
    t.grid_x = (t.splits + 7) / 8 * 8 * mtiles * ntiles;
  }
  return 0;
}

// gkg_linear_wgrad_x6_det_workspace_bytes: slab images of the larger of the aligned and the unaligned plan (0: the call is rejected)
inline int x6_wdet_max_slabs(int R, int cin, int cout, int nb, int ldg, int ldx, int force_slabs, int* rc, const char** msg) {
  int S = 0;
  for (int al = 0; al < 2; ++al) {
    X6WgradPlan pl;
    if ((*rc = x6_wgrad_plan(X6WgradCall{R, cin, cout, nb, ldg, ldx, 0, 0, al != 0, 0, 0, force_slabs}, &pl, msg))) return 0;
    if (pl.slabs() > S) S = pl.slabs();
  }
  return S;
}

// The weight gradients of n layers in one launch per X6W_BATCH problems (+ the ragged remainders' own launches): the argument
// checks, the launch order (largest problems first: the tail of the launch is made of the short ones), every problem's plan, its
// place in its launch group and, `det`, the floats of slab images the deterministic form needs.
struct X6WgradBatchPlan {
  int n;
  int order[X6W_MAX_PROBLEMS];     // launch position -> index into the caller's array; everything below is indexed by launch position
  X6WgradPlan pl[X6W_MAX_PROBLEMS];
  int slot[X6W_MAX_PROBLEMS];      // place in its launch group (X6WgradBatch::p[slot]); -1: no whole units, nothing in a group
  int rot[X6W_MAX_PROBLEMS];       // the XCD rotation of its workgroups (consecutive problems start on different XCDs)
  int end[X6W_MAX_PROBLEMS];       // X6WgradBatch::begin[slot + 1]: the group's workgroups up to and including this problem
  size_t det_floats;
};

inline int x6_wgrad_batch_plan(const GkgWgradProblem* p, int n, int units_per_slab, bool det, X6WgradBatchPlan* bp, const char** msg) {
  auto fail = [&](int code, const char* m) { *msg = m; return code; };
  if (!p || n <= 0) return fail(GKG_ERR_NULL, det ? "gkg_linear_wgrad_x6_batch_det: no problems" : "gkg_linear_wgrad_x6_batch: no problems");
  if (units_per_slab < 0 || units_per_slab > 4096)
    return fail(GKG_ERR_SHAPE, det ? "gkg_linear_wgrad_x6_batch_det: units_per_slab out of range" : "gkg_linear_wgrad_x6_batch: units_per_slab out of range");
  if (n > X6W_MAX_PROBLEMS)
    return fail(GKG_ERR_SHAPE, det ? "gkg_linear_wgrad_x6_batch_det: at most 256 problems per call" : "gkg_linear_wgrad_x6_batch: at most 256 problems per call");
  if (units_per_slab == 0) units_per_slab = 20;
  int* order = bp->order;
  for (int i = 0; i < n; ++i) order[i] = i;
  auto work = [&](int i) { return (double)p[i].R * p[i].cin * p[i].cout * p[i].nb; };
  for (int i = 1; i < n; ++i)                     // insertion sort, descending work
    for (int j = i; j > 0 && work(order[j]) > work(order[j - 1]); --j) { const int t = order[j]; order[j] = order[j - 1]; order[j - 1] = t; }
  bp->n = n;
  bp->det_floats = 0;
  int rot = 0, open = 0, begin = 0;                // problems and workgroups of the open group
  for (int oi = 0; oi < n; ++oi) {
    const GkgWgradProblem& q = p[order[oi]];
    if (!q.dy || !q.x || !q.dw) return fail(GKG_ERR_NULL, "gkg_linear_wgrad_x6: null pointer");
    X6WgradPlan& pl = bp->pl[oi];
    const int rc = x6_wgrad_plan(X6WgradCall{q.R, q.cin, q.cout, q.nb, q.ldg, q.ldx, q.g_bstride, q.x_bstride,
                                             (((size_t)q.dy | (size_t)q.x) & 15) == 0, units_per_slab, q.kperm, 0}, &pl, msg);
    if (rc) return rc;
    if (det && !x6_wdet_elems_ok(q.cin, q.cout, q.nb)) return fail(GKG_ERR_UNSUPPORTED, "gkg_linear_wgrad_x6_batch_det: more than 2^31 elements of a dw");
    bp->det_floats += (size_t)pl.slabs() * q.nb * q.cout * q.cin;
    bp->slot[oi] = -1;
    if (pl.main.rows > 0) {
      bp->slot[oi] = open;
      bp->rot[oi] = rot;
      rot = (rot + (pl.main.share > 1 ? 0 : pl.main.splits)) & 7;
      bp->end[oi] = begin += pl.main.grid_x * q.nb;
      if (++open == X6W_BATCH) open = begin = 0;
    }
  }
  return 0;
}

}  // namespace gkg
