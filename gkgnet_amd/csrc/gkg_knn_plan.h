// gkg_knn_plan.h — the k-NN's launch plan: everything a call decides from its sizes, flags and role, as pure host code (no HIP
// header, nothing __device__: tests/knn_plan/plan_dump.cpp is built by a plain C++17 compiler).  The entry points (gkg_knn.hip) fill a
// KnnCall, knn_plan turns it into a KnnPlan, the launch sequence and the per-unit launchers only read that plan.  A producer that
// prepares tokens for a later call plans the SAME problem under its own role (tests/test_knn_plan_host.py holds the two together).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "gkg_hip.h"

namespace gkg {

constexpr int QT = 64;   // queries per workgroup (one per lane)
constexpr int KT = 32;   // keys per MFMA tile
constexpr int NW = 4;    // waves per workgroup
constexpr uint32_t IDX_BITS = 0x1fffffffu;          // 29 bits: key index < 2^29 (gkg_knn_common.h: top-KD list)
constexpr int KNN_BUF = 16;        // buffered selection: entries per lane (8 bytes each: 32 KB per workgroup)
constexpr int PF_EXTRA = 8;        // prefilter: survivors beyond KD a query may have before it takes the slow path
constexpr int KNN_EL_F32 = 0, KNN_EL_BF16 = 1, KNN_EL_F16 = 2;     // the contraction's element format (gkg_knn_tile.h)
// list sizes of the tile kernel: the lengths GKGNet's configurations use (k*d = 9, 18, 27; pvig_m k = 18: 18, 36) plus
// 64 to cover everything else (each instantiation is a kernel of its own); 10..18 share the 18-entry list
constexpr int kListSizes[] = {9, 18, 27, 36, 64};

enum KnnRole {
  KNN_GRAPH, KNN_FUSED,  // gkg_knn_fwd / _tm / _tm16; gkg_knn_mr_fwd_tm: the aggregation in the tile kernel's epilogue
  KNN_FUSED_PROBE,       // gkg_knn_mr_fused_supported: would KNN_FUSED run?  (0 / GKG_ERR_UNSUPPORTED, no message)
  KNN_PRODUCE_QUERIES, KNN_PRODUCE_KEYS,   // gkg_bn_apply_knn_prep / gkg_affine_knn_prep: PREPARATION ONLY of one operand for the call that
                                           // follows with GKG_KNN_X_PREPARED (_Y_PREPARED) — that call up to its preparation launch
  KNN_QUERY_PREP_PLAN    // knn_query_prep_plan: a queries producer that runs the preparation inside a kernel of its own
};

struct KnnCall {
  int BG, G_tm;          // problems; G_tm > 0: token-major (B, T, C = G_tm c) input, 0: channel-major (BG, c, T)
  int c, N, M, k, dilation, dtype;
  unsigned flags; bool has_y, has_relpos;
  int ldx, xchunk;       // x as a view (token-major fp32 callers): row pitch in floats (0: G_tm c), chunk (gkg_common.h "XM layout")
  KnnRole role; bool consumer_fused;     // producer roles: the call that follows is KNN_FUSED
};

struct KnnPlan {
  int kd, KD, S, tps, nqt, cp16, cp16p, Nr, Mr;
  int cpad_ws, cpad;     // channel padding the workspace was budgeted with (multiple of 8) / the launches use (<= cpad_ws)
  size_t off_xh, off_yh, off_sqx, off_sqy, off_pv, off_pi, off_xp, off_yp, off_flags, total;
  int ldx, el; bool norm;                // the x view's row pitch, resolved; KNN_EL_*; normalised tokens
  bool pf; float margin; // prefilter launch in front of the tile kernel (which then is its clean-up pass), 2 * eps
  int ku; bool guard; int buf, waves; bool mrf;        // tile form: knn_tile_kernel<KD, rp, ku, guard, buf, el, waves, mrf>
  int pf_kdw, pf_buf; bool pf_sb;                      // prefilter form: knn_pf_kernel<KD, pf_kdw, rp, pf_buf, pf_sb>
  size_t lds_tile, lds_pf;                             // dynamic LDS bytes of the two launches
  unsigned grid_x; int rp_major, rp_group;             // workgroup map (gkg_knn_common.h knn_map); grid = (grid_x, 1, S)
  bool prep_x, prep_y;   // operand sets this call's own preparation launch covers
};

// ------------------------------------------------------------------------------------------ LDS
constexpr size_t knn_cand_bytes(int entries, int waves) { return (size_t)entries * 64 * waves * 8; }   // candidate buffer (float2 per lane)
constexpr size_t knn_bound_bytes(int waves) { return (size_t)waves * 64 * sizeof(float); }               // shared admission bounds
// staged query tile: fp32 [cpad][64], or (16-bit forms) 64 rows of cp16 + 8 elements
constexpr size_t knn_tile_query_bytes(int el, int cpad, int cp16) { return el ? (size_t)QT * (cp16 + 8) * 2 : (size_t)cpad * QT * sizeof(float); }
// the streaming phase: queries + candidate buffer + the per-wave shared admission bounds behind them
constexpr size_t knn_tile_lds_stream(int el, int cpad, int cp16, int buf, int waves) {
  return knn_tile_query_bytes(el, cpad, cp16) + (buf > 0 ? knn_cand_bytes(buf, waves) + knn_bound_bytes(waves) : 0);
}
// the tile kernel's dynamic LDS: the streaming phase, the merge area of the per-wave lists (none for one wave) and, fused
// aggregation, the final lists of the 64 queries behind the merge area
constexpr size_t knn_tile_lds(int KD, int el, int cpad, int cp16, int buf, int waves, bool mrf, int k) {
  size_t lds = knn_tile_lds_stream(el, cpad, cp16, buf, waves);
  const size_t merge = waves == 1 ? 0 : (size_t)waves * KD * 64 * 2 * sizeof(float);
  if (lds < merge) lds = merge;
  if (mrf && lds < merge + (size_t)k * 64 * sizeof(int)) lds = merge + (size_t)k * 64 * sizeof(int);
  return lds;
}
constexpr size_t knn_pf_stage_bytes(int cp16p) { return (size_t)2 * QT * (cp16p + 8) * 2; }     // hi + lo query planes
// the prefilter kernel's dynamic LDS: staged planes + candidate buffer + bounds, or the lists / survivors of its epilogue
constexpr size_t knn_pf_lds(int KD, int KDW, int cp16p, int pbuf) {
  const size_t lists = (size_t)2 * NW * KDW * 64 * 4 + (size_t)(KD + PF_EXTRA) * 64 * (4 + 2) + 64 * 4 + 16;
  const size_t need = knn_pf_stage_bytes(cp16p) + knn_cand_bytes(pbuf, NW) + (pbuf ? knn_bound_bytes(NW) : 0);
  return need > lists ? need : lists;
}

// ------------------------------------------------------------------------------------------ sizes
inline int knn_pick_splits(int BG, int N, int M) {
  const int qtiles = (N + QT - 1) / QT;
  const int ktiles = (M + KT - 1) / KT;
  const long wgs = (long)qtiles * BG;
  int S = 1;
  if (wgs < 256) {                                 // fewer workgroups than CUs: split the keys
    S = (int)((512 + wgs - 1) / wgs);
    const int smax = (ktiles + 7) / 8;          // keep >= 8 key tiles (2 per wave) per split
    if (S > smax) S = smax;
    if (S < 1) S = 1;
    if (S > 64) S = 64;
  }
  return S;
}

// sizes, list size, key splits and the workspace layout (has_y: the keys' slots are budgeted)
inline int knn_plan_sizes(int BG, int c, int N, int M, int k, int dilation, bool has_y, KnnPlan* p) {
  if (BG <= 0 || c <= 0 || N <= 0 || M <= 0 || k <= 0 || dilation <= 0) return GKG_ERR_SHAPE;
  if ((long)k * dilation > M) return GKG_ERR_SHAPE;
  if (!has_y && M != N) return GKG_ERR_SHAPE;
  p->cpad_ws = p->cpad = (c + 7) & ~7;          // zero-padded channels: fma(0,0,acc) == acc keeps the chain exact
  p->kd = k * dilation; p->KD = -1;
  for (int i = 4; i >= 0; --i) if (kListSizes[i] >= p->kd) p->KD = kListSizes[i];      // the first that holds k d
  if (p->KD < 0) return GKG_ERR_UNSUPPORTED;
  if ((size_t)p->cpad * QT * sizeof(float) > 150 * 1024) return GKG_ERR_UNSUPPORTED;   // c <= 600
  if (BG > 65535) return GKG_ERR_UNSUPPORTED;           // token_prep uses grid.y = BG
  if ((long)M + KT > (long)IDX_BITS) return GKG_ERR_UNSUPPORTED;   // key indices live in 29 bits of the list keys
  p->S = knn_pick_splits(BG, N, M);
  const int ktiles = (M + KT - 1) / KT;
  p->tps = (ktiles + p->S - 1) / p->S;
  p->S = (ktiles + p->tps - 1) / p->tps;
  p->nqt = (N + QT - 1) / QT;
  p->cp16 = (c + 15) & ~15;
  p->cp16p = (c + 2 + 15) & ~15;            // prefilter planes: + the two |th|^2 channels (see PrepSet)
  p->Nr = (N + 31) & ~31; p->Mr = (M + 31) & ~31;
  auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
  size_t o = 0;
  p->off_xh = o; o = al(o + sizeof(float) * (size_t)BG * p->cpad * N);
  p->off_sqx = o; o = al(o + sizeof(float) * ((size_t)BG * N + 32));
  if (has_y) {
    p->off_yh = o; o = al(o + sizeof(float) * (size_t)BG * p->cpad * M);
    p->off_sqy = o; o = al(o + sizeof(float) * ((size_t)BG * M + 32));
  } else {
    p->off_yh = p->off_xh; p->off_sqy = p->off_sqx;
  }
  if (p->S > 1) {
    p->off_pv = o; o = al(o + sizeof(float) * (size_t)p->S * BG * N * p->kd);
    p->off_pi = o; o = al(o + sizeof(int) * (size_t)p->S * BG * N * p->kd);
    p->off_xp = p->off_yp = p->off_flags = 0;
  } else {
    p->off_pv = p->off_pi = 0;
    // prefilter mode (un-split problems): bf16 hi + lo planes (BG, T, cp16p) of the queries and keys
    p->off_xp = o; o = al(o + 2 * sizeof(uint16_t) * (size_t)BG * p->Nr * p->cp16p);
    if (has_y) { p->off_yp = o; o = al(o + 2 * sizeof(uint16_t) * (size_t)BG * p->Mr * p->cp16p); }
    else p->off_yp = p->off_xp;
    p->off_flags = o; o = al(o + sizeof(int) * (size_t)p->nqt * ((BG + 7) / 8) * 8);   // one per workgroup
  }
  p->total = o;
  return 0;
}

// ------------------------------------------------------------------------------------------ the plan
// 0, or a GKG_ERR_* code with the message for gkg_fail in *msg (null: the code alone — KNN_FUSED_PROBE's answer).
inline int knn_plan(const KnnCall& q, KnnPlan* plan, const char** msg) {
  KnnPlan& p = *plan;
  p = KnnPlan{};
  *msg = nullptr;
  auto fail = [&](int code, const char* m) { *msg = m; return code; };
  const unsigned flags = q.flags;
  const int c = q.c, N = q.N, M = q.M, BG = q.BG, dtype = q.dtype, G_tm = q.G_tm;
  const bool probe = q.role == KNN_FUSED_PROBE;
  const bool pq = q.role == KNN_PRODUCE_QUERIES || q.role == KNN_QUERY_PREP_PLAN, pk = q.role == KNN_PRODUCE_KEYS;
  const bool prep_only = pq || pk;
  const bool mr = q.role == KNN_FUSED || (prep_only && q.consumer_fused);      // the tile launch is (will be) the fused form
  // fp16 contraction (GKG_KNN_F16_CONTRACT): normalised tokens only (raw ones can overflow fp16), one 16-bit format per call, no
  // prepared copies, no preparing producer, not the fused k-NN + aggregation.  Rejected on the flag word, before anything else.
  const bool f16_asked = (flags & GKG_KNN_F16_CONTRACT) != 0;
  if (f16_asked) {
    if (probe) return GKG_ERR_UNSUPPORTED;
    if (!(flags & GKG_KNN_NORMALIZE)) return fail(GKG_ERR_UNSUPPORTED, "GKG_KNN_F16_CONTRACT: needs GKG_KNN_NORMALIZE");
    if (flags & GKG_KNN_BF16_CONTRACT) return fail(GKG_ERR_UNSUPPORTED, "GKG_KNN_F16_CONTRACT: not together with GKG_KNN_BF16_CONTRACT");
    if (flags & (GKG_KNN_X_PREPARED | GKG_KNN_Y_PREPARED)) return fail(GKG_ERR_UNSUPPORTED, "GKG_KNN_X/Y_PREPARED: not with the fp16 contraction");
    if (prep_only) return fail(GKG_ERR_UNSUPPORTED, "gkg_bn_apply_knn_prep: not with the fp16 contraction");
    if (mr) return fail(GKG_ERR_UNSUPPORTED, "gkg_knn_mr_fwd_tm: not with the fp16 contraction");
  }
  const bool x_prepared = (flags & GKG_KNN_X_PREPARED) != 0, y_prepared = (flags & GKG_KNN_Y_PREPARED) != 0;
  if (y_prepared && (!q.has_y || prep_only || G_tm <= 0 || dtype != GKG_F32 || (c & 3)))
    return fail(GKG_ERR_SHAPE, "GKG_KNN_Y_PREPARED: a token-major fp32 k-NN call with keys");
  if (prep_only && x_prepared) return fail(GKG_ERR_SHAPE, "gkg_bn_apply_knn_prep: GKG_KNN_X_PREPARED makes no sense here");
  if ((prep_only || x_prepared) && (G_tm <= 0 || dtype != GKG_F32 || (c & 3)))
    return fail(GKG_ERR_UNSUPPORTED, "prepared queries: token-major fp32 callers with c % 4 == 0 only");
  // ldx / xchunk (token-major fp32 callers, G_tm > 0): x as a view — row pitch ldx floats (0: G_tm * c), chunk xchunk
  // (gkg_common.h "XM layout": xchunk = C / 4 with ldx = 2 C is the x half of the grouped projection's operand buffer)
  int ldx = q.ldx, xchunk = q.xchunk;
  if (G_tm > 0) {
    const int C = G_tm * c;
    if (ldx == 0) ldx = C;
    if (ldx < C || xchunk < 0 || (xchunk > 0 && (dtype != GKG_F32 || (xchunk & 3) || (c & 3) || (ldx & 3) || C % xchunk || ldx < 2 * C)))
      return fail(GKG_ERR_SHAPE, "gkg_knn_fwd_tm: bad x view (ldx >= C; a chunk needs fp32, c % 4 == 0, chunk % 4 == 0, chunk | C, ldx >= 2 C)");
  } else if (ldx != 0 || xchunk != 0) {
    return fail(GKG_ERR_SHAPE, "gkg_knn_fwd: x views are a token-major feature");
  }
  if (dtype != GKG_F32 && dtype != GKG_BF16 && dtype != GKG_F16) return fail(GKG_ERR_UNSUPPORTED, "gkg_knn_fwd: dtype must be GKG_F32, GKG_BF16 or GKG_F16");
  const int rc = knn_plan_sizes(BG, c, N, M, q.k, q.dilation, q.has_y, &p);
  if (rc == GKG_ERR_SHAPE) return fail(rc, "gkg_knn_fwd: bad sizes (need >0, k*dilation <= M, M == N for the self graph)");
  if (rc != 0) return fail(rc, "gkg_knn_fwd: unsupported size (k*dilation <= 64, c <= 600, BG <= 65535)");
  p.ldx = ldx;
  p.norm = (flags & GKG_KNN_NORMALIZE) != 0;
  // bf16 contraction: the normalised copies are bf16 octet-major planes (they fit the fp32 copies' workspace slots); needs
  // c >= 9, i.e. cpad >= 16 (below that the fp32 staging area, which sizes the LDS, is smaller than the bf16 one) —
  // otherwise the flag is ignored
  // (fp16 contraction: fp16 planes of the same size in the same slots, the same launch plan; `bf` covers both 16-bit formats)
  const bool hf = f16_asked && p.cpad >= 16;
  const bool bf = ((flags & GKG_KNN_BF16_CONTRACT) != 0 && p.cpad >= 16) || hf;
  p.el = hf ? KNN_EL_F16 : (bf ? KNN_EL_BF16 : KNN_EL_F32);
  const int cp16 = p.cp16, cp16p = p.cp16p;
  // prefilter mode: the bit-exact contract path for normalised, un-split problems with lists up to 36 entries (LDS)
  // Where it pays (MI355X, tools/bench_ops.py, prefilter vs fp32 tile kernel, us per launch incl. the extra preparation
  // work): long key streams, where the contraction dominates — pvig_s@576 stage 3 (c = 200, 1296 x 1296) k*d = 18:
  // 437 + 92 vs 594 + 57, k*d = 27: 525 + 91 vs 827 + 56; stage 2 (c = 80, 5184 x 1296, k*d = 9): 675 + 82 vs 882 + 58;
  // stage 1 (c = 40, 20736 x 1296): 2203 + 143 vs 2382 + 97.  It loses on short streams, where its serial tail (merge,
  // exact pass, final ranking in one wave) is not amortised (cfg2 label graph 34 vs 25, C = 640 / k*d = 27 at 18 x 18: 210
  // vs 119; the cfg2 Grapher graph is a tie: 51 + 22 vs 54 + 15), and against the BUFFERED selection of narrow groups with
  // long lists (pvig_m: c = 24 / k*d = 18: 4469 vs 3149).  GKG_KNN_FORCE_PREFILTER overrides the rule (tests).
  const bool pf_pays = M >= 1024 && (p.KD <= 12 ? p.cpad >= 40 : (p.KD <= 27 && p.cpad >= 128));
  // The prefilter's error bound (knn_pf_kernel, step 3) is derived for |relative_pos| <= 1.125: the bias is the initial value of
  // the accumulators, so the rounding of the accumulation scales with |bias| + 2.  A call with a bias takes the prefilter only
  // when the caller vouches for that range (GKG_KNN_RELPOS_UNIT; GKGNet's bias -2 PE PE^T / D lies in [-1, 0]) — ADVICE r3.
  const bool rp_ok = !q.has_relpos || (flags & GKG_KNN_RELPOS_UNIT);
  const bool pf = !bf && p.norm && p.S == 1 && c >= 16 && p.KD <= 36 && !(flags & GKG_KNN_NO_PREFILTER) && rp_ok
                  && knn_pf_stage_bytes(cp16p) <= 150 * 1024 && (pf_pays || (flags & GKG_KNN_FORCE_PREFILTER));
  p.pf = pf;
  const bool short_stream = p.tps < 10 * NW;
  // Selection mode.  Buffered selection (see the kernel) wins where the per-candidate insert dominates and its 32 KB
  // buffer does not cost occupancy — measured on MI355X (tools/bench_ops.py, direct -> buffered): pvig_m@768 k=18
  // stage 1 (c=12, kd=18) 15.97 -> 10.61 ms, stage 2 4.46 -> 3.13 ms, stage 3 (c=48, kd=36) 2.59 -> 1.55 ms; pvig_s@576
  // stage 1 2.52 -> 2.42 ms, stage 2 0.96 -> 0.89 ms, label graph over 20 736 keys 250 -> 214 us; it LOSES with wide groups
  // (c=200: query tile 51 KB + buffer -> one workgroup per CU, 607 -> 876 us) and on short streams with 9-entry lists
  // (cfg2 label graph 24.6 -> 31.5 us).  The GKG_KNN_SELECT_DIRECT / _BUFFERED flags override the rule (measurement / tests).
  const int force = (flags & GKG_KNN_SELECT_BUFFERED) ? 2 : ((flags & GKG_KNN_SELECT_DIRECT) ? 1 : 0);
  const size_t lds_q = knn_tile_query_bytes(KNN_EL_F32, p.cpad, cp16);
  const bool lds_ok = knn_tile_lds_stream(KNN_EL_F32, p.cpad, cp16, KNN_BUF, NW) <= 150 * 1024;
  const bool pays = p.tps >= 2 * NW && (p.tps >= 4 * NW || p.KD >= 18 || p.S > 1);      // (the 16-bit forms' rule as well)
  const bool buffered = lds_ok && (force == 2 || (force == 0 && (lds_q <= 24 * 1024 && pays)));
  // fp32 contract forms: single-wave workgroups for the narrowest groups (pvig_m stage 1: c = 12, 36 864 queries x 2 304 keys,
  // k*d = 18): one list per query instead of four quarter-stream lists — measured on the model's activations 9 045 -> 7 872 us per
  // launch; no gain at c = 24 / 48 (2 748 -> 2 761, 1 225 -> 1 238 us), where the per-wave query image costs occupancy
  const bool solo32 = buffered && !pf && p.S == 1 && (size_t)p.nqt * BG >= 2048 && lds_q <= 4 * 1024;
  // Round 5: the buffered fp32 forms also exist with 6 k-pairs per operand batch — channels padded to a multiple of 12 where
  // that is no more than the multiple of 8 (c = 9..12, 17..24, 33..36, 57..60: pvig_m's groups of 12 and 24).  The workspace is sized
  // for the wider padding (cpad_ws); cpad is only the row count / stride of the prepared copies.
  const int c12 = (c + 11) / 12 * 12;
  if (buffered && !pf && !bf && !mr && !probe && p.KD <= 36 && (c12 % 16) != 0 && (c12 < p.cpad || (c12 == p.cpad && (p.cpad % 16) != 0)))
    p.cpad = c12;
  if (mr || probe) {
    // The fused form: the fp32 tile kernel with merged per-wave lists (no key splits, no prefilter, no single-wave form), lists of at
    // most 36 entries, token-major fp32 callers
    const bool ok = !bf && dtype == GKG_F32 && G_tm > 0 && p.S == 1 && !pf && !solo32 && p.KD <= 36 && q.k <= 18 && M <= 65536 && (c & 3) == 0 &&
                    knn_tile_lds(p.KD, KNN_EL_F32, p.cpad, cp16, buffered ? KNN_BUF : 0, NW, true, q.k) <= 150 * 1024;
    if (probe) return ok ? 0 : GKG_ERR_UNSUPPORTED;
    if (!ok) return fail(GKG_ERR_UNSUPPORTED, "gkg_knn_mr_fwd_tm: this shape does not take the fused form (gkg_knn_mr_fused_supported)");
  }
  if (prep_only) {                               // ONE operand (with its BN-apply): the other belongs to its own producer / the k-NN call
    if (bf) return fail(GKG_ERR_UNSUPPORTED, "gkg_bn_apply_knn_prep: not with the bf16 contraction");
    if (pk && !q.has_y) return fail(GKG_ERR_SHAPE, "gkg_bn_apply_knn_prep: a keys producer needs a k-NN problem with keys");
    p.prep_x = q.role == KNN_PRODUCE_QUERIES; p.prep_y = pk;
  } else if (x_prepared || y_prepared) {         // copies already in place (a producer's work): only what is missing
    if (bf) return fail(GKG_ERR_UNSUPPORTED, "GKG_KNN_X/Y_PREPARED: not with the bf16 contraction");
    p.prep_x = !x_prepared; p.prep_y = q.has_y && !y_prepared;
  } else {
    p.prep_x = true; p.prep_y = q.has_y;
  }
  p.grid_x = (unsigned)(p.nqt * ((BG + 7) / 8) * 8);
  p.rp_major = 0; p.rp_group = 1;
  // bf16 / fp16 form with a positional bias at least twice the size of the keys it meets (64 x 4 B of relative_pos against
  // 2 x cp16 B of a key per (query tile, key) pair, i.e. c <= 64) and enough query tiles to spread over the XCDs: map the
  // workgroups relative_pos-major (see the kernel).  Measured (tools/bench_knn_bf.py, us): pvig_m stages 1-2 6031 -> 5101,
  // 1590 -> 1487; pvig_s stage 1 1259 -> 1187.
  if (bf && q.has_relpos && !pf && p.nqt >= 64 && BG >= 8 && (size_t)QT * 4 >= (size_t)cp16 * 2 * 2) {
    p.rp_major = 1;
    p.grid_x = (unsigned)(((p.nqt + 7) / 8) * 8 * BG);
  }
  // Exact forms (fp32 tile kernel, prefilter kernel) with a positional bias that is far beyond an L2 (>= 8 MB: GKGNet-576
  // stage 1: 107 MB, stage 2: 27 MB; pvig_m stage 1: 340 MB): problem-major order streams the WHOLE bias once per problem
  // (counters, pvig_s stage 1: 7.5 GB of L2 misses per launch at B*G = 64 — the launch ran at the speed of that stream).
  // Interleave the XCD's problems in groups whose key sets stay in the L2 (<= 2 MB): the bias is fetched once per group.
  if (q.has_relpos && p.rp_major == 0 && p.S == 1 && BG >= 16 && (size_t)N * M * 4 >= ((size_t)8 << 20)) {
    const size_t key_bytes = (size_t)M * (pf ? (size_t)cp16p * 4 : (size_t)p.cpad * 4);
    const int bpx = (BG + 7) / 8;
    int g = (int)(((size_t)2 << 20) / (key_bytes ? key_bytes : 1));
    g = g > bpx ? bpx : g;
    while (g >= 2 && bpx % g) --g;               // a divisor of the XCD's problem count: the grid (and the flag array) keep their size
    if (g >= 2) { p.rp_major = 2; p.rp_group = g; }
  }
  if (pf) {
    // eps = split terms dropped (3 * 2^-18 * 2 = 2.3e-5) + |y|^2 entering as its two leading bf16 terms (2^-17 |y|^2 <= 7.7e-6)
    // + fp32 accumulation of the 3c + 2 products and the bias on partial sums <= |bias| + 2 + |y|^2 <= 4.125 (12.4c * 2^-24) +
    // the contract's own chain (2c * 2^-24): 14.4 c u = 8.6e-7 c; margin = 2 eps
    p.margin = 2.0f * (4.0e-5f + 9.0e-7f * (float)cp16p);
    p.pf_kdw = p.KD <= 9 ? 12 : p.KD;            // KDW exceeds KD for the short list (see knn_pf_kernel)
    // buffered selection with the largest candidate buffer (16 or 12 entries per lane: 32 / 24 KiB) that keeps the
    // workgroups per CU the register budget allows (3 for lists <= 16, 2 above)
    const size_t per_wg = (size_t)160 * 1024 / (p.pf_kdw <= 16 ? 3 : 2);
    const size_t stage = knn_pf_stage_bytes(cp16p);
    p.pf_buf = stage + knn_cand_bytes(16, NW) <= per_wg ? 16 : (stage + knn_cand_bytes(12, NW) <= per_wg ? 12 : 0);
    p.pf_sb = p.pf_kdw <= 16 && q.has_relpos && cp16p <= 64;      // single-batch form (see the kernel): narrow groups
    p.lds_pf = knn_pf_lds(p.KD, p.pf_kdw, cp16p, p.pf_buf);
  }
  p.ku = 4; p.guard = true; p.buf = 0; p.waves = NW; p.mrf = false;
  if (bf) {
    // enough query tiles to fill the chip with single-wave workgroups (2+ waves per SIMD) and the keys not split: one list per query
    // (measured, bf16 form, 4 waves -> 1: pvig_s stage 1 1353 -> 1257 us, pvig_m stages 1-3 6661 -> 6051, 1697 -> 1592,
    // 801 -> 731; it loses when the per-wave query image costs occupancy: stage 2, c = 80, 458 -> 540)
    const bool solo = p.S == 1 && (size_t)p.nqt * BG >= 2048 && knn_tile_query_bytes(p.el, p.cpad, cp16) <= 8 * 1024;
    // 16-bit forms: the staged query tile is 64 x (cp16 + 8) elements — buffered selection with the largest candidate buffer (16 or
    // 12 entries per lane) that keeps the workgroups per CU the register budget allows
    const int wgs = q.has_relpos ? (p.KD <= 18 ? 3 : 2) : (p.KD <= 12 ? 4 : (p.KD <= 27 ? 3 : 2));
    const size_t per_wg = (size_t)160 * 1024 / wgs;
    int wbuf = knn_tile_lds_stream(p.el, p.cpad, cp16, 16, NW) <= per_wg ? 16 : (knn_tile_lds_stream(p.el, p.cpad, cp16, 12, NW) <= per_wg ? 12 : 0);
    if (force == 1 || (force == 0 && !pays)) wbuf = 0;
    if (force == 2 && wbuf == 0) wbuf = 12;
    // 64-entry lists: direct insert only (the buffered forms spilled to scratch)
    if (wbuf > 0 && p.KD <= 36) {
      p.guard = false;
      if (solo) {
        // 9-entry lists: 12-entry candidate buffers (flush when a lane holds more than 4) — with one short list per query the
        // fresher threshold is worth more than fuller flushes (cfg3 forward, k-NN kernels 5.08 -> 4.90 ms); longer lists keep
        // 16 (cfg5, k*d = 18 / 36: 29.8 -> 33.2 ms with 12).  Measured on the models' own activations: random tokens
        // (tools/bench_knn_bf.py) rank the two the other way round for k*d = 18.
        p.waves = 1; p.buf = p.KD <= 12 ? 12 : KNN_BUF;
      } else {
        // 9-entry lists: 12 entries per lane (fresher thresholds); longer lists: 16, or 12 where 16 would cost a workgroup per CU
        p.buf = (p.KD <= 12 || wbuf < 16) ? 12 : KNN_BUF;
      }
    }
  } else {
    // fp32 contract forms: 8 k-pairs per register batch when the channel count allows, 6 for padded widths of 12, 24, 36, 60 ...
    // in the buffered forms without aggregation (the only ones the plan pads to a multiple of 12 for), else 4
    const bool deep = (p.cpad % 16) == 0, six = !deep && (p.cpad % 12) == 0;
    p.mrf = mr;
    p.ku = deep ? 8 : 4;
    // the catch-all 64-entry list has no buffered form: its list (128 registers) + the 16-entry batch + the merge network's
    // temporaries spilled 100-400 VGPRs to scratch in every such instantiation; the guarded direct insert fits
    if (buffered && p.KD <= 36) {
      // solo32: buffered selection with ONE wave per workgroup (the wave streams all keys of its 64 queries: one list per query
      // instead of four quarter-stream lists, no merge) — launches with enough query tiles to fill the chip that way
      p.guard = false; p.buf = KNN_BUF; p.waves = solo32 ? 1 : NW;
      if (six && !mr) p.ku = 6;
    } else if (!buffered && short_stream && p.KD == 9) {
      // direct selection without the ballot guard — short key streams (< 10 key tiles per wave: the 18x18 stage, label graphs
      // over it), only for the 9-entry list: with 18 or 27 entries the insert is expensive enough that skipping it wins again
      // (measured: k*d = 27 at 18x18 is 19 % slower without the guard)
      p.guard = false;
    }
  }
  p.lds_tile = knn_tile_lds(p.KD, p.el, p.cpad, cp16, p.buf, p.waves, p.mrf, q.k);
  return 0;
}

}  // namespace gkg
