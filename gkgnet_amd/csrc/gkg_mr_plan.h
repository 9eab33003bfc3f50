// gkg_mr_plan.h — the max-relative aggregation's launch plans: everything a call decides from its sizes, flags and dtype, as pure host
// code (no HIP header, nothing __device__: tests/mr_plan/mr_plan_dump.cpp is built by a plain C++17 compiler).  The entry points
// (gkg_mr.hip) fill a call, a plan function turns it into a plan (or a GKG_ERR_* code and the message gkg_fail gets), the launchers
// only read that plan.  gkg_mr_bwd_tm_bnstats_supported is mr_bwd_tm_plan with want_stats and nothing else.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "gkg_hip.h"

namespace gkg {

constexpr int MR_LDS_BUDGET = 96 * 1024;   // bytes of LDS for source rows / accumulators

// ------------------------------------------------------------------------------------------ formulas, each once
constexpr size_t mr_i64_lds(int M, int cw) { return (size_t)M * cw * 8 + 16; }      // [M][cw] 64-bit accumulators + control words
constexpr size_t mr_f32_lds(int M, int cw) { return (size_t)M * cw * 4; }           // [M][cw] fp32 image
constexpr size_t mr_stats_floor(int nt, int cw) { return (size_t)(nt / 64) * 2 * cw * 8; }     // room for MrStat::flush
constexpr size_t mr_cm_lds(int CH, int M, int k) { return (size_t)CH * M * 4 + (size_t)k * 256 * 4; }     // channel-major: rows + index tile
constexpr bool mr_divides(int C, int c, int cw) { return C % cw == 0 && c % cw == 0; }      // a chunk stays inside a group
// one workgroup per (channel chunk, image), images padded to a multiple of 8 (XCD round-robin), and its one-launch guard
constexpr unsigned mr_chunk_grid(int C, int cw, int B) { return (unsigned)((C / cw) * ((B + 7) / 8) * 8); }
constexpr bool mr_chunk_grid_ok(int C, int cw, int B) { return (long)(C / cw) * (B + 7) < 0x7fffffffL; }
inline int mr_shmax(int N) {                 // the fixed-point forms' headroom: 38 - bits of N
  int bitsN = 0;
  while ((1 << bitsN) <= N) ++bitsN;         // N < 2^bitsN
  return 38 - bitsN;
}
inline int mr_pick_ch(int c, int M, int k) {  // channel-major: channels per workgroup, as many rows as fit beside the index tile
  long ch = ((long)MR_LDS_BUDGET - (long)mr_cm_lds(0, M, k)) / ((long)M * 4);
  if (ch > c) ch = c;
  if (ch > 64) ch = 64;
  return (int)ch;
}

// the flags word of gkg_mr_bwd_tm: two public bits and the measurement bits (tools/bench_mr_bwd.py, tools/ubench/mr_bwd_shape.py)
struct MrFlags {
  bool det, f32;         // GKG_MR_DETERMINISTIC, GKG_MR_FP32_ATOMICS
  int forced_cw;         // bits 8..15: chunk width
  int sv;                // bits 16..17: 1 streaming form, 2 its fp64-atomic variant, 3 the two-sweep kernel wherever it fits
  bool nt256, rows8;     // (sv) bits 20..21 = 2: 256 threads; bit 22: 8 rows in flight
  bool planes;           // (sv, arg_kind 1) bit 23: 8-channel planes of winning rows
};
constexpr MrFlags mr_flags(unsigned f) {
  return {(f & GKG_MR_DETERMINISTIC) != 0, (f & GKG_MR_FP32_ATOMICS) != 0, (int)((f >> 8) & 0xff), (int)((f >> 16) & 3),
          ((f >> 20) & 3) == 2, ((f >> 22) & 1) != 0, ((f >> 23) & 1) != 0};
}

// ------------------------------------------------------------------------------------------ token-major backward
enum MrBwdForm { MR_STREAM, MR_STREAM_F64, MR_TWO_SWEEP, MR_DET_PRIVATE, MR_DET_WALK, MR_LDS_F32, MR_GLOBAL_F32 };

struct MrBwdTmCall {     // gkg_mr_bwd_tm, _bnstats (want_stats), _bnstats_supported (want_stats, no pointers at all)
  int B, G, c, N, M, k, mode, arg_kind;
  unsigned flags;
  bool self_graph, want_stats;
};

struct MrBwdTmPlan {
  MrBwdForm form;
  int NT, ACC, U; bool STATS;      // mr_bwd_tm_stream_kernel<NT, ., ., ., ACC, U, STATS>; two-sweep: STATS only
  int cw;                          // chunk width; MR_DET_PRIVATE: TL, the private accumulators per workgroup; 0: the form has none
  unsigned grid_x, grid_y, block;
  size_t lds;                      // dynamic LDS bytes (statistics floor included)
  int shmax;                       // fixed-point forms: 38 - bits of N, | 1 << 16: planes of winning rows
  unsigned seed_grid;              // > 0: mr_bwd_tm_init_kernel goes first (gx = direct - gm) ...
  size_t gsrc_bytes;               // ... and (> 0) gsrc is cleared
  double work;                     // the profiler's algorithmic bytes
};

// Exact integer accumulation (see mr_bwd_tm_scatter_i64_kernel): the default whenever an (image, channel chunk) of 64-bit
// accumulators fits the LDS budget — order-independent, so it is also the deterministic form.  GKG_MR_FP32_ATOMICS keeps
// the fp32-atomic kernels (measurement, tests).
// Where it is selected (MI355X, tools/bench_mr_bwd.py, us, exact vs fp32 atomics at their best chunk widths): 18 x 18
// images — cfg2 21.2 vs 24.4-27.6, its label graph 9.4 vs 10.9, C = 640 39.3 vs 44.9-51.5; a tie at 36 x 36 (116.7 vs
// 113.5-118.2); it LOSES where the gradients stream from HBM and are swept twice (pooled 1 296-key images under 5 184 /
// 20 736 queries: 209 vs 164, 492 vs 425).  Rule: destination images of up to 512 rows; with GKG_MR_DETERMINISTIC wherever it
// fits (the private-accumulator form it replaces there is 1.6x the fp32 time).  Chunk width 8 (measured best or tied at
// every shape: the kernel lives on workgroups per CU), 4 when 8 does not fit.
// Streaming fixed-point form (mr_bwd_tm_stream_kernel, round 5): the default from 160 query rows per image wherever an (image,
// channel chunk) of 64-bit accumulators fits the LDS budget — one sweep, 4 / 8 rows per thread in flight, 512 threads.  Order-
// independent like the two-sweep form, so it serves GKG_MR_DETERMINISTIC too.  Measured against what it replaces
// (tools/bench_mr_bwd.py, us, profiles/r05_bench_mr_bwd_stream.txt): cfg2 21.8 -> 16.6, C = 640 at 18 x 18 38.7 -> 25.1,
// 36 x 36 self graph 117.6 -> 89.9, pooled 1 296-key images under 5 184 / 20 736 queries 165 -> 133 / 424 -> 359; the label
// graphs (80 queries) keep the two-sweep kernel (8.6 vs 9.2-9.9).  Chunk width: the widest of 16 / 8 / 4 channels that fits.
// Measurement (MrFlags): sv = 1 forces this form (with forced_cw, nt256, rows8), 2 = its fp64-atomic variant (ds_add_f64: 45-98
// cycles per wave instruction against 170-183 for ds_add_f32 — tools/ubench/lds_atomic_rate.hip), 3 = the two-sweep kernel
// wherever it fits.
inline int mr_bwd_tm_plan(const MrBwdTmCall& q, MrBwdTmPlan* p, const char** msg) {
  auto fail = [&](int code, const char* m) { *msg = m; return code; };
  const int B = q.B, G = q.G, c = q.c, N = q.N, M = q.M, k = q.k, ak = q.arg_kind;
  if (ak != 0 && ak != 1) return fail(GKG_ERR_SHAPE, "gkg_mr_bwd_tm: arg_kind is 0 or 1");
  if (B <= 0 || G <= 0 || c <= 0 || N <= 0 || M <= 0 || k <= 0 || k > 255 || (c & 3)) return fail(GKG_ERR_SHAPE, "gkg_mr_bwd_tm: bad sizes");
  if (q.mode != 0 && q.mode != 1) return fail(GKG_ERR_SHAPE, "gkg_mr_bwd_tm: mode is 0 or 1");
  if (q.mode == 1 && ((G * c) & 15)) return fail(GKG_ERR_SHAPE, "gkg_mr_bwd_tm: mode 1 needs C % 16 == 0");
  if (q.self_graph && M != N) return fail(GKG_ERR_SHAPE, "gkg_mr_bwd_tm: self graph needs M == N");
  *p = MrBwdTmPlan{};
  // algorithmic bytes (SURVEY §8d "MR bwd"): g + int64 indices + argmax + gx (+ gsrc); arg_kind 1: u16 winning rows, no indices
  p->work = 4.0 * B * (double)G * c * N + (ak == 1 ? 0.0 : 8.0 * B * (double)G * N * k) + (ak == 1 ? 2.0 : 1.0) * B * (double)G * c * N
            + 4.0 * B * (double)G * c * N + (q.self_graph ? 0.0 : 4.0 * B * (double)G * c * M);
  const int C = G * c;
  const MrFlags f = mr_flags(q.flags);
  const int sv = f.sv;
  // with statistics: only the library's own choice among the two exact forms (no measurement overrides), XM gradient layout
  if (q.want_stats && (q.mode != 1 || sv || f.forced_cw || f.f32))
    return fail(GKG_ERR_UNSUPPORTED, "gkg_mr_bwd_tm_bnstats: mode 1 and the default scatter form only");
  auto fits = [&](int cw, size_t budget) { return mr_i64_lds(M, cw) <= budget && mr_divides(C, c, cw); };
  auto fixed_point = [&](MrBwdForm form, int nt, int cw) {
    p->form = form; p->NT = nt; p->U = 4; p->STATS = q.want_stats; p->cw = cw;
    p->grid_x = mr_chunk_grid(C, cw, B); p->grid_y = 1; p->block = (unsigned)nt;
    p->lds = mr_i64_lds(M, cw);
    if (q.want_stats && p->lds < mr_stats_floor(nt, cw)) p->lds = mr_stats_floor(nt, cw);
    p->shmax = mr_shmax(N);
    return 0;
  };
  if (N < (1 << 24) && (sv == 1 || sv == 2 || (sv == 0 && !f.f32 && N >= 160))) {
    int CW = f.forced_cw;
    if (!CW || !sv) CW = fits(16, MR_LDS_BUDGET) ? 16 : (fits(8, MR_LDS_BUDGET) ? 8 : 4);
    if ((sv && fits(CW, 150 * 1024)) || fits(CW, MR_LDS_BUDGET)) {
      // long sweeps over a pooled key image (GKGNet-576 stages 1 / 2: N = 16 M / 4 M, M = 1 296): 256-thread workgroups with 4 rows
      // in flight — two workgroups per CU overlap one's store phase with the other's sweep (round 6, on the XM gradient layout,
      // us: stage 1 379.6 -> 334.9, stage 2 145.7 -> 141.0; the self graphs keep 512 threads: 36 x 36 89.7 vs 93.5)
      const bool long_sweep = M > 512 && (long)N >= 4L * M;
      const bool nt256 = sv == 2 ? false : sv ? f.nt256 : long_sweep;
      const bool u8 = sv == 2 ? false : sv ? f.rows8 : (M > 512 && !long_sweep);       // 8 rows in flight
      if (q.want_stats && (nt256 || u8)) return fail(GKG_ERR_UNSUPPORTED, "gkg_mr_bwd_tm_bnstats: long-sweep streaming forms carry no statistics");
      fixed_point(sv == 2 ? MR_STREAM_F64 : MR_STREAM, nt256 ? 256 : 512, CW);
      p->ACC = sv == 2; p->U = u8 ? 8 : 4;
      if (sv && f.planes && ak == 1) p->shmax |= 1 << 16;       // measurement: 8-channel planes of winning rows
      return 0;
    }
    if (sv) return fail(GKG_ERR_UNSUPPORTED, "gkg_mr_bwd_tm: forced streaming form does not fit");
  }
  if (!f.f32 && N < (1 << 24) && (M <= 512 || sv == 3 || f.det)) {
    int CW = fits(8, MR_LDS_BUDGET) ? 8 : 4;
    if (f.forced_cw) CW = f.forced_cw;         // measurement only
    if (fits(CW, MR_LDS_BUDGET) && mr_chunk_grid_ok(C, CW, B)) return fixed_point(MR_TWO_SWEEP, 256, CW);
  }
  if (q.want_stats) return fail(GKG_ERR_UNSUPPORTED, "gkg_mr_bwd_tm_bnstats: this shape takes a scatter form without statistics");
  const size_t total = (size_t)B * N * (C / 4);
  const unsigned seed_grid = (unsigned)((total + 255) / 256);
  const size_t gsrc_bytes = q.self_graph ? 0 : sizeof(float) * (size_t)B * M * C;
  if (f.det) {
    if (B > 65535) return fail(GKG_ERR_UNSUPPORTED, "gkg_mr_bwd_tm: B <= 65535");
    long TL = (long)(144 * 1024) / ((long)M * 16);
    if (TL > 64) TL = 64;
    p->block = 64;
    if (TL >= 1) {
      p->form = MR_DET_PRIVATE; p->cw = (int)TL; p->grid_x = (unsigned)(C / 4); p->grid_y = (unsigned)B; p->lds = (size_t)TL * M * 16;
    } else {                         // seed (gx = direct - gm; gsrc = 0), then the ordered global walk
      p->form = MR_DET_WALK; p->grid_x = (unsigned)((B * (C / 4) + 63) / 64); p->grid_y = 1;
      p->seed_grid = seed_grid; p->gsrc_bytes = gsrc_bytes;
    }
    return 0;
  }
  // channel chunk: largest power of two (4..64) dividing C and c whose [M][CW] fp32 image fits the LDS budget, shrunk
  // until the grid has ~2 workgroups per CU
  auto fits32 = [&](int cw) { return mr_f32_lds(M, cw) <= (size_t)MR_LDS_BUDGET && mr_divides(C, c, cw); };
  int CW = 64;
  while (CW > 4 && !fits32(CW)) CW >>= 1;
  while (CW > 8 && (long)(C / CW) * B < 512) CW >>= 1;
  if (f.forced_cw) CW = f.forced_cw;           // measurement only
  p->grid_y = 1; p->block = 256;
  if (fits32(CW) && mr_chunk_grid_ok(C, CW, B)) {
    p->form = MR_LDS_F32; p->cw = CW; p->grid_x = mr_chunk_grid(C, CW, B); p->lds = mr_f32_lds(M, CW);
  } else {                           // destination image too large for LDS: elementwise seed + fp32 global atomics
    p->form = MR_GLOBAL_F32; p->grid_x = seed_grid; p->seed_grid = seed_grid; p->gsrc_bytes = gsrc_bytes;
  }
  return 0;
}

// ------------------------------------------------------------------------------------------ token-major forward
struct MrFwdTmCall {     // gkg_mr_fwd_tm, gkg_mr_fwd_tm16 (idx16)
  int B, G, c, N, M, k, mode, out_dtype, arg_kind;
  int ldx, xchunk;       // x as a view: row pitch in floats (0: C), chunk (gkg_common.h "XM layout")
  bool has_src, x_is_out, has_argmax, idx16;       // x_is_out: the pointers x and out are equal
};

struct MrFwdTmPlan {
  int ldx, lds_, schunk;           // the views of x and of the source rows, resolved
  int write_x;                     // mode 1: 0 when x already lives in the operand buffer (the caller passed that buffer's x half as x)
  unsigned grid;                   // 256 threads, one channel quad each
  int KS, AK; bool out_bf16;       // mr_fwd_tm_kernel<KS, 1, float | uint16_t, AK, int64_t | uint16_t (idx16)>
  double work;
};

inline int mr_fwd_tm_plan(const MrFwdTmCall& q, MrFwdTmPlan* p, const char** msg) {
  auto fail = [&](int code, const char* m) { *msg = m; return code; };
  const int B = q.B, G = q.G, c = q.c, N = q.N, M = q.M, k = q.k;
  if (q.idx16 && M > 65536) return fail(GKG_ERR_UNSUPPORTED, "gkg_mr_fwd_tm16: M <= 65536 (u16 rows)");
  if (q.arg_kind != 0 && q.arg_kind != 1) return fail(GKG_ERR_SHAPE, "gkg_mr_fwd_tm: arg_kind is 0 (u8 slot) or 1 (u16 row index)");
  if (q.arg_kind == 1 && M > 65536) return fail(GKG_ERR_UNSUPPORTED, "gkg_mr_fwd_tm: arg_kind 1 needs M <= 65536");
  if (B <= 0 || G <= 0 || c <= 0 || N <= 0 || M <= 0 || k <= 0 || k > 255 || (c & 3)) return fail(GKG_ERR_SHAPE, "gkg_mr_fwd_tm: bad sizes (c % 4 == 0, k <= 255)");
  if (q.mode != 0 && q.mode != 1) return fail(GKG_ERR_SHAPE, "gkg_mr_fwd_tm: mode is 0 or 1");
  if (q.mode == 1 && ((G * c) & 15)) return fail(GKG_ERR_SHAPE, "gkg_mr_fwd_tm: mode 1 needs C % 16 == 0");
  if (q.out_dtype != GKG_F32 && q.out_dtype != GKG_BF16) return fail(GKG_ERR_UNSUPPORTED, "gkg_mr_fwd_tm: out_dtype is GKG_F32 or GKG_BF16");
  *p = MrFwdTmPlan{};
  const int C = G * c, xchunk = q.xchunk;
  const int ldx = q.ldx == 0 ? C : q.ldx;
  if (ldx < C || (ldx & 3) || xchunk < 0 || (xchunk & 3) || (xchunk > 0 && (C % xchunk || ldx < 2 * C)))
    return fail(GKG_ERR_SHAPE, "gkg_mr_fwd_tm: bad x view (ldx >= C, ldx % 4 == 0; a chunk is a multiple of 4 dividing C, with ldx >= 2 C)");
  if (!q.has_src && M != N) return fail(GKG_ERR_SHAPE, "gkg_mr_fwd_tm: self graph needs M == N");
  p->ldx = ldx; p->lds_ = q.has_src ? C : ldx; p->schunk = q.has_src ? 0 : xchunk;
  // mode 1: x already lives in the operand buffer when the caller passes that buffer's x half as the view of x
  p->write_x = !(q.mode == 1 && q.x_is_out && ldx == 2 * C && xchunk == (C >> 2) && q.out_dtype == GKG_F32);
  if (q.mode == 1 && q.x_is_out && p->write_x) return fail(GKG_ERR_SHAPE, "gkg_mr_fwd_tm: x aliases out but is not its x half (ldx = 2 C, xchunk = C / 4, fp32)");
  // algorithmic bytes (SURVEY §8d "MR gather-max fwd"): x + (keys) + indices + m (+ 1 byte of argmax per element)
  p->out_bf16 = q.out_dtype == GKG_BF16;
  p->work = 4.0 * B * (double)G * c * N + (q.has_src ? 4.0 * B * (double)G * c * M : 0.0) + (q.idx16 ? 2.0 : 8.0) * B * (double)G * N * k
            + (p->out_bf16 ? 2.0 : 4.0) * B * (double)G * c * N + (q.has_argmax ? 1.0 * B * (double)G * c * N : 0.0);
  // one channel quad per thread: two quads per thread (shared index row) measured 20 % slower at cfg2 — the kernel
  // wants more threads in flight, not fewer index loads
  const long bpi = ((long)N * (G * c / 4) + 255) / 256;
  if (bpi * (((long)B + 7) / 8) * 8 > 0x7fffffffL) return fail(GKG_ERR_UNSUPPORTED, "gkg_mr_fwd_tm: problem too large for one launch");
  p->grid = (unsigned)(bpi * ((B + 7) / 8) * 8);
  p->KS = k == 9 ? 9 : 0; p->AK = q.arg_kind;
  return 0;
}

// ------------------------------------------------------------------------------------------ channel-major (gkg_mr_fwd, gkg_mr_bwd)
struct MrCmCall { bool bwd; int BG, c, N, M, k, dtype; bool self_graph; };

struct MrCmPlan {
  bool fallback;         // the rows do not fit in LDS — forward: gather from L2; backward: fp32 global atomics (fp32 tensors only)
  int CH;                // channels per workgroup (LDS forms)
  unsigned grid_x, grid_y, grid_z;
  size_t lds;
  unsigned seed_grid;    // backward fallback, self graph: negate_kernel writes gx = -g first ...
  size_t gsrc_bytes;     // ... bipartite: gsrc is cleared first
};

inline int mr_cm_plan(const MrCmCall& q, MrCmPlan* p, const char** msg) {
  auto fail = [&](int code, const char* m) { *msg = m; return code; };
  const int BG = q.BG, c = q.c, N = q.N, M = q.M, k = q.k;
  if (BG <= 0 || c <= 0 || N <= 0 || M <= 0 || k <= 0 || k > 255)
    return fail(GKG_ERR_SHAPE, q.bwd ? "gkg_mr_bwd: bad sizes (k <= 255)" : "gkg_mr_fwd: bad sizes (k <= 255)");
  if (q.self_graph && M != N) return fail(GKG_ERR_SHAPE, q.bwd ? "gkg_mr_bwd: self graph needs M == N" : "gkg_mr_fwd: self graph needs M == N");
  if (q.dtype != GKG_F32 && q.dtype != GKG_BF16 && q.dtype != GKG_F16) return fail(GKG_ERR_UNSUPPORTED, q.bwd ? "gkg_mr_bwd: dtype" : "gkg_mr_fwd: dtype");
  if (BG > 65535) return fail(GKG_ERR_UNSUPPORTED, q.bwd ? "gkg_mr_bwd: BG <= 65535" : "gkg_mr_fwd: BG <= 65535");
  *p = MrCmPlan{};
  const unsigned ntiles = (unsigned)((N + 255) / 256);
  // channels per workgroup: as many rows as fit, but keep enough workgroups to fill the chip
  int CH = mr_pick_ch(c, M, k);
  if (CH < 1) {
    if (q.bwd && q.dtype != GKG_F32) return fail(GKG_ERR_UNSUPPORTED, "gkg_mr_bwd: M too large for the LDS accumulator and dtype is not fp32");
    p->fallback = true;
    p->grid_x = ntiles; p->grid_y = (unsigned)(c < 64 ? c : 64); p->grid_z = (unsigned)BG;
    if (q.bwd && q.self_graph) p->seed_grid = (unsigned)(((size_t)BG * c * N + 255) / 256);
    if (q.bwd && !q.self_graph) p->gsrc_bytes = sizeof(float) * (size_t)BG * c * M;
    return 0;
  }
  const long sweeps = q.bwd ? 1 : (long)ntiles;       // workgroups per (channel chunk, problem)
  while (CH > (q.bwd ? 2 : 4) && sweeps * ((c + CH - 1) / CH) * BG < 1024) CH = (CH + 1) / 2;
  p->CH = CH; p->lds = mr_cm_lds(CH, M, k);
  const unsigned chunks = (unsigned)((c + CH - 1) / CH);
  if (q.bwd) { p->grid_x = chunks; p->grid_y = (unsigned)BG; p->grid_z = 1; }
  else { p->grid_x = ntiles; p->grid_y = chunks; p->grid_z = (unsigned)BG; }
  return 0;
}

}  // namespace gkg
