// gkg_mr_fc2_bf16.hip — bf16 inference: the second half of a Grapher (max-relative aggregation + grouped 1x1 projection + BN + GELU,
// then fc2 + BN + residual) as ONE kernel; the (T, 2C) bf16 matrix between the two projections never exists in memory.
//
// Reference chain (mmcls/models/backbones/vig_model/torch_vertex.py:47-62 MRConv2d.forward, torch_nn.py:57-69 BasicConv,
// torch_vertex.py:325-333 Grapher.fc2 + shortcut) under bf16 autocast with gradients off.  As two launches — gkg_mr_linear_bf16
// (csrc/gkg_mrgemm.hip) and gkg_linear_bf16 (csrc/gkg_linear_bf16.hip) — the first writes the (T, 2C) bf16 matrix
// and the second reads it back; here the workgroup that produced a token tile's rows of it contracts them with fc2's weight at once.
//
// One workgroup (8 waves) owns 64 tokens, ALL 2C hidden columns and ALL C <= 192 output columns.  Two forms (template parameters
// MAXB / VB, blocks of 32 x 32 per wave in GEMM 1 / GEMM 2): wide (3 / 2: up to C = 192) and narrow (2 / 1: up to C = 128, the
// stage-1 widths, whose phases are gather latency: fewer accumulators, three workgroups per CU at k = 9 instead of two).
//   phases 0-2  gkg_mrgemm_tile.h, the code mr_linear_bf16_kernel<.., QG = 4> runs: index rows -> LDS, gather + max_k(x_j - x_i) +
//               [x, m] interleave -> the four conv groups' bf16 A tiles in LDS, GEMM 1 on v_mfma_f32_32x32x16_bf16 (wave w: row
//               block w & 1, up to 3 (conv group, column block) pairs), the grouped weight's fragments streamed from L2;
//   hidden      after a barrier (every wave is done with the A tiles) h = bf16(act(fma(a1, acc, c1))) — mg_hidden, the element as
//               the first launch stores it — goes into a DENSE row image of the hidden tile in the A tiles' place: 64 rows x 2C
//               columns (column q co + n), pitch 4C + 16 B (conflict-free 16-byte reads).  Not the per-group tiles: fc2's steps of
//               16 straddle conv groups where co = C / 2 is no multiple of 16 (C = 80, 48);
//   GEMM 2      image (64 x 2C) . W2 (2C x C): wave w takes row block w & 1 and column blocks (w >> 1) + 4 v, v < 2 — at C = 192
//               waves 0-3 hold two blocks and waves 4-7 one, i.e. every SIMD (waves s and s + 4) three of the twelve; fc2's
//               fragments ([2C / 8][co2] x 16 B, gkg_linear_bf16's array) stream from L2 three steps ahead, the first of them
//               issued before the barrier that completes the image; ascending steps of 16 over all of 2C (2C % 32 == 0: no
//               padding), no K-split — the contraction order of the second launch;
//   epilogue    gkg_linear_bf16's: z = fma(a2, acc, c2) (a2 == NULL: acc + c2) staged in the (free again) LDS, walked as
//               8-column segments: residual read as 2 x float4, fp32 result stored as 2 x 16 B, bf16 result (the rounding of the
//               fp32 one, pack_bf16x2) as 16 B.
// Every output bit is that of gkg_mr_linear_bf16[_nn16](.. -> h16) followed by gkg_linear_bf16(h16, ..): one definition of the
// gather, the clamp, the tie rule, the GELU and the rounding (the shared header), the same MFMA over the same steps in both
// contractions, the second launch's epilogue arithmetic.  Workgroups are dealt to the XCDs so that each XCD walks a contiguous
// range of token tiles.  No workgroup waits for another: no counters, no flags, no scratch buffer.  Rows >= T are zero A rows,
// never stored; nothing outside columns [0, C) of rows [0, T) of either output is written.
//
// LDS: the four A tiles (4 x 64 x (ci_pad + 8) x 2 B; the hidden image and the epilogue stage are never larger and take their
// place) + the index rows [64][G][k], kept as u16 where M <= 65 536 (every shape of the models), int32 beyond.  At the widest
// shape (C 192, G 8, k 18) that is 53 248 + 18 432 = 71 680 B: TWO workgroups per CU (160 KB), 4 waves per SIMD, which the
// register allocation is held to (launch bounds: 128 VGPRs); with int32 rows the same shape takes 90 112 B, one workgroup per CU.
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; NO scratch and NO VGPR spills in any
// of the twelve instantiations, 0 AGPRs in all; the u16 and int32 index-row forms have the same figures):
//   mr_fc2_bf16_kernel<KS, INF, ., MAXB, VB, WPE>   VGPRs  SGPRs  waves / SIMD   LDS (dynamic) at             workgroups / CU: registers, LDS
//   < 9, 1, ., 2, 1, 6>  narrow, k = 9                 78    102       6         30 976 B  cfg3 stage 1 (C  80, G 2)        3, 5
//   <18, 1, ., 2, 1, 4>  narrow, k = 18               100    104       5 -> 4    47 104 B  cfg5 stage 1 (C  96, G 8)        2, 3
//   < 0, 1, ., 2, 1, 6>  narrow, any k                 79    106       6         (by G k)                                  3
//   < 9, 2, ., 3, 2, 4>  wide,   k = 9                127    106       4         47 360 B  cfg3 stage 2 (C 160, G 2)        2, 3
//   <18, 1, ., 3, 2, 4>  wide,   k = 18               110    104       4         71 680 B  cfg5 stage 2 (C 192, G 8)        2, 2
//   < 0, 1, ., 3, 2, 4>  wide,   any k                111    106       4         (by G k)                                  2
// (KS: the compiled neighbour count, 0 = any k <= 64; INF: (token, channel quad) items in flight per thread in phase 1.  A
// workgroup is 8 waves, 2 per SIMD: 5 waves per SIMD by registers are 2 workgroups.  The two any-k forms keep 12 / 6 scalar
// registers in lanes of a vector register across the runtime-k loop ("SGPRs Spill" 12 / 6: v_writelane, no memory); the compiled-k
// forms none.  With the GEMM 1 fragments fetched three steps ahead, as mr_linear_bf16_kernel does, the wide any-k form spilled 72
// vector registers: GEMM 1 has at most 6 steps here and fetches two ahead.)
// Measured, MI355X, fused against the pair (tools/bench_lin_bf16.py --tail; EXPERIMENTS.md "Fused bf16 Grapher tail"): the wide form
// at every width first — cfg3 stage 1 523 -> 500 us, cfg5 stage 1 989 -> 924 us, two workgroups per CU; the narrow form took cfg3
// stage 1 to 428 us (k = 9: three workgroups per CU) and cfg5 stage 1 to 912 us (k = 18: the 19 rows in flight keep it at two).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gkg_common.h"
#include "gkg_mrgemm_tile.h"

namespace gkg {

constexpr int MF_MAXC = 192;                     // widest C: GEMM 2 holds 64 x C fp32 accumulators, two blocks per wave at the most
constexpr int MF_VB = 2;                         // output blocks of GEMM 2 per wave (wide form; the narrow one: 1)
constexpr int MF_D1 = 2;                        // the grouped weight's fragments are fetched this many steps ahead (at most 6 steps)
constexpr int MF_D = 3;                         // fc2's (up to 24 steps)
constexpr size_t MF_LDS_MAX = 160 * 1024;        // the CU's LDS

struct MrFc2Args {
  MrGemmArgs m;                                  // the first projection's operands (out / ldo unused: the hidden stays in LDS)
  const uint4* w2; const float* a2; const float* c2;    // [2C / 8][co2] fragments; [C] or null (= 1); [C]
  const float* res; int ldr;                     // (T, ldr) fp32 or null
  float* o32; int ldo32;                         // (T, ldo32) or null
  uint16_t* o16; int ldo16;                      // (T, ldo16) bf16 or null
  int co2;                                       // C padded to 32: the columns of fc2's fragment array
  int ids_off;                                   // bytes: where the index rows start in LDS
};

static inline size_t mf_tile_bytes(int C) {
  const int ci_pad = (C / 2 + 15) & ~15, co2 = (C + 31) & ~31;
  const size_t a = (size_t)4 * MG_ROWS * (ci_pad + 8) * 2;           // the four A tiles
  const size_t h = (size_t)MG_ROWS * (2 * C + 8) * 2;                // the hidden image
  const size_t s = (size_t)MG_ROWS * (co2 + 4) * 4;                  // the epilogue stage
  return a > h ? (a > s ? a : s) : (h > s ? h : s);
}
static inline size_t mf_lds_bytes(int C, int G, int k, bool ids16) {
  return mf_tile_bytes(C) + (size_t)MG_ROWS * G * k * (ids16 ? 2 : 4);
}

// KS: the compiled neighbour count (0: any k <= 64); INF: (token, channel quad) items in flight per thread in phase 1; IdT: the index
// rows' type in LDS; MAXB / VB: blocks of GEMM 1 / GEMM 2 per wave — 3 / 2 up to C = 192 (the wide form), 2 / 1 up to C = 128 (the
// narrow form: fewer accumulators, more waves per SIMD where the phases are latency); WPE: waves per SIMD the registers must allow
template <int KS, int INF, typename IdT, int MAXB, int VB, int WPE>
__global__ __launch_bounds__(64 * MG_NW, WPE) void mr_fc2_bf16_kernel(MrFc2Args a) {
  extern __shared__ __align__(16) unsigned char mf_lds[];
  constexpr int NT = 64 * MG_NW;
  const MrGemmArgs& g = a.m;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  // XCD-aware map (workgroups are dealt round-robin over the 8 XCDs): XCD i walks token tiles [i * tiles_per_xcd, ...) — whole
  // contiguous token ranges, a token's neighbours are rows of its own image
  const int lin = blockIdx.x;
  const int tl = lin >> 3, tile = (lin & 7) * g.tiles_per_xcd + tl;
  if (tl >= g.tiles_per_xcd || tile >= g.tiles) return;
  const long long t0 = (long long)tile * MG_ROWS;
  const int pitch = (g.ci_pad + 8) * 2;                  // bytes per A-tile row
  const int qstride = MG_ROWS * pitch;
  const int hpitch = (2 * g.C + 8) * 2;                  // bytes per row of the hidden image
  const int k = KS > 0 ? KS : g.k;

  // ---------------------------------------------------------------- phases 0-2: the grouped projection's accumulators
  IdT* ids = reinterpret_cast<IdT*>(mf_lds + a.ids_off);             // [64][G][k]
  mg_index_rows(g, ids, t0, 0, g.G, k, tid);
  __syncthreads();
  mg_gather_tile<KS, 4, INF>(g, mf_lds, ids, t0, 0, 0, g.G, k, pitch, qstride, tid);
  __syncthreads();
  const int l31 = lane & 31, kg = lane >> 5;
  const int rb = w & 1;
  const int ncb = g.co_pad >> 5;
  mg_f32x16 acc1[MAXB];
  bool has[MAXB];
  mg_group_gemm<4, MAXB, MF_D1>(g, mf_lds, 0, pitch, qstride, w, lane, acc1, has);

  // the BN vectors of the wave's hidden columns: on their way while the waves meet (fc2's first fragments follow the image's writes,
  // ahead of the barrier that completes it: issued here, beside GEMM 1's accumulators, they cost the any-k form vector spills)
  float av1[MAXB], cv1[MAXB];
  int hcol[MAXB];                                     // the block's column of this lane in the hidden image, -1: none
#pragma unroll
  for (int u = 0; u < MAXB; ++u) {
    const int p = (w >> 1) + (MG_NW / 2) * u;
    const int qi = has[u] ? p / ncb : 0, cb = has[u] ? p - qi * ncb : 0;
    const int col = 32 * cb + l31;
    hcol[u] = (has[u] && col < g.co) ? qi * g.co + col : -1;
    av1[u] = hcol[u] >= 0 ? g.a[hcol[u]] : 0.f;
    cv1[u] = hcol[u] >= 0 ? g.cs[hcol[u]] : 0.f;
  }
  const int nb2 = a.co2 >> 5;
  const int S2 = g.C >> 3;                               // steps of 16 over the 2C hidden columns
  bool has2[VB];
  const uint4* w2p[VB];
#pragma unroll
  for (int v = 0; v < VB; ++v) {
    const int cb = (w >> 1) + (MG_NW / 2) * v;
    has2[v] = cb < nb2;                                  // wave-uniform
    w2p[v] = a.w2 + (size_t)kg * a.co2 + 32 * (has2[v] ? cb : 0) + l31;
  }

  // ---------------------------------------------------------------- the hidden tile: BN (eval) + activation -> bf16 -> dense rows
  __syncthreads();                                       // every wave is done reading the A tiles: the image takes their place
#pragma unroll
  for (int u = 0; u < MAXB; ++u) {
    if (hcol[u] >= 0) {
      unsigned char* hp = mf_lds + 2 * hcol[u];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = 32 * rb + (r & 3) + 8 * (r >> 2) + 4 * kg;
        *reinterpret_cast<uint16_t*>(hp + row * hpitch) = mg_hidden(av1[u], acc1[u][r], cv1[u], g.act);
      }
    }
  }
  uint4 bq[MF_D][VB];
#pragma unroll
  for (int d = 0; d < MF_D; ++d)
#pragma unroll
    for (int v = 0; v < VB; ++v)
      bq[d][v] = (has2[v] && d < S2) ? w2p[v][(size_t)(2 * d) * a.co2] : make_uint4(0, 0, 0, 0);
  __syncthreads();

  // ---------------------------------------------------------------- GEMM 2: (64 x 2C) @ W2^T, the second launch's contraction
  mg_f32x16 acc2[VB];
#pragma unroll
  for (int v = 0; v < VB; ++v)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc2[v][r] = 0.f;
  {
    const unsigned char* ap = mf_lds + (32 * rb + l31) * hpitch + 16 * kg;
    for (int s0 = 0; s0 < S2; s0 += MF_D) {
#pragma unroll
      for (int d = 0; d < MF_D; ++d) {
        const int s = s0 + d;
        if (s < S2) {                                    // uniform
          uint4 bc[VB];
#pragma unroll
          for (int v = 0; v < VB; ++v) bc[v] = bq[d][v];
#pragma unroll
          for (int v = 0; v < VB; ++v)
            if (has2[v] && s + MF_D < S2) bq[d][v] = w2p[v][(size_t)(2 * (s + MF_D)) * a.co2];
          if (has2[0]) {                                 // (a wave without a first block has no second)
            const mg_bf16x8 xv = __builtin_bit_cast(mg_bf16x8, *reinterpret_cast<const uint4*>(ap + 32 * s));
#pragma unroll
            for (int v = 0; v < VB; ++v)
              if (has2[v]) acc2[v] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xv, __builtin_bit_cast(mg_bf16x8, bc[v]), acc2[v], 0, 0, 0);
          }
        }
      }
    }
  }

  // ---------------------------------------------------------------- epilogue 2: BN (eval) -> stage -> + residual -> rows out
  __syncthreads();                                       // every wave is done reading the image: the stage takes its place
  const int C = g.C;
  const int SP = a.co2 + 4;                              // floats per stage row
  float* st = reinterpret_cast<float*>(mf_lds);          // [64][SP]
  auto affine = [&](bool scaled) __attribute__((always_inline)) {
#pragma unroll
    for (int v = 0; v < VB; ++v) {
      const int col = 32 * ((w >> 1) + (MG_NW / 2) * v) + l31;
      if (has2[v] && col < C) {
        const float cv = a.c2[col];
        const float av = scaled ? a.a2[col] : 1.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = 32 * rb + (r & 3) + 8 * (r >> 2) + 4 * kg;
          st[row * SP + col] = scaled ? __builtin_fmaf(av, acc2[v][r], cv) : acc2[v][r] + cv;
        }
      }
    }
  };
  if (a.a2) affine(true); else affine(false);            // the mode tests once, not per element
  __syncthreads();
  const int NS = C >> 3;                                 // 8-column segments per row (C % 16 == 0: none partial)
  for (int it = tid; it < MG_ROWS * NS; it += NT) {
    const int rl = it / NS, col = 8 * (it - rl * NS);
    const long long t = t0 + rl;
    if (t < g.T) {
      float4 z0 = *reinterpret_cast<const float4*>(st + rl * SP + col);
      float4 z1 = *reinterpret_cast<const float4*>(st + rl * SP + col + 4);
      if (a.res) {
        const float* rp = a.res + (size_t)t * a.ldr + col;
        const float4 q0 = *reinterpret_cast<const float4*>(rp), q1 = *reinterpret_cast<const float4*>(rp + 4);
        z0.x += q0.x; z0.y += q0.y; z0.z += q0.z; z0.w += q0.w;
        z1.x += q1.x; z1.y += q1.y; z1.z += q1.z; z1.w += q1.w;
      }
      if (a.o32) {
        float* op = a.o32 + (size_t)t * a.ldo32 + col;
        *reinterpret_cast<float4*>(op) = z0;
        *reinterpret_cast<float4*>(op + 4) = z1;
      }
      if (a.o16)
        *reinterpret_cast<uint4*>(a.o16 + (size_t)t * a.ldo16 + col) =
            make_uint4(pack_bf16x2(z0.x, z0.y), pack_bf16x2(z0.z, z0.w), pack_bf16x2(z1.x, z1.y), pack_bf16x2(z1.z, z1.w));
    }
  }
}

template <int KS, int INF, typename IdT, int MAXB, int VB, int WPE>
static hipError_t mf_launch(const MrFc2Args& a, size_t lds, hipStream_t st) {
  if (lds > 64 * 1024) {
    const hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void*>(&mr_fc2_bf16_kernel<KS, INF, IdT, MAXB, VB, WPE>),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (ea != hipSuccess) return ea;
  }
  hipLaunchKernelGGL((mr_fc2_bf16_kernel<KS, INF, IdT, MAXB, VB, WPE>), dim3((unsigned)(a.m.tiles_per_xcd * 8)), dim3(64 * MG_NW), lds, st,
                     a);
  return hipGetLastError();
}

template <typename IdT>
static hipError_t mf_launch_k(const MrFc2Args& a, size_t lds, hipStream_t st) {
  const int k = a.m.k;
  // the narrow form where every wave has at most 2 blocks in GEMM 1 and 1 in GEMM 2 (C <= 128: the stage-1 widths)
  if (4 * (a.m.co_pad >> 5) <= (MG_NW / 2) * 2 && (a.co2 >> 5) <= MG_NW / 2)
    return k == 9 ? mf_launch<9, 1, IdT, 2, 1, 6>(a, lds, st)
                  : (k == 18 ? mf_launch<18, 1, IdT, 2, 1, 4>(a, lds, st) : mf_launch<0, 1, IdT, 2, 1, 6>(a, lds, st));
  return k == 9 ? mf_launch<9, 2, IdT, MG_MAXB, MF_VB, 4>(a, lds, st)
                : (k == 18 ? mf_launch<18, 1, IdT, MG_MAXB, MF_VB, 4>(a, lds, st) : mf_launch<0, 1, IdT, MG_MAXB, MF_VB, 4>(a, lds, st));
}

static int mr_fc2_bf16_impl(const float* x, const float* src, const int64_t* nn_idx, const uint16_t* nn16, const void* wplanes,
                            const float* a1, const float* c1, const void* w2planes, const float* a2, const float* c2, const float* res,
                            int ldr, float* out_f32, int ldo32, void* out_bf16, int ldo16, int B, int G, int c, int N, int M, int k,
                            int act, void* stream) {
  if (!x || (!nn_idx && !nn16) || !wplanes || !a1 || !c1 || !w2planes || !c2 || (!out_f32 && !out_bf16))
    return gkg_fail(GKG_ERR_NULL, "gkg_mr_fc2_bf16: null pointer");
  if (B <= 0 || G <= 0 || c <= 0 || N <= 0 || M <= 0 || k <= 0 || act < 0 || act > 1)
    return gkg_fail(GKG_ERR_SHAPE, "gkg_mr_fc2_bf16: bad sizes (need > 0, act in 0..1)");
  if (!src && M != N) return gkg_fail(GKG_ERR_SHAPE, "gkg_mr_fc2_bf16: self graph needs M == N");
  if (!gkg_mr_fc2_bf16_supported(B, G, c, N, M, k, res != nullptr, out_f32 != nullptr, out_bf16 != nullptr, act))
    return gkg_fail(GKG_ERR_UNSUPPORTED, "gkg_mr_fc2_bf16: need C % 16 == 0, c % 4 == 0, C <= 192, k <= 64, index rows that fit the LDS and a grid that fits");
  if (nn16 && M > 65536) return gkg_fail(GKG_ERR_UNSUPPORTED, "gkg_mr_fc2_bf16_nn16: M <= 65536 (u16 rows)");
  if ((out_bf16 && (ldo16 & 7)) || (out_f32 && (ldo32 & 3)) || (res && (ldr & 3)))
    return gkg_fail(GKG_ERR_UNSUPPORTED, "gkg_mr_fc2_bf16: need ldo16 % 8 == 0, ldo32 % 4 == 0, ldr % 4 == 0");
  if (((uintptr_t)x | (uintptr_t)src | (uintptr_t)wplanes | (uintptr_t)w2planes | (uintptr_t)res | (uintptr_t)out_f32 | (uintptr_t)out_bf16) & 15)
    return gkg_fail(GKG_ERR_UNSUPPORTED, "gkg_mr_fc2_bf16: x, src, the fragment arrays, res and the outputs must be 16-byte aligned");
  const int C = G * c;
  if ((out_bf16 && ldo16 < C) || (out_f32 && ldo32 < C) || (res && ldr < C))
    return gkg_fail(GKG_ERR_SHAPE, "gkg_mr_fc2_bf16: a row pitch is below the row's width");
  MrFc2Args a;
  MrGemmArgs& g = a.m;
  g.x = x; g.src = src; g.nn_idx = nn_idx; g.nn16 = nn16; g.wp = (const uint4*)wplanes; g.a = a1; g.cs = c1;
  g.out = nullptr; g.ldo = 0;
  g.B = B; g.G = G; g.c = c; g.N = N; g.M = M; g.k = k; g.C = C; g.Cq = C / 4; g.ci = C / 2; g.co = C / 2;
  g.ci_pad = (g.ci + 15) & ~15; g.co_pad = (g.co + 31) & ~31; g.act = act;
  g.T = (long long)B * N;
  const long long tiles = (g.T + MG_ROWS - 1) / MG_ROWS;
  g.tiles = (int)tiles;
  g.tiles_per_xcd = (int)((tiles + 7) / 8);
  a.w2 = (const uint4*)w2planes; a.a2 = a2; a.c2 = c2; a.res = res; a.ldr = ldr;
  a.o32 = out_f32; a.ldo32 = ldo32; a.o16 = (uint16_t*)out_bf16; a.ldo16 = ldo16;
  a.co2 = (C + 31) & ~31;
  a.ids_off = (int)mf_tile_bytes(C);
  const bool ids16 = M <= 65536;
  const size_t lds = mf_lds_bytes(C, G, k, ids16);
  hipStream_t st = (hipStream_t)stream;
  const hipError_t e = ids16 ? mf_launch_k<uint16_t>(a, lds, st) : mf_launch_k<int>(a, lds, st);
  return e == hipSuccess ? 0 : gkg_fail_hip(e, "mr_fc2_bf16_kernel");
}

}  // namespace gkg
using namespace gkg;

extern "C" int gkg_mr_fc2_bf16_supported(int B, int G, int c, int N, int M, int k, int has_res, int want_f32, int want_bf16, int act) {
  (void)has_res;
  if (B <= 0 || G <= 0 || c <= 0 || N <= 0 || M <= 0 || k <= 0 || k > 64) return 0;
  if ((!want_f32 && !want_bf16) || act < 0 || act > 1) return 0;
  const long long C = (long long)G * c;
  if ((C & 15) || (c & 3) || C > MF_MAXC) return 0;
  if (mf_lds_bytes((int)C, G, k, M <= 65536) > MF_LDS_MAX) return 0;
  return ((long long)B * N + MG_ROWS - 1) / MG_ROWS <= 0x3ffffff0LL ? 1 : 0;       // the grid fits
}

extern "C" int gkg_mr_fc2_bf16(const float* x, const float* src, const int64_t* nn_idx, const void* wplanes, const float* a1,
                               const float* c1, const void* w2planes, const float* a2, const float* c2, const float* res, int ldr,
                               float* out_f32, int ldo32, void* out_bf16, int ldo16, int B, int G, int c, int N, int M, int k, int act,
                               void* stream) {
  return mr_fc2_bf16_impl(x, src, nn_idx, nullptr, wplanes, a1, c1, w2planes, a2, c2, res, ldr, out_f32, ldo32, out_bf16, ldo16, B, G, c,
                          N, M, k, act, stream);
}

// gkg_mr_fc2_bf16 over the compact neighbour lists of gkg_knn_fwd_tm16 (u16 rows, M <= 65 536): same result.
extern "C" int gkg_mr_fc2_bf16_nn16(const float* x, const float* src, const uint16_t* nn16, const void* wplanes, const float* a1,
                                    const float* c1, const void* w2planes, const float* a2, const float* c2, const float* res, int ldr,
                                    float* out_f32, int ldo32, void* out_bf16, int ldo16, int B, int G, int c, int N, int M, int k,
                                    int act, void* stream) {
  return mr_fc2_bf16_impl(x, src, nullptr, nn16, wplanes, a1, c1, w2planes, a2, c2, res, ldr, out_f32, ldo32, out_bf16, ldo16, B, G, c,
                          N, M, k, act, stream);
}
