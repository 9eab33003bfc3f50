// gkg_ffn_bf16.hip — bf16 inference: an FFN (fc1 + BN + GELU, fc2 + BN + residual) as ONE kernel; the (R, hid) hidden matrix
// never exists in memory.
//
// Reference layers (mmcls/models/backbones/gkgnet.py:46-72 FFN.fc1 / act / fc2 / shortcut) under bf16 autocast with gradients
// off.  As two launches of gkg_linear_bf16 (csrc/gkg_linear_bf16.hip) the bf16 hidden matrix, 4x the width of the block's input,
// is written by the first and read back by the second; here a workgroup keeps the slice of it that it needs in LDS.
//
// One workgroup of 4 waves owns a row tile and ALL cout <= 192 columns.  Two forms (template parameter CS, waves per group of 32 rows):
//   narrow (CS 1: cin <= 96 and cout <= 96, the stage-1 widths)   128-row tile, wave w takes rows [32 w, 32 w + 32) x every column;
//   wide   (CS 2: everything else up to 192)                       64-row tile, a PAIR of waves shares 32 rows: each takes one of a
//          chunk's two hidden blocks in GEMM 1 and half of the output blocks in GEMM 2 — a wave's accumulators halve (48 + 16
//          registers at cout 192 instead of 96 + 32), which is what lets two workgroups share a CU at these widths.
//   x          a wave's 32 rows are loaded once, straight into the A-operand layout (lane = row, 8 consecutive channels per
//              16-byte register group), and stay in registers: NS1 <= 12 MFMA steps of 16 channels (cin <= 192).
//   main loop  the hidden is walked in chunks of 64 columns.  Per chunk and group of 32 rows
//                GEMM 1   x (32 x cin) . W1 chunk (cin x 64) -> a 32 x 64 accumulator (2 blocks), all of cin, ascending steps;
//                epi 1    h = bf16(act(fma(a1, acc, c1))) — the hidden element exactly as gkg_linear_bf16 would have stored it —
//                         into the group's LDS slab (32 rows x 64 columns, pitch 144 B).  In the accumulator layout a lane owns a
//                         COLUMN, the A operand wants a ROW per lane: the slab is that transposition.  Only the group's own waves
//                         read it back: a wave barrier (narrow) or one workgroup barrier (wide).  Hidden columns >= hid are written
//                         as zeros (a1 / c1 are not read there);
//                GEMM 2   slab (32 x 64) . W2 chunk (64 x cout) accumulated into the group's 32 x cout output accumulators (NO <= 6
//                         blocks), ascending steps — over all chunks the contraction order of the second launch.
//              The W1 / W2 fragments and the BN vectors of chunk j + 1 go global -> registers before the MFMAs of chunk j and into
//              LDS after them: the other buffer and ONE workgroup barrier per chunk (narrow), the same buffer between two barriers
//              (wide: 58 KB of LDS per workgroup instead of 117).
//   epilogue   gkg_linear_bf16's: z = fma(a2, acc, c2) staged in the (now free) LDS, walked as 8-column segments: residual read
//              as 2 x float4 (all of a lane's segments issued up front), fp32 result stored as 2 x 16 B, bf16 result as 16 B.
// Both contractions run v_mfma_f32_32x32x16_bf16 over ascending 16-element steps and run exactly the steps of the padded
// contraction, as the two launches do; the hidden goes through the same gelu_f / pack_bf16x2: every output bit is that of
//   gkg_linear_bf16(x, .., w1planes, a1, c1, no residual, bf16 h (R, hid), act)  ->  gkg_linear_bf16(h, .., w2planes, a2, c2, res, ..)
// in either form (an output element's two contractions run in the same order in both).
// Workgroups are dealt to the XCDs so that each XCD walks a contiguous range of row tiles.  No workgroup waits for another: no
// counters, no flags.  Partial tiles in every dimension: rows >= R, channels >= cin, hidden columns >= hid and output columns >=
// cout are zero-filled on the way in and never stored on the way out; nothing is read or written outside the operands.
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; no scratch in any, 0 AGPRs in all):
//   ffn_bf16_kernel<NO, NS1, CS>   cin <=  cout <=   VGPRs  SGPRs   LDS (dynamic)   workgroups / CU: registers, LDS   waves / SIMD
//   <3,  6, 1>  narrow                96      96      195     75       67 584 B                2, 2                      2
//   <6,  6, 2>  wide                  96     192      212     84       50 176 B                2, 3                      2
//   <6, 12, 2>  wide                 192     192      254     90       58 368 B                2, 2                      2
// (The wide form always carries six output blocks: at cout 160 the sixth is zero fragments, never stored.)
// How it got here, MI355X, fused against the pair of launches (tools/bench_lin_bf16.py --ffn; EXPERIMENTS.md "Fused bf16 FFN"):
// with a guard per MFMA step and the BN vectors loaded inside the chunk the wide shapes lost 24-29 % (every step its own
// scheduling region, a vmcnt(0) for two floats that also waited for the whole prefetch); straight-line steps and prefetched
// vectors made them even; the wide form (two workgroups per CU: one's memory phases beside the other's MFMAs, the GELU free)
// took another 29 % off.  The narrow widths through a wide form (four output blocks) measured 4 % slower than the narrow form: kept apart.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "gkg_common.h"

namespace gkg {

typedef float ff_f32x16 __attribute__((ext_vector_type(16)));
typedef __attribute__((__vector_size__(8 * sizeof(__bf16)))) __bf16 ff_bf16x8;

constexpr int FF_HC = 64;                        // hidden columns per chunk (2 blocks of GEMM 1, 4 MFMA steps of GEMM 2)
constexpr int FF_NT = 256;
constexpr int FF_SPITCH = (FF_HC + 8) * 2;       // bytes per slab row: conflict-free 16-byte reads
constexpr int FF_SLAB = 32 * FF_SPITCH;          // one wave's slab: 4 608 B
constexpr int FF_MAXC = 192;                     // widest cin / cout

struct FfnBf16Args {
  const uint16_t* x; int ldx;                    // (R, ldx) bf16
  const uint4* w1; const float* a1; const float* c1;    // [ci1 / 8][hp32] fragments; [hid] or null (= 1); [hid]
  const uint4* w2; const float* a2; const float* c2;    // [hp16 / 8][co2] fragments; [cout] or null (= 1); [cout]
  const float* res; int ldr;                     // (R, ldr) fp32 or null
  float* o32; int ldo32;                         // (R, ldo32) or null
  uint16_t* o16; int ldo16;                      // (R, ldo16) bf16 or null
  int R, cin, hid, cout, act;
  int ci1, hp32, hp16, co2;                      // the fragment arrays' paddings: cin -> 16, hid -> 32 (W1 columns) / 16 (W2 rows), cout -> 32
  int tiles, tiles_per_xcd;
};

constexpr int ff_w1_bytes(int NS1) { return 2 * NS1 * FF_HC * 16; }
constexpr int ff_w2_bytes(int NO) { return (FF_HC / 8) * 32 * NO * 16; }
constexpr int ff_stage_bytes(int NO, int CS) { return (4 / CS) * 32 * (32 * NO + 4) * 4; }
constexpr size_t ff_lds_bytes(int NO, int NS1, int CS) {
  const int loop = (CS == 1 ? 2 : 1) * (ff_w1_bytes(NS1) + ff_w2_bytes(NO)) + (4 / CS) * FF_SLAB;
  return (size_t)(loop > ff_stage_bytes(NO, CS) ? loop : ff_stage_bytes(NO, CS));
}

// NO: output column blocks of 32 (cout padded to 32 <= 32 NO); NS1: MFMA steps GEMM 1 has registers for (cin padded to 16 <= 16 NS1);
// CS: waves that share a group of 32 rows (1: the narrow form, 128-row tile, W double-buffered; 2: the wide form, 64-row tile, each
// wave of a pair takes one of the chunk's two hidden blocks and half of the output blocks, W single-buffered — a workgroup's
// registers and LDS halve, two workgroups fit a CU)
template <int NO, int NS1, int CS>
__global__ __launch_bounds__(FF_NT, 2) void ffn_bf16_kernel(FfnBf16Args g) {
  extern __shared__ __align__(16) unsigned char ff_lds[];
  constexpr int BN = 32 * NO;
  constexpr int RG = 4 / CS;                             // groups of 32 rows per workgroup
  constexpr int BM = 32 * RG;                            // rows per workgroup
  constexpr int UB = 2 / CS;                             // hidden blocks of a chunk per wave
  constexpr int VB = NO / CS;                            // output blocks per wave
  constexpr int NBUF = CS == 1 ? 2 : 1;
  constexpr int W1B = ff_w1_bytes(NS1), W2B = ff_w2_bytes(NO);
  constexpr int NW1 = 2 * NS1 * FF_HC / FF_NT;           // W1 granules (16 B) per thread and chunk: NS1 / 2
  constexpr int NW2 = (FF_HC / 8) * BN / FF_NT;          // W2 granules per thread and chunk: NO
  constexpr int SP = BN + 4;                             // floats per row of a row group's epilogue stage
  static_assert((NS1 == 6 || NS1 == 12) && (CS == 1 || CS == 2) && NO % CS == 0 && 16 * NS1 <= FF_MAXC && BN <= FF_MAXC,
                "tile form out of the envelope");
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int rw = w / CS, cp = w % CS;                    // the wave's row group and its column part
  // XCD-aware map (workgroups are dealt round-robin over the 8 XCDs): XCD i walks row tiles [i * tiles_per_xcd, ...)
  const int lin = blockIdx.x;
  const int tl = lin >> 3, tile = (lin & 7) * g.tiles_per_xcd + tl;
  if (tl >= g.tiles_per_xcd || tile >= g.tiles) return;
  const long long r0 = (long long)tile * BM + 32 * rw;   // the wave's first row
  unsigned char* w1buf = ff_lds;                         // [NBUF][2 NS1][64][16 B]
  unsigned char* w2buf = ff_lds + NBUF * W1B;            // [NBUF][8][BN][16 B]
  unsigned char* slab = ff_lds + NBUF * (W1B + W2B) + rw * FF_SLAB;  // this row group's [32][144 B]
  // the two syncs of a row group's waves: around the slab and around the epilogue stage
  auto group_sync = [&]() __attribute__((always_inline)) {
    if constexpr (CS == 1) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    } else {
      __syncthreads();
    }
  };

  const int S1 = g.ci1 >> 4, S2 = g.hp16 >> 4;           // MFMA steps of the two contractions
  const int nf1 = g.ci1 >> 3, nf2 = g.hp16 >> 3;         // fragment rows of the two arrays
  const int NCH = (g.hp32 + FF_HC - 1) / FF_HC;
  const int l31 = lane & 31, kg = lane >> 5;

  // the wave's x rows as A operands: step s, lane (row l31, half kg) holds channels [16 s + 8 kg, + 8)
  uint4 xa[NS1];
  {
    const long long row = r0 + l31;
    const uint16_t* xp = g.x + (size_t)(row < g.R ? row : 0) * g.ldx + 8 * kg;
#pragma unroll
    for (int s = 0; s < NS1; ++s)
      xa[s] = (row < g.R && 16 * s + 8 * kg < g.cin) ? *reinterpret_cast<const uint4*>(xp + 16 * s) : make_uint4(0, 0, 0, 0);
  }

  // W1 / W2 fragments and the wave's blocks' BN scale / shift of the NEXT chunk: loaded a whole chunk before they are needed, so
  // that no wait for them falls between the MFMAs (a lane owns one hidden column per block: one register each)
  uint4 q1[NW1], q2[NW2];
  float qa[UB], qc[UB];
  auto fetch = [&](int j) __attribute__((always_inline)) {
    const int h0 = j * FF_HC;
#pragma unroll
    for (int u = 0; u < UB; ++u) {
      const int col = h0 + 32 * (cp * UB + u) + l31;
      qc[u] = col < g.hid ? g.c1[col] : 0.f;
      qa[u] = (g.a1 && col < g.hid) ? g.a1[col] : 1.f;
    }
#pragma unroll
    for (int i = 0; i < NW1; ++i) {
      const int gi = tid + FF_NT * i;
      const int f = gi / FF_HC, n = h0 + (gi % FF_HC);
      q1[i] = (f < nf1 && n < g.hp32) ? g.w1[(size_t)f * g.hp32 + n] : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < NW2; ++i) {
      const int gi = tid + FF_NT * i;
      const int f = (h0 >> 3) + gi / BN, n = gi % BN;
      q2[i] = (f < nf2 && n < g.co2) ? g.w2[(size_t)f * g.co2 + n] : make_uint4(0, 0, 0, 0);
    }
  };
  auto stash = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NW1; ++i) *reinterpret_cast<uint4*>(w1buf + buf * W1B + 16 * (tid + FF_NT * i)) = q1[i];
#pragma unroll
    for (int i = 0; i < NW2; ++i) *reinterpret_cast<uint4*>(w2buf + buf * W2B + 16 * (tid + FF_NT * i)) = q2[i];
  };

  ff_f32x16 acc2[VB];
#pragma unroll
  for (int v = 0; v < VB; ++v)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc2[v][r] = 0.f;

  // epilogue 1 of one 32-column block (u: its index in the chunk): the hidden element as the first launch rounds it, zeros beyond hid
  auto hidden = [&](const ff_f32x16& acc, int col, int u, float av, float cv, bool scaled, bool gelu) __attribute__((always_inline)) {
    const bool in = col < g.hid;
    unsigned char* sp = slab + 2 * (32 * u + l31);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = (r & 3) + 8 * (r >> 2) + 4 * kg;
      float z = scaled ? __builtin_fmaf(av, acc[r], cv) : acc[r] + cv;
      if (gelu) z = gelu_f(z);
      *reinterpret_cast<uint16_t*>(sp + row * FF_SPITCH) = in ? (uint16_t)pack_bf16x2(z, 0.f) : (uint16_t)0;
    }
  };

  fetch(0);
  stash(0);
  float ca[UB], cc[UB];                                  // the current chunk's scale / shift
#pragma unroll
  for (int u = 0; u < UB; ++u) { ca[u] = qa[u]; cc[u] = qc[u]; }
  __syncthreads();
  for (int j = 0; j < NCH; ++j) {
    const int buf = NBUF == 2 ? (j & 1) : 0;
    const int h0 = j * FF_HC;
    if (j + 1 < NCH) fetch(j + 1);
    // ---- GEMM 1: 32 rows x the wave's hidden blocks of the chunk, over all of cin
    ff_f32x16 acc1[UB];
#pragma unroll
    for (int u = 0; u < UB; ++u)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc1[u][r] = 0.f;
    {
      // exactly the S1 steps of the padded contraction (the first launch runs no other), as straight-line code per step count:
      // the x fragments are registers, and a guard per step would end the scheduling region at every step
      const unsigned char* bp = w1buf + buf * W1B + (kg * FF_HC + 32 * cp * UB + l31) * 16;
      auto gemm1 = [&](auto steps) __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < decltype(steps)::value; ++s) {
          const ff_bf16x8 av = __builtin_bit_cast(ff_bf16x8, xa[s]);
#pragma unroll
          for (int u = 0; u < UB; ++u) {
            const ff_bf16x8 bv = __builtin_bit_cast(ff_bf16x8, *reinterpret_cast<const uint4*>(bp + (2 * s * FF_HC + 32 * u) * 16));
            acc1[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, acc1[u], 0, 0, 0);
          }
        }
      };
      switch (S1) {                                      // NS1 - 6 < S1 <= NS1 (the launcher picks NS1 so)
        case NS1: gemm1(std::integral_constant<int, NS1>{}); break;
        case NS1 - 1: gemm1(std::integral_constant<int, NS1 - 1>{}); break;
        case NS1 - 2: gemm1(std::integral_constant<int, NS1 - 2>{}); break;
        case NS1 - 3: gemm1(std::integral_constant<int, NS1 - 3>{}); break;
        case NS1 - 4: gemm1(std::integral_constant<int, NS1 - 4>{}); break;
        default: gemm1(std::integral_constant<int, NS1 - 5>{}); break;
      }
    }
    // ---- epilogue 1 into the row group's slab (the mode tests once per chunk, not per element)
#pragma unroll
    for (int u = 0; u < UB; ++u) {
      const int ub = cp * UB + u;
      const int col = h0 + 32 * ub + l31;
      if (g.a1) {
        if (g.act == 1) hidden(acc1[u], col, ub, ca[u], cc[u], true, true); else hidden(acc1[u], col, ub, ca[u], cc[u], true, false);
      } else {
        if (g.act == 1) hidden(acc1[u], col, ub, 1.f, cc[u], false, true); else hidden(acc1[u], col, ub, 1.f, cc[u], false, false);
      }
    }
    group_sync();                                        // the slab is complete
    // ---- GEMM 2: the chunk's 4 steps of the second contraction (those inside hid padded to 16), the wave's output blocks
    {
      const unsigned char* ap = slab + l31 * FF_SPITCH + 16 * kg;
      const unsigned char* bp = w2buf + buf * W2B + (kg * BN + 32 * cp * VB + l31) * 16;
      auto step = [&](int s) __attribute__((always_inline)) {
        const ff_bf16x8 av = __builtin_bit_cast(ff_bf16x8, *reinterpret_cast<const uint4*>(ap + 32 * s));
#pragma unroll
        for (int v = 0; v < VB; ++v) {
          const ff_bf16x8 bv = __builtin_bit_cast(ff_bf16x8, *reinterpret_cast<const uint4*>(bp + (2 * s * BN + 32 * v) * 16));
          acc2[v] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, acc2[v], 0, 0, 0);
        }
      };
      const int steps = min(FF_HC / 16, S2 - (h0 >> 4));
      if (steps == FF_HC / 16) {
        // a full chunk: straight-line code, a step's fragment reads issue under the MFMAs of the one before
#pragma unroll
        for (int s = 0; s < FF_HC / 16; ++s) step(s);
      } else {
        for (int s = 0; s < steps; ++s) step(s);         // the last chunk of a hidden that is no multiple of 64
      }
    }
    if constexpr (NBUF == 1) __syncthreads();            // one buffer: every wave is done with this chunk's fragments and slabs
    if (j + 1 < NCH) {
      stash(NBUF == 2 ? (buf ^ 1) : 0);
#pragma unroll
      for (int u = 0; u < UB; ++u) { ca[u] = qa[u]; cc[u] = qc[u]; }
    }
    if (NBUF == 2 || j + 1 < NCH) __syncthreads();       // the next chunk's fragments are complete (two buffers: and this one, the slabs, free)
  }

  // ---------------------------------------------------------------- epilogue 2 (the last barrier freed the whole LDS)
  float* st = reinterpret_cast<float*>(ff_lds) + rw * 32 * SP;         // this row group's 32 rows x BN columns
  auto affine = [&](bool scaled) __attribute__((always_inline)) {
#pragma unroll
    for (int v = 0; v < VB; ++v) {
      const int col = 32 * (cp * VB + v) + l31;
      if (col < g.cout) {
        const float cv = g.c2[col];
        const float av = scaled ? g.a2[col] : 1.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = (r & 3) + 8 * (r >> 2) + 4 * kg;
          st[row * SP + col] = scaled ? __builtin_fmaf(av, acc2[v][r], cv) : acc2[v][r] + cv;
        }
      }
    }
  };
  if (g.a2) affine(true); else affine(false);
  group_sync();
  // The row group's 32 rows are walked as 8-column segments, 2 NO / CS per lane.  The accumulators are dead by now: ALL of a lane's
  // residual loads are issued before the first is used — one memory round trip per tile instead of one per segment.
  constexpr int NG = BN / 8;                                           // 8-column segments per row
  constexpr int NSEG = 32 * NG / (64 * CS);                            // segments per lane
  float4 p0[NSEG], p1[NSEG];
  if (g.res) {
#pragma unroll
    for (int i = 0; i < NSEG; ++i) {
      const int it = lane + 64 * (cp + CS * i);
      const int rl = it / NG, col = 8 * (it % NG);
      const long long row = r0 + rl;
      if (row < g.R && col < g.cout) {
        const float* rp = g.res + (size_t)row * g.ldr + col;
        p0[i] = *reinterpret_cast<const float4*>(rp);
        p1[i] = *reinterpret_cast<const float4*>(rp + 4);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < NSEG; ++i) {
    const int it = lane + 64 * (cp + CS * i);
    const int rl = it / NG, col = 8 * (it % NG);
    const long long row = r0 + rl;
    if (row < g.R && col < g.cout) {
      float4 z0 = *reinterpret_cast<const float4*>(st + rl * SP + col);
      float4 z1 = *reinterpret_cast<const float4*>(st + rl * SP + col + 4);
      if (g.res) {
        z0.x += p0[i].x; z0.y += p0[i].y; z0.z += p0[i].z; z0.w += p0[i].w;
        z1.x += p1[i].x; z1.y += p1[i].y; z1.z += p1[i].z; z1.w += p1[i].w;
      }
      if (g.o32) {
        float* op = g.o32 + (size_t)row * g.ldo32 + col;
        *reinterpret_cast<float4*>(op) = z0;
        *reinterpret_cast<float4*>(op + 4) = z1;
      }
      if (g.o16)
        *reinterpret_cast<uint4*>(g.o16 + (size_t)row * g.ldo16 + col) =
            make_uint4(pack_bf16x2(z0.x, z0.y), pack_bf16x2(z0.z, z0.w), pack_bf16x2(z1.x, z1.y), pack_bf16x2(z1.z, z1.w));
    }
  }
}

template <int NO, int NS1, int CS>
static hipError_t ff_launch(FfnBf16Args& g, hipStream_t st) {
  constexpr size_t lds = ff_lds_bytes(NO, NS1, CS);
  static_assert(2 * lds <= 160 * 1024, "two workgroups' LDS must fit the CU");
  constexpr int BM = 32 * (4 / CS);
  g.tiles = (int)(((long long)g.R + BM - 1) / BM);
  g.tiles_per_xcd = (g.tiles + 7) / 8;
  if (lds > 64 * 1024) {
    const hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void*>(&ffn_bf16_kernel<NO, NS1, CS>),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (ea != hipSuccess) return ea;
  }
  hipLaunchKernelGGL((ffn_bf16_kernel<NO, NS1, CS>), dim3((unsigned)(g.tiles_per_xcd * 8)), dim3(FF_NT), lds, st, g);
  return hipGetLastError();
}

// The paddings of the two fragment arrays (gkg_linear_bf16_planes_bytes: contraction to 16, output columns to 32)
static inline int ff_pad16(int n) { return (n + 15) & ~15; }
static inline int ff_pad32(int n) { return (n + 31) & ~31; }

}  // namespace gkg
using namespace gkg;

extern "C" int gkg_ffn_bf16_supported(int R, int cin, int hid, int cout, int has_res, int want_f32, int want_bf16, int act) {
  (void)has_res;
  if (R < 1 || cin <= 0 || hid <= 0 || cout <= 0 || (cin & 7) || (hid & 7) || (cout & 7)) return 0;
  if (cin > FF_MAXC || cout > FF_MAXC || hid > (1 << 24)) return 0;
  if ((!want_f32 && !want_bf16) || act < 0 || act > 1) return 0;
  return ((long long)R + 63) / 64 <= 0x3ffffff0LL ? 1 : 0;      // 64-row tiles at the least: the grid fits
}

extern "C" int gkg_ffn_bf16(const void* x, int ldx, const void* w1planes, const float* a1, const float* c1, const void* w2planes,
                            const float* a2, const float* c2, const float* res, int ldr, float* out_f32, int ldo32, void* out_bf16,
                            int ldo16, int R, int cin, int hid, int cout, int act, void* stream) {
  if (!x || !w1planes || !c1 || !w2planes || !c2 || (!out_f32 && !out_bf16)) return gkg_fail(GKG_ERR_NULL, "gkg_ffn_bf16: null pointer");
  if (R < 1 || cin <= 0 || hid <= 0 || cout <= 0 || act < 0 || act > 1)
    return gkg_fail(GKG_ERR_SHAPE, "gkg_ffn_bf16: bad sizes (need R >= 1, cin, hid, cout > 0, act in 0..1)");
  if (!gkg_ffn_bf16_supported(R, cin, hid, cout, res != nullptr, out_f32 != nullptr, out_bf16 != nullptr, act))
    return gkg_fail(GKG_ERR_UNSUPPORTED, "gkg_ffn_bf16: need cin, hid, cout % 8 == 0, cin <= 192, cout <= 192 and a grid that fits");
  if ((ldx & 7) || (out_bf16 && (ldo16 & 7)) || (out_f32 && (ldo32 & 3)) || (res && (ldr & 3)))
    return gkg_fail(GKG_ERR_UNSUPPORTED, "gkg_ffn_bf16: need ldx % 8 == 0, ldo16 % 8 == 0, ldo32 % 4 == 0, ldr % 4 == 0");
  if (((uintptr_t)x | (uintptr_t)w1planes | (uintptr_t)w2planes | (uintptr_t)res | (uintptr_t)out_f32 | (uintptr_t)out_bf16) & 15)
    return gkg_fail(GKG_ERR_UNSUPPORTED, "gkg_ffn_bf16: x, the fragment arrays, res and the outputs must be 16-byte aligned");
  if (ldx < cin || (out_bf16 && ldo16 < cout) || (out_f32 && ldo32 < cout) || (res && ldr < cout))
    return gkg_fail(GKG_ERR_SHAPE, "gkg_ffn_bf16: a row pitch is below the row's width");
  FfnBf16Args g;
  g.x = (const uint16_t*)x; g.ldx = ldx;
  g.w1 = (const uint4*)w1planes; g.a1 = a1; g.c1 = c1;
  g.w2 = (const uint4*)w2planes; g.a2 = a2; g.c2 = c2;
  g.res = res; g.ldr = ldr; g.o32 = out_f32; g.ldo32 = ldo32; g.o16 = (uint16_t*)out_bf16; g.ldo16 = ldo16;
  g.R = R; g.cin = cin; g.hid = hid; g.cout = cout; g.act = act;
  g.ci1 = ff_pad16(cin); g.hp32 = ff_pad32(hid); g.hp16 = ff_pad16(hid); g.co2 = ff_pad32(cout);
  hipStream_t st = (hipStream_t)stream;
  const int no = g.co2 / 32;
  hipError_t e;
  if (g.ci1 <= 96 && no <= 3) e = ff_launch<3, 6, 1>(g, st);                     // the narrow form: stage-1 widths
  else if (g.ci1 <= 96) e = ff_launch<6, 6, 2>(g, st);
  else e = ff_launch<6, 12, 2>(g, st);
  return e == hipSuccess ? 0 : gkg_fail_hip(e, "ffn_bf16_kernel");
}
