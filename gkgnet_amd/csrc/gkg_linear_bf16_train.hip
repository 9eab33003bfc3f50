// gkg_linear_bf16_train.hip — training under bf16 autocast (opt-in GKG_ENABLE=train_bf16): the weight gradient of a dense 1x1
// projection, dw (cout, cin) += bf16(dy)^T bf16(x), on v_mfma_f32_32x32x16_bf16 — ONE matrix product with fp32 accumulation where
// gkg_linear_wgrad_x6 runs six for fp32 accuracy.  (The layer's other two products, Y = x W^T and dx = dY W, are
// gkg_linear_bf16_f32a: gkg_linear_bf16.hip.)  Reference layers: Conv2d(1x1) of Grapher.fc1 / fc2 (mmcls/models/backbones/vig_model/
// torch_vertex.py:290-306) and FFN.fc1 / fc2 (mmcls/models/backbones/gkgnet.py:46-72) under mixed precision.
//
// The output is tiny and the contraction (the R rows) long.  One workgroup (4 waves, 2 x 2, each 64 x 64 of the tile: four 32 x 32
// accumulators) owns a 128 (cout) x 128 (cin) tile of dw and ONE slab of rows, and adds its partial tile to dw with fp32 vector
// atomics (global_atomic_add_f32; one accumulator register = two 128-byte segments in two rows per wave-instruction, the full-rate
// shape) — gkg_linear_wgrad_x6's accumulation contract: the caller zeroes dw, the summation order is run-dependent.  The number of
// slabs is chosen so that tiles x slabs reaches WG_TARGET = 512 workgroups (two per CU of 256: what the registers hold) with slabs of at least
// WG_MIN_SLAB = 256 rows (8 chunks: the atomics of a slab stay a small part of it), the slab length a multiple of the chunk.
// Work items are dealt to the XCDs by the map of gkg_linear_bf16.hip: XCD i walks a contiguous range of items, tile fastest, so
// the tiles that read one slab of rows run on one XCD (one L2).
//
// Both operands arrive k-major: a row of dy / x is ONE contraction index, while a lane's MFMA operand is 8 consecutive contraction
// indices of ONE column.  The transposition is done on the way into LDS (the "stash transposed, read with plain 16-byte reads"
// form, not ds_read_b64_tr_b16): per chunk of WG_KC = 32 rows a thread loads an 8-row x 4-column block of its operand (8 x 16 B;
// waves 0-1 dy, waves 2-3 x), rounds it to bf16 in registers (pack_bf16x2, round to nearest even) and writes, per column, the 8
// consecutive rows as ONE 16-byte piece of the image [column][32 rows], column pitch 80 B = 20 dwords.
// LDS bank rules (MI355X_MICROARCH.md, LDS): ds_write_b128 is served in groups of 8 CONTIGUOUS lanes, bank (a / 4) mod 32;
// ds_read_b128 in four 16-lane groups ({0-3, 12-15, 20-27}, ...), bank (a / 4) mod 64.
//   write  the lanes of a wave are dealt row block fastest: lane = 4 cgl + kb (kb: 8-row block 0..3, cgl: 4-column group 0..15 of
//          the wave's 64 columns).  A write group is then 2 column groups x 4 row blocks: for the piece of column 4 cg + j the four
//          kb lanes cover 16 consecutive dwords (one column's 64 bytes), and the second column group lies 4 columns = 80 dwords
//          = 16 mod 32 further: the 8 lanes cover all 32 banks once — conflict-free.  (Dealt column group fastest — lane = cg —
//          the 8 lanes of a group would be 80 dwords apart each, i.e. alternate between two bank quads: 4-way, 32 LDS-array
//          cycles per store against the instruction's 13.  The first form of this kernel did that.)  The price is in the global
//          loads: a wave-instruction reads 4 rows x 256 contiguous bytes instead of 2 x 512.
//   read   lane l31 of a 32 x 32 block reads 16 bytes at column l31, dword 20 l31 + const: 16-byte quad 5 l31 + const mod 16, and
//          the l31 of a 16-lane group are all different mod 16 (5 is odd) — conflict-free, one ds_read_b128 per fragment.
// Against the transposed-read form (a row-major [row][column] bf16 image read with ds_read_b64_tr_b16): that form needs two
// 8-byte transposed reads per fragment where this one issues one ds_read_b128 (same bytes, twice the LDS instructions in the
// MFMA loop), and EXEC all ones as an invariant of every read at partial tiles; its stash would write a thread's block as 8
// ds_write_b64 (4 columns of one row each) against 4 ds_write_b128 here.  Both forms can be made conflict-free on both sides, so
// the choice rests on the instruction counts, not on bank conflicts.
// Pipeline: two register sets, the loads of chunk c + 2 issued before the MFMAs of chunk c (gkg_linear_bf16.hip's scheme: with one
// chunk of look-ahead every chunk waited out a whole memory latency, 1.7 TB/s at the stage-1 shapes), two LDS buffers, ONE
// barrier per chunk.  Partial tiles in all three dimensions: rows outside the slab / >= R and columns >= cout / cin are
// zero-filled on the way in, elements outside dw are never added; nothing is read or written outside the operands.
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   linear_wgrad_bf16_kernel   140 VGPRs, 64 AGPRs (the accumulators), 58 SGPRs   LDS 40 960 B (static)   no scratch   2 waves / SIMD
// by registers (the LDS would hold three workgroups; a launch bound of three costs 152 B of scratch per lane: not taken).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gkg_common.h"

namespace gkg {

typedef float wg_f32x16 __attribute__((ext_vector_type(16)));
typedef __attribute__((__vector_size__(8 * sizeof(__bf16)))) __bf16 wg_bf16x8;

constexpr int WG_T = 128;                          // edge of a workgroup's dw tile (cout rows x cin columns)
constexpr int WG_KC = 32;                          // rows (contraction indices) per LDS chunk: 2 MFMA steps of 16
constexpr int WG_NT = 256;
constexpr int WG_PITCH = WG_KC * 2 + 16;           // bytes per column of an operand image: 32 bf16 + a 16-byte pad
constexpr int WG_OPBYTES = WG_T * WG_PITCH;        // 10 240
constexpr int WG_MIN_SLAB = 256;                   // rows of the shortest slab
constexpr int WG_TARGET = 512;                     // workgroups a launch aims at: two per CU

struct WgradBf16Args {
  const float* dy; int ldg;       // (R, ldg) fp32
  const float* x; int ldx;        // (R, ldx) fp32
  float* dw;                      // (cout, cin) fp32, +=
  int R, cin, cout;
  int tiles_n, tiles;             // cin tiles, all tiles
  int slab_rows;                  // a multiple of WG_KC
  int items, items_per_xcd;       // tiles x slabs
};

__global__ __launch_bounds__(WG_NT) void linear_wgrad_bf16_kernel(WgradBf16Args g) {
  __shared__ __align__(16) unsigned char lds[2][2][WG_OPBYTES];      // [buffer][dy, x][column][32 rows + pad]
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  // XCD-aware map (workgroups are dealt round-robin over the 8 XCDs): XCD i walks items [i * items_per_xcd, ...), tile fastest
  const int lin = blockIdx.x;
  const int il = lin >> 3, item = (lin & 7) * g.items_per_xcd + il;
  if (il >= g.items_per_xcd || item >= g.items) return;
  const int slab = item / g.tiles, tile = item - slab * g.tiles;
  const int tm = tile / g.tiles_n, tn = tile - tm * g.tiles_n;
  const int m0 = tm * WG_T, n0 = tn * WG_T;                          // first cout row / cin column of the tile
  const long long rbeg = (long long)slab * g.slab_rows;
  const long long rend = min((long long)g.R, rbeg + g.slab_rows);
  const int NC = (int)((rend - rbeg + WG_KC - 1) / WG_KC);

  // staging: waves 0-1 take dy, waves 2-3 x; a thread owns rows [8 kb, 8 kb + 8) x columns [4 cg, 4 cg + 4) of its operand's chunk
  const int op = w >> 1;
  const float* src = op ? g.x : g.dy;
  const int ld = op ? g.ldx : g.ldg;
  // (row block fastest over the lanes: the 8 lanes of a ds_write_b128 group are 2 column groups x 4 row blocks — see the header)
  const int kb = lane & 3, cg = 16 * (w & 1) + (lane >> 2);
  const int scol = (op ? n0 : m0) + 4 * cg;
  const bool colok = scol < (op ? g.cin : g.cout);                   // widths are multiples of 8: the 4 columns are in or out together
  // two register sets: the loads of chunk c + 2 are issued before the MFMAs of chunk c, the set holding chunk c + 1 is written to
  // the other LDS buffer after them — a load has two chunks of matrix work (and the CU's other workgroups) to land
  float4 ra[2][8];
  auto fetch = [&](int c, float4 (&rg)[8]) __attribute__((always_inline)) {
    const long long row0 = rbeg + (long long)c * WG_KC + 8 * kb;
#pragma unroll
    for (int i = 0; i < 8; ++i)
      rg[i] = (colok && row0 + i < rend) ? *reinterpret_cast<const float4*>(src + (size_t)(row0 + i) * ld + scol)
                                         : make_float4(0.f, 0.f, 0.f, 0.f);
  };
  auto stash = [&](int buf, const float4 (&rg)[8]) __attribute__((always_inline)) {
    unsigned char* base = &lds[buf][op][0] + (4 * cg) * WG_PITCH + 16 * kb;
    *reinterpret_cast<uint4*>(base) = make_uint4(pack_bf16x2(rg[0].x, rg[1].x), pack_bf16x2(rg[2].x, rg[3].x),
                                                 pack_bf16x2(rg[4].x, rg[5].x), pack_bf16x2(rg[6].x, rg[7].x));
    *reinterpret_cast<uint4*>(base + WG_PITCH) = make_uint4(pack_bf16x2(rg[0].y, rg[1].y), pack_bf16x2(rg[2].y, rg[3].y),
                                                            pack_bf16x2(rg[4].y, rg[5].y), pack_bf16x2(rg[6].y, rg[7].y));
    *reinterpret_cast<uint4*>(base + 2 * WG_PITCH) = make_uint4(pack_bf16x2(rg[0].z, rg[1].z), pack_bf16x2(rg[2].z, rg[3].z),
                                                                pack_bf16x2(rg[4].z, rg[5].z), pack_bf16x2(rg[6].z, rg[7].z));
    *reinterpret_cast<uint4*>(base + 3 * WG_PITCH) = make_uint4(pack_bf16x2(rg[0].w, rg[1].w), pack_bf16x2(rg[2].w, rg[3].w),
                                                                pack_bf16x2(rg[4].w, rg[5].w), pack_bf16x2(rg[6].w, rg[7].w));
  };

  // compute: wave (wm, wn) owns rows [64 wm, 64 wm + 64) x columns [64 wn, 64 wn + 64) of the tile as 2 x 2 blocks of 32 x 32
  const int wm = w & 1, wn = w >> 1;
  const int l31 = lane & 31, kg = lane >> 5;
  bool hasm[2], hasn[2];                                             // wave-uniform: the block meets dw
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    hasm[i] = m0 + 64 * wm + 32 * i < g.cout;
    hasn[i] = n0 + 64 * wn + 32 * i < g.cin;
  }
  wg_f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  auto compute = [&](int buf) __attribute__((always_inline)) {
    const unsigned char* ap = &lds[buf][0][0] + (64 * wm + l31) * WG_PITCH + 16 * kg;
    const unsigned char* bp = &lds[buf][1][0] + (64 * wn + l31) * WG_PITCH + 16 * kg;
#pragma unroll
    for (int s = 0; s < WG_KC / 16; ++s) {
      wg_bf16x8 av[2], bv[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        av[i] = __builtin_bit_cast(wg_bf16x8, *reinterpret_cast<const uint4*>(ap + 32 * i * WG_PITCH + 32 * s));
        bv[i] = __builtin_bit_cast(wg_bf16x8, *reinterpret_cast<const uint4*>(bp + 32 * i * WG_PITCH + 32 * s));
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          if (hasm[i] && hasn[j]) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[i], bv[j], acc[i][j], 0, 0, 0);
    }
  };

  fetch(0, ra[0]);
  if (NC > 1) fetch(1, ra[1]);
  stash(0, ra[0]);
  __syncthreads();
  for (int c = 0; c < NC; c += 2) {
    // chunk c (LDS buffer 0).  A stash targets the buffer the PREVIOUS chunk was read from, behind the barrier that ended it.
    if (c + 2 < NC) fetch(c + 2, ra[0]);
    compute(0);
    if (c + 1 < NC) stash(1, ra[1]);
    __syncthreads();
    if (c + 1 >= NC) break;
    // chunk c + 1 (LDS buffer 1)
    if (c + 3 < NC) fetch(c + 3, ra[1]);
    compute(1);
    if (c + 2 < NC) stash(0, ra[0]);
    __syncthreads();
  }

  // in the 32 x 32 accumulator layout register r of a lane is row (r & 3) + 8 (r >> 2) + 4 kg, column l31 of the block
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = n0 + 64 * wn + 32 * j + l31;
      if (hasm[i] && hasn[j] && col < g.cin) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = m0 + 64 * wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * kg;
          if (row < g.cout) unsafeAtomicAdd(g.dw + (size_t)row * g.cin + col, acc[i][j][r]);
        }
      }
    }
}

// The launch plan for checked sizes; false when the grid would not fit.
static bool wg_plan(WgradBf16Args& g, int R, int cin, int cout) {
  const int tiles_m = (cout + WG_T - 1) / WG_T;
  g.tiles_n = (cin + WG_T - 1) / WG_T;
  const long long tiles = (long long)tiles_m * g.tiles_n;
  if (tiles > 0x3fffffffLL) return false;
  g.tiles = (int)tiles;
  const long long want = (WG_TARGET + tiles - 1) / tiles;                             // >= 1
  const long long most = ((long long)R + WG_MIN_SLAB - 1) / WG_MIN_SLAB;             // >= 1
  long long slabs = want < most ? want : most;
  const long long rows = (((long long)R + slabs - 1) / slabs + WG_KC - 1) / WG_KC * WG_KC;
  slabs = ((long long)R + rows - 1) / rows;
  if (tiles * slabs > 0x3fffffffLL) return false;
  g.slab_rows = (int)rows;
  g.items = (int)(tiles * slabs);
  g.items_per_xcd = (g.items + 7) / 8;
  return true;
}

}  // namespace gkg
using namespace gkg;

extern "C" int gkg_linear_wgrad_bf16_supported(int R, int cin, int cout) {
  if (R > 0x7fffffff - WG_KC) return 0;                          // the slab length (R rounded up to a chunk) must fit an int
  if (R < 1 || cin <= 0 || cout <= 0 || (cin & 7) || (cout & 7) || cin > (1 << 24) || cout > (1 << 24)) return 0;
  WgradBf16Args g;
  return wg_plan(g, R, cin, cout) ? 1 : 0;
}

extern "C" int gkg_linear_wgrad_bf16(const float* dy, int ldg, const float* x, int ldx, float* dw, int R, int cin, int cout,
                                     void* stream) {
  if (!dy || !x || !dw) return gkg_fail(GKG_ERR_NULL, "gkg_linear_wgrad_bf16: null pointer");
  if (R < 1 || cin <= 0 || cout <= 0) return gkg_fail(GKG_ERR_SHAPE, "gkg_linear_wgrad_bf16: bad sizes (need R >= 1, cin, cout > 0)");
  WgradBf16Args g;
  if (!gkg_linear_wgrad_bf16_supported(R, cin, cout) || !wg_plan(g, R, cin, cout))
    return gkg_fail(GKG_ERR_UNSUPPORTED, "gkg_linear_wgrad_bf16: need cin % 8 == 0, cout % 8 == 0 and a grid that fits");
  if ((ldg & 3) || (ldx & 3)) return gkg_fail(GKG_ERR_UNSUPPORTED, "gkg_linear_wgrad_bf16: need ldg % 4 == 0, ldx % 4 == 0");
  if (((uintptr_t)dy | (uintptr_t)x | (uintptr_t)dw) & 15)
    return gkg_fail(GKG_ERR_UNSUPPORTED, "gkg_linear_wgrad_bf16: dy, x and dw must be 16-byte aligned");
  if (ldg < cout || ldx < cin) return gkg_fail(GKG_ERR_UNSUPPORTED, "gkg_linear_wgrad_bf16: a row pitch is below the row's width");
  g.dy = dy; g.ldg = ldg; g.x = x; g.ldx = ldx; g.dw = dw; g.R = R; g.cin = cin; g.cout = cout;
  hipLaunchKernelGGL(linear_wgrad_bf16_kernel, dim3((unsigned)(g.items_per_xcd * 8)), dim3(WG_NT), 0, (hipStream_t)stream, g);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : gkg_fail_hip(e, "linear_wgrad_bf16_kernel");
}
