// gkg_linear_bf16.hip — bf16 inference: a dense 1x1 projection (Conv2d 1x1 + eval-mode BN [+ GELU] [+ residual]) as ONE kernel.
// (F32A below: the same kernel with an fp32 A operand, a training layer's forward and input gradient under bf16 autocast.)
//
// Reference layers (mmcls/models/backbones/vig_model/torch_vertex.py:290-306 Grapher.fc1 / fc2, mmcls/models/backbones/gkgnet.py:46-72
// FFN.fc1 / fc2, torch_nn.py:57-69) under bf16 autocast with gradients off.  The library-GEMM form of these layers is
// (GEMM with a bias epilogue) for fc1 and (GEMM -> fp32 (T, cout) matrix in memory -> gkg_affine_act_dual) for the layers with a
// residual; here the BN scale / shift, the GELU, the fp32 residual add and BOTH output precisions (the fp32 residual stream and the
// bf16 operand of the next projection) are the GEMM's epilogue: the pre-BN matrix never exists in memory.
//
// One workgroup (4 waves, stacked on rows) owns a 128-row x (32 NB)-column tile, NB = 4 or 2:
//   main loop  contraction chunks of 64: the A rows (already bf16: no split, no conversion) and the B fragments ([ci_pad/8][co_pad][8]
//              planes: 16 B x (32 NB) contiguous pieces per fragment row) go global -> registers -> LDS, double-buffered, the loads
//              of chunk c + 2 issued before the MFMAs of chunk c (two register sets), ONE barrier per chunk;
//              v_mfma_f32_32x32x16_bf16, wave w takes rows [32 w, 32 w + 32) x NB column blocks.  A rows have a 16-byte pad
//              (pitch 144 B): conflict-free 16-byte reads.
//   epilogue   in the 32x32 accumulator layout a lane owns ONE column per block: a[n] / cshift[n] are one register each.
//              z = act(fma(a, acc, c)) goes to the (now free) LDS, each wave into its own quarter; the wave then walks its 32 rows as
//              8-column segments: residual read as 2 x float4, fp32 result stored as 2 x 16 B, bf16 result as 16 B.
// Workgroups are dealt to the XCDs so that each XCD (own L2) walks a contiguous range of tiles, the column tiles of one row tile
// adjacent: the A rows are read from memory once.  Partial tiles in every dimension: rows >= R, columns >= cout and contraction
// granules >= cin are zero-filled on the way in and never stored on the way out; nothing is read or written outside the operands.
//
// Resource usage (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; no scratch in either):
//   linear_bf16_kernel<4>  128 x 128 tile   234 VGPRs, 0 AGPRs, 66 SGPRs   LDS 69 632 B (dynamic)   2 waves / SIMD by registers
//   linear_bf16_kernel<2>  128 x  64 tile   152 VGPRs, 0 AGPRs, 62 SGPRs   LDS 53 248 B (dynamic)   3 waves / SIMD by registers
// The LDS allows 2 (<4>) / 3 (<2>) workgroups of 4 waves per CU, i.e. the same 2 / 3 waves per SIMD: registers and LDS agree.
// (The straight-line chunk body and the edge-tile body keep separate accumulator registers: 138 / 94 VGPRs before them, at
// 5–10 % more time per layer.)
//
// PREP = true (gkg_linear_bf16_knn_prep: a Grapher's fc1, fp32 result only): the same tiling, accumulation order and epilogue, then
// the launch also prepares its output as the QUERIES of the k-NN call behind it (gkg_knn_prep.h: token_prep_coop_body — the ordered
// chains need a token's whole group, c = 12 .. 320 channels, which a column tile holds only for the narrowest layers).  Where one
// column tile covers all of cout, the workgroup prepares the rows it has just stored.  Otherwise every workgroup stores its tile
// write-through, drains the stores, meets and counts its arrival in a per-row-tile counter; the LAST of a row tile's column tiles
// acquires, re-arms the counter (zero on entry, zero on exit: no memset per call) and walks the tile's rows — per image the tile meets, per
// group, TK = 64 / 32 / 16 tokens at a time (c <= 192 / 384 / 600: c (TK + 1) floats in the operand LDS, free by then), reading the
// rows back from `out` (just written by the same XCD's neighbours where the column tiles are adjacent).  Where the k-NN call's
// plan has prefilter planes, the tile's hi / lo planes follow from the normalised tile in LDS, and the row tile that holds an
// image's last token writes that image's pad rows: one writer per (b, g).  Narrow groups (c <= 52: c x 256 floats fit) take
// token_prep_flat_rows instead: one thread per (row, group) pair and no barrier, one pass per two groups.  Measured (MI355X,
// tools/bench_lin_bf16.py --prep; the rule and its table: linear_bf16.py prep_pays): it pays where one column tile holds every
// group and the groups are narrow — the stage-1 shapes, fc1 94 -> 220 us against a 145 us preparation launch — and loses wherever
// a last arrival works alone behind its neighbours.  The plan (workspace offsets, cpad, planes or not) is
// knn_plan's own (gkg_knn_plan.h, through knn_query_prep_plan), nothing of it is restated here.
//   linear_bf16_kernel<4, true>   237 VGPRs, 0 AGPRs, 106 SGPRs   same LDS, no scratch   2 waves / SIMD
//   linear_bf16_kernel<2, true>   155 VGPRs, 0 AGPRs, 106 SGPRs   same LDS, no scratch   3 waves / SIMD
// The non-PREP instantiations are unchanged by the parameter (234 / 66 and 152 / 62 as above).
//
// F32A = true (gkg_linear_bf16_f32a: training under bf16 autocast, where the activations and gradients stay fp32): x is fp32
// (R, ldx); a granule of 8 floats is fetched as two 16-byte loads and rounded to bf16 (pack_bf16x2, round to nearest even) when
// it is stashed, so the LDS image, the contraction order and the epilogue — and with them every output bit — are those of the
// bf16 kernel on x.to(bf16).  The staged A registers double (32 -> 64 with the two chunks of look-ahead kept), which the <4> form
// (234 VGPRs) cannot take without scratch: this entry point runs the 64-column form at EVERY shape (the tile form changes no
// bit: an output element's contraction runs in the same order in both), look-ahead unchanged.
//   linear_bf16_kernel<2, false, true>   186 VGPRs, 0 AGPRs, 62 SGPRs   LDS 53 248 B (dynamic), no scratch   2 waves / SIMD by registers
// The other four instantiations keep their figures (234 / 66, 152 / 62, 237 / 106, 155 / 106).
//
// E = LbElem::F16 (gkg_linear_f16_f32a: training under fp16 autocast, GKG_ENABLE=train_f16): the fp32-A 64-column form with IEEE fp16
// in the places where the element kind shows — the stash packs with pack_f16x2 (round to nearest even, overflow to inf, subnormals
// kept), the fragments are _Float16 x 8 for v_mfma_f32_32x32x16_f16 (the bf16 instruction's rate and lane maps), the 16-bit output
// is fp16.  Fragment layout, LDS pitches, look-ahead, barriers, zero-fill, tile map, epilogue and refusals are the shared code.
//   linear_bf16_kernel<2, false, true, LbElem::F16>   184 VGPRs, 0 AGPRs, 62 SGPRs   LDS 53 248 B (dynamic), no scratch   2 waves / SIMD
// The five bf16 instantiations keep their figures with the parameter (234 / 66, 152 / 62, 237 / 106, 155 / 106, 186 / 62).
//
// GROUPED = true (gkg_linear_bf16_f32a_grouped / gkg_linear_f16_f32a_grouped: BasicConv's Conv2d(1x1, groups = 4) behind the
// max-relative aggregation, torch_nn.py:57-69 behind torch_vertex.py:57-61, under 16-bit autocast with gradients, opt-in
// GKG_ENABLE=train_grouped): the fp32-A 64-column form with a group dimension.  One launch computes nb independent products; group
// q's x, fragment array and output are the launch's base pointers plus q times a per-operand stride (LinBf16GroupedArgs).  The only
// thing that differs from the single-matrix form is the origin of a tile's pointers: the workgroup derives q from its tile index
// (workgroup-uniform: scalar registers, 64-bit offsets) and from there on runs the shared code — element rounding, LDS image,
// contraction order, zero-fill of partial tiles, store path — on its group's own (R, cin) x (cout, cin) problem, so group q's bits
// are those of gkg_linear_{bf16,f16}_f32a on group q's views.  A pure product: scale, shift, activation, residual and the 16-bit
// output are compiled out (what remains is the single-matrix form's acc + 0 of a NULL shift vector).
// Tile map: tiles = row tiles x nb x col_tiles inside the per-XCD contiguous ranges, column tile fastest, then the group, then the
// row tile: the nb groups of one 128-row tile are adjacent on one XCD.  In the forward a row of XM holds all four groups' chunks in
// 4 ci contiguous floats, so its cache lines come from memory once per L2; in the input gradient the same holds for the rows of dXM
// being written.
//   linear_bf16_kernel<2, false, true, LbElem::BF16, true>   191 VGPRs, 0 AGPRs, 64 SGPRs   LDS 53 248 B (dynamic), no scratch   2 waves / SIMD
//   linear_bf16_kernel<2, false, true, LbElem::F16, true>    189 VGPRs, 0 AGPRs, 64 SGPRs   LDS 53 248 B (dynamic), no scratch   2 waves / SIMD
// The six instantiations above keep their figures AND their instructions with the parameter (234 / 66, 152 / 62, 237 / 106,
// 155 / 106, 186 / 62, 184 / 62): without it the kernel's text is what it was.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <type_traits>

#include "gkg_common.h"
#include "gkg_knn_prep.h"

namespace gkg {

typedef float lb_f32x16 __attribute__((ext_vector_type(16)));
typedef __attribute__((__vector_size__(8 * sizeof(__bf16)))) __bf16 lb_bf16x8;
typedef __attribute__((__vector_size__(8 * sizeof(_Float16)))) _Float16 lb_f16x8;

constexpr int LB_BM = 128;                       // rows per workgroup: 4 waves x 32
constexpr int LB_KC = 64;                        // contraction elements per LDS stage (4 MFMA steps of 16)
constexpr int LB_NT = 256;
constexpr int LB_APITCH = (LB_KC + 8) * 2;       // bytes per A row in LDS
constexpr int LB_ABYTES = LB_BM * LB_APITCH;     // 18 432

struct LinBf16Args {
  const uint16_t* x; int ldx;       // (R, ldx) bf16
  const uint4* wp;                  // [ci_pad / 8][co_pad] fragments of 8 consecutive input channels (bf16)
  const float* a;                   // [cout] or null (= 1)
  const float* cs;                  // [cout]
  const float* res; int ldr;        // (R, ldr) fp32 or null
  float* o32; int ldo32;            // (R, ldo32) or null
  uint16_t* o16; int ldo16;         // (R, ldo16) bf16 or null
  int R, cin, cout, ci_pad, co_pad, act;
  int col_tiles, tiles, tiles_per_xcd;
};

// PREP (gkg_linear_bf16_knn_prep): the layer is a Grapher's fc1 and the launch also prepares its output as the QUERIES of the k-NN
// call behind it.  q: the queries' set of that call's own plan (knn_query_prep_plan; q.s.t == o32, token-major rows of B images x
// N tokens, G groups of c channels); cnt: one arrival counter per row tile, zero between launches.
struct LinBf16PrepArgs : LinBf16Args { KnnQueryPrep q; unsigned* cnt; int B, G, c, N; };

// GROUPED (gkg_linear_bf16_f32a_grouped / gkg_linear_f16_f32a_grouped): nb independent products in one launch.  Group q's operands
// are the base pointers plus q times a stride: x + q x_gs and o32 + q out_gs in floats, wp + q wp_gs in fragments (the nb fragment
// arrays lie back to back).  tiles = row tiles x nb x col_tiles.
struct LinBf16GroupedArgs : LinBf16Args { long long x_gs, out_gs, wp_gs; int nb; };

template <bool PREP, bool GROUPED>
using lb_args_t = std::conditional_t<PREP, LinBf16PrepArgs, std::conditional_t<GROUPED, LinBf16GroupedArgs, LinBf16Args>>;

constexpr size_t lb_lds_bytes(int NB) { return 2 * (size_t)(LB_ABYTES + (LB_KC / 8) * 32 * NB * 16); }
// tokens per cooperative preparation tile: c (TK + 1) floats fit the operand buffers of either tile form (53 248 B)
constexpr bool lb_prep_fits(int cmax, int TK) { return (size_t)cmax * (TK + 1) * 4 <= lb_lds_bytes(2); }
static_assert(lb_prep_fits(192, 64) && lb_prep_fits(384, 32) && lb_prep_fits(600, 16), "the preparation tile must fit the operand buffers");

// A 16-byte store that goes through to memory at device scope (what a relaxed agent-scope atomic store is, per dword): visible to
// the other XCDs' workgroups once the issuing wave's store counter has drained.
typedef float lb_f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void lb_store_wt(float* p, const float4& v) {
  const lb_f32x4 d = {v.x, v.y, v.z, v.w};
  asm volatile("global_store_dwordx4 %0, %1, off sc1" : : "v"(p), "v"(d) : "memory");
}

// The last workgroup of a row tile prepares the tile's tokens, rows [row, rend) of `out`: per image the tile meets, per group, TK
// tokens at a time (token_prep_coop_body: the bits of the stand-alone launch), the prefilter planes where the plan has them, and
// the planes' pad rows for the image whose last token the tile holds (one row tile per image: one writer per (b, g)).
template <bool NORM, int TK>
__device__ __forceinline__ void lb_prep_rows(const LinBf16PrepArgs& g, float* col, long long row, long long rend) {
  const PrepSet& S = g.q.s;
  const bool planes = S.tb_lo != nullptr;
  while (row < rend) {
    const int b = (int)(row / g.N), nlo = (int)(row - (long long)b * g.N);
    const int nhi = (int)min((long long)g.N, nlo + (rend - row));
    for (int gi = 0; gi < g.G; ++gi) {
      const int bg = b * g.G + gi;
      for (int n0 = nlo; n0 < nhi; n0 += TK) {
        const int nt = min(TK, nhi - n0);
        token_prep_coop_body<NORM, TK, false>(S, col, bg, n0, nt, g.c, g.q.cpad, BnDerive{}, nullptr, nullptr);
        if (planes) {
          __syncthreads();
          token_prep_planes_tile<TK>(S, col, bg, n0, nt, g.c);
        }
        __syncthreads();                       // the tile is free again
      }
      if (planes && nhi == g.N) token_prep_planes_pad(S, bg, g.c);
    }
    row += nhi - nlo;
  }
}

// The 16-bit element kind of the operands in LDS, of the weight fragments and of the 16-bit output: one packing helper, one
// fragment type, one MFMA per kind; everything else of the kernel is shared.
enum class LbElem { BF16, F16 };
template <LbElem E>
__device__ __forceinline__ uint32_t lb_pack2(float lo, float hi) {
  if constexpr (E == LbElem::F16) return pack_f16x2(lo, hi);
  else return pack_bf16x2(lo, hi);
}
template <LbElem E>
__device__ __forceinline__ lb_f32x16 lb_mfma(const uint4& a, const uint4& b, lb_f32x16 c) {
  if constexpr (E == LbElem::F16)
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(lb_f16x8, a), __builtin_bit_cast(lb_f16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(lb_bf16x8, a), __builtin_bit_cast(lb_bf16x8, b), c, 0, 0, 0);
}

template <int NB, bool PREP = false, bool F32A = false, LbElem E = LbElem::BF16, bool GROUPED = false>
__global__ __launch_bounds__(LB_NT, 2) void linear_bf16_kernel(lb_args_t<PREP, GROUPED> g) {
  static_assert(!(PREP && F32A), "the fp32-A form has no token preparation");
  static_assert(!GROUPED || (F32A && NB == 2), "the grouped form: the fp32-A 64-column form only");
  static_assert(E == LbElem::BF16 || (F32A && NB == 2), "fp16 operands: the fp32-A 64-column form only");
  extern __shared__ __align__(16) unsigned char lb_lds[];
  constexpr int BN = 32 * NB;
  constexpr int BBYTES = (LB_KC / 8) * BN * 16;
  constexpr int NA = LB_BM * (LB_KC / 8) / LB_NT;        // 16-byte A granules per thread and chunk: 4
  constexpr int NBG = (LB_KC / 8) * BN / LB_NT;          // B granules per thread and chunk: 4 (NB = 4), 2 (NB = 2)
  constexpr int NAR = F32A ? 2 * NA : NA;                // registers (16 B) an A chunk is staged in: an fp32 granule is two of them
  constexpr int SP = BN + 4;                             // floats per row of a wave's epilogue stage
  static_assert(4 * 32 * SP * 4 <= 2 * (LB_ABYTES + BBYTES), "the epilogue stage must fit the operand buffers");
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  // XCD-aware map (workgroups are dealt round-robin over the 8 XCDs): XCD i walks tiles [i * tiles_per_xcd, ...), column tile fastest
  const int lin = blockIdx.x;
  const int tl = lin >> 3, tile = (lin & 7) * g.tiles_per_xcd + tl;
  if (tl >= g.tiles_per_xcd || tile >= g.tiles) return;
  // the origin of the tile's operands: the launch's own pointers, or (GROUPED) those of the tile's group — column tile fastest, then
  // the group, then the row tile: the nb groups of one 128-row tile are adjacent on one XCD, so where they share their rows' cache
  // lines (the forward: a row of XM holds every group's chunk) the lines come from memory once per L2.  The group index is a
  // function of blockIdx alone: the three pointers are scalar registers, their offsets 64-bit.
  int gtile = tile;
  if constexpr (GROUPED) {
    const int per = g.nb * g.col_tiles;
    const int grt = tile / per, rem = tile - grt * per;
    const int q = rem / g.col_tiles;
    gtile = grt * g.col_tiles + (rem - q * g.col_tiles);               // the tile's index within its group's own matrix
    g.x = reinterpret_cast<const uint16_t*>(reinterpret_cast<const float*>(g.x) + (long long)q * g.x_gs);
    g.wp += (long long)q * g.wp_gs;
    g.o32 += (long long)q * g.out_gs;
  }
  const int rt = gtile / g.col_tiles, ct = gtile - rt * g.col_tiles;
  const long long r0 = (long long)rt * LB_BM;
  const int n0 = ct * BN;
  unsigned char* abuf = lb_lds;                          // [2][128][144 B]
  unsigned char* bbuf = lb_lds + 2 * LB_ABYTES;          // [2][8][BN][16 B]

  const int S = g.ci_pad >> 4;                           // MFMA steps
  const int NC = (g.ci_pad + LB_KC - 1) / LB_KC;         // LDS chunks
  const int nfrag = g.ci_pad >> 3;

  // two register sets: the loads of chunk c + 2 are issued before the MFMAs of chunk c (set c & 1), the set holding chunk c + 1 is
  // written to the other LDS buffer after them — a load has two chunks of matrix work (and the CU's other workgroups) to land
  uint4 ra[2][NAR], rb[2][NBG];
  auto fetch = [&](int c, uint4 (&qa)[NAR], uint4 (&qb)[NBG]) __attribute__((always_inline)) {
    const int k0 = c * LB_KC;
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int gi = tid + LB_NT * i;
      const long long row = r0 + (gi >> 3);
      const int k = k0 + 8 * (gi & 7);
      if constexpr (F32A) {                                // x is fp32 (R, ldx): the granule's 8 floats stay fp32 until the stash
        const uint4* xp = reinterpret_cast<const uint4*>(reinterpret_cast<const float*>(g.x) + (size_t)row * g.ldx + k);
        const bool in = row < g.R && k < g.cin;
        qa[2 * i] = in ? xp[0] : make_uint4(0, 0, 0, 0);
        qa[2 * i + 1] = in ? xp[1] : make_uint4(0, 0, 0, 0);
      } else {
        qa[i] = (row < g.R && k < g.cin) ? *reinterpret_cast<const uint4*>(g.x + (size_t)row * g.ldx + k) : make_uint4(0, 0, 0, 0);
      }
    }
#pragma unroll
    for (int i = 0; i < NBG; ++i) {
      const int gi = tid + LB_NT * i;
      const int f = (k0 >> 3) + gi / BN, n = n0 + (gi % BN);
      qb[i] = (f < nfrag && n < g.co_pad) ? g.wp[(size_t)f * g.co_pad + n] : make_uint4(0, 0, 0, 0);
    }
  };
  auto stash = [&](int buf, const uint4 (&qa)[NAR], const uint4 (&qb)[NBG]) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int gi = tid + LB_NT * i;
      uint4 v;
      if constexpr (F32A) {                                // round to nearest even here: the LDS image is the 16-bit kernel's
        const float4 f0 = __builtin_bit_cast(float4, qa[2 * i]), f1 = __builtin_bit_cast(float4, qa[2 * i + 1]);
        v = make_uint4(lb_pack2<E>(f0.x, f0.y), lb_pack2<E>(f0.z, f0.w), lb_pack2<E>(f1.x, f1.y), lb_pack2<E>(f1.z, f1.w));
      } else {
        v = qa[i];
      }
      *reinterpret_cast<uint4*>(abuf + buf * LB_ABYTES + (gi >> 3) * LB_APITCH + 16 * (gi & 7)) = v;
    }
#pragma unroll
    for (int i = 0; i < NBG; ++i) *reinterpret_cast<uint4*>(bbuf + buf * BBYTES + 16 * (tid + LB_NT * i)) = qb[i];
  };

  const int l31 = lane & 31, kg = lane >> 5;
  bool has[NB];
#pragma unroll
  for (int u = 0; u < NB; ++u) has[u] = n0 + 32 * u < g.co_pad;     // workgroup-uniform
  lb_f32x16 acc[NB];
#pragma unroll
  for (int u = 0; u < NB; ++u)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[u][r] = 0.f;

  auto compute = [&](int c, int buf) __attribute__((always_inline)) {
    const unsigned char* ap = abuf + buf * LB_ABYTES + (32 * w + l31) * LB_APITCH + 16 * kg;
    const unsigned char* bp = bbuf + buf * BBYTES + (kg * BN + l31) * 16;
    const int steps = min(LB_KC / 16, S - c * (LB_KC / 16));
    auto step = [&](int s, bool all) __attribute__((always_inline)) {
      const uint4 av = *reinterpret_cast<const uint4*>(ap + 32 * s);
#pragma unroll
      for (int u = 0; u < NB; ++u)
        if (all || has[u]) {
          const uint4 bv = *reinterpret_cast<const uint4*>(bp + (2 * s * BN + 32 * u) * 16);
          acc[u] = lb_mfma<E>(av, bv, acc[u]);
        }
    };
    if (steps == LB_KC / 16 && has[NB - 1]) {
      // a full chunk of a full column tile: straight-line code, a step's fragment reads issue under the MFMAs of the one before
#pragma unroll
      for (int s = 0; s < LB_KC / 16; ++s) step(s, true);
    } else {
      for (int s = 0; s < steps; ++s) step(s, false);
    }
  };

  fetch(0, ra[0], rb[0]);
  if (NC > 1) fetch(1, ra[1], rb[1]);
  stash(0, ra[0], rb[0]);
  __syncthreads();
  for (int c = 0; c < NC; c += 2) {
    // chunk c (LDS buffer 0).  A stash targets the buffer the PREVIOUS chunk was read from, behind the barrier that ended it.
    if (c + 2 < NC) fetch(c + 2, ra[0], rb[0]);
    compute(c, 0);
    if (c + 1 < NC) stash(1, ra[1], rb[1]);
    __syncthreads();
    if (c + 1 >= NC) break;
    // chunk c + 1 (LDS buffer 1)
    if (c + 3 < NC) fetch(c + 3, ra[1], rb[1]);
    compute(c + 1, 1);
    if (c + 2 < NC) stash(0, ra[0], rb[0]);
    __syncthreads();
  }

  // ---------------------------------------------------------------- epilogue (the last barrier freed the operand buffers)
  float* st = reinterpret_cast<float*>(lb_lds) + w * 32 * SP;        // this wave's 32 rows x BN columns
  auto affine = [&](bool scaled, bool gelu) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      const int col = n0 + 32 * u + l31;
      if (has[u] && col < g.cout) {
        float cv;
        if constexpr (GROUPED) cv = 0.f;
        else if constexpr (F32A) cv = g.cs ? g.cs[col] : 0.f;          // (the fp32-A entry point only: no shift vector = zeros)
        else cv = g.cs[col];
        const float av = scaled ? g.a[col] : 1.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = (r & 3) + 8 * (r >> 2) + 4 * kg;
          float z = scaled ? __builtin_fmaf(av, acc[u][r], cv) : acc[u][r] + cv;
          if (gelu) z = gelu_f(z);
          st[row * SP + 32 * u + l31] = z;
        }
      }
    }
  };
  if constexpr (GROUPED) {                                           // a pure product: no scale, no shift vector (acc + 0), no activation
    affine(false, false);
  } else if (g.a) {                                                  // the mode tests once, not per element
    if (g.act == 1) affine(true, true); else affine(true, false);
  } else {
    if (g.act == 1) affine(false, true); else affine(false, false);
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  constexpr int NG = BN / 8;                                         // 8-column segments per row
  for (int it = lane; it < 32 * NG; it += 64) {
    const int rl = it / NG, col = n0 + 8 * (it % NG);
    const long long row = r0 + 32 * w + rl;
    if (row < g.R && col < g.cout) {
      float4 z0 = *reinterpret_cast<const float4*>(st + rl * SP + 8 * (it % NG));
      float4 z1 = *reinterpret_cast<const float4*>(st + rl * SP + 8 * (it % NG) + 4);
      if (!GROUPED && g.res) {
        const float* rp = g.res + (size_t)row * g.ldr + col;
        const float4 q0 = *reinterpret_cast<const float4*>(rp), q1 = *reinterpret_cast<const float4*>(rp + 4);
        z0.x += q0.x; z0.y += q0.y; z0.z += q0.z; z0.w += q0.w;
        z1.x += q1.x; z1.y += q1.y; z1.z += q1.z; z1.w += q1.w;
      }
      if (GROUPED || g.o32) {
        float* op = g.o32 + (size_t)row * g.ldo32 + col;
        if (PREP && g.col_tiles > 1) {                               // another workgroup prepares these rows: write-through stores
          lb_store_wt(op, z0);
          lb_store_wt(op + 4, z1);
        } else {
          *reinterpret_cast<float4*>(op) = z0;
          *reinterpret_cast<float4*>(op + 4) = z1;
        }
      }
      if (!GROUPED && g.o16)
        *reinterpret_cast<uint4*>(g.o16 + (size_t)row * g.ldo16 + col) =
            make_uint4(lb_pack2<E>(z0.x, z0.y), lb_pack2<E>(z0.z, z0.w), lb_pack2<E>(z1.x, z1.y), lb_pack2<E>(z1.z, z1.w));
    }
  }
  if constexpr (PREP) {
    if (g.col_tiles > 1) {
      // The hand-off of the split-K last-arriver reduce (gkg_gemm_x6_tile.h), without cache-wide fences (an agent-scope release
      // writes the whole L2 back — once per workgroup here: measured 1.4 ms on a 98 us launch): the tile went out write-through
      // (lb_store_wt), every wave drains its stores, the workgroup meets, ONE lane counts the arrival; the last of the row tile's
      // column tiles acquires (its L1 is the only cache that could hold stale lines of `out`), re-arms the counter for the next
      // launch and prepares the rows.
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      unsigned* flag = reinterpret_cast<unsigned*>(lb_lds);          // (the barrier freed the epilogue stage)
      if (tid == 0) *flag = __hip_atomic_fetch_add(g.cnt + rt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __syncthreads();
      const bool last = *flag == (unsigned)(g.col_tiles - 1);
      __syncthreads();                                               // everyone has read the flag: the LDS is the preparation's
      if (!last) return;
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      if (tid == 0) __hip_atomic_store(g.cnt + rt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      // one column tile holds every group: the workgroup prepares the rows it has just stored itself
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __syncthreads();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
    float* col = reinterpret_cast<float*>(lb_lds);
    const long long rend = min(r0 + LB_BM, (long long)g.R);
    const int c = g.c;
    if ((size_t)c * LB_NT * sizeof(float) <= lb_lds_bytes(2)) {
      // narrow groups (c <= 52): one thread per (row, group) pair, no barriers — one pass per two groups instead of 2 G dependent
      // cooperative tiles (measured at the stage-1 shape of GKGNet-576, c = 40: 205 us of tail with the cooperative form)
      if (g.q.norm) token_prep_flat_rows<true>(g.q.s, col, r0, (int)(rend - r0), g.G, c, g.q.cpad);
      else token_prep_flat_rows<false>(g.q.s, col, r0, (int)(rend - r0), g.G, c, g.q.cpad);
    } else if (g.q.norm) {
      if (c <= 192) lb_prep_rows<true, 64>(g, col, r0, rend);
      else if (c <= 384) lb_prep_rows<true, 32>(g, col, r0, rend);
      else lb_prep_rows<true, 16>(g, col, r0, rend);
    } else {
      if (c <= 192) lb_prep_rows<false, 64>(g, col, r0, rend);
      else if (c <= 384) lb_prep_rows<false, 32>(g, col, r0, rend);
      else lb_prep_rows<false, 16>(g, col, r0, rend);
    }
  }
}

template <int NB, bool PREP = false, bool F32A = false, LbElem E = LbElem::BF16, bool GROUPED = false, typename Args>
static hipError_t lb_launch(const Args& g, hipStream_t st) {
  static_assert(std::is_same_v<Args, lb_args_t<PREP, GROUPED>>, "the form's own argument struct");
  constexpr size_t lds = lb_lds_bytes(NB);
  if (lds > 64 * 1024) {
    const hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void*>(&linear_bf16_kernel<NB, PREP, F32A, E, GROUPED>),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (ea != hipSuccess) return ea;
  }
  hipLaunchKernelGGL((linear_bf16_kernel<NB, PREP, F32A, E, GROUPED>), dim3((unsigned)(g.tiles_per_xcd * 8)), dim3(LB_NT), lds, st, g);
  return hipGetLastError();
}

// The one place that knows the paddings of the fragment array: contraction to 16 (one MFMA step), output columns to 32 (one block).
static inline int lb_ci_pad(int cin) { return (cin + 15) & ~15; }
static inline int lb_co_pad(int cout) { return (cout + 31) & ~31; }

// Tiles of the launch for NB column blocks per workgroup; 0 when the grid would not fit an int.
static long long lb_tiles(int R, int co_pad, int NB, int* col_tiles) {
  const long long rt = ((long long)R + LB_BM - 1) / LB_BM;
  *col_tiles = (co_pad + 32 * NB - 1) / (32 * NB);
  return rt * *col_tiles;
}
// Column blocks per workgroup: 128-column tiles while they give every CU (256) a workgroup, 64-column tiles for narrow layers and
// for matrices of fewer tiles than that.  (Measured at the last stage of GKGNet-576, 10 368 rows x 640 columns = 405 tiles of 128
// columns: one round of those ran 13-20 % faster than the 810 64-column tiles, which are one full round of 768 resident
// workgroups plus a tail.)
static int lb_pick_nb(int R, int co_pad) {
  int ct;
  return (co_pad <= 64 || lb_tiles(R, co_pad, 4, &ct) < 256) ? 2 : 4;
}

// The launch's arguments and tile form (returned: column blocks per workgroup) for checked operands
static int lb_fill(LinBf16Args& g, const void* x, int ldx, const void* wplanes, const float* a, const float* cshift, const float* res,
                   int ldr, float* out_f32, int ldo32, void* out_bf16, int ldo16, int R, int cin, int cout, int act, int force_nb = 0) {
  g.x = (const uint16_t*)x; g.ldx = ldx; g.wp = (const uint4*)wplanes; g.a = a; g.cs = cshift; g.res = res; g.ldr = ldr;
  g.o32 = out_f32; g.ldo32 = ldo32; g.o16 = (uint16_t*)out_bf16; g.ldo16 = ldo16;
  g.R = R; g.cin = cin; g.cout = cout; g.ci_pad = lb_ci_pad(cin); g.co_pad = lb_co_pad(cout); g.act = act;
  const int NB = force_nb ? force_nb : lb_pick_nb(R, g.co_pad);
  const long long tiles = lb_tiles(R, g.co_pad, NB, &g.col_tiles);
  g.tiles = (int)tiles;
  g.tiles_per_xcd = (int)((tiles + 7) / 8);
  return NB;
}

}  // namespace gkg
using namespace gkg;

extern "C" size_t gkg_linear_bf16_planes_bytes(int cin, int cout) {
  if (cin <= 0 || cout <= 0 || (cin & 7) || (cout & 7)) return 0;
  return (size_t)(lb_ci_pad(cin) / 8) * lb_co_pad(cout) * 16;
}

extern "C" int gkg_linear_bf16_supported(int R, int cin, int cout, int has_res, int want_f32, int want_bf16, int act) {
  (void)has_res;
  if (R < 1 || cin <= 0 || cout <= 0 || (cin & 7) || (cout & 7) || cin > (1 << 24) || cout > (1 << 24)) return 0;
  if ((!want_f32 && !want_bf16) || act < 0 || act > 1) return 0;
  int ct;
  return lb_tiles(R, lb_co_pad(cout), lb_pick_nb(R, lb_co_pad(cout)), &ct) <= 0x3fffffffLL ? 1 : 0;
}

extern "C" int gkg_linear_bf16(const void* x, int ldx, const void* wplanes, const float* a, const float* cshift, const float* res,
                               int ldr, float* out_f32, int ldo32, void* out_bf16, int ldo16, int R, int cin, int cout, int act,
                               void* stream) {
  if (!x || !wplanes || !cshift || (!out_f32 && !out_bf16)) return gkg_fail(GKG_ERR_NULL, "gkg_linear_bf16: null pointer");
  if (R < 1 || cin <= 0 || cout <= 0 || act < 0 || act > 1)
    return gkg_fail(GKG_ERR_SHAPE, "gkg_linear_bf16: bad sizes (need R >= 1, cin, cout > 0, act in 0..1)");
  if (!gkg_linear_bf16_supported(R, cin, cout, res != nullptr, out_f32 != nullptr, out_bf16 != nullptr, act))
    return gkg_fail(GKG_ERR_UNSUPPORTED, "gkg_linear_bf16: need cin % 8 == 0, cout % 8 == 0 and a grid that fits");
  if ((ldx & 7) || (out_bf16 && (ldo16 & 7)) || (out_f32 && (ldo32 & 3)) || (res && (ldr & 3)))
    return gkg_fail(GKG_ERR_UNSUPPORTED, "gkg_linear_bf16: need ldx % 8 == 0, ldo16 % 8 == 0, ldo32 % 4 == 0, ldr % 4 == 0");
  if (((uintptr_t)x | (uintptr_t)wplanes | (uintptr_t)res | (uintptr_t)out_f32 | (uintptr_t)out_bf16) & 15)
    return gkg_fail(GKG_ERR_UNSUPPORTED, "gkg_linear_bf16: x, wplanes, res and the outputs must be 16-byte aligned");
  if (ldx < cin || (out_bf16 && ldo16 < cout) || (out_f32 && ldo32 < cout) || (res && ldr < cout))
    return gkg_fail(GKG_ERR_SHAPE, "gkg_linear_bf16: a row pitch is below the row's width");
  LinBf16Args g;
  const int NB = lb_fill(g, x, ldx, wplanes, a, cshift, res, ldr, out_f32, ldo32, out_bf16, ldo16, R, cin, cout, act);
  hipStream_t st = (hipStream_t)stream;
  const hipError_t e = NB == 4 ? lb_launch<4>(g, st) : lb_launch<2>(g, st);
  return e == hipSuccess ? 0 : gkg_fail_hip(e, "linear_bf16_kernel");
}

// ---------------------------------------------------------------------------------------------- fp32 A operand (training)
extern "C" int gkg_linear_bf16_f32a_supported(int R, int cin, int cout, int has_res, int want_f32, int want_bf16, int act) {
  if (!gkg_linear_bf16_supported(R, cin, cout, has_res, want_f32, want_bf16, act)) return 0;
  int ct;
  return lb_tiles(R, lb_co_pad(cout), 2, &ct) <= 0x3fffffffLL ? 1 : 0;              // the 64-column form at every shape
}

// One body for the two element kinds: `fn` names the entry point in the messages
template <LbElem E>
static int lb_f32a_call(const char* fn, const float* x, int ldx, const void* wplanes, const float* a, const float* cshift, const float* res,
                        int ldr, float* out_f32, int ldo32, void* out16, int ldo16, int R, int cin, int cout, int act, void* stream) {
  char msg[160];
  auto fail = [&](int code, const char* what) { snprintf(msg, sizeof msg, "%s: %s", fn, what); return gkg_fail(code, msg); };
  if (!x || !wplanes || (!out_f32 && !out16)) return fail(GKG_ERR_NULL, "null pointer");
  if (R < 1 || cin <= 0 || cout <= 0 || act < 0 || act > 1)
    return fail(GKG_ERR_SHAPE, "bad sizes (need R >= 1, cin, cout > 0, act in 0..1)");
  if (!gkg_linear_bf16_f32a_supported(R, cin, cout, res != nullptr, out_f32 != nullptr, out16 != nullptr, act))
    return fail(GKG_ERR_UNSUPPORTED, "need cin % 8 == 0, cout % 8 == 0 and a grid that fits");
  if ((ldx & 3) || (out16 && (ldo16 & 7)) || (out_f32 && (ldo32 & 3)) || (res && (ldr & 3)))
    return fail(GKG_ERR_UNSUPPORTED, "need ldx % 4 == 0, ldo16 % 8 == 0, ldo32 % 4 == 0, ldr % 4 == 0");
  if (((uintptr_t)x | (uintptr_t)wplanes | (uintptr_t)res | (uintptr_t)out_f32 | (uintptr_t)out16) & 15)
    return fail(GKG_ERR_UNSUPPORTED, "x, wplanes, res and the outputs must be 16-byte aligned");
  if (ldx < cin || (out16 && ldo16 < cout) || (out_f32 && ldo32 < cout) || (res && ldr < cout))
    return fail(GKG_ERR_SHAPE, "a row pitch is below the row's width");
  LinBf16Args g;
  lb_fill(g, x, ldx, wplanes, a, cshift, res, ldr, out_f32, ldo32, out16, ldo16, R, cin, cout, act, 2);
  const hipError_t e = lb_launch<2, false, true, E>(g, (hipStream_t)stream);
  return e == hipSuccess ? 0 : gkg_fail_hip(e, E == LbElem::F16 ? "linear_bf16_kernel (fp32 A, fp16 operands)" : "linear_bf16_kernel (fp32 A)");
}

extern "C" int gkg_linear_bf16_f32a(const float* x, int ldx, const void* wplanes, const float* a, const float* cshift, const float* res,
                                    int ldr, float* out_f32, int ldo32, void* out_bf16, int ldo16, int R, int cin, int cout, int act,
                                    void* stream) {
  return lb_f32a_call<LbElem::BF16>("gkg_linear_bf16_f32a", x, ldx, wplanes, a, cshift, res, ldr, out_f32, ldo32, out_bf16, ldo16, R, cin,
                                    cout, act, stream);
}

// ---------------------------------------------------------------------------------------------- fp32 A operand, fp16 operands (training)
// The fragment array's paddings, the tile form and the size limits are the element kind's business nowhere: the bf16 answers.
extern "C" size_t gkg_linear_f16_planes_bytes(int cin, int cout) { return gkg_linear_bf16_planes_bytes(cin, cout); }

extern "C" int gkg_linear_f16_f32a_supported(int R, int cin, int cout, int has_res, int want_f32, int want_f16, int act) {
  return gkg_linear_bf16_f32a_supported(R, cin, cout, has_res, want_f32, want_f16, act);
}

extern "C" int gkg_linear_f16_f32a(const float* x, int ldx, const void* wplanes_f16, const float* a, const float* cshift, const float* res,
                                   int ldr, float* out_f32, int ldo32, void* out_f16, int ldo16, int R, int cin, int cout, int act,
                                   void* stream) {
  return lb_f32a_call<LbElem::F16>("gkg_linear_f16_f32a", x, ldx, wplanes_f16, a, cshift, res, ldr, out_f32, ldo32, out_f16, ldo16, R, cin,
                                   cout, act, stream);
}

// ---------------------------------------------------------------------------------------------- fp32 A operand, nb groups (training)
extern "C" int gkg_linear_bf16_f32a_grouped_supported(int R, int cin, int cout, int nb) {
  if (nb < 1 || nb > 64 || !gkg_linear_bf16_f32a_supported(R, cin, cout, 0, 1, 0, 0)) return 0;
  int ct;
  return (long long)nb * lb_tiles(R, lb_co_pad(cout), 2, &ct) <= 0x3fffffffLL ? 1 : 0;
}

// One body for the two element kinds: `fn` names the entry point in the messages
template <LbElem E>
static int lb_grouped_call(const char* fn, const float* x, int ldx, long long x_gs, const void* wplanes, float* out, int ldo,
                           long long out_gs, int R, int cin, int cout, int nb, void* stream) {
  char msg[160];
  auto fail = [&](int code, const char* what) { snprintf(msg, sizeof msg, "%s: %s", fn, what); return gkg_fail(code, msg); };
  if (!x || !wplanes || !out) return fail(GKG_ERR_NULL, "null pointer");
  if (R < 1 || cin <= 0 || cout <= 0 || x_gs < 0 || out_gs < 0)
    return fail(GKG_ERR_SHAPE, "bad sizes (need R >= 1, cin, cout > 0, group strides >= 0)");
  if (!gkg_linear_bf16_f32a_grouped_supported(R, cin, cout, nb))
    return fail(GKG_ERR_UNSUPPORTED, "need cin % 8 == 0, cout % 8 == 0, 1 <= nb <= 64 and a grid that fits");
  if ((ldx & 3) || (ldo & 3) || (x_gs & 3) || (out_gs & 3))
    return fail(GKG_ERR_UNSUPPORTED, "need ldx % 4 == 0, ldo % 4 == 0, x_gs % 4 == 0, out_gs % 4 == 0");
  if (((uintptr_t)x | (uintptr_t)wplanes | (uintptr_t)out) & 15) return fail(GKG_ERR_UNSUPPORTED, "x, wplanes and out must be 16-byte aligned");
  if (ldx < cin || ldo < cout) return fail(GKG_ERR_SHAPE, "a row pitch is below the row's width");
  LinBf16GroupedArgs g;
  lb_fill(g, x, ldx, wplanes, nullptr, nullptr, nullptr, 0, out, ldo, nullptr, 0, R, cin, cout, 0, 2);
  g.x_gs = x_gs; g.out_gs = out_gs; g.nb = nb;
  g.wp_gs = (long long)(gkg_linear_bf16_planes_bytes(cin, cout) / sizeof(uint4));
  const long long tiles = (long long)g.tiles * nb;                      // row tiles x nb x column tiles
  g.tiles = (int)tiles;
  g.tiles_per_xcd = (int)((tiles + 7) / 8);
  const hipError_t e = lb_launch<2, false, true, E, true>(g, (hipStream_t)stream);
  return e == hipSuccess ? 0 : gkg_fail_hip(e, E == LbElem::F16 ? "linear_bf16_kernel (grouped, fp16 operands)" : "linear_bf16_kernel (grouped)");
}

extern "C" int gkg_linear_bf16_f32a_grouped(const float* x, int ldx, long long x_gs, const void* wplanes, float* out, int ldo,
                                            long long out_gs, int R, int cin, int cout, int nb, void* stream) {
  return lb_grouped_call<LbElem::BF16>("gkg_linear_bf16_f32a_grouped", x, ldx, x_gs, wplanes, out, ldo, out_gs, R, cin, cout, nb, stream);
}

extern "C" int gkg_linear_f16_f32a_grouped_supported(int R, int cin, int cout, int nb) {
  return gkg_linear_bf16_f32a_grouped_supported(R, cin, cout, nb);
}

extern "C" int gkg_linear_f16_f32a_grouped(const float* x, int ldx, long long x_gs, const void* wplanes, float* out, int ldo,
                                           long long out_gs, int R, int cin, int cout, int nb, void* stream) {
  return lb_grouped_call<LbElem::F16>("gkg_linear_f16_f32a_grouped", x, ldx, x_gs, wplanes, out, ldo, out_gs, R, cin, cout, nb, stream);
}

// ---------------------------------------------------------------------------------------------- fc1 + the k-NN's token preparation
// Scope of the fused form (include/gkg_hip.h): queries of a plain token-major output, fp32 contraction (neither 16-bit one).  0: in scope.
static int lbp_scope(int ochunk, int as_keys, const float* res_tm, const float* out_nchw, unsigned knn_flags) {
  return (ochunk != 0 || as_keys != 0 || res_tm || out_nchw || (knn_flags & (GKG_KNN_BF16_CONTRACT | GKG_KNN_F16_CONTRACT))) ? GKG_ERR_UNSUPPORTED : 0;
}
static bool lbp_sizes_ok(int cin, int B, int G, int c, int N) {
  if (B <= 0 || G <= 0 || c <= 0 || N <= 0 || (c & 3)) return false;
  if ((long long)B * N > 0x7fffffffLL || (long long)G * c > (1 << 24)) return false;
  return gkg_linear_bf16_supported(B * N, cin, G * c, 0, 1, 0, 0) != 0;
}

extern "C" size_t gkg_linear_bf16_knn_prep_scratch_bytes(int R) {
  return R < 1 ? 0 : sizeof(unsigned) * (size_t)(((long long)R + LB_BM - 1) / LB_BM);      // one arrival counter per row tile
}

extern "C" int gkg_linear_bf16_knn_prep_supported(int cin, int B, int G, int c, int N, int M, int k, int dilation, int has_y,
                                                  int has_relpos, unsigned knn_flags, int fused_mr) {
  if (lbp_scope(0, 0, nullptr, nullptr, knn_flags) != 0 || !lbp_sizes_ok(cin, B, G, c, N)) return 0;
  static float dummy[4];                            // the plan only computes addresses: nothing is read or written
  KnnQueryPrep q;
  return knn_query_prep_plan(dummy, G * c, B, G, c, N, M, k, dilation, has_y, has_relpos, knn_flags, fused_mr, dummy, ~(size_t)0, &q) == 0;
}

extern "C" int gkg_linear_bf16_knn_prep(const void* x, int ldx, const void* wplanes, int cin, const float* a, const float* cshift,
                                        float* out, int ldo, int ochunk, int B, int G, int c, int N, int M, int k, int dilation,
                                        int has_y, int has_relpos, unsigned knn_flags, int fused_mr, int as_keys, const float* res_tm,
                                        float* out_nchw, void* knn_workspace, size_t knn_workspace_bytes, void* scratch,
                                        size_t scratch_bytes, void* stream) {
  if (!x || !wplanes || !cshift || !out || !knn_workspace) return gkg_fail(GKG_ERR_NULL, "gkg_linear_bf16_knn_prep: null pointer");
  if (lbp_scope(ochunk, as_keys, res_tm, out_nchw, knn_flags) != 0)
    return gkg_fail(GKG_ERR_UNSUPPORTED, "gkg_linear_bf16_knn_prep: queries into plain rows only (no ochunk, as_keys, res_tm, out_nchw, bf16 / fp16 contraction)");
  if (B <= 0 || G <= 0 || c <= 0 || N <= 0 || cin <= 0) return gkg_fail(GKG_ERR_SHAPE, "gkg_linear_bf16_knn_prep: bad sizes");
  if (!lbp_sizes_ok(cin, B, G, c, N))
    return gkg_fail(GKG_ERR_UNSUPPORTED, "gkg_linear_bf16_knn_prep: need c % 4 == 0, cin % 8 == 0, (G c) % 8 == 0 and a grid that fits");
  const int R = B * N, cout = G * c;
  if (ldo == 0) ldo = cout;
  if ((ldx & 7) || (ldo & 3)) return gkg_fail(GKG_ERR_UNSUPPORTED, "gkg_linear_bf16_knn_prep: need ldx % 8 == 0, ldo % 4 == 0");
  if (((uintptr_t)x | (uintptr_t)wplanes | (uintptr_t)out) & 15)
    return gkg_fail(GKG_ERR_UNSUPPORTED, "gkg_linear_bf16_knn_prep: x, wplanes and out must be 16-byte aligned");
  if (ldx < cin || ldo < cout) return gkg_fail(GKG_ERR_SHAPE, "gkg_linear_bf16_knn_prep: a row pitch is below the row's width");
  if (!scratch || ((uintptr_t)scratch & 3) || scratch_bytes < gkg_linear_bf16_knn_prep_scratch_bytes(R))
    return gkg_fail(GKG_ERR_WORKSPACE, "gkg_linear_bf16_knn_prep: scratch too small (see gkg_linear_bf16_knn_prep_scratch_bytes)");
  LinBf16PrepArgs g;
  const int rc = knn_query_prep_plan(out, ldo, B, G, c, N, M, k, dilation, has_y, has_relpos, knn_flags, fused_mr, knn_workspace,
                                     knn_workspace_bytes, &g.q);
  if (rc != 0) return rc;
  if (g.q.s.tb && !g.q.s.tb_lo) return gkg_fail(GKG_ERR_UNSUPPORTED, "gkg_linear_bf16_knn_prep: not with the bf16 contraction");
  const int NB = lb_fill(g, x, ldx, wplanes, a, cshift, nullptr, 0, out, ldo, nullptr, 0, R, cin, cout, 0);
  g.cnt = (unsigned*)scratch; g.B = B; g.G = G; g.c = c; g.N = N;
  hipStream_t st = (hipStream_t)stream;
  const hipError_t e = NB == 4 ? lb_launch<4, true>(g, st) : lb_launch<2, true>(g, st);
  return e == hipSuccess ? 0 : gkg_fail_hip(e, "linear_bf16_kernel (k-NN preparation)");
}
