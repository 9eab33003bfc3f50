// gkg_mrgemm_tile.h — the phases the kernels that take the max-relative aggregation as the A-OPERAND PRODUCER of the grouped 1x1
// projection share: mr_linear_bf16_kernel (csrc/gkg_mrgemm.hip: ... + BN + GELU -> the (T, 2C) bf16 matrix) and
// mr_fc2_bf16_kernel (csrc/gkg_mr_fc2_bf16.hip: ... + fc2 behind it, the (T, 2C) matrix kept in LDS).  ONE definition of the index
// clamp, the maximum's tie rule, the GELU, the gather and the grouped contraction: the second kernel's bit contract is the first's.
//   mg_index_rows     phase 0  the tile's index rows -> LDS once (clamped; int32, or u16 where the caller knows M <= 65 536)
//   mg_gather_tile    phase 1  gather + max_k(x_j - x_i) + [x, m] interleave -> the bf16 A tiles in LDS, one per conv group
//   mg_group_gemm     phase 2  v_mfma_f32_32x32x16_bf16 over those tiles, the weight fragments streamed from L2
// The caller places the barriers between them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gkg_common.h"

namespace gkg {

typedef float mg_f32x16 __attribute__((ext_vector_type(16)));
typedef __attribute__((__vector_size__(8 * sizeof(__bf16)))) __bf16 mg_bf16x8;

constexpr int MG_ROWS = 64;       // tokens per workgroup
constexpr int MG_NW = 8;          // waves per workgroup (512 threads)
constexpr int MG_MAXB = 3;        // 32 x 32 output blocks per wave (wide layers; narrow ones: 2)
constexpr int MG_D = 3;           // weight fragments are fetched this many contraction steps ahead (registers)

struct MrGemmArgs {
  const float* x;          // (B, N, C) token-major fp32
  const float* src;        // (B, M, C) or null (self graph: src = x, M = N)
  const int64_t* nn_idx;   // (B*G, N, k)
  const uint16_t* nn16;    // (B*G, N, k) compact lists (gkg_knn_fwd_tm16) instead of nn_idx, or null
  const uint4* wp;         // [4][ci_pad/8][co_pad] fragments of 8 consecutive input channels (bf16)
  const float* a;          // (4*co) BN scale
  const float* cs;         // (4*co) BN shift (conv bias folded)
  uint16_t* out;           // (T, ldo) bf16; conv group q writes columns [q*co, (q+1)*co)
  int ldo;
  int B, G, c, N, M, k, C, Cq, ci, co, ci_pad, co_pad, act;
  long long T;
  int tiles, tiles_per_xcd;
};

__device__ __forceinline__ int mg_clamp(int64_t v, int M) { return (int)(v < 0 ? 0 : (v >= M ? M - 1 : v)); }
// torch.max semantics (same as gkg_mr.hip::takes): NaN propagates, first maximum wins
__device__ __forceinline__ bool mg_takes(float v, float best) { return v > best || (v != v && best == best); }
// GELU (erf form) with erf from Abramowitz & Stegun 7.1.26 (|error| <= 1.5e-7): ~15 vector instructions instead of the
// ~40 of erff.  The result is rounded to bf16 (2^-9 relative), so against the exact erf it differs only where a rounding
// boundary falls within 1e-7: the compile-time ablation showed erff as 21-26 % of this kernel at every stage shape.
__device__ __forceinline__ float mg_gelu(float z) {
  const float x = fabsf(z) * 0.70710678118654752440f;
  const float t = __builtin_amdgcn_rcpf(__builtin_fmaf(0.3275911f, x, 1.0f));
  float p = __builtin_fmaf(1.061405429f, t, -1.453152027f);
  p = __builtin_fmaf(p, t, 1.421413741f);
  p = __builtin_fmaf(p, t, -0.284496736f);
  p = __builtin_fmaf(p, t, 0.254829592f);
  const float e = 1.0f - p * t * __expf(-x * x);          // erf(|z| / sqrt 2)
  return 0.5f * z * (1.0f + copysignf(e, z));
}
// The hidden element of the grouped projection as the (T, 2C) bf16 matrix holds it
__device__ __forceinline__ uint16_t mg_hidden(float av, float acc, float cv, int act) {
  float o = __builtin_fmaf(av, acc, cv);
  if (act == 1) o = mg_gelu(o);
  return __builtin_bit_cast(uint16_t, (__bf16)o);
}

// ---------------------------------------------------------------- phase 0: the tile's index rows -> LDS (clamped)
// ids [64][NG][k]: the k-NN groups [glo, glo + NG) the workgroup's channels touch.  IdT = uint16_t needs M <= 65 536.
template <typename IdT>
__device__ __forceinline__ void mg_index_rows(const MrGemmArgs& g, IdT* ids, long long t0, int glo, int NG, int k, int tid) {
  constexpr int NT = 64 * MG_NW;
  const int N = g.N, M = g.M;
  const int per_tok = NG * k;
  for (int e = tid; e < MG_ROWS * per_tok; e += NT) {
    const int tok = e / per_tok, r = e - tok * per_tok;
    const int gi = r / k, jj = r - gi * k;
    const long long t = t0 + tok;
    int v = 0;
    if (t < g.T) {
      const int b = (int)(t / N), n = (int)(t - (long long)b * N);
      const size_t ie = (((size_t)b * g.G + glo + gi) * N + n) * k + jj;
      v = g.nn16 ? min((int)g.nn16[ie], M - 1) : mg_clamp(g.nn_idx[ie], M);
    }
    ids[e] = (IdT)v;
  }
}

// ---------------------------------------------------------------- phase 1: the A tile = interleaved [x, max-relative]
// every thread gathers the k neighbour rows of (token, 4 channels) from L2 (token-major rows: one float4 per neighbour; INF
// items in flight per thread), takes the max of the differences — the same arithmetic, in the same order, as mr_fwd_tm_kernel —
// and writes the interleaved [x, m] values as bf16 (round-to-nearest-even) straight into the LDS image of the GEMM's A tile:
// 64 rows x ci = C/2 input channels per conv group (QG tiles, `qstride` bytes apart, rows of `pitch` bytes), conv groups
// [ch_lo / Cq, + QG).
template <int KS, int QG, int INF, typename IdT>
__device__ __forceinline__ void mg_gather_tile(const MrGemmArgs& g, unsigned char* lds, const IdT* ids, long long t0, int ch_lo,
                                               int glo, int NG, int k, int pitch, int qstride, int tid) {
  constexpr int NT = 64 * MG_NW;
  const int C = g.C, N = g.N, M = g.M;
  const int Q4 = g.Cq >> 2;                              // channel quads per conv group
  const int QW = QG * Q4;                                // quads per token in this workgroup
  const float* srcb = g.src ? g.src : g.x;
  const int nitems = MG_ROWS * QW;
  struct Item { float4 xi; float4 nb[KS > 0 ? KS : 1]; int tok, qq; bool live; };
  auto fetch = [&](int it, Item& I) __attribute__((always_inline)) {
    I.live = false;
    I.tok = 0; I.qq = 0;
    if (it >= nitems) return;
    const int tok = it / QW, qq = it - tok * QW;         // qq = qi * Q4 + quad: consecutive threads, consecutive channels
    I.tok = tok; I.qq = qq;
    const long long t = t0 + tok;
    if (t >= g.T) return;
    I.live = true;
    const int b = (int)(t / N);
    const int ch = ch_lo + 4 * qq;                        // original channel (4 channels never straddle a k-NN group)
    const IdT* ip = ids + (tok * NG + (ch / g.c - glo)) * k;
    I.xi = *reinterpret_cast<const float4*>(g.x + (size_t)t * C + ch);
    const float* sb = srcb + (size_t)b * M * C + ch;
    if (KS > 0) {
#pragma unroll
      for (int u = 0; u < KS; ++u) I.nb[u] = *reinterpret_cast<const float4*>(sb + (size_t)ip[u] * C);
    }
  };
  auto finish = [&](const Item& I, int it) __attribute__((always_inline)) {
    if (it >= nitems) return;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (I.live) {
      const float4 xi = I.xi;
      float4 best;
      if (KS > 0) {
        best = make_float4(I.nb[0].x - xi.x, I.nb[0].y - xi.y, I.nb[0].z - xi.z, I.nb[0].w - xi.w);
#pragma unroll
        for (int u = 1; u < KS; ++u) {
          const float d0 = I.nb[u].x - xi.x, d1 = I.nb[u].y - xi.y, d2 = I.nb[u].z - xi.z, d3 = I.nb[u].w - xi.w;
          if (mg_takes(d0, best.x)) best.x = d0;
          if (mg_takes(d1, best.y)) best.y = d1;
          if (mg_takes(d2, best.z)) best.z = d2;
          if (mg_takes(d3, best.w)) best.w = d3;
        }
      } else {
        const long long t = t0 + I.tok;
        const int b = (int)(t / N);
        const int ch = ch_lo + 4 * I.qq;
        const IdT* ip = ids + (I.tok * NG + (ch / g.c - glo)) * k;
        const float* sb = srcb + (size_t)b * M * C + ch;
        const float4 n0 = *reinterpret_cast<const float4*>(sb + (size_t)ip[0] * C);
        best = make_float4(n0.x - xi.x, n0.y - xi.y, n0.z - xi.z, n0.w - xi.w);
        for (int u = 1; u < k; ++u) {
          const float4 nv = *reinterpret_cast<const float4*>(sb + (size_t)ip[u] * C);
          const float d0 = nv.x - xi.x, d1 = nv.y - xi.y, d2 = nv.z - xi.z, d3 = nv.w - xi.w;
          if (mg_takes(d0, best.x)) best.x = d0;
          if (mg_takes(d1, best.y)) best.y = d1;
          if (mg_takes(d2, best.z)) best.z = d2;
          if (mg_takes(d3, best.w)) best.w = d3;
        }
      }
      v = make_uint4(pack_bf16x2(xi.x, best.x), pack_bf16x2(xi.y, best.y), pack_bf16x2(xi.z, best.z),
                     pack_bf16x2(xi.w, best.w));
    }
    const int qi = I.qq / Q4, quad = I.qq - qi * Q4;
    *reinterpret_cast<uint4*>(lds + qi * qstride + I.tok * pitch + 16 * quad) = v;
  };
  if (KS > 0 && KS <= 12 && INF == 2) {
    for (int it = tid; it < nitems; it += 2 * NT) {      // two items in flight per thread: 2 (k + 1) row loads outstanding
      Item I0, I1;
      fetch(it, I0);
      fetch(it + NT, I1);
      finish(I0, it);
      finish(I1, it + NT);
    }
  } else {
    for (int it = tid; it < nitems; it += NT) {          // long index rows: one item's k + 1 loads fill the register budget
      Item I0;
      fetch(it, I0);
      finish(I0, it);
    }
  }
  if (g.ci_pad > g.ci && tid < MG_ROWS * QG)             // contraction padding (ci % 16 == 8): one zero fragment per row
    *reinterpret_cast<uint4*>(lds + (tid / MG_ROWS) * qstride + (tid % MG_ROWS) * pitch + 2 * g.ci) = make_uint4(0, 0, 0, 0);
}

// ---------------------------------------------------------------- phase 2: (64 x ci) @ W_q^T on the bf16 matrix cores
// wave w: row block rb = w & 1 and the (conv group, column block) pairs p = (w >> 1) + (NW / 2) u, u < MAXB (has[u]: p exists;
// wave-uniform); conv groups [q0, q0 + QG).  The weights stream from L2 as pre-arranged 16-byte fragments [q][ci/8][co][8],
// fetched DEPTH contraction steps ahead into registers, fp32 accumulation over ascending steps of 16.
template <int QG, int MAXB, int DEPTH>
__device__ __forceinline__ void mg_group_gemm(const MrGemmArgs& g, const unsigned char* lds, int q0, int pitch, int qstride, int w,
                                              int lane, mg_f32x16 (&acc)[MAXB], bool (&has)[MAXB]) {
  const int l31 = lane & 31, kg = lane >> 5;
  const int rb = w & 1;
  const int ncb = g.co_pad >> 5;
  const int npairs = QG * ncb;
  const int S = g.ci_pad >> 4;
  const size_t wq_stride = (size_t)(g.ci_pad >> 3) * g.co_pad;       // fragments per conv group
  const uint4* wptr[MAXB];
  const unsigned char* aptr[MAXB];
#pragma unroll
  for (int u = 0; u < MAXB; ++u) {
    const int p = (w >> 1) + (MG_NW / 2) * u;
    has[u] = p < npairs;                                             // wave-uniform
    const int qi = has[u] ? p / ncb : 0, cb = has[u] ? p - qi * ncb : 0;
    wptr[u] = g.wp + (size_t)(q0 + qi) * wq_stride + (size_t)kg * g.co_pad + 32 * cb + l31;
    aptr[u] = lds + qi * qstride + (32 * rb + l31) * pitch + 16 * kg;
  }
#pragma unroll
  for (int u = 0; u < MAXB; ++u)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[u][r] = 0.f;
  uint4 bq[DEPTH][MAXB];
#pragma unroll
  for (int d = 0; d < DEPTH; ++d)
#pragma unroll
    for (int u = 0; u < MAXB; ++u)
      bq[d][u] = (has[u] && d < S) ? wptr[u][(size_t)(2 * d) * g.co_pad] : make_uint4(0, 0, 0, 0);
  for (int s0 = 0; s0 < S; s0 += DEPTH) {
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) {
      const int s = s0 + d;
      if (s < S) {                                                   // uniform
        uint4 bc[MAXB];
#pragma unroll
        for (int u = 0; u < MAXB; ++u) bc[u] = bq[d][u];
#pragma unroll
        for (int u = 0; u < MAXB; ++u)
          if (has[u] && s + DEPTH < S) bq[d][u] = wptr[u][(size_t)(2 * (s + DEPTH)) * g.co_pad];
#pragma unroll
        for (int u = 0; u < MAXB; ++u)
          if (has[u]) {
            const mg_bf16x8 av = __builtin_bit_cast(mg_bf16x8, *reinterpret_cast<const uint4*>(aptr[u] + 32 * s));
            acc[u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, __builtin_bit_cast(mg_bf16x8, bc[u]), acc[u], 0, 0, 0);
          }
      }
    }
  }
}

}  // namespace gkg
