// gkg_knn_prep.h — the k-NN token preparation (normalised copies, |t|^2, prefilter planes) as device bodies shared by its
// stand-alone kernels (gkg_knn.hip) and by producers that prepare the tokens they write (gkg_linear_bf16.hip).
#pragma once
#include "gkg_knn_common.h"

namespace gkg {

// ------------------------------------------------------------------------------------------ prep
struct PrepStrides { int G; size_t sb, sg, sc, sn; int chunk; };      // chunk > 0 (token-major fp32 only): the x half of an XM
                                                                        // buffer (gkg_common.h) — channel ch at column xm_col(ch, chunk)

// One thread per token.  The two ordered fma chains over the channels are inherently serial per token and the
// problem has few tokens per CU (cfg2: 160), so the kernel is latency-bound.  Structure: (1) pull the token's
// whole channel column into a thread-private LDS column with 16 loads in flight and no arithmetic in between
// (token-major input: float4 loads of the contiguous channel run), (2) run both chains out of LDS, (3) store
// the normalised copy coalesced along the token axis.  PT (tokens per workgroup) shrinks with c so the column
// block always fits: PT * c * 4 B <= 48 KB.
// One launch prepares the queries AND (bipartite graphs) the keys: workgroups blockIdx.x >= nbx1 take the second
// tensor — for the short label-branch problems a second dependent launch costs as much as the work itself.
// tb != null: the normalised copy is written as bf16 in OCTET-major planes (bg, cp16 / 8, n, 8), zero-padded to cp16
// channels — a matrix-core operand fragment (one token, 8 consecutive channels) is 16 contiguous bytes and the fragments of
// consecutive tokens are adjacent, so a wave's fragment load / store touches 8 full cache lines instead of 32+ partial ones
// (measured: the token-major (bg, n, cp16) form left the contraction bound by the texture-address path) — instead of fp32
// channel-major th.  HF (GKG_KNN_F16_CONTRACT): those planes hold fp16 instead — round-to-nearest-even of the fp32 th, a
// subnormal result replaced by +0 (pack_f16x2_flush) — same geometry; |th|^2 comes from the unrounded th either way.
// tb_lo != null (prefilter mode, see knn_pf_kernel): besides the fp32 channel-major copy th (the exact re-rank reads it) the
// two leading bf16 terms of every normalised value, hi = bf16(v) and lo = bf16(v - hi), are written as token-major
// (bg, n, cp16) planes (tb = hi, tb_lo = lo) for the matrix-core prefilter.
// Prefilter planes, round 5: channels c and c + 1 of the HI plane carry the two leading bf16 terms of the token's |th|^2 (LO plane:
// zeros) — the kernel stages a query's copy of those two channels as (1, 1), so the matrix cores add |y|^2 to every distance and
// the selection loses a v_readlane + s_nop + v_add per candidate; the planes have `rows` = Tn rounded up to 32 rows, the pad rows
// hold MASKED_SQ there (keys past M mask themselves).  cp16 >= c + 2 in that mode.
// raw != null (round 6, queries of a fused block only): the input is a projection's PRE-BN output and this pass is also its
// BN-apply (kernel argument `d`: scale / shift derived from the projection's fp64 column sums, or given) — every token is
// affine-transformed as it is gathered, stored to `raw` (a token-major view: row pitch raw_ld, chunk raw_chunk — the x half of
// the grouped projection's operand buffer) and normalised from the same registers: the Grapher's fc1 BN-apply and the k-NN's
// token preparation in ONE pass over the tokens (reference torch_vertex.py:326 -> torch_edge.py:167-173).
// res_tm / nchw (the KEYS of a label graph produced by the Grapher in front of it, reference torch_vertex.py:331 -> :392-403): the
// pass is that Grapher's fc2 BN-apply — a y + c + res_tm[token] goes to `raw` (the token-major companion the label block reads as
// values), to `nchw` (B, C, Tn: the block's channel-major output) and, normalised, into the label k-NN's workspace as its keys.
struct PrepSet { const void* t; float* th; float* sq; int Tn; PrepStrides ps; uint16_t* tb; int cp16; uint16_t* tb_lo; int rows;
                 float* raw; int raw_ld, raw_chunk; const float* res_tm; float* nchw; };

// scale / shift of the group's c channels into LDS (tab[0..c) = a, tab[c..2c) = shift): derived from the column sums like every
// BN-apply pass (gkg_common.h bn_derive_channel; the first workgroup of image 0's groups writes the saved statistics and updates the
// running ones), or copied from the caller's a / c
__device__ __forceinline__ void prep_affine_table(const BnDerive& d, const float* __restrict__ a_in, const float* __restrict__ c_in,
                                                  float* tab, int c, int C, int bg, int G, int nthreads) {
  const int g = bg % G;
  const bool side = blockIdx.x == 0 && bg < G;                 // image 0: one workgroup per group
  for (int ch = threadIdx.x; ch < c; ch += nthreads) {
    const size_t o = (size_t)g * c + ch;
    float av, cv;
    if (d.sums) bn_derive_channel(d, o, d.sums[o], d.sums[C + o], side, av, cv);
    else { av = a_in[o]; cv = c_in[o]; }
    tab[ch] = av; tab[c + ch] = cv;
  }
  if (d.sums && blockIdx.x == 0 && bg == 0) {
    if (threadIdx.x == 0 && d.nbt) *d.nbt += 1;
    for (size_t i = threadIdx.x; i < d.zero_doubles; i += nthreads) d.zero_buf[i] = 0.0;
  }
  __syncthreads();
}

// fp32 pair -> packed fp16, round-to-nearest-even (the plain conversion under the default rounding mode; the pk_rtz conversion
// truncates and is not this), with a result below 2^-14 in magnitude — an fp16 subnormal, or a zero of either sign — stored as +0:
// the contraction never depends on what the matrix core does with subnormal inputs, and a zero exponent field means zero.
__device__ __forceinline__ uint32_t pack_f16x2_flush(float lo, float hi) {
  uint32_t l = __builtin_bit_cast(uint16_t, (_Float16)lo), h = __builtin_bit_cast(uint16_t, (_Float16)hi);
  l = (l & 0x7c00u) ? l : 0u;
  h = (h & 0x7c00u) ? h : 0u;
  return l | (h << 16);
}

template <typename T, bool NORM, int PT, bool PROD, bool HF = false>
__device__ __forceinline__ void token_prep_body(const PrepSet& s1, const PrepSet& s2, int nbx1, int c, int cpad, const BnDerive& d,
                                                const float* __restrict__ aff_a, const float* __restrict__ aff_c) {
  extern __shared__ float col[];          // [c][PT] (+ [2][c] scale / shift: PROD)
  const bool second = (int)blockIdx.x >= nbx1;
  const PrepSet& S = second ? s2 : s1;
  constexpr bool affine = PROD;                                  // a producer launch has ONE set: the BN-applied operand
  float* tab = col + (size_t)c * PT;
  if (affine) prep_affine_table(d, aff_a, aff_c, tab, c, s1.ps.G * c, blockIdx.y, s1.ps.G, PT);
  const T* __restrict__ t = static_cast<const T*>(S.t);
  float* __restrict__ th = S.th;
  float* __restrict__ sq = S.sq;
  const int Tn = S.Tn;
  const PrepStrides ps = S.ps;
  const int n = ((int)blockIdx.x - (second ? nbx1 : 0)) * PT + threadIdx.x;
  const int bg = blockIdx.y;
  if (n >= Tn) {
    if (S.tb_lo && n < S.rows) {                    // prefilter planes: pad rows up to a multiple of 32 mask themselves
      uint4* ohi = reinterpret_cast<uint4*>(S.tb) + (size_t)bg * (S.cp16 >> 3) * S.rows + n;
      uint4* olo = reinterpret_cast<uint4*>(S.tb_lo) + (size_t)bg * (S.cp16 >> 3) * S.rows + n;
      for (int c0 = 0; c0 < S.cp16; c0 += 8) {
        uint32_t wv[4] = {0u, 0u, 0u, 0u};
        if (c >= c0 && c < c0 + 8) {
          const uint32_t mk = (uint32_t)__builtin_bit_cast(uint16_t, (__bf16)MASKED_SQ);
          wv[(c - c0) >> 1] = ((c - c0) & 1) ? (mk << 16) : mk;
        }
        ohi[(size_t)(c0 >> 3) * S.rows] = make_uint4(wv[0], wv[1], wv[2], wv[3]);
        olo[(size_t)(c0 >> 3) * S.rows] = make_uint4(0u, 0u, 0u, 0u);
      }
    }
    return;
  }
  // element (bg = b*G + g, ch, n) of the input lives at  b*sb + g*sg + ch*sc + n*sn
  const T* tp = t + (size_t)(bg / ps.G) * ps.sb + (size_t)(bg % ps.G) * ps.sg + (size_t)n * ps.sn;
  float* cp = col + threadIdx.x;
  // ---- (1) gather the column
  if (sizeof(T) == 4 && ps.sc == 1 && (c & 3) == 0 && ((ps.sn | ps.sg | ps.sb) & 3) == 0) {
    const int goff = (bg % ps.G) * (int)ps.sg;      // the group's first channel; quad q sits xm_col(goff + 4 q) - goff floats into tp
    const float* tpf = reinterpret_cast<const float*>(tp) - goff;
    int q = 0;
    float* rawp = affine ? S.raw + ((size_t)(bg / ps.G) * Tn + n) * S.raw_ld : nullptr;
    auto apply = [&](float4& v, int q4) __attribute__((always_inline)) {       // BN-apply of 4 channels + the raw store
      if (affine) {
        v.x = __builtin_fmaf(tab[q4], v.x, tab[c + q4]); v.y = __builtin_fmaf(tab[q4 + 1], v.y, tab[c + q4 + 1]);
        v.z = __builtin_fmaf(tab[q4 + 2], v.z, tab[c + q4 + 2]); v.w = __builtin_fmaf(tab[q4 + 3], v.w, tab[c + q4 + 3]);
        if (S.res_tm) {
          const float4 r4 = *reinterpret_cast<const float4*>(S.res_tm + ((size_t)(bg / ps.G) * Tn + n) * (size_t)(ps.G * c) + goff + q4);
          v.x += r4.x; v.y += r4.y; v.z += r4.z; v.w += r4.w;
        }
        *reinterpret_cast<float4*>(rawp + xm_col(goff + q4, S.raw_chunk)) = v;
      }
    };
    for (; q + 8 <= (c >> 2); q += 8) {
      float4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const float4*>(tpf + xm_col(goff + 4 * (q + u), ps.chunk));
#pragma unroll
      for (int u = 0; u < 8; ++u) apply(v[u], 4 * (q + u));
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        cp[(4 * (q + u) + 0) * PT] = v[u].x; cp[(4 * (q + u) + 1) * PT] = v[u].y;
        cp[(4 * (q + u) + 2) * PT] = v[u].z; cp[(4 * (q + u) + 3) * PT] = v[u].w;
      }
    }
    for (; q < (c >> 2); ++q) {
      float4 v = *reinterpret_cast<const float4*>(tpf + xm_col(goff + 4 * q, ps.chunk));
      apply(v, 4 * q);
      cp[(4 * q + 0) * PT] = v.x; cp[(4 * q + 1) * PT] = v.y; cp[(4 * q + 2) * PT] = v.z; cp[(4 * q + 3) * PT] = v.w;
    }
  } else {
    int ch = 0;
    for (; ch + 16 <= c; ch += 16) {
      float v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) v[u] = ldf(tp + (size_t)(ch + u) * ps.sc);
#pragma unroll
      for (int u = 0; u < 16; ++u) cp[(ch + u) * PT] = v[u];
    }
    for (; ch < c; ++ch) cp[ch * PT] = ldf(tp + (size_t)ch * ps.sc);
  }
  // ---- (2) ordered chains out of LDS (own column: no barrier needed)
  float den = 1.0f;
  if (NORM) {
    float s = 0.0f;
#pragma unroll 8
    for (int ch = 0; ch < c; ++ch) { const float v = cp[ch * PT]; s = __builtin_fmaf(v, v, s); }
    den = fmaxf(sqrtf(s), 1e-12f);
  }
  // ---- (3) normalise, store, |th|^2
  float q2 = 0.0f;
  if (S.tb_lo) {                                    // prefilter mode: bf16 hi / lo planes (token-major) + th / sq below
    // the fp32 copy and |th|^2 first (the exact re-rank reads them): the two leading bf16 terms of |th|^2 ride in channels c, c + 1
    float q2p = 0.0f;
    {
      float* op = th + (size_t)bg * cpad * Tn + n;
      float* np_ = (affine && S.nchw) ? S.nchw + ((size_t)(bg / ps.G) * (ps.G * c) + (size_t)(bg % ps.G) * c) * Tn + n : nullptr;
#pragma unroll 8
      for (int ch = 0; ch < c; ++ch) {
        float v = cp[ch * PT];
        if (np_) np_[(size_t)ch * Tn] = v;
        if (NORM) { v = v / den; cp[ch * PT] = v; }      // the planes below split the normalised value: one division per element
        op[(size_t)ch * Tn] = v;
        q2p = __builtin_fmaf(v, v, q2p);
      }
      for (int chp = c; chp < cpad; ++chp) op[(size_t)chp * Tn] = 0.0f;
      sq[(size_t)bg * Tn + n] = q2p;
    }
    const float q2h = __uint_as_float(((uint32_t)__builtin_bit_cast(uint16_t, (__bf16)q2p)) << 16);
    const float q2l = q2p - q2h;
    // octet-major planes (bg, cp16 / 8, rows, 8): consecutive tokens are consecutive 16-byte fragments
    const int R = S.rows;
    uint4* ohi = reinterpret_cast<uint4*>(S.tb) + (size_t)bg * (S.cp16 >> 3) * R + n;
    uint4* olo = reinterpret_cast<uint4*>(S.tb_lo) + (size_t)bg * (S.cp16 >> 3) * R + n;
    for (int c0 = 0; c0 < S.cp16; c0 += 8) {
      uint32_t wh[4], wl[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e0 = c0 + 2 * u, e1 = e0 + 1;
        float v0 = e0 < c ? cp[e0 * PT] : 0.0f;
        float v1 = e1 < c ? cp[e1 * PT] : 0.0f;
        float l0 = v0 - __uint_as_float(((uint32_t)__builtin_bit_cast(uint16_t, (__bf16)v0)) << 16);
        float l1 = v1 - __uint_as_float(((uint32_t)__builtin_bit_cast(uint16_t, (__bf16)v1)) << 16);
        if (e0 == c) { v0 = q2h; l0 = 0.0f; } else if (e0 == c + 1) { v0 = q2l; l0 = 0.0f; }
        if (e1 == c) { v1 = q2h; l1 = 0.0f; } else if (e1 == c + 1) { v1 = q2l; l1 = 0.0f; }
        wh[u] = pack_bf16x2(v0, v1);
        wl[u] = pack_bf16x2(l0, l1);
      }
      ohi[(size_t)(c0 >> 3) * R] = make_uint4(wh[0], wh[1], wh[2], wh[3]);
      olo[(size_t)(c0 >> 3) * R] = make_uint4(wl[0], wl[1], wl[2], wl[3]);
    }
    return;
  }
  if (S.tb) {                                       // bf16 (HF: fp16) octet-major copy: 16-byte stores of 8 channels
    uint4* ob = reinterpret_cast<uint4*>(S.tb) + (size_t)bg * (S.cp16 >> 3) * Tn + n;      // octet-major (bg, cp16/8, Tn, 8)
    for (int c0 = 0; c0 < S.cp16; c0 += 8) {
      uint32_t wv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float v0 = c0 + 2 * u < c ? cp[(c0 + 2 * u) * PT] : 0.0f;
        float v1 = c0 + 2 * u + 1 < c ? cp[(c0 + 2 * u + 1) * PT] : 0.0f;
        if (NORM) { v0 = v0 / den; v1 = v1 / den; }
        q2 = __builtin_fmaf(v0, v0, q2);
        q2 = __builtin_fmaf(v1, v1, q2);
        wv[u] = HF ? pack_f16x2_flush(v0, v1) : pack_bf16x2(v0, v1);
      }
      ob[(size_t)(c0 >> 3) * Tn] = make_uint4(wv[0], wv[1], wv[2], wv[3]);
    }
    sq[(size_t)bg * Tn + n] = q2;
    return;
  }
  float* op = th + (size_t)bg * cpad * Tn + n;
  float* np_ = (affine && S.nchw) ? S.nchw + ((size_t)(bg / ps.G) * (ps.G * c) + (size_t)(bg % ps.G) * c) * Tn + n : nullptr;
#pragma unroll 8
  for (int ch = 0; ch < c; ++ch) {
    float v = cp[ch * PT];
    if (np_) np_[(size_t)ch * Tn] = v;
    if (NORM) v = v / den;
    op[(size_t)ch * Tn] = v;
    q2 = __builtin_fmaf(v, v, q2);
  }
  for (int chp = c; chp < cpad; ++chp) op[(size_t)chp * Tn] = 0.0f;
  sq[(size_t)bg * Tn + n] = q2;
}

// Small problems (a few ten thousand token-groups: the 18 x 18 stages, the label graphs): one thread per token-group leaves
// less than one wave per SIMD, each walking three dependent c-long passes (gather, norm chain, divide + |.|^2 chain) — the
// launch is pure latency (13-14 us at cfg2).  Cooperative form for fp32 token-major input: a 256-thread workgroup owns TK
// tokens of one (b, g); all threads gather the tile (16 lanes per token row: 256-byte runs), every wave recomputes the
// ordered norm chain of its token from LDS (no exchange), the divisions and the channel-major stores are spread over
// 256 / TK channel lanes per token, and the ordered |th|^2 chain runs on the normalised tile.  Same operations in the same
// order per value: bit-identical outputs.
// The body takes its place from the caller: tokens [n0, n0 + nt) (nt <= TK) of problem bg of set S, the tile in `col`
// ([c][TK + 1] floats of LDS, + [2][c] scale / shift: PROD) — a stand-alone kernel passes its block indices, a producer that
// prepares the tokens it has just written (gkg_linear_bf16.hip) walks its own rows.  All 256 threads of the workgroup call it; on
// return `col` holds the tile's normalised values (not PROD: zeros in lanes tok >= nt) and may be read after a barrier.
template <bool NORM, int TK, bool PROD>
__device__ __forceinline__ void token_prep_coop_body(const PrepSet& S, float* col, int bg, int n0, int nt, int c, int cpad,
                                                     const BnDerive& d, const float* __restrict__ aff_a,
                                                     const float* __restrict__ aff_c) {
  constexpr int LP = TK + 1, CL = 256 / TK;      // channel lanes per token
  const int tid = threadIdx.x;
  constexpr bool affine = PROD;
  float* tab = col + (size_t)c * LP;
  if (affine) prep_affine_table(d, aff_a, aff_c, tab, c, S.ps.G * c, bg, S.ps.G, 256);
  const int Tn = S.Tn;
  const PrepStrides ps = S.ps;
  const float* tp = static_cast<const float*>(S.t) + (size_t)(bg / ps.G) * ps.sb + (size_t)(bg % ps.G) * ps.sg + (size_t)n0 * ps.sn;
  const int c4 = c >> 2;
  const int goff = (bg % ps.G) * (int)ps.sg;      // the group's first channel (token-major: sg == c)
  // ---- (1) gather: lane (tid & 15) walks the float4s of the rows tid >> 4, + 16, ...
  for (int q = tid & 15; q < c4; q += 16) {
    float4 v[TK / 16];
    const int xo = xm_col(goff + 4 * q, ps.chunk) - goff;
#pragma unroll
    for (int u = 0; u < TK / 16; ++u) {
      const int tok = (tid >> 4) + 16 * u;
      v[u] = tok < nt ? *reinterpret_cast<const float4*>(tp + (size_t)tok * ps.sn + xo) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (affine) {                                   // BN-apply of the 4 channels + the raw store (the x half of the operand buffer)
      const float4 a4 = *reinterpret_cast<const float4*>(tab + 4 * q), c4 = *reinterpret_cast<const float4*>(tab + c + 4 * q);
      const int ro = xm_col(goff + 4 * q, S.raw_chunk);
#pragma unroll
      for (int u = 0; u < TK / 16; ++u) {
        const int tok = (tid >> 4) + 16 * u;
        v[u].x = __builtin_fmaf(a4.x, v[u].x, c4.x); v[u].y = __builtin_fmaf(a4.y, v[u].y, c4.y);
        v[u].z = __builtin_fmaf(a4.z, v[u].z, c4.z); v[u].w = __builtin_fmaf(a4.w, v[u].w, c4.w);
        if (tok < nt) {
          const size_t trow = (size_t)(bg / ps.G) * Tn + n0 + tok;
          if (S.res_tm) {
            const float4 r4 = *reinterpret_cast<const float4*>(S.res_tm + trow * (size_t)(ps.G * c) + goff + 4 * q);
            v[u].x += r4.x; v[u].y += r4.y; v[u].z += r4.z; v[u].w += r4.w;
          }
          *reinterpret_cast<float4*>(S.raw + trow * S.raw_ld + ro) = v[u];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < TK / 16; ++u) {
      const int tok = (tid >> 4) + 16 * u;
      col[(4 * q + 0) * LP + tok] = v[u].x; col[(4 * q + 1) * LP + tok] = v[u].y;
      col[(4 * q + 2) * LP + tok] = v[u].z; col[(4 * q + 3) * LP + tok] = v[u].w;
    }
  }
  __syncthreads();
  const int tok = tid % TK, cl = tid / TK;
  const float* cp = col + tok;
  // ---- (2) the token's ordered norm chain (every channel lane recomputes it: no exchange)
  float den = 1.0f;
  if (NORM) {
    float s = 0.0f;
#pragma unroll 8
    for (int ch = 0; ch < c; ++ch) { const float v = cp[ch * LP]; s = __builtin_fmaf(v, v, s); }
    den = fmaxf(sqrtf(s), 1e-12f);
  }
  __syncthreads();                          // everyone has read the raw tile
  // ---- (3) normalise + store: channel lane cl takes channels cl, cl + CL, ...
  float* op = S.th + (size_t)bg * cpad * Tn + n0 + tok;
  float* np_ = (affine && S.nchw && tok < nt) ? S.nchw + ((size_t)(bg / ps.G) * (ps.G * c) + (size_t)(bg % ps.G) * c) * Tn + n0 + tok : nullptr;
#pragma unroll 4
  for (int ch = cl; ch < c; ch += CL) {
    float v = cp[ch * LP];
    if (np_) np_[(size_t)ch * Tn] = v;                    // the block's channel-major output (coalesced along the tokens)
    if (NORM) v = v / den;
    col[ch * LP + tok] = v;
    if (tok < nt) op[(size_t)ch * Tn] = v;
  }
  if (tok < nt)
    for (int chp = c + cl; chp < cpad; chp += CL) op[(size_t)chp * Tn] = 0.0f;
  __syncthreads();
  // ---- (4) ordered |th|^2 chain
  if (cl == 0 && tok < nt) {
    float q2 = 0.0f;
#pragma unroll 8
    for (int ch = 0; ch < c; ++ch) { const float v = cp[ch * LP]; q2 = __builtin_fmaf(v, v, q2); }
    S.sq[(size_t)bg * Tn + n0 + tok] = q2;
  }
}

// Prefilter planes (PrepSet::tb_lo) of a tile token_prep_coop_body has just normalised — `col` as it left it, behind a barrier:
// the values token_prep_body writes there, per element from the same normalised value and the same ordered |th|^2 chain (every
// channel lane recomputes it), the octets of a token spread over its 256 / TK channel lanes.
template <int TK>
__device__ __forceinline__ void token_prep_planes_tile(const PrepSet& S, const float* col, int bg, int n0, int nt, int c) {
  constexpr int LP = TK + 1, CL = 256 / TK;
  const int tok = threadIdx.x % TK, cl = threadIdx.x / TK;
  if (tok >= nt) return;
  const float* cp = col + tok;
  float q2p = 0.0f;
#pragma unroll 8
  for (int ch = 0; ch < c; ++ch) { const float v = cp[ch * LP]; q2p = __builtin_fmaf(v, v, q2p); }
  const float q2h = __uint_as_float(((uint32_t)__builtin_bit_cast(uint16_t, (__bf16)q2p)) << 16);
  const float q2l = q2p - q2h;
  const int R = S.rows;
  uint4* ohi = reinterpret_cast<uint4*>(S.tb) + (size_t)bg * (S.cp16 >> 3) * R + n0 + tok;
  uint4* olo = reinterpret_cast<uint4*>(S.tb_lo) + (size_t)bg * (S.cp16 >> 3) * R + n0 + tok;
  for (int c0 = 8 * cl; c0 < S.cp16; c0 += 8 * CL) {
    uint32_t wh[4], wl[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e0 = c0 + 2 * u, e1 = e0 + 1;
      float v0 = e0 < c ? cp[e0 * LP] : 0.0f;
      float v1 = e1 < c ? cp[e1 * LP] : 0.0f;
      float l0 = v0 - __uint_as_float(((uint32_t)__builtin_bit_cast(uint16_t, (__bf16)v0)) << 16);
      float l1 = v1 - __uint_as_float(((uint32_t)__builtin_bit_cast(uint16_t, (__bf16)v1)) << 16);
      if (e0 == c) { v0 = q2h; l0 = 0.0f; } else if (e0 == c + 1) { v0 = q2l; l0 = 0.0f; }
      if (e1 == c) { v1 = q2h; l1 = 0.0f; } else if (e1 == c + 1) { v1 = q2l; l1 = 0.0f; }
      wh[u] = pack_bf16x2(v0, v1);
      wl[u] = pack_bf16x2(l0, l1);
    }
    ohi[(size_t)(c0 >> 3) * R] = make_uint4(wh[0], wh[1], wh[2], wh[3]);
    olo[(size_t)(c0 >> 3) * R] = make_uint4(wl[0], wl[1], wl[2], wl[3]);
  }
}
// ... and the planes' pad rows [Tn, rows) of problem bg (token_prep_body's n >= Tn branch): one workgroup per problem calls this.
__device__ __forceinline__ void token_prep_planes_pad(const PrepSet& S, int bg, int c) {
  for (int n = S.Tn + (int)threadIdx.x; n < S.rows; n += (int)blockDim.x) {
    uint4* ohi = reinterpret_cast<uint4*>(S.tb) + (size_t)bg * (S.cp16 >> 3) * S.rows + n;
    uint4* olo = reinterpret_cast<uint4*>(S.tb_lo) + (size_t)bg * (S.cp16 >> 3) * S.rows + n;
    for (int c0 = 0; c0 < S.cp16; c0 += 8) {
      uint32_t wv[4] = {0u, 0u, 0u, 0u};
      if (c >= c0 && c < c0 + 8) {
        const uint32_t mk = (uint32_t)__builtin_bit_cast(uint16_t, (__bf16)MASKED_SQ);
        wv[(c - c0) >> 1] = ((c - c0) & 1) ? (mk << 16) : mk;
      }
      ohi[(size_t)(c0 >> 3) * S.rows] = make_uint4(wv[0], wv[1], wv[2], wv[3]);
      olo[(size_t)(c0 >> 3) * S.rows] = make_uint4(0u, 0u, 0u, 0u);
    }
  }
}

// Narrow groups inside a producer's 256-thread workgroup (gkg_linear_bf16.hip): one thread per (row, group) pair of up to 128
// token-major rows [row0, row0 + nrows) of set S (plain rows: ps.chunk == 0; a row is image row / Tn, token row % Tn, so a range
// may cross images), two groups per pass — token_prep_body's arithmetic per token, value for value (gather into a thread-private
// LDS column col[ch * 256 + tid], the ordered norm chain, one division per element, the ordered |th|^2 chain, the prefilter planes
// where S has them; the thread of an image's last token also writes that image's pad rows), with no barrier at all: where
// c * 256 floats fit, one pass replaces 2 G dependent cooperative tiles.
template <bool NORM>
__device__ __forceinline__ void token_prep_flat_rows(const PrepSet& S, float* col, long long row0, int nrows, int G, int c, int cpad) {
  constexpr int PT = 256, RT = 128;
  const int tid = threadIdx.x, rl = tid & (RT - 1);
  if (rl >= nrows) return;
  const int Tn = S.Tn;
  const PrepStrides ps = S.ps;
  const long long row = row0 + rl;
  const int b = (int)(row / Tn), n = (int)(row - (long long)b * Tn);
  float* cp = col + tid;
  for (int g = tid >> 7; g < G; g += PT / RT) {
    const int bg = b * G + g;
    const float* tp = static_cast<const float*>(S.t) + (size_t)b * ps.sb + (size_t)g * ps.sg + (size_t)n * ps.sn;
    // ---- (1) gather the column
    int q = 0;
    for (; q + 8 <= (c >> 2); q += 8) {
      float4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const float4*>(tp + 4 * (q + u));
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        cp[(4 * (q + u) + 0) * PT] = v[u].x; cp[(4 * (q + u) + 1) * PT] = v[u].y;
        cp[(4 * (q + u) + 2) * PT] = v[u].z; cp[(4 * (q + u) + 3) * PT] = v[u].w;
      }
    }
    for (; q < (c >> 2); ++q) {
      const float4 v = *reinterpret_cast<const float4*>(tp + 4 * q);
      cp[(4 * q + 0) * PT] = v.x; cp[(4 * q + 1) * PT] = v.y; cp[(4 * q + 2) * PT] = v.z; cp[(4 * q + 3) * PT] = v.w;
    }
    // ---- (2) ordered norm chain
    float den = 1.0f;
    if (NORM) {
      float s = 0.0f;
#pragma unroll 8
      for (int ch = 0; ch < c; ++ch) { const float v = cp[ch * PT]; s = __builtin_fmaf(v, v, s); }
      den = fmaxf(sqrtf(s), 1e-12f);
    }
    // ---- (3) normalise, store, |th|^2
    float q2 = 0.0f;
    float* op = S.th + (size_t)bg * cpad * Tn + n;
#pragma unroll 8
    for (int ch = 0; ch < c; ++ch) {
      float v = cp[ch * PT];
      if (NORM) { v = v / den; cp[ch * PT] = v; }
      op[(size_t)ch * Tn] = v;
      q2 = __builtin_fmaf(v, v, q2);
    }
    for (int chp = c; chp < cpad; ++chp) op[(size_t)chp * Tn] = 0.0f;
    S.sq[(size_t)bg * Tn + n] = q2;
    if (!S.tb_lo) continue;
    // ---- (4) prefilter planes: hi / lo of every normalised value, the two leading bf16 terms of |th|^2 in channels c, c + 1
    const float q2h = __uint_as_float(((uint32_t)__builtin_bit_cast(uint16_t, (__bf16)q2)) << 16);
    const float q2l = q2 - q2h;
    const int R = S.rows;
    uint4* ohi = reinterpret_cast<uint4*>(S.tb) + (size_t)bg * (S.cp16 >> 3) * R + n;
    uint4* olo = reinterpret_cast<uint4*>(S.tb_lo) + (size_t)bg * (S.cp16 >> 3) * R + n;
    for (int c0 = 0; c0 < S.cp16; c0 += 8) {
      uint32_t wh[4], wl[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e0 = c0 + 2 * u, e1 = e0 + 1;
        float v0 = e0 < c ? cp[e0 * PT] : 0.0f;
        float v1 = e1 < c ? cp[e1 * PT] : 0.0f;
        float l0 = v0 - __uint_as_float(((uint32_t)__builtin_bit_cast(uint16_t, (__bf16)v0)) << 16);
        float l1 = v1 - __uint_as_float(((uint32_t)__builtin_bit_cast(uint16_t, (__bf16)v1)) << 16);
        if (e0 == c) { v0 = q2h; l0 = 0.0f; } else if (e0 == c + 1) { v0 = q2l; l0 = 0.0f; }
        if (e1 == c) { v1 = q2h; l1 = 0.0f; } else if (e1 == c + 1) { v1 = q2l; l1 = 0.0f; }
        wh[u] = pack_bf16x2(v0, v1);
        wl[u] = pack_bf16x2(l0, l1);
      }
      ohi[(size_t)(c0 >> 3) * R] = make_uint4(wh[0], wh[1], wh[2], wh[3]);
      olo[(size_t)(c0 >> 3) * R] = make_uint4(wl[0], wl[1], wl[2], wl[3]);
    }
    if (n == Tn - 1) {                              // the image's last token: its pad rows mask themselves
      const uint32_t mk = (uint32_t)__builtin_bit_cast(uint16_t, (__bf16)MASKED_SQ);
      for (int np = Tn; np < R; ++np)
        for (int c0 = 0; c0 < S.cp16; c0 += 8) {
          uint32_t wv[4] = {0u, 0u, 0u, 0u};
          if (c >= c0 && c < c0 + 8) wv[(c - c0) >> 1] = ((c - c0) & 1) ? (mk << 16) : mk;
          ohi[(size_t)(c0 >> 3) * R + (np - n)] = make_uint4(wv[0], wv[1], wv[2], wv[3]);
          olo[(size_t)(c0 >> 3) * R + (np - n)] = make_uint4(0u, 0u, 0u, 0u);
        }
    }
  }
}

// What a producer that runs the queries' preparation inside its own kernel needs of the k-NN call's plan (knn_plan, gkg_knn_plan.h: the one
// place that makes it): the queries' set (workspace addresses, plane geometry; tb_lo != null: prefilter planes exist), the row
// count of the normalised copies, the normalisation switch.  Host code, gkg_knn.hip; nothing is launched.  Returns 0 or a GKG_ERR_*
// code with the error string set.
struct KnnQueryPrep { PrepSet s; int cpad; int norm; };
int knn_query_prep_plan(const float* tokens, int ld, int B, int G, int c, int N, int M, int k, int dilation, int has_y, int has_relpos,
                        unsigned knn_flags, int fused_mr, void* knn_workspace, size_t knn_workspace_bytes, KnnQueryPrep* plan);

}  // namespace gkg
