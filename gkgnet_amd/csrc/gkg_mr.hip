// gkg_mr.hip — max-relative neighbour aggregation and its backward scatter (gfx950).
//
// Forward replaces batched_index_select(x, edge_index[1]) + batched_index_select(src, edge_index[0]) +
// torch.max(x_j - x_i, -1)  (reference torch_vertex.py:49-54, torch_nn.py:84-105) without building the
// (BG,c,N,k) gathered tensors.  Backward replaces autograd's max_backward -> sub -> index_put_(accumulate).
//
// Layout: features are channel-major (BG,c,T); one (bg,ch) row of the source is contiguous and small
// (T*4 B <= 83 KB), so a workgroup keeps CH source rows in LDS and gathers / scatters there:
//   fwd : grid (n-tiles, channel chunks, BG); thread = one query n, its k indices in LDS (int32);
//         per channel: k LDS gathers, k subtracts (x_j - x_i as the reference does), first-max select;
//         writes m and the argmax byte coalesced along n.
//   bwd : grid (channel chunks, BG); LDS accumulator acc[CH][M]; all N queries of the (bg, chunk) are
//         swept, g is added at idx[n][argmax] with ds_add_f32, then the rows are stored coalesced
//         (gsrc / gx are fully overwritten -> no memset, no global atomics).
#include <type_traits>

#include "gkg_common.h"
#include "gkg_mr_plan.h"

namespace gkg {

// Caller-provided neighbour indices are trusted to be in [0, M); clamping costs two integer ops per index and keeps a
// corrupted index tensor from becoming an out-of-bounds access.
__device__ __forceinline__ int clamp_idx(int64_t v, int M) { return (int)(v < 0 ? 0 : (v >= M ? M - 1 : v)); }

// torch.max semantics for the running maximum (reference torch_vertex.py:54): a NaN candidate replaces a non-NaN best and
// then stays (first NaN wins, like the first-max tie rule), so a diverging run surfaces NaN instead of hiding it.
__device__ __forceinline__ bool takes(float v, float best) { return v > best || (v != v && best == best); }

// ------------------------------------------------------------------------------------------ forward
// These kernels move ~1 flop per byte and, at the sizes of this path, every operand is L2/MALL resident:
// they are bound by memory *latency*, so each thread issues all of its independent loads before the
// first use (index row, centre values, then k gathers per channel from the LDS-staged source rows).
constexpr int MR_CB = 4;        // channels processed together per thread (loads batched across them)

template <typename T>
__global__ __launch_bounds__(256) void mr_fwd_kernel(const T* __restrict__ x, const T* __restrict__ src,
                                                     const int64_t* __restrict__ nn_idx, T* __restrict__ m_out,
                                                     uint8_t* __restrict__ argmax, int c, int N, int M, int k, int CH) {
  extern __shared__ float smem[];
  float* rows = smem;                                   // [CH][M]
  int* idx_s = reinterpret_cast<int*>(smem + (size_t)CH * M);   // [k][256]
  const int tid = threadIdx.x;
  const int bg = blockIdx.z;
  const int ch0 = blockIdx.y * CH;
  const int nch = min(CH, c - ch0);
  const int n0 = blockIdx.x * 256;
  const int n = n0 + tid;

  {
    const T* sp = src + ((size_t)bg * c + ch0) * M;
    const int total = nch * M;
    for (int i = tid; i < total; i += 1024) {
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = (i + 256 * u < total) ? ldf(sp + i + 256 * u) : 0.f;
#pragma unroll
      for (int u = 0; u < 4; ++u) if (i + 256 * u < total) rows[i + 256 * u] = v[u];
    }
    // indices of this tile: (256, k) int64 contiguous -> idx_s[j][q]
    const int64_t* ip = nn_idx + ((size_t)bg * N + n0) * k;
    const int cnt = min(256, N - n0) * k;
    for (int i = tid; i < cnt; i += 1024) {
      int64_t v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = (i + 256 * u < cnt) ? ip[i + 256 * u] : 0;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = i + 256 * u;
        if (e < cnt) { const int q = e / k; idx_s[(e - q * k) * 256 + q] = clamp_idx(v[u], M); }
      }
    }
  }
  __syncthreads();
  if (n >= N) return;
  for (int cb = 0; cb < nch; cb += MR_CB) {
    float xi[MR_CB], best[MR_CB];
    int arg[MR_CB];
#pragma unroll
    for (int u = 0; u < MR_CB; ++u) {
      const int ch = min(cb + u, nch - 1);
      xi[u] = ldf(x + ((size_t)bg * c + ch0 + ch) * N + n);
    }
#pragma unroll
    for (int u = 0; u < MR_CB; ++u) {
      const float* r = rows + (size_t)min(cb + u, nch - 1) * M;
      best[u] = r[idx_s[tid]] - xi[u];
      arg[u] = 0;
    }
    for (int j = 1; j < k; ++j) {
      const int id = idx_s[j * 256 + tid];
#pragma unroll
      for (int u = 0; u < MR_CB; ++u) {
        const float v = rows[(size_t)min(cb + u, nch - 1) * M + id] - xi[u];
        if (takes(v, best[u])) { best[u] = v; arg[u] = j; }
      }
    }
#pragma unroll
    for (int u = 0; u < MR_CB; ++u) {
      if (cb + u < nch) {
        const size_t o = ((size_t)bg * c + ch0 + cb + u) * N + n;
        stf(m_out + o, best[u]);
        if (argmax) argmax[o] = (uint8_t)arg[u];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ backward
template <typename T, bool SELF>
__global__ __launch_bounds__(256) void mr_bwd_kernel(const T* __restrict__ g, const int64_t* __restrict__ nn_idx,
                                                     const uint8_t* __restrict__ argmax, T* __restrict__ gx,
                                                     T* __restrict__ gsrc, int c, int N, int M, int k, int CH) {
  extern __shared__ float smem[];
  float* acc = smem;                                    // [CH][M]
  int* idx_s = reinterpret_cast<int*>(smem + (size_t)CH * M);   // [256][k] as [q*k + j]
  const int tid = threadIdx.x;
  const int bg = blockIdx.y;
  const int ch0 = blockIdx.x * CH;
  const int nch = min(CH, c - ch0);
  const size_t gbase = ((size_t)bg * c + ch0) * N;

  {
    const int total = nch * N;                          // centre term: gx = -g (self: seeds the accumulator)
    for (int i = tid; i < total; i += 1024) {
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = (i + 256 * u < total) ? ldf(g + gbase + i + 256 * u) : 0.f;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = i + 256 * u;
        if (e < total) { if (SELF) acc[e] = -v[u]; else stf(gx + gbase + e, -v[u]); }
      }
    }
    if (!SELF) for (int i = tid; i < nch * M; i += 256) acc[i] = 0.0f;
  }
  for (int n0 = 0; n0 < N; n0 += 256) {
    __syncthreads();                                    // acc init done / previous tile's idx consumed
    const int64_t* ip = nn_idx + ((size_t)bg * N + n0) * k;
    const int cnt = min(256, N - n0) * k;
    for (int i = tid; i < cnt; i += 1024) {
      int64_t v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = (i + 256 * u < cnt) ? ip[i + 256 * u] : 0;
#pragma unroll
      for (int u = 0; u < 4; ++u) if (i + 256 * u < cnt) idx_s[i + 256 * u] = clamp_idx(v[u], M);
    }
    __syncthreads();
    const int n = n0 + tid;
    if (n < N) {
      for (int cb = 0; cb < nch; cb += MR_CB) {
        float gv[MR_CB];
        int am[MR_CB];
#pragma unroll
        for (int u = 0; u < MR_CB; ++u) {
          const size_t o = gbase + (size_t)min(cb + u, nch - 1) * N + n;
          gv[u] = ldf(g + o);
          am[u] = argmax[o];
        }
#pragma unroll
        for (int u = 0; u < MR_CB; ++u)
          if (cb + u < nch) atomicAdd(&acc[(size_t)(cb + u) * M + idx_s[tid * k + min(am[u], k - 1)]], gv[u]);
      }
    }
  }
  __syncthreads();
  T* out = SELF ? gx : gsrc;
  const size_t obase = ((size_t)bg * c + ch0) * M;
  for (int i = tid; i < nch * M; i += 256) stf(out + obase + i, acc[i]);
}

// ------------------------------------------------------------------------------------------ large-M fallbacks
// When one source row (M*4 B) does not fit the LDS budget (label graph over >24k image tokens) the rows stay in
// L2: the forward gathers straight from global memory, the backward scatters with fp32 global atomics.
template <typename T>
__global__ __launch_bounds__(256) void mr_fwd_gather_kernel(const T* __restrict__ x, const T* __restrict__ src,
                                                            const int64_t* __restrict__ nn_idx, T* __restrict__ m_out,
                                                            uint8_t* __restrict__ argmax, int c, int N, int M, int k) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  const int bg = blockIdx.z;
  if (n >= N) return;
  const int64_t* ip = nn_idx + ((size_t)bg * N + n) * k;
  for (int ch = blockIdx.y; ch < c; ch += gridDim.y) {
    const size_t o = ((size_t)bg * c + ch) * N + n;
    const T* r = src + ((size_t)bg * c + ch) * M;
    const float xi = ldf(x + o);
    float best = ldf(r + clamp_idx(ip[0], M)) - xi;
    int arg = 0;
    for (int j = 1; j < k; ++j) {
      const float v = ldf(r + clamp_idx(ip[j], M)) - xi;
      if (takes(v, best)) { best = v; arg = j; }
    }
    stf(m_out + o, best);
    if (argmax) argmax[o] = (uint8_t)arg;
  }
}

__global__ __launch_bounds__(256) void mr_bwd_atomic_kernel(const float* __restrict__ g, const int64_t* __restrict__ nn_idx,
                                                            const uint8_t* __restrict__ argmax, float* __restrict__ gx,
                                                            float* __restrict__ dst, int c, int N, int M, int k, int self) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  const int bg = blockIdx.z;
  if (n >= N) return;
  const int64_t* ip = nn_idx + ((size_t)bg * N + n) * k;
  for (int ch = blockIdx.y; ch < c; ch += gridDim.y) {
    const size_t o = ((size_t)bg * c + ch) * N + n;
    const float gv = g[o];
    if (!self) gx[o] = -gv;
    atomicAdd(dst + ((size_t)bg * c + ch) * M + clamp_idx(ip[min((int)argmax[o], k - 1)], M), gv);
  }
}

__global__ __launch_bounds__(256) void negate_kernel(const float* __restrict__ g, float* __restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = -g[i];
}

// ------------------------------------------------------------------------------------------ token-major variants
// Inside the fused Grapher block activations are token-major (B, N, C): a neighbour is then ONE contiguous row
// segment of c floats, so the aggregation is a coalesced row gather — no LDS staging.  One thread = one token x
// 4 consecutive channels (one group): k float4 gathers + centre float4, all issued before the max chain.
//   mode 0: m (B,N,C) token-major.
//   mode 1: the grouped 1x1 projection's operand buffer XM (T, 2C) (gkg_common.h "XM layout"): the reference's interleave
//           [x_0, m_0, x_1, m_1, ...] (torch_vertex.py:57-61) + Conv2d(groups=4) channel split (torch_nn.py:61) with the
//           columns of each conv group reordered to [x chunk | m chunk] — a permutation of the weight's input columns that the
//           weight-plane build folds in, so nothing is interleaved at run time.  m goes to the m chunks; the x chunks are
//           written only when `write_x` (x does not live in the buffer already: the producer of x writes it there itself).
// x / src are token-major VIEWS (pointer, row pitch, chunk): chunk 0 = plain rows, chunk h = the x half of an XM buffer.
// AK — what `argmax` holds for the backward: 0 = the winning SLOT j (u8, the C-ABI's documented form), 1 = the winning
// neighbour's ROW INDEX itself (u16; needs M <= 65536).  With the row stored the backward scatters straight from it: no
// index-row lookup, i.e. one dependent global round trip less per query and no 72-byte index rows to fetch.
__device__ __forceinline__ int clamp_idx(uint16_t v, int M) { return min((int)v, M - 1); }     // compact lists (gkg_mr_fwd_tm16)

template <int KS, int QP, typename OutT = float, int AK = 0, typename IdxT = int64_t>   // KS: compile-time k (all k index loads and row gathers issued up front);
                            // QP: channel quads per thread (share one index row; QP*4 channels stay inside a group)
                            // OutT: element type of `out` (float, or uint16_t = bf16 for the grouped GEMM's operand)
__global__ __launch_bounds__(256) void mr_fwd_tm_kernel(const float* __restrict__ x, const float* __restrict__ src,
                                                        const IdxT* __restrict__ nn_idx, OutT* __restrict__ out,
                                                        uint8_t* __restrict__ argmax, int B, int G, int c, int N, int M,
                                                        int k_rt, int mode, int ldx, int xchunk, int lds_, int schunk,
                                                        int write_x) {
  const int k = KS > 0 ? KS : k_rt;
  const int C = G * c, CT = C / (4 * QP);                         // thread-columns per token
  const size_t T = (size_t)B * N;
  // XCD-aware map: a token's k neighbours are rows of ITS image, so all workgroups of one image get linear ids that are
  // congruent mod 8 — one XCD, one L2 — and adjacent in dispatch order: the image's rows (N*C*4 bytes: 415 KB at cfg2)
  // are fetched into that L2 once and every gather after the first hits it.  With the plain linear map the k-fold
  // re-reads were spread over all 8 L2s (measured FETCH_SIZE 40 MB per launch against 13 MB of source rows).
  const int bpi = (N * CT + 255) / 256;                          // workgroups per image
  const int lin = blockIdx.x;
  const int xcd = lin & 7, seq = lin >> 3;
  const int b = (seq / bpi) * 8 + xcd;
  if (b >= B) return;                                            // grid padded to a multiple of 8 images
  const int jt = (seq - (seq / bpi) * bpi) * 256 + (int)threadIdx.x;
  if (jt >= N * CT) return;
  const int n = jt / CT;
  const int ch = 4 * QP * (jt - n * CT);
  const size_t t = (size_t)b * N + n;
  const int g = ch / c;
  const IdxT* ip = nn_idx + (((size_t)b * G + g) * N + n) * k;
  const float* sb = src + (size_t)b * M * lds_ + xm_col(ch, schunk);
  const float* xb = x + t * (size_t)ldx + xm_col(ch, xchunk);
  float4 xi[QP], best[QP];
  int ai[QP][4];                                                  // winner per channel: neighbour slot j (AK == 0) / row index (AK == 1)
#pragma unroll
  for (int q = 0; q < QP; ++q) xi[q] = *reinterpret_cast<const float4*>(xb + 4 * q);
  // `takes` (first maximum wins, a NaN is the maximum and sticks) costs 3 compares + 2 scalar mask operations + exec-masked
  // moves per (channel, neighbour): 420 vector + 330 scalar instructions per thread (SQ counters, profiles/r04_pmc_mr_stage1.txt).
  // Fast chain: a plain '>' (identical to `takes` whenever no difference is NaN) while chk accumulates d * 0 — NaN as soon as
  // any difference is NaN or infinite; a wave in which some lane's chk is NaN (non-finite inputs only) redoes its chain with
  // `takes`.  (What bounds the kernel is neither this nor HBM nor the L2 row gathers nor the store pattern — each was
  // removed in turn, EXPERIMENTS.md round 4 — but the in-order vector-memory pipe: a wave's stores are acknowledged 4 k cycles
  // after issue and its first loads return after 8 k under load.)
  auto chain = [&](auto careful, int q, const float4* v, const int* id, int kk) {
    float c0 = 0.f, c1 = 0.f, c2 = 0.f, c3 = 0.f;
    for (int j = 0; j < kk; ++j) {
      const float d0 = v[j].x - xi[q].x, d1 = v[j].y - xi[q].y, d2 = v[j].z - xi[q].z, d3 = v[j].w - xi[q].w;
      const int w = AK == 1 ? id[j] : j;
      if (j == 0) { best[q] = make_float4(d0, d1, d2, d3); ai[q][0] = ai[q][1] = ai[q][2] = ai[q][3] = w; }
      else if constexpr (decltype(careful)::value) {
        if (takes(d0, best[q].x)) { best[q].x = d0; ai[q][0] = w; }
        if (takes(d1, best[q].y)) { best[q].y = d1; ai[q][1] = w; }
        if (takes(d2, best[q].z)) { best[q].z = d2; ai[q][2] = w; }
        if (takes(d3, best[q].w)) { best[q].w = d3; ai[q][3] = w; }
      } else {
        const bool t0 = d0 > best[q].x, t1 = d1 > best[q].y, t2 = d2 > best[q].z, t3 = d3 > best[q].w;
        best[q].x = t0 ? d0 : best[q].x; ai[q][0] = t0 ? w : ai[q][0];
        best[q].y = t1 ? d1 : best[q].y; ai[q][1] = t1 ? w : ai[q][1];
        best[q].z = t2 ? d2 : best[q].z; ai[q][2] = t2 ? w : ai[q][2];
        best[q].w = t3 ? d3 : best[q].w; ai[q][3] = t3 ? w : ai[q][3];
      }
      if constexpr (!decltype(careful)::value) {
        c0 = __builtin_fmaf(d0, 0.f, c0); c1 = __builtin_fmaf(d1, 0.f, c1);
        c2 = __builtin_fmaf(d2, 0.f, c2); c3 = __builtin_fmaf(d3, 0.f, c3);
      }
    }
    return (c0 + c1) + (c2 + c3);
  };
  if (KS > 0) {
    int id[KS > 0 ? KS : 1];
#pragma unroll
    for (int j = 0; j < KS; ++j) id[j] = clamp_idx(ip[j], M);
#pragma unroll
    for (int q = 0; q < QP; ++q) {
      float4 v[KS > 0 ? KS : 1];
#pragma unroll
      for (int j = 0; j < KS; ++j) v[j] = *reinterpret_cast<const float4*>(sb + (size_t)id[j] * lds_ + 4 * q);
      const float chk = chain(std::false_type{}, q, v, id, KS);
      if (__builtin_amdgcn_ballot_w64(chk != chk) != 0ull) (void)chain(std::true_type{}, q, v, id, KS);
    }
  } else {
    for (int j = 0; j < k; ++j) {
      const int rid = clamp_idx(ip[j], M);
      const size_t row = (size_t)rid * lds_;
#pragma unroll
      for (int q = 0; q < QP; ++q) {
        const float4 v = *reinterpret_cast<const float4*>(sb + row + 4 * q);
        const float d0 = v.x - xi[q].x, d1 = v.y - xi[q].y, d2 = v.z - xi[q].z, d3 = v.w - xi[q].w;
        const int w = AK == 1 ? rid : j;
        if (j == 0) { best[q] = make_float4(d0, d1, d2, d3); ai[q][0] = ai[q][1] = ai[q][2] = ai[q][3] = w; continue; }
        if (takes(d0, best[q].x)) { best[q].x = d0; ai[q][0] = w; }
        if (takes(d1, best[q].y)) { best[q].y = d1; ai[q][1] = w; }
        if (takes(d2, best[q].z)) { best[q].z = d2; ai[q][2] = w; }
        if (takes(d3, best[q].w)) { best[q].w = d3; ai[q][3] = w; }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < QP; ++q) {
    const int chq = ch + 4 * q;
    if (argmax) {
      if (AK == 1) *reinterpret_cast<uint2*>(argmax + 2 * (t * C + chq)) =
          make_uint2((uint32_t)ai[q][0] | ((uint32_t)ai[q][1] << 16), (uint32_t)ai[q][2] | ((uint32_t)ai[q][3] << 16));
      else *reinterpret_cast<uint32_t*>(argmax + t * C + chq) =
          (uint32_t)ai[q][0] | ((uint32_t)ai[q][1] << 8) | ((uint32_t)ai[q][2] << 16) | ((uint32_t)ai[q][3] << 24);
    }
    if (mode == 0) {
      stf4(out + t * C + chq, best[q]);
    } else {
      const int Cq = C >> 2;                      // channels per conv group = chunk width of the XM buffer (C % 16 == 0)
      OutT* o = out + t * (size_t)(2 * C) + xm_col(chq, Cq);
      if (write_x) stf4(o, xi[q]);
      stf4(o + Cq, best[q]);
    }
  }
}

// Backward, pass 1: gx[t][ch] = direct[t][ch] - gm[t][ch]   (mode 1: direct / gm are the x / m chunks of dXM)
__global__ __launch_bounds__(256) void mr_bwd_tm_init_kernel(const float* __restrict__ gin, float* __restrict__ gx,
                                                             int C, size_t T, int mode) {
  const int C4 = C >> 2;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= T * C4) return;
  const size_t t = i / C4;
  const int ch = 4 * (int)(i - t * C4);
  float4 o;
  if (mode == 0) {
    const float4 g = *reinterpret_cast<const float4*>(gin + t * C + ch);
    o = make_float4(-g.x, -g.y, -g.z, -g.w);
  } else {
    const int Cq = C >> 2;
    const float* p = gin + t * (size_t)(2 * C) + xm_col(ch, Cq);
    const float4 u0 = *reinterpret_cast<const float4*>(p), u1 = *reinterpret_cast<const float4*>(p + Cq);
    o = make_float4(u0.x - u1.x, u0.y - u1.y, u0.z - u1.z, u0.w - u1.w);
  }
  *reinterpret_cast<float4*>(gx + t * C + ch) = o;
}

// Backward in ONE kernel.  One workgroup = one image x a chunk of CW channels; the destination rows of that (image,
// chunk) live in LDS ([M][CW] fp32).  Phase 1 seeds the image: self graph -> gx seed = direct - gm (read straight
// from the upstream gradient), bipartite graph -> zeros.  Phase 2 sweeps all N queries: gm is added at
// idx[n][argmax] with ds_add_f32 and, for the bipartite graph, gx = direct - gm is stored on the way.  Phase 3
// stores the image rows.  gx / gsrc are fully overwritten, no global atomics, no separate init pass.
// MODE / AK as template constants in the LDS-image kernels: with run-time `mode` / `ak` branches the float4 pairs and the
// target array went through SCRATCH memory (24 scratch_load/store_dword between the ds_add_f32 of the inner loop,
// .private_segment_fixed_size 40 — VERDICT r3); the run-time forms (MODE < 0) remain for the global-atomic fallbacks.
template <int MODE = -1>
__device__ __forceinline__ void load_grad(const float* __restrict__ gin, size_t T, size_t t, int C, int ch, int mode,
                                          float4& direct, float4& gm) {
  if (MODE >= 0) mode = MODE;
  if (mode == 0) {
    gm = *reinterpret_cast<const float4*>(gin + t * C + ch);
    direct = make_float4(0.f, 0.f, 0.f, 0.f);
  } else {                                     // XM layout (T, 2C): the x chunk carries the direct gradient, the m chunk gm
    const int Cq = C >> 2;
    const float* p = gin + t * (size_t)(2 * C) + xm_col(ch, Cq);
    direct = *reinterpret_cast<const float4*>(p);
    gm = *reinterpret_cast<const float4*>(p + Cq);
  }
}

// destination rows of the 4 channels of one thread: from the winning slots + the index row (AK == 0) or directly (AK == 1)
template <int AK = -1>
__device__ __forceinline__ void mr_targets(const uint8_t* __restrict__ argmax, int ak, size_t elem, const int64_t* __restrict__ ip,
                                           int k, int M, int (&j)[4]) {
  if (AK >= 0) ak = AK;
  if (ak == 1) {
    const uint2 v = *reinterpret_cast<const uint2*>(argmax + 2 * elem);
    j[0] = min((int)(v.x & 0xffff), M - 1); j[1] = min((int)(v.x >> 16), M - 1);
    j[2] = min((int)(v.y & 0xffff), M - 1); j[3] = min((int)(v.y >> 16), M - 1);
  } else {
    const uint32_t am = *reinterpret_cast<const uint32_t*>(argmax + elem);
    const int km = k - 1;
    j[0] = clamp_idx(ip[min((int)(am & 0xff), km)], M); j[1] = clamp_idx(ip[min((int)((am >> 8) & 0xff), km)], M);
    j[2] = clamp_idx(ip[min((int)((am >> 16) & 0xff), km)], M); j[3] = clamp_idx(ip[min((int)((am >> 24) & 0xff), km)], M);
  }
}

template <bool SELF, int MODE, int AK>
__global__ __launch_bounds__(256) void mr_bwd_tm_scatter_kernel(const float* __restrict__ gin, const int64_t* __restrict__ nn_idx,
                                                                const uint8_t* __restrict__ argmax, float* __restrict__ gx,
                                                                float* __restrict__ gsrc, int B, int G, int c, int N, int M,
                                                                int k, int mode, int CW, int ak) {
  extern __shared__ float acc[];                  // [M][CW]
  const int C = G * c;
  // XCD-aware map (see mr_fwd_tm_kernel): the C/CW channel-chunk workgroups of one image read interleaved pieces of the
  // same gradient rows and index rows -> same XCD, adjacent in dispatch order
  const int nchunk = C / CW;
  const int lin = blockIdx.x;
  const int xcd = lin & 7, seq = lin >> 3;
  const int b = (seq / nchunk) * 8 + xcd;
  if (b >= B) return;
  const int ch0 = (seq - (seq / nchunk) * nchunk) * CW;
  const int cw4 = CW >> 2;                        // quads per row chunk
  const int tid = threadIdx.x;
  const int qd = tid % cw4, tl = tid / cw4, TL = 256 / cw4;
  const size_t T = (size_t)B * N;
  const int ch = ch0 + 4 * qd;
  // phase 1: seed the LDS image (self graph: a token's own "direct - gm"; bipartite graph: zeros).  Seeding with the same
  // LDS atomics as the scatter, to read every gradient row once instead of twice, was measured SLOWER (31.8 -> 40 us at
  // cfg2): the second read hits L2, the four extra atomics per row do not come free.
  if (tl < TL) {
    for (int m = tl; m < M; m += TL) {
      float4 seed = make_float4(0.f, 0.f, 0.f, 0.f);
      if (SELF) {
        float4 direct, gm;
        load_grad<MODE>(gin, T, (size_t)b * N + m, C, ch, mode, direct, gm);
        seed = make_float4(direct.x - gm.x, direct.y - gm.y, direct.z - gm.z, direct.w - gm.w);
      }
      *reinterpret_cast<float4*>(acc + (size_t)m * CW + 4 * qd) = seed;
    }
  }
  __syncthreads();
  // phase 2: sweep the queries; the destination rows come straight from the saved row indices (arg kind 1)
  if (tl < TL) {
    const int g = ch / c;
    for (int n = tl; n < N; n += TL) {
      const size_t t = (size_t)b * N + n;
      const int64_t* ip = nn_idx + (((size_t)b * G + g) * N + n) * k;
      int j[4];
      mr_targets<AK>(argmax, ak, t * C + ch, ip, k, M, j);
      float4 direct, gm;
      load_grad<MODE>(gin, T, t, C, ch, mode, direct, gm);
      if (!SELF)
        *reinterpret_cast<float4*>(gx + t * C + ch) = make_float4(direct.x - gm.x, direct.y - gm.y, direct.z - gm.z, direct.w - gm.w);
      atomicAdd(acc + (size_t)j[0] * CW + 4 * qd + 0, gm.x);
      atomicAdd(acc + (size_t)j[1] * CW + 4 * qd + 1, gm.y);
      atomicAdd(acc + (size_t)j[2] * CW + 4 * qd + 2, gm.z);
      atomicAdd(acc + (size_t)j[3] * CW + 4 * qd + 3, gm.w);
    }
  }
  __syncthreads();
  if (tl < TL) {
    float* db = (SELF ? gx : gsrc) + (size_t)b * M * C + ch0;
    for (int m = tl; m < M; m += TL)
      *reinterpret_cast<float4*>(db + (size_t)m * C + 4 * qd) = *reinterpret_cast<const float4*>(acc + (size_t)m * CW + 4 * qd);
  }
}

// ---- exact integer accumulation (round 4; the default LDS-image form) -------------------------------------------------------
// Hardware fact (tools/ubench/lds_atomic_rate.hip, profiles/r04_ubench_lds_atomic_rate.txt, SQ counters in
// profiles/r04_pmc_mr_stage1.txt): on gfx950 `ds_add_f32` retires at ~170 cycles per wave instruction (2.7 cycles per LANE,
// whatever the addresses), `ds_add_u64` at 30-66, `ds_add_u32` at 16-31.  The fp32 scatter above spends two thirds of its
// time in the LDS atomic unit.  This form accumulates in 64-bit FIXED POINT instead:
//   sweep 1  over the workgroup's (image, channel chunk): gx = direct - gm (bipartite graphs) and the largest |gm| bit
//            pattern (ds_max_u32) -> e_max, the scale of this workgroup;
//   sweep 2  every gm becomes  sign * (24-bit mantissa << sh),  sh = e - e_max + SHMAX  with SHMAX = 38 - bits(N): the
//            largest value keeps 24 + SHMAX bits, the sum of up to N of them fits 62 bits, values down to 2^-SHMAX of the
//            largest keep their FULL mantissa (29 binary orders at N = 324, 23 at N = 20 736; below that the low bits are
//            truncated — against a total that is then >= 2^24 times larger); one ds_add_u64 per value;
//   store    acc * 2^(e_max - 150 - SHMAX) converted to fp32 at the end — through a double (53 bits), so the 62-bit total is
//            rounded twice, not once, and the self graphs' "direct - gm" seed is one more fp32 add.
// Integer addition is associative: the result does not depend on the order the lanes arrive in — bit-identical from run
// to run (this form also serves GKG_MR_DETERMINISTIC) — and the sum carries the rounding of its conversion only (plus the
// truncation of addends more than 2^-SHMAX below the chunk's largest), where an fp32 atomic chain rounds after every addend:
// deterministic and at least as accurate as the fp32 sum, not "correctly rounded".  Non-finite gradients (the GradScaler overflow protocol needs inf / NaN
// to reach the parameters) show up as e_max = 255: the workgroup then re-runs the fp32-atomic form on the same LDS.
__device__ __forceinline__ long long mr_to_fixed(float v, int emax, int shmax) {
  const unsigned bits = __float_as_uint(v);
  const int e = (int)((bits >> 23) & 0xff);
  const unsigned long long mant = (unsigned long long)((bits & 0x7fffffu) | (e ? 0x800000u : 0u));
  const int sh = (e ? e : 1) - emax + shmax;
  const unsigned long long mag = sh >= 0 ? (mant << sh) : (mant >> min(-sh, 63));
  return (bits >> 31) ? -(long long)mag : (long long)mag;
}
__device__ __forceinline__ float mr_from_fixed(long long a, int emax, int shmax) {
  return (float)__builtin_ldexp((double)a, emax - 150 - shmax);
}

// ---- BN backward statistics in the scatter (round 8, gkg_mr_bwd_tm_bnstats) ------------------------------------------------
// gx is the upstream gradient of the layer  x = BN(y)  in front of the aggregation (a Grapher's fc1, act == 0).  A STATS
// instantiation reads y next to every FINAL gx value it stores (the store phase of the self graph, the first sweep of the
// bipartite one) and keeps  sum g, sum g * yhat  (yhat = (y - mean) * invstd) for the thread's four channels; at its exit the
// workgroup (one image x one channel chunk x all rows) combines its row lanes — across the lanes of a wave by shuffles, across
// the waves through LDS, in fp64 — and adds ONE fp64 atomic pair per channel to `sums` ([2][C], zero on entry): what
// bn_bwd_stats_kernel<0> would have left there after a pass of its own over gx and y.  gx / gsrc are untouched.
struct MrBnArgs { const float* y; const float* mean; const float* invstd; double* sums; };

template <bool ON> struct MrStat {};
template <> struct MrStat<true> {
  const float* y;
  float4 m4, i4, s, q;
  __device__ __forceinline__ void init(const MrBnArgs& a, int ch) {
    y = a.y;
    m4 = *reinterpret_cast<const float4*>(a.mean + ch);
    i4 = *reinterpret_cast<const float4*>(a.invstd + ch);
    s = make_float4(0.f, 0.f, 0.f, 0.f);
    q = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  // g: the four gx values stored at element offset `off` of the (T, C) gradient — y has the same shape
  __device__ __forceinline__ float4 ld(size_t off) const { return *reinterpret_cast<const float4*>(y + off); }
  __device__ __forceinline__ void add(const float4& g, size_t off) { acc(g, ld(off)); }
  // (ld early — with the iteration's other loads — and acc once g is known keeps y's latency off the store loops)
  __device__ __forceinline__ void acc(const float4& g, const float4& v) {
    s.x += g.x; s.y += g.y; s.z += g.z; s.w += g.w;
    q.x += g.x * ((v.x - m4.x) * i4.x); q.y += g.y * ((v.y - m4.y) * i4.y);
    q.z += g.z * ((v.z - m4.z) * i4.z); q.w += g.w * ((v.w - m4.w) * i4.w);
  }
  // every thread of the workgroup, from uniform control flow; `lds`: the accumulator image (free after the barrier), at least
  // (NT / 64) * 2 * CW doubles.  CW is 4, 8 or 16: the lanes of a wave that share a channel quad are lane % (CW / 4).
  template <int NT>
  __device__ __forceinline__ void flush(void* lds, double* __restrict__ sums, int C, int ch0, int CW) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, cw4 = CW >> 2;
    double d[8] = {(double)s.x, (double)s.y, (double)s.z, (double)s.w, (double)q.x, (double)q.y, (double)q.z, (double)q.w};
    for (int o = 32; o >= cw4; o >>= 1) {
#pragma unroll
      for (int i = 0; i < 8; ++i) d[i] += __shfl_xor(d[i], o);
    }
    __syncthreads();
    double* red = reinterpret_cast<double*>(lds);       // [wave][2][CW]
    if (lane < cw4) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        red[(wave * 2 + 0) * CW + 4 * lane + i] = d[i];
        red[(wave * 2 + 1) * CW + 4 * lane + i] = d[4 + i];
      }
    }
    __syncthreads();
    if (tid < 2 * CW) {
      const int which = tid / CW, col = tid - which * CW;
      double a = 0.0;
#pragma unroll
      for (int w = 0; w < NT / 64; ++w) a += red[(w * 2 + which) * CW + col];
      __hip_atomic_fetch_add(sums + (size_t)which * C + ch0 + col, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
};

template <bool SELF, int MODE, int AK, bool STATS = false>
__device__ __forceinline__ void mr_scatter_f32_body(float* acc, const float* __restrict__ gin, const int64_t* __restrict__ nn_idx,
                                                    const uint8_t* __restrict__ argmax, float* __restrict__ gx,
                                                    float* __restrict__ gsrc, int b, int G, int c, int N, int M, int k, int CW,
                                                    int ch0, size_t T, bool write_gx, MrStat<STATS>* stat = nullptr) {
  const int C = G * c;
  const int cw4 = CW >> 2;
  const int tid = threadIdx.x;
  const int qd = tid % cw4, tl = tid / cw4, TL = 256 / cw4;
  const int ch = ch0 + 4 * qd;
  if (tl < TL) {
    for (int m = tl; m < M; m += TL) {
      float4 seed = make_float4(0.f, 0.f, 0.f, 0.f);
      if (SELF) {
        float4 direct, gm;
        load_grad<MODE>(gin, T, (size_t)b * N + m, C, ch, MODE, direct, gm);
        seed = make_float4(direct.x - gm.x, direct.y - gm.y, direct.z - gm.z, direct.w - gm.w);
      }
      *reinterpret_cast<float4*>(acc + (size_t)m * CW + 4 * qd) = seed;
    }
  }
  __syncthreads();
  if (tl < TL) {
    const int g = ch / c;
    for (int n = tl; n < N; n += TL) {
      const size_t t = (size_t)b * N + n;
      const int64_t* ip = nn_idx + (((size_t)b * G + g) * N + n) * k;
      int j[4];
      mr_targets<AK>(argmax, AK, t * C + ch, ip, k, M, j);
      float4 direct, gm;
      load_grad<MODE>(gin, T, t, C, ch, MODE, direct, gm);
      if (!SELF && write_gx) {
        const float4 o = make_float4(direct.x - gm.x, direct.y - gm.y, direct.z - gm.z, direct.w - gm.w);
        if constexpr (STATS) stat->add(o, t * C + ch);
        *reinterpret_cast<float4*>(gx + t * C + ch) = o;
      }
      atomicAdd(acc + (size_t)j[0] * CW + 4 * qd + 0, gm.x);
      atomicAdd(acc + (size_t)j[1] * CW + 4 * qd + 1, gm.y);
      atomicAdd(acc + (size_t)j[2] * CW + 4 * qd + 2, gm.z);
      atomicAdd(acc + (size_t)j[3] * CW + 4 * qd + 3, gm.w);
    }
  }
  __syncthreads();
  if (tl < TL) {
    float* db = (SELF ? gx : gsrc) + (size_t)b * M * C + ch0;
    for (int m = tl; m < M; m += TL) {
      const float4 o = *reinterpret_cast<const float4*>(acc + (size_t)m * CW + 4 * qd);
      if constexpr (STATS && SELF) stat->add(o, ((size_t)b * M + m) * C + ch);
      *reinterpret_cast<float4*>(db + (size_t)m * C + 4 * qd) = o;
    }
  }
}

template <bool SELF, int MODE, int AK, bool STATS = false>
__global__ __launch_bounds__(256) void mr_bwd_tm_scatter_i64_kernel(const float* __restrict__ gin, const int64_t* __restrict__ nn_idx,
                                                                    const uint8_t* __restrict__ argmax, float* __restrict__ gx,
                                                                    float* __restrict__ gsrc, int B, int G, int c, int N, int M,
                                                                    int k, int CW, int shmax, MrBnArgs bn = MrBnArgs{}) {
  extern __shared__ long long acc64[];            // [M][CW] + control words
  const int C = G * c;
  const int nchunk = C / CW;
  const int lin = blockIdx.x;
  const int xcd = lin & 7, seq = lin >> 3;        // XCD-aware map, as mr_bwd_tm_scatter_kernel
  const int b = (seq / nchunk) * 8 + xcd;
  if (b >= B) return;
  const int ch0 = (seq - (seq / nchunk) * nchunk) * CW;
  const int cw4 = CW >> 2;
  const int tid = threadIdx.x;
  const int qd = tid % cw4, tl = tid / cw4, TL = 256 / cw4;
  const size_t T = (size_t)B * N;
  const int ch = ch0 + 4 * qd;
  unsigned* ctl = reinterpret_cast<unsigned*>(acc64 + (size_t)M * CW);
  for (int i = tid; i < M * CW; i += 256) acc64[i] = 0;
  if (tid == 0) ctl[0] = 0;
  __syncthreads();
  // ---- sweep 1: gx of the bipartite graph, and the chunk's largest |gm| bit pattern
  unsigned mx = 0;
  MrStat<STATS> stat;
  if constexpr (STATS) stat.init(bn, ch);
  if (tl < TL) {
    for (int n = tl; n < N; n += TL) {
      const size_t t = (size_t)b * N + n;
      float4 direct, gm, yv;
      if constexpr (STATS && !SELF) yv = stat.ld(t * C + ch);
      load_grad<MODE>(gin, T, t, C, ch, MODE, direct, gm);
      if (!SELF) {
        const float4 o = make_float4(direct.x - gm.x, direct.y - gm.y, direct.z - gm.z, direct.w - gm.w);
        if constexpr (STATS) stat.acc(o, yv);
        *reinterpret_cast<float4*>(gx + t * C + ch) = o;
      }
      mx = max(max(mx, __float_as_uint(gm.x) & 0x7fffffffu), max(__float_as_uint(gm.y) & 0x7fffffffu,
               max(__float_as_uint(gm.z) & 0x7fffffffu, __float_as_uint(gm.w) & 0x7fffffffu)));
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) mx = max(mx, (unsigned)__shfl_xor((int)mx, o));
  if ((tid & 63) == 0) atomicMax(ctl, mx);
  __syncthreads();
  mx = ctl[0];
  const int emax = (int)(mx >> 23);
  if (emax == 255) {                              // inf / NaN somewhere in this chunk: the fp32-atomic form propagates them
    __syncthreads();
    mr_scatter_f32_body<SELF, MODE, AK, STATS>(reinterpret_cast<float*>(acc64), gin, nn_idx, argmax, gx, gsrc, b, G, c, N, M, k, CW, ch0,
                                               T, false, &stat);
    if constexpr (STATS) stat.template flush<256>(acc64, bn.sums, C, ch0, CW);
    return;
  }
  // ---- sweep 2: exact accumulation
  if (tl < TL && mx != 0) {
    const int g = ch / c;
    const int em = max(emax, 1);
    for (int n = tl; n < N; n += TL) {
      const size_t t = (size_t)b * N + n;
      const int64_t* ip = nn_idx + (((size_t)b * G + g) * N + n) * k;
      int j[4];
      mr_targets<AK>(argmax, AK, t * C + ch, ip, k, M, j);
      float4 direct, gm;
      load_grad<MODE>(gin, T, t, C, ch, MODE, direct, gm);
      atomicAdd(reinterpret_cast<unsigned long long*>(acc64 + (size_t)j[0] * CW + 4 * qd + 0), (unsigned long long)mr_to_fixed(gm.x, em, shmax));
      atomicAdd(reinterpret_cast<unsigned long long*>(acc64 + (size_t)j[1] * CW + 4 * qd + 1), (unsigned long long)mr_to_fixed(gm.y, em, shmax));
      atomicAdd(reinterpret_cast<unsigned long long*>(acc64 + (size_t)j[2] * CW + 4 * qd + 2), (unsigned long long)mr_to_fixed(gm.z, em, shmax));
      atomicAdd(reinterpret_cast<unsigned long long*>(acc64 + (size_t)j[3] * CW + 4 * qd + 3), (unsigned long long)mr_to_fixed(gm.w, em, shmax));
    }
  }
  __syncthreads();
  // ---- store: one rounding per element (+ the token's own seed for the self graph)
  if (tl < TL) {
    const int em = max(emax, 1);
    float* db = (SELF ? gx : gsrc) + (size_t)b * M * C + ch0;
    for (int m = tl; m < M; m += TL) {
      const long long* a = acc64 + (size_t)m * CW + 4 * qd;
      float4 o = make_float4(mr_from_fixed(a[0], em, shmax), mr_from_fixed(a[1], em, shmax), mr_from_fixed(a[2], em, shmax),
                             mr_from_fixed(a[3], em, shmax));
      if (SELF) {
        float4 direct, gm;
        load_grad<MODE>(gin, T, (size_t)b * N + m, C, ch, MODE, direct, gm);
        o = make_float4(o.x + (direct.x - gm.x), o.y + (direct.y - gm.y), o.z + (direct.z - gm.z), o.w + (direct.w - gm.w));
      }
      if constexpr (STATS && SELF) stat.add(o, ((size_t)b * M + m) * C + ch);
      *reinterpret_cast<float4*>(db + (size_t)m * C + 4 * qd) = o;
    }
  }
  if constexpr (STATS) stat.template flush<256>(acc64, bn.sums, C, ch0, CW);
}

// ---- streaming form of the exact scatter (round 5) ----------------------------------------------------------------------
// At the HBM-bound shapes (pooled 1 296-key images under 5 184 / 20 736 queries, the 36 x 36 self graphs) BOTH kernels above take
// the same time whatever their accumulator type (tools/bench_mr_bwd.py: 420-426 us at stage 1 for fp32 and 64-bit atomics, chunk
// widths 4 / 8): they are bound by their sweep — one (index, gradient) row per thread and iteration, nothing in flight behind
// it — and the fixed-point form pays that sweep twice to learn its scale first.  This form
//   * keeps U = 4 / 8 rows per thread in flight (all winning-row / gradient loads of an iteration issued before the first use) in
//     512-thread workgroups: one workgroup per CU (83 KB of accumulators at 1 296 rows x 8 channels) still has >= 80 KB of loads
//     outstanding (1 024-thread workgroups measured the same);
//   * sweeps ONCE: the fixed-point scale is the exact maximum when a thread's first U rows are the whole sweep (the 18 x 18
//     stages: the two-sweep kernel's bits), otherwise the maximum of a strided SAMPLE of the chunk's rows (requested together
//     with the first iteration's rows: one round trip) plus HEAD binary orders of headroom.  A gradient beyond the headroom (or
//     inf / NaN) raises a flag; the
//     workgroup then discards its image and re-runs the exact two-sweep form — same result contract, rare path.  The sample,
//     the flag and therefore the path taken depend on the data only: bit-identical from run to run, like the two-sweep form
//     (the scale sits HEAD orders above the sampled maximum: values more than 2^-(SHMAX - HEAD) below THAT lose low bits —
//     17 binary orders at N = 20 736).
// ACC == 1 (measurement): fp64 LDS atomics (ds_add_f64) instead of fixed point — no scale at all, not order-independent.
template <int NT, bool SELF, int MODE, int AK, bool STATS = false>
__device__ __forceinline__ void mr_i64_two_sweep_body(long long* acc64, unsigned* ctl, const float* __restrict__ gin,
                                                      const int64_t* __restrict__ nn_idx, const uint8_t* __restrict__ argmax,
                                                      float* __restrict__ gx, float* __restrict__ gsrc, int b, int G, int c, int N,
                                                      int M, int k, int CW, int ch0, size_t T, int shmax, bool write_gx,
                                                      MrStat<STATS>* stat = nullptr) {
  const int C = G * c;
  const int cw4 = CW >> 2;
  const int tid = threadIdx.x;
  const int qd = tid % cw4, tl = tid / cw4, TL = NT / cw4;
  const int ch = ch0 + 4 * qd;
  unsigned mx = 0;
  if (tl < TL) {
    for (int n = tl; n < N; n += TL) {
      const size_t t = (size_t)b * N + n;
      float4 direct, gm;
      load_grad<MODE>(gin, T, t, C, ch, MODE, direct, gm);
      if (!SELF && write_gx) {
        const float4 o = make_float4(direct.x - gm.x, direct.y - gm.y, direct.z - gm.z, direct.w - gm.w);
        if constexpr (STATS) stat->add(o, t * C + ch);
        *reinterpret_cast<float4*>(gx + t * C + ch) = o;
      }
      mx = max(max(mx, __float_as_uint(gm.x) & 0x7fffffffu), max(__float_as_uint(gm.y) & 0x7fffffffu,
               max(__float_as_uint(gm.z) & 0x7fffffffu, __float_as_uint(gm.w) & 0x7fffffffu)));
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) mx = max(mx, (unsigned)__shfl_xor((int)mx, o));
  if ((tid & 63) == 0) atomicMax(ctl, mx);
  __syncthreads();
  mx = ctl[0];
  const int emax = (int)(mx >> 23);
  if (emax == 255) {                              // inf / NaN somewhere in this chunk: the fp32-atomic form propagates them
    __syncthreads();
    float* acc = reinterpret_cast<float*>(acc64);   // fp32 atomics on the same LDS (mr_scatter_f32_body for NT threads)
    if (tl < TL) {
      for (int m = tl; m < M; m += TL) {
        float4 seed = make_float4(0.f, 0.f, 0.f, 0.f);
        if (SELF) {
          float4 direct, gm;
          load_grad<MODE>(gin, T, (size_t)b * N + m, C, ch, MODE, direct, gm);
          seed = make_float4(direct.x - gm.x, direct.y - gm.y, direct.z - gm.z, direct.w - gm.w);
        }
        *reinterpret_cast<float4*>(acc + (size_t)m * CW + 4 * qd) = seed;
      }
    }
    __syncthreads();
    if (tl < TL) {
      const int g = ch / c;
      for (int n = tl; n < N; n += TL) {
        const size_t t = (size_t)b * N + n;
        const int64_t* ip = nn_idx + (((size_t)b * G + g) * N + n) * k;
        int j[4];
        mr_targets<AK>(argmax, AK, t * C + ch, ip, k, M, j);
        float4 direct, gm;
        load_grad<MODE>(gin, T, t, C, ch, MODE, direct, gm);
        atomicAdd(acc + (size_t)j[0] * CW + 4 * qd + 0, gm.x);
        atomicAdd(acc + (size_t)j[1] * CW + 4 * qd + 1, gm.y);
        atomicAdd(acc + (size_t)j[2] * CW + 4 * qd + 2, gm.z);
        atomicAdd(acc + (size_t)j[3] * CW + 4 * qd + 3, gm.w);
      }
    }
    __syncthreads();
    if (tl < TL) {
      float* db = (SELF ? gx : gsrc) + (size_t)b * M * C + ch0;
      for (int m = tl; m < M; m += TL) {
        const float4 o = *reinterpret_cast<const float4*>(acc + (size_t)m * CW + 4 * qd);
        if constexpr (STATS && SELF) stat->add(o, ((size_t)b * M + m) * C + ch);
        *reinterpret_cast<float4*>(db + (size_t)m * C + 4 * qd) = o;
      }
    }
    return;
  }
  if (tl < TL && mx != 0) {
    const int g = ch / c;
    const int em = max(emax, 1);
    for (int n = tl; n < N; n += TL) {
      const size_t t = (size_t)b * N + n;
      const int64_t* ip = nn_idx + (((size_t)b * G + g) * N + n) * k;
      int j[4];
      mr_targets<AK>(argmax, AK, t * C + ch, ip, k, M, j);
      float4 direct, gm;
      load_grad<MODE>(gin, T, t, C, ch, MODE, direct, gm);
      atomicAdd(reinterpret_cast<unsigned long long*>(acc64 + (size_t)j[0] * CW + 4 * qd + 0), (unsigned long long)mr_to_fixed(gm.x, em, shmax));
      atomicAdd(reinterpret_cast<unsigned long long*>(acc64 + (size_t)j[1] * CW + 4 * qd + 1), (unsigned long long)mr_to_fixed(gm.y, em, shmax));
      atomicAdd(reinterpret_cast<unsigned long long*>(acc64 + (size_t)j[2] * CW + 4 * qd + 2), (unsigned long long)mr_to_fixed(gm.z, em, shmax));
      atomicAdd(reinterpret_cast<unsigned long long*>(acc64 + (size_t)j[3] * CW + 4 * qd + 3), (unsigned long long)mr_to_fixed(gm.w, em, shmax));
    }
  }
  __syncthreads();
  if (tl < TL) {
    const int em = max(emax, 1);
    float* db = (SELF ? gx : gsrc) + (size_t)b * M * C + ch0;
    for (int m = tl; m < M; m += TL) {
      const long long* a = acc64 + (size_t)m * CW + 4 * qd;
      float4 o = make_float4(mr_from_fixed(a[0], em, shmax), mr_from_fixed(a[1], em, shmax), mr_from_fixed(a[2], em, shmax),
                             mr_from_fixed(a[3], em, shmax));
      if (SELF) {
        float4 direct, gm;
        load_grad<MODE>(gin, T, (size_t)b * N + m, C, ch, MODE, direct, gm);
        o = make_float4(o.x + (direct.x - gm.x), o.y + (direct.y - gm.y), o.z + (direct.z - gm.z), o.w + (direct.w - gm.w));
      }
      if constexpr (STATS && SELF) stat->add(o, ((size_t)b * M + m) * C + ch);
      *reinterpret_cast<float4*>(db + (size_t)m * C + 4 * qd) = o;
    }
  }
}

constexpr int MR_STREAM_HEAD = 6;       // binary orders of headroom above the sampled maximum

template <int NT, bool SELF, int MODE, int AK, int ACC, int U, bool STATS = false>     // U: rows in flight per thread
__global__ __launch_bounds__(NT) void mr_bwd_tm_stream_kernel(const float* __restrict__ gin, const int64_t* __restrict__ nn_idx,
                                                               const uint8_t* __restrict__ argmax, float* __restrict__ gx,
                                                               float* __restrict__ gsrc, int B, int G, int c, int N, int M,
                                                               int k, int CW, int shmax, int arg_planes, MrBnArgs bn = MrBnArgs{}) {
  extern __shared__ long long acc64[];            // [M][CW] (fixed point, or the bits of doubles) + control words
  const int C = G * c;
  const int nchunk = C / CW;
  const int lin = blockIdx.x;
  const int xcd = lin & 7, seq = lin >> 3;        // XCD-aware map, as mr_bwd_tm_scatter_kernel
  const int b = (seq / nchunk) * 8 + xcd;
  if (b >= B) return;
  const int ch0 = (seq - (seq / nchunk) * nchunk) * CW;
  const int cw4 = CW >> 2;
  const int tid = threadIdx.x;
  const int qd = tid % cw4, tl = tid / cw4, TL = NT / cw4;
  const size_t T = (size_t)B * N;
  const int ch = ch0 + 4 * qd;
  const int g = ch / c;
  unsigned* ctl = reinterpret_cast<unsigned*>(acc64 + (size_t)M * CW);
  // arg_planes (measurement, AK == 1): the winning rows as 8-channel planes (B, C / 8, N, 8) instead of (B, N, C) rows — a chunk's
  // 16 bytes per query row are then contiguous over the rows
  const size_t pl_base = (((size_t)b * (C >> 3) + (ch >> 3)) * N) * 8 + (ch & 7);
  float4 direct[U], gm[U];
  int j[U][4];
  auto load_rows = [&](int n0) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int n = min(n0 + u * TL, N - 1);
      const size_t t = (size_t)b * N + n;
      const int64_t* ip = AK == 1 ? nullptr : nn_idx + (((size_t)b * G + g) * N + n) * k;
      mr_targets<AK>(argmax, AK, arg_planes ? pl_base + (size_t)n * 8 : t * C + ch, ip, k, M, j[u]);
      load_grad<MODE>(gin, T, t, C, ch, MODE, direct[u], gm[u]);
    }
  };
  auto absmax4 = [](const float4& v) -> unsigned {
    return max(max(__float_as_uint(v.x) & 0x7fffffffu, __float_as_uint(v.y) & 0x7fffffffu),
               max(__float_as_uint(v.z) & 0x7fffffffu, __float_as_uint(v.w) & 0x7fffffffu));
  };
  // ---- prologue: the first U rows of every thread AND (longer sweeps) a strided sample of the chunk's rows are requested in one
  //      go; the LDS image is cleared in their shadow.  The fixed-point scale comes from what arrived: the exact maximum when the
  //      first iteration is the whole sweep (N <= TL * U: the 18 x 18 stages — no headroom needed, the flag cannot rise), the
  //      sample's maximum plus HEAD binary orders otherwise.
  const bool whole = N <= TL * U;                 // uniform
  unsigned mx = 0;
  float4 sd[2], sg[2];
  if (ACC == 0 && !whole) {
    const int stride = max(N / (TL * 2), 1);
#pragma unroll
    for (int u = 0; u < 2; ++u)
      load_grad<MODE>(gin, T, (size_t)b * N + min((tl + u * TL) * stride, N - 1), C, ch, MODE, sd[u], sg[u]);
  }
  load_rows(tl);
  for (int i = tid; i < M * CW; i += NT) acc64[i] = 0;
  if (tid == 0) { ctl[0] = 0; ctl[1] = 0; }
  __syncthreads();
  int em = 0;
  unsigned lim = 0xffffffffu;
  if (ACC == 0) {
    if (!whole) mx = max(absmax4(sg[0]), absmax4(sg[1]));
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (tl + u * TL < N) mx = max(mx, absmax4(gm[u]));
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mx = max(mx, (unsigned)__shfl_xor((int)mx, o));
    if ((tid & 63) == 0) atomicMax(ctl, mx);
    __syncthreads();
    mx = ctl[0];
    // an all-zero (or denormal) sample still gets a scale — whatever lies above it raises the flag
    em = min(max((int)(mx >> 23), 1) + (whole ? 0 : MR_STREAM_HEAD), 254);
    lim = (unsigned)(em + 1) << 23;               // |bits| >= lim: beyond the scale (inf / NaN always are)
  }
  bool over = false;
  MrStat<STATS> stat;
  if constexpr (STATS) stat.init(bn, ch);
  auto process_rows = [&](int n0) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int n = n0 + u * TL;
      if (n < N) {
        const size_t t = (size_t)b * N + n;
        if (!SELF) {
          const float4 o = make_float4(direct[u].x - gm[u].x, direct[u].y - gm[u].y, direct[u].z - gm[u].z, direct[u].w - gm[u].w);
          if constexpr (STATS) stat.add(o, t * C + ch);
          *reinterpret_cast<float4*>(gx + t * C + ch) = o;
        }
        if (ACC == 0) {
          over |= absmax4(gm[u]) >= lim;
          atomicAdd(reinterpret_cast<unsigned long long*>(acc64 + (size_t)j[u][0] * CW + 4 * qd + 0), (unsigned long long)mr_to_fixed(gm[u].x, em, shmax));
          atomicAdd(reinterpret_cast<unsigned long long*>(acc64 + (size_t)j[u][1] * CW + 4 * qd + 1), (unsigned long long)mr_to_fixed(gm[u].y, em, shmax));
          atomicAdd(reinterpret_cast<unsigned long long*>(acc64 + (size_t)j[u][2] * CW + 4 * qd + 2), (unsigned long long)mr_to_fixed(gm[u].z, em, shmax));
          atomicAdd(reinterpret_cast<unsigned long long*>(acc64 + (size_t)j[u][3] * CW + 4 * qd + 3), (unsigned long long)mr_to_fixed(gm[u].w, em, shmax));
        } else {
          double* ad = reinterpret_cast<double*>(acc64);
          unsafeAtomicAdd(ad + (size_t)j[u][0] * CW + 4 * qd + 0, (double)gm[u].x);
          unsafeAtomicAdd(ad + (size_t)j[u][1] * CW + 4 * qd + 1, (double)gm[u].y);
          unsafeAtomicAdd(ad + (size_t)j[u][2] * CW + 4 * qd + 2, (double)gm[u].z);
          unsafeAtomicAdd(ad + (size_t)j[u][3] * CW + 4 * qd + 3, (double)gm[u].w);
        }
      }
    }
  };
  // ---- the sweep: U rows per thread in flight
  process_rows(tl);
  for (int n0 = tl + TL * U; n0 < N; n0 += TL * U) {
    load_rows(n0);
    process_rows(n0);
  }
  if (ACC == 0) {
    if (over) ctl[1] = 1;
    __syncthreads();
    if (ctl[1]) {                                   // beyond the scale somewhere (inf / NaN included): the exact two-sweep form on a clean image
      __syncthreads();
      for (int i = tid; i < M * CW; i += NT) acc64[i] = 0;
      if (tid == 0) ctl[0] = 0;
      __syncthreads();
      mr_i64_two_sweep_body<NT, SELF, MODE, AK, STATS>(acc64, ctl, gin, nn_idx, argmax, gx, gsrc, b, G, c, N, M, k, CW, ch0, T, shmax, false,
                                                       &stat);
      if constexpr (STATS) stat.template flush<NT>(acc64, bn.sums, C, ch0, CW);
      return;
    }
  } else {
    __syncthreads();
  }
  // ---- store: one conversion per element (+ the token's own seed for the self graph)
  if (tl < TL) {
    float* db = (SELF ? gx : gsrc) + (size_t)b * M * C + ch0;
    for (int m = tl; m < M; m += TL) {
      const long long* a = acc64 + (size_t)m * CW + 4 * qd;
      float4 o, yv;
      if constexpr (STATS && SELF) yv = stat.ld(((size_t)b * M + m) * C + ch);
      if (ACC == 0) {
        o = make_float4(mr_from_fixed(a[0], em, shmax), mr_from_fixed(a[1], em, shmax), mr_from_fixed(a[2], em, shmax),
                        mr_from_fixed(a[3], em, shmax));
      } else {
        const double* ad = reinterpret_cast<const double*>(a);
        o = make_float4((float)ad[0], (float)ad[1], (float)ad[2], (float)ad[3]);
      }
      if (SELF) {
        float4 direct1, gm1;
        load_grad<MODE>(gin, T, (size_t)b * N + m, C, ch, MODE, direct1, gm1);
        o = make_float4(o.x + (direct1.x - gm1.x), o.y + (direct1.y - gm1.y), o.z + (direct1.z - gm1.z), o.w + (direct1.w - gm1.w));
      }
      if constexpr (STATS && SELF) stat.acc(o, yv);
      *reinterpret_cast<float4*>(db + (size_t)m * C + 4 * qd) = o;
    }
  }
  if constexpr (STATS) stat.template flush<NT>(acc64, bn.sums, C, ch0, CW);
}

// Deterministic scatter (GKG_MR_DETERMINISTIC): the LDS-atomic kernel above adds the fan-in of a key in whatever order
// its lanes arrive, so gsrc differs in the last bit from run to run (like the reference's CUDA index_put_(accumulate)).
// Here a workgroup owns ONE channel quad of one image; each of its TL threads sweeps its own residue class of queries
// (n = tl, tl + TL, ...) in ascending order into a PRIVATE copy of the destination rows ([TL][M] float4 in LDS, plain
// read-modify-write, no atomics); the copies are then added in thread order.  Every sum has a fixed order -> results
// are bit-identical from run to run.
template <bool SELF, int MODE, int AK>
__global__ __launch_bounds__(64) void mr_bwd_tm_det_kernel(const float* __restrict__ gin, const int64_t* __restrict__ nn_idx,
                                                           const uint8_t* __restrict__ argmax, float* __restrict__ gx,
                                                           float* __restrict__ gsrc, int B, int G, int c, int N, int M,
                                                           int k, int mode, int TL, int ak) {
  extern __shared__ float acc[];                  // [TL][M][4]
  const int C = G * c;
  const int b = blockIdx.y;
  const int ch = 4 * blockIdx.x;
  const int tl = threadIdx.x;
  const size_t T = (size_t)B * N;
  const int g = ch / c;
  for (int i = tl; i < TL * M; i += 64) *reinterpret_cast<float4*>(acc + 4 * (size_t)i) = make_float4(0.f, 0.f, 0.f, 0.f);
  __syncthreads();
  if (tl < TL) {
    float* mine = acc + (size_t)tl * M * 4;
    for (int n = tl; n < N; n += TL) {
      const size_t t = (size_t)b * N + n;
      const int64_t* ip = nn_idx + (((size_t)b * G + g) * N + n) * k;
      int j[4];
      mr_targets<AK>(argmax, ak, t * C + ch, ip, k, M, j);
      float4 direct, gm;
      load_grad<MODE>(gin, T, t, C, ch, mode, direct, gm);
      if (!SELF)
        *reinterpret_cast<float4*>(gx + t * C + ch) = make_float4(direct.x - gm.x, direct.y - gm.y, direct.z - gm.z, direct.w - gm.w);
      mine[4 * j[0] + 0] += gm.x;
      mine[4 * j[1] + 1] += gm.y;
      mine[4 * j[2] + 2] += gm.z;
      mine[4 * j[3] + 3] += gm.w;
    }
  }
  __syncthreads();
  float* db = (SELF ? gx : gsrc) + (size_t)b * M * C + ch;
  for (int m = tl; m < M; m += 64) {
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (SELF) {                                    // centre term of the self graph: direct - gm of the token itself
      float4 direct, gm;
      load_grad<MODE>(gin, T, (size_t)b * N + m, C, ch, mode, direct, gm);
      s = make_float4(direct.x - gm.x, direct.y - gm.y, direct.z - gm.z, direct.w - gm.w);
    }
    for (int t2 = 0; t2 < TL; ++t2) {
      const float4 v = *reinterpret_cast<const float4*>(acc + ((size_t)t2 * M + m) * 4);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    *reinterpret_cast<float4*>(db + (size_t)m * C) = s;
  }
}

// Deterministic fallback for destination images too large for LDS (label graphs over > 9 600 keys: few queries): one
// thread per (image, channel quad) walks its queries in order and read-modify-writes the pre-seeded global rows.
template <int MODE, int AK>
__device__ __forceinline__ void det_global_walk(const float* __restrict__ gin, const int64_t* __restrict__ nn_idx,
                                                const uint8_t* __restrict__ argmax, float* __restrict__ db, int b, int g, int ch,
                                                int C, int G, int N, int M, int k, size_t T) {
  for (int n = 0; n < N; ++n) {
    const size_t t = (size_t)b * N + n;
    const int64_t* ip = nn_idx + (((size_t)b * G + g) * N + n) * k;
    int j[4];
    mr_targets<AK>(argmax, AK, t * C + ch, ip, k, M, j);
    float4 direct, gm;
    load_grad<MODE>(gin, T, t, C, ch, MODE, direct, gm);
    db[(size_t)j[0] * C + 0] += gm.x;
    db[(size_t)j[1] * C + 1] += gm.y;
    db[(size_t)j[2] * C + 2] += gm.z;
    db[(size_t)j[3] * C + 3] += gm.w;
  }
}

__global__ __launch_bounds__(64) void mr_bwd_tm_det_global_kernel(const float* __restrict__ gin, const int64_t* __restrict__ nn_idx,
                                                                  const uint8_t* __restrict__ argmax, float* __restrict__ dst,
                                                                  int B, int G, int c, int N, int M, int k, int mode, int ak) {
  const int C = G * c, C4 = C >> 2;
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= B * C4) return;
  const int b = i / C4, ch = 4 * (i - b * C4);
  const size_t T = (size_t)B * N;
  const int g = ch / c;
  float* db = dst + (size_t)b * M * C + ch;
  // the (mode, arg kind) branches are hoisted out of the walk: inside it they sent the float4s through scratch memory
  if (mode == 0) {
    if (ak) det_global_walk<0, 1>(gin, nn_idx, argmax, db, b, g, ch, C, G, N, M, k, T);
    else det_global_walk<0, 0>(gin, nn_idx, argmax, db, b, g, ch, C, G, N, M, k, T);
  } else {
    if (ak) det_global_walk<1, 1>(gin, nn_idx, argmax, db, b, g, ch, C, G, N, M, k, T);
    else det_global_walk<1, 0>(gin, nn_idx, argmax, db, b, g, ch, C, G, N, M, k, T);
  }
}

// Fallback when a destination image does not fit in LDS even for a 4-channel chunk: fp32 global atomics.
__global__ __launch_bounds__(256) void mr_bwd_tm_scatter_atomic_kernel(const float* __restrict__ gin, const int64_t* __restrict__ nn_idx,
                                                                       const uint8_t* __restrict__ argmax, float* __restrict__ dst,
                                                                       int B, int G, int c, int N, int M, int k, int mode, int ak) {
  const int C = G * c, C4 = C >> 2;
  const size_t T = (size_t)B * N;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= T * C4) return;
  const size_t t = i / C4;
  const int ch = 4 * (int)(i - t * C4);
  const int b = (int)(t / N), n = (int)(t - (size_t)b * N);
  const int g = ch / c;
  const int64_t* ip = nn_idx + (((size_t)b * G + g) * N + n) * k;
  int j[4];
  mr_targets(argmax, ak, t * C + ch, ip, k, M, j);
  float4 gm;
  if (mode == 0) {
    gm = *reinterpret_cast<const float4*>(gin + t * C + ch);
  } else {
    const int Cq = C >> 2;
    gm = *reinterpret_cast<const float4*>(gin + t * (size_t)(2 * C) + xm_col(ch, Cq) + Cq);
  }
  float* db = dst + (size_t)b * M * C + ch;
  atomicAdd(db + (size_t)j[0] * C + 0, gm.x);
  atomicAdd(db + (size_t)j[1] * C + 1, gm.y);
  atomicAdd(db + (size_t)j[2] * C + 2, gm.z);
  atomicAdd(db + (size_t)j[3] * C + 3, gm.w);
}

}  // namespace gkg

using namespace gkg;

// ------------------------------------------------------------------------------------------ entry points
// Each one fills a call, asks gkg_mr_plan.h for the plan, opens the profiler scope and launches what the plan names.

// Three runtime switches -> compile-time constants: f(std::bool_constant<a>, std::bool_constant<b>, std::bool_constant<c>).  The
// token-major kernels are instantiated per (self graph, mode, arg kind) — the forward per (k == 9, arg kind, bf16 out) — and picked here.
template <typename F>
static void mr_dispatch3(bool a, bool b, bool c, F&& f) {
  auto on_c = [&](auto A, auto B) { if (c) f(A, B, std::true_type{}); else f(A, B, std::false_type{}); };
  auto on_b = [&](auto A) { if (b) on_c(A, std::true_type{}); else on_c(A, std::false_type{}); };
  if (a) on_b(std::true_type{}); else on_b(std::false_type{});
}

// f(T{}) for the element type of a channel-major call (the plan has rejected every other dtype)
template <typename F>
static void mr_dispatch_dtype(int dtype, F&& f) {
  if (dtype == GKG_F32) f(float{}); else if (dtype == GKG_F16) f(_Float16{}); else f(uint16_t{});
}

// a launch with more than 64 KB of dynamic LDS has to be allowed per kernel
template <typename K>
static void mr_allow_lds(K* kernel, size_t lds) {
  if (lds > 64 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

static int mr_done(const char* where) { const hipError_t e = hipGetLastError(); return e == hipSuccess ? 0 : gkg_fail_hip(e, where); }

extern "C" int gkg_mr_fwd(const void* x, const void* src, const int64_t* nn_idx, void* m_out, uint8_t* argmax,
                          int BG, int c, int N, int M, int k, int dtype, void* stream) {
  if (!x || !nn_idx || !m_out) return gkg_fail(GKG_ERR_NULL, "gkg_mr_fwd: x, nn_idx and m_out must be non-null");
  MrCmPlan p;
  const char* msg = nullptr;
  if (const int rc = mr_cm_plan(MrCmCall{false, BG, c, N, M, k, dtype, src == nullptr}, &p, &msg)) return gkg_fail(rc, msg);
  if (!src) src = x;
  hipStream_t st = (hipStream_t)stream;
  GkgProfScope prof(GKG_PROF_MR_FWD, st);
  const dim3 grid(p.grid_x, p.grid_y, p.grid_z);
  if (p.fallback) mr_dispatch_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((mr_fwd_gather_kernel<T>), grid, dim3(256), 0, st, (const T*)x, (const T*)src, nn_idx, (T*)m_out, argmax, c, N, M, k);
  });
  else mr_dispatch_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    mr_allow_lds(&mr_fwd_kernel<T>, p.lds);
    hipLaunchKernelGGL((mr_fwd_kernel<T>), grid, dim3(256), p.lds, st, (const T*)x, (const T*)src, nn_idx, (T*)m_out, argmax, c, N, M, k, p.CH);
  });
  return mr_done(p.fallback ? "mr_fwd_gather_kernel" : "mr_fwd_kernel");
}

extern "C" int gkg_mr_bwd(const void* g, const int64_t* nn_idx, const uint8_t* argmax, void* gx, void* gsrc,
                          int BG, int c, int N, int M, int k, int dtype, void* stream) {
  if (!g || !nn_idx || !argmax || !gx) return gkg_fail(GKG_ERR_NULL, "gkg_mr_bwd: g, nn_idx, argmax and gx must be non-null");
  MrCmPlan p;
  const char* msg = nullptr;
  if (const int rc = mr_cm_plan(MrCmCall{true, BG, c, N, M, k, dtype, gsrc == nullptr}, &p, &msg)) return gkg_fail(rc, msg);
  hipStream_t st = (hipStream_t)stream;
  GkgProfScope prof(GKG_PROF_MR_BWD, st);
  const dim3 grid(p.grid_x, p.grid_y, p.grid_z);
  if (p.fallback) {                  // fp32 global atomics into gsrc = 0 / gx = -g
    if (p.gsrc_bytes) (void)hipMemsetAsync(gsrc, 0, p.gsrc_bytes, st);
    if (p.seed_grid) hipLaunchKernelGGL(negate_kernel, dim3(p.seed_grid), dim3(256), 0, st, (const float*)g, (float*)gx, (size_t)BG * c * N);
    hipLaunchKernelGGL(mr_bwd_atomic_kernel, grid, dim3(256), 0, st, (const float*)g, nn_idx, argmax, (float*)gx,
                       gsrc ? (float*)gsrc : (float*)gx, c, N, M, k, gsrc ? 0 : 1);
    return mr_done("mr_bwd_atomic_kernel");
  }
  mr_dispatch_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    auto go = [&](auto* kernel) {
      mr_allow_lds(kernel, p.lds);
      hipLaunchKernelGGL(kernel, grid, dim3(256), p.lds, st, (const T*)g, nn_idx, argmax, (T*)gx, (T*)gsrc, c, N, M, k, p.CH);
    };
    if (gsrc) go(&mr_bwd_kernel<T, false>); else go(&mr_bwd_kernel<T, true>);
  });
  return mr_done("mr_bwd_kernel");
}

// ------------------------------------------------------------------------------------------ token-major entry points
template <typename IdxT>
static int mr_fwd_tm_impl(const float* x, int ldx, int xchunk, const float* src, const IdxT* nn_idx, void* out, uint8_t* argmax,
                          int B, int G, int c, int N, int M, int k, int mode, int out_dtype, int arg_kind, void* stream) {
  const MrFwdTmCall q{B, G, c, N, M, k, mode, out_dtype, arg_kind, ldx, xchunk, src != nullptr, (const void*)x == (const void*)out,
                      argmax != nullptr, sizeof(IdxT) == 2};
  MrFwdTmPlan p;
  const char* msg = nullptr;
  if (const int rc = mr_fwd_tm_plan(q, &p, &msg)) return gkg_fail(rc, msg);
  if (!x || !nn_idx || !out) return gkg_fail(GKG_ERR_NULL, "gkg_mr_fwd_tm: x, nn_idx and out must be non-null");
  if (!src) src = x;
  hipStream_t st = (hipStream_t)stream;
  GkgProfScope prof(GKG_PROF_MR_FWD, st, p.work);
  mr_dispatch3(p.out_bf16, p.KS == 9, p.AK == 1, [&](auto BF, auto K9, auto A) {
    using OutT = std::conditional_t<BF.value, uint16_t, float>;
    hipLaunchKernelGGL((mr_fwd_tm_kernel<K9.value ? 9 : 0, 1, OutT, A.value ? 1 : 0, IdxT>), dim3(p.grid), dim3(256), 0, st, x, src, nn_idx,
                       (OutT*)out, argmax, B, G, c, N, M, k, mode, p.ldx, xchunk, p.lds_, p.schunk, p.write_x);
  });
  return mr_done("mr_fwd_tm_kernel");
}

extern "C" int gkg_mr_fwd_tm(const float* x, int ldx, int xchunk, const float* src, const int64_t* nn_idx, void* out, uint8_t* argmax,
                             int B, int G, int c, int N, int M, int k, int mode, int out_dtype, int arg_kind, void* stream) {
  return mr_fwd_tm_impl<int64_t>(x, ldx, xchunk, src, nn_idx, out, argmax, B, G, c, N, M, k, mode, out_dtype, arg_kind, stream);
}

// gkg_mr_fwd_tm over the compact neighbour lists of gkg_knn_fwd_tm16 (u16 rows, M <= 65 536): same outputs, same bits; the
// index stream is a quarter of the int64 one (SURVEY §8d "MR gather-max fwd": 8 B G N k -> 2 B G N k bytes).
extern "C" int gkg_mr_fwd_tm16(const float* x, int ldx, int xchunk, const float* src, const uint16_t* nn16, void* out, uint8_t* argmax,
                               int B, int G, int c, int N, int M, int k, int mode, int out_dtype, int arg_kind, void* stream) {
  return mr_fwd_tm_impl<uint16_t>(x, ldx, xchunk, src, nn16, out, argmax, B, G, c, N, M, k, mode, out_dtype, arg_kind, stream);
}

struct MrBwdTmPtrs { const float* gin; const int64_t* nn_idx; const uint8_t* argmax; float* gx; float* gsrc; MrBnArgs bn; };

// The LDS-image backward kernels are instantiated per (self graph, mode, arg kind): f(bool_constant<SELF>, integral_constant<int, MODE>,
// integral_constant<int, AK>) for the call's three
template <typename F>
static void mr_bwd_tm_dispatch(const MrBwdTmCall& q, F&& f) {
  mr_dispatch3(q.self_graph, q.mode == 0, q.arg_kind == 1, [&](auto S, auto M0, auto A) {
    f(S, std::integral_constant<int, M0.value ? 0 : 1>{}, std::integral_constant<int, A.value ? 1 : 0>{});
  });
}
// go(kernel) for the streaming / two-sweep instantiation of the call; with the BN backward statistics of gx (MrStat): the XM gradient
// layout (mode 1) only
template <int NT, int ACC, int U, bool STATS, typename Go>
static void mr_bwd_tm_stream(const MrBwdTmCall& q, Go&& go) {
  mr_bwd_tm_dispatch(q, [&](auto S, auto MO, auto A) {
    if constexpr (!STATS || MO.value == 1) go(&mr_bwd_tm_stream_kernel<NT, S.value, MO.value, A.value, ACC, U, STATS>);
  });
}
template <bool STATS, typename Go>
static void mr_bwd_tm_i64(const MrBwdTmCall& q, Go&& go) {
  mr_bwd_tm_dispatch(q, [&](auto S, auto MO, auto A) {
    if constexpr (!STATS || MO.value == 1) go(&mr_bwd_tm_scatter_i64_kernel<S.value, MO.value, A.value, STATS>);
  });
}

// The launches of a planned backward.  hipErrorInvalidValue: the plan names a form no kernel of this unit holds.
static hipError_t mr_bwd_tm_launch(const MrBwdTmCall& q, const MrBwdTmPlan& p, const MrBwdTmPtrs& a, hipStream_t st) {
  const dim3 grid(p.grid_x, p.grid_y), block(p.block);
  if (p.seed_grid) {                 // seed (gx = direct - gm; gsrc = 0), then the ordered walk / the fp32 global atomics
    if (p.form != MR_DET_WALK && p.form != MR_GLOBAL_F32) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mr_bwd_tm_init_kernel, dim3(p.seed_grid), dim3(256), 0, st, a.gin, a.gx, q.G * q.c, (size_t)q.B * q.N, q.mode);
    if (p.gsrc_bytes) (void)hipMemsetAsync(a.gsrc, 0, p.gsrc_bytes, st);
    hipLaunchKernelGGL(p.form == MR_DET_WALK ? mr_bwd_tm_det_global_kernel : mr_bwd_tm_scatter_atomic_kernel, grid, block, 0, st, a.gin,
                       a.nn_idx, a.argmax, a.gsrc ? a.gsrc : a.gx, q.B, q.G, q.c, q.N, q.M, q.k, q.mode, q.arg_kind);
    return hipSuccess;
  }
  hipError_t e = hipErrorInvalidValue;
  auto go = [&](auto* kernel, auto... tail) {                // every kernel of the family starts with the same eleven arguments
    mr_allow_lds(kernel, p.lds);
    hipLaunchKernelGGL(kernel, grid, block, p.lds, st, a.gin, a.nn_idx, a.argmax, a.gx, a.gsrc, q.B, q.G, q.c, q.N, q.M, q.k, tail...);
    e = hipSuccess;
  };
  auto i64 = [&](auto* kernel) { go(kernel, p.cw, p.shmax, a.bn); };
  auto stream = [&](auto* kernel) { go(kernel, p.cw, p.shmax & 0xffff, p.shmax >> 16, a.bn); };
  auto is_stream = [&](int nt, int acc, int u, bool stats) {
    return p.form == (acc ? MR_STREAM_F64 : MR_STREAM) && p.NT == nt && p.ACC == acc && p.U == u && p.STATS == stats;
  };
  if (p.form == MR_TWO_SWEEP && !p.STATS) mr_bwd_tm_i64<false>(q, i64);
  else if (is_stream(512, 0, 4, true)) mr_bwd_tm_stream<512, 0, 4, true>(q, stream);
  else if (is_stream(512, 1, 4, false)) mr_bwd_tm_stream<512, 1, 4, false>(q, stream);
  else if (is_stream(256, 0, 8, false)) mr_bwd_tm_stream<256, 0, 8, false>(q, stream);
  else if (is_stream(256, 0, 4, false)) mr_bwd_tm_stream<256, 0, 4, false>(q, stream);
  else if (is_stream(512, 0, 8, false)) mr_bwd_tm_stream<512, 0, 8, false>(q, stream);
  else if (is_stream(512, 0, 4, false)) mr_bwd_tm_stream<512, 0, 4, false>(q, stream);
  else if (p.form == MR_TWO_SWEEP) mr_bwd_tm_i64<true>(q, i64);
  else if (p.form == MR_DET_PRIVATE || p.form == MR_LDS_F32)
    mr_bwd_tm_dispatch(q, [&](auto S, auto MO, auto A) {
      if (p.form == MR_DET_PRIVATE) go(&mr_bwd_tm_det_kernel<S.value, MO.value, A.value>, MO.value, p.cw, A.value);
      else go(&mr_bwd_tm_scatter_kernel<S.value, MO.value, A.value>, MO.value, p.cw, A.value);
    });
  return e;
}

static int mr_bwd_tm_run(const MrBwdTmPtrs& a, int B, int G, int c, int N, int M, int k, int mode, int arg_kind, unsigned flags,
                         bool want_stats, void* stream) {
  const MrBwdTmCall q{B, G, c, N, M, k, mode, arg_kind, flags, a.gsrc == nullptr, want_stats};
  MrBwdTmPlan p;
  const char* msg = nullptr;
  if (const int rc = mr_bwd_tm_plan(q, &p, &msg)) return gkg_fail(rc, msg);
  // arg_kind 1: the saved winning ROWS are the scatter targets — the index tensor is not read and may be null (the fused
  // k-NN + aggregation forward, gkg_knn_mr_fwd_tm, never materialises one)
  if (!a.gin || (!a.nn_idx && arg_kind != 1) || !a.argmax || !a.gx) return gkg_fail(GKG_ERR_NULL, "gkg_mr_bwd_tm: gin, argmax, gx (and nn_idx unless arg_kind == 1) must be non-null");
  hipStream_t st = (hipStream_t)stream;
  GkgProfScope prof(GKG_PROF_MR_BWD, st, p.work);
  static const char* const where[] = {"mr_bwd_tm_stream_kernel", "mr_bwd_tm_stream_kernel", "mr_bwd_tm_scatter_i64_kernel", "mr_bwd_tm (deterministic)",
                                      "mr_bwd_tm (deterministic)", "mr_bwd_tm", "mr_bwd_tm"};       // by MrBwdForm
  const hipError_t e = mr_bwd_tm_launch(q, p, a, st);
  return e != hipSuccess ? gkg_fail_hip(e, where[p.form]) : mr_done(where[p.form]);
}

extern "C" int gkg_mr_bwd_tm(const float* gin, const int64_t* nn_idx, const uint8_t* argmax, float* gx, float* gsrc,
                             int B, int G, int c, int N, int M, int k, int mode, int arg_kind, unsigned flags, void* stream) {
  return mr_bwd_tm_run(MrBwdTmPtrs{gin, nn_idx, argmax, gx, gsrc, MrBnArgs{}}, B, G, c, N, M, k, mode, arg_kind, flags, false, stream);
}

// gkg_mr_bwd_tm that is ALSO the statistics pass of the BN backward whose upstream gradient gx is (the layer x = BN(y) in front
// of the aggregation: nb == 1, act == 0): y (B*N, C), mean / invstd [C], `sums` [2][C] fp64, ZERO on entry, receives sum gx and
// sum gx * yhat with atomics — what gkg_bn_bwd_atomic's first launch would leave there; follow it with
// gkg_bn_bwd_apply_from_sums.  gx / gsrc have the bits of gkg_mr_bwd_tm.  GKG_ERR_UNSUPPORTED (nothing launched, nothing
// written) when the shape or the flags select a scatter form that carries no statistics: run the plain call and
// gkg_bn_bwd_atomic then.
extern "C" int gkg_mr_bwd_tm_bnstats(const float* gin, const int64_t* nn_idx, const uint8_t* argmax, float* gx, float* gsrc,
                                     int B, int G, int c, int N, int M, int k, int mode, int arg_kind, unsigned flags,
                                     const float* y, const float* mean, const float* invstd, double* sums, void* stream) {
  if (!y || !mean || !invstd || !sums) return gkg_fail(GKG_ERR_NULL, "gkg_mr_bwd_tm_bnstats: null pointer");
  return mr_bwd_tm_run(MrBwdTmPtrs{gin, nn_idx, argmax, gx, gsrc, MrBnArgs{y, mean, invstd, sums}}, B, G, c, N, M, k, mode, arg_kind, flags,
                       true, stream);
}

// 1 when gkg_mr_bwd_tm_bnstats would run for these sizes and flags (0: GKG_ERR_UNSUPPORTED or bad sizes): the plan's answer, for
// callers that must book their scratch buffer before the call.
extern "C" int gkg_mr_bwd_tm_bnstats_supported(int B, int G, int c, int N, int M, int k, int mode, int arg_kind, int self_graph,
                                               unsigned flags) {
  MrBwdTmPlan p;
  const char* msg = nullptr;
  return mr_bwd_tm_plan(MrBwdTmCall{B, G, c, N, M, k, mode, arg_kind, flags, self_graph != 0, true}, &p, &msg) == 0;
}
