// gkg_knn.hip — fused dilated k-NN graph construction for MI355X (gfx950 / CDNA4).
//
// Replaces the reference's  F.normalize -> (|x|^2 - 2 x.y^T + |y|^2) -> += relative_pos -> topk -> [::d]
// chain (mmcls/models/backbones/vig_model/torch_edge.py:9-51, 54-106, 139-176) without ever
// materialising the (BG,N,M) distance matrix.
//
// Pipeline (all on the caller's stream):
//   1. token_prep_kernel   : (one launch for queries and keys) per token, ordered-fma L2 norm over the group's channels, normalised fp32
//                            copy th (BG,cpad,T) (cpad = c rounded up to a multiple of 8, zero padded) + |th|^2.
//   2. knn_tile_kernel<KD> : one workgroup = 64 queries of one (b,g) problem x one key split; its 4 waves
//                            take key tiles of 32 round-robin.  Per key tile a wave runs the contraction on
//                            the fp32 matrix cores (v_mfma_f32_32x32x2_f32: exact fp32, == an ordered fmaf
//                            chain over channels) with keys as the A operand (streamed from L2/HBM in the
//                            reference's native channel-major layout: a lane reads y[ch][m0+lane]) and the
//                            64 staged queries as two B operands from LDS.  The two 32x32 accumulators are
//                            exchanged with v_permlane32_swap so that lane l owns query n0+l and all 32
//                            key distances of the tile; each lane keeps a sorted top-KD list of fp64
//                            (distance, index) keys in registers (v_min_f64 + v_max_f64 per slot).  The 4 per-wave lists of a
//                            query are merged through LDS; ranks 0,d,2d,.. go out as int64.
//   3. knn_merge_kernel    : only when the keys were split over several workgroups (few queries, many
//                            keys — the label graph): merges the S partial lists of each query.
//
// Arithmetic contract: include/gkg_hip.h (restated in oracle/gkg_oracle.c).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "gkg_knn_common.h"
#include "gkg_knn_prep.h"
#include "gkg_knn_tile.h"

namespace gkg {

// ------------------------------------------------------------------------------------------ prep (bodies: gkg_knn_prep.h)
// HF: the octet-major planes (PrepSet::tb) hold fp16 (GKG_KNN_F16_CONTRACT) instead of bf16
template <typename T, bool NORM, int PT, bool HF = false>
__global__ __launch_bounds__(PT) void token_prep_kernel(PrepSet s1, PrepSet s2, int nbx1, int c, int cpad) {
  token_prep_body<T, NORM, PT, false, HF>(s1, s2, nbx1, c, cpad, BnDerive{}, nullptr, nullptr);
}
// The same pass as a projection's BN-apply (PrepSet::raw): what a trace shows for the Grapher's fc1 / the label block's fc1 / the
// Grapher's fc2 in front of a label block — one launch = BN-apply (+ residual, + both layouts) + the k-NN's token preparation
template <bool NORM, int PT>
__global__ __launch_bounds__(PT) void bn_apply_knn_prep_kernel(PrepSet s1, int c, int cpad, BnDerive d, const float* __restrict__ aff_a,
                                                               const float* __restrict__ aff_c) {
  token_prep_body<float, NORM, PT, true>(s1, s1, 0x7fffffff, c, cpad, d, aff_a, aff_c);
}

template <bool NORM, int TK>
__global__ __launch_bounds__(256) void token_prep_coop_kernel(PrepSet s1, PrepSet s2, int nbx1, int c, int cpad) {
  extern __shared__ float col[];          // [c][TK + 1]
  const bool second = (int)blockIdx.x >= nbx1;
  const PrepSet& S = second ? s2 : s1;
  const int n0 = ((int)blockIdx.x - (second ? nbx1 : 0)) * TK;
  token_prep_coop_body<NORM, TK, false>(S, col, blockIdx.y, n0, min(TK, S.Tn - n0), c, cpad, BnDerive{}, nullptr, nullptr);
}
template <bool NORM, int TK>
__global__ __launch_bounds__(256) void bn_apply_knn_prep_coop_kernel(PrepSet s1, int c, int cpad, BnDerive d, const float* __restrict__ aff_a,
                                                                     const float* __restrict__ aff_c) {
  extern __shared__ float col[];          // [c][TK + 1] + [2][c] scale / shift
  const int n0 = (int)blockIdx.x * TK;
  token_prep_coop_body<NORM, TK, true>(s1, col, blockIdx.y, n0, min(TK, s1.Tn - n0), c, cpad, d, aff_a, aff_c);
}

// ------------------------------------------------------------------------------------------ split merge
// One thread per partial-list ELEMENT: its final rank = its position in its own (sorted) list + the number of
// lexicographically smaller (dist, idx) pairs in every other split's list (binary search).  Ranks are unique,
// so ranks 0,d,2d,.. < kd are written straight to their output slot — no serial merge.
__global__ __launch_bounds__(256) void knn_merge_kernel(const float* __restrict__ part_v, const int* __restrict__ part_i,
                                                        int64_t* __restrict__ nn_idx, int64_t* __restrict__ center,
                                                        uint16_t* __restrict__ nn16,
                                                        int S, int BG, int N, int M, int k, int dilation, int kd) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;        // (s, q, p) flattened as s*nq*kd + q*kd + p
  const size_t nq = (size_t)BG * N;
  const size_t stride = nq * kd;                                   // between splits
  if (e >= stride * S) return;
  const int s = (int)(e / stride);
  const size_t rem = e - (size_t)s * stride;
  const size_t q = rem / kd;
  const int p = (int)(rem - q * kd);
  const float v = part_v[e];
  const int id = part_i[e];
  // the centre plane does not depend on the distances: split 0's threads write it for every output slot, so ranks that
  // no finite candidate claims (non-finite inputs only) still carry a defined centre index
  if (center && s == 0 && p < k) center[q * k + p] = (int64_t)(q % N);
  if (id == 0x7fffffff) return;                                    // padding of a short list
  int rank = p;
  for (int s2 = 0; s2 < S && rank < kd; ++s2) {
    if (s2 == s) continue;
    const float* ov = part_v + (size_t)s2 * stride + q * kd;
    const int* oi = part_i + (size_t)s2 * stride + q * kd;
    int lo = 0, hi = kd;                                           // first entry >= (v, id)
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      const float mv = ov[mid]; const int mi = oi[mid];
      const bool less = (mv < v) || (mv == v && mi < id);
      if (less) lo = mid + 1; else hi = mid;
    }
    rank += lo;
  }
  if (rank < kd && rank % dilation == 0) {
    const int outj = rank / dilation;
    if (outj < k) {
      const int bc = id < M ? id : 0;               // masked tail keys can only rank here on non-finite inputs
      if (nn16) nn16[q * k + outj] = (uint16_t)bc;
      else nn_idx[q * k + outj] = bc;
    }
  }
}

}  // namespace gkg

// ================================================================================================ host side
using namespace gkg;

// The request of a token-major entry point (B images x G groups) as a value
static KnnCall knn_call_tm(KnnRole role, int B, int G, int c, int N, int M, int k, int dilation, int dtype, unsigned flags, bool has_y,
                           bool has_relpos, int ldx, int xchunk, bool consumer_fused = false) {
  KnnCall q{};
  q.BG = B * G; q.G_tm = G; q.c = c; q.N = N; q.M = M; q.k = k; q.dilation = dilation; q.dtype = dtype; q.flags = flags;
  q.has_y = has_y; q.has_relpos = has_relpos; q.ldx = ldx; q.xchunk = xchunk; q.role = role; q.consumer_fused = consumer_fused;
  return q;
}

extern "C" size_t gkg_knn_workspace_bytes(int BG, int c, int N, int M, int k, int dilation, int dtype, unsigned flags) {
  (void)dtype; (void)flags;
  // y presence is unknown here: budget for it (upper bound) unless the shapes make it impossible
  KnnCall q = knn_call_tm(KNN_GRAPH, BG, 1, c, N, M, k, dilation, GKG_F32, 0, true, false, 0, 0);
  q.G_tm = 0;
  KnnPlan p;
  const char* msg;
  return knn_plan(q, &p, &msg) == 0 ? p.total : 0;
}

// BN-apply producer of the queries (PrepSet::raw): coefficients derived from column sums (d.sums) or given (a, c)
struct PrepAffine { BnDerive d; const float* a; const float* c; };

template <typename T, int PT>
static void launch_prep_pt(const PrepSet& s1, const PrepSet* s2, int BG, int c, int cpad, bool norm, hipStream_t st, const PrepAffine& pa,
                           bool hf) {
  const int nbx1 = ((s1.tb_lo ? s1.rows : s1.Tn) + PT - 1) / PT;
  const int nbx2 = s2 ? ((s2->tb_lo ? s2->rows : s2->Tn) + PT - 1) / PT : 0;
  dim3 grid(nbx1 + nbx2, BG);
  const size_t lds = (size_t)c * PT * sizeof(float) + (s1.raw ? (size_t)2 * c * sizeof(float) : 0);
  const PrepSet second = s2 ? *s2 : s1;
  if (s1.raw) {                                  // BN-apply producer: fp32 tokens, one set
    if constexpr (sizeof(T) == 4) {
      if (norm) hipLaunchKernelGGL((bn_apply_knn_prep_kernel<true, PT>), grid, dim3(PT), lds, st, s1, c, cpad, pa.d, pa.a, pa.c);
      else hipLaunchKernelGGL((bn_apply_knn_prep_kernel<false, PT>), grid, dim3(PT), lds, st, s1, c, cpad, pa.d, pa.a, pa.c);
    }
    return;
  }
  if (hf) {                                      // fp16 planes: normalised tokens only (knn_plan)
    hipLaunchKernelGGL((token_prep_kernel<T, true, PT, true>), grid, dim3(PT), lds, st, s1, second, nbx1, c, cpad);
    return;
  }
  if (norm) hipLaunchKernelGGL((token_prep_kernel<T, true, PT>), grid, dim3(PT), lds, st, s1, second, nbx1, c, cpad);
  else hipLaunchKernelGGL((token_prep_kernel<T, false, PT>), grid, dim3(PT), lds, st, s1, second, nbx1, c, cpad);
}

template <int TK>
static void launch_prep_coop(const PrepSet& s1, const PrepSet* s2, int BG, int c, int cpad, bool norm, hipStream_t st, const PrepAffine& pa) {
  const int nbx1 = (s1.Tn + TK - 1) / TK;
  const int nbx2 = s2 ? (s2->Tn + TK - 1) / TK : 0;
  dim3 grid(nbx1 + nbx2, BG);
  const size_t lds = (size_t)c * (TK + 1) * sizeof(float) + (s1.raw ? (size_t)2 * c * sizeof(float) : 0);
  const PrepSet second = s2 ? *s2 : s1;
  if (s1.raw) {
    if (norm) hipLaunchKernelGGL((bn_apply_knn_prep_coop_kernel<true, TK>), grid, dim3(256), lds, st, s1, c, cpad, pa.d, pa.a, pa.c);
    else hipLaunchKernelGGL((bn_apply_knn_prep_coop_kernel<false, TK>), grid, dim3(256), lds, st, s1, c, cpad, pa.d, pa.a, pa.c);
    return;
  }
  if (norm) hipLaunchKernelGGL((token_prep_coop_kernel<true, TK>), grid, dim3(256), lds, st, s1, second, nbx1, c, cpad);
  else hipLaunchKernelGGL((token_prep_coop_kernel<false, TK>), grid, dim3(256), lds, st, s1, second, nbx1, c, cpad);
}

static bool prep_coop_ok(const PrepSet& s) {       // fp32 token-major rows of whole float4s, fp32 channel-major output
  return !s.tb && s.ps.sc == 1 && ((s.ps.sn | s.ps.sg | s.ps.sb) & 3) == 0 && ((size_t)s.t & 15) == 0;
}

template <typename T>
static hipError_t launch_prep(const PrepSet& s1, const PrepSet* s2, int BG, int c, int cpad, bool norm, hipStream_t st,
                              const PrepAffine& pa = PrepAffine{}, bool hf = false) {     // hf: fp16 planes in PrepSet::tb
  GkgProfScope prof(GKG_PROF_TOKEN_PREP, st);
  if (sizeof(T) == 4 && (c & 3) == 0 && prep_coop_ok(s1) && (!s2 || prep_coop_ok(*s2)) &&
      (size_t)(s1.Tn + (s2 ? s2->Tn : 0)) * BG <= 262144) {                          // latency-bound sizes only
    if (c <= 192) launch_prep_coop<64>(s1, s2, BG, c, cpad, norm, st, pa);               // <= 49 KB tile
    else if (c <= 384) launch_prep_coop<32>(s1, s2, BG, c, cpad, norm, st, pa);
    else launch_prep_coop<16>(s1, s2, BG, c, cpad, norm, st, pa);
    return hipGetLastError();
  }
  if (c <= 192) launch_prep_pt<T, 64>(s1, s2, BG, c, cpad, norm, st, pa, hf);      // <= 48 KB column block
  else if (c <= 384) launch_prep_pt<T, 32>(s1, s2, BG, c, cpad, norm, st, pa, hf);
  else launch_prep_pt<T, 16>(s1, s2, BG, c, cpad, norm, st, pa, hf);                // c <= 600 (plan limit)
  return hipGetLastError();
}

// What a call hands over besides its KnnCall.  Producer roles: `x` is a projection's pre-BN output (B, T, C); the preparation pass
// applies the BN (aff), stores the result to `raw` (keys: + res_tm, also to nchw) and leaves the normalised copies / norms
// (/ prefilter planes) in the workspace exactly where the k-NN call with the same problem + GKG_KNN_X_PREPARED (_Y_PREPARED) expects
// them.  KNN_QUERY_PREP_PLAN: no launch — the producer runs the preparation inside a kernel of its own and gets the queries'
// PrepSet, cpad and the normalisation switch of this plan in *want.
struct KnnPtrs {
  const void* x; const void* y; const float* relpos;
  int64_t* nn_idx; int64_t* center;     // (BG, N, k) int64 lists / centre plane, or null
  uint16_t* nn16;                       // compact u16 lists INSTEAD of (KNN_FUSED: besides) the int64 plane, or null
  void* workspace; size_t workspace_bytes; void* stream;
  float* mr_out; uint16_t* mr_arg;      // KNN_FUSED: XM (B * N, 2 C) and the winning neighbour rows (B, N, C)
  PrepAffine aff; float* raw; int raw_ld, raw_chunk; const float* res_tm; float* nchw;
  KnnQueryPrep* want;
};

// The launch sequence of every role: plan, the two operand sets, the preparation launch the plan asks for, then (k-NN calls) the
// prefilter if planned, the tile kernel, the merge of split keys.  Every decision is the plan's (gkg_knn_plan.h).
static int knn_fwd_impl(const KnnCall& q, const KnnPtrs& t) {
  KnnPlan p;
  const char* msg;
  const int rc = knn_plan(q, &p, &msg);
  if (rc != 0) return msg ? gkg_fail(rc, msg) : rc;
  if (!t.x || !t.workspace || (q.role == KNN_GRAPH && !t.nn_idx && !t.nn16)) return gkg_fail(GKG_ERR_NULL, "gkg_knn_fwd: x, nn_idx and workspace must be non-null");
  if (t.workspace_bytes < p.total) return gkg_fail(GKG_ERR_WORKSPACE, "gkg_knn_fwd: workspace too small (see gkg_knn_workspace_bytes)");
  const int BG = q.BG, c = q.c, N = q.N, M = q.M, G_tm = q.G_tm;
  hipStream_t st = (hipStream_t)t.stream;
  char* ws = (char*)t.workspace;
  float *xh = (float*)(ws + p.off_xh), *yh = (float*)(ws + p.off_yh), *sqx = (float*)(ws + p.off_sqx), *sqy = (float*)(ws + p.off_sqy);
  uint16_t *xpl = (uint16_t*)(ws + p.off_xp), *ypl = (uint16_t*)(ws + p.off_yp);                     // prefilter planes: hi, then lo
  uint16_t *xpl_lo = xpl + (size_t)BG * p.Nr * p.cp16p, *ypl_lo = ypl + (size_t)BG * p.Mr * p.cp16p;
  // input addressing: channel-major (BG,c,T)  or  token-major (B,T,C=G*c) when G_tm > 0
  auto strides = [&](int Tn, int ld, int chunk) {
    PrepStrides ps;
    if (G_tm > 0) { ps.G = G_tm; ps.sb = (size_t)Tn * ld; ps.sg = c; ps.sc = 1; ps.sn = (size_t)ld; ps.chunk = chunk; }
    else { ps.G = 1; ps.sb = (size_t)c * Tn; ps.sg = 0; ps.sc = Tn; ps.sn = 1; ps.chunk = 0; }
    return ps;
  };
  // 16-bit contraction: the normalised copies are octet-major 16-bit planes in the fp32 copies' workspace slots
  const bool bf = p.el != KNN_EL_F32, hf = p.el == KNN_EL_F16;
  const bool pq = q.role == KNN_PRODUCE_QUERIES || q.role == KNN_QUERY_PREP_PLAN, pk = q.role == KNN_PRODUCE_KEYS;
  const PrepSet sx{t.x, xh, sqx, N, strides(N, p.ldx, q.xchunk), p.pf ? xpl : (bf ? (uint16_t*)xh : nullptr), p.pf ? p.cp16p : p.cp16,
                   p.pf ? xpl_lo : nullptr, p.Nr, pq ? t.raw : nullptr, pq ? t.raw_ld : 0, pq ? t.raw_chunk : 0, nullptr, nullptr};
  // (a keys producer reads its pre-BN input through `x`)
  const PrepSet sy{pk ? t.x : t.y, yh, sqy, M, strides(M, G_tm * c, 0), p.pf ? ypl : (bf ? (uint16_t*)yh : nullptr), p.pf ? p.cp16p : p.cp16,
                   p.pf ? ypl_lo : nullptr, p.Mr, pk ? t.raw : nullptr, pk ? t.raw_ld : 0, pk ? t.raw_chunk : 0, pk ? t.res_tm : nullptr,
                   pk ? t.nchw : nullptr};
  if (q.role == KNN_QUERY_PREP_PLAN) { *t.want = KnnQueryPrep{sx, p.cpad, p.norm ? 1 : 0}; return 0; }
  hipError_t e = hipSuccess;
  if (const PrepSet* first = p.prep_x ? &sx : (p.prep_y ? &sy : nullptr)) {      // ONE launch for what this call prepares
    const PrepSet* second = p.prep_x && p.prep_y ? &sy : nullptr;
    if (q.dtype == GKG_F32) e = launch_prep<float>(*first, second, BG, c, p.cpad, p.norm, st, t.aff, hf);
    else if (q.dtype == GKG_F16) e = launch_prep<_Float16>(*first, second, BG, c, p.cpad, p.norm, st, t.aff, hf);
    else e = launch_prep<uint16_t>(*first, second, BG, c, p.cpad, p.norm, st, t.aff, hf);
    if (e != hipSuccess) return gkg_fail_hip(e, "token_prep");
  }
  if (pq || pk) return 0;
  gkg_prof_add_work(GKG_PROF_KNN_TILE, 2.0 * BG * (double)c * N * (double)M);    // algorithmic flop of the distance contraction
  KnnArgs a{};
  a.xh = xh; a.yh = yh; a.sqx = sqx; a.sqy = sqy; a.relpos = t.relpos;
  a.nn_idx = t.nn_idx; a.center = t.center;
  a.part_v = (float*)(ws + p.off_pv); a.part_i = (int*)(ws + p.off_pi);
  a.BG = BG; a.cpad = p.cpad; a.N = N; a.M = M; a.k = q.k; a.dilation = q.dilation; a.kd = p.kd;
  a.splits = p.S; a.tiles_per_split = p.tps; a.nqt = p.nqt; a.rp_major = p.rp_major; a.rp_group = p.rp_group;
  a.xb = (const uint16_t*)xh; a.yb = (const uint16_t*)yh; a.cp16 = p.cp16;
  a.margin = p.margin; a.nn16 = t.nn16; a.mr_G = 1; a.mr_c = c; a.mr_ldx = a.mr_lds = c; a.mr_write_x = 1;
  if (p.pf) {
    a.xb = xpl; a.xb_lo = xpl_lo;
    a.yb = t.y ? ypl : xpl; a.yb_lo = t.y ? ypl_lo : xpl_lo;
    a.cp16 = p.cp16p; a.pf_c = c; a.pf_nrows = p.Nr; a.pf_mrows = t.y ? p.Mr : p.Nr;
    a.wg_flags = (int*)(ws + p.off_flags);
    e = hipMemsetAsync(a.wg_flags, 0, sizeof(int) * (size_t)p.grid_x, st);
    if (e != hipSuccess) return gkg_fail_hip(e, "knn_pf_kernel (flags)");
    e = launch_knn_prefilter(a, p, st);
    if (e != hipSuccess) return gkg_fail_hip(e, "knn_pf_kernel");
    // the fp32 tile kernel below runs as the clean-up pass over the tiles the prefilter flagged
    // (a.wg_flags != null: every other workgroup exits at once)
  }
  if (q.role == KNN_FUSED) {
    a.mr_x = (const float*)t.x; a.mr_src = (const float*)(t.y ? t.y : t.x);
    a.mr_out = t.mr_out; a.mr_arg = t.mr_arg; a.mr_G = G_tm; a.mr_c = c;
    a.mr_ldx = p.ldx; a.mr_xchunk = q.xchunk;
    a.mr_lds = t.y ? G_tm * c : p.ldx; a.mr_schunk = t.y ? 0 : q.xchunk;
    // x already lives in the operand buffer when the caller passes that buffer's x half as the view of x
    a.mr_write_x = !((const void*)t.x == (const void*)t.mr_out && p.ldx == 2 * G_tm * c && q.xchunk == (G_tm * c) / 4);
  }
  e = (hf ? launch_knn_tile_hf : (bf ? launch_knn_tile_bf : (p.mrf ? launch_knn_tile_f32_mr : launch_knn_tile_f32)))(a, p, st);
  if (e != hipSuccess) return gkg_fail_hip(e, "knn_tile_kernel");
  if (p.S > 1) {
    const size_t ne = (size_t)BG * N * p.kd * p.S;
    GkgProfScope prof(GKG_PROF_KNN_MERGE, st);
    // ranks that no finite candidate claims (non-finite inputs only) must still hold a valid index
    if (t.nn16) (void)hipMemsetAsync(t.nn16, 0, sizeof(uint16_t) * (size_t)BG * N * q.k, st);
    else (void)hipMemsetAsync(t.nn_idx, 0, sizeof(int64_t) * (size_t)BG * N * q.k, st);
    hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, st, a.part_v, a.part_i,
                       t.nn_idx, t.center, t.nn16, p.S, BG, N, M, q.k, q.dilation, p.kd);
    e = hipGetLastError();
    if (e != hipSuccess) return gkg_fail_hip(e, "knn_merge_kernel");
  }
  return 0;
}

extern "C" int gkg_knn_fwd(const void* x, const void* y, const float* relpos, int64_t* nn_idx, int64_t* center,
                           int BG, int c, int N, int M, int k, int dilation, int dtype, unsigned flags,
                           void* workspace, size_t workspace_bytes, void* stream) {
  KnnCall q = knn_call_tm(KNN_GRAPH, BG, 1, c, N, M, k, dilation, dtype, flags, y != nullptr, relpos != nullptr, 0, 0);
  q.G_tm = 0;                                    // channel-major (BG, c, T)
  return knn_fwd_impl(q, KnnPtrs{x, y, relpos, nn_idx, center, nullptr, workspace, workspace_bytes, stream});
}

extern "C" int gkg_knn_fwd_tm(const void* x, int ldx, int xchunk, const void* y, const float* relpos, int64_t* nn_idx, int64_t* center,
                              int B, int G, int c, int N, int M, int k, int dilation, int dtype, unsigned flags,
                              void* workspace, size_t workspace_bytes, void* stream) {
  if (B <= 0 || G <= 0) return gkg_fail(GKG_ERR_SHAPE, "gkg_knn_fwd_tm: bad B / G");
  return knn_fwd_impl(knn_call_tm(KNN_GRAPH, B, G, c, N, M, k, dilation, dtype, flags, y != nullptr, relpos != nullptr, ldx, xchunk),
                      KnnPtrs{x, y, relpos, nn_idx, center, nullptr, workspace, workspace_bytes, stream});
}

// The same graph as gkg_knn_fwd_tm with COMPACT neighbour lists: nn16 (B * G, N, k) u16 rows instead of the (2, B G, N, k) int64
// edge_index — for callers that consume the graph on the device and never hand it out (Grapher.forward discards it, reference
// torch_vertex.py:330).  At GKGNet-576's stage 1 the int64 pair is 191 MB written per launch, the compact lists 24 MB (pvig_m
// stage 1, k = 18: 1.36 GB / 170 MB).  Needs M <= 65 536.  Same bits as the int64 lists (tests/test_hip_knn_compact.py).
extern "C" int gkg_knn_fwd_tm16(const void* x, int ldx, int xchunk, const void* y, const float* relpos, uint16_t* nn16, int B, int G, int c, int N, int M,
                                int k, int dilation, int dtype, unsigned flags, void* workspace, size_t workspace_bytes, void* stream) {
  if (B <= 0 || G <= 0) return gkg_fail(GKG_ERR_SHAPE, "gkg_knn_fwd_tm16: bad B / G");
  if (!nn16) return gkg_fail(GKG_ERR_NULL, "gkg_knn_fwd_tm16: nn16 must be non-null");
  if (M > 65536) return gkg_fail(GKG_ERR_UNSUPPORTED, "gkg_knn_fwd_tm16: M <= 65536 (u16 rows)");
  return knn_fwd_impl(knn_call_tm(KNN_GRAPH, B, G, c, N, M, k, dilation, dtype, flags, y != nullptr, relpos != nullptr, ldx, xchunk),
                      KnnPtrs{x, y, relpos, nullptr, nullptr, nn16, workspace, workspace_bytes, stream});
}

// Row g2: k-NN + max-relative aggregation in one kernel (knn_tile_kernel<..., MRF = true>) for token-major fp32 callers.
// x (B, N, C = G c), y (B, M, C) or NULL (self graph), relative_pos (N, M) or NULL -> the graph of gkg_knn_fwd_tm (same
// contract, same bits) is built and consumed on the spot: xm_out (B N, 2 C) = the grouped projection's operand buffer of
// gkg_mr_fwd_tm mode 1 (m into the m chunks; the x chunks are written unless x IS that buffer's x half: x == xm_out,
// ldx == 2 C, xchunk == C / 4), arg_out (B, N, C) u16 = the winning neighbour rows of gkg_mr_fwd_tm arg_kind 1,
// nn16_out (B G, N, k) u16 = the neighbour lists (optional); nn_idx_out / center_out (B G, N, k) int64 = gkg_knn_fwd_tm's outputs
// for callers that return the graph (GrapherLabel), optional — otherwise no int64 index tensor and no centre plane exist.
extern "C" int gkg_knn_mr_fused_supported(int B, int G, int c, int N, int M, int k, int dilation, int has_y, int has_relpos,
                                          unsigned flags) {
  if (B <= 0 || G <= 0 || c <= 0 || ((G * c) & 15)) return 0;
  KnnPlan p;
  const char* msg;
  const int rc = knn_plan(knn_call_tm(KNN_FUSED_PROBE, B, G, c, N, M, k, dilation, GKG_F32, flags, has_y != 0, has_relpos != 0, 0, 0), &p, &msg);
  if (rc != 0 && msg) gkg_fail(rc, msg);
  return rc == 0 ? 1 : 0;
}

extern "C" int gkg_knn_mr_fwd_tm(const float* x, int ldx, int xchunk, const float* y, const float* relpos, float* xm_out,
                                 uint16_t* arg_out, uint16_t* nn16_out, int64_t* nn_idx_out, int64_t* center_out, int B, int G, int c,
                                 int N, int M, int k, int dilation, unsigned flags, void* workspace, size_t workspace_bytes,
                                 void* stream) {
  if (B <= 0 || G <= 0) return gkg_fail(GKG_ERR_SHAPE, "gkg_knn_mr_fwd_tm: bad B / G");
  if (!xm_out || !arg_out) return gkg_fail(GKG_ERR_NULL, "gkg_knn_mr_fwd_tm: null output");
  if ((G * c) & 15) return gkg_fail(GKG_ERR_SHAPE, "gkg_knn_mr_fwd_tm: C = G * c must be a multiple of 16");
  if (((size_t)x & 15) || ((size_t)y & 15) || ((size_t)xm_out & 15) || ((size_t)arg_out & 7) || (ldx & 3))
    return gkg_fail(GKG_ERR_SHAPE, "gkg_knn_mr_fwd_tm: 16-byte aligned rows");
  if ((const void*)x == (const void*)xm_out && !(ldx == 2 * G * c && xchunk == (G * c) / 4))
    return gkg_fail(GKG_ERR_SHAPE, "gkg_knn_mr_fwd_tm: x aliases xm_out but is not its x half (ldx = 2 C, xchunk = C / 4)");
  if (center_out && !nn_idx_out) return gkg_fail(GKG_ERR_NULL, "gkg_knn_mr_fwd_tm: center_out without nn_idx_out");
  return knn_fwd_impl(knn_call_tm(KNN_FUSED, B, G, c, N, M, k, dilation, GKG_F32, flags, y != nullptr, relpos != nullptr, ldx, xchunk),
                      KnnPtrs{x, y, relpos, nn_idx_out, center_out, nn16_out, workspace, workspace_bytes, stream, xm_out, arg_out});
}

// The Grapher's fc1 BN-apply (train mode, statistics from the projection's fp64 column sums: gkg_bn_apply_train's contract with
// nb == 1, act == 0, no residual) and the k-NN's token preparation of the SAME tokens in one pass (round 6):
//   y (B N, C) pre-BN projection output -> x = a y + c, written to `out` (row pitch ldo floats; ochunk > 0: the x half of the
//   grouped projection's operand buffer, include/gkg_hip.h "XM layout") AND normalised into `knn_workspace` — the workspace of the
//   k-NN call (gkg_knn_fwd_tm / _tm16 / gkg_knn_mr_fwd_tm) with the SAME (B, G, c, N, M, k, dilation, y / relative_pos presence,
//   flags) that follows with GKG_KNN_X_PREPARED set and x = `out`: it then launches no preparation for the queries (none at all
//   for a self graph).  fused_mr != 0: that call is gkg_knn_mr_fwd_tm.  Same arithmetic, same bits as apply + token_prep.
static int bn_apply_knn_prep_impl(const float* y, const double* sums, const float* gamma, const float* beta, const float* bias,
                                  float* running_mean, float* running_var, long long* num_batches_tracked, float* a, float* c_out,
                                  float* mean, float* invstd, float* out, int ldo, int ochunk, int B, int G, int c, int N, int M,
                                  int k, int dilation, int has_y, int has_relpos, unsigned knn_flags, int fused_mr,
                                  int as_keys, const float* res_tm, float* out_nchw,
                                  void* knn_workspace, size_t knn_workspace_bytes, float momentum, float eps, double* zero_buf,
                                  size_t zero_doubles, void* stream, const double* count, float* count_out) {
  if (!y || !sums || !gamma || !beta || !a || !c_out || !mean || !invstd || !out || !knn_workspace)
    return gkg_fail(GKG_ERR_NULL, "gkg_bn_apply_knn_prep: null pointer");
  if (!as_keys && (res_tm || out_nchw)) return gkg_fail(GKG_ERR_SHAPE, "gkg_bn_apply_knn_prep: res_tm / out_nchw belong to a keys producer");
  if (as_keys && (!has_y || ochunk != 0 || ((size_t)res_tm & 15))) return gkg_fail(GKG_ERR_SHAPE, "gkg_bn_apply_knn_prep: a keys producer writes plain rows for a problem with keys");
  if ((running_mean == nullptr) != (running_var == nullptr)) return gkg_fail(GKG_ERR_NULL, "gkg_bn_apply_knn_prep: running stats come in pairs");
  if (B <= 0 || G <= 0 || c <= 0 || (c & 3) || N <= 0) return gkg_fail(GKG_ERR_SHAPE, "gkg_bn_apply_knn_prep: bad sizes (c % 4 == 0)");
  const int C = G * c;
  if (ldo == 0) ldo = C;
  if (ldo < C || (ldo & 3) || ochunk < 0 || (ochunk & 3) || (ochunk > 0 && (C % ochunk || ldo < 2 * C)) || ((size_t)out & 15) || ((size_t)y & 15) ||
      (zero_doubles && !zero_buf))
    return gkg_fail(GKG_ERR_SHAPE, "gkg_bn_apply_knn_prep: bad output view");
  KnnPtrs t{y, nullptr, nullptr, nullptr, nullptr, nullptr, knn_workspace, knn_workspace_bytes, stream};
  t.aff.d = BnDerive{sums, gamma, beta, bias, running_mean, running_var, num_batches_tracked, a, c_out, mean, invstd,
                     B * (as_keys ? M : N), momentum, eps, zero_buf, zero_doubles, count, count_out};
  t.raw = out; t.raw_ld = ldo; t.raw_chunk = ochunk; t.res_tm = res_tm; t.nchw = out_nchw;
  return knn_fwd_impl(knn_call_tm(as_keys ? KNN_PRODUCE_KEYS : KNN_PRODUCE_QUERIES, B, G, c, N, M, k, dilation, GKG_F32, knn_flags, has_y != 0,
                                  has_relpos != 0, 0, 0, fused_mr != 0), t);
}

extern "C" int gkg_bn_apply_knn_prep(const float* y, const double* sums, const float* gamma, const float* beta, const float* bias,
                                     float* running_mean, float* running_var, long long* num_batches_tracked, float* a, float* c_out,
                                     float* mean, float* invstd, float* out, int ldo, int ochunk, int B, int G, int c, int N, int M,
                                     int k, int dilation, int has_y, int has_relpos, unsigned knn_flags, int fused_mr,
                                     int as_keys, const float* res_tm, float* out_nchw,
                                     void* knn_workspace, size_t knn_workspace_bytes, float momentum, float eps, double* zero_buf,
                                     size_t zero_doubles, void* stream) {
  return bn_apply_knn_prep_impl(y, sums, gamma, beta, bias, running_mean, running_var, num_batches_tracked, a, c_out, mean, invstd, out,
                                ldo, ochunk, B, G, c, N, M, k, dilation, has_y, has_relpos, knn_flags, fused_mr, as_keys, res_tm,
                                out_nchw, knn_workspace, knn_workspace_bytes, momentum, eps, zero_buf, zero_doubles, stream, nullptr,
                                nullptr);
}

// gkg_bn_apply_knn_prep behind a cross-rank exchange of the statistics: `sums` added up over the ranks, `count` / `count_out` as
// in gkg_bn_apply_train_sync (B: this rank's images).
extern "C" int gkg_bn_apply_knn_prep_sync(const float* y, const double* sums, const float* gamma, const float* beta, const float* bias,
                                          float* running_mean, float* running_var, long long* num_batches_tracked, float* a,
                                          float* c_out, float* mean, float* invstd, float* out, int ldo, int ochunk, int B, int G,
                                          int c, int N, int M, int k, int dilation, int has_y, int has_relpos, unsigned knn_flags,
                                          int fused_mr, int as_keys, const float* res_tm, float* out_nchw, void* knn_workspace,
                                          size_t knn_workspace_bytes, float momentum, float eps, double* zero_buf,
                                          size_t zero_doubles, const double* count, float* count_out, void* stream) {
  if (!count) return gkg_fail(GKG_ERR_NULL, "gkg_bn_apply_knn_prep_sync: null count");
  return bn_apply_knn_prep_impl(y, sums, gamma, beta, bias, running_mean, running_var, num_batches_tracked, a, c_out, mean, invstd, out,
                                ldo, ochunk, B, G, c, N, M, k, dilation, has_y, has_relpos, knn_flags, fused_mr, as_keys, res_tm,
                                out_nchw, knn_workspace, knn_workspace_bytes, momentum, eps, zero_buf, zero_doubles, stream, count,
                                count_out);
}

// gkg_knn_prep.h: the queries' preparation plan for a producer that prepares tokens it has just written to `tokens` (B N rows of
// pitch ld floats) inside its own kernel.  The plan of the k-NN call that follows (knn_plan, role KNN_QUERY_PREP_PLAN), no launch.
int gkg::knn_query_prep_plan(const float* tokens, int ld, int B, int G, int c, int N, int M, int k, int dilation, int has_y, int has_relpos,
                        unsigned knn_flags, int fused_mr, void* knn_workspace, size_t knn_workspace_bytes, KnnQueryPrep* plan) {
  KnnPtrs t{tokens, nullptr, nullptr, nullptr, nullptr, nullptr, knn_workspace, knn_workspace_bytes};
  t.want = plan;
  return knn_fwd_impl(knn_call_tm(KNN_QUERY_PREP_PLAN, B, G, c, N, M, k, dilation, GKG_F32, knn_flags, has_y != 0, has_relpos != 0, ld, 0,
                                  fused_mr != 0), t);
}

// The same pass behind an eval-mode (frozen) BatchNorm: the caller passes the folded scale / shift (gkg_bn_eval_affine) instead of
// column sums — out = a y + c (+ res_tm) with the arithmetic of gkg_affine_act / gkg_tm_affine_to_nchw_dual, then the k-NN's own
// preparation from the same registers.  Nothing but out, out_nchw and the workspace is written: no saved statistics, no running
// statistics, no scratch buffer to clear (BnDerive::sums == null keeps prep_affine_table away from all of them).
extern "C" int gkg_affine_knn_prep(const float* y, const float* a, const float* c_in, float* out, int ldo, int ochunk, int B, int G,
                                   int c, int N, int M, int k, int dilation, int has_y, int has_relpos, unsigned knn_flags,
                                   int fused_mr, int as_keys, const float* res_tm, float* out_nchw, void* knn_workspace,
                                   size_t knn_workspace_bytes, void* stream) {
  if (!y || !a || !c_in || !out || !knn_workspace) return gkg_fail(GKG_ERR_NULL, "gkg_affine_knn_prep: null pointer");
  if (!as_keys && (res_tm || out_nchw)) return gkg_fail(GKG_ERR_SHAPE, "gkg_affine_knn_prep: res_tm / out_nchw belong to a keys producer");
  if (as_keys && (!has_y || ochunk != 0 || ((size_t)res_tm & 15))) return gkg_fail(GKG_ERR_SHAPE, "gkg_affine_knn_prep: a keys producer writes plain rows for a problem with keys");
  if (B <= 0 || G <= 0 || c <= 0 || (c & 3) || N <= 0) return gkg_fail(GKG_ERR_SHAPE, "gkg_affine_knn_prep: bad sizes (c % 4 == 0)");
  const int C = G * c;
  if (ldo == 0) ldo = C;
  if (ldo < C || (ldo & 3) || ochunk < 0 || (ochunk & 3) || (ochunk > 0 && (C % ochunk || ldo < 2 * C)) || ((size_t)out & 15) || ((size_t)y & 15))
    return gkg_fail(GKG_ERR_SHAPE, "gkg_affine_knn_prep: bad output view");
  KnnPtrs t{y, nullptr, nullptr, nullptr, nullptr, nullptr, knn_workspace, knn_workspace_bytes, stream};
  t.aff.a = a; t.aff.c = c_in;                     // aff.d.sums == null: the table is copied from a / c
  t.raw = out; t.raw_ld = ldo; t.raw_chunk = ochunk; t.res_tm = res_tm; t.nchw = out_nchw;
  return knn_fwd_impl(knn_call_tm(as_keys ? KNN_PRODUCE_KEYS : KNN_PRODUCE_QUERIES, B, G, c, N, M, k, dilation, GKG_F32, knn_flags, has_y != 0,
                                  has_relpos != 0, 0, 0, fused_mr != 0), t);
}
