// gkg_gconv.hip — the GIN and graph-attention aggregations of GraphConv2d (reference vig_model/torch_vertex.py:134-150
// GINConv2d, :16-37 GraphAtten), the graph convolutions GKGNet's configs do not select ('mr' is) but Grapher(conv='gin' /
// 'gat') offers.  (conv='sage' needs no kernel of its own: nn1 is per-position linear, so it runs on gkg_edge.hip with qc NULL.)
//
// Both reference forms materialise (B, C, N, k) gathers (GAT also a (B, 2C, N, k) concatenation reduced to one logit per edge);
// here every edge is read in place:
//   GIN   h[n] = (1 + eps) x[n] + sum_k src[j_nk]                                 eps read from device memory (no host sync)
//   GAT   t[n] = a[:C] . x[n] + bias,  s[m] = a[C:] . src[m],  e_nk = t[n] + s[j_nk]
//         p_nk = softmax_k(e_nk) (max-subtracted),  agg[n] = sum_k p_nk src[j_nk]          p (B, N, k) saved for the backward
// The centre of every edge is the query itself (edge_index[1][b][n][k] == n, as the k-NN produces it and the max-relative
// and edge kernels assume): the caller does not pass edge_index[1].
//
// Backward.  The source gradients are scatters over the edges (gsrc[j] += ...).  They are computed as a GATHER over the
// transposed graph instead: gc_transpose builds, per image, the list of edges that end at each key (CSR; counting with
// integer atomics, then every key's list sorted by edge number), and one thread per (b, c, m) sums its key's edges in that
// order.  No floating-point atomics anywhere: every result is bit-identical from run to run.  The parameter gradients
// (GIN eps, GAT a / bias) are per-channel fp64 block reductions in a fixed order, then a fixed-order sum.
//   GIN   gx = (1 + eps) gh  (+ the scatter for a self graph);  gsrc[j] += gh[n];  geps = sum gh x
//   GAT   dp_nk = g[n] . src[j];  de_nk = p_nk (dp_nk - sum_k' p dp);  gsrc[j] += p_nk g[n] + de_nk a[C:];
//         gx[n] += (sum_k de_nk) a[:C];  da[:C] = sum_n (sum_k de_nk) x[n];  da[C:] = sum de_nk src[j];  dbias = sum de
// Layout: channel-major fp32 (B, C, N) / (B, C, M), nn_idx (B, N, k) int64; out-of-range indices are clamped into the row.
#include "gkg_common.h"

namespace gkg {

__device__ __forceinline__ int gc_idx(int64_t v, int M) { return (int)(v < 0 ? 0 : (v >= M ? M - 1 : v)); }

__device__ __forceinline__ double gc_block_sum(double v, double* sm) {     // 256 threads, fixed reduction tree
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sm[w] = v;
  __syncthreads();
  return (sm[0] + sm[1]) + (sm[2] + sm[3]);
}

// ---- workspace: [cnt B*M | off B*(M+1) | list B*N*k] int32, [f0 B*N*k | f1 B*N | f2 B*M] fp32, [part 2C+2] fp64
struct GcWs {
  int *cnt, *off, *list;
  float *f0, *f1, *f2;
  double* part;
};
static size_t gc_align(size_t v) { return (v + 255) & ~(size_t)255; }
static size_t gc_ws_layout(int B, int C, int N, int M, int k, char* base, GcWs* w) {
  const size_t E = (size_t)B * N * k;
  size_t o = 0;
  const size_t o_cnt = o; o = gc_align(o + 4 * (size_t)B * M);
  const size_t o_off = o; o = gc_align(o + 4 * (size_t)B * (M + 1));
  const size_t o_list = o; o = gc_align(o + 4 * E);
  const size_t o_f0 = o; o = gc_align(o + 4 * E);
  const size_t o_f1 = o; o = gc_align(o + 4 * (size_t)B * N);
  const size_t o_f2 = o; o = gc_align(o + 4 * (size_t)B * M);
  const size_t o_part = o; o = gc_align(o + 8 * (size_t)(2 * C + 2));
  if (w) {
    w->cnt = (int*)(base + o_cnt); w->off = (int*)(base + o_off); w->list = (int*)(base + o_list);
    w->f0 = (float*)(base + o_f0); w->f1 = (float*)(base + o_f1); w->f2 = (float*)(base + o_f2);
    w->part = (double*)(base + o_part);
  }
  return o;
}

// ---- transposed graph ---------------------------------------------------------------------------------------------------
// The counters are cleared by a kernel, not by hipMemsetAsync: every step of the sequence is then a kernel node when the call is
// captured into a hipGraph (a capture with the two memset nodes between the kernels faulted on replay: EXPERIMENTS.md "GIN / GAT
// kernels vs fp64").
__global__ __launch_bounds__(256) void gc_zero_kernel(int* __restrict__ p, long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = 0;
}

__global__ __launch_bounds__(256) void gc_count_kernel(const int64_t* __restrict__ idx, int* __restrict__ cnt, int M, int NK,
                                                       long long E) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  const int b = (int)(e / NK);
  atomicAdd(cnt + (size_t)b * M + gc_idx(idx[e], M), 1);
}

__global__ __launch_bounds__(256) void gc_scan_kernel(const int* __restrict__ cnt, int* __restrict__ off, int M) {
  __shared__ int part[256];
  const int b = blockIdx.x, t = threadIdx.x;
  const int per = (M + 255) / 256;
  const int lo = min(M, t * per), hi = min(M, lo + per);
  const int* c = cnt + (size_t)b * M;
  int* o = off + (size_t)b * (M + 1);
  int s = 0;
  for (int m = lo; m < hi; ++m) s += c[m];
  part[t] = s;
  __syncthreads();
  if (t == 0) {
    int run = 0;
    for (int i = 0; i < 256; ++i) { const int v = part[i]; part[i] = run; run += v; }
    o[M] = run;
  }
  __syncthreads();
  int run = part[t];
  for (int m = lo; m < hi; ++m) { o[m] = run; run += c[m]; }
}

__global__ __launch_bounds__(256) void gc_fill_kernel(const int64_t* __restrict__ idx, const int* __restrict__ off,
                                                      int* __restrict__ cursor, int* __restrict__ list, int M, int NK, long long E) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  const int b = (int)(e / NK);
  const int local = (int)(e - (long long)b * NK);
  const int j = gc_idx(idx[e], M);
  const int pos = atomicAdd(cursor + (size_t)b * M + j, 1);
  list[(size_t)b * NK + off[(size_t)b * (M + 1) + j] + pos] = local;
}

// the fill order depends on the atomics' arrival order: sorting every key's list by edge number makes it canonical
__global__ __launch_bounds__(256) void gc_sort_kernel(const int* __restrict__ off, int* __restrict__ list, int M, int NK, long long BM) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= BM) return;
  const int b = (int)(t / M), m = (int)(t - (long long)b * M);
  int* L = list + (size_t)b * NK;
  const int lo = off[(size_t)b * (M + 1) + m], hi = off[(size_t)b * (M + 1) + m + 1];
  for (int i = lo + 1; i < hi; ++i) {
    const int v = L[i];
    int q = i - 1;
    while (q >= lo && L[q] > v) { L[q + 1] = L[q]; --q; }
    L[q + 1] = v;
  }
}

static int gc_transpose(const int64_t* idx, int B, int N, int M, int k, const GcWs& w, hipStream_t st) {
  const int NK = N * k;
  const long long E = (long long)B * NK, BM = (long long)B * M;
  hipLaunchKernelGGL(gc_zero_kernel, dim3((unsigned)((BM + 255) / 256)), dim3(256), 0, st, w.cnt, BM);
  hipLaunchKernelGGL(gc_count_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, st, idx, w.cnt, M, NK, E);
  hipLaunchKernelGGL(gc_scan_kernel, dim3(B), dim3(256), 0, st, w.cnt, w.off, M);
  hipLaunchKernelGGL(gc_zero_kernel, dim3((unsigned)((BM + 255) / 256)), dim3(256), 0, st, w.cnt, BM);   // the counts become the fill cursors
  hipLaunchKernelGGL(gc_fill_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, st, idx, w.off, w.cnt, w.list, M, NK, E);
  hipLaunchKernelGGL(gc_sort_kernel, dim3((unsigned)((BM + 255) / 256)), dim3(256), 0, st, w.off, w.list, M, NK, BM);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : gkg_fail_hip(e, "gc_transpose");
}

// out[c] = sum_{b, n < L} u[b ub + c uc + n] * (v ? v[b vb + c vc + n] : 1), fp64, one workgroup per channel, fixed order
__global__ __launch_bounds__(256) void gc_chan_dot_kernel(const float* __restrict__ u, size_t ub, size_t uc,
                                                          const float* __restrict__ v, size_t vb, size_t vc,
                                                          double* __restrict__ out, int B, int L) {
  __shared__ double sm[4];
  const int c = blockIdx.x;
  double s = 0.0;
  const long long T = (long long)B * L;
  for (long long i = threadIdx.x; i < T; i += 256) {
    const int b = (int)(i / L), n = (int)(i - (long long)b * L);
    const double uu = (double)u[b * ub + c * uc + n];
    s += v ? uu * (double)v[b * vb + c * vc + n] : uu;
  }
  s = gc_block_sum(s, sm);
  if (threadIdx.x == 0) out[c] = s;
}

__global__ __launch_bounds__(256) void gc_sum_kernel(const double* __restrict__ in, int n, double* __restrict__ out) {
  __shared__ double sm[4];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += in[i];
  s = gc_block_sum(s, sm);
  if (threadIdx.x == 0) out[0] = s;
}

// ---- GIN ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gin_fwd_kernel(const float* __restrict__ x, const float* __restrict__ src,
                                                      const int64_t* __restrict__ idx, const float* __restrict__ eps,
                                                      float* __restrict__ h, int C, int N, int M, int k) {
  const int n = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y, b = blockIdx.z;
  if (n >= N) return;
  const float* s = src + ((size_t)b * C + c) * M;
  const int64_t* ip = idx + ((size_t)b * N + n) * k;
  float acc = 0.f;
  for (int kk = 0; kk < k; ++kk) acc += s[gc_idx(ip[kk], M)];
  const size_t at = ((size_t)b * C + c) * N + n;
  h[at] = (1.f + eps[0]) * x[at] + acc;
}

template <bool SELF>
__global__ __launch_bounds__(256) void gin_bwd_kernel(const float* __restrict__ gh, const float* __restrict__ eps,
                                                      const int* __restrict__ off, const int* __restrict__ list,
                                                      float* __restrict__ gx, float* __restrict__ gsrc, int C, int N, int M, int k) {
  const int t = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y, b = blockIdx.z;
  const float s1 = 1.f + eps[0];
  const float* g = gh + ((size_t)b * C + c) * N;
  if (!SELF && t < N) gx[((size_t)b * C + c) * N + t] = s1 * g[t];
  if (t >= M) return;
  const int* o = off + (size_t)b * (M + 1);
  const int* L = list + (size_t)b * N * k;
  float acc = SELF ? s1 * g[t] : 0.f;
  for (int q = o[t]; q < o[t + 1]; ++q) acc += g[L[q] / k];
  (SELF ? gx : gsrc)[((size_t)b * C + c) * M + t] = acc;
}

// ---- GAT ----------------------------------------------------------------------------------------------------------------
// t[b][n] = sum_c w[c] x[b][c][n] (+ bias[0]); one thread per node, channels in order
__global__ __launch_bounds__(256) void gat_logit_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ bias, float* __restrict__ t, int C, int N) {
  const int n = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (n >= N) return;
  const float* xp = x + (size_t)b * C * N + n;
  float acc = 0.f;
  for (int c = 0; c < C; ++c) acc += w[c] * xp[(size_t)c * N];
  t[(size_t)b * N + n] = bias ? acc + bias[0] : acc;
}

__global__ __launch_bounds__(256) void gat_softmax_kernel(const float* __restrict__ t, const float* __restrict__ s,
                                                          const int64_t* __restrict__ idx, float* __restrict__ p, int N, int M,
                                                          int k, long long BN) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= BN) return;
  const int b = (int)(i / N);
  const int64_t* ip = idx + (size_t)i * k;
  float* pp = p + (size_t)i * k;
  const float* sb = s + (size_t)b * M;
  const float ti = t[i];
  float mx = -INFINITY;
  for (int kk = 0; kk < k; ++kk) {
    const float e = ti + sb[gc_idx(ip[kk], M)];
    pp[kk] = e;
    mx = fmaxf(mx, e);
  }
  float den = 0.f;
  for (int kk = 0; kk < k; ++kk) {
    const float v = expf(pp[kk] - mx);
    pp[kk] = v;
    den += v;
  }
  for (int kk = 0; kk < k; ++kk) pp[kk] = pp[kk] / den;
}

__global__ __launch_bounds__(256) void gat_agg_kernel(const float* __restrict__ src, const int64_t* __restrict__ idx,
                                                      const float* __restrict__ p, float* __restrict__ agg, int C, int N, int M,
                                                      int k) {
  const int n = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y, b = blockIdx.z;
  if (n >= N) return;
  const float* s = src + ((size_t)b * C + c) * M;
  const int64_t* ip = idx + ((size_t)b * N + n) * k;
  const float* pp = p + ((size_t)b * N + n) * k;
  float acc = 0.f;
  for (int kk = 0; kk < k; ++kk) acc += pp[kk] * s[gc_idx(ip[kk], M)];
  agg[((size_t)b * C + c) * N + n] = acc;
}

// dp[e] = g[b][:][n] . src[b][:][j_e], one thread per edge
__global__ __launch_bounds__(256) void gat_dp_kernel(const float* __restrict__ g, const float* __restrict__ src,
                                                     const int64_t* __restrict__ idx, float* __restrict__ dp, int C, int N, int M,
                                                     int k, long long E) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  const long long bn = e / k;
  const int b = (int)(bn / N), n = (int)(bn - (long long)b * N);
  const int j = gc_idx(idx[e], M);
  const float* gp = g + (size_t)b * C * N + n;
  const float* sp = src + (size_t)b * C * M + j;
  float acc = 0.f;
  for (int c = 0; c < C; ++c) acc += gp[(size_t)c * N] * sp[(size_t)c * M];
  dp[e] = acc;
}

// in place dp -> de = p (dp - sum_k p dp); sde[b][n] = sum_k de
__global__ __launch_bounds__(256) void gat_de_kernel(const float* __restrict__ p, float* __restrict__ de, float* __restrict__ sde,
                                                     int k, long long BN) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= BN) return;
  const float* pp = p + (size_t)i * k;
  float* d = de + (size_t)i * k;
  float dot = 0.f;
  for (int kk = 0; kk < k; ++kk) dot += pp[kk] * d[kk];
  float s = 0.f;
  for (int kk = 0; kk < k; ++kk) {
    const float v = pp[kk] * (d[kk] - dot);
    d[kk] = v;
    s += v;
  }
  sde[i] = s;
}

// sdes[b][m] = sum of de over the edges that end at key m, in edge order
__global__ __launch_bounds__(256) void gat_key_de_kernel(const float* __restrict__ de, const int* __restrict__ off,
                                                         const int* __restrict__ list, float* __restrict__ sdes, int M, int NK,
                                                         long long BM) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= BM) return;
  const int b = (int)(t / M), m = (int)(t - (long long)b * M);
  const int* L = list + (size_t)b * NK;
  const float* d = de + (size_t)b * NK;
  float acc = 0.f;
  for (int q = off[(size_t)b * (M + 1) + m]; q < off[(size_t)b * (M + 1) + m + 1]; ++q) acc += d[L[q]];
  sdes[t] = acc;
}

template <bool SELF>
__global__ __launch_bounds__(256) void gat_bwd_gather_kernel(const float* __restrict__ g, const float* __restrict__ p,
                                                             const float* __restrict__ de, const float* __restrict__ sde,
                                                             const float* __restrict__ a, const int* __restrict__ off,
                                                             const int* __restrict__ list, float* __restrict__ gx,
                                                             float* __restrict__ gsrc, int C, int N, int M, int k) {
  const int t = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y, b = blockIdx.z;
  const float a1 = a[c], a2 = a[C + c];
  const float* gb = g + ((size_t)b * C + c) * N;
  if (!SELF && t < N) gx[((size_t)b * C + c) * N + t] = sde[(size_t)b * N + t] * a1;
  if (t >= M) return;
  const int* o = off + (size_t)b * (M + 1);
  const int* L = list + (size_t)b * N * k;
  const float* pb = p + (size_t)b * N * k;
  const float* db = de + (size_t)b * N * k;
  float acc = SELF ? sde[(size_t)b * N + t] * a1 : 0.f;
  for (int q = o[t]; q < o[t + 1]; ++q) {
    const int e = L[q];
    acc += pb[e] * gb[e / k] + db[e] * a2;
  }
  (SELF ? gx : gsrc)[((size_t)b * C + c) * M + t] = acc;
}

static int gc_check(const void* x, const void* idx, int B, int C, int N, int M, int k, const char* who) {
  if (!x || !idx) return gkg_fail(GKG_ERR_NULL, who);
  if (B <= 0 || C <= 0 || N <= 0 || M <= 0 || k <= 0 || B > 65535 || C > 65535 || (long long)N * k > 0x7fffffffLL ||
      (long long)B * N * k > 0x7fffffffLL * 256LL || (long long)B * M > 0x7fffffffLL * 256LL)
    return gkg_fail(GKG_ERR_SHAPE, who);
  return 0;
}

static int gc_ws(void* ws, size_t ws_bytes, int B, int C, int N, int M, int k, GcWs* w, const char* who) {
  if (!ws) return gkg_fail(GKG_ERR_NULL, who);
  if (ws_bytes < gc_ws_layout(B, C, N, M, k, nullptr, nullptr)) return gkg_fail(GKG_ERR_WORKSPACE, who);
  gc_ws_layout(B, C, N, M, k, (char*)ws, w);
  return 0;
}

}  // namespace gkg
using namespace gkg;

extern "C" size_t gkg_gconv_workspace_bytes(int B, int C, int N, int M, int k) {
  if (B <= 0 || C <= 0 || N <= 0 || M <= 0 || k <= 0) return 0;
  return gc_ws_layout(B, C, N, M, k, nullptr, nullptr);
}

extern "C" int gkg_gin_fwd(const float* x, const float* src, const int64_t* nn_idx, const float* eps, float* h, int B, int C,
                           int N, int M, int k, void* stream) {
  if (int rc = gc_check(x, nn_idx, B, C, N, M, k, "gkg_gin_fwd: bad pointer / size")) return rc;
  if (!eps || !h) return gkg_fail(GKG_ERR_NULL, "gkg_gin_fwd: eps, h required");
  if (!src && M != N) return gkg_fail(GKG_ERR_SHAPE, "gkg_gin_fwd: self graph needs M == N");
  hipLaunchKernelGGL(gin_fwd_kernel, dim3((N + 255) / 256, C, B), dim3(256), 0, (hipStream_t)stream, x, src ? src : x, nn_idx, eps,
                     h, C, N, M, k);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : gkg_fail_hip(e, "gin_fwd_kernel");
}

extern "C" int gkg_gin_bwd(const float* gh, const float* x, const float* eps, const int64_t* nn_idx, float* gx, float* gsrc,
                           double* geps, int B, int C, int N, int M, int k, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = gc_check(gh, nn_idx, B, C, N, M, k, "gkg_gin_bwd: bad pointer / size")) return rc;
  if (!eps || !gx || (geps && !x)) return gkg_fail(GKG_ERR_NULL, "gkg_gin_bwd: eps, gx required (x too when geps is given)");
  if (!gsrc && M != N) return gkg_fail(GKG_ERR_SHAPE, "gkg_gin_bwd: self graph needs M == N");
  GcWs w;
  if (int rc = gc_ws(ws, ws_bytes, B, C, N, M, k, &w, "gkg_gin_bwd: workspace")) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = gc_transpose(nn_idx, B, N, M, k, w, st)) return rc;
  const dim3 grid((max(N, M) + 255) / 256, C, B);
  if (gsrc) hipLaunchKernelGGL(gin_bwd_kernel<false>, grid, dim3(256), 0, st, gh, eps, w.off, w.list, gx, gsrc, C, N, M, k);
  else hipLaunchKernelGGL(gin_bwd_kernel<true>, grid, dim3(256), 0, st, gh, eps, w.off, w.list, gx, gsrc, C, N, M, k);
  if (geps) {
    hipLaunchKernelGGL(gc_chan_dot_kernel, dim3(C), dim3(256), 0, st, gh, (size_t)C * N, (size_t)N, x, (size_t)C * N, (size_t)N,
                       w.part, B, N);
    hipLaunchKernelGGL(gc_sum_kernel, dim3(1), dim3(256), 0, st, w.part, C, geps);
  }
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : gkg_fail_hip(e, "gin_bwd_kernel");
}

extern "C" int gkg_gat_fwd(const float* x, const float* src, const int64_t* nn_idx, const float* a, const float* bias, float* agg,
                           float* p, int B, int C, int N, int M, int k, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = gc_check(x, nn_idx, B, C, N, M, k, "gkg_gat_fwd: bad pointer / size")) return rc;
  if (!a || !agg || !p) return gkg_fail(GKG_ERR_NULL, "gkg_gat_fwd: a, agg, p required");
  if (!src && M != N) return gkg_fail(GKG_ERR_SHAPE, "gkg_gat_fwd: self graph needs M == N");
  GcWs w;
  if (int rc = gc_ws(ws, ws_bytes, B, C, N, M, k, &w, "gkg_gat_fwd: workspace")) return rc;
  hipStream_t st = (hipStream_t)stream;
  const float* s = src ? src : x;
  const long long BN = (long long)B * N;
  hipLaunchKernelGGL(gat_logit_kernel, dim3((N + 255) / 256, B), dim3(256), 0, st, x, a, bias, w.f1, C, N);
  hipLaunchKernelGGL(gat_logit_kernel, dim3((M + 255) / 256, B), dim3(256), 0, st, s, a + C, (const float*)nullptr, w.f2, C, M);
  hipLaunchKernelGGL(gat_softmax_kernel, dim3((unsigned)((BN + 255) / 256)), dim3(256), 0, st, w.f1, w.f2, nn_idx, p, N, M, k, BN);
  hipLaunchKernelGGL(gat_agg_kernel, dim3((N + 255) / 256, C, B), dim3(256), 0, st, s, nn_idx, p, agg, C, N, M, k);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : gkg_fail_hip(e, "gat_fwd kernels");
}

extern "C" int gkg_gat_bwd(const float* g, const float* x, const float* src, const int64_t* nn_idx, const float* a, const float* p,
                           float* gx, float* gsrc, double* da, double* dbias, int B, int C, int N, int M, int k, void* ws,
                           size_t ws_bytes, void* stream) {
  if (int rc = gc_check(g, nn_idx, B, C, N, M, k, "gkg_gat_bwd: bad pointer / size")) return rc;
  if (!x || !a || !p || !gx) return gkg_fail(GKG_ERR_NULL, "gkg_gat_bwd: x, a, p, gx required");
  if ((!src) != (!gsrc)) return gkg_fail(GKG_ERR_NULL, "gkg_gat_bwd: src and gsrc are given together (bipartite) or not at all");
  if (!src && M != N) return gkg_fail(GKG_ERR_SHAPE, "gkg_gat_bwd: self graph needs M == N");
  GcWs w;
  if (int rc = gc_ws(ws, ws_bytes, B, C, N, M, k, &w, "gkg_gat_bwd: workspace")) return rc;
  hipStream_t st = (hipStream_t)stream;
  const float* s = src ? src : x;
  const long long E = (long long)B * N * k, BN = (long long)B * N, BM = (long long)B * M;
  if (int rc = gc_transpose(nn_idx, B, N, M, k, w, st)) return rc;
  hipLaunchKernelGGL(gat_dp_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, st, g, s, nn_idx, w.f0, C, N, M, k, E);
  hipLaunchKernelGGL(gat_de_kernel, dim3((unsigned)((BN + 255) / 256)), dim3(256), 0, st, p, w.f0, w.f1, k, BN);
  const dim3 grid((max(N, M) + 255) / 256, C, B);
  if (gsrc) hipLaunchKernelGGL(gat_bwd_gather_kernel<false>, grid, dim3(256), 0, st, g, p, w.f0, w.f1, a, w.off, w.list, gx, gsrc,
                               C, N, M, k);
  else hipLaunchKernelGGL(gat_bwd_gather_kernel<true>, grid, dim3(256), 0, st, g, p, w.f0, w.f1, a, w.off, w.list, gx, gsrc, C, N,
                          M, k);
  if (da) {
    hipLaunchKernelGGL(gat_key_de_kernel, dim3((unsigned)((BM + 255) / 256)), dim3(256), 0, st, w.f0, w.off, w.list, w.f2, M, N * k, BM);
    hipLaunchKernelGGL(gc_chan_dot_kernel, dim3(C), dim3(256), 0, st, x, (size_t)C * N, (size_t)N, (const float*)w.f1, (size_t)N,
                       (size_t)0, da, B, N);
    hipLaunchKernelGGL(gc_chan_dot_kernel, dim3(C), dim3(256), 0, st, s, (size_t)C * M, (size_t)M, (const float*)w.f2, (size_t)M,
                       (size_t)0, da + C, B, M);
  }
  if (dbias)
    hipLaunchKernelGGL(gc_chan_dot_kernel, dim3(1), dim3(256), 0, st, (const float*)w.f1, (size_t)N, (size_t)0, (const float*)nullptr,
                       (size_t)0, (size_t)0, dbias, B, N);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : gkg_fail_hip(e, "gat_bwd kernels");
}
