// gkg_gemm_x6.hip — the Grapher block's dense projections (forward and input-gradient) on the bf16 matrix cores at fp32
// accuracy: every fp32 operand is split into three bf16 terms, x = hi + mid + lo (exactly: each residual is computed in
// fp32 and is representable), and six of the nine cross products are kept
//     a*b ~= ah*bh + [ah*bm + am*bh + am*bm + ah*bl + al*bh]          (dropped: am*bl, al*bm, al*bl <= 2^-24 |a*b|)
// accumulated in fp32 by v_mfma_f32_32x32x16_bf16, the bracketed corrections in their own accumulator.  Measured against
// an fp64 evaluation (tools/ubench/gemm_x6_bench.hip, K = 320..1280): max error 5.0e-8 * sum|a b|, mean 4.6e-9 — three
// to four times SMALLER than the fp32-MFMA kernel of gkg_gemm.hip (1.5e-7 / 1.7e-8) and than any fp32 fma chain of that
// length; 6 bf16 MFMAs cost 6*32 cycles per 32x32x16 block where the fp32 MFMA costs 8*64.
//
// Replaces (reference torch_vertex.py:290-306 fc1 / fc2, :57-62 + torch_nn.py:57-69 BasicConv groups=4, :334-360
// FFNLabel — the 1x1 convolutions and their input gradients):
//     forward   Y[m][n]  = sum_k X[m][k]  W[n][k]     (+ train-mode BN column statistics in the epilogue)
//     dgrad     dX[m][n] = sum_k dY[m][k] W[k][n]
// Both are C = A * B^T with A a row-major fp32 activation matrix and B a WEIGHT matrix, so the weights are split once per
// optimiser step by x6_prep_kernel (both orientations, all registered layers, one launch) into
//     planes[p][k/8][n][8]  bf16      p = hi, mid, lo;  n padded to 128, k padded to 32 (zeros)
// and only the activation operand is split inside the GEMM.
//
// Kernel (256 threads = 4 waves, tile 128 rows x 32*NI columns, K-step 32):
//   * waves are stacked 4(M) x 1(N): wave w owns rows [32w, 32w+32), so each A element is split by exactly one wave.  Its
//     rows travel global -> the wave's PRIVATE LDS ring (LDS-DMA, 3 stages, no workgroup barrier on that path) -> registers
//     (2 ds_read_b128 per 16-deep half step; the ring image is XOR-swizzled on the SOURCE address, conflict-free), where
//     the 44-instruction split runs in the shadow of the MFMAs (4-5 VALU per MFMA gap: measured free up to ~5,
//     tools/ubench/mfma_bf16_fill.hip);
//   * the weight planes are DMA'd as 1-KiB contiguous pieces (64 n x 16 B) into a 2-stage image [p][k/8][n] that every
//     wave reads conflict-free with ds_read_b128 — no VALU on the B side at all;
//   * one workgroup barrier per K-step, in the MIDDLE of the step: it certifies stage kt+1 (first read right after it)
//     and releases stage kt's B image and the wave's oldest A slot for the DMA issued next; counted vmcnt leaves the
//     newest A stage in flight across it;
//   * XCD-aware 1-D grid: the column tiles of one 128-row block run back to back on one XCD, so the row block is fetched
//     from HBM into that L2 once.
#include "gkg_common.h"
#include "gkg_x6_plan.h"
#include <stdlib.h>

namespace gkg {

typedef float x6_f32x16 __attribute__((ext_vector_type(16)));
typedef __attribute__((__vector_size__(8 * sizeof(__bf16)))) __bf16 x6_bf16x8;
typedef __bf16 x6_bf16x2 __attribute__((ext_vector_type(2)));
typedef float x6_f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned x6_cvt2(float a, float b) {
  x6_f32x2 v = {a, b};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, x6_bf16x2));      // v_cvt_pk_bf16_f32 (RNE)
}

// two floats -> packed (hi, mid, lo) bf16 pairs; the residuals are exact fp32 differences
__device__ __forceinline__ void x6_split2(float x0, float x1, unsigned& h, unsigned& m, unsigned& l) {
  h = x6_cvt2(x0, x1);
  const float r0 = x0 - __uint_as_float(h << 16), r1 = x1 - __uint_as_float(h & 0xffff0000u);
  m = x6_cvt2(r0, r1);
  const float s0 = r0 - __uint_as_float(m << 16), s1 = r1 - __uint_as_float(m & 0xffff0000u);
  l = x6_cvt2(s0, s1);
}

// ---- weight planes ------------------------------------------------------------------------------------------------------
// One descriptor per registered projection weight w (nb, N, K) row-major (N = cout, K = cin per group):
//   forward planes  pf: [nb][3][KCf][NPf][8]   B[n][k] = w[n][k]      NPf = roundup(N, 128), KCf = roundup(K, 32) / 8
//   dgrad planes    pd: [nb][3][KCd][NPd][8]   B[n][k] = w[k][n]      NPd = roundup(K, 128), KCd = roundup(N, 32) / 8
// A work unit is one (k/8, n) pair = 8 floats in, 3 x 16 B out; unit_begin is the running unit count over descriptors.
// kperm (the grouped projection behind the max-relative aggregation, reference torch_vertex.py:57-61 + torch_nn.py:61): the
// activation operand arrives as [x chunk | m chunk] (gkg_common.h "XM layout") instead of the reference's interleave
// [x_0, m_0, x_1, m_1, ...], so the planes hold the weight's INPUT columns in that order: plane position p < K/2 is column 2p
// (an x channel), p >= K/2 column 2 (p - K/2) + 1 (its m).  The weight tensor itself keeps the reference's layout.
struct X6PrepDesc {
  const float* w;
  uint4* pf;
  uint4* pd;
  int nb, N, K;
  int unit_begin;
  int kperm;
};
__device__ __host__ __forceinline__ int x6_kperm_src(int p, int K) { const int h = K >> 1; return p < h ? 2 * p : 2 * (p - h) + 1; }

// Zero jobs riding in the same launch (round 5): a training step begins by clearing its gradient arena and the BN scratch — two
// more 5 us launches in front of the first projection.  Workgroups past the unit blocks clear up to two buffers (16-byte units).
struct X6ZeroJobs {
  uint4* p[2];
  unsigned long long n16[2];        // 16-byte units
  int unit_blocks;                  // workgroups [0, unit_blocks) split weights, the rest clear
};

__global__ __launch_bounds__(256) void x6_prep_kernel(const X6PrepDesc* __restrict__ descs, int ndesc, int total_units, X6ZeroJobs zj) {
  if ((int)blockIdx.x >= zj.unit_blocks) {
    const unsigned long long zb = blockIdx.x - zj.unit_blocks, stride = (unsigned long long)(gridDim.x - zj.unit_blocks) * 256;
#pragma unroll
    for (int j = 0; j < 2; ++j)
      for (unsigned long long i = zb * 256 + threadIdx.x; i < zj.n16[j]; i += stride) zj.p[j][i] = make_uint4(0, 0, 0, 0);
    return;
  }
  __shared__ int begin[256];
  __shared__ int first;
  const int u0 = blockIdx.x * 256;
  if ((int)threadIdx.x < ndesc) begin[threadIdx.x] = descs[threadIdx.x].unit_begin;
  __syncthreads();
  if (threadIdx.x == 0) {                      // the block's 256 consecutive units start in this descriptor
    int d0 = 0;
    while (d0 + 1 < ndesc && begin[d0 + 1] <= u0) ++d0;
    first = d0;
  }
  __syncthreads();
  const int u = u0 + threadIdx.x;
  if (u >= total_units) return;
  int d = first;
  while (d + 1 < ndesc && begin[d + 1] <= u) ++d;
  const X6PrepDesc g = descs[d];
  int v = u - g.unit_begin;
  const int NPf = (g.N + X6_NPAD - 1) / X6_NPAD * X6_NPAD, KCf = (g.K + 31) / 32 * 4;
  const int NPd = (g.K + X6_NPAD - 1) / X6_NPAD * X6_NPAD, KCd = (g.N + 31) / 32 * 4;
  const int fwd_units = g.pf ? g.nb * KCf * NPf : 0;        // an orientation nobody asked for (null planes) has no units
  const bool dgrad = v >= fwd_units;
  if (dgrad) v -= fwd_units;
  const int NP = dgrad ? NPd : NPf, KC = dgrad ? KCd : KCf;
  const int Nn = dgrad ? g.K : g.N, Kk = dgrad ? g.N : g.K;      // extents of (n, k) in this orientation
  const int n = v % NP, kc = (v / NP) % KC, z = v / (NP * KC);
  const float* w = g.w + (size_t)z * g.N * g.K;
  float f[8];
  if (g.kperm) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = kc * 8 + j;
      f[j] = (n < Nn && k < Kk) ? (dgrad ? w[(size_t)k * g.K + x6_kperm_src(n, g.K)] : w[(size_t)n * g.K + x6_kperm_src(k, g.K)]) : 0.f;
    }
  } else if (!dgrad && n < Nn && kc * 8 + 8 <= Kk && (g.K & 3) == 0) {          // forward orientation: 8 consecutive floats of row n
    const float4 v0 = *reinterpret_cast<const float4*>(w + (size_t)n * g.K + kc * 8);
    const float4 v1 = *reinterpret_cast<const float4*>(w + (size_t)n * g.K + kc * 8 + 4);
    f[0] = v0.x; f[1] = v0.y; f[2] = v0.z; f[3] = v0.w; f[4] = v1.x; f[5] = v1.y; f[6] = v1.z; f[7] = v1.w;
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = kc * 8 + j;
      f[j] = (n < Nn && k < Kk) ? (dgrad ? w[(size_t)k * g.K + n] : w[(size_t)n * g.K + k]) : 0.f;
    }
  }
  uint4 h, m, l;
  x6_split2(f[0], f[1], h.x, m.x, l.x); x6_split2(f[2], f[3], h.y, m.y, l.y);
  x6_split2(f[4], f[5], h.z, m.z, l.z); x6_split2(f[6], f[7], h.w, m.w, l.w);
  uint4* P = (dgrad ? g.pd : g.pf) + (size_t)z * 3 * KC * NP;
  const size_t plane = (size_t)KC * NP, at = (size_t)kc * NP + n;
  P[at] = h; P[plane + at] = m; P[2 * plane + at] = l;
}

// ---- the GEMM -----------------------------------------------------------------------------------------------------------
struct X6Args {
  const float* A;  size_t a_bstride;  int lda;          // (nb, M, K) activations, row pitch lda floats (lda % 4 == 0)
  const uint4* P;  size_t p_bstride;                    // weight planes of this orientation, uint4 units per batch
  float* C;  size_t c_bstride;  int ldc;
  int M, N, K;
  int NP, KC;                                           // plane geometry (padded n, k/8 chunks)
  int mtiles, ntiles;
  double* sums;  int nslots, nbatch;                    // EPI_BNSTATS: [nslots][nb][2][N] fp64, accumulated with atomics
  // EPI_BNBWD (input-gradient GEMM): the tile it has just produced is the upstream gradient g of the BN (+ GELU) layer that
  // made this GEMM's input in the forward.  Its backward statistics  sum dz, sum dz * yhat  (dz = g * act'(a y + c),
  // yhat = (y - mean) * invstd) are accumulated here, from the accumulators and one read of y, instead of by a stand-alone
  // pass over g and y.  Output column n belongs to BN group n / pco, channel n % pco; y is (pnb, M, pco).
  const float* py; const float* pa; const float* pc; const float* pmean; const float* pinvstd;
  double* psums;  int pco, pact;                        // psums: [pnb][2][pco] fp64 (atomics)
  // split-K (ksplit > 1): workgroup (tile, ks) contracts K-steps [ks * kper, (ks + 1) * kper) and leaves its 128 x BN partial
  // in part[(z * tiles + tile) * ksplit + ks]; the LAST of a tile's ksplit workgroups to arrive (cnt[z * tiles + tile], reset
  // by it) adds the partials in split order — the same bits whoever arrives last — and runs the epilogue on the sum.
  int ksplit, kper;
  float* part;  unsigned* cnt;
  const float* add;                                     // X6_STORE: C = A B^T + add (same shape and pitch as C), or null
  // X6_STORE_NCHW: the tile goes out channel-major, C (M / nchw_n, nchw_c == N, nchw_n) — row m is token m % nchw_n of image
  // m / nchw_n — while `add` stays token-major (row pitch ldc).  nchw_n % 4 == 0 and M == images * nchw_n.
  int nchw_n, nchw_c;
  int walk_nb;                                          // gemm_x6_walk_kernel: the batches folded into its 1-D grid
};

__device__ __forceinline__ void x6_chan_merge(double& n, double& mean, double& m2, double nb, double mb, double m2b) {
  if (nb <= 0.0) return;
  const double tot = n + nb;
  const double delta = mb - mean;
  mean += delta * (nb / tot);
  m2 += m2b + delta * delta * (n * nb / tot);
  n = tot;
}

// LDS-DMA of one 1-KiB piece: 64 lanes x 16 B from (sbase + voff) to LDS bytes [lds_dst, lds_dst + 1024).  M0 carries the
// destination and is compiler-reserved: saved and restored inside the statement.  Invisible to the compiler's waitcnt
// bookkeeping — completion is counted by hand (s_waitcnt vmcnt(N)) before the barrier that precedes the reads.
__device__ __forceinline__ void x6_dma16(const void* sbase, unsigned voff, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds_dst) : "memory");
}

// BN: columns per tile — 32 NI, or 80 with NI = 3 (the last 32-column block is half used).  Every GKGNet width is a multiple of
// 80, so 80-column tiles cover 80 / 160 outputs with one / two workgroups per row block where 64-column tiles need two / three:
// at the short-K stage-1 / stage-2 shapes the launch time follows the number of requests (A is fetched once per column tile,
// B once per tile and K-step), not the arithmetic (profiles/r04_x6_one_vs_two_column_tiles.txt).
// The kernel's text is gkg_gemm_x6_tile.h, compiled in two forms: one tile per workgroup, and a static walk over several.
#define X6_WALK 0
#include "gkg_gemm_x6_tile.h"
#undef X6_WALK
#define X6_WALK 1
#include "gkg_gemm_x6_tile.h"
#undef X6_WALK

// The dynamic-LDS attribute of ONE kernel (the one about to be launched) and, where `slots` asks, its resident-workgroup count
// (workgroups per CU x CUs) are per DEVICE (a per-process guard left a second GPU of the same process without the attribute —
// ADVICE r3): set / queried on the first use there.  The only hipFuncSetAttribute of this file.
template <auto KERNEL>
static hipError_t x6_kernel_once(size_t sh, int* slots = nullptr) {
  static int known[64] = {};                             // 0: not set up; -1: attribute set; else the resident workgroups of the device
  int dev = 0;
  (void)hipGetDevice(&dev);
  const bool cached = dev >= 0 && dev < 64;
  int n = cached ? known[dev] : 0;
  if (n == 0) {
    hipError_t e = hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh);
    if (e != hipSuccess) return e;
    n = -1;
  }
  if (n < 0 && slots) {
    int per_cu = 0, cus = 0;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)KERNEL, 256, sh);
    if (e != hipSuccess) return e;
    e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return e;
    n = per_cu * cus;
    if (n < 8) return hipErrorInvalidConfiguration;
  }
  if (cached) known[dev] = n;
  if (slots) *slots = n;
  return hipSuccess;
}

// ---- few rows: the waves of a workgroup split K, not M (round 5) --------------------------------------------------------
// gemm_x6_kernel has a floor of ~10 us per launch whatever the size (2.4 us of prologue DMA issue for three 16 KB A stages and
// two B stages per workgroup, a barrier per K-step, a 128-row epilogue) and needed a cross-workgroup split-K seam (5-13 us) to
// fill the chip with the label branch's 2 560-row matrices: ten launches of 13-28 us per cfg2 step.  Here a workgroup owns
// 32 rows x 64 columns and its four waves take a QUARTER OF THE CONTRACTION each: every wave streams its own A rows through a
// private 3 x 4 KB LDS ring (LDS-DMA, as above), reads its B fragments straight from the weight planes (they are stored in
// MFMA operand order: one 16-byte load per lane and product, L2-resident, one K-step ahead in registers), and never meets
// another wave before the end — no barrier in the loop, no partial tiles through global memory.  The four 32 x 64 partials
// are added through LDS in wave order (deterministic), and the workgroup stores its tile (+ residual) and, EPI_BNSTATS, adds
// the tile's centred column statistics to the fp64 sums like the kernel above.  2 560 x 320 -> 320: 400 workgroups of
// 3 + 3 + 2 + 2 K-steps.
// MI — 32-row blocks per workgroup (and wave): 1 (default), or 2 (opt-in: 64-row tiles halve the plane traffic at one wave per
// SIMD and a 2-stage ring; measured no better, see the launch site).
template <int EPI, int MI>
__global__ __launch_bounds__(256, MI == 1 ? 2 : 1) void gemm_x6_ks_kernel(X6Args g) {
  constexpr int NI = 2, BN = 64, BM = 32 * MI, BK = 32, SA = MI == 1 ? 3 : 2, STAGE = 4096 * MI;
  extern __shared__ uint4 lds[];                       // [4 waves][SA][STAGE] A rings; then [4][BM][64] fp32 partials (aliased)
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int z = blockIdx.y;
  const int lin = blockIdx.x, xcd = lin & 7, slot = lin >> 3;
  const int tn = slot % g.ntiles, tm = (slot / g.ntiles) * 8 + xcd;      // the column tiles of a row block on one XCD
  if (tm >= g.mtiles) return;
  const int m0 = tm * BM, n0 = tn * BN;
  const int M = g.M, N = g.N, K = g.K;
  const int nk_total = (K + BK - 1) / BK;
  const int kbase = nk_total >> 2, krem = nk_total & 3;
  const int cnt = kbase + (w < krem ? 1 : 0);                            // this wave's K-steps
  const int kt0 = w * kbase + min(w, krem);
  const bool ktail = (K & (BK - 1)) != 0;
  const float* A = g.A + (size_t)z * g.a_bstride;
  const uint4* P = g.P + (size_t)z * g.p_bstride;
  const unsigned lds0 = (unsigned)(size_t)lds + w * (SA * STAGE);
  const char* ring = (const char*)lds + w * (SA * STAGE);

  // A pieces (as gemm_x6_kernel): LDS slot L = 64 i + lane of the BM x 128-B image holds chunk (L & 7) ^ ((row >> 1) & 7) of row L >> 3
  unsigned aoff[4 * MI];
  int achunk[4 * MI];
#pragma unroll
  for (int i = 0; i < 4 * MI; ++i) {
    const int L = 64 * i + lane, row = L >> 3, chunk = (L & 7) ^ ((row >> 1) & 7);
    const int gr = min(m0 + row, M - 1);
    aoff[i] = (unsigned)((size_t)gr * g.lda + chunk * 4) * 4u;
    achunk[i] = chunk;
  }
  auto dma_a = [&](int k) {                                              // k: this wave's step index
    const int kt = kt0 + k;
    const char* base = (const char*)A + (size_t)kt * (BK * 4);
    const unsigned dst = lds0 + (k % SA) * STAGE;
    const bool last = ktail && kt == nk_total - 1;
#pragma unroll
    for (int i = 0; i < 4 * MI; ++i) {
      unsigned o = aoff[i];
      if (last && kt * BK + achunk[i] * 4 >= K) o -= achunk[i] * 16;    // past K: a valid address, masked after the read
      x6_dma16(base, o, dst + i * 1024);
    }
  };
  const int r = lane & 31, h = lane >> 5, sw = (r >> 1) & 7;
  const size_t plane = (size_t)g.KC * g.NP;                              // uint4 units
  auto load_b = [&](uint4 (&b)[NI][3], int k, int s2) {                  // the 6 operand fragments of half s2 of K-step k
    const uint4* base = P + ((size_t)(kt0 + k) * 4 + h + 2 * s2) * g.NP + n0 + r;
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int p = 0; p < 3; ++p) b[j][p] = base[p * plane + j * 32];
  };
  x6_f32x16 acc[MI][NI], accs[MI][NI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int q = 0; q < 16; ++q) { acc[mi][j][q] = 0.f; accs[mi][j][q] = 0.f; }

  uint4 b0f[NI][3], b1f[NI][3], bn0[NI][3], bn1[NI][3];      // both halves of the current K-step and of the next one
  // issue order per wave: A0 A1 A2 B0.0 B0.1 | B(k+1).0 B(k+1).1 (wait A(k), B(k)) step k, A(k+3) | ...
  if (cnt > 0) dma_a(0);
  if (cnt > 1) dma_a(1);
  if (SA > 2 && cnt > 2) dma_a(2);
  if (cnt > 0) { load_b(b0f, 0, 0); load_b(b1f, 0, 1); }
  auto mma = [&](const char* ab, int s2, bool last, int kglob, const uint4 (&bq)[NI][3]) {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
      const char* rowp = ab + (32 * mi + r) * 128;
      const float4 f0 = *(const float4*)(rowp + (((4 * s2 + 2 * h) ^ sw) << 4));
      const float4 f1 = *(const float4*)(rowp + (((4 * s2 + 2 * h + 1) ^ sw) << 4));
      float f[8] = {f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w};
      if (last) {
        const int kb = kglob * BK + 16 * s2 + 8 * h;
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = kb + e < K ? f[e] : 0.f;
      }
      uint4 ah, am, al;
      x6_split2(f[0], f[1], ah.x, am.x, al.x); x6_split2(f[2], f[3], ah.y, am.y, al.y);
      x6_split2(f[4], f[5], ah.z, am.z, al.z); x6_split2(f[6], f[7], ah.w, am.w, al.w);
      const x6_bf16x8 a0 = __builtin_bit_cast(x6_bf16x8, ah), a1 = __builtin_bit_cast(x6_bf16x8, am), a2 = __builtin_bit_cast(x6_bf16x8, al);
#pragma unroll
      for (int j = 0; j < NI; ++j) {
        const x6_bf16x8 b0 = __builtin_bit_cast(x6_bf16x8, bq[j][0]), b1 = __builtin_bit_cast(x6_bf16x8, bq[j][1]),
                        b2 = __builtin_bit_cast(x6_bf16x8, bq[j][2]);
        // small terms first, the hi*hi product into its own accumulator (gemm_x6_kernel's order)
        accs[mi][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, b0, accs[mi][j], 0, 0, 0);
        accs[mi][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b2, accs[mi][j], 0, 0, 0);
        accs[mi][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, accs[mi][j], 0, 0, 0);
        accs[mi][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, accs[mi][j], 0, 0, 0);
        accs[mi][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, accs[mi][j], 0, 0, 0);
        acc[mi][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc[mi][j], 0, 0, 0);
      }
    }
  };
  for (int k = 0; k < cnt; ++k) {
    const bool more = k + 1 < cnt;
    if (more) { load_b(bn0, k + 1, 0); load_b(bn1, k + 1, 1); }
    // A(k) and both halves of B(k) have landed once at most the operations issued AFTER B(k).1 are outstanding: A(k - 1 + SA)
    // (issued at the end of step k-1; k == 0: the prologue's A pieces are OLDER than B0) and the 12 loads just issued.  (The
    // compiler's own waits cover the plain loads it can see; this asm wait is for the LDS-DMA pieces it cannot.)
    const int after = (more ? 12 : 0) + ((k >= 1 && k - 1 + SA < cnt) ? 4 * MI : 0);
    if (after == 12 + 4 * MI) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(12 + 4 * MI) : "memory");
    else if (after == 12) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
    else if (after == 4 * MI) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(4 * MI) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const char* ab = ring + (k % SA) * STAGE;
    const bool last = ktail && kt0 + k == nk_total - 1;
    mma(ab, 0, last, kt0 + k, b0f);
    mma(ab, 1, last, kt0 + k, b1f);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                   // the ring slot's reads are in registers: it may be refilled
    if (more) {
      // the copies first (their wait sees only this step's loads, a whole step old), then the DMA: behind it the compiler's count
      // of outstanding loads would be short by the DMA pieces
#pragma unroll
      for (int j = 0; j < NI; ++j)
#pragma unroll
        for (int p = 0; p < 3; ++p) { b0f[j][p] = bn0[j][p]; b1f[j][p] = bn1[j][p]; }
    }
    asm volatile("" ::: "memory");
    if (k + SA < cnt) dma_a(k + SA);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();                                                       // every wave is done with its ring
  float* red = reinterpret_cast<float*>(lds);                            // [4][BM][64]
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int row = 32 * mi + (q & 3) + 8 * (q >> 2) + 4 * h;
        red[(w * BM + row) * BN + j * 32 + r] = acc[mi][j][q] + accs[mi][j][q];
      }
  // X6_BNBWD (see X6Args): thread tid sums column tid & 63 over rows (tid >> 6) + 4 u below; the producer's y values at those
  // places are fetched ahead of the barrier, so that their latency overlaps the other waves' arrival
  float yv[EPI == X6_BNBWD ? 8 * MI : 1];
  float pav = 0.f, pcv = 0.f, pmv = 0.f, piv = 0.f, s0 = 0.f, s1 = 0.f;
  if constexpr (EPI == X6_BNBWD) {
    const int n = n0 + (tid & 63);
#pragma unroll
    for (int u = 0; u < 8 * MI; ++u) yv[u] = 0.f;
    if (n < N) {
      const int pq = n / g.pco, pi = n - pq * g.pco;
      pav = g.pa[n]; pcv = g.pc[n]; pmv = g.pmean[n]; piv = g.pinvstd[n];
      const float* yp = g.py + ((size_t)pq * M + m0 + (tid >> 6)) * (size_t)g.pco + pi;
#pragma unroll
      for (int u = 0; u < 8 * MI; ++u)
        if (m0 + (tid >> 6) + 4 * u < M) yv[u] = yp[(size_t)(4 * u) * g.pco];
    }
  }
  __syncthreads();
  float* C = g.C + (size_t)z * g.c_bstride;
  float v[8 * MI];
#pragma unroll
  for (int u = 0; u < 8 * MI; ++u) {
    const int e = tid + 256 * u, row = e >> 6, col = e & 63;
    v[u] = ((red[e] + red[BM * BN + e]) + red[2 * BM * BN + e]) + red[3 * BM * BN + e];      // wave order: the same bits every run
    const int m = m0 + row, n = n0 + col;
    if (m < M && n < N) {
      float o = v[u];
      if ((EPI == X6_STORE || EPI == X6_BNBWD) && g.add) o += g.add[(size_t)z * g.c_bstride + (size_t)m * g.ldc + n];
      C[(size_t)m * g.ldc + n] = o;
      if constexpr (EPI == X6_BNBWD) {                 // the BN's upstream gradient is the stored value, residual included
        float dz = o;
        if (g.pact == 1) dz *= gelu_grad_f(__builtin_fmaf(pav, yv[u], pcv));
        s0 += dz;
        s1 += dz * ((yv[u] - pmv) * piv);
      }
    }
  }
  if constexpr (EPI == X6_BNBWD) {
    // the four waves' partial column sums (8 rows each) meet in LDS and are added in fp64: ONE atomic pair per column and
    // workgroup, like the statistics below
    __syncthreads();                                   // every thread has read its partials
    red[((tid >> 6) * BN + (tid & 63)) * 2] = s0;
    red[((tid >> 6) * BN + (tid & 63)) * 2 + 1] = s1;
    __syncthreads();
    if (tid < BN && n0 + tid < N) {
      double t0 = 0.0, t1 = 0.0;
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) { t0 += (double)red[(rg * BN + tid) * 2]; t1 += (double)red[(rg * BN + tid) * 2 + 1]; }
      const int n = n0 + tid, pq = n / g.pco, pi = n - pq * g.pco;
      double* sz = g.psums + (size_t)pq * 2 * g.pco + pi;
      __hip_atomic_fetch_add(sz, t0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_add(sz + g.pco, t1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return;
  }
  if (EPI != X6_BNSTATS) return;
  // train-mode BN statistics of the tile's columns: the summed tile back into LDS, one thread per column takes the centred
  // (mean, M2) over the tile's valid rows, ONE fp64 atomic pair per column and tile:  S += n mean,  Q += M2 + n mean^2
  __syncthreads();
#pragma unroll
  for (int u = 0; u < 8 * MI; ++u) red[tid + 256 * u] = v[u];
  __syncthreads();
  if (tid < BN && n0 + tid < N) {
    const int rows = max(0, min(BM, M - m0));
    float sum = 0.f;
    for (int row = 0; row < rows; ++row) sum += red[row * BN + tid];
    const float mean = rows > 0 ? sum / (float)rows : 0.f;
    float m2 = 0.f;
    for (int row = 0; row < rows; ++row) { const float d = red[row * BN + tid] - mean; m2 += d * d; }
    const double nd = (double)rows, md = (double)mean;
    double* sz = g.sums + ((size_t)(tm % g.nslots) * g.nbatch + z) * 2 * N + n0 + tid;
    __hip_atomic_fetch_add(sz, nd * md, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(sz + N, (double)m2 + nd * md * md, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---- the launch: what the plan (gkg_x6_plan.h) names, nothing decided here ----------------------------------------------
template <auto KERNEL>
static hipError_t x6_go(const X6GemmPlan& pl, const X6Args& a, hipStream_t st, bool attr = true) {
  if (attr) {
    if (hipError_t e = x6_kernel_once<KERNEL>(pl.lds); e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(KERNEL, dim3(pl.grid_x, pl.grid_y), dim3(256), pl.lds, st, a);
  return hipGetLastError();
}

// Where the plan says that the device's resident-workgroup count decides (X6GemmPlan::walkable): ask about the walk instantiation
// of this epilogue — the kernel the launch would be, with the LDS the plan names for it (walk_lds) — and plan again.  The
// instantiation is the switchboard's X6_BODY_WALK entry: the ladder's walk rung is NI = 2, BN = 64 and nothing else.
template <int EPI>
static hipError_t x6_plan_walk(X6GemmCall& q, X6GemmPlan& pl) {
  if constexpr (EPI != X6_BNBWD) {
    if (pl.walkable && q.slots <= 0) {
      hipError_t e = x6_kernel_once<gemm_x6_walk_kernel<2, EPI, 64>>(pl.walk_lds, &q.slots);
      if (e != hipSuccess) return e;
      x6_gemm_ladder(q, &pl);
    }
  }
  return hipSuccess;
}

// The operand-independent half of a call, the operands and the size-dependent half of the kernel arguments, each filled in ONE place.
static X6GemmCall x6_call(X6Role role, int M, int N, int K, int nb, const float* A, int lda, size_t a_bstride, const void* sk_ws,
                          size_t sk_bytes, unsigned flags) {
  X6GemmCall q{};
  q.role = role; q.M = M; q.N = N; q.K = K; q.nb = nb;
  q.lda = lda; q.a_bstride = a_bstride; q.a_aligned = ((size_t)A & 15) == 0;
  q.has_ws = sk_ws != nullptr; q.ws_aligned = ((size_t)sk_ws & 15) == 0; q.ws_bytes = sk_bytes;
  q.flags = flags;
  return q;
}

static X6Args x6_operands(const float* A, const void* planes, float* C, size_t c_bstride, int ldc, const float* add = nullptr) {
  X6Args a{};
  a.A = A; a.P = (const uint4*)planes; a.C = C; a.c_bstride = c_bstride; a.ldc = ldc; a.add = add;
  return a;
}

static void x6_sizes(X6Args& a, const X6GemmCall& q, const X6GemmPlan& pl, void* sk_ws) {
  a.a_bstride = q.a_bstride; a.lda = q.lda;
  a.p_bstride = pl.p_bstride; a.NP = pl.NP; a.KC = pl.KC;
  a.M = q.M; a.N = q.N; a.K = q.K;
  a.mtiles = pl.mtiles; a.ntiles = pl.ntiles; a.ksplit = pl.ksplit; a.kper = pl.kper;
  if (pl.ksplit > 1) {                                   // the split-K workspace: [tile counters][partials] (the plan checked its size)
    a.cnt = reinterpret_cast<unsigned*>(sk_ws);
    a.part = reinterpret_cast<float*>(reinterpret_cast<char*>(sk_ws) + X6_SK_CNT_BYTES);
  }
  a.nslots = pl.nslots; a.nbatch = q.nb;
  a.walk_nb = pl.body == X6_BODY_WALK ? q.nb : 0;
}

// (body, NI, BN, EPI, walk) -> instantiation; a combination the library does not hold is hipErrorInvalidValue.  80-column tiles
// exist for the plain and the BN-statistics epilogue, the walk form not for X6_BNBWD, the short-matrix body (48 KiB: no attribute)
// not with the channel-major store.  `a` arrives with the operands and leaves with the plan's sizes.
template <int EPI>
static hipError_t x6_launch(X6GemmCall& q, X6GemmPlan& pl, X6Args a, void* sk_ws, hipStream_t st) {
  GkgProfScope prof(GKG_PROF_GEMM_X6, st, pl.work);
  if (pl.epi != EPI) return hipErrorInvalidValue;
  if (hipError_t e = x6_plan_walk<EPI>(q, pl); e != hipSuccess) return e;
  x6_sizes(a, q, pl, sk_ws);
  if (pl.body == X6_BODY_KS) {
    if constexpr (EPI != X6_STORE_NCHW) return x6_go<gemm_x6_ks_kernel<EPI, 1>>(pl, a, st, false);
  } else if (pl.body == X6_BODY_TILE && pl.NI == 2 && pl.BN == 64) {
    return x6_go<gemm_x6_kernel<2, EPI, 64>>(pl, a, st);
  } else if (pl.body == X6_BODY_TILE && pl.NI == 3 && pl.BN == 80) {
    if constexpr (EPI == X6_STORE || EPI == X6_BNSTATS) return x6_go<gemm_x6_kernel<3, EPI, 80>>(pl, a, st);
  } else if (pl.body == X6_BODY_TILE && pl.NI == 1 && pl.BN == 32) {
    return x6_go<gemm_x6_kernel<1, EPI, 32>>(pl, a, st);
  } else if (pl.body == X6_BODY_WALK && pl.NI == 2 && pl.BN == 64) {
    if constexpr (EPI != X6_BNBWD) return x6_go<gemm_x6_walk_kernel<2, EPI, 64>>(pl, a, st);
  }
  return hipErrorInvalidValue;
}

// ---- weight gradient ----------------------------------------------------------------------------------------------------
// dW[m][n] = sum_k dY[k][m] X[k][n]: the contraction runs over the token axis, so BOTH operands are activations (split in
// registers) and both are "k-strided" for the matrix core, whose operand lane (r, h) wants 8 consecutive k of ONE column.
// Here that is 8 dword loads of 8 consecutive rows at a fixed column — lanes r = consecutive columns, so every load
// instruction is two fully used 128-B row segments — straight from global/L2 into registers: no LDS, no barriers, each
// wave streams its own K range.  A workgroup = one 64 x 64 tile of dW x one slab of rows; its 4 waves take a quarter of
// the slab each (2 x 2 blocks of 32 x 32 per wave: 24 MFMAs per 16 rows), add their tiles through LDS and issue ONE set of
// fp32 atomics into the pre-zeroed dW (summation order over slabs is run-dependent, like the vendor library's split-K).
// Loads run three 16-row steps ahead in a 3-deep register ring; the 176-instruction split of the next step's four
// fragments sits in the MFMA gaps (7-8 per gap; the compiled loop, counted by tools/count_loop_insts.py, holds 417 vector and
// 263 scalar instructions per 48 MFMAs — 8.7 / MFMA, most of the rest address and bounds arithmetic of the 32 loads: it is
// address-bound, and for the long-K, small-output shapes it exists for it is the HBM stream that sets the time).  The three
// kernels of this section share ONE definition of the split sequence (x6w_op).
struct X6WgradArgs {
  const float* A;  size_t a_bstride;  int lda;       // dY (nb, K, M)
  const float* B;  size_t b_bstride;  int ldb;       // X  (nb, K, N)
  float* C;  size_t c_bstride;  int ldc;             // dW (nb, M, N), zero on entry
  int M, N, K;
  int mtiles, ntiles, splits, rows_per_split;        // rows_per_split % 128 == 0
  int swap;                                          // wide kernel: A / B roles exchanged, C written transposed
  int share, rot;                                    // workgroup -> (slab, tile) map of batched launches (x6w_map); 0, 0 otherwise
  int ubase, urem;                                   // LDS-DMA kernels: slab s = ubase + (s < urem) units of 128 rows (K = 128 * units)
  int kperm;                                         // X arrives as [x chunk | m chunk] (X6PrepDesc::kperm): operand column j of X is
                                                     // dW column x6_kperm_src(j, cin) — applied where the tile is added to dW
};

typedef unsigned x6_u32x4 __attribute__((ext_vector_type(4)));
typedef float x6_f32x2 __attribute__((ext_vector_type(2)));
typedef x6_u32x4 X6WFrag[4][3];               // [A0, A1, B0, B1][hi, mid, lo]: 4 packed bf16 pairs = one MFMA operand each
typedef x6_u32x4 X6WFragW[6][3];              // wide form: [A0, A1, B0, B1, B2, B3][hi, mid, lo]

__device__ __forceinline__ x6_bf16x8 x6w_operand(const x6_u32x4& f) { return __builtin_bit_cast(x6_bf16x8, f); }
// step I (0 .. 44 NB - 1) of the split of NB raw fragments into `fn`: block I / 44, and within a block the four pairs
// interleaved (4 independent chains).  Single-instruction asm volatile: fixed order, not sunk, not SLP-packed.  ONE definition
// for the register-load kernel (NB = 4), the 64 x 64 LDS-DMA body (NB = 4) and the wide body (NB = 6).
// The two residual subtractions of a pair stay two v_sub_f32: one v_pk_add_f32 on a register pair is 9 instructions per pair
// instead of 11, but beside MFMAs the packed instruction costs more than the two it replaces (tools/ubench/mfma_bf16_fill,
// ksplit: 28.4 against 23.1 ns per MFMA slot for this very stream; EXPERIMENTS.md).
// LDSW (the LDS-DMA bodies): the fragments were read by x6w_readblk — 4 ds_read2 per block, in block order, which the compiler's
// waitcnt bookkeeping does not see — so the first step of block b waits until at most the 4 (NB - 1 - b) reads of the later
// blocks are outstanding (LDS reads return in order; 15 is the counter's largest operand, a smaller one only waits longer).
template <int I, int NB, bool LDSW>
__device__ __forceinline__ void x6w_op(float (&raw)[NB][8], x6_u32x4 (&fn)[NB][3], unsigned (&t0)[4], unsigned (&t1)[4]) {
  constexpr int blk = I / 44, u = I % 44, p = u & 3, o = u >> 2;
  float& x0 = raw[blk][2 * p]; float& x1 = raw[blk][2 * p + 1];
  unsigned w;
  if constexpr (LDSW && u == 0) {
    constexpr int left = 4 * (NB - 1 - blk);
    asm volatile("s_waitcnt lgkmcnt(%0)" :: "n"(left < 15 ? left : 15) : "memory");
  }
  if constexpr (o == 0) { asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(w) : "v"(x0), "v"(x1)); fn[blk][0][p] = w; }
  if constexpr (o == 1) asm volatile("v_lshlrev_b32 %0, 16, %1" : "=v"(t0[p]) : "v"(fn[blk][0][p]));
  if constexpr (o == 2) asm volatile("v_and_b32 %0, 0xffff0000, %1" : "=v"(t1[p]) : "v"(fn[blk][0][p]));
  if constexpr (o == 3) asm volatile("v_sub_f32 %0, %0, %1" : "+v"(x0) : "v"(t0[p]));
  if constexpr (o == 4) asm volatile("v_sub_f32 %0, %0, %1" : "+v"(x1) : "v"(t1[p]));
  if constexpr (o == 5) { asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(w) : "v"(x0), "v"(x1)); fn[blk][1][p] = w; }
  if constexpr (o == 6) asm volatile("v_lshlrev_b32 %0, 16, %1" : "=v"(t0[p]) : "v"(fn[blk][1][p]));
  if constexpr (o == 7) asm volatile("v_and_b32 %0, 0xffff0000, %1" : "=v"(t1[p]) : "v"(fn[blk][1][p]));
  if constexpr (o == 8) asm volatile("v_sub_f32 %0, %0, %1" : "+v"(x0) : "v"(t0[p]));
  if constexpr (o == 9) asm volatile("v_sub_f32 %0, %0, %1" : "+v"(x1) : "v"(t1[p]));
  if constexpr (o == 10) { asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(w) : "v"(x0), "v"(x1)); fn[blk][2][p] = w; }
}
template <int I, int END, bool LDSW = false, int NB>
__device__ __forceinline__ void x6w_ops(float (&raw)[NB][8], x6_u32x4 (&fn)[NB][3], unsigned (&t0)[4], unsigned (&t1)[4]) {
  if constexpr (I < END && I < 44 * NB) { x6w_op<I, NB, LDSW>(raw, fn, t0, t1); x6w_ops<I + 1, END, LDSW>(raw, fn, t0, t1); }
}
// MFMA slot SI (0..23) of a 16-row step: block (i, j) = SI / 6, product t = SI % 6; then 8 split steps in its shadow
template <int SI, bool SPLIT, bool LDSW = false>
__device__ __forceinline__ void x6w_slots(const X6WFrag& fc, X6WFrag& fn, x6_f32x16 (&acc)[2][2], x6_f32x16 (&accs)[2][2],
                                          float (&raw)[4][8], unsigned (&t0)[4], unsigned (&t1)[4]) {
  if constexpr (SI < 24) {
    constexpr int i = SI / 12, j = (SI / 6) & 1, t = SI % 6;
    constexpr int pa = t == 0 ? 2 : (t == 2 || t == 3) ? 1 : 0;         // small terms first, hi*hi last into its own accumulator
    constexpr int pb = t == 1 ? 2 : (t == 2 || t == 4) ? 1 : 0;
    if constexpr (t < 5) accs[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x6w_operand(fc[i][pa]), x6w_operand(fc[2 + j][pb]), accs[i][j], 0, 0, 0);
    else acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x6w_operand(fc[i][0]), x6w_operand(fc[2 + j][0]), acc[i][j], 0, 0, 0);
    if constexpr (SPLIT) x6w_ops<SI * 8, SI * 8 + 8, LDSW>(raw, fn, t0, t1);
    __builtin_amdgcn_sched_barrier(0);
    x6w_slots<SI + 1, SPLIT, LDSW>(fc, fn, acc, accs, raw, t0, t1);
  }
}

// DET (all three bodies): the workgroup STORES its tile of slab `split` into image `split` of a workspace (g.C: image 0 of this
// launch, `sstride` floats per image of nb x M x N elements, laid out like dW) instead of adding it to dW — the deterministic
// entry points (gkg_linear_wgrad_x6_det), whose ordered reduction (wgrad_x6_det_reduce_kernel) then writes dW.  Same
// decomposition and arithmetic up to that store; the atomic forms are the kernels they were before the deterministic ones came.
// The register-load kernel's text is gkg_wgrad_x6_rows.h, compiled in both forms (as a template body called from two kernels
// the atomic form came out with 16 more VGPRs); the two LDS-DMA bodies are templates.
#define X6W_DET 0
#include "gkg_wgrad_x6_rows.h"
#undef X6W_DET
#define X6W_DET 1
#include "gkg_wgrad_x6_rows.h"
#undef X6W_DET

// The same workgroup / wave decomposition with the rows staged through LDS: each wave copies the next 16 rows of its own K
// range (64 columns of dY, 64 of X: 8 KiB) global -> a private 4-stage LDS ring by LDS-DMA — eight 16-byte-per-lane
// instructions per step where the register form above needs 32 dword loads (16 address cycles per 256 B each: measured
// texture-address-bound) — and reads the column fragments back with ds_read_b32.  No barriers: a wave only ever reads what
// it copied itself.  Requires every row of the launch to be inside the tensor (the host gives the ragged remainder to the
// register-load kernel) and 16-byte aligned rows; columns past M / N are DMA'd from a clamped address and never read: their
// lanes read a zero-filled region instead (below).  Step s issues the DMA of step s + 4, waits until step s + 2 has landed
// (counted vmcnt) and reads it.  Compiled loop (two steps, tools/count_loop_insts.py): 48 MFMAs, 370 vector instructions
// (7.7 / MFMA, 7.33 of them the split), 57 scalar; edge and interior tiles run the same instructions.
// (split, tile) of workgroup `lin` of a weight-gradient launch.  Default map: slab s runs with ALL its tiles on XCD s % 8 (lin & 7
// is the XCD the hardware dispatches workgroup lin to).  g.share = t > 1 (batched launches of few-slab problems, splits * t == 8):
// t XCDs share a slab and take every t-th tile of it each, so that a problem of 1 / 2 / 4 slabs still spreads over all 8 XCDs
// with no idle workgroup ids.  `rot` rotates the XCD assignment (batched launches: consecutive problems start on different XCDs).
__device__ __forceinline__ bool x6w_map(const X6WgradArgs& g, int lin, int& split, int& tile) {
  const int ntile = g.mtiles * g.ntiles;
  const int xcd = (lin + g.rot) & 7, slot = lin >> 3;
  if (g.share > 1) {
    split = xcd / g.share;
    tile = slot * g.share + xcd % g.share;
    return split < g.splits && tile < ntile;
  }
  split = (slot / ntile) * 8 + xcd;
  tile = slot % ntile;
  return split < g.splits;
}

// Beside the rings lies a zero-filled region of X6W_ZERO_BYTES, cleared once per workgroup: a lane whose column lies outside
// the matrix reads its fragments THERE (its read base is chosen per step from a per-lane mask, one select per block) instead
// of reading the clamped column's values and zeroing them after every LDS read (8 selects per block).  Exactly 0.0f, as before.
// The region covers the eight row offsets of a fragment at the 128-column pitch: 7 x 512 + 4 bytes.

// LDS-DMA of four consecutive 1-KiB pieces (x6_dma16) in one statement: M0 is saved and restored once and stepped by 1 KiB
// between the pieces — 14 instructions where four x6_dma16 are 24.
__device__ __forceinline__ void x6w_dma4(const void* sbase, unsigned v0, unsigned v1, unsigned v2, unsigned v3, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %6\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %5\n\t"
               "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %5\n\t"
               "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %3, %5\n\t"
               "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %4, %5\n\t"
               "s_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(v0), "v"(v1), "v"(v2), "v"(v3), "s"(sbase), "s"(lds_dst) : "memory", "scc");
}
// One fragment block: rows 0 .. 7 of one column from LDS byte address `addr`, row pitch 64 PB floats, as four ds_read2st64_b32
// (rows 2p and 2p + 1 in one instruction, address + immediate: no per-row address arithmetic).  Asynchronous and unknown to
// the compiler's waitcnt bookkeeping: the split steps wait (x6w_op, LDSW).
template <int PB>
__device__ __forceinline__ void x6w_readblk(float (&f)[8], unsigned addr) {
  x6_f32x2 v0, v1, v2, v3;
  asm volatile("ds_read2st64_b32 %0, %1 offset0:%2 offset1:%3" : "=v"(v0) : "v"(addr), "n"(0), "n"(PB) : "memory");
  asm volatile("ds_read2st64_b32 %0, %1 offset0:%2 offset1:%3" : "=v"(v1) : "v"(addr), "n"(2 * PB), "n"(3 * PB) : "memory");
  asm volatile("ds_read2st64_b32 %0, %1 offset0:%2 offset1:%3" : "=v"(v2) : "v"(addr), "n"(4 * PB), "n"(5 * PB) : "memory");
  asm volatile("ds_read2st64_b32 %0, %1 offset0:%2 offset1:%3" : "=v"(v3) : "v"(addr), "n"(6 * PB), "n"(7 * PB) : "memory");
  f[0] = v0.x; f[1] = v0.y; f[2] = v1.x; f[3] = v1.y; f[4] = v2.x; f[5] = v2.y; f[6] = v3.x; f[7] = v3.y;
}
// the workgroup clears the zero region (256 threads x 16 bytes); the caller's barrier orders it before the first fragment read
__device__ __forceinline__ void x6w_clear_zero(float* wlds, unsigned ring_bytes, int tid) {
  static_assert(X6W_ZERO_BYTES == 256 * 16, "one 16-byte store per thread");
  reinterpret_cast<float4*>(wlds + ring_bytes / 4)[tid] = float4{0.f, 0.f, 0.f, 0.f};
}

template <bool DET>
__device__ __forceinline__ void wgrad_x6_dma_body(const X6WgradArgs& g, const int lin, const int z, const size_t sstride) {
  extern __shared__ float wlds[];               // [4 waves][4 stages][2 operands][16 rows][64 cols], then reused for the reduce
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  int split, tile;
  if (!x6w_map(g, lin, split, tile)) return;
  const int m0 = (tile / g.ntiles) * 64, n0 = (tile % g.ntiles) * 64;
  const int r = lane & 31, h = lane >> 5;
  // the last slab may be shorter (whole 128-row units: 4 waves x 2 steps x 16 rows)
  // balanced slabs of whole 128-row units: the first g.urem slabs hold one unit more (a fixed slab length left the last slab
  // — and, with slab s on XCD s % 8, one XCD — with as little as a third of the others' rows)
  const long long slab0 = 128ll * ((long long)split * g.ubase + min(split, g.urem));
  const int rows_here = 128 * (g.ubase + (split < g.urem ? 1 : 0));
  const int rows_per_wave = rows_here >> 2;
  const long long k_begin = slab0 + (long long)w * rows_per_wave;
  const int T = rows_per_wave >> 4;
  const char* Az = (const char*)(g.A + (size_t)z * g.a_bstride);
  const char* Bz = (const char*)(g.B + (size_t)z * g.b_bstride);
  constexpr unsigned RING_BYTES = 4 * 4 * 8192;
  const unsigned lds_base = (unsigned)(size_t)wlds;
  const unsigned lds0 = lds_base + w * (4 * 8192), lds_end = lds0 + 4 * 8192, lds_zero = lds_base + RING_BYTES;
  x6w_clear_zero(wlds, RING_BYTES, tid);

  // DMA piece p (4 per operand): rows 4p .. 4p+3; lane -> row 4p + (lane >> 4), 16-byte column chunk lane & 15.  The per-piece
  // offsets are formed once; a step advances the two row bases and the destination stage
  const int prow = lane >> 4, pch = lane & 15;
  const int ca = min(m0 + 4 * pch, g.M - 4), cb = min(n0 + 4 * pch, g.N - 4);      // clamped: such columns are never read
  const unsigned dA = (unsigned)(((size_t)prow * g.lda + ca) * 4), dB = (unsigned)(((size_t)prow * g.ldb + cb) * 4);
  const unsigned strideA = (unsigned)g.lda * 16u, strideB = (unsigned)g.ldb * 16u;            // 4 rows, bytes
  unsigned va[4], vb[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) { va[p] = dA + p * strideA; vb[p] = dB + p * strideB; }
  const char* arow = Az + k_begin * g.lda * 4;                                                // step 0's 16 rows
  const char* brow = Bz + k_begin * g.ldb * 4;
  const size_t stepA = (size_t)g.lda * 64, stepB = (size_t)g.ldb * 64;                        // 16 rows, bytes
  unsigned wr = lds0;                                                                         // stage the next DMA step fills
  auto dma = [&]() __attribute__((always_inline)) {
    x6w_dma4(arow, va[0], va[1], va[2], va[3], wr);
    x6w_dma4(brow, vb[0], vb[1], vb[2], vb[3], wr + 4096);
    arow += stepA; brow += stepB;
    wr += 8192;
    if (wr == lds_end) wr = lds0;
  };
  // fragment (block i of operand o) of a stage: lane (r, h) reads rows 8h .. 8h+7 at column 32 i + r — or the zero region
  const bool ok[4] = {m0 + r < g.M, m0 + 32 + r < g.M, n0 + r < g.N, n0 + 32 + r < g.N};
  unsigned lo[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) lo[q] = (unsigned)(((q >> 1) * 1024 + (8 * h) * 64 + 32 * (q & 1) + r) * 4);
  unsigned rd = lds0;                                                                         // stage the next read step reads
  auto readfr = [&](float (&raw)[4][8]) __attribute__((always_inline)) {
#pragma unroll
    for (int q = 0; q < 4; ++q) x6w_readblk<1>(raw[q], ok[q] ? rd + lo[q] : lds_zero);
    rd += 8192;
    if (rd == lds_end) rd = lds0;
  };
  float raw0[4][8], raw1[4][8];
  X6WFrag fr0, fr1;
  unsigned t0[4], t1[4];
  x6_f32x16 acc[2][2], accs[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int q = 0; q < 16; ++q) { acc[i][j][q] = 0.f; accs[i][j][q] = 0.f; }

  // prologue: DMA steps 0..3; read steps 0 and 1; split step 0
  dma();
  if (T > 1) dma();
  if (T > 2) dma();
  if (T > 3) dma();
  __syncthreads();                              // the zero region is cleared
  if (T > 3) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  readfr(raw0);
  if (T > 1) readfr(raw1);
  x6w_ops<0, 176, true>(raw0, fr0, t0, t1);
  // step s (fr[s&1]): splits raw[(s+1)&1] (step s+1); then DMA step s+4, wait for step s+2, read it into raw[s&1]
  auto tailwork = [&](float (&rawn)[4][8], int s) __attribute__((always_inline)) {
    if (s + 4 < T) dma();
    if (s + 2 < T) {
      if (s + 4 < T) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");       // steps s+3, s+4 may stay in flight
      else if (s + 3 < T) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      readfr(rawn);
    }
  };
  for (int s = 0; s + 2 < T; s += 2) {
    x6w_slots<0, true, true>(fr0, fr1, acc, accs, raw1, t0, t1);     // step s: splits step s+1 (raw1) into fr1
    tailwork(raw0, s);                                                  // raw0 <- step s+2
    x6w_slots<0, true, true>(fr1, fr0, acc, accs, raw0, t0, t1);     // step s+1: splits step s+2 (raw0) into fr0
    tailwork(raw1, s + 1);                                              // raw1 <- step s+3
  }
  x6w_slots<0, true, true>(fr0, fr1, acc, accs, raw1, t0, t1);
  x6w_slots<0, false>(fr1, fr0, acc, accs, raw0, t0, t1);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  __syncthreads();                              // every wave is done with its ring: reuse the LDS for the reduction
  float* red = wlds;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int row = 32 * i + (q & 3) + 8 * (q >> 2) + 4 * h, col = 32 * j + r;
        red[w * 4096 + row * 64 + col] = acc[i][j][q] + accs[i][j][q];
      }
  __syncthreads();
  float* C = g.C + (size_t)z * g.c_bstride;
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const int e = tid + 256 * u, row = e >> 6, col = e & 63;
    const float v = (red[e] + red[4096 + e]) + (red[8192 + e] + red[12288 + e]);
    if (m0 + row < g.M && n0 + col < g.N) {
      float* dst = C + (size_t)(m0 + row) * g.ldc + (g.kperm ? x6_kperm_src(n0 + col, g.N) : n0 + col);
      if constexpr (DET) dst[(size_t)split * sstride] = v;
      else __hip_atomic_fetch_add(dst, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

__global__ __launch_bounds__(256) void wgrad_x6_dma_kernel(X6WgradArgs g) { wgrad_x6_dma_body<false>(g, blockIdx.x, blockIdx.y, 0); }
__global__ __launch_bounds__(256) void wgrad_x6_dma_det_kernel(X6WgradArgs g, size_t sstride) { wgrad_x6_dma_body<true>(g, blockIdx.x, blockIdx.y, sstride); }

// ---- wide form: 64 x 128 output tile per workgroup --------------------------------------------------------------------
// Same decomposition (a workgroup = one tile of dW x one slab of rows, its 4 waves a quarter of the slab each, private LDS
// rings filled by DMA, no barriers in the loop), but a wave owns 2 x 4 blocks of 32 x 32: six fragments per 16-row step feed
// 48 MFMAs, so the split is 264 / 48 = 5.5 vector instructions per MFMA where the 64 x 64 form needs 176 / 24 = 7.33.  The
// compiled loop (two steps, tools/count_loop_insts.py) holds 96 MFMAs, 554 vector instructions (5.77 / MFMA: the split, and
// per step six read-base additions and six selects) and 61 scalar, the same in edge and interior tiles; about 5 vector
// instructions hide in a bf16 MFMA's shadow (tools/ubench/mfma_bf16_fill), so this loop is still paced by the split.  The
// products are issued product-major over the eight accumulators (a dependent MFMA is 8 slots away), small terms first, all
// into ONE accumulator per block: 128 accumulator registers + 2 x 48 raw + 2 x 72 split fragments fit the 512 of a
// one-wave-per-SIMD kernel.  Ring: 3 stages x (16 x 64 of dY | 16 x 128 of X) x 4 B = 36 KiB per wave, 144 KiB per workgroup;
// step s issues the DMA of step s + 3 into the stage whose rows were read two steps ago, waits (counted vmcnt) for step
// s + 2 and reads its fragments, which are split during step s + 1.  The fragment reads are written out (x6w_readblk) and
// waited for inside the split (x6w_op, LDSW); a step's twelve DMA pieces are three statements (x6w_dma4).

// MFMA slot SI (0..47) of a 16-row step: product t = SI / 8 (small terms first, hi x hi last), block (i, j) = SI % 8;
// then its share (5 or 6) of the next step's 264 split instructions
template <int SI, bool SPLIT>
__device__ __forceinline__ void x6ww_slots(const X6WFragW& fc, X6WFragW& fn, x6_f32x16 (&acc)[2][4], float (&raw)[6][8],
                                           unsigned (&t0)[4], unsigned (&t1)[4]) {
  if constexpr (SI < 48) {
    constexpr int t = SI / 8, i = (SI % 8) / 4, j = SI % 4;
    constexpr int pa = t == 0 ? 2 : (t == 2 || t == 3) ? 1 : 0;
    constexpr int pb = t == 1 ? 2 : (t == 2 || t == 4) ? 1 : 0;
    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x6w_operand(fc[i][pa]), x6w_operand(fc[2 + j][pb]), acc[i][j], 0, 0, 0);
    if constexpr (SPLIT) x6w_ops<(SI * 11) / 2, ((SI + 1) * 11) / 2, true>(raw, fn, t0, t1);
    __builtin_amdgcn_sched_barrier(0);
    x6ww_slots<SI + 1, SPLIT>(fc, fn, acc, raw, t0, t1);
  }
}

template <bool DET>
__device__ __forceinline__ void wgrad_x6_wide_body(const X6WgradArgs& g, const int lin, const int z, const size_t sstride) {
  extern __shared__ float wlds[];               // [4 waves][3 stages][16 x 64 | 16 x 128], then reused for the reduce
  constexpr int STAGE_BYTES = 16 * 192 * 4, STAGE_F = 16 * 192;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  int split, tile;
  if (!x6w_map(g, lin, split, tile)) return;
  const int m0 = (tile / g.ntiles) * 64, n0 = (tile % g.ntiles) * 128;
  const int r = lane & 31, h = lane >> 5;
  // balanced slabs of whole 128-row units: the first g.urem slabs hold one unit more (a fixed slab length left the last slab
  // — and, with slab s on XCD s % 8, one XCD — with as little as a third of the others' rows)
  const long long slab0 = 128ll * ((long long)split * g.ubase + min(split, g.urem));
  const int rows_here = 128 * (g.ubase + (split < g.urem ? 1 : 0));
  const int rows_per_wave = rows_here >> 2;
  const long long k_begin = slab0 + (long long)w * rows_per_wave;
  const int T = rows_per_wave >> 4;              // even, >= 2
  const char* Az = (const char*)(g.A + (size_t)z * g.a_bstride);
  const char* Bz = (const char*)(g.B + (size_t)z * g.b_bstride);
  constexpr unsigned RING_BYTES = 4 * 3 * STAGE_BYTES;
  const unsigned lds_base = (unsigned)(size_t)wlds;
  const unsigned lds0 = lds_base + w * (3 * STAGE_BYTES), lds_end = lds0 + 3 * STAGE_BYTES, lds_zero = lds_base + RING_BYTES;
  x6w_clear_zero(wlds, RING_BYTES, tid);

  // DMA pieces of 1 KiB: dY 4 x (4 rows x 256 B), X 8 x (2 rows x 512 B); columns past M / N come from a clamped address
  // and are never read.  The per-piece offsets are formed once; a step advances the two row bases and the destination stage
  const int ca = min(m0 + 4 * (lane & 15), g.M - 4), cb = min(n0 + 4 * (lane & 31), g.N - 4);
  const unsigned dA = (unsigned)(((size_t)(lane >> 4) * g.lda + ca) * 4), dB = (unsigned)(((size_t)(lane >> 5) * g.ldb + cb) * 4);
  const unsigned strideA = (unsigned)g.lda * 16u, strideB = (unsigned)g.ldb * 8u;
  unsigned va[4], vb[8];
#pragma unroll
  for (int p = 0; p < 4; ++p) va[p] = dA + p * strideA;
#pragma unroll
  for (int p = 0; p < 8; ++p) vb[p] = dB + p * strideB;
  const char* arow = Az + k_begin * g.lda * 4;                                                // step 0's 16 rows
  const char* brow = Bz + k_begin * g.ldb * 4;
  const size_t stepA = (size_t)g.lda * 64, stepB = (size_t)g.ldb * 64;                        // 16 rows, bytes
  unsigned wr = lds0;                                                                         // stage the next DMA step fills
  auto dma = [&]() __attribute__((always_inline)) {
    x6w_dma4(arow, va[0], va[1], va[2], va[3], wr);
    x6w_dma4(brow, vb[0], vb[1], vb[2], vb[3], wr + 4096);
    x6w_dma4(brow, vb[4], vb[5], vb[6], vb[7], wr + 8192);
    arow += stepA; brow += stepB;
    wr += STAGE_BYTES;
    if (wr == lds_end) wr = lds0;
  };
  // fragment block q (0, 1: dY columns 32 q + r; 2 .. 5: X columns 32 (q - 2) + r) of a stage: lane (r, h) reads rows 8h .. 8h+7
  // of its column — or the zero region
  bool ok[6];
  unsigned lo[6];
#pragma unroll
  for (int q = 0; q < 2; ++q) { ok[q] = m0 + 32 * q + r < g.M; lo[q] = (unsigned)(((8 * h) * 64 + 32 * q + r) * 4); }
#pragma unroll
  for (int q = 0; q < 4; ++q) { ok[2 + q] = n0 + 32 * q + r < g.N; lo[2 + q] = (unsigned)((1024 + (8 * h) * 128 + 32 * q + r) * 4); }
  unsigned rd = lds0;                                                                         // stage the next read step reads
  auto readfr = [&](float (&raw)[6][8]) __attribute__((always_inline)) {
#pragma unroll
    for (int q = 0; q < 2; ++q) x6w_readblk<1>(raw[q], ok[q] ? rd + lo[q] : lds_zero);
#pragma unroll
    for (int q = 2; q < 6; ++q) x6w_readblk<2>(raw[q], ok[q] ? rd + lo[q] : lds_zero);
    rd += STAGE_BYTES;
    if (rd == lds_end) rd = lds0;
  };
  float raw0[6][8], raw1[6][8];
  X6WFragW fr0, fr1;
  unsigned t0[4], t1[4];
  x6_f32x16 acc[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;

  // prologue: DMA steps 0..2; read steps 0 and 1; split step 0
  dma();
  dma();
  if (T > 2) dma();
  __syncthreads();                              // the zero region is cleared
  if (T > 2) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  readfr(raw0);
  readfr(raw1);
  x6w_ops<0, 264, true>(raw0, fr0, t0, t1);
  // after step s: DMA step s + 3 (its stage held step s, read two steps ago), wait for step s + 2, read it
  auto tailwork = [&](float (&rawn)[6][8], int s) __attribute__((always_inline)) {
    if (s + 3 < T) dma();
    if (s + 2 < T) {
      if (s + 3 < T) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      readfr(rawn);
    }
  };
  for (int s = 0; s + 2 < T; s += 2) {
    x6ww_slots<0, true>(fr0, fr1, acc, raw1, t0, t1);          // step s: splits step s+1 (raw1) into fr1
    tailwork(raw0, s);                                            // raw0 <- step s+2
    x6ww_slots<0, true>(fr1, fr0, acc, raw0, t0, t1);          // step s+1: splits step s+2 (raw0) into fr0
    tailwork(raw1, s + 1);                                        // raw1 <- step s+3
  }
  x6ww_slots<0, true>(fr0, fr1, acc, raw1, t0, t1);
  x6ww_slots<0, false>(fr1, fr0, acc, raw0, t0, t1);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  __syncthreads();                              // every wave is done with its ring: reuse the LDS for the reduction
  float* red = wlds;                            // [4][64][129]: odd pitch, so that the transposed walk below is conflict-free
  constexpr int RP = 129, RW = 64 * RP;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int row = 32 * i + (q & 3) + 8 * (q >> 2) + 4 * h, col = 32 * j + r;
        red[w * RW + row * RP + col] = acc[i][j][q];
      }
  __syncthreads();
  float* C = g.C + (size_t)z * g.c_bstride;
#pragma unroll 4
  for (int u = 0; u < 32; ++u) {
    // consecutive threads walk the dimension that is contiguous in dW: the tile's columns, or (roles exchanged) its rows
    const int e = tid + 256 * u;
    const int row = g.swap ? (e & 63) : (e >> 7), col = g.swap ? (e >> 6) : (e & 127);
    const int o = row * RP + col;
    const float v = (red[o] + red[RW + o]) + (red[2 * RW + o] + red[3 * RW + o]);
    if (m0 + row < g.M && n0 + col < g.N) {
      // (roles exchanged: the kernel's M side is cin)
      const int wr = g.swap ? n0 + col : m0 + row, wc0 = g.swap ? m0 + row : n0 + col;
      const int wc = g.kperm ? x6_kperm_src(wc0, g.swap ? g.M : g.N) : wc0;
      float* dst = C + (size_t)wr * g.ldc + wc;
      if constexpr (DET) dst[(size_t)split * sstride] = v;
      else __hip_atomic_fetch_add(dst, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

__global__ __launch_bounds__(256) void wgrad_x6_wide_kernel(X6WgradArgs g) { wgrad_x6_wide_body<false>(g, blockIdx.x, blockIdx.y, 0); }
__global__ __launch_bounds__(256) void wgrad_x6_wide_det_kernel(X6WgradArgs g, size_t sstride) { wgrad_x6_wide_body<true>(g, blockIdx.x, blockIdx.y, sstride); }

// ---- batched form: the weight gradients of SEVERAL layers in one launch ------------------------------------------------
// A weight gradient is off the backward's critical path (nothing downstream reads dW), and at this path's sizes each one is
// a launch of 50-400 workgroups on 256 CUs that lives 12-40 us: ten of them per Grapher + GrapherLabel step, a fifth of the
// step.  The host side queues them while the backward runs and issues ONE launch at its end: workgroup ids [begin[i],
// begin[i+1]) belong to problem i (begin[] in multiples of 8, so lin & 7 stays the XCD inside a problem), which runs the
// 64 x 64 or the 64 x 128 body above exactly as its own launch would.  The descriptors travel in the kernel arguments (a
// hipGraph node keeps them by value).
struct X6WgradBatch {
  int n;
  int begin[X6W_BATCH + 1];
  int gridx[X6W_BATCH];                         // workgroups per group z of the problem (a multiple of 8)
  int wide[X6W_BATCH];
  X6WgradArgs p[X6W_BATCH];
};

__global__ __launch_bounds__(256) void wgrad_x6_batch_kernel(X6WgradBatch b) {
  const int bid = blockIdx.x;
  int i = 0;
  while (i + 1 < b.n && bid >= b.begin[i + 1]) ++i;
  const int local = bid - b.begin[i], gx = b.gridx[i];
  const int z = local / gx, lin = local - z * gx;
  const X6WgradArgs g = b.p[i];
  if (b.wide[i]) wgrad_x6_wide_body<false>(g, lin, z, 0);
  else wgrad_x6_dma_body<false>(g, lin, z, 0);
}

// The deterministic batch: the same launch with every problem's tiles stored into that problem's slab images (p[i].C: image 0)
struct X6WgradBatchDet {
  X6WgradBatch b;
  size_t sstride[X6W_BATCH];                    // floats per slab image of problem i (nb x cout x cin)
};

__global__ __launch_bounds__(256) void wgrad_x6_batch_det_kernel(X6WgradBatchDet d) {
  const int bid = blockIdx.x;
  int i = 0;
  while (i + 1 < d.b.n && bid >= d.b.begin[i + 1]) ++i;
  const int local = bid - d.b.begin[i], gx = d.b.gridx[i];
  const int z = local / gx, lin = local - z * gx;
  const X6WgradArgs g = d.b.p[i];
  if (d.b.wide[i]) wgrad_x6_wide_body<true>(g, lin, z, d.sstride[i]);
  else wgrad_x6_dma_body<true>(g, lin, z, d.sstride[i]);
}

// The ordered reduction behind the deterministic launches: thread e of problem i walks the S slab images of its element in
// slab order, dw[e] = (((0 + P_0) + P_1) + ...) + P_{S-1} — fp32, eight independent loads in flight, the adds sequential —
// and stores it: every element of dw exactly once, whatever it held.  Workgroups [begin[i], begin[i+1]) serve problem i.
struct X6WdetReduce {
  int n;
  int S[X6W_BATCH];
  int begin[X6W_BATCH + 1];
  float* dw[X6W_BATCH];
  const float* ws[X6W_BATCH];
  size_t E[X6W_BATCH];
};

__global__ __launch_bounds__(256) void wgrad_x6_det_reduce_kernel(X6WdetReduce d) {
  const int bid = blockIdx.x;
  int i = 0;
  while (i + 1 < d.n && bid >= d.begin[i + 1]) ++i;
  const size_t E = d.E[i], e = (size_t)(bid - d.begin[i]) * 256 + threadIdx.x;
  if (e >= E) return;
  const float* p = d.ws[i] + e;
  const int S = d.S[i];
  float v = 0.f;
  int s = 0;
  for (; s + 8 <= S; s += 8) {
    float t[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) t[j] = p[(size_t)(s + j) * E];
#pragma unroll
    for (int j = 0; j < 8; ++j) v += t[j];
  }
  for (; s < S; ++s) v += p[(size_t)s * E];
  d.dw[i][e] = v;
}

}  // namespace gkg
using namespace gkg;

namespace gkg {
// Train-mode BN parameters from the fp64 column sums of Y (which EXCLUDES the conv bias, folded here); re-zeroes the sums
// so the scratch buffer is clean for the next projection (it is shared, stream-ordered, by all layers).
//   mean = S/R, var = Q/R - mean^2 (biased), invstd = rsqrt(var + eps), a = gamma*invstd, c = beta - a*mean
//   running_mean <- (1-mom)*rm + mom*(mean + bias), running_var <- (1-mom)*rv + mom*var*R/(R-1)
__global__ __launch_bounds__(256) void bn_sums_finalize_kernel(double* __restrict__ sums, int R, int C,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta,
                                                               const float* __restrict__ bias, float* __restrict__ running_mean,
                                                               float* __restrict__ running_var, float* __restrict__ a,
                                                               float* __restrict__ cs, float* __restrict__ mean,
                                                               float* __restrict__ invstd, float momentum, float eps,
                                                               long long* __restrict__ nbt, int nslots, int nb) {
  const int ch = blockIdx.x * 256 + threadIdx.x;
  const int q = blockIdx.y;
  if (nbt && ch == 0 && q == 0) *nbt += 1;
  if (ch >= C) return;
  // `nslots` copies of the sums ([slot][nb][2][C]): producers with thousands of row tiles spread their atomics over the
  // copies (same-address fp64 atomics serialise); added here in slot order
  double S = 0.0, Q = 0.0;
  for (int sl = 0; sl < nslots; ++sl) {
    double* sz = sums + ((size_t)sl * nb + q) * 2 * C + ch;
    S += sz[0]; Q += sz[C];
    sz[0] = 0.0; sz[C] = 0.0;
  }
  const double m = S / R;
  double var = Q / R - m * m;
  if (var < 0.0) var = 0.0;
  const size_t o = (size_t)q * C + ch;
  const float is = (float)(1.0 / sqrt(var + (double)eps));
  const float av = gamma[o] * is;
  a[o] = av;
  cs[o] = beta[o] - av * (float)m;
  mean[o] = (float)m;
  invstd[o] = is;
  if (running_mean) {
    const float bv = bias ? bias[o] : 0.f;
    running_mean[o] = (1.f - momentum) * running_mean[o] + momentum * ((float)m + bv);
    const double unb = R > 1 ? var * (double)R / (double)(R - 1) : var;
    running_var[o] = (1.f - momentum) * running_var[o] + momentum * (float)unb;
  }
}

hipError_t launch_bn_sums_finalize(double* stats, int R, int cout, int nb, const float* gamma, const float* beta,
                                   const float* bias, float* running_mean, float* running_var, float* bn_a, float* bn_c,
                                   float* bn_mean, float* bn_invstd, float momentum, float eps, long long* nbt, hipStream_t st,
                                   int nslots) {
  hipLaunchKernelGGL(bn_sums_finalize_kernel, dim3((cout + 255) / 256, nb), dim3(256), 0, st, stats, R, cout, gamma, beta,
                     bias, running_mean, running_var, bn_a, bn_c, bn_mean, bn_invstd, momentum, eps, nbt, nslots, nb);
  return hipGetLastError();
}

}  // namespace gkg


extern "C" size_t gkg_x6_planes_bytes(int cin, int cout, int nb, int dgrad) {
  if (x6_bad_dim(cin) || x6_bad_dim(cout) || nb <= 0) return 0;
  return 16 * (dgrad ? x6_plane_units(cin, cout, nb) : x6_plane_units(cout, cin, nb));
}

extern "C" int gkg_x6_prep_desc_bytes(void) { return (int)sizeof(X6PrepDesc); }

// Fills descriptor `index` of a HOST array laid out as gkg_x6_prep_desc_bytes() per entry (one of the two plane pointers may
// be null: that orientation is not produced) and returns the unit count after
// it (pass it as unit_begin of the next entry; the last return value is total_units of gkg_x6_prep_weights).
extern "C" long long gkg_x6_prep_desc_fill(void* host_descs, int index, const float* w, void* planes_fwd, void* planes_dgrad,
                                           int cin, int cout, int nb, long long unit_begin, int kperm) {
  if (!host_descs || !w || (!planes_fwd && !planes_dgrad) || x6_bad_dim(cin) || x6_bad_dim(cout) || nb <= 0 || index < 0) return -1;
  if (kperm && (cin & 1)) return -1;
  X6PrepDesc* d = reinterpret_cast<X6PrepDesc*>(host_descs) + index;
  d->w = w; d->pf = (uint4*)planes_fwd; d->pd = (uint4*)planes_dgrad;
  d->nb = nb; d->N = cout; d->K = cin; d->unit_begin = (int)unit_begin; d->kperm = kperm ? 1 : 0;
  const long long units = (long long)((planes_fwd ? x6_plane_units(cout, cin, nb) : 0) + (planes_dgrad ? x6_plane_units(cin, cout, nb) : 0)) / 3;
  if (unit_begin + units > 0x7fffffffLL) return -1;
  return unit_begin + units;
}

// One launch splits every described weight into its forward and dgrad planes.  `descs_dev`: the descriptor array copied to
// the device (it holds device pointers only).
static int x6_prep_impl(const void* descs_dev, int ndesc, long long total_units, void* z0, size_t z0_bytes, void* z1,
                        size_t z1_bytes, void* stream) {
  if (!descs_dev) return gkg_fail(GKG_ERR_NULL, "gkg_x6_prep_weights: null descriptor array");
  if (ndesc <= 0 || ndesc > 256 || total_units <= 0 || total_units > 0x7fffffffLL) return gkg_fail(GKG_ERR_SHAPE, "gkg_x6_prep_weights: need 1 <= ndesc <= 256 and 0 < total_units < 2^31");
  if (((size_t)z0 & 15) || ((size_t)z1 & 15) || (z0_bytes & 15) || (z1_bytes & 15) || (!z0 && z0_bytes) || (!z1 && z1_bytes))
    return gkg_fail(GKG_ERR_SHAPE, "gkg_x6_prep_weights_zero: buffers to clear must be 16-byte aligned multiples of 16 bytes");
  X6ZeroJobs zj{};
  zj.p[0] = (uint4*)z0; zj.n16[0] = z0_bytes / 16;
  zj.p[1] = (uint4*)z1; zj.n16[1] = z1_bytes / 16;
  zj.unit_blocks = (int)((total_units + 255) / 256);
  const unsigned long long zmax = zj.n16[0] > zj.n16[1] ? zj.n16[0] : zj.n16[1];
  unsigned zblocks = (unsigned)((zmax + 256 * 16 - 1) / (256 * 16));          // ~16 stores per thread
  if (zblocks > 1024) zblocks = 1024;
  hipLaunchKernelGGL(x6_prep_kernel, dim3((unsigned)zj.unit_blocks + zblocks), dim3(256), 0, (hipStream_t)stream,
                     (const X6PrepDesc*)descs_dev, ndesc, (int)total_units, zj);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : gkg_fail_hip(e, "x6_prep_kernel");
}

extern "C" int gkg_x6_prep_weights(const void* descs_dev, int ndesc, long long total_units, void* stream) {
  return x6_prep_impl(descs_dev, ndesc, total_units, nullptr, 0, nullptr, 0, stream);
}

// gkg_x6_prep_weights that also CLEARS up to two buffers (zero0 / zero1, 16-byte aligned, byte counts multiples of 16; NULL / 0:
// none) in the same launch: what a training step clears before its first projection anyway — the flat gradient buffer the
// weight-gradient kernels accumulate into and the fp64 BN scratch.
extern "C" int gkg_x6_prep_weights_zero(const void* descs_dev, int ndesc, long long total_units, void* zero0, size_t zero0_bytes,
                                        void* zero1, size_t zero1_bytes, void* stream) {
  return x6_prep_impl(descs_dev, ndesc, total_units, zero0, zero0_bytes, zero1, zero1_bytes, stream);
}

// ---- entry points: fill a call, plan it (gkg_x6_plan.h), check the pointers, launch what the plan names -------------------------
// fp64 column-sum scratch of the projections' BN-statistics epilogue: doubles per buffer
extern "C" int gkg_linear_stats_doubles() { return X6_STATS_DOUBLES; }

extern "C" size_t gkg_x6_splitk_workspace_bytes(void) { return X6_SK_BYTES; }

// gkg_linear_bn_fwd with the weights given as forward planes (gkg_x6_prep_weights).  x (nb, R, cin) with row pitch ldx and
// batch stride x_bstride (floats); y (nb, R, cout) contiguous.  Same `train` modes and outputs as gkg_linear_bn_fwd.
// The _sk form takes a split-K workspace (gkg_x6_splitk_workspace_bytes() bytes, its first 4 KiB ZERO before the first use; every
// launch leaves them zero again): few-row / long-contraction shapes then run as several K ranges per tile.
extern "C" int gkg_linear_bn_fwd_x6_sk(const float* x, int ldx, size_t x_bstride, const void* planes_fwd, float* y, int R,
                                       int cin, int cout, int nb, int train, const float* gamma, const float* beta,
                                       const float* bias, float* running_mean, float* running_var,
                                       long long* num_batches_tracked, float* bn_a, float* bn_c, float* bn_mean,
                                       float* bn_invstd, float momentum, float eps, double* stats, void* splitk_ws,
                                       size_t splitk_bytes, unsigned flags, void* stream) {
  X6GemmCall q = x6_call(X6R_FWD, R, cout, cin, nb, x, ldx, x_bstride, splitk_ws, splitk_bytes, flags);
  q.train = train;
  X6GemmPlan pl;
  const char* msg = nullptr;
  if (const int rc = x6_gemm_plan(q, &pl, &msg)) return gkg_fail(rc, msg);
  if (!x || !planes_fwd || !y) return gkg_fail(GKG_ERR_NULL, "gkg_linear_bn_fwd_x6: null pointer");
  if (train) {
    if (!stats) return gkg_fail(GKG_ERR_NULL, "gkg_linear_bn_fwd_x6: training needs the stats scratch");
    if (train != 2) {
      if (!gamma || !beta || !bn_a || !bn_c || !bn_mean || !bn_invstd) return gkg_fail(GKG_ERR_NULL, "gkg_linear_bn_fwd_x6: training needs gamma, beta and the four outputs");
      if ((running_mean == nullptr) != (running_var == nullptr)) return gkg_fail(GKG_ERR_NULL, "gkg_linear_bn_fwd_x6: running stats come in pairs");
    }
  }
  hipStream_t st = (hipStream_t)stream;
  X6Args a = x6_operands(x, planes_fwd, y, (size_t)R * cout, cout);
  a.sums = stats;
  hipError_t e = train ? x6_launch<X6_BNSTATS>(q, pl, a, splitk_ws, st) : x6_launch<X6_STORE>(q, pl, a, splitk_ws, st);
  if (e == hipSuccess && train && train != 2) {
    e = launch_bn_sums_finalize(stats, R, cout, nb, gamma, beta, bias, running_mean, running_var, bn_a, bn_c, bn_mean, bn_invstd,
                                momentum, eps, num_batches_tracked, st, pl.nslots);
  }
  return e == hipSuccess ? 0 : gkg_fail_hip(e, "gemm_x6_kernel (forward)");
}

extern "C" int gkg_linear_bn_fwd_x6(const float* x, int ldx, size_t x_bstride, const void* planes_fwd, float* y, int R,
                                    int cin, int cout, int nb, int train, const float* gamma, const float* beta,
                                    const float* bias, float* running_mean, float* running_var,
                                    long long* num_batches_tracked, float* bn_a, float* bn_c, float* bn_mean,
                                    float* bn_invstd, float momentum, float eps, double* stats, void* stream) {
  return gkg_linear_bn_fwd_x6_sk(x, ldx, x_bstride, planes_fwd, y, R, cin, cout, nb, train, gamma, beta, bias, running_mean, running_var,
                                 num_batches_tracked, bn_a, bn_c, bn_mean, bn_invstd, momentum, eps, stats, nullptr, 0, 0, stream);
}

// Workgroups of the tile-walk launch that y (nb, R, cout) = x (nb, R, cin) W^T takes on the current device with these flags and
// with / without a split-K workspace — the forward's plan with the plain epilogue (X6GemmCall::slots has the quirk), for callers and
// tests that must know the launch form beforehand; 0: the launch does not walk (another body, a split contraction, not two rounds,
// GKG_X6_NO_WALK); < 0: error.
extern "C" int gkg_x6_walk_workgroups(int R, int cin, int cout, int nb, int has_ws, unsigned flags) {
  if (R <= 0 || x6_bad_dim(cin) || x6_bad_dim(cout) || nb <= 0 || nb > 64) return gkg_fail(GKG_ERR_SHAPE, "gkg_x6_walk_workgroups: bad shape");
  X6GemmCall q = x6_call(X6R_FWD, R, cout, cin, nb, nullptr, cin, (size_t)R * cin, nullptr, has_ws ? X6_SK_BYTES : 0, flags);
  q.has_ws = has_ws != 0;
  X6GemmPlan pl;
  x6_gemm_ladder(q, &pl);
  if (hipError_t e = x6_plan_walk<X6_STORE>(q, pl); e != hipSuccess) return gkg_fail_hip(e, "gkg_x6_walk_workgroups");
  return pl.body == X6_BODY_WALK ? (int)pl.grid_x : 0;
}

// dx (nb, R, cin) = dy (nb, R, cout; row pitch ldg, batch stride g_bstride) * w, the weights given as dgrad planes; dx with row
// pitch ldx / batch stride x_bstride (ldx == 0: contiguous).  `residual` (nb, R, cin) contiguous or null: dx = dy w + residual —
// the gradient that reaches the layer's input along a skip connection (reference torch_vertex.py:331,354,402 `+ _tmp`), added in
// the epilogue instead of by a stand-alone kernel.
extern "C" int gkg_linear_dgrad_x6_sk(const float* dy, int ldg, size_t g_bstride, const void* planes_dgrad, float* dx, int R,
                                      int cin, int cout, int nb, const float* residual, void* splitk_ws, size_t splitk_bytes,
                                      int ldx, size_t x_bstride, unsigned flags, void* stream) {
  X6GemmCall q = x6_call(X6R_DGRAD, R, cin, cout, nb, dy, ldg, g_bstride, splitk_ws, splitk_bytes, flags);
  q.ldc = ldx; q.c_bstride = x_bstride; q.has_residual = residual != nullptr;
  X6GemmPlan pl;
  const char* msg = nullptr;
  if (const int rc = x6_gemm_plan(q, &pl, &msg)) return gkg_fail(rc, msg);
  if (!dy || !planes_dgrad || !dx) return gkg_fail(GKG_ERR_NULL, "gkg_linear_dgrad_x6: null pointer");
  const X6Args a = x6_operands(dy, planes_dgrad, dx, ldx ? x_bstride : (size_t)R * cin, ldx ? ldx : cin, residual);
  hipError_t e = x6_launch<X6_STORE>(q, pl, a, splitk_ws, (hipStream_t)stream);
  return e == hipSuccess ? 0 : gkg_fail_hip(e, "gemm_x6_kernel (dgrad)");
}

extern "C" int gkg_linear_dgrad_x6(const float* dy, int ldg, size_t g_bstride, const void* planes_dgrad, float* dx, int R,
                                   int cin, int cout, int nb, void* stream) {
  return gkg_linear_dgrad_x6_sk(dy, ldg, g_bstride, planes_dgrad, dx, R, cin, cout, nb, nullptr, nullptr, 0, 0, 0, 0, stream);
}

// The un-grouped input gradient (+ token-major residual) stored CHANNEL-MAJOR: dx (B, cin, N) = (dy w + residual)^T per image,
// R == B * N rows — a block's first layer, whose input gradient leaves the block as an NCHW tensor (round 8: the re-layout pass
// behind gkg_linear_dgrad_x6_sk and its kernel boundary are gone).  The 128-row tile kernel stores so itself (X6_STORE_NCHW) where
// the plan allows (x6_nchw_two_launch); otherwise the two launches run as before: gkg_linear_dgrad_x6_sk into `dx_tm` (R, cin;
// scratch, required) and gkg_tm_affine_to_nchw.  Either way dx has the bits of that two-launch form.
extern "C" int gkg_linear_dgrad_x6_nchw(const float* dy, int ldg, const void* planes_dgrad, float* dx, float* dx_tm, int R, int cin,
                                        int cout, const float* residual, int B, int N, void* splitk_ws, size_t splitk_bytes,
                                        unsigned flags, void* stream) {
  X6GemmCall q = x6_call(X6R_DGRAD_NCHW, R, cin, cout, 1, dy, ldg, 0, splitk_ws, splitk_bytes, flags);
  q.has_residual = residual != nullptr; q.nchw_b = B; q.nchw_n = N; q.dx_aligned = ((size_t)dx & 15) == 0;
  X6GemmPlan pl;
  const char* msg = nullptr;
  if (const int rc = x6_gemm_plan(q, &pl, &msg)) return gkg_fail(rc, msg);
  if (!dy || !planes_dgrad || !dx || !dx_tm) return gkg_fail(GKG_ERR_NULL, "gkg_linear_dgrad_x6_nchw: null pointer");
  if (pl.two_launch) {
    const int rc = gkg_linear_dgrad_x6_sk(dy, ldg, (size_t)R * cout, planes_dgrad, dx_tm, R, cin, cout, 1, residual, splitk_ws, splitk_bytes, 0, 0,
                                          flags, stream);
    return rc != 0 ? rc : gkg_tm_affine_to_nchw(dx_tm, nullptr, nullptr, nullptr, dx, B, cin, N, nullptr, stream);
  }
  X6Args a = x6_operands(dy, planes_dgrad, dx, (size_t)R * cin, cin, residual);
  a.nchw_n = N; a.nchw_c = cin;
  hipError_t e = x6_launch<X6_STORE_NCHW>(q, pl, a, splitk_ws, (hipStream_t)stream);
  return e == hipSuccess ? 0 : gkg_fail_hip(e, "gemm_x6_kernel (dgrad, channel-major store)");
}

// The same input gradient with the BACKWARD statistics of the producer's BN in the epilogue (X6_BNBWD): dx is the upstream
// gradient of the layer  h = act(BN(py))  that made this projection's input; psums [pnb][2][pco] fp64 receives (atomics)
// sum dz and sum dz * yhat per channel — what gkg_bn_bwd_atomic's statistics pass would compute from dx and py.  Un-grouped
// projections only (nb == 1): dx (R, cin), cin == pnb * pco, py (pnb, R, pco).
// With gkg_linear_dgrad_x6_sk's choice of kernel body (round 9): given the split-K workspace the launch takes the short-matrix
// body / the cross-workgroup split exactly where gkg_linear_dgrad_x6_sk does for the same shape and flags, so dx has that call's
// bits, and `residual` (R, cin; or NULL) is added in front of the statistics (the BN's upstream gradient is the sum).  The 128-row
// tile body takes no residual here: gkg_linear_dgrad_x6_bnbwd_sk_supported() tells, and an unsupported call returns
// GKG_ERR_UNSUPPORTED with nothing launched.
extern "C" int gkg_linear_dgrad_x6_bnbwd_sk_supported(int R, int cin, int has_residual, int has_ws, unsigned flags) {
  return (!has_residual || x6_bnbwd_takes_residual(R, cin, has_ws != 0, flags)) ? 1 : 0;
}

extern "C" int gkg_linear_dgrad_x6_bnbwd_sk(const float* dy, int ldg, const void* planes_dgrad, float* dx, int R, int cin, int cout,
                                            const float* residual, const float* py, const float* pa, const float* pc,
                                            const float* pmean, const float* pinvstd, double* psums, int pnb, int pco, int pact,
                                            void* splitk_ws, size_t splitk_bytes, unsigned flags, void* stream) {
  X6GemmCall q = x6_call(X6R_DGRAD_BNBWD, R, cin, cout, 1, dy, ldg, 0, splitk_ws, splitk_bytes, flags);
  q.has_residual = residual != nullptr; q.pnb = pnb; q.pco = pco; q.pact = pact;
  X6GemmPlan pl;
  const char* msg = nullptr;
  if (const int rc = x6_gemm_plan(q, &pl, &msg)) return gkg_fail(rc, msg);
  if (!dy || !planes_dgrad || !dx || !py || !pa || !pc || !pmean || !pinvstd || !psums)
    return gkg_fail(GKG_ERR_NULL, "gkg_linear_dgrad_x6_bnbwd_sk: null pointer");
  X6Args a = x6_operands(dy, planes_dgrad, dx, (size_t)R * cin, cin, residual);
  a.py = py; a.pa = pa; a.pc = pc; a.pmean = pmean; a.pinvstd = pinvstd; a.psums = psums; a.pco = pco; a.pact = pact;
  hipError_t e = x6_launch<X6_BNBWD>(q, pl, a, splitk_ws, (hipStream_t)stream);
  return e == hipSuccess ? 0 : gkg_fail_hip(e, "gemm_x6 (dgrad + BN backward statistics)");
}

extern "C" int gkg_linear_dgrad_x6_bnbwd(const float* dy, int ldg, const void* planes_dgrad, float* dx, int R, int cin, int cout,
                                         const float* py, const float* pa, const float* pc, const float* pmean,
                                         const float* pinvstd, double* psums, int pnb, int pco, int pact, void* stream) {
  // no workspace, no residual: always the 128-row tile body
  return gkg_linear_dgrad_x6_bnbwd_sk(dy, ldg, planes_dgrad, dx, R, cin, cout, nullptr, py, pa, pc, pmean, pinvstd, psums, pnb, pco, pact,
                                      nullptr, 0, 0, stream);
}

// ---- weight gradients ---------------------------------------------------------------------------------------------------------
// dw (nb, cout, cin) += dy^T x over the R rows; dw must be ZERO on entry (the slabs of rows are added with fp32 atomics).
// dy (nb, R, cout) row pitch ldg / batch stride g_bstride, x (nb, R, cin) row pitch ldx / batch stride x_bstride (floats).
// The deterministic forms (gkg_linear_wgrad_x6_det, _batch_det; include/gkg_hip.h has the definition) are the same launches with
// the DET instantiations of their bodies — slab s of the plan stores its tiles into image s of the caller's workspace (main
// launch's slabs first, then the ragged remainder's, both in ascending row order) — and ONE small launch behind them that adds
// the images in that order and writes dW.  No atomics, no memset, no counters: the kernel boundary orders the partial stores
// before the reduction's loads.
namespace gkg {
static X6WgradCall x6w_call(const float* dy, int ldg, size_t g_bstride, const float* x, int ldx, size_t x_bstride, int R, int cin, int cout,
                            int nb, int kperm, int force_slabs) {
  return X6WgradCall{R, cin, cout, nb, ldg, ldx, g_bstride, x_bstride, (((size_t)dy | (size_t)x) & 15) == 0, 0, kperm, force_slabs};
}
static X6WgradCall x6w_call(const GkgWgradProblem& q) {
  return x6w_call(q.dy, q.ldg, q.g_bstride, q.x, q.ldx, q.x_bstride, q.R, q.cin, q.cout, q.nb, q.kperm, 0);
}

// bind: the operands of one planned launch (`part`: the plan's main or rest) into its kernel arguments.  C: dw, or image 0 of the
// launch in a deterministic workspace.
static X6WgradArgs x6w_bind(const X6WgradCall& q, const X6WgradPlan& pl, const X6WgradPart& part, const float* dy, const float* x, float* C) {
  X6WgradArgs a{};
  const bool swap = &part == &pl.main && pl.swap;      // the kernel's "A" (64-wide side) is x, its "B" (128-wide side) dy
  dy += (size_t)part.row0 * q.ldg; x += (size_t)part.row0 * q.ldx;
  a.A = swap ? x : dy; a.a_bstride = swap ? q.x_bstride : q.g_bstride; a.lda = swap ? q.ldx : q.ldg;
  a.B = swap ? dy : x; a.b_bstride = swap ? q.g_bstride : q.x_bstride; a.ldb = swap ? q.ldg : q.ldx;
  a.C = C; a.c_bstride = (size_t)q.cout * q.cin; a.ldc = q.cin;
  a.M = part.M; a.N = part.N; a.K = part.rows;
  a.mtiles = part.mtiles; a.ntiles = part.ntiles; a.splits = part.splits; a.rows_per_split = part.rows_per_split;
  a.swap = swap ? 1 : 0; a.share = part.share; a.ubase = part.ubase; a.urem = part.urem;
  a.kperm = pl.kperm;
  return a;
}

// the ragged remainder's own launch (register-load kernel); E: floats per slab image (DET)
template <bool DET>
static int x6w_launch_rest(const X6WgradArgs& t, int grid_x, int nb, size_t E, hipStream_t st) {
  if constexpr (DET) hipLaunchKernelGGL(wgrad_x6_det_kernel, dim3(grid_x, nb), dim3(256), 0, st, t, E);
  else hipLaunchKernelGGL(wgrad_x6_kernel, dim3(grid_x, nb), dim3(256), 0, st, t);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : gkg_fail_hip(e, DET ? "wgrad_x6_det_kernel" : "wgrad_x6_kernel");
}

// one problem's launches.  C: dw (zero on entry), or DET the workspace (slab images of E floats)
template <bool DET>
static int x6w_run(const X6WgradCall& q, const X6WgradPlan& pl, const float* dy, const float* x, float* C, size_t E, hipStream_t st) {
  if (pl.main.rows > 0) {
    const X6WgradArgs m = x6w_bind(q, pl, pl.main, dy, x, C);
    const size_t sh = pl.wide ? X6W_SH_WIDE : X6W_SH_DMA;
    const dim3 grid(pl.main.grid_x, q.nb);
    hipError_t e;
    if constexpr (DET) {
      e = pl.wide ? x6_kernel_once<wgrad_x6_wide_det_kernel>(sh) : x6_kernel_once<wgrad_x6_dma_det_kernel>(sh);
      if (e != hipSuccess) return gkg_fail_hip(e, "wgrad_x6 deterministic kernel (attribute)");
      if (pl.wide) hipLaunchKernelGGL(wgrad_x6_wide_det_kernel, grid, dim3(256), sh, st, m, E);
      else hipLaunchKernelGGL(wgrad_x6_dma_det_kernel, grid, dim3(256), sh, st, m, E);
    } else {
      e = pl.wide ? x6_kernel_once<wgrad_x6_wide_kernel>(sh) : x6_kernel_once<wgrad_x6_dma_kernel>(sh);
      if (e != hipSuccess) return gkg_fail_hip(e, "wgrad_x6 DMA kernel (attribute)");
      if (pl.wide) hipLaunchKernelGGL(wgrad_x6_wide_kernel, grid, dim3(256), sh, st, m);
      else hipLaunchKernelGGL(wgrad_x6_dma_kernel, grid, dim3(256), sh, st, m);
    }
    e = hipGetLastError();
    if (e != hipSuccess) return gkg_fail_hip(e, DET ? "wgrad_x6 deterministic DMA kernel" : "wgrad_x6 DMA kernel");
  }
  if (pl.rest.rows > 0)
    return x6w_launch_rest<DET>(x6w_bind(q, pl, pl.rest, dy, x, C + (DET ? (size_t)pl.main_slabs() * E : 0)), pl.rest.grid_x, q.nb, E, st);
  return 0;
}

// the reduction launches of up to X6W_BATCH problems each
struct X6WdetReducer {
  X6WdetReduce d{};
  hipStream_t st;
  int flush() {
    if (d.n == 0) return 0;
    hipLaunchKernelGGL(wgrad_x6_det_reduce_kernel, dim3(d.begin[d.n]), dim3(256), 0, st, d);
    hipError_t e = hipGetLastError();
    d.n = 0;
    return e == hipSuccess ? 0 : gkg_fail_hip(e, "wgrad_x6_det_reduce_kernel");
  }
  int add(float* dw, const float* ws, size_t E, int S) {
    const long long blocks = (long long)((E + 255) / 256);
    if (d.n == X6W_BATCH || (d.n > 0 && (long long)d.begin[d.n] + blocks > 0x7fffffffll)) {
      int rc = flush();
      if (rc) return rc;
    }
    const int i = d.n;
    d.dw[i] = dw; d.ws[i] = ws; d.E[i] = E; d.S[i] = S;
    d.begin[i + 1] = d.begin[i] + (int)blocks;
    d.n = i + 1;
    return 0;
  }
};

// The weight gradients of n layers in ONE launch per 16 problems (wgrad_x6_batch_kernel): problem i is what
// gkg_linear_wgrad_x6(p[i].dy, ..., p[i].nb) would compute — every dw ZERO on entry.  Problems whose rows are not whole
// 128-row units / 16-byte aligned fall back to their own launches, in the plan's order between the group launches.
// DET: every problem's slab images in the workspace, then every dw in slab order (X6WdetReducer).
template <bool DET>
static int x6w_batch_run(const GkgWgradProblem* p, int n, int units_per_slab, void* workspace, size_t workspace_bytes, hipStream_t st) {
  X6WgradBatchPlan bp;
  const char* msg = nullptr;
  int rc = x6_wgrad_batch_plan(p, n, units_per_slab, DET, &bp, &msg);
  if (rc) return gkg_fail(rc, msg);
  if (DET && (!workspace || ((size_t)workspace & 15) || workspace_bytes < ((bp.det_floats * 4 + 15) & ~(size_t)15)))
    return gkg_fail(GKG_ERR_WORKSPACE, "gkg_linear_wgrad_x6_batch_det: workspace NULL, not 16-byte aligned or below gkg_linear_wgrad_x6_batch_det_workspace_bytes()");
  X6WgradBatchDet b{};
  auto flush = [&]() -> int {
    if (b.b.n == 0) return 0;
    hipError_t e = DET ? x6_kernel_once<wgrad_x6_batch_det_kernel>(X6W_SH_WIDE) : x6_kernel_once<wgrad_x6_batch_kernel>(X6W_SH_WIDE);
    if (e != hipSuccess) return gkg_fail_hip(e, DET ? "wgrad_x6 deterministic kernel (attribute)" : "wgrad_x6 batch kernel (attribute)");
    if constexpr (DET) hipLaunchKernelGGL(wgrad_x6_batch_det_kernel, dim3(b.b.begin[b.b.n]), dim3(256), X6W_SH_WIDE, st, b);
    else hipLaunchKernelGGL(wgrad_x6_batch_kernel, dim3(b.b.begin[b.b.n]), dim3(256), X6W_SH_WIDE, st, b.b);
    e = hipGetLastError();
    b.b.n = 0;
    return e == hipSuccess ? 0 : gkg_fail_hip(e, DET ? "wgrad_x6_batch_det_kernel" : "wgrad_x6_batch_kernel");
  };
  float* cur = (float*)workspace;
  for (int oi = 0; oi < n; ++oi) {
    const GkgWgradProblem& q = p[bp.order[oi]];
    const X6WgradPlan& pl = bp.pl[oi];
    const X6WgradCall qc = x6w_call(q);
    const size_t E = (size_t)q.nb * q.cout * q.cin;
    float* C = DET ? cur : q.dw;
    if (const int i = bp.slot[oi]; i >= 0) {
      b.b.p[i] = x6w_bind(qc, pl, pl.main, q.dy, q.x, C);
      b.b.p[i].rot = bp.rot[oi];
      b.b.wide[i] = pl.wide ? 1 : 0; b.b.gridx[i] = pl.main.grid_x; b.sstride[i] = E;
      b.b.begin[i + 1] = bp.end[oi];
      b.b.n = i + 1;
      if (b.b.n == X6W_BATCH && (rc = flush())) return rc;
    }
    if (pl.rest.rows > 0 &&
        (rc = x6w_launch_rest<DET>(x6w_bind(qc, pl, pl.rest, q.dy, q.x, C + (DET ? (size_t)pl.main_slabs() * E : 0)), pl.rest.grid_x, q.nb, E, st)))
      return rc;
    if (DET) cur += (size_t)pl.slabs() * E;
  }
  if ((rc = flush())) return rc;
  if constexpr (DET) {
    X6WdetReducer red;
    red.st = st;
    cur = (float*)workspace;
    for (int oi = 0; oi < n; ++oi) {
      const GkgWgradProblem& q = p[bp.order[oi]];
      const size_t E = (size_t)q.nb * q.cout * q.cin;
      const int S = bp.pl[oi].slabs();
      if ((rc = red.add(q.dw, cur, E, S))) return rc;
      cur += (size_t)S * E;
    }
    return red.flush();
  }
  return 0;
}
}  // namespace gkg

extern "C" int gkg_linear_wgrad_x6(const float* dy, int ldg, size_t g_bstride, const float* x, int ldx, size_t x_bstride,
                                   float* dw, int R, int cin, int cout, int nb, int kperm, void* stream) {
  if (!dy || !x || !dw) return gkg_fail(GKG_ERR_NULL, "gkg_linear_wgrad_x6: null pointer");
  const X6WgradCall q = x6w_call(dy, ldg, g_bstride, x, ldx, x_bstride, R, cin, cout, nb, kperm, 0);
  X6WgradPlan pl;
  const char* msg = nullptr;
  if (const int rc = x6_wgrad_plan(q, &pl, &msg)) return gkg_fail(rc, msg);
  return x6w_run<false>(q, pl, dy, x, dw, 0, (hipStream_t)stream);
}

extern "C" int gkg_linear_wgrad_x6_batch(const GkgWgradProblem* p, int n, int units_per_slab, void* stream) {
  return x6w_batch_run<false>(p, n, units_per_slab, nullptr, 0, (hipStream_t)stream);
}

extern "C" size_t gkg_linear_wgrad_x6_det_workspace_bytes(int R, int cin, int cout, int nb, int ldg, int ldx, int slabs) {
  if (slabs < 0 || slabs > 4096 || !x6_wdet_elems_ok(cin, cout, nb)) return 0;
  int rc = 0;
  const char* msg = nullptr;
  const int S = x6_wdet_max_slabs(R, cin, cout, nb, ldg, ldx, slabs, &rc, &msg);
  if (rc) gkg_fail(rc, msg);
  return ((size_t)S * nb * cout * cin * 4 + 15) & ~(size_t)15;
}

extern "C" int gkg_linear_wgrad_x6_det_slabs(int R, int cin, int cout, int nb, int ldg, int ldx, int aligned, int units_per_slab,
                                             int slabs, int* first_row, int* rows, int cap) {
  if (slabs < 0 || slabs > 4096 || units_per_slab < 0 || units_per_slab > 4096)
    return gkg_fail(GKG_ERR_SHAPE, "gkg_linear_wgrad_x6_det_slabs: slabs / units_per_slab out of range");
  if (cap > 0 && (!first_row || !rows)) return gkg_fail(GKG_ERR_NULL, "gkg_linear_wgrad_x6_det_slabs: null pointer");
  if (!x6_wdet_elems_ok(cin, cout, nb) && cin > 0 && cout > 0 && nb > 0)
    return gkg_fail(GKG_ERR_UNSUPPORTED, "gkg_linear_wgrad_x6_det: more than 2^31 elements of dw");
  X6WgradPlan pl;
  const char* msg = nullptr;
  if (const int rc = x6_wgrad_plan(X6WgradCall{R, cin, cout, nb, ldg, ldx, 0, 0, aligned != 0, units_per_slab, 0,
                                               units_per_slab > 0 ? 0 : slabs}, &pl, &msg))
    return gkg_fail(rc, msg);
  const int n = pl.slabs();
  for (int s = 0; s < n && s < cap; ++s) pl.slab_rows(s, first_row + s, rows + s);
  return n;
}

extern "C" int gkg_linear_wgrad_x6_det(const float* dy, int ldg, size_t g_bstride, const float* x, int ldx, size_t x_bstride,
                                       float* dw, int R, int cin, int cout, int nb, int kperm, int slabs, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  if (slabs < 0 || slabs > 4096) return gkg_fail(GKG_ERR_SHAPE, "gkg_linear_wgrad_x6_det: slabs out of range (0 .. 4096)");
  if (!dy || !x || !dw) return gkg_fail(GKG_ERR_NULL, "gkg_linear_wgrad_x6: null pointer");
  const X6WgradCall q = x6w_call(dy, ldg, g_bstride, x, ldx, x_bstride, R, cin, cout, nb, kperm, slabs);
  X6WgradPlan pl;
  const char* msg = nullptr;
  int rc = x6_wgrad_plan(q, &pl, &msg);
  if (rc) return gkg_fail(rc, msg);
  if (!x6_wdet_elems_ok(cin, cout, nb)) return gkg_fail(GKG_ERR_UNSUPPORTED, "gkg_linear_wgrad_x6_det: more than 2^31 elements of dw");
  const size_t need = gkg_linear_wgrad_x6_det_workspace_bytes(R, cin, cout, nb, ldg, ldx, slabs);
  if (!workspace || ((size_t)workspace & 15) || workspace_bytes < need || need == 0)
    return gkg_fail(GKG_ERR_WORKSPACE, "gkg_linear_wgrad_x6_det: workspace NULL, not 16-byte aligned or below gkg_linear_wgrad_x6_det_workspace_bytes()");
  hipStream_t st = (hipStream_t)stream;
  const size_t E = (size_t)nb * cout * cin;
  if ((rc = x6w_run<true>(q, pl, dy, x, (float*)workspace, E, st))) return rc;
  X6WdetReducer red;
  red.st = st;
  if ((rc = red.add(dw, (const float*)workspace, E, pl.slabs()))) return rc;
  return red.flush();
}

extern "C" size_t gkg_linear_wgrad_x6_batch_det_workspace_bytes(const GkgWgradProblem* p, int n, int units_per_slab) {
  X6WgradBatchPlan bp;
  const char* msg = nullptr;
  if (const int rc = x6_wgrad_batch_plan(p, n, units_per_slab, true, &bp, &msg)) { gkg_fail(rc, msg); return 0; }
  return (bp.det_floats * 4 + 15) & ~(size_t)15;
}

extern "C" int gkg_linear_wgrad_x6_batch_det(const GkgWgradProblem* p, int n, int units_per_slab, void* workspace,
                                             size_t workspace_bytes, void* stream) {
  return x6w_batch_run<true>(p, n, units_per_slab, workspace, workspace_bytes, (hipStream_t)stream);
}

