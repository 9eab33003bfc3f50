// Micro-benchmark: which VALU / LDS instructions hide in the shadow of v_mfma_f32_32x32x16_bf16 (one wave per SIMD)?
// Each variant runs 12 x { MFMA ; fillers } per iteration from one asm block, so the order is exactly as written.
#include <hip/hip_runtime.h>
#include <cstdio>
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define MF "v_mfma_f32_32x32x16_bf16 %[c0], %[a], %[b], %[c0]\n\t"
#define MF2 "v_mfma_f32_32x32x16_bf16 %[c1], %[a], %[b], %[c1]\n\t"
#define ADD4 "v_add_f32 %[v0], %[v0], %[c]\n\tv_add_f32 %[v1], %[v1], %[c]\n\tv_add_f32 %[v2], %[v2], %[c]\n\tv_add_f32 %[v3], %[v3], %[c]\n\t"
#define ADD2 "v_add_f32 %[v0], %[v0], %[c]\n\tv_add_f32 %[v1], %[v1], %[c]\n\t"
// the split chain on (%4,%5) -> packed in %6, residuals back in %4,%5
#define CHAIN "v_cvt_pk_bf16_f32 %[v2], %[v0], %[v1]\n\tv_lshlrev_b32 %[v3], 16, %[v2]\n\tv_and_b32 %[t], 0xffff0000, %[v2]\n\tv_sub_f32 %[v0], %[v0], %[v3]\n\tv_sub_f32 %[v1], %[v1], %[t]\n\t"
// CHAINPK, the same chain with ONE v_pk_add_f32 %[p], %[p], %[q] neg_lo:[0,1] neg_hi:[0,1] for the two subtractions, needs (v0, v1) and
// (v3, t) as 64-bit pairs: it is timed by ksplit<true> below, against ksplit<false>, in the weight-gradient loop's own layout.
#define DSR "ds_read_b128 %[d], %[addr]\n\t"
#define R6(x) x x x x x x
#define R12(x) R6(x) R6(x)

template <int V>
__global__ __launch_bounds__(256) void k(float* out, int iters) {
  __shared__ float4 sm[1024];
  const int lane = threadIdx.x & 63;
  sm[threadIdx.x] = float4{1.f, 2.f, 3.f, 4.f};
  __syncthreads();
  f32x16 acc0 = {0}, acc1 = {0};
  f32x4 a = {lane * 0.001f, 1.f, 2.f, 3.f}, b = {1.0f, lane * 1e-4f, 0.5f, 0.25f};
  float v0 = lane, v1 = lane + 1.f, v2 = lane + 2.f, v3 = lane + 3.f, c = 1e-3f, t = 0.f;
  f32x4 d = {0, 0, 0, 0};
  const unsigned addr = (threadIdx.x & 255) * 16;
  for (int it = 0; it < iters; ++it) {
    if (V == 0) asm volatile(R12(MF) : [c0] "+v"(acc0), [c1] "+v"(acc1), [v0] "+v"(v0), [v1] "+v"(v1), [v2] "+v"(v2), [v3] "+v"(v3), [t] "+v"(t), [d] "+v"(d) : [a] "v"(a), [b] "v"(b), [c] "v"(c), [addr] "v"(addr));
    if (V == 1) asm volatile(R12(MF ADD4) : [c0] "+v"(acc0), [c1] "+v"(acc1), [v0] "+v"(v0), [v1] "+v"(v1), [v2] "+v"(v2), [v3] "+v"(v3), [t] "+v"(t), [d] "+v"(d) : [a] "v"(a), [b] "v"(b), [c] "v"(c), [addr] "v"(addr));
    if (V == 2) asm volatile(R12(MF ADD4 ADD2) : [c0] "+v"(acc0), [c1] "+v"(acc1), [v0] "+v"(v0), [v1] "+v"(v1), [v2] "+v"(v2), [v3] "+v"(v3), [t] "+v"(t), [d] "+v"(d) : [a] "v"(a), [b] "v"(b), [c] "v"(c), [addr] "v"(addr));
    if (V == 3) asm volatile(R12(MF CHAIN) : [c0] "+v"(acc0), [c1] "+v"(acc1), [v0] "+v"(v0), [v1] "+v"(v1), [v2] "+v"(v2), [v3] "+v"(v3), [t] "+v"(t), [d] "+v"(d) : [a] "v"(a), [b] "v"(b), [c] "v"(c), [addr] "v"(addr));
    if (V == 4) asm volatile(R12(MF ADD4 ADD4) : [c0] "+v"(acc0), [c1] "+v"(acc1), [v0] "+v"(v0), [v1] "+v"(v1), [v2] "+v"(v2), [v3] "+v"(v3), [t] "+v"(t), [d] "+v"(d) : [a] "v"(a), [b] "v"(b), [c] "v"(c), [addr] "v"(addr));
    if (V == 5) asm volatile(R12(MF DSR) "s_waitcnt lgkmcnt(0)\n\t" : [c0] "+v"(acc0), [c1] "+v"(acc1), [v0] "+v"(v0), [v1] "+v"(v1), [v2] "+v"(v2), [v3] "+v"(v3), [t] "+v"(t), [d] "+v"(d) : [a] "v"(a), [b] "v"(b), [c] "v"(c), [addr] "v"(addr));
    if (V == 6) asm volatile(R12(MF CHAIN DSR) "s_waitcnt lgkmcnt(0)\n\t" : [c0] "+v"(acc0), [c1] "+v"(acc1), [v0] "+v"(v0), [v1] "+v"(v1), [v2] "+v"(v2), [v3] "+v"(v3), [t] "+v"(t), [d] "+v"(d) : [a] "v"(a), [b] "v"(b), [c] "v"(c), [addr] "v"(addr));
    if (V == 7) asm volatile(R6(MF MF2) : [c0] "+v"(acc0), [c1] "+v"(acc1), [v0] "+v"(v0), [v1] "+v"(v1), [v2] "+v"(v2), [v3] "+v"(v3), [t] "+v"(t), [d] "+v"(d) : [a] "v"(a), [b] "v"(b), [c] "v"(c), [addr] "v"(addr));
    if (V == 8) asm volatile(R12(CHAIN) : [c0] "+v"(acc0), [c1] "+v"(acc1), [v0] "+v"(v0), [v1] "+v"(v1), [v2] "+v"(v2), [v3] "+v"(v3), [t] "+v"(t), [d] "+v"(d) : [a] "v"(a), [b] "v"(b), [c] "v"(c), [addr] "v"(addr));
    if (V == 9) asm volatile(R12(MF "s_nop 7\n\ts_nop 7\n\t") : [c0] "+v"(acc0), [c1] "+v"(acc1), [v0] "+v"(v0), [v1] "+v"(v1), [v2] "+v"(v2), [v3] "+v"(v3), [t] "+v"(t), [d] "+v"(d) : [a] "v"(a), [b] "v"(b), [c] "v"(c), [addr] "v"(addr));
  }
  float s = v0 + v1 + v2 + v3 + d.x + t;
#pragma unroll
  for (int i = 0; i < 16; ++i) s += acc0[i] + acc1[i];
  out[blockIdx.x * 256 + threadIdx.x] = s;
}

// The weight-gradient loop's own stream (gkg_gemm_x6.hip, wide body), written the way that kernel writes it: single-instruction
// asm volatile steps between MFMA builtins, four pairs interleaved, the next raw values read from LDS at the end of a trip.  One
// trip = 16 MFMAs and the split of two 8-float fragments: 88 steps (5.5 per gap) with two v_sub_f32 per residual pair, 72 (4.5 per
// gap) with one v_pk_add_f32 (CHAINPK above; the pairs are 64-bit values from the LDS read on, so no v_mov forms them).
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

template <bool PK, int I>
__device__ __forceinline__ void split_op(f32x2 (&x)[2][4], u32x4 (&fn)[2][3], f32x2 (&t)[4]) {
  constexpr int PER = PK ? 36 : 44, blk = I / PER, u = I % PER, p = u & 3, o = u >> 2;
  constexpr int lvl = PK ? o / 4 : o / 5, k = PK ? o % 4 : o % 5;
  unsigned w;
  float a;
  if constexpr (k == 0) { asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(w) : "v"(x[blk][p].x), "v"(x[blk][p].y)); fn[blk][lvl][p] = w; }
  if constexpr (k == 1) { asm volatile("v_lshlrev_b32 %0, 16, %1" : "=v"(a) : "v"(fn[blk][lvl][p])); t[p].x = a; }
  if constexpr (k == 2) { asm volatile("v_and_b32 %0, 0xffff0000, %1" : "=v"(a) : "v"(fn[blk][lvl][p])); t[p].y = a; }
  if constexpr (PK) {
    if constexpr (k == 3) asm volatile("v_pk_add_f32 %0, %0, %1 neg_lo:[0,1] neg_hi:[0,1]" : "+v"(x[blk][p]) : "v"(t[p]));
  } else {
    if constexpr (k == 3) asm volatile("v_sub_f32 %0, %0, %1" : "+v"(x[blk][p].x) : "v"(t[p].x));
    if constexpr (k == 4) asm volatile("v_sub_f32 %0, %0, %1" : "+v"(x[blk][p].y) : "v"(t[p].y));
  }
}
template <bool PK, int I, int END>
__device__ __forceinline__ void split_ops(f32x2 (&x)[2][4], u32x4 (&fn)[2][3], f32x2 (&t)[4]) {
  if constexpr (I < END) { split_op<PK, I>(x, fn, t); split_ops<PK, I + 1, END>(x, fn, t); }
}
template <bool PK, int SI>
__device__ __forceinline__ void split_slots(const u32x4 (&fc)[2][3], u32x4 (&fn)[2][3], f32x16 (&acc)[4], f32x2 (&x)[2][4], f32x2 (&t)[4]) {
  if constexpr (SI < 16) {
    constexpr int N = PK ? 72 : 88;
    acc[SI & 3] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fc[0][SI % 3]), __builtin_bit_cast(bf16x8, fc[1][(SI / 3) % 3]), acc[SI & 3], 0, 0, 0);
    split_ops<PK, SI * N / 16, (SI + 1) * N / 16>(x, fn, t);
    __builtin_amdgcn_sched_barrier(0);
    split_slots<PK, SI + 1>(fc, fn, acc, x, t);
  }
}

template <bool PK>
__global__ __launch_bounds__(256) void ksplit(float* out, int iters) {
  __shared__ float sm[4608];
  for (int i = threadIdx.x; i < 4608; i += 256) sm[i] = 1.0f + 1e-3f * (float)((i * 37) & 1023);
  __syncthreads();
  const float* base = sm + (threadIdx.x & 255);
  f32x16 acc[4];
  for (int i = 0; i < 4; ++i) for (int q = 0; q < 16; ++q) acc[i][q] = 0.f;
  f32x2 x[2][4], t[4];
  u32x4 f0[2][3], f1[2][3];
  // rows 2p and 2p + 1 (pitch 64 floats) of a column land in ONE aligned register pair: written out as ds_read2_b32, because left
  // to itself the compiler pairs the two blocks of a row instead and then moves every value into place
  auto rd = [&](int it) __attribute__((always_inline)) {
    const unsigned b = (unsigned)(size_t)(base + (it & 1) * 2048);
#pragma unroll
    for (int blk = 0; blk < 2; ++blk)
#pragma unroll
      for (int p = 0; p < 4; ++p)
        asm volatile("ds_read2_b32 %0, %1 offset0:%2 offset1:%3" : "=v"(x[blk][p]) : "v"(b + (p >> 1) * 1024), "n"(blk * 32 + (2 * (p & 1)) * 64), "n"(blk * 32 + (2 * (p & 1) + 1) * 64));
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  };
  rd(0);
  split_ops<PK, 0, PK ? 72 : 88>(x, f0, t);
  rd(1);
  for (int it = 0; it < iters; it += 2) {
    split_slots<PK, 0>(f0, f1, acc, x, t);
    rd(it);
    split_slots<PK, 0>(f1, f0, acc, x, t);
    rd(it + 1);
  }
  float s = f0[0][0][0] + f1[1][2][3];
  for (int i = 0; i < 4; ++i) for (int q = 0; q < 16; ++q) s += acc[i][q];
  out[blockIdx.x * 256 + threadIdx.x] = s;
}

template <bool PK>
void run_split(const char* name, float* out) {
  hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
  const int iters = 4000;
  ksplit<PK><<<256, 256>>>(out, 10);
  hipDeviceSynchronize();
  for (int rep = 0; rep < 3; ++rep) {
    hipEventRecord(e0);
    ksplit<PK><<<256, 256>>>(out, iters);
    hipEventRecord(e1); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1);
    printf("%-44s %8.1f ns / 16 slots  = %6.1f ns per slot\n", name, ms * 1e6 / iters, ms * 1e6 / iters / 16);
  }
}

template <int V>
void run(const char* name, float* out) {
  hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
  const int iters = 4000;
  k<V><<<256, 256>>>(out, 10);
  hipDeviceSynchronize();
  hipEventRecord(e0);
  k<V><<<256, 256>>>(out, iters);
  hipEventRecord(e1); hipEventSynchronize(e1);
  float ms; hipEventElapsedTime(&ms, e0, e1);
  printf("%-44s %8.1f ns / 12 slots  = %6.1f ns per slot\n", name, ms * 1e6 / iters, ms * 1e6 / iters / 12);
}

int main() {
  float* out; hipMalloc(&out, 256 * 256 * sizeof(float));
  run<0>("12 MFMA (one chain)", out);
  run<7>("12 MFMA (two chains)", out);
  run<9>("MFMA + 2 s_nop 7", out);
  run<1>("MFMA + 4 v_add_f32", out);
  run<2>("MFMA + 6 v_add_f32", out);
  run<4>("MFMA + 8 v_add_f32", out);
  run<3>("MFMA + split chain (5 dependent VALU)", out);
  run<8>("split chain only (5 VALU)", out);
  run<5>("MFMA + ds_read_b128", out);
  run<6>("MFMA + split chain + ds_read_b128", out);
  run_split<false>("wgrad stream, 5.5 / gap (2 v_sub_f32)", out);
  run_split<true>("wgrad stream, 4.5 / gap (v_pk_add_f32)", out);
  return 0;
}
