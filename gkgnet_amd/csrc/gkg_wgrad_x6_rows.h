// The register-load weight-gradient kernel (gkg_gemm_x6.hip has its description), compiled in two forms:
//   X6W_DET 0   wgrad_x6_kernel: one fp32 atomic per element into the zeroed dW
//   X6W_DET 1   wgrad_x6_det_kernel: the workgroup stores its tile of slab `split` into image `split` of a workspace (g.C: image 0
//               of this launch, `sstride` floats per image) for the ordered reduction of gkg_linear_wgrad_x6_det
// Included inside namespace gkg, behind X6WgradArgs and the x6w_* helpers; no include guard: the text is the kernel.
#if X6W_DET
__global__ __launch_bounds__(256) void wgrad_x6_det_kernel(X6WgradArgs g, size_t sstride) {
#else
__global__ __launch_bounds__(256) void wgrad_x6_kernel(X6WgradArgs g) {
#endif
  __shared__ float red[4 * 64 * 64];
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int z = blockIdx.y;
  // XCD-aware: the tiles of one row slab run on one XCD (its rows are fetched into that L2 once)
  const int ntile = g.mtiles * g.ntiles;
  const int lin = blockIdx.x, xcd = lin & 7, slot = lin >> 3;
  const int split = (slot / ntile) * 8 + xcd, tile = slot % ntile;
  if (split >= g.splits) return;
  const int m0 = (tile / g.ntiles) * 64, n0 = (tile % g.ntiles) * 64;
  const int r = lane & 31, h = lane >> 5;
  const int rows_per_wave = g.rows_per_split >> 2;
  const long long k_begin = (long long)split * g.rows_per_split + (long long)w * rows_per_wave;
  const int T = rows_per_wave >> 4;                                  // 16-row steps of this wave (even)
  const char* Az = (const char*)(g.A + (size_t)z * g.a_bstride);
  const char* Bz = (const char*)(g.B + (size_t)z * g.b_bstride);
  const long long abytes = (long long)g.K * g.lda * 4, bbytes = (long long)g.K * g.ldb * 4;

  // per-lane byte offset of each fragment's first row (8 h) at its column; the 8 rows j of a fragment come from 8
  // descriptors whose base is advanced by j rows (so the hardware range check stays exact at the end of the tensor);
  // columns outside the matrix get an offset no range check passes
  unsigned off[4];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int ca = m0 + 32 * i + r, cb = n0 + 32 * i + r;
    off[i] = ca < g.M ? (unsigned)((8 * h * g.lda + ca) * 4) : 0xfffffff0u;
    off[2 + i] = cb < g.N ? (unsigned)((8 * h * g.ldb + cb) * 4) : 0xfffffff0u;
  }
  auto load = [&](float (&raw)[4][8], int s) __attribute__((always_inline)) {
    const long long row0 = k_begin + 16ll * s;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const long long ao = (row0 + j) * g.lda * 4, bo = (row0 + j) * g.ldb * 4;
      const long long ra_ = abytes - ao, rb_ = bbytes - bo;
      const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void*)(Az + (ra_ > 0 ? ao : 0)), 0,
                                                                          (int)(ra_ > 0 ? (ra_ > 0x7fffffffll ? 0x7fffffffll : ra_) : 0), 0x00020000);
      const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc((void*)(Bz + (rb_ > 0 ? bo : 0)), 0,
                                                                          (int)(rb_ > 0 ? (rb_ > 0x7fffffffll ? 0x7fffffffll : rb_) : 0), 0x00020000);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        raw[i][j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ra, off[i], 0, 0));
        raw[2 + i][j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rb, off[2 + i], 0, 0));
      }
    }
  };
  float raw0[4][8], raw1[4][8];                 // raw fragments two 16-row steps deep
  X6WFrag fr0, fr1;
  unsigned t0[4], t1[4];
  x6_f32x16 acc[2][2], accs[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int q = 0; q < 16; ++q) { acc[i][j][q] = 0.f; accs[i][j][q] = 0.f; }

  // one 16-row step s: MFMAs on `fc`; the gaps split `rs` (step s + 1) into `fn`; then `rs` is reloaded for step s + 3.
  // The last step (no split) is peeled out of the loop: two variants of the MFMA chain inside it would put the
  // accumulators behind phi nodes (the register allocator then copies whole tiles per MFMA).
  load(raw0, 0);
  if (T > 1) load(raw1, 1);
  x6w_ops<0, 176>(raw0, fr0, t0, t1);
  if (T > 2) load(raw0, 2);
  for (int s = 0; s + 2 < T; s += 2) {          // buffer roles alternate: 2 steps per trip (T is even)
    x6w_slots<0, true>(fr0, fr1, acc, accs, raw1, t0, t1);       // step s: splits step s+1 (raw1) ...
    if (s + 3 < T) load(raw1, s + 3);                             // ... then raw1 <- step s+3
    x6w_slots<0, true>(fr1, fr0, acc, accs, raw0, t0, t1);       // step s+1: splits step s+2 (raw0)
    if (s + 4 < T) load(raw0, s + 4);
  }
  x6w_slots<0, true>(fr0, fr1, acc, accs, raw1, t0, t1);         // step T-2
  x6w_slots<0, false>(fr1, fr0, acc, accs, raw0, t0, t1);        // step T-1

  // ---- the four waves' tiles -> LDS -> one atomic add per element
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
    if (m0 + row < g.M && n0 + col < g.N)
#if X6W_DET
      C[(size_t)split * sstride + (size_t)(m0 + row) * g.ldc + (g.kperm ? x6_kperm_src(n0 + col, g.N) : n0 + col)] = v;
#else
      __hip_atomic_fetch_add(C + (size_t)(m0 + row) * g.ldc + (g.kperm ? x6_kperm_src(n0 + col, g.N) : n0 + col), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
  }
}
