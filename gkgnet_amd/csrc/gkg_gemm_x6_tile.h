// gkg_gemm_x6_tile.h — the 128-row tile kernel of gkg_gemm_x6.hip (its head comment describes the kernel), included there TWICE:
//   X6_WALK 0   gemm_x6_kernel        one tile per workgroup.  Every line outside the #if X6_WALK sections is this form's, so a
//                                     change to the other form cannot move its code;
//   X6_WALK 1   gemm_x6_walk_kernel   the form for launches of two rounds of resident workgroups (round 11; the rule and its
//       numbers: x6_walk_grid): the grid is one round and a workgroup runs a LIST of tiles, a pure function of blockIdx.x — no counter, no atomics, no
//       workgroup waits for another, and all four waves walk the same list, so every barrier is met by all.  XCD x (workgroups
//       lin & 7 == x) owns the row blocks u = z * mtiles + tm (batches folded in) with u & 7 == x; its sequence is those blocks in
//       order, the column tiles of a block back to back, and workgroup i = lin >> 3 takes entries i, i + W, i + 2 W, ...
//       (W = gridDim.x / 8) — the column tiles of one row block still run side by side on one XCD.  The (tile, K-step) pairs of the
//       list are ONE stream of stages: ring slots follow the running stage number (A: mod 3, B: parity), and the DMA calls of a
//       tile's last K-steps already fetch the next tile's first stages (further ahead when a tile has fewer than three K-steps),
//       which land under the epilogue.  The epilogue's LDS scratch therefore has its own region behind the rings, and a tile ends
//       with vmcnt(0) + barrier: the epilogue's loads and stores share vmcnt with the DMA pieces.  A tile's arithmetic is the
//       one-tile form's, instruction for instruction: the same bits.  Un-split contractions only (ksplit == 1), and not the
//       X6_BNBWD epilogue (measured slower walking; its LDS scratch still aliases the rings).
template <int NI, int EPI, int BN = 32 * NI>
#if X6_WALK
__global__ __launch_bounds__(256, 2) void gemm_x6_walk_kernel(X6Args g) {       // two workgroups per CU, as the one-tile form
#else
__global__ __launch_bounds__(256) void gemm_x6_kernel(X6Args g) {
#endif
  static_assert(BN <= 32 * NI && BN > 32 * (NI - 1) && BN % 16 == 0 && (12 * BN * 16) % 1024 == 0, "tile width");
#if X6_WALK
  static_assert(EPI != X6_BNBWD, "no walk form of the BN-backward statistics epilogue");
#endif
  constexpr int BM = 128, BK = 32, SA = 3;
  constexpr bool PARTIAL = BN != 32 * NI;                // lanes r >= BN - 32 (NI - 1) of the last block hold no column
  constexpr int A_STAGE = 4 * 4096, B_STAGE = 12 * BN * 16, B_BASE = SA * A_STAGE;
  constexpr int PIECES = 12 * BN * 16 / 1024;            // 1-KiB pieces of one B stage image
  constexpr int BI = (PIECES + 3) / 4;                   // ... per wave per K-step (wave w: pieces w, w+4, ...), and the
  constexpr int BI_MIN = PIECES / 4;                     // fewest any wave issues: what the counted waits may assume
  extern __shared__ uint4 lds[];
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
#if X6_WALK
  // entry p of this XCD's sequence -> (z, tm, tn); the workgroup owns entries slot + e * walk_w, e < ntile
  const int lin = blockIdx.x, xcd = lin & 7, slot = lin >> 3, walk_w = gridDim.x >> 3;
  auto walk_tile = [&](int e, int& wz, int& wtm, int& wtn) {
    const int p = slot + e * walk_w, j = p / g.ntiles, u = j * 8 + xcd;
    wtn = p - j * g.ntiles; wz = u / g.mtiles; wtm = u - wz * g.mtiles;
  };
  const int ntile = (((g.walk_nb * g.mtiles - xcd + 7) >> 3) * g.ntiles - slot + walk_w - 1) / walk_w;
  if (ntile <= 0) return;
  int z, tm, tn;
  walk_tile(0, z, tm, tn);
  int m0 = tm * BM, n0 = tn * BN;
  const int M = g.M, N = g.N, K = g.K;
#else
  const int z = blockIdx.y;
  const int lin = blockIdx.x, xcd = lin & 7, slot = lin >> 3;
  // the column tiles and the K splits of one 128-row block run back to back on one XCD
  const int per_row = g.ntiles * g.ksplit, inner = slot % per_row;
  const int tn = inner % g.ntiles, ks = inner / g.ntiles, tm = (slot / per_row) * 8 + xcd;
  if (tm >= g.mtiles) return;
  const int m0 = tm * BM, n0 = tn * BN;
  const int M = g.M, N = g.N;
  const int K = g.ksplit > 1 ? min(g.K - ks * g.kper * BK, g.kper * BK) : g.K;       // this workgroup's share of the contraction
  const float* A = g.A + (size_t)z * g.a_bstride + (size_t)ks * g.kper * BK;
  const uint4* P = g.P + (size_t)z * g.p_bstride + (size_t)ks * g.kper * 4 * g.NP;
#endif
  const unsigned lds0 = (unsigned)(size_t)lds;
  const int nk = (K + BK - 1) / BK;
  const bool ktail = (K & (BK - 1)) != 0;
#if X6_WALK
  const int nstage = ntile * nk;                         // the length of the workgroup's stage stream ...
  int sbase = 0;                                         // ... and the stream number of the current tile's first K-step
#endif

  // A pieces: LDS slot L = 64 i + lane of the wave's 32 x 128-B image holds chunk (L & 7) ^ ((row >> 1) & 7) of row L >> 3
  unsigned aoff[4];
  int achunk[4];
#if X6_WALK
  auto set_aoff = [&](int am0) {                         // aoff belongs to the tile being FETCHED
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int L = 64 * i + lane, row = L >> 3, chunk = (L & 7) ^ ((row >> 1) & 7);
      const int gr = min(am0 + 32 * w + row, M - 1);
      aoff[i] = (unsigned)((size_t)gr * g.lda + chunk * 4) * 4u;
      achunk[i] = chunk;
    }
  };
  set_aoff(m0);
#else
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int L = 64 * i + lane, row = L >> 3, chunk = (L & 7) ^ ((row >> 1) & 7);
    const int gr = min(m0 + 32 * w + row, M - 1);        // rows past the end re-read the last row (never stored)
    aoff[i] = (unsigned)((size_t)gr * g.lda + chunk * 4) * 4u;
    achunk[i] = chunk;
  }
#endif
  const size_t plane = (size_t)g.KC * g.NP * 16;
  // B pieces: slot s = 64 piece + lane of the stage image [3 planes][4 chunks][BN] holds n = s % BN of row s / BN (a piece
  // may straddle two rows when BN is not a multiple of 64: the source address is per lane, the destination linear)
  unsigned boff[BI];
#pragma unroll
  for (int i = 0; i < BI; ++i) {
    const int sidx = (w + 4 * i) * 64 + lane, rowid = sidx / BN, n = sidx - rowid * BN, p = rowid >> 2, chunk = rowid & 3;
#if X6_WALK
    boff[i] = (unsigned)(p * plane + ((size_t)chunk * g.NP + n) * 16);          // n0 rides in the fetch cursor's base
#else
    boff[i] = (unsigned)(p * plane + ((size_t)chunk * g.NP + n0 + n) * 16);
#endif
  }
#if X6_WALK
  // The two fetch cursors of the stream: each call issues the cursor's stage (K-step c?_k of its tile, ring slot by the stream
  // number c?_s) and moves on, into the next tile of the list behind a tile's last K-step.
  int ca_e = 0, ca_k = 0, ca_s = 0, cb_e = 0, cb_k = 0, cb_s = 0;
  const float* ca_A = g.A + (size_t)z * g.a_bstride;
  const uint4* cb_P = g.P + (size_t)z * g.p_bstride + n0;
  auto dma_a = [&]() {
    const int kt = ca_k;
    const char* base = (const char*)ca_A + (size_t)kt * (BK * 4);
    const unsigned dst = lds0 + (ca_s % SA) * A_STAGE + w * 4096;
    const bool last = ktail && kt == nk - 1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      unsigned o = aoff[i];
      if (last && kt * BK + achunk[i] * 4 >= K) o -= achunk[i] * 16;      // past K: a valid address, masked after the read
      x6_dma16(base, o, dst + i * 1024);
    }
    ++ca_s;
    if (++ca_k == nk) {
      int wz, wtm, wtn;
      ca_k = 0;
      walk_tile(++ca_e, wz, wtm, wtn);
      ca_A = g.A + (size_t)wz * g.a_bstride;
      set_aoff(wtm * BM);
    }
  };
  auto dma_b = [&]() {
    const char* base = (const char*)cb_P + (size_t)cb_k * 4 * g.NP * 16;
    const unsigned dst = lds0 + B_BASE + (cb_s & 1) * B_STAGE;
#pragma unroll
    for (int i = 0; i < BI; ++i)
      if ((i + 1) * 4 <= PIECES || w + 4 * i < PIECES) x6_dma16(base, boff[i], dst + (w + 4 * i) * 1024);
    ++cb_s;
    if (++cb_k == nk) {
      int wz, wtm, wtn;
      cb_k = 0;
      walk_tile(++cb_e, wz, wtm, wtn);
      cb_P = g.P + (size_t)wz * g.p_bstride + wtn * BN;
    }
  };
#else
  auto dma_a = [&](int kt) {
    const char* base = (const char*)A + (size_t)kt * (BK * 4);
    const unsigned dst = lds0 + (kt % SA) * A_STAGE + w * 4096;
    const bool last = ktail && kt == nk - 1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      unsigned o = aoff[i];
      if (last && kt * BK + achunk[i] * 4 >= K) o -= achunk[i] * 16;      // past K: a valid address, masked after the read
      x6_dma16(base, o, dst + i * 1024);
    }
  };
  auto dma_b = [&](int kt) {
    const char* base = (const char*)P + (size_t)kt * 4 * g.NP * 16;
    const unsigned dst = lds0 + B_BASE + (kt & 1) * B_STAGE;
#pragma unroll
    for (int i = 0; i < BI; ++i)
      if ((i + 1) * 4 <= PIECES || w + 4 * i < PIECES) x6_dma16(base, boff[i], dst + (w + 4 * i) * 1024);
  };
#endif

  x6_f32x16 acc[NI], accs[NI];
#pragma unroll
  for (int j = 0; j < NI; ++j)
#pragma unroll
    for (int q = 0; q < 16; ++q) { acc[j][q] = 0.f; accs[j][q] = 0.f; }

  const int r = lane & 31, h = lane >> 5, sw = (r >> 1) & 7;
  int ac[2][2];
#pragma unroll
  for (int s = 0; s < 2; ++s) { ac[s][0] = r * 128 + (((4 * s + 2 * h) ^ sw) << 4); ac[s][1] = r * 128 + (((4 * s + 2 * h + 1) ^ sw) << 4); }

  float f[8];                        // raw A fragment of the next half step, split in place
  unsigned sh_[4], sm_[4], sl_[4], t0_[4], t1_[4];
  x6_bf16x8 a[2][3], b[2][NI][3];

  auto read_raw = [&](int kt, int s) {
#if X6_WALK
    const char* ab = (const char*)lds + ((sbase + kt) % SA) * A_STAGE + w * 4096;
#else
    const char* ab = (const char*)lds + (kt % SA) * A_STAGE + w * 4096;
#endif
    const float4 f0 = *(const float4*)(ab + ac[s][0]);
    const float4 f1 = *(const float4*)(ab + ac[s][1]);
    f[0] = f0.x; f[1] = f0.y; f[2] = f0.z; f[3] = f0.w; f[4] = f1.x; f[5] = f1.y; f[6] = f1.z; f[7] = f1.w;
    if (ktail && kt == nk - 1) {
      const int kb = kt * BK + 16 * s + 8 * h;
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] = kb + j < K ? f[j] : 0.f;
    }
  };
  auto read_b = [&](int kt, int s, int buf) {
#if X6_WALK
    const uint4* bb = lds + (B_BASE + ((sbase + kt) & 1) * B_STAGE) / 16 + r;
#else
    const uint4* bb = lds + (B_BASE + (kt & 1) * B_STAGE) / 16 + r;
#endif
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int p = 0; p < 3; ++p) b[buf][j][p] = __builtin_bit_cast(x6_bf16x8, bb[(p * 4 + 2 * s + h) * BN + j * 32]);
  };
  // The split of f[] as 44 single-instruction steps (asm volatile: fixed order, never sunk into another block).  Step i
  // works on pair i & 3, so consecutive steps are independent.
  auto op = [&](int i) {
    const int p = i & 3, o = i >> 2;
    float& x0 = f[2 * p]; float& x1 = f[2 * p + 1];
    if (o == 0) asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(sh_[p]) : "v"(x0), "v"(x1));
    if (o == 1) asm volatile("v_lshlrev_b32 %0, 16, %1" : "=v"(t0_[p]) : "v"(sh_[p]));
    if (o == 2) asm volatile("v_and_b32 %0, 0xffff0000, %1" : "=v"(t1_[p]) : "v"(sh_[p]));
    if (o == 3) asm volatile("v_sub_f32 %0, %0, %1" : "+v"(x0) : "v"(t0_[p]));
    if (o == 4) asm volatile("v_sub_f32 %0, %0, %1" : "+v"(x1) : "v"(t1_[p]));
    if (o == 5) asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(sm_[p]) : "v"(x0), "v"(x1));
    if (o == 6) asm volatile("v_lshlrev_b32 %0, 16, %1" : "=v"(t0_[p]) : "v"(sm_[p]));
    if (o == 7) asm volatile("v_and_b32 %0, 0xffff0000, %1" : "=v"(t1_[p]) : "v"(sm_[p]));
    if (o == 8) asm volatile("v_sub_f32 %0, %0, %1" : "+v"(x0) : "v"(t0_[p]));
    if (o == 9) asm volatile("v_sub_f32 %0, %0, %1" : "+v"(x1) : "v"(t1_[p]));
    if (o == 10) asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(sl_[p]) : "v"(x0), "v"(x1));
  };
  auto commit = [&](int buf) {
    a[buf][0] = __builtin_bit_cast(x6_bf16x8, uint4{sh_[0], sh_[1], sh_[2], sh_[3]});
    a[buf][1] = __builtin_bit_cast(x6_bf16x8, uint4{sm_[0], sm_[1], sm_[2], sm_[3]});
    a[buf][2] = __builtin_bit_cast(x6_bf16x8, uint4{sl_[0], sl_[1], sl_[2], sl_[3]});
  };
  // One half step (16 deep): the MFMAs of buffer `cur`; in their gaps the NEXT half step's (stage nkt, half ns) B fragments
  // are read and its raw A fragment (read at the top) is split into buffer cur ^ 1.
  constexpr int SLOTS = 6 * NI, OPS_PER = (44 + SLOTS - 2) / (SLOTS - 1);
  auto half = [&](int cur, bool has_next, int nkt, int ns) {
#if X6_WALK
    const uint4* bb = lds + (B_BASE + ((sbase + nkt) & 1) * B_STAGE) / 16 + r;
#else
    const uint4* bb = lds + (B_BASE + (nkt & 1) * B_STAGE) / 16 + r;
#endif
    if (has_next) read_raw(nkt, ns);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < NI; ++j) {
#pragma unroll
      for (int t = 0; t < 6; ++t) {
        const int si = j * 6 + t;
        // small terms first, the hi*hi product into its own accumulator
        if (t == 0) accs[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[cur][2], b[cur][j][0], accs[j], 0, 0, 0);
        if (t == 1) accs[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[cur][0], b[cur][j][2], accs[j], 0, 0, 0);
        if (t == 2) accs[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[cur][1], b[cur][j][1], accs[j], 0, 0, 0);
        if (t == 3) accs[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[cur][1], b[cur][j][0], accs[j], 0, 0, 0);
        if (t == 4) accs[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[cur][0], b[cur][j][1], accs[j], 0, 0, 0);
        if (t == 5) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[cur][0], b[cur][j][0], acc[j], 0, 0, 0);
        if (has_next) {
          if (si < 3 * NI) {
            const int jj = si / 3, pp = si % 3;
            b[cur ^ 1][jj][pp] = __builtin_bit_cast(x6_bf16x8, bb[(pp * 4 + 2 * ns + h) * BN + jj * 32]);
          }
          if (si >= 1) {
#pragma unroll
            for (int o = 0; o < OPS_PER; ++o) { const int i = (si - 1) * OPS_PER + o; if (i < 44) op(i); }
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if (has_next) commit(cur ^ 1);
  };

  // ---- pipeline.  DMA issue order per wave: [A0] [B0] [A1] [B1] [A2], then per step after the barrier [B kt+2] [A kt+3]:
  // at the barrier of step kt the wave needs A kt+1 and B kt+1 and may leave A kt+2 (its newest 4 pieces) in flight.
#if X6_WALK
  // Here the same order runs over the STREAM's stages, so what a step fetches may be the next tile's, and a tile's last K-step
  // has the barrier and the DMA issue too (the one-tile form has nothing left to fetch there).
  dma_a(); dma_b();
  if (nstage > 1) { dma_a(); dma_b(); }
  if (nstage > 2) dma_a();
  if (nstage > 2) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(8 + BI_MIN) : "memory");
  else if (nstage > 1) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(4 + BI_MIN) : "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  auto step = [&](int st) {                      // stage st's counted wait, barrier and DMA issue
    if (st + 2 < nstage) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (st + 2 < nstage) dma_b();
    if (st + 3 < nstage) dma_a();
  };
  for (int e = 0;; ++e) {                        // the workgroup's tiles
  read_raw(0, 0); read_b(0, 0, 0);
#pragma unroll
  for (int i = 0; i < 44; ++i) op(i);
  commit(0);
  for (int kt = 0; kt + 1 < nk; ++kt) {
    half(0, true, kt, 1);
    step(sbase + kt);
    half(1, true, kt + 1, 0);
  }
  half(0, true, nk - 1, 1);
  step(sbase + nk - 1);
  half(1, false, 0, 0);
  auto epilogue = [&]() __attribute__((always_inline)) {
#else
  dma_a(0); dma_b(0);
  if (nk > 1) { dma_a(1); dma_b(1); }
  if (nk > 2) dma_a(2);
  if (nk > 2) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(8 + BI_MIN) : "memory");
  else if (nk > 1) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(4 + BI_MIN) : "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  read_raw(0, 0); read_b(0, 0, 0);
#pragma unroll
  for (int i = 0; i < 44; ++i) op(i);
  commit(0);
  for (int kt = 0; kt + 1 < nk; ++kt) {
    half(0, true, kt, 1);                        // s = 0 on buffer 0; fetches and splits (kt, s = 1) into buffer 1
    if (kt + 2 < nk) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (kt + 2 < nk) dma_b(kt + 2);
    if (kt + 3 < nk) dma_a(kt + 3);
    half(1, true, kt + 1, 0);                    // s = 1 on buffer 1; fetches and splits (kt+1, s = 0) into buffer 0
  }
  half(0, true, nk - 1, 1);
  half(1, false, 0, 0);
#endif

  // X6_BNBWD: the producer's y values of this lane's 16 rows x NI columns are fetched NOW, ahead of the tile's stores and the
  // barrier, so that their latency is off the workgroup's tail
  float yv[EPI == X6_BNBWD ? NI : 1][16];
  float pav[NI], pcv[NI], pmv[NI], piv[NI];
  if (EPI == X6_BNBWD) {
    const int rbase = m0 + 32 * w;
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int n = n0 + j * 32 + r;
      pav[j] = pcv[j] = pmv[j] = piv[j] = 0.f;
#pragma unroll
      for (int q = 0; q < 16; ++q) yv[j][q] = 0.f;
      if (n < N && (!PARTIAL || j * 32 + r < BN)) {
        const int pq = n / g.pco, pi = n - pq * g.pco;
        const size_t po = (size_t)pq * g.pco + pi;
        pav[j] = g.pa[po]; pcv[j] = g.pc[po]; pmv[j] = g.pmean[po]; piv[j] = g.pinvstd[po];
        const float* yp = g.py + ((size_t)pq * M + rbase) * (size_t)g.pco + pi;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int row = (q & 3) + 8 * (q >> 2) + 4 * h;
          if (rbase + row < M) yv[j][q] = yp[(size_t)row * g.pco];
        }
      }
    }
  }
  // ---- epilogue.  Block j, register q: row 32 w + (q & 3) + 8 (q >> 2) + 4 h, column 32 j + r
  float* C = g.C + (size_t)z * g.c_bstride;
#pragma unroll
  for (int j = 0; j < NI; ++j)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[j][q] += accs[j][q];
#if !X6_WALK
  if (g.ksplit > 1) {
    // split-K: the partial goes out in register order (element (j, q) of thread tid at (j * 16 + q) * 256 + tid: every store
    // instruction of a wave is one 256-byte run).  Hand-off without cache-wide fences (an agent-scope release writes the whole
    // L2 back: measured 57-150 us per launch in this place): every payload store is write-through (relaxed agent-scope atomic
    // store = sc1), every storing wave drains its stores, the workgroup meets, ONE lane counts the arrival; the last arrival
    // reads all partials with sc1 loads (they bypass this CU's L1, the only cache that could hold a stale copy).
    const size_t tile_id = ((size_t)z * g.mtiles + tm) * g.ntiles + tn;
    typedef __attribute__((address_space(1))) float gfloat;
    typedef __attribute__((address_space(1))) unsigned gu32;
    gfloat* mine = (gfloat*)(g.part + (tile_id * g.ksplit + ks) * (size_t)(NI * 16 * 256));
    gu32* cnt = (gu32*)(g.cnt + tile_id);
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int q = 0; q < 16; ++q) __hip_atomic_store(mine + (j * 16 + q) * 256 + tid, acc[j][q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    unsigned* flag = reinterpret_cast<unsigned*>(lds);
    if (tid == 0) *flag = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (*flag != (unsigned)(g.ksplit - 1)) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");          // no instruction: keeps the loads below the count
    if (tid == 0) __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // re-armed for the next launch
    const gfloat* all = (const gfloat*)(g.part + tile_id * g.ksplit * (size_t)(NI * 16 * 256));
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[j][q] = 0.f;
    for (int s2 = 0; s2 < g.ksplit; ++s2) {                         // range order: the same bits whoever arrives last
      const gfloat* ps = all + (size_t)s2 * (NI * 16 * 256) + tid;
#pragma unroll
      for (int j = 0; j < NI; ++j)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[j][q] += __hip_atomic_load(ps + (j * 16 + q) * 256, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
#endif
  if constexpr (EPI == X6_STORE_NCHW) {
    // registers 4 qg .. 4 qg + 3 of a block are four consecutive tokens of ONE channel: 16 contiguous bytes of the (image,
    // channel, token) tensor.  Tokens per image and M are multiples of 4, so a group never crosses an image and is stored or
    // skipped as a whole.  Same values as X6_STORE (the residual is read token-major and added in the same order).
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int n = n0 + j * 32 + r;
      const bool mine = n < N && (!PARTIAL || j * 32 + r < BN);
#pragma unroll
      for (int qg = 0; qg < 4; ++qg) {
        const int m = m0 + 32 * w + 8 * qg + 4 * h;
        if (m < M && mine) {
          float4 v = make_float4(acc[j][4 * qg], acc[j][4 * qg + 1], acc[j][4 * qg + 2], acc[j][4 * qg + 3]);
          if (g.add) {
            const float* ap = g.add + (size_t)z * g.c_bstride + (size_t)m * g.ldc + n;
            v.x += ap[0]; v.y += ap[g.ldc]; v.z += ap[2 * (size_t)g.ldc]; v.w += ap[3 * (size_t)g.ldc];
          }
          const int img = m / g.nchw_n, tok = m - img * g.nchw_n;
          *reinterpret_cast<float4*>(C + ((size_t)img * g.nchw_c + n) * g.nchw_n + tok) = v;
        }
      }
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < NI; ++j) {
    const int n = n0 + j * 32 + r;
    const bool mine = n < N && (!PARTIAL || j * 32 + r < BN);
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int m = m0 + 32 * w + (q & 3) + 8 * (q >> 2) + 4 * h;
      if (m < M && mine) {
        float v = acc[j][q];
        if (EPI == X6_STORE && g.add) v += g.add[(size_t)z * g.c_bstride + (size_t)m * g.ldc + n];
        C[(size_t)m * g.ldc + n] = v;
      }
    }
  }
  if (EPI == X6_BNBWD) {
    // Backward statistics of the PRODUCER's BN (see X6Args): per lane the 16 rows of its column, y read with the same
    // 128-byte row segments the tile was stored with; the two half-waves and the four waves are combined through LDS in
    // fp64 and leave ONE atomic pair per column and tile, like the forward statistics below.
    __syncthreads();                                   // every wave is done with the DMA rings
    float* red = reinterpret_cast<float*>(lds);        // [4 waves][BN][2]
    const int rbase = m0 + 32 * w;
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int n = n0 + j * 32 + r;
      float s0 = 0.f, s1 = 0.f;
      if (n < N && (!PARTIAL || j * 32 + r < BN)) {
        const float av = pav[j], cv = pcv[j], mv = pmv[j], iv = piv[j];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int row = (q & 3) + 8 * (q >> 2) + 4 * h;
          float dz = rbase + row < M ? acc[j][q] : 0.f;
          if (g.pact == 1) dz *= gelu_grad_f(__builtin_fmaf(av, yv[j][q], cv));
          s0 += dz;
          s1 += dz * ((yv[j][q] - mv) * iv);
        }
      }
      s0 += __shfl_xor(s0, 32);
      s1 += __shfl_xor(s1, 32);
      if (h == 0 && (!PARTIAL || j * 32 + r < BN)) { float* o = red + ((w * BN) + j * 32 + r) * 2; o[0] = s0; o[1] = s1; }
    }
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

  // Train-mode BN statistics of the tile's columns (as gkg_gemm.hip's epilogue): per wave (its 32 rows) centred
  // (mean, M2) from registers, Chan-merged over the four waves in fp64, then ONE fp64 atomic pair per column and tile:
  // S += n mean, Q += M2 + n mean^2.  No workgroup waits for another.
#if X6_WALK
  // (red has its own region behind the rings, which hold the next tile's stages by now)
  float* red = reinterpret_cast<float*>(reinterpret_cast<char*>(lds) + x6_ring_bytes(NI, BN));        // [4 waves][BN][2]
#else
  __syncthreads();                                   // every wave is done with the DMA rings
  float* red = reinterpret_cast<float*>(lds);        // [4 waves][BN][2]
#endif
  const int rbase = m0 + 32 * w;
  const int cnt = max(0, min(32, M - rbase));
#pragma unroll
  for (int j = 0; j < NI; ++j) {
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) s += rbase + (q & 3) + 8 * (q >> 2) + 4 * h < M ? acc[j][q] : 0.f;
    s += __shfl_xor(s, 32);
    const float mean = cnt > 0 ? s / (float)cnt : 0.f;
    float m2 = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const float d = acc[j][q] - mean;
      m2 += rbase + (q & 3) + 8 * (q >> 2) + 4 * h < M ? d * d : 0.f;
    }
    m2 += __shfl_xor(m2, 32);
    if (h == 0 && (!PARTIAL || j * 32 + r < BN)) { float* o = red + ((w * BN) + j * 32 + r) * 2; o[0] = mean; o[1] = m2; }
  }
  __syncthreads();
  if (tid < BN && n0 + tid < N) {
    double n = 0.0, mean = 0.0, m2 = 0.0;
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
      const int c = max(0, min(32, M - (m0 + rg * 32)));
      x6_chan_merge(n, mean, m2, (double)c, (double)red[(rg * BN + tid) * 2], (double)red[(rg * BN + tid) * 2 + 1]);
    }
    double* sz = g.sums + ((size_t)(tm % g.nslots) * g.nbatch + z) * 2 * N + n0 + tid;
    __hip_atomic_fetch_add(sz, n * mean, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(sz + N, m2 + n * mean * mean, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
#if X6_WALK
  };
  epilogue();
  if (e + 1 == ntile) return;
  // The next tile of the list.  Its first stages were issued by the last K-steps above and have been in flight for the whole
  // epilogue; the full wait also retires the epilogue's own loads and stores, which share vmcnt with the DMA pieces, so that the
  // counted waits of the loop see DMA pieces only.
  sbase += nk;
  walk_tile(e + 1, z, tm, tn);
  m0 = tm * BM; n0 = tn * BN;
#pragma unroll
  for (int j = 0; j < NI; ++j)
#pragma unroll
    for (int q = 0; q < 16; ++q) { acc[j][q] = 0.f; accs[j][q] = 0.f; }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  }
#endif
}
