// Development-only GEMM kernels: included by gemm256.hip under PI3_DEV_VARIANTS, right after launch256 (same
// translation unit; they use its g4_glds16, g2_epilogue_lds, g2_persistent_grid and G2_* constants, and launch through
// gemm_launch of gemm_common.h).  pi3_gemm256_try picks them by knob.  Never part of the product library.
// ---------------------------------------------------------------------------------------------------------------
// Two-workgroups-per-CU form (PI3_GEMM_IMPL=3 / per-shape choice): 128 (m) x 256 (n) tile, 256 threads = 4 waves, each
// wave the same 128 x 64 output block (and therefore the same epilogues) as in gemm256_kernel, BK = 32, a 3-stage
// LDS-DMA ring of 24 KiB stages (72 KiB per workgroup: two workgroups fit a CU's 160 KiB, their 4 + 4 waves give every
// SIMD one wave of each).  The two workgroups of a CU are independent, so one's epilogue (an HBM-rate store stream the
// 256 x 256 kernel cannot hide at one workgroup per CU) runs under the other's main loop, and barrier / LDS-latency
// stalls of one are filled by the other.  Price: 1.5 x the L2 -> LDS bytes per flop of the 256 x 256 tile.
// MEASURED (round 2, M = 64300): qkv 0.525 / proj 0.257 / fc1 0.702 / fc2 0.657 ms against 0.439 / 0.222 / 0.640 / 0.510 ms
// of gemm256_kernel on the same box, tile-group sizes 4...64 within 5 % of each other: the epilogue does overlap, but
// the main loop drops from ~1.25 to ~0.85 PF/s (LDS array busy 75 % of the MFMA time instead of 62 %: the same
// fragment reads plus 1.5 x the DMA writes, and one barrier per 32 MFMAs).  Kept as a correct A/B variant, not default.
//   stage image: act 128 rows x 64 B, then W 256 rows x 64 B; 16-byte chunk c of row r sits at c ^ F[(r >> 2) & 3],
//   F = {0, 2, 3, 1}: conflict-free for the ds_read_b128 fragment pattern on 64-byte rows (each 16-lane group of the
//   instruction then covers one whole 256-byte bank row).
//   iteration u: s_waitcnt vmcnt(6) (stage u landed, stage u+1 may fly) -> s_barrier -> LDS-DMA of stage u+2 (its slot
//   was last read in iteration u-1, which every wave has left) -> 12 fragment reads -> 32 MFMAs.
// ---------------------------------------------------------------------------------------------------------------
#define G3_BM 128
#define G3_BN 256
#define G3_STAGE 24576
#define G3_LDS (3 * G3_STAGE)        // 72 KiB; the epilogue reuses it (4 waves x 18 KiB)

template <bool OUT_BF16, int ACT, bool QK = false>
__global__ __launch_bounds__(256, 2) void gemm3_kernel(GemmParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  const int nbm = (p.M + G3_BM - 1) / G3_BM, nbn = p.N / G3_BN;
  const int nwg = nbm * nbn;
  const int id = xcd_remap(blockIdx.x, nwg);
  const int GM = p.tile_gm > 0 ? p.tile_gm : 16;
  const int per_group = GM * nbn;
  const int g = id / per_group;
  const int gm = min(GM, nbm - g * GM);
  const int rem = id - g * per_group;
  const int bm = g * GM + rem % gm;
  const int bn = rem / gm;

  const char* Ab = (const char*)p.A;
  const char* Wb = (const char*)p.W;
  const long lda_b = p.lda * 2, ldw_b = p.ldw * 2;
  const int nk = p.K >> 5;

  // swizzle table F = {0, 2, 3, 1} packed 2 bits each: 0b01'11'10'00 = 0x78
  auto F = [](int q) { return (0x78 >> (2 * q)) & 3; };

  // ---- staging addresses: lane i of a 1 KiB segment covers row i >> 2 (16 rows), slot i & 3
  const int srow = lane >> 2, spos = lane & 3;
  const char* a_src[2];
  const char* w_src[4];
  int a_dst[2], w_dst[4];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int seg = wave * 2 + i, row = seg * 16 + srow;
    int grow = bm * G3_BM + row;
    grow = grow < p.M ? grow : p.M - 1;
    a_src[i] = Ab + (long)grow * lda_b + ((spos ^ F((row >> 2) & 3)) << 4);
    a_dst[i] = seg * 1024;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int seg = wave * 4 + i, row = seg * 16 + srow;
    w_src[i] = Wb + (long)(bn * G3_BN + row) * ldw_b + ((spos ^ F((row >> 2) & 3)) << 4);
    w_dst[i] = 8192 + seg * 1024;
  }
#define G3_STAGE_IN(U)                                                                                    \
  {                                                                                                       \
    char* sb = smem + ((U) % 3) * G3_STAGE;                                                               \
    const long kb = (long)(U) * 64;                                                                       \
    _Pragma("unroll") for (int i = 0; i < 2; ++i)                                                         \
      __builtin_amdgcn_global_load_lds(GLB_PTR(a_src[i] + kb), LDS_PTR(sb + a_dst[i]), 16, 0, 0);        \
    _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                         \
      __builtin_amdgcn_global_load_lds(GLB_PTR(w_src[i] + kb), LDS_PTR(sb + w_dst[i]), 16, 0, 0);        \
  }

  f32x4 acc[4][8];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // fragment addresses inside a stage: rows mi*16 + frow (act) / wave*64 + ni*16 + frow (W), chunk lane >> 4
  const int frow = lane & 15;
  const int foff = frow * 64 + (((lane >> 4) ^ F((frow >> 2) & 3)) << 4);
  const int w_base = 8192 + wave * 64 * 64 + foff;

  G3_STAGE_IN(0)
  if (nk > 1) G3_STAGE_IN(1)

  for (int u = 0; u < nk; ++u) {
    if (u + 1 < nk) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (u + 2 < nk) G3_STAGE_IN(u + 2)
    const char* sb = smem + (u % 3) * G3_STAGE;
    bf16x8 fw[4], fa[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) fw[i] = *(const bf16x8*)(sb + w_base + i * 1024);
#pragma unroll
    for (int j = 0; j < 8; ++j) fa[j] = *(const bf16x8*)(sb + foff + j * 1024);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw[i], fa[j], acc[i][j], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
  }
  // every wave must be out of its last fragment reads before the epilogue reuses the ring
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");

  if constexpr (OUT_BF16)
    g2_epilogue_lds<OUT_BF16, ACT, QK>(p, acc, bm * G3_BM, bn * G3_BN + wave * 64, smem + wave * G2_EPI_WAVE, lane);
  else
    gemm_epilogue<OUT_BF16, ACT, 4, 8>(p, acc, bm * G3_BM, bn * G3_BN + wave * 64, lane);
#undef G3_STAGE_IN
}

template <bool OUT_BF16, int ACT, bool QK = false>
static int launch3(const GemmParams& p, hipStream_t stream) {
  const int nbm = (p.M + G3_BM - 1) / G3_BM, nbn = p.N / G3_BN;
  return gemm_launch<gemm3_kernel<OUT_BF16, ACT, QK>>("gemm3", nbm * nbn, 256, G3_LDS, p, stream);
}

// ---------------------------------------------------------------------------------------------------------------
// Four-wave form (round 4 experiment, knob gemm_4w = 1): the same 256 x 256 x 64 tile, LDS image, swizzle and persistent
// tile walk, but ONE wave per SIMD, each owning a 128 (m) x 128 (n) block = 8 x 8 MFMA tiles = 256 accumulator registers
// (the wave may use 512: accumulators in AGPRs).  Why: gemm256_kernel is bound by the LDS port - per K tile its eight
// waves read 8 x 24 KB of fragments beside the 64 KB the LDS-DMA writes, 2 048 cycles of the 128 B/clk port against 2 048
// cycles of MFMA.  A 128 x 128 wave block reads (128 + 128) rows x 128 B = 32 KB per wave and K tile: 4 x 32 + 64 = 192 KB
// per K tile, 1 536 port cycles against the same 2 048 MFMA cycles.  Price: no partner wave to cover a wave's waits, so
// the K loop is software-pipelined inside the wave: a K tile is two 32-deep halves, the fragments of the NEXT half are
// read while the 64 MFMAs of the current one run, one barrier per K tile:
//   half A(u): read frags (u, kk=1);   64 MFMAs on (u, kk=0);   vmcnt(0) [DMA(u+1) landed], lgkmcnt(0);   s_barrier
//   half B(u): read frags (u+1, kk=0) from the other buffer;   LDS-DMA of tile u+2 into this buffer;   64 MFMAs on (u, kk=1)
// Hazards: buffer (u & 1) is re-staged after the barrier that follows every wave's last read of it (its kk=1 fragments,
// returned: lgkmcnt(0) before the barrier); DMA(u+1) is waited for by the issuing wave before the same barrier and read
// after it.  The LDS-DMA is issued from inline asm (M0 = wave-uniform LDS base), so hipcc's waitcnt pass puts no
// vmcnt(0) in front of later ds_reads; the only vmcnt waits are the ones written here.
// ---------------------------------------------------------------------------------------------------------------
// LDS-DMA through g4_glds16 (gemm256.hip): a scalar base and a 32-bit lane offset, one VGPR per staged segment instead
// of a 64-bit pointer (with 16 segments per wave and K tile the 64-bit pointers were hoisted out of the K loop, spilled,
// and their scratch reloads brought vmcnt(0) waits in front of every DMA)

// fragment read from inline asm (immediate offset), so that its place between the asm MFMAs is the place it is issued
// at: a C++ load may be hoisted by the scheduler to the top of the block, which is what leaves a lone wave's MFMAs waiting
// behind a burst of 16 reads + 16 LDS-DMA issues.  The consumer waits with an explicit s_waitcnt lgkmcnt(0).
template <int OFF>
__device__ __forceinline__ void g4_lds_read(bf16x8& d, unsigned addr) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "n"(OFF));
}

template <bool OUT_BF16, int ACT, bool QK = false, bool ILV = false>
__global__ __launch_bounds__(256) void gemm4w_kernel(GemmParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // scalar: LDS-DMA destinations (M0) are SALU arithmetic
  const int wm = wave >> 1, wn = wave & 1;
  const int nbm = (p.M + G2_BM - 1) / G2_BM, nbn = p.N / G2_BN;
  const int nwg = nbm * nbn;
  const char* Ab = (const char*)p.A;
  const char* Wb = (const char*)p.W;
  const long lda_b = p.lda * 2, ldw_b = p.ldw * 2;
  const int nk = p.K >> 6;
  const int GM = p.tile_gm > 0 ? p.tile_gm : 8;
  const int per_group = GM * nbn;

  const int* pos_l = nullptr;
  const float* cs_l = nullptr;
  if constexpr (QK) {      // RoPE tables -> LDS once per workgroup (as gemm256_kernel)
    if (p.qk_pos && p.qk_T * 8 + 16 <= G2_TAB_BYTES) {
      int* scratch = (int*)(smem + G2_LDS_TOTAL);
      int* pl = scratch + 4;
      if (tid == 0) scratch[0] = 0;
      __syncthreads();
      int mx = 0;
      for (int i = tid; i < 2 * p.qk_T; i += 256) {
        const int v = p.qk_pos[i];
        pl[i] = v;
        mx = max(mx, v);
      }
      mx = (int)wave_max((float)mx);
      if (lane == 0) atomicMax(scratch, mx);
      __syncthreads();
      const int npos = scratch[0] + 1;
      const int tab0 = 16 + ((p.qk_T * 8 + 15) & ~15);
      if (tab0 + npos * 128 <= G2_TAB_BYTES) {
        float* cl = (float*)(smem + G2_LDS_TOTAL + tab0);
        for (int i = tid; i < npos * 32; i += 256) cl[i] = p.qk_cs[i];
        pos_l = pl;
        cs_l = cl;
      }
      __syncthreads();
    }
  }

  const int frow = lane & 15;
  const int swz = (lane >> 1) & 7;
  const int cq = lane >> 4;
  const int off0 = ((cq) ^ swz) << 4, off1 = ((cq + 4) ^ swz) << 4;
  const int a_base = wm * G2_HALF + frow * 128;
  const int w_base = (2 + wn) * G2_HALF + frow * 128;
  const unsigned lds0 = __builtin_amdgcn_readfirstlane(
      (unsigned)(__UINTPTR_TYPE__)((__attribute__((address_space(3))) void*)(smem)));

  for (int vb = blockIdx.x; vb < nwg; vb += gridDim.x) {
    const int id = xcd_remap(vb, nwg);
    const int g = id / per_group;
    const int gm = min(GM, nbm - g * GM);
    const int rem = id - g * per_group;
    const int bm = p.tile_order ? g * GM + rem / nbn : g * GM + rem % gm;
    const int bn = p.tile_order ? rem % nbn : rem / gm;

    f32x4 acc[8][8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // staging offsets of this tile: segment (half h, i) = rows h * 128 + (wave * 4 + i) * 8 .. + 7, lane -> (row, 16-byte chunk)
    unsigned aoff[8], woff[8];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = (wave * 4 + i) * 8 + (lane >> 3);
        const int c = (lane & 7) ^ ((row >> 1) & 7);
        int ga = bm * G2_BM + h * 128 + row, gw = bn * G2_BN + h * 128 + row;
        ga = ga < p.M ? ga : p.M - 1;
        gw = gw < p.N ? gw : p.N - 1;
        aoff[h * 4 + i] = (unsigned)((long)ga * lda_b + c * 16);
        woff[h * 4 + i] = (unsigned)((long)gw * ldw_b + c * 16);
      }
#define G4_STAGE(U)                                                                                     \
  {                                                                                                     \
    const unsigned sb = lds0 + ((U) & 1) * G2_BUF + wave * 4096;                                        \
    const char* sa = Ab + (long)(U) * 128;                                                              \
    const char* sw = Wb + (long)(U) * 128;                                                              \
    _Pragma("unroll") for (int h = 0; h < 2; ++h)                                                       \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                     \
      g4_glds16(sa, aoff[h * 4 + i], sb + h * G2_HALF + i * 1024);                                      \
      g4_glds16(sw, woff[h * 4 + i], sb + (2 + h) * G2_HALF + i * 1024);                                \
    }                                                                                                   \
  }
#define G4_READ(FA, FW, BUFP, OFF)                                                         \
  _Pragma("unroll") for (int i = 0; i < 8; ++i) {                                           \
    FW[i] = *(const bf16x8*)((BUFP) + w_base + i * 2048 + (OFF));                           \
    FA[i] = *(const bf16x8*)((BUFP) + a_base + i * 2048 + (OFF));                           \
  }
// MFMAs from inline asm with the accumulators constrained to AGPRs ("+a"): left to the builtin, hipcc treats the 512
// registers as one pool, parks fragments and addresses in AGPRs and shuttles accumulators through v_accvgpr_read / mov in
// the K loop (seen in the ISA).  With the constraint the 256 accumulators stay in a0-a255 and the 256 VGPRs hold the two
// fragment sets (128), the staging offsets and the addressing.
#define G4_MFMA(FA, FW)                                                                     \
  _Pragma("unroll") for (int i = 0; i < 8; ++i)                                             \
  _Pragma("unroll") for (int j = 0; j < 8; ++j)                                             \
    asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc[i][j]) : "v"(FW[i]), "v"(FA[j]));
#define G4_BARRIER()                  \
  asm volatile("" ::: "memory");      \
  __builtin_amdgcn_s_barrier();       \
  asm volatile("" ::: "memory");

    bf16x8 fa0[8], fw0[8], fa1[8], fw1[8];
    // prologue: tile 0 landed (16 DMA per wave and K tile), tile 1 in flight
    G4_STAGE(0)
    if (nk > 1) {
      G4_STAGE(1)
      asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    G4_BARRIER()
    if constexpr (ILV) {
      // Interleaved form: every half is eight groups of {2 fragment reads of the NEXT half, (half B) 2 LDS-DMA issues of
      // tile u + 2, 8 MFMAs of the current half}, all inline asm and therefore issued in exactly this order: the matrix
      // pipe never waits behind a burst of issue-only instructions (a 16x16x32 MFMA holds the vector issue for 8 of its 16
      // cycles; the reads and DMA issues ride in the other 8).
      const unsigned abase0 = lds0 + a_base, wbase0 = lds0 + w_base;
#define G4_RD1(FA, FW, AB, WB, I) g4_lds_read<(I) * 2048>(FW[I], WB); g4_lds_read<(I) * 2048>(FA[I], AB);
#define G4_MF8(FA, FW, I)                                                                  \
  _Pragma("unroll") for (int j = 0; j < 8; ++j)                                            \
    asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc[I][j]) : "v"(FW[I]), "v"(FA[j]));
#define G4_ST2(U, I)                                                                       \
  {                                                                                        \
    const unsigned sb = lds0 + ((U) & 1) * G2_BUF + wave * 4096;                           \
    const char* sa = Ab + (long)(U) * 128;                                                 \
    const char* sw = Wb + (long)(U) * 128;                                                 \
    g4_glds16(sa, aoff[I], sb + ((I) >> 2) * G2_HALF + ((I) & 3) * 1024);                  \
    g4_glds16(sw, woff[I], sb + (2 + ((I) >> 2)) * G2_HALF + ((I) & 3) * 1024);            \
  }
#define G4_GROUP_A(I) G4_RD1(fa1, fw1, ab + off1, wb + off1, I) G4_MF8(fa0, fw0, I)
// (the 16 DMA issues of tile u + 2 sit in the FIRST four groups: the last one then has 1.75 halves to land instead of 1)
#define G4_GROUP_B(I)                                                                      \
  if (more1) { G4_RD1(fa0, fw0, abn + off0, wbn + off0, I) }                               \
  if (more2 && (I) < 4) { G4_ST2(u + 2, 2 * (I)) G4_ST2(u + 2, 2 * (I) + 1) }              \
  G4_MF8(fa1, fw1, I)
      {
        const unsigned ab = abase0, wb = wbase0;
        G4_RD1(fa0, fw0, ab + off0, wb + off0, 0) G4_RD1(fa0, fw0, ab + off0, wb + off0, 1)
        G4_RD1(fa0, fw0, ab + off0, wb + off0, 2) G4_RD1(fa0, fw0, ab + off0, wb + off0, 3)
        G4_RD1(fa0, fw0, ab + off0, wb + off0, 4) G4_RD1(fa0, fw0, ab + off0, wb + off0, 5)
        G4_RD1(fa0, fw0, ab + off0, wb + off0, 6) G4_RD1(fa0, fw0, ab + off0, wb + off0, 7)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      }
      for (int u = 0; u < nk; ++u) {
        const unsigned ab = abase0 + (u & 1) * G2_BUF, wb = wbase0 + (u & 1) * G2_BUF;
        const unsigned abn = abase0 + ((u + 1) & 1) * G2_BUF, wbn = wbase0 + ((u + 1) & 1) * G2_BUF;
        const bool more1 = u + 1 < nk, more2 = u + 2 < nk;
        // ---- half A: reads of (u, kk = 1) under the MFMAs of (u, kk = 0)
        G4_GROUP_A(0) G4_GROUP_A(1) G4_GROUP_A(2) G4_GROUP_A(3) G4_GROUP_A(4) G4_GROUP_A(5) G4_GROUP_A(6) G4_GROUP_A(7)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // DMA(u + 1) landed
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // the reads of buffer (u & 1) returned
        G4_BARRIER()
        // ---- half B: reads of (u + 1, kk = 0) and the DMA of tile u + 2 under the MFMAs of (u, kk = 1)
        G4_GROUP_B(0) G4_GROUP_B(1) G4_GROUP_B(2) G4_GROUP_B(3) G4_GROUP_B(4) G4_GROUP_B(5) G4_GROUP_B(6) G4_GROUP_B(7)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // fa0 / fw0 for the next half A
      }
#undef G4_RD1
#undef G4_MF8
#undef G4_ST2
#undef G4_GROUP_A
#undef G4_GROUP_B
    } else {
    G4_READ(fa0, fw0, smem, off0)
    for (int u = 0; u < nk; ++u) {
      const char* bp = smem + (u & 1) * G2_BUF;
      const char* bq = smem + ((u + 1) & 1) * G2_BUF;
      // ---- half A
      G4_READ(fa1, fw1, bp, off1)
      G4_MFMA(fa0, fw0)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      G4_BARRIER()
      // ---- half B
      if (u + 1 < nk) { G4_READ(fa0, fw0, bq, off0) }
      if (u + 2 < nk) { G4_STAGE(u + 2) }
      G4_MFMA(fa1, fw1)
    }
    }   // !ILV
    // the hazard recogniser does not see into the asm MFMAs: let the last ones retire before the epilogue reads AGPRs
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) asm volatile("" : "+a"(acc[i][j]));     // pins the epilogue's reads behind the nops
    // nobody reads the pipeline buffers after the last barrier: the epilogue may reuse them at once
    const int m_base = bm * G2_BM + wm * 128, n_base = bn * G2_BN + wn * 128;
    if constexpr (OUT_BF16) {
      char* wl = smem + wave * G2_EPI_WAVE;
      g2_epilogue_lds<OUT_BF16, ACT, QK>(p, *(f32x4(*)[4][8]) & acc[0], m_base, n_base, wl, lane, pos_l, cs_l);
      g2_epilogue_lds<OUT_BF16, ACT, QK>(p, *(f32x4(*)[4][8]) & acc[4], m_base, n_base + 64, wl, lane, pos_l, cs_l);
    } else {
      gemm_epilogue<OUT_BF16, ACT, 8, 8>(p, acc, m_base, n_base, lane);
    }
    if (vb + (int)gridDim.x < nwg) { G4_BARRIER() }
#undef G4_STAGE
#undef G4_READ
#undef G4_MFMA
#undef G4_BARRIER
  }
}

template <bool OUT_BF16, int ACT, bool QK = false, bool ILV = false>
static int launch4w(const GemmParams& p, hipStream_t stream) {
  const int nwg = ((p.M + G2_BM - 1) / G2_BM) * (p.N / G2_BN);
  return gemm_launch<gemm4w_kernel<OUT_BF16, ACT, QK, ILV>>("gemm4w", g2_persistent_grid(nwg), 256,
                                                            QK ? G2_LDS_QK : G2_LDS_TOTAL, p, stream);
}
