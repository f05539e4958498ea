// 256x256-tile bf16 GEMM with a phase-pipelined K loop (the transformer GEMMs of the north-star chunk: M = 64 300,
// N in {1024, 3072, 4096}, K in {1024, 2048, 4096}).  Same math / epilogue as gemm.hip, different staging structure:
// one 512-thread workgroup per CU (8 waves, 2 per SIMD), LDS-DMA prefetch kept in flight ACROSS barriers with counted
// s_waitcnt vmcnt(N), raw s_barrier, one MFMA cluster per phase (cdna guide "256^2 8-phase template", re-derived here
// for the swapped-operand orientation).
//
// Geometry: BK = 64 (one 128-byte row per operand row).  Waves 2 (m) x 4 (n): wave (wm, wn) owns the 128 (m) x 64 (n)
// output = 8 x 4 MFMA 16x16x32 tiles = 128 accumulator registers.  LDS = 2 K-tile buffers x {act half 0, act half 1,
// W half 0, W half 1} x 16 KiB = 128 KiB; a wave reads exactly one act half (wm) and one W half (wn >> 1) per K tile.
//
// Per K tile u (buffer u & 1) there are two phases, each: fragment ds_reads -> two half-tile LDS-DMA prefetches (4 x
// global_load_lds_dwordx4 per thread) -> s_waitcnt -> [s_barrier] -> 32 MFMAs at wave priority 1 (a 64 x 64 half of the
// wave's block, K = 64) -> s_barrier:
//   phase ab: read W(nh0)[4] + W(nh1)[4] + act(mh0)[8]   prefetch act halves 0, 1 of tile u+1   MFMA (mh0, nh0), (mh0, nh1)
//   phase cd: read act(mh1)[8]   prefetch W halves 0, 1 of tile u+2, then s_waitcnt vmcnt(4)    MFMA (mh1, nh1), (mh1, nh0)
// The prologue stages tile 0 and the W halves of tile 1 and waits with vmcnt(4): tile 0 complete, W(1) in flight.
// Hazards: a buffer region is re-staged only after the barrier that follows its last fragment read (W halves and act
// half 0 after phase ab, act half 1 after phase cd); staged data is read in the phase AFTER the counted wait + barrier
// that retires it (cd's vmcnt(4) leaves only the two newest half-tiles, W(u+2), in flight: tile u+1 is complete).  The
// second wave of every SIMD runs one barrier behind the first (STAG, below); since a region is re-staged ONE phase
// after its last read, a wave's fragment reads must have RETURNED (s_waitcnt lgkmcnt(0)) and its counted vmcnt wait
// must have been executed before the mid barrier of the phase, not merely issued before it.
// The LDS-DMA is issued from inline asm (g4_glds16) with per-tile 32-bit lane offsets: hipcc does not see the LDS write
// and places no vmcnt(0) of its own in the loop, and eight offset dwords replace nine 64-bit staging pointers (no vector
// spills).  The 32-bit offsets bound the operand footprint: pi3_gemm256_try declines matrices of 4 GiB and more.
//
// Forms that lost, one line each; the numbers are in the "GEMM family" table of profiles/EXPERIMENTS.md:
//   four phases per K tile (round 2), two phases with every operand staged three phases ahead: row "four phases per K tile"
//   staging through the LDS-DMA builtin with a 64-bit pointer per piece: row "LDS-DMA of the K loop from inline asm"
//   two LDS-DMA pieces behind one write of M0: row "two LDS-DMA pieces behind one write of M0"
//   no wave priorities / the load segment at priority 1: row "wave priorities of the ping-pong loop"
//   plain instead of non-temporal stores of the bf16 output: row "non-temporal stores of the bf16 output rows"
// Development builds (make dev) add the variants of gemm256_dev.inc and the STAG = false / ILVK / M32 instances.
//
// Host side: pi3_gemm256_try (called from gemm.hip) declines what the kernel does not serve, sets the launch's own fields
// in its copy of the block and maps (out_dtype, act) to an instance with gemm_dispatch; launch256 (and launch3 / launch4w
// of gemm256_dev.inc) size the grid and go through gemm_launch (gemm_common.h).
#include "gemm_common.h"
#include <stdlib.h>

#define G2_BM 256
#define G2_BN 256
#define G2_HALF 16384          // 128 rows x 128 B
#define G2_BUF (4 * G2_HALF)   // act h0 | act h1 | W h0 | W h1
#define G2_LDS (2 * G2_BUF)
#define G2_EPI_WAVE 18432        // per-wave epilogue staging: 128 rows x 144 B (bf16) or 64 rows x 272 B (f32) <= 18 KiB
#define G2_LDS_TOTAL (8 * G2_EPI_WAVE > G2_LDS ? 8 * G2_EPI_WAVE : G2_LDS)
// fused q/k epilogue: the RoPE tables of the launch live in the 16 KiB of LDS above the pipeline / transpose buffers
// (pos [T][2] int + cos/sin [npos][16][2] float, staged once per workgroup): round 2 fetched them per 16-row group with
// two DEPENDENT global loads (position, then the table row) in front of the arithmetic.
#define G2_TAB_BYTES 16384
#define G2_LDS_QK (G2_LDS_TOTAL + G2_TAB_BYTES)

// sum over the four 16-lane rows of a wave (lanes l, l^16, l^32, l^48), result in every lane: two VALU swaps instead of
// two ds_bpermute round trips (the LayerNorm(64) statistic is a chain of two such sums per 16-row group)
__device__ __forceinline__ float g2_sum_rows4(float s) {
  unsigned u = __float_as_uint(s);
  auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);     // {rows 0,0,2,2 | rows 1,1,3,3}
  s = __uint_as_float(a[0]) + __uint_as_float(a[1]);
  u = __float_as_uint(s);
  auto b = __builtin_amdgcn_permlane32_swap(u, u, false, false);     // {lower half twice | upper half twice}
  return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}

// LDS-DMA of one 1 KiB segment from inline asm: scalar base, 32-bit lane offset, LDS destination in M0.  hipcc does not
// see the LDS write, so no compiler-placed s_waitcnt vmcnt(0) appears in front of later fragment reads: every wait on
// these loads is a counted one written by hand.
__device__ __forceinline__ void g4_glds16(const char* sbase, unsigned voff, unsigned lds_dst) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(sbase), "s"(lds_dst)
               : "memory", "m0");
}

// ---- pieces of the fused q/k epilogue (g2_epilogue_lds<.., QK>)
// ksq += the squares of the four bf16 values of one stored u32x2, one packed word (lo^2 + hi^2) at a time: |k|^2 of the
// STORED values, as the attention kernel will read them.  By reference: the sum keeps its association.
__device__ __forceinline__ void g2_add_squares(float& ksq, u32x2 o) {
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const float lo = __uint_as_float(o[e] << 16), hi = __uint_as_float(o[e] & 0xffff0000u);
    ksq += lo * lo + hi * hi;
  }
}

// Row m's |k|^2 (ksq: this lane's 16 of the 64 dims) into the running maximum of its attention batch: k2 for rows below
// qk_split (the first row of the next batch), k2n from there on
__device__ __forceinline__ void g2_fold_k2(float ksq, int m, int M, long qk_split, float& k2, float& k2n) {
  ksq = g2_sum_rows4(ksq);
  if (m < M) {
    if (m < qk_split) k2 = fmaxf(k2, ksq);
    else k2n = fmaxf(k2n, ksq);
  }
}

// (cos, sin) of frequencies nq .. nq + 3 at token t's y and x position; pos [T][2] and cs [npos][16][2] are the tables
// of the launch, in LDS or in global memory
struct G2Rope { f32x4 cy0, cy1, cx0, cx1; };
__device__ __forceinline__ G2Rope g2_rope_fetch(const int* pos, const float* cs, int t, int nq) {
  const int py = pos[2 * t], px = pos[2 * t + 1];
  const float* ty = cs + ((long)py * 16 + nq) * 2;
  const float* tx = cs + ((long)px * 16 + nq) * 2;
  return {*(const f32x4*)ty, *(const f32x4*)(ty + 4), *(const f32x4*)tx, *(const f32x4*)(tx + 4)};
}

// Epilogue through LDS (all pipeline buffers are dead after the last barrier): each wave transposes its 128 (m) x 64 (n)
// accumulator block into row-major [m][n] rows in its private LDS region, then streams whole rows out with 16-byte
// lanes: 128-byte (bf16) / 256-byte (f32) contiguous segments per output row instead of 8/16-byte pieces per lane.
// The register-direct epilogue of gemm.hip costs this kernel +35..70 % at K = 1024 (one workgroup per CU: the store
// tail is not hidden behind another block's math).  bias / qscale / activation / LayerScale are applied in registers
// before the transpose; residual and table adds in the streaming pass (coalesced 16-byte loads).
// Row pitch 144 B (bf16) / 272 B (f32): 16-byte aligned for ds_read_b128, at most 2-way write conflicts.
// QK (bf16 output only): the wave's 64 columns are exactly one head of q, k or v (n_base % 64 == 0) and the lane holds,
// for each of its 8 rows m, 16 of the head's 64 dims: d = ni*16 + nq + r.  The RoPE partner of dim d < 16 (d + 16) and
// of 32 <= d < 48 (d + 16) sits in the SAME lane (tiles ni and ni + 1, same r); the LayerNorm row statistic is an
// in-lane sum of 16 values + two shuffles (lanes frow, frow+16, frow+32, frow+48).  Rounding points as the stand-alone
// pi3_qknorm_rope pass (and the reference under autocast): the Linear output is rounded to bf16 first.
template <bool OUT_BF16, int ACT, bool QK = false>
__device__ __forceinline__ void g2_epilogue_lds(const GemmParams& p, f32x4 (&acc)[4][8], int m_base, int n_base,
                                                char* wl, int lane, const int* pos_l = nullptr,
                                                const float* cs_l = nullptr) {
  const int frow = lane & 15;
  const int nq = (lane >> 4) * 4;
  // ---- fused q/k head epilogue state
  int qk_part = 2, qk_head = 0;
  f32x4 lnw[4], lnb[4];
  bool qk_ln = false;
  float k2 = 0.f, k2n = 0.f;  // running max_rows |k|^2 of this lane (k heads only): first / next attention batch
  long qk_split = 0;          // first row of the next attention batch (the wave's 128 rows span at most two: attnS >= 128)
  if constexpr (QK) {
    const int hh = n_base >> 6;
    qk_part = hh / p.qk_H;
    qk_head = hh - qk_part * p.qk_H;
    const float* w = qk_part == 0 ? p.qk_qw : p.qk_kw;
    const float* b = qk_part == 0 ? p.qk_qb : p.qk_kb;
    qk_ln = (qk_part < 2) && (w != nullptr);
    if (p.qk_k2max) qk_split = ((long)(m_base / p.qk_attnS) + 1) * p.qk_attnS;
    if (qk_ln) {
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        lnw[ni] = *(const f32x4*)(w + ni * 16 + nq);
        lnb[ni] = *(const f32x4*)(b + ni * 16 + nq);
      }
    }
  }
  int qk_t0 = 0;              // token index of the wave's first row (rows of a wave are consecutive tokens)
  if constexpr (QK) {
    if (p.qk_pos) qk_t0 = m_base % p.qk_T;
  }
  f32x4 bias4[4], gamma4[4];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) {
    bias4[ni] = (f32x4){0.f, 0.f, 0.f, 0.f};
    gamma4[ni] = (f32x4){1.f, 1.f, 1.f, 1.f};
  }
  if (p.bias) {
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) bias4[ni] = *(const f32x4*)(p.bias + n_base + ni * 16 + nq);
  }
  if constexpr (!QK) {      // (the fused-qkv instance has no LayerScale: pi3_gemm256_try refuses it; 16 registers less there)
    if (p.gamma) {
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) gamma4[ni] = *(const f32x4*)(p.gamma + n_base + ni * 16 + nq);
    }
  }
  constexpr int PITCH = OUT_BF16 ? 144 : 272;
  constexpr int ROWS_PER_PASS = OUT_BF16 ? 128 : 64;
  constexpr int MI_PER_PASS = ROWS_PER_PASS / 16;
#pragma unroll
  for (int pass = 0; pass < 128 / ROWS_PER_PASS; ++pass) {
    // ---- registers -> LDS (row = local m, 4 consecutive n per lane and tile)
#pragma unroll
    for (int mq = 0; mq < MI_PER_PASS; ++mq) {
      const int mi = pass * MI_PER_PASS + mq;
      char* rowp = wl + (mq * 16 + frow) * PITCH;
      if constexpr (QK) {
        if (qk_part < 2 && (qk_ln || p.qk_pos)) {      // q / k head with LayerNorm and / or RoPE
          f32x4 x[4];
#pragma unroll
          for (int ni = 0; ni < 4; ++ni) {
            const f32x4 v = acc[ni][mi] + bias4[ni];
#pragma unroll
            for (int r = 0; r < 4; ++r) x[ni][r] = (float)(bf16_t)v[r];       // the Linear output is a bf16 tensor
          }
          if (qk_ln) {
            float s = 0.f;
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) s += (x[ni][0] + x[ni][1]) + (x[ni][2] + x[ni][3]);
            s = g2_sum_rows4(s);
            const float mean = s * (1.0f / 64.0f);
            float q = 0.f;
#pragma unroll
            for (int ni = 0; ni < 4; ++ni)
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                x[ni][r] -= mean;
                q += x[ni][r] * x[ni][r];
              }
            q = g2_sum_rows4(q);
            const float rstd = rsqrtf(q * (1.0f / 64.0f) + p.qk_eps);
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) x[ni] = x[ni] * rstd * lnw[ni] + lnb[ni];
          }
          if (p.qk_pos) {
            G2Rope rc;
            if (pos_l) {     // tables in LDS; the row's token index without a division (rows beyond M: any valid token)
              int t = qk_t0 + pass * ROWS_PER_PASS + mq * 16 + frow;
              if (p.qk_T >= 256) t = t >= p.qk_T ? t - p.qk_T : t;
              else t %= p.qk_T;
              rc = g2_rope_fetch(pos_l, cs_l, t, nq);
            } else {
              const int m = m_base + pass * ROWS_PER_PASS + mq * 16 + frow;
              rc = g2_rope_fetch(p.qk_pos, p.qk_cs, (m < p.M ? m : p.M - 1) % p.qk_T, nq);
            }
            const f32x4 cy0 = rc.cy0, cy1 = rc.cy1, cx0 = rc.cx0, cx1 = rc.cx1;
            const float cyv[4] = {cy0[0], cy0[2], cy1[0], cy1[2]}, syv[4] = {cy0[1], cy0[3], cy1[1], cy1[3]};
            const float cxv[4] = {cx0[0], cx0[2], cx1[0], cx1[2]}, sxv[4] = {cx0[1], cx0[3], cx1[1], cx1[3]};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float a0 = x[0][r], a1 = x[1][r], b0 = x[2][r], b1 = x[3][r];
              x[0][r] = a0 * cyv[r] - a1 * syv[r];      // dim j < 16:  x cos - partner sin
              x[1][r] = a1 * cyv[r] + a0 * syv[r];      // dim j + 16:  x cos + partner sin
              x[2][r] = b0 * cxv[r] - b1 * sxv[r];
              x[3][r] = b1 * cxv[r] + b0 * sxv[r];
            }
          }
          const float sc = qk_part == 0 ? p.qk_qscale : 1.0f;
          float ksq = 0.f;
#pragma unroll
          for (int ni = 0; ni < 4; ++ni) {
            u32x2 o;
            o[0] = pack_bf16x2(x[ni][0] * sc, x[ni][1] * sc);
            o[1] = pack_bf16x2(x[ni][2] * sc, x[ni][3] * sc);
            *(u32x2*)(rowp + (ni * 16 + nq) * 2) = o;
            if (qk_part == 1) g2_add_squares(ksq, o);
          }
          if (qk_part == 1 && p.qk_k2max)
            g2_fold_k2(ksq, m_base + pass * ROWS_PER_PASS + mq * 16 + frow, p.M, qk_split, k2, k2n);
          continue;
        }
      }
      float ksq_plain = 0.f;     // QK, a k head without LayerNorm / RoPE (encoder blocks): only max |k|^2 is wanted
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        f32x4 v = acc[ni][mi] + bias4[ni];
        // qcols is a multiple of 64 (whole heads of q), so the test is the same for every lane of the wave: a scalar
        // branch instead of a compare + four selects + two packed multiplies per tile in every bf16 epilogue
        if (n_base + ni * 16 < p.qcols) v *= p.qscale;
        if constexpr (ACT == 1) {
          v = gelu_erf4(v);
        } else if constexpr (ACT == 3) {      // the round 1-3 GELU form (A/B partner, knob gelu_form = 1)
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = gelu_erf_as(v[r]);
        } else if constexpr (ACT == 2) {
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
        }
        if constexpr (!QK) v *= gamma4[ni];
        if constexpr (OUT_BF16) {
          u32x2 o;
          o[0] = pack_bf16x2(v[0], v[1]);
          o[1] = pack_bf16x2(v[2], v[3]);
          *(u32x2*)(rowp + (ni * 16 + nq) * 2) = o;
          if constexpr (QK) {
            if (qk_part == 1 && p.qk_k2max) g2_add_squares(ksq_plain, o);
          }
        } else {
          *(f32x4*)(rowp + (ni * 16 + nq) * 4) = v;
        }
      }
      if constexpr (QK) {
        if (qk_part == 1 && p.qk_k2max)
          g2_fold_k2(ksq_plain, m_base + pass * ROWS_PER_PASS + mq * 16 + frow, p.M, qk_split, k2, k2n);
      }
    }
    // ---- LDS -> global, whole rows
    constexpr int CHUNKS = OUT_BF16 ? 8 : 16;          // 16-byte chunks per row
    constexpr int ROWS_PER_IT = 64 / CHUNKS;
    const int ch = lane % CHUNKS, rsub = lane / CHUNKS;
#pragma unroll 4
    for (int it = 0; it < ROWS_PER_PASS / ROWS_PER_IT; ++it) {
      const int lrow = it * ROWS_PER_IT + rsub;
      const int m = m_base + pass * ROWS_PER_PASS + lrow;
      if (m >= p.M) continue;
      long orow = m;
      int trow = 0;
      if (p.rpg > 0) {
        const int gq = m / p.rpg;
        trow = m - gq * p.rpg;
        orow = (long)gq * p.gstride + p.goff + trow;
      }
      if constexpr (OUT_BF16) {
        const u32x4 v = *(const u32x4*)(wl + lrow * PITCH + ch * 16);
        // non-temporal: the 0.4-0.5 GB an output takes stay out of the L2 the operand panels live in (the f32 outputs
        // keep plain stores: the LayerNorm that follows reads them)
        __builtin_nontemporal_store(v, (u32x4*)((bf16_t*)p.out + orow * p.ldo + n_base + ch * 8));
      } else {
        f32x4 v = *(const f32x4*)(wl + lrow * PITCH + ch * 16);
        const int n0 = n_base + ch * 4;
        if (p.resid) v += *(const f32x4*)(p.resid + orow * p.ldr + n0);
        if (p.addtab) v += *(const f32x4*)(p.addtab + (long)trow * p.ldadd + n0);
        *(f32x4*)((float*)p.out + orow * p.ldo + n0) = v;
      }
    }
  }
  if constexpr (QK) {
    if (qk_part == 1 && p.qk_k2max) {
      // one atomic per wave and attention batch (non-negative floats order like their bit patterns)
      const int b_lo = m_base / p.qk_attnS;
      const float mx = wave_max(k2), mxn = wave_max(k2n);
      if (lane == 0 && m_base < p.M) {
        atomicMax((unsigned*)&p.qk_k2max[(long)b_lo * p.qk_H + qk_head], __float_as_uint(mx));
        if (qk_split <= (long)min(m_base + 127, p.M - 1))
          atomicMax((unsigned*)&p.qk_k2max[(long)(b_lo + 1) * p.qk_H + qk_head], __float_as_uint(mxn));
      }
    }
  }
}

// NOEPI: timing-only ablation (no output) to separate the main loop from the epilogue.
// STAG: waves 4-7 (the second wave of every SIMD) run one barrier behind waves 0-3, and every phase has a second
// barrier between its LDS reads / LDS-DMA issues and its MFMAs: while one wave of a SIMD is in its MFMA segment the
// other is in its load segment, instead of both loading and then both competing for the matrix pipe.  The staging
// schedule already keeps every restage >= 2 phases after the last read of the region and reads a staged tile a phase
// after the vmcnt wait that retires it, which is what the half-phase lag of the second group needs.
// M32 (development builds, knob gemm_mfma32): the K loop on v_mfma_f32_32x32x16_bf16 - half as many MFMA issues for the
// same products (an MFMA holds the SIMD's vector issue port 8 cycles whatever its shape: 1 024 of a K tile's 2 048 cycles
// per SIMD with 16x16x32, 512 with 32x32x16).  Prototype: same staging, LDS image, phases and counted waits; the
// accumulators are brought into the 16x16 register layout through the wave's epilogue LDS region, so that every epilogue
// runs unchanged (one extra LDS round trip per output tile).
template <bool OUT_BF16, int ACT, bool NOEPI = false, bool STAG = false, bool QK = false, bool ILVK = false, bool M32 = false>
__global__ __launch_bounds__(512, 2) void gemm256_kernel(GemmParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const unsigned lds0 = __builtin_amdgcn_readfirstlane(
      (unsigned)(__UINTPTR_TYPE__)((__attribute__((address_space(3))) void*)(smem)));
  const int wm = wave >> 2, wn = wave & 3;

  const int nbm = (p.M + G2_BM - 1) / G2_BM, nbn = p.N / G2_BN;
  const int nwg = nbm * nbn;
  const char* Ab = (const char*)p.A;
  const char* Wb = (const char*)p.W;
  const long lda_b = p.lda * 2, ldw_b = p.ldw * 2;
  const int nk = p.K >> 6;
  const int GM = p.tile_gm > 0 ? p.tile_gm : 8;
  const int per_group = GM * nbn;

  // fused q/k epilogue: RoPE tables -> LDS, once per workgroup (the launch passes G2_LDS_QK bytes of LDS then)
  const int* pos_l = nullptr;
  const float* cs_l = nullptr;
  if constexpr (QK) {
    if (p.qk_pos && p.qk_T * 8 + 16 <= G2_TAB_BYTES) {
      int* scratch = (int*)(smem + G2_LDS_TOTAL);
      int* pl = scratch + 4;
      if (tid == 0) scratch[0] = 0;
      __syncthreads();
      int mx = 0;
      for (int i = tid; i < 2 * p.qk_T; i += 512) {
        const int v = p.qk_pos[i];
        pl[i] = v;
        mx = max(mx, v);
      }
      mx = (int)wave_max((float)mx);
      if (lane == 0) atomicMax(scratch, mx);
      __syncthreads();
      const int npos = scratch[0] + 1;
      const int tab0 = 16 + ((p.qk_T * 8 + 15) & ~15);
      if (tab0 + npos * 128 <= G2_TAB_BYTES) {       // uniform: every thread sees the same npos
        float* cl = (float*)(smem + G2_LDS_TOTAL + tab0);
        for (int i = tid; i < npos * 32; i += 512) cl[i] = p.qk_cs[i];
        pos_l = pl;
        cs_l = cl;
      }
      __syncthreads();
    }
  }

  // Start stagger (knob gemm_stagger_ns, default 0): workgroup b begins b * stagger_ns late, so that the workgroups'
  // epilogues (HBM-rate store / read-modify-write bursts with the matrix pipe idle) do not all fall into the same
  // window.  The persistent grid walks tiles b, b + grid, ...: the highest-numbered workgroups have one tile fewer, so
  // a delay of up to one tile time on them costs nothing at the tail.
#ifdef PI3_DEV_VARIANTS   // measured without effect (profiles/EXPERIMENTS.md): development builds only
  if (p.stagger_ns > 0) {
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();               // 100 MHz
    const unsigned long long ticks = (unsigned long long)blockIdx.x * (unsigned)p.stagger_ns / 10ull;
    while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(4);
  }
#endif

  // Persistent form: the grid is one workgroup per CU (a multiple of 8, so a workgroup stays on its XCD) and every
  // workgroup walks the tiles vb = blockIdx.x, + gridDim.x, ... - the order a tile-per-workgroup launch dispatches them
  // in.  The output stores of tile i are still in flight while the LDS-DMA prologue of tile i + 1 is issued, and the
  // per-workgroup launch / drain latency is paid once per kernel.  gridDim.x = nwg gives the tile-per-workgroup form.
  for (int vb = blockIdx.x; vb < nwg; vb += gridDim.x) {
  const int id = xcd_remap(vb, nwg);
  const int g = id / per_group;
  const int gm = min(GM, nbm - g * GM);
  const int rem = id - g * per_group;
  // order 0: consecutive ids walk the group's m-tiles first (a round of 32 ids on an XCD = GM row panels x 32 / GM
  // column panels); order 1: the column tiles of one row panel first (the activation panel of a row is fetched by
  // one round of workgroups of one XCD; the weight panels are the re-read operand instead)
  const int bm = p.tile_order ? g * GM + rem / nbn : g * GM + rem % gm;
  const int bn = p.tile_order ? rem % nbn : rem / gm;

  f32x4 acc[4][8];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int frow32 = lane & 31, ch32 = lane >> 5;       // M32 (development variant)
  f32x16 acc32[2][4];          // [n tile of 32][m tile of 32]
  if constexpr (M32) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc32[i][t][v] = 0.f;
  }

  // 32-bit staging offsets of this tile: piece (half h, i) = rows h * 128 + (wave * 2 + i) * 8 .. + 7
  unsigned aoff[4], woff[4];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = (wave * 2 + i) * 8 + (lane >> 3);
      const int c = (lane & 7) ^ ((row >> 1) & 7);
      int ga = bm * G2_BM + h * 128 + row, gw = bn * G2_BN + h * 128 + row;
      ga = ga < p.M ? ga : p.M - 1;
      gw = gw < p.N ? gw : p.N - 1;
      aoff[h * 2 + i] = (unsigned)((long)ga * lda_b + c * 16);
      woff[h * 2 + i] = (unsigned)((long)gw * ldw_b + c * 16);
    }
#define STAGE_A(U, HALF)                                                                  \
  {                                                                                       \
    const unsigned sb_ = lds0 + ((U) & 1) * G2_BUF + (HALF) * G2_HALF + wave * 2048;      \
    g4_glds16(Ab + (long)(U) * 128, aoff[(HALF) * 2], sb_);                               \
    g4_glds16(Ab + (long)(U) * 128, aoff[(HALF) * 2 + 1], sb_ + 1024);                    \
  }
#define STAGE_W(U, HALF)                                                                  \
  {                                                                                       \
    const unsigned sb_ = lds0 + ((U) & 1) * G2_BUF + (2 + (HALF)) * G2_HALF + wave * 2048; \
    g4_glds16(Wb + (long)(U) * 128, woff[(HALF) * 2], sb_);                               \
    g4_glds16(Wb + (long)(U) * 128, woff[(HALF) * 2 + 1], sb_ + 1024);                    \
  }

  if constexpr (ILVK) {
    // ---- Interleaved K loop (knob gemm_ilv, round 4 experiment): no ping-pong between the two waves of a SIMD.  A K tile
    // is two phases of 32 MFMAs, one per 32-deep half (kk); every accumulator gets one MFMA per phase.  The fragments of a
    // phase (8 act + 4 W, 48 registers) are double-buffered: while the MFMAs of phase kk0 run, the 12 fragment reads of
    // kk1 are issued between them (one or two per group of four MFMAs); during kk1 the reads of the NEXT tile's kk0 and
    // the eight LDS-DMA pieces of tile u + 2 (into the buffer tile u just left).  One barrier per K tile, between the two
    // phases: by then every wave has its kk1 fragments (nobody reads tile u's buffer any more) and has retired its
    // pieces of tile u + 1 (issued a whole phase earlier).  Everything whose order matters is inline asm.
    const int frow = lane & 15;
    const int swz = (lane >> 1) & 7;
    const int cq = lane >> 4;
    const unsigned off0 = ((cq) ^ swz) << 4, off1 = ((cq + 4) ^ swz) << 4;
    const unsigned a_rd = lds0 + wm * G2_HALF + frow * 128;
    const unsigned w_rd = lds0 + (2 + (wn >> 1)) * G2_HALF + ((wn & 1) * 64 + frow) * 128;
    bf16x8 fa0[8], fw0[4], fa1[8], fw1[4];
#define GI_RD(D, ADDR, OFF) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(D) : "v"(ADDR), "n"(OFF));
#define GI_RD_GROUP(FA, FW, AADDR, WADDR, G)                 \
  GI_RD(FA[G], AADDR, (G) * 2048)                            \
  if constexpr ((G) < 4) { GI_RD(FW[G], WADDR, (G) * 2048) }
// read number R of a phase's twelve: 0..7 = act fragment R, 8..11 = W fragment R - 8; two per group in groups 0..5
#define GI_RD1(FA, FW, AADDR, WADDR, R)                                        \
  if constexpr ((R) < 8) { GI_RD(FA[(R) & 7], AADDR, ((R) & 7) * 2048) }        \
  else { GI_RD(FW[(R) & 3], WADDR, ((R) & 3) * 2048) }
#define GI_RD2(FA, FW, AADDR, WADDR, G)                                                              \
  if constexpr ((G) < 6) { GI_RD1(FA, FW, AADDR, WADDR, 2 * (G)) GI_RD1(FA, FW, AADDR, WADDR, 2 * (G) + 1) }
#define GI_MF4(FA, FW, G)                                                                                        \
  _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                                   \
    asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(acc[i][G]) : "v"(FW[i]), "v"(FA[G]));
#define GI_DMA(U, G)                                                                                              \
  {                                                                                                               \
    const unsigned sb_ = lds0 + ((U) & 1) * G2_BUF + wave * 2048;                                                 \
    if constexpr ((G) < 4) g4_glds16(Ab + (long)(U) * 128, aoff[G], sb_ + ((G) >> 1) * G2_HALF + ((G) & 1) * 1024); \
    else g4_glds16(Wb + (long)(U) * 128, woff[(G) - 4], sb_ + (2 + (((G) - 4) >> 1)) * G2_HALF + ((G) & 1) * 1024);  \
  }
    // prologue: tiles 0 and 1 staged, tile 0 landed, its kk0 fragments in registers
    STAGE_A(0, 0);
    STAGE_A(0, 1);
    STAGE_W(0, 0);
    STAGE_W(0, 1);
    if (nk > 1) {
      STAGE_A(1, 0);
      STAGE_A(1, 1);
      STAGE_W(1, 0);
      STAGE_W(1, 1);
      asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    {
      const unsigned aa = a_rd + off0, ww = w_rd + off0;
      GI_RD_GROUP(fa0, fw0, aa, ww, 0) GI_RD_GROUP(fa0, fw0, aa, ww, 1) GI_RD_GROUP(fa0, fw0, aa, ww, 2)
      GI_RD_GROUP(fa0, fw0, aa, ww, 3) GI_RD_GROUP(fa0, fw0, aa, ww, 4) GI_RD_GROUP(fa0, fw0, aa, ww, 5)
      GI_RD_GROUP(fa0, fw0, aa, ww, 6) GI_RD_GROUP(fa0, fw0, aa, ww, 7)
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    if (p.ilv_prio == 1 && wm == 1) __builtin_amdgcn_s_setprio(1);
    for (int u = 0; u < nk; ++u) {
      const unsigned slot = (u & 1) * G2_BUF, nslot = slot ^ G2_BUF;
      const bool more1 = (u + 1 < nk), more2 = (u + 2 < nk);
      if (p.ilv_prio == 2) { if (wm == 0) __builtin_amdgcn_s_setprio(1); else __builtin_amdgcn_s_setprio(0); }
      {   // phase kk0: MFMAs on (fa0, fw0); the kk1 fragments of this tile arrive
        const unsigned aa = a_rd + slot + off1, ww = w_rd + slot + off1;
#define GI_A(G) GI_MF4(fa0, fw0, G) GI_RD2(fa1, fw1, aa, ww, G)
        GI_A(0) GI_A(1) GI_A(2) GI_A(3) GI_A(4) GI_A(5) GI_A(6) GI_A(7)
#undef GI_A
      }
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_waitcnt vmcnt(0)" ::: "memory");   // kk1 fragments; own pieces of tile u + 1
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      if (p.ilv_prio == 2) { if (wm == 1) __builtin_amdgcn_s_setprio(1); else __builtin_amdgcn_s_setprio(0); }
      {   // phase kk1: MFMAs on (fa1, fw1); kk0 fragments of tile u + 1 arrive; tile u + 2 goes into tile u's buffer
        const unsigned aa = a_rd + nslot + off0, ww = w_rd + nslot + off0;
#define GI_B(G)                                           \
  GI_MF4(fa1, fw1, G)                                     \
  if (more1) { GI_RD2(fa0, fw0, aa, ww, G) }              \
  if (more2) { GI_DMA(u + 2, G) }
        GI_B(0) GI_B(1) GI_B(2) GI_B(3) GI_B(4) GI_B(5) GI_B(6) GI_B(7)
#undef GI_B
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    if (p.ilv_prio) __builtin_amdgcn_s_setprio(0);
    // the hazard recogniser does not see into the asm MFMAs: let the last ones retire before the epilogue reads them
    asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 7" ::: "memory");
    // (empty statements that redefine every accumulator: volatile asm keeps its order, so no instruction of the epilogue
    // that reads an accumulator can be scheduled in front of the nops)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) asm volatile("" : "+v"(acc[i][j]));
#undef GI_RD
#undef GI_RD_GROUP
#undef GI_RD1
#undef GI_RD2
#undef GI_MF4
#undef GI_DMA
  } else {
  // prologue: tile 0 complete, W halves of tile 1 in flight
  STAGE_A(0, 0);
  STAGE_A(0, 1);
  STAGE_W(0, 0);
  STAGE_W(0, 1);
  if (nk > 1) {
    STAGE_W(1, 0);
    STAGE_W(1, 1);
    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");

  const int frow = lane & 15;
  const int swz = (lane >> 1) & 7;
  const int cq = lane >> 4;
  const int off0 = ((cq) ^ swz) << 4, off1 = ((cq + 4) ^ swz) << 4;   // kk = 0, 1
  // fragment bases inside a K-tile buffer
  const int a_base = wm * G2_HALF + frow * 128;                                    // act half wm, rows mi*16 + frow
  const int w_base = (2 + (wn >> 1)) * G2_HALF + ((wn & 1) * 64 + frow) * 128;     // W half, rows (wn&1)*64 + ni*16 + frow

  bf16x8 fa[4][2], fw[4][2];   // act fragments of the current m-half [mi][kk]; W fragments [ni (0..3)][kk]
  // M32: the same 16 + 8 ds_read_b128 per K tile, as fa[t * 2 + (ks >> 1)][ks & 1] = act rows 32 t + (lane & 31) of the
  // current m-half, 16-byte chunk 2 ks + (lane >> 5) (ks = 16-deep step 0..3), and fw[i * 2 + (ks >> 1)][ks & 1] alike
  const int swz32 = (frow32 >> 1) & 7;
  const int a_base32 = wm * G2_HALF + frow32 * 128;
  const int w_base32 = (2 + (wn >> 1)) * G2_HALF + ((wn & 1) * 64 + frow32) * 128;

#define READ_W(BUFP, NH)                                                                   \
  if constexpr (M32) {                                                                      \
    _Pragma("unroll") for (int ks = 0; ks < 4; ++ks)                                        \
      fw[2 * (NH) + (ks >> 1)][ks & 1] =                                                    \
          *(const bf16x8*)((BUFP) + w_base32 + (NH) * 4096 + (((2 * ks + ch32) ^ swz32) << 4)); \
  } else                                                                                    \
  _Pragma("unroll") for (int i = 0; i < 2; ++i) {                                           \
    fw[2 * (NH) + i][0] = *(const bf16x8*)((BUFP) + w_base + (2 * (NH) + i) * 2048 + off0); \
    fw[2 * (NH) + i][1] = *(const bf16x8*)((BUFP) + w_base + (2 * (NH) + i) * 2048 + off1); \
  }
#define READ_A(BUFP, MH)                                                                 \
  if constexpr (M32) {                                                                    \
    _Pragma("unroll") for (int t = 0; t < 2; ++t)                                         \
    _Pragma("unroll") for (int ks = 0; ks < 4; ++ks)                                      \
      fa[2 * t + (ks >> 1)][ks & 1] =                                                     \
          *(const bf16x8*)((BUFP) + a_base32 + (2 * (MH) + t) * 4096 + (((2 * ks + ch32) ^ swz32) << 4)); \
  } else                                                                                  \
  _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                         \
    fa[i][0] = *(const bf16x8*)((BUFP) + a_base + (4 * (MH) + i) * 2048 + off0);          \
    fa[i][1] = *(const bf16x8*)((BUFP) + a_base + (4 * (MH) + i) * 2048 + off1);          \
  }
#define MFMA_Q(MH, NH)                                                                                   \
  __builtin_amdgcn_s_setprio(1);                                                                         \
  if constexpr (M32) {                                                                                   \
    _Pragma("unroll") for (int ks = 0; ks < 4; ++ks)                                                      \
    _Pragma("unroll") for (int t = 0; t < 2; ++t)                                                         \
      acc32[NH][2 * (MH) + t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(                                  \
          fw[2 * (NH) + (ks >> 1)][ks & 1], fa[2 * t + (ks >> 1)][ks & 1], acc32[NH][2 * (MH) + t], 0, 0, 0); \
  } else                                                                                                 \
  _Pragma("unroll") for (int kk = 0; kk < 2; ++kk)                                                        \
  _Pragma("unroll") for (int i = 0; i < 2; ++i)                                                           \
  _Pragma("unroll") for (int j = 0; j < 4; ++j)                                                           \
    acc[2 * (NH) + i][4 * (MH) + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(                            \
        fw[2 * (NH) + i][kk], fa[j][kk], acc[2 * (NH) + i][4 * (MH) + j], 0, 0, 0);                       \
  __builtin_amdgcn_s_setprio(0);
// raw barrier (no vmcnt drain); the empty asm statements with a memory clobber stop the compiler from moving LDS reads /
// LDS-DMA issues across it (s_barrier itself is not a memory operation to LLVM)
#define PHASE_END()                            \
  asm volatile("" ::: "memory");               \
  __builtin_amdgcn_s_barrier();                \
  asm volatile("" ::: "memory");
#define PHASE_MID() if constexpr (STAG) { PHASE_END() }

  if constexpr (STAG) {
    if (wm == 1) { PHASE_END() }
  }
  // Residual touch (knob gemm_rpref, f32 output + residual, no row remap): the epilogue's residual read is the one
  // HBM stream of this kernel that does not depend on the accumulators.  During K tiles nk-6 .. nk-3 every lane loads
  // ONE dword of one 128-byte line of the wave's 128 x 64 residual block (256 lines = 4 instructions per wave) into a
  // register nobody reads, which pulls the lines into L2 / the memory-side cache while HBM is idle under the MFMAs.  The
  // loads are issued right AFTER phase cd's counted wait, so the next counted wait (vmcnt(4) one K tile later, which
  // must retire the act halves issued after them) finds them a whole K tile old; the register stays reserved ("+v")
  // until the last tile's vmcnt(0).
#ifdef PI3_DEV_VARIANTS   // knob gemm_rpref (development builds; measured without effect)
  unsigned pf_sink = 0;
  const char* pf_ptr = nullptr;
  if constexpr (!OUT_BF16 && !NOEPI) {
    if (p.rpref && p.resid && p.rpg == 0) {
      int prow = bm * G2_BM + wm * 128 + (lane >> 1);
      prow = prow < p.M ? prow : p.M - 1;
      pf_ptr = (const char*)(p.resid + (long)prow * p.ldr + bn * G2_BN + wn * 64 + (lane & 1) * 32);
    }
  }
  const long pf_step = 32l * p.ldr * 4;       // instruction i covers rows 32 i .. 32 i + 31 of the wave's block
#endif
#ifdef PI3_DEV_ABLATIONS   // timing-only, WRONG results (development builds): where a K tile's 1.5 us go
  const bool abl_dma = (p.abl & 2) != 0, abl_rd = (p.abl & 4) != 0, abl_wait = (p.abl & 8) != 0;
#else
  constexpr bool abl_dma = false, abl_rd = false, abl_wait = false;
#endif
  for (int u = 0; u < nk; ++u) {
    const char* bp = smem + (u & 1) * G2_BUF;
    const bool pre1 = (u + 1 < nk) && !abl_dma, pre2 = (u + 2 < nk) && !abl_dma;
    if (!abl_rd) {
      READ_W(bp, 0)
      READ_W(bp, 1)
      READ_A(bp, 0)
    }
    if (pre1) { STAGE_A(u + 1, 0); STAGE_A(u + 1, 1); }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    PHASE_MID()
    MFMA_Q(0, 0)
    MFMA_Q(0, 1)
    PHASE_END()
    if (!abl_rd) {
      READ_A(bp, 1)
    }
    if (pre2) {
      STAGE_W(u + 2, 0);
      STAGE_W(u + 2, 1);
      if (!abl_wait) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    } else {
      if (!abl_wait) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
#ifdef PI3_DEV_VARIANTS
    if constexpr (!OUT_BF16 && !NOEPI) {
      const int pi = u - (nk - 6);
      if (pf_ptr && pi >= 0 && pi < 4) {       // wave-uniform
        long off = pi * pf_step;
        if (bm * G2_BM + wm * 128 + pi * 32 + 31 >= p.M) off = 0;    // last row panel: stay inside the matrix
        asm volatile("global_load_dword %0, %1, off" : "+v"(pf_sink) : "v"(pf_ptr + off) : "memory");
      }
    }
#endif
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    PHASE_MID()
    MFMA_Q(1, 1)
    MFMA_Q(1, 0)
    PHASE_END()
  }
#ifdef PI3_DEV_VARIANTS
  asm volatile("" ::"v"(pf_sink));
#endif
  if constexpr (STAG) {
    if (wm == 0) { PHASE_END() }   // barrier counts match again; nobody touches the epilogue LDS before everyone is out
  }
  }   // !ILVK

  if constexpr (M32) {
    // 32x32 accumulators -> the 16x16 register layout the epilogues are written for, through this wave's LDS region:
    // element (n, m) of the wave's 64 x 128 block sits in acc32[n / 32][m / 32][8 ((n % 32) / 8) + n % 4] of lane
    // (m % 32) + 32 ((n % 8) / 4), and belongs in acc[n / 16][m / 16][n % 4] of lane (m % 16) + 16 ((n % 16) / 4)
    float* cv = (float*)(smem + wave * G2_EPI_WAVE);       // 32 rows (n) x 132 floats (128 m + pad): 16.5 KiB
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int v = 0; v < 16; ++v)
          cv[(8 * (v >> 2) + 4 * ch32 + (v & 3)) * 132 + 32 * t + frow32] = acc32[i][t][v];
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int nn = 0; nn < 2; ++nn)
#pragma unroll
        for (int mj = 0; mj < 8; ++mj)
#pragma unroll
          for (int v = 0; v < 4; ++v)
            acc[2 * i + nn][mj][v] = cv[(16 * nn + 4 * (lane >> 4) + v) * 132 + 16 * mj + (lane & 15)];
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
  }
  // ---- epilogue
  if constexpr (NOEPI) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) asm volatile("" ::"v"(acc[i][j]));
  } else {
    // bf16 outputs go through the LDS transpose (8-byte pieces per lane otherwise); f32 outputs already store 64-byte
    // row segments per 4 lanes straight from the accumulators, and the LDS round trip measured slower for them
    if constexpr (OUT_BF16)
      g2_epilogue_lds<OUT_BF16, ACT, QK>(p, acc, bm * G2_BM + wm * 128, bn * G2_BN + wn * 64,
                                         smem + wave * G2_EPI_WAVE, lane, pos_l, cs_l);
    else
      gemm_epilogue<OUT_BF16, ACT, 4, 8>(p, acc, bm * G2_BM + wm * 128, bn * G2_BN + wn * 64, lane);
  }
  // the next tile's prologue overwrites the LDS the epilogue transposes went through: every wave must be out of them
  if (vb + (int)gridDim.x < nwg) { PHASE_END() }
  }   // tiles of this workgroup
}

// Grid of the persistent form: one workgroup per CU, the CU count rounded down to a multiple of 8 (a workgroup stays
// on its XCD), 256 where the device cannot be asked; fewer tiles than that: a workgroup per tile.
static int g2_persistent_grid(int nwg) {
  static int ncu = 0;
  if (!ncu) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess)
      ncu = prop.multiProcessorCount & ~7;
    if (ncu <= 0) ncu = 256;
  }
  return nwg > ncu ? ncu : nwg;
}

template <bool OUT_BF16, int ACT, bool NOEPI = false, bool STAG = false, bool QK = false, bool ILVK = false, bool M32 = false>
static int launch256(const GemmParams& p, hipStream_t stream) {
  const int nwg = ((p.M + G2_BM - 1) / G2_BM) * (p.N / G2_BN);
  // development switch PI3_GEMM_PERSIST: 1 (default) one workgroup per CU walking tiles | 0 a workgroup per tile
  const int grid = PI3_DEV_ENV_INT("PI3_GEMM_PERSIST", 1) ? g2_persistent_grid(nwg) : nwg;
  return gemm_launch<gemm256_kernel<OUT_BF16, ACT, NOEPI, STAG, QK, ILVK, M32>>("gemm256", grid, 512,
                                                                               QK ? G2_LDS_QK : G2_LDS_TOTAL, p, stream);
}

#ifdef PI3_DEV_VARIANTS   // gemm3_kernel (PI3_GEMM_IMPL=3) and gemm4w_kernel (knob gemm_4w): measured slower, bit-identical - development builds
#include "gemm256_dev.inc"
#endif   // PI3_DEV_VARIANTS

// Used by pi3_gemm / pi3_gemm_qkv (gemm.hip) for bf16 operands when N % 256 == 0 and M is large.  Returns 1 if not
// applicable.  p is the caller's block by value: what the 256x256 launch adds to it (below) stays in here.
using G256Pairs = OutActs<OutAct<true, 0>, OutAct<true, 1>, OutAct<true, 3>, OutAct<false, 0>>;
#ifdef PI3_DEV_VARIANTS
using G256DevPairs = OutActs<OutAct<true, 0>, OutAct<true, 1>, OutAct<false, 0>>;   // every development family
#endif

int pi3_gemm256_try(GemmParams p, int out_dtype, int act, hipStream_t stream) {
  if ((p.N % G2_BN) != 0 || (p.K % 64) != 0 || p.M < 1024) return 1;
  if (p.qcols % 16) return 1;          // the bf16 epilogue tests n < qcols per 16-column tile (wave-uniform)
  if (out_dtype == 0 && (p.resid || p.addtab)) return 1;   // the bf16 streaming pass carries no residual / table add
  // the LDS-DMA addresses a row through a 32-bit byte offset from the matrix base
  if ((long)p.M * p.lda * 2 >= (1l << 32) || (long)p.N * p.ldw * 2 >= (1l << 32)) return 1;
  if (p.qk_mode) {   // fused q/k head epilogue: bf16 output, no activation, one head per wave column block
    if (out_dtype != 0 || act != 0 || p.gamma || p.rpg || p.N != 3 * p.qk_H * 64 ||
        (p.qk_k2max && p.qk_attnS < 128))
      return 1;
  }
  // ---- the fields of the block that belong to this launch (nobody else sets them)
  // development switches (constants in the product build, common.h): PI3_GEMM_GM = m-tiles per scheduling group (any
  // value gives the same results); PI3_GEMM_ORDER: 0 m-tiles first inside a group | 1 column tiles first | -1: by shape.
  // With four column tiles (N = 1024: proj, fc2) walking a row panel's column tiles first measured 2 % / 3-4 % faster
  // (the activation panel of a row is fetched by one round of one XCD's workgroups and the 2-8 MB of weights stay in
  // L2 anyway); with 12-16 column tiles (qkv, fc1) it is 2-3 % slower.
  p.tile_gm = PI3_DEV_ENV_INT("PI3_GEMM_GM", 0);
  const int order_knob = PI3_DEV_ENV_INT("PI3_GEMM_ORDER", -1);
  p.tile_order = order_knob >= 0 ? order_knob : (p.N / G2_BN <= 4 ? 1 : 0);
  p.stagger_ns = (int)PI3_DEV_KNOB("gemm_stagger_ns", 0);
  p.rpref = (int)PI3_DEV_KNOB("gemm_rpref", 0);
  const int ilv = (int)PI3_DEV_KNOB("gemm_ilv", 0);      // interleaved K loop (development builds), 2 / 3: wave priorities
  p.ilv_prio = ilv ? ilv - 1 : 0;
#ifdef PI3_DEV_ABLATIONS   // timing-only variant that writes NOTHING: development builds only
  // knob gemm_abl (bits): 1 = no epilogue at all, 2 = no LDS-DMA issues in the K loop, 4 = no fragment reads
  p.abl = (int)PI3_KNOB("gemm_abl", 0);
#endif
  // knob gelu_form (product): 1 = the sigmoid form of GELU's tanh approximation in the fc1 epilogue
  if (act == 1 && PI3_KNOB("gelu_form", 0) == 1) act = 3;
#ifdef PI3_DEV_VARIANTS
  // Development variants, every one bit-identical to the shipped kernel (tests/test_dev_variants_gpu.py):
  //   PI3_GEMM_IMPL=3  gemm3_kernel: two 128 x 256 workgroups per CU;
  //   knob gemm_4w     gemm4w_kernel: one wave per SIMD, 128 x 128 per wave (2: reads and DMA issues between the MFMAs);
  //   knob gemm_ilv    the eight-wave kernel's interleaved K loop;
  //   knob gemm_mfma32 the 32x32x16 K loop (prototype: see gemm256_kernel);
  //   PI3_GEMM_STAG=0  all eight waves in lockstep.
  // The first family that is switched on and has the (out_dtype, act) pair serves the call (both GELU forms: its one).
  {
    const bool impl3 = PI3_DEV_ENV_INT("PI3_GEMM_IMPL", 0) == 3 && (p.K % 32) == 0;
    const int impl4 = (int)PI3_KNOB("gemm_4w", 0);
    if (p.qk_mode) {
      if (impl4 == 2) return launch4w<true, 0, true, true>(p, stream);
      if (impl4) return launch4w<true, 0, true>(p, stream);
      if (impl3) return launch3<true, 0, true>(p, stream);
      if (ilv) return launch256<true, 0, false, false, true, true>(p, stream);
      return launch256<true, 0, false, true, true>(p, stream);
    }
#ifdef PI3_DEV_ABLATIONS
    const bool noepi = (p.abl & 1) != 0;
#else
    const bool noepi = false;
#endif
    const int dact = act == 3 ? 1 : act;
    auto family = [&](auto launch) { return gemm_dispatch(G256DevPairs{}, out_dtype, dact, launch); };
    int rc = 1;
    if (impl4 == 2) rc = family([&](auto oa) { return launch4w<oa.OUT16, oa.ACT, false, true>(p, stream); });
    if (rc == 1 && impl4) rc = family([&](auto oa) { return launch4w<oa.OUT16, oa.ACT>(p, stream); });
    if (rc == 1 && impl3) rc = family([&](auto oa) { return launch3<oa.OUT16, oa.ACT>(p, stream); });
    if (rc != 1) return rc;
    if (ilv) {
      if (noepi) return launch256<true, 0, true, false, false, true>(p, stream);
      rc = family([&](auto oa) { return launch256<oa.OUT16, oa.ACT, false, false, false, true>(p, stream); });
      if (rc != 1) return rc;
    }
    if ((int)PI3_KNOB("gemm_mfma32", 0)) {
      if (noepi) return launch256<true, 0, true, true, false, false, true>(p, stream);
      rc = family([&](auto oa) { return launch256<oa.OUT16, oa.ACT, false, true, false, false, true>(p, stream); });
      if (rc != 1) return rc;
    }
    const int stag = PI3_DEV_ENV_INT("PI3_GEMM_STAG", 1);
    if (noepi) return stag ? launch256<true, 0, true, true>(p, stream) : launch256<true, 0, true>(p, stream);
    if (!stag) {
      rc = family([&](auto oa) { return launch256<oa.OUT16, oa.ACT>(p, stream); });
      if (rc != 1) return rc;
    }
  }
#endif
  // the shipped kernel: eight waves, waves 4-7 one barrier behind waves 0-3 (STAG)
  if (p.qk_mode) return launch256<true, 0, false, true, true>(p, stream);
  return gemm_dispatch(G256Pairs{}, out_dtype, act,
                       [&](auto oa) { return launch256<oa.OUT16, oa.ACT, false, true>(p, stream); });
}
