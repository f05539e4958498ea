// Attention forward for long sequences: 64 query rows per wave (two 32-row blocks A/B), 8 waves = 512 query rows per
// workgroup (PI3_ATTN_NW=4: 256).
//
// Same math and data flow as attn.hip (see its header: S^T = K.Q^T with the query on the lane, the bf16-converted
// accumulators are the B operand of O^T += V^T.P^T, deferred rescale of the online max), but every K fragment
// (ds_read_b128) and every V^T fragment (ds_read_b64_tr_b16) feeds TWO MFMAs, one per query block:
//   * K/V global->LDS traffic per FLOP drops 4x (512 instead of 128 query rows share a staged tile): the ablation of
//     attn.hip shows 19 % of its time is the staging path (7 TB/s of L2/MALL reads at S = 64 300);
//   * LDS fragment reads per FLOP halve;
//   * the two blocks are independent, so one block's softmax (VALU) overlaps the other block's MFMAs inside a wave.
// Cost: ~230 VGPRs -> 2 waves per SIMD (one 512-thread workgroup per CU).
//
// Bounded-score path (NOMAX).  The loop is VALU-ISSUE bound, not MFMA bound: per 64x64 tile a wave issues 32 MFMAs
// (1024 matrix-pipe cycles) but ~1900 cycles of single-issue vector work (64 v_exp, 64 v_sub, 64 adds, 40 max, 32 cvt).
// The running maximum exists only to keep exp2 in range.  By Cauchy-Schwarz |q.k| <= |q| |k|, and softmax is invariant
// to the subtracted constant, so when  |q_row| * max_keys |k|  <= 90  (exp2 domain; q carries scale*log2e) for every
// row of a wave, that wave uses m = 0: p = exp2(s) lies in [2^-90, 2^90], nothing overflows or underflows in fp32 / bf16
// (8 exponent bits both; row sums stay below 2^106),
// and the max, the compare, the rescale branch and all 64 subtractions disappear.  pi3's q/k are LayerNorm'ed per head
// (qk_norm, pi3/models/layers/attention.py:321-323), which is what makes the bound hold in practice; waves whose rows
// exceed it take the online-max loop, so the result is the same softmax for every input.  max |k|^2 per (batch, head)
// comes from a ~30 us pre-pass over K (a64_knorm_kernel).
//
// What the loop is bound by (s_memtime stamps around the phases of a tile, 2.05 GHz under load; the stamp code is gone,
// the row "where a workgroup's 24.5 us go" of profiles/EXPERIMENTS.md names the last tree that has it): per tile and SIMD,
// QK^T of the two resident waves = 32 MFMAs = 1012 cycles with the VALU idle, then softmax + PV = ~2400 cycles bound by
// VALU issue (64 v_exp at 8 cycles, 32 cvt_pk, MFMA issue slots) with the matrix pipe half idle.  Tried and measured
// slower than this kernel, so not kept: (a) ping-pong halves (waves 0-3 in QK^T while waves 4-7 are in softmax + PV,
// two barriers per tile, with and without s_setprio / throttled QK^T): an in-order wave stalls on the busy matrix pipe
// and its vector work stalls behind it, 4-6 % slower; (b) block B of each wave half a tile late, so that each phase has
// independent matrix and vector work: V fragments are then read twice and hipcc's schedule leaves the MFMAs clustered,
// 9 % slower; (c) one wave per SIMD with 128 rows per wave, two block groups half a tile apart, chunks of
// {MFMA, 2 exp, MFMA, 2 exp, 2 cvt, row-sum MFMA} pinned with sched_barrier and the QK^T MFMAs in asm so that the scores
// stay in arch VGPRs (hipcc otherwise puts every MFMA result of a 512-register kernel in the accumulator file and the
// softmax pays 400 v_accvgpr copies per tile): 123 cycles per chunk against 64 of matrix pipe, 8 % slower; (d) the
// gemm256-style stagger with pure segments (M: PV(t) + QK(t+1), 32 MFMAs; V: softmax(t+1); waves 4-7 one barrier behind,
// 3-deep rings): the lone wave in M exposes its LDS fragment latency (1800 cycles for 1024 of matrix pipe) and the
// younger wave's vector segment doubles under the partner's priority, 20 % slower.
// tools/micro/valu_rates.hip gives the reason: ONE wave's stream issues a v_exp every 8 cycles and a v_cvt_pk every 6
// (two waves on a SIMD together: 5.3 and 3.0), so a single in-order stream cannot feed the matrix pipe at d = 64, and two
// streams per SIMD is what the 64-row register budget allows.  The row-sum-on-MFMA and bounded-score steps above are
// what this form could still give.
#include "common.h"
#include <stdlib.h>

#include "attn64_params.h"
#define A64_BOUND2 8100.0f   // (90)^2: p in [2^-90, 2^90], l <= 2^106, O <= 2^110: inside fp32 / bf16 range

#define A64_QB 256
#define A64_KT 64
#define A64_THR 6.0f

__device__ __forceinline__ bf16x8 a64_cat4(bf16x4 a, bf16x4 b) {
  return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
}


// LDS-DMA issued from inline asm.  Through the builtin, hipcc's waitcnt pass treats every later ds_read_b64_tr_b16 (an
// intrinsic without alias-scope info) as possibly aliasing the in-flight DMA and inserts s_waitcnt vmcnt(0) in front
// of the first V read of the tile: the K/V stream then lands under nobody's cover.  The pass does not see this form, so
// the only vmcnt waits in the loops are the counted ones written below.  lds_dst must be wave-uniform (it goes in M0);
// lane i's 16 bytes land at lds_dst + 16 i.
__device__ __forceinline__ void a64_glds16(const void* gsrc, const void* lds_dst) {
  const unsigned m0v = __builtin_amdgcn_readfirstlane(
      (unsigned)(__UINTPTR_TYPE__)((__attribute__((address_space(3))) void*)(lds_dst)));
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(gsrc), "s"(m0v) : "memory", "m0");
}

// F16: q / k / v / o are IEEE half instead of bf16 (MoGe, which the reference runs under fp16 autocast, moge/model/v2.py:228):
// the same fragments through v_mfma_f32_32x32x16_f16 (same rate), probabilities packed as half.  Half has 5 exponent
// bits, so that form always runs the online-max loop (p <= 2^A64_THR = 64); the bounded-score loop is bf16 only.
template <bool F16>
__device__ __forceinline__ f32x16 a64_mfma(bf16x8 a, bf16x8 b, f32x16 c) {
  if constexpr (F16)
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
template <bool F16>
__device__ __forceinline__ uint32_t a64_pack(float lo, float hi) {
  if constexpr (F16) return pack_f16x2(lo, hi);
  else return pack_bf16x2(lo, hi);
}

// Optimistic bounded-score loop (round 5, knob attn_nomax = 2, the default).  The a-priori bound |q| max|k| <= 90 is a
// Cauchy-Schwarz bound: it fails as soon as ONE key of a head has a large norm although the scores themselves stay
// moderate (the learned q/k LayerNorm gains of real weights decide, and nobody has them offline).  The loop without a
// running maximum is exact whenever no p = exp2(s) overflows and the terms that matter are normal numbers, and both can
// be read off the result: a workgroup whose waves are not all inside the a-priori bound (those need no test: |s| <= 90)
// runs the loop anyway and ACCEPTS it iff for each row of the waves outside the bound
//   2^-60 <= l <= 2^120  and every accumulator of O is finite.
// l finite: no p overflowed (p <= l).  l >= 2^-60: the largest p of the row is >= 2^-60 / S >= 2^-77, so every term within
// 2^-49 of it is a normal bf16 / fp32 number and what was flushed is below fp32 resolution of the sum.  l <= 2^120 keeps
// the sums themselves away from the top of the range; O = sum p v is tested directly (|v| > 2^7 can overflow it first).
// In score terms: a row is kept when its largest score lies in about [-76, 120 - log2(#keys near the maximum)].
// A rejected workgroup (workgroup-uniform: one __syncthreads_or) stores NOTHING but a mark - the bf16 pattern A64_MARK (a
// NaN with a payload) in the first output element it owns - and a second launch of the compiler-scheduled kernel (redo = 1,
// same grid) runs the online-max loop for exactly the marked workgroups; every other workgroup of that launch reads one
// element and leaves.  A genuine result that happens to carry the pattern only costs a re-run that stores the same softmax
// again.  The result is therefore the same softmax for every input.  Price (profiles/r05c_attention_optimistic_ab.log, one
// process): the almost empty second launch is not measurable (14.655 against 14.648 ms for the a-priori form); with one
// 8 x-norm key per head - the a-priori bound broken for 2 015 of 2 016 workgroups, scores moderate - the a-priori form takes
// 17.74 ms, the online-max loop 17.76 ms and this form 14.69 ms with no workgroup rejected.  A rejected workgroup pays its
// time again on the slower loop: in the frame-wise launches 24 us spread over the card, in the global launch the 2.1 ms ONE
// workgroup takes to sweep 1 005 key tiles however few are rejected; every workgroup rejected would cost both loops.
// In-kernel re-runs (a second inlined body, or a loop around one) were built first: hipcc then spills 70-80 registers per
// lane in the main loops (ScratchSize 32 -> 320 bytes in the hand-placed kernel).  o must not alias q/k/v.
#define A64_MARK 0x7FC1
#define A64_LSUM_LO 8.673617379884035e-19f    // 2^-60
#define A64_LSUM_HI 1.329227995784916e+36f    // 2^120
__device__ __forceinline__ bool a64_reject(float lpart, const f32x16 (&o)[2]) {
  const float l = lpart + __shfl_xor(lpart, 32, 64);
  float chk = 0.f;       // inf / NaN in any accumulator ends up here (a finite sum that overflows only costs a re-run)
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int i = 0; i < 16; ++i) chk += fabsf(o[dt][i]);
  return !(l >= A64_LSUM_LO && l <= A64_LSUM_HI && chk <= 3.0e38f);
}
// the first output element a workgroup owns (row qb * rows-per-workgroup < S always exists)
__device__ __forceinline__ unsigned short* a64_mark_ptr(const Attn64Params& p, int b, int qb, int head, int rows) {
  return (unsigned short*)(p.o + (long)b * p.o_batch_stride + (long)qb * rows * p.o_tok_stride + head * 64);
}

// online-softmax step of one 32-row block on its two raw score tiles; m is the per-lane running max (exp2 domain).
// MSUM (bounded-score path only): the row sum is taken by the matrix pipe, which idles through most of this VALU-bound
// phase: v_mfma_f32_4x4x4_16B_bf16 with an all-ones A operand adds the lane's own four packed bf16 probabilities into
// lacc (D_b[i][j] = sum_k B_b[k][j], and lane 4b+j holds both column j of B_b and column j of D_b).  16 two-pass MFMAs
// replace 68 v_add_f32 per tile, and l sums exactly the bf16 values that P.V multiplies.
typedef short s16x4 __attribute__((ext_vector_type(4)));
// NKT = 1: only the first 32 keys of the tile exist (a short last tile): sc[1] / pf[1] are not touched.
template <bool FIRST, bool NOMAX, bool MSUM, int NKT = 2, bool F16 = false>
__device__ __forceinline__ void a64_softmax(f32x16 (&sc)[2], float& m, f32x16 (&o)[2], float& l, f32x4& lacc,
                                            bf16x8 (&pf)[2][2]) {
  if constexpr (NOMAX) {
    float ps0 = 0.f, ps1 = 0.f;
    const s16x4 ones = {0x3f80, 0x3f80, 0x3f80, 0x3f80};
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        u32x4 pw;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const float p0 = __builtin_amdgcn_exp2f(sc[kt][8 * s2 + 2 * jj]);
          const float p1 = __builtin_amdgcn_exp2f(sc[kt][8 * s2 + 2 * jj + 1]);
          if constexpr (!MSUM) {
            ps0 += p0;
            ps1 += p1;
          }
          pw[jj] = pack_bf16x2(p0, p1);
        }
        if constexpr (MSUM) {
          u32x2 lo2, hi2;
          lo2[0] = pw[0]; lo2[1] = pw[1]; hi2[0] = pw[2]; hi2[1] = pw[3];
          lacc = __builtin_amdgcn_mfma_f32_4x4x4bf16_1k(ones, __builtin_bit_cast(s16x4, lo2), lacc, 0, 0, 0);
          lacc = __builtin_amdgcn_mfma_f32_4x4x4bf16_1k(ones, __builtin_bit_cast(s16x4, hi2), lacc, 0, 0, 0);
        }
        pf[kt][s2] = __builtin_bit_cast(bf16x8, pw);
      }
    if constexpr (!MSUM) l += ps0 + ps1;
    return;
  }
  float tmax = sc[0][0];
#pragma unroll
  for (int i = 1; i < 16; ++i) tmax = fmaxf(tmax, sc[0][i]);
  if constexpr (NKT == 2) {
#pragma unroll
    for (int i = 0; i < 16; ++i) tmax = fmaxf(tmax, sc[1][i]);
  }
  tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
  if (FIRST) {
    m = tmax;
  } else if (!__all(tmax <= m + A64_THR)) {
    const float mn = fmaxf(m, tmax);
    float alpha = __builtin_amdgcn_exp2f(m - mn);
    asm volatile("s_nop 1" : "+v"(alpha));  // v_exp -> VALU (trans) hazard is not padded ahead of inline asm
    l *= alpha;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int i = 0; i < 16; ++i) asm volatile("v_mul_f32 %0, %1, %0" : "+v"(o[dt][i]) : "v"(alpha));
    m = mn;
  }
  float psum = 0.f;
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      u32x4 pw;
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const float p0 = __builtin_amdgcn_exp2f(sc[kt][8 * s2 + 2 * jj] - m);
        const float p1 = __builtin_amdgcn_exp2f(sc[kt][8 * s2 + 2 * jj + 1] - m);
        psum += p0 + p1;
        pw[jj] = a64_pack<F16>(p0, p1);
      }
      pf[kt][s2] = __builtin_bit_cast(bf16x8, pw);
    }
  l += psum;
}

// NW = waves per workgroup (4 or 8): NW * 64 query rows share one staged K/V tile.
// GLDS: stage K/V with LDS-DMA (global_load_lds, swizzle on the source address) instead of registers + ds_write.
// (the kernel body as a function of the LDS block: attn_fwd64_kernel wraps it; attn_fwd64a_kernel, below, falls back to it)
template <int NW, bool GLDS = false, bool MSUM = false, bool F16 = false>
__device__ __forceinline__ void a64_body(const Attn64Params& p, char* lds, const int wg) {   // wg: workgroup index (blockIdx.x in the primary launches)   // lds: K ring [2][64][128 B] then V ring [2][64][128 B]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int nwg = p.nqb * p.H * p.B;
  const int id = xcd_remap(wg, nwg);
  const int qb = id % p.nqb;
  const int head = (id / p.nqb) % p.H;
  const int b = id / (p.nqb * p.H);
  const int S = p.S;
  if (!F16 && p.redo) {      // follow-up launch of the optimistic form: only marked workgroups run (workgroup-uniform)
    if (__builtin_nontemporal_load(a64_mark_ptr(p, b, qb, head, NW * 64)) != A64_MARK) return;
    __syncthreads();         // every wave has read the mark before wave 0's stores can replace it
  }

  const int q0 = qb * (NW * 64) + wave * 64;
  bf16x8 qfA[4], qfB[4];
  {
    const int ra = min(q0 + r, S - 1), rb = min(q0 + 32 + r, S - 1);
    const bf16_t* pa = p.q + (long)b * p.batch_stride + (long)ra * p.tok_stride + head * 64;
    const bf16_t* pb = p.q + (long)b * p.batch_stride + (long)rb * p.tok_stride + head * 64;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      qfA[s] = *(const bf16x8*)(pa + 16 * s + 8 * h);
      qfB[s] = *(const bf16x8*)(pb + 16 * s + 8 * h);
    }
  }
  f32x16 oA[2], oB[2];
  float mA = 0.f, mB = 0.f;
  oA[0] = oA[1] = oB[0] = oB[1] = (f32x16)(0.f);
  float lA = 0.f, lB = 0.f;
  f32x4 laccA = (f32x4)(0.f), laccB = (f32x4)(0.f);   // MSUM: row sums accumulated by the matrix pipe

  const int nt = (S + A64_KT - 1) / A64_KT;
  const bf16_t* kbase = p.k + (long)b * p.batch_stride + head * 64;
  const bf16_t* vbase = p.v + (long)b * p.batch_stride + head * 64;
  constexpr int CPT = 512 / (NW * 64);   // 16-byte chunks of K (and of V) per thread and tile
  int srow[CPT], sch[CPT], kw[CPT], vw[CPT];
  unsigned goff[CPT];
#pragma unroll
  for (int i = 0; i < CPT; ++i) {
    const int cid = tid + NW * 64 * i;
    srow[i] = cid >> 3;
    sch[i] = cid & 7;
    kw[i] = srow[i] * 128 + ((sch[i] ^ ((srow[i] >> 1) & 7)) << 4);
    vw[i] = 16384 + srow[i] * 128 + ((sch[i] ^ (((srow[i] >> 1) & 1) << 2)) << 4);
    goff[i] = (unsigned)(srow[i] * p.tok_stride + sch[i] * 8) * 2u;
  }
  u32x4 kr[CPT], vr[CPT];
  auto load_tile = [&](int T, bool clamp) {
    if (clamp) {
#pragma unroll
      for (int i = 0; i < CPT; ++i) {
        int grow = T * A64_KT + srow[i];
        grow = grow < S ? grow : S - 1;
        kr[i] = *(const u32x4*)(kbase + (long)grow * p.tok_stride + sch[i] * 8);
        vr[i] = *(const u32x4*)(vbase + (long)grow * p.tok_stride + sch[i] * 8);
      }
    } else {
      const char* kt_ = (const char*)(kbase + (long)T * A64_KT * p.tok_stride);
      const char* vt_ = (const char*)(vbase + (long)T * A64_KT * p.tok_stride);
#pragma unroll
      for (int i = 0; i < CPT; ++i) {
        kr[i] = *(const u32x4*)(kt_ + goff[i]);
        vr[i] = *(const u32x4*)(vt_ + goff[i]);
      }
    }
  };
  // LDS-DMA form: wave w, instruction i writes the 1 KiB segment (rows 8*seg .. 8*seg+7) of the K (V) tile; the lane's
  // slot (row, pos) must receive source chunk pos ^ f(row).
  // Four-wave workgroups (frame-wise sequences) carry the source pointers of the un-clamped tiles from tile to tile (one
  // 64-bit add each) instead of rebuilding them from the tile index (~17 vector instructions per tile): -5 % on
  // 100 x 643 tokens.  The same change makes the eight-wave kernel 1.3 % SLOWER at S = 64 300 (measured in one
  // process, interleaved: 15.04 against 14.85 ms), so that one keeps the branch-free index form.
  constexpr bool CARRY = (NW <= 4);
  const long tile_bytes = (long)A64_KT * p.tok_stride * 2;
  const char* kp[CPT];
  const char* vp[CPT];
  if constexpr (CARRY) {
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      const int seg = wave * CPT + i;
      const int row = seg * 8 + (lane >> 3), pos = lane & 7;
      kp[i] = (const char*)(kbase + (long)row * p.tok_stride) + ((pos ^ ((row >> 1) & 7)) << 4) + tile_bytes;   // tile 1
      vp[i] = (const char*)(vbase + (long)row * p.tok_stride) + ((pos ^ (((row >> 1) & 1) << 2)) << 4) + tile_bytes;
    }
  }
  auto glds_tile = [&](int T, bool clamp, int buf) {
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      const int seg = wave * CPT + i;
      if (!CARRY || clamp) {
        const int row = seg * 8 + (lane >> 3), pos = lane & 7;
        int grow = T * A64_KT + row;
        if (clamp) grow = grow < S ? grow : S - 1;
        const char* ks = (const char*)(kbase + (long)grow * p.tok_stride) + ((pos ^ ((row >> 1) & 7)) << 4);
        const char* vs = (const char*)(vbase + (long)grow * p.tok_stride) + ((pos ^ (((row >> 1) & 1) << 2)) << 4);
        a64_glds16(ks, lds + buf * 8192 + seg * 1024);
        a64_glds16(vs, lds + 16384 + buf * 8192 + seg * 1024);
      } else {                 // tiles 1, 2, ... in order: the carried pointers
        a64_glds16(kp[i], lds + buf * 8192 + seg * 1024);
        a64_glds16(vp[i], lds + 16384 + buf * 8192 + seg * 1024);
        kp[i] += tile_bytes;
        vp[i] += tile_bytes;
      }
    }
  };
  auto write_tile = [&](int buf) {
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      *(u32x4*)(lds + buf * 8192 + kw[i]) = kr[i];
      *(u32x4*)(lds + buf * 8192 + vw[i]) = vr[i];
    }
  };
  if constexpr (GLDS) {
    glds_tile(0, true, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the asm-issued DMA is invisible to the compiler's own waits
  } else {
    load_tile(0, true);
    write_tile(0);
  }
  __syncthreads();

  const int kswz = (r >> 1) & 7;
  const int krow_off = r * 128;
  const int gi = lane & 15, gg = (lane >> 4) & 1;
  const int vrow_l = 4 * h + (gi >> 2);
  const int vcol_l = 16 * gg + 4 * (gi & 3);
  const int vch_l = vcol_l >> 3;
  const int vin_l = (vcol_l & 7) * 2;
  const int vswz = ((vrow_l >> 1) & 1) << 2;

#define A64_MASK(T, SC, NKT)                                                                                     \
  {                                                                                                               \
    const int kb = (T) * A64_KT + 4 * h;                                                                          \
    _Pragma("unroll") for (int kt = 0; kt < (NKT); ++kt)                                                          \
    _Pragma("unroll") for (int i = 0; i < 16; ++i) {                                                              \
      const int key = kb + 32 * kt + (i & 3) + 8 * (i >> 2);                                                      \
      if (key >= S) SC[kt][i] = -INFINITY;                                                                        \
    }                                                                                                             \
  }

// NB = query blocks this wave owns (2; a wave at the end of a short sequence owns 1 or 0: it still stages K/V and
// keeps the barriers, but issues no MFMA / softmax work for rows that do not exist - on 643-token frames the third
// workgroup's waves own 2, 2, 1 (3 rows) and 0 blocks).  NKT = 32-key halves of this tile (2; 1 for a last tile with
// <= 32 keys: 643 = 10 x 64 + 3).
#define A64_TILE(T, BUF, FIRST, LAST, CLAMPNEXT, NOMAX, NB, NKT)                                                  \
  {                                                                                                               \
    const int buf = (BUF);                                                                                        \
    if (!(LAST)) { if constexpr (GLDS) glds_tile((T) + 1, CLAMPNEXT, buf ^ 1); else load_tile((T) + 1, CLAMPNEXT); } \
    f32x16 scA[2], scB[2];                                                                                        \
    bf16x8 pfA[2][2], pfB[2][2];                                                                                  \
    const char* kl = lds + buf * 8192 + krow_off;                                                                 \
    const char* vl = lds + 16384 + buf * 8192;                                                                    \
    const bool masktail = (LAST) && (S & (A64_KT - 1));                                                           \
    if ((NB) > 0) {                                                                                               \
      {                                                                                                           \
        const int off = (h ^ kswz) << 4;                                                                          \
        const bf16x8 a0 = *(const bf16x8*)(kl + off);                                                             \
        scA[0] = a64_mfma<F16>(a0, qfA[0], (f32x16)(0.f));                     \
        if ((NB) == 2) scB[0] = a64_mfma<F16>(a0, qfB[0], (f32x16)(0.f));      \
        if ((NKT) == 2) {                                                                                         \
          const bf16x8 a1 = *(const bf16x8*)(kl + 32 * 128 + off);                                                \
          scA[1] = a64_mfma<F16>(a1, qfA[0], (f32x16)(0.f));                   \
          if ((NB) == 2) scB[1] = a64_mfma<F16>(a1, qfB[0], (f32x16)(0.f));    \
        }                                                                                                         \
      }                                                                                                           \
      _Pragma("unroll") for (int s = 1; s < 4; ++s) {                                                             \
        const int off = ((2 * s + h) ^ kswz) << 4;                                                                \
        const bf16x8 a0 = *(const bf16x8*)(kl + off);                                                             \
        scA[0] = a64_mfma<F16>(a0, qfA[s], scA[0]);                            \
        if ((NB) == 2) scB[0] = a64_mfma<F16>(a0, qfB[s], scB[0]);             \
        if ((NKT) == 2) {                                                                                         \
          const bf16x8 a1 = *(const bf16x8*)(kl + 32 * 128 + off);                                                \
          scA[1] = a64_mfma<F16>(a1, qfA[s], scA[1]);                          \
          if ((NB) == 2) scB[1] = a64_mfma<F16>(a1, qfB[s], scB[1]);           \
        }                                                                                                         \
      }                                                                                                           \
      if (masktail) { A64_MASK(T, scA, NKT) if ((NB) == 2) { A64_MASK(T, scB, NKT) } }                            \
      a64_softmax<FIRST, NOMAX, MSUM, NKT, F16>(scA, mA, oA, lA, laccA, pfA);                                          \
      if ((NB) == 2) a64_softmax<FIRST, NOMAX, MSUM, NKT, F16>(scB, mB, oB, lB, laccB, pfB);                           \
      _Pragma("unroll") for (int kt = 0; kt < (NKT); ++kt)                                                        \
      _Pragma("unroll") for (int s2 = 0; s2 < 2; ++s2) {                                                          \
        const int row0 = 32 * kt + 16 * s2 + vrow_l;                                                              \
        _Pragma("unroll") for (int dt = 0; dt < 2; ++dt) {                                                        \
          const int ch = (4 * dt + vch_l) ^ vswz;                                                                 \
          const char* a = vl + row0 * 128 + (ch << 4) + vin_l;                                                    \
          const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(                                             \
              (__attribute__((address_space(3))) bf16x4*)LDS_PTR(a));                                             \
          const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(                                             \
              (__attribute__((address_space(3))) bf16x4*)LDS_PTR(a + 8 * 128));                                   \
          const bf16x8 vf = a64_cat4(lo, hi);                                                                     \
          oA[dt] = a64_mfma<F16>(vf, pfA[kt][s2], oA[dt]);                     \
          if ((NB) == 2) oB[dt] = a64_mfma<F16>(vf, pfB[kt][s2], oB[dt]);      \
        }                                                                                                         \
      }                                                                                                           \
    }                                                                                                             \
    if (!(LAST)) {                                                                                                \
      if constexpr (!GLDS) write_tile(buf ^ 1);                                                                   \
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                       \
      __syncthreads();                                                                                            \
    }                                                                                                             \
  }

// the whole key sweep for a wave that owns NB query blocks; the last tile takes the 32-key form when it holds <= 32 keys
#define A64_SWEEP(NOMAX, NB)                                                                                      \
  {                                                                                                               \
    if (nt == 1) {                                                                                                \
      if (half_last) { A64_TILE(0, 0, true, true, false, NOMAX, NB, 1) }                                          \
      else { A64_TILE(0, 0, true, true, false, NOMAX, NB, 2) }                                                    \
    } else {                                                                                                      \
      A64_TILE(0, 0, true, false, (tail && nt == 2), NOMAX, NB, 2)                                                \
      for (int t = 1; t < nt - 1; ++t) A64_TILE(t, (t & 1), false, false, (tail && t == nt - 2), NOMAX, NB, 2)    \
      if (half_last) { A64_TILE(nt - 1, ((nt - 1) & 1), false, true, false, NOMAX, NB, 1) }                       \
      else { A64_TILE(nt - 1, ((nt - 1) & 1), false, true, false, NOMAX, NB, 2) }                                 \
    }                                                                                                             \
  }

  const bool tail = (S & (A64_KT - 1)) != 0;
  // the last tile holds S - 64 (nt - 1) keys: when that is <= 32 its second 32-key half is skipped (frame-wise
  // sequences: 643 = 10 x 64 + 3); long sequences keep one code path (their last tile is one of a thousand)
  const bool half_last = (NW <= 4) && p.tailopt && (S - (nt - 1) * A64_KT <= 32);
  // query blocks this wave owns (see A64_TILE); long sequences (NW == 8) keep the single two-block path
  const int nb = (NW <= 4 && p.tailopt) ? (q0 >= S ? 0 : (q0 + 32 >= S ? 1 : 2)) : 2;
  // bounded-score test (see header): wave-uniform
  bool fast = false;       // the a-priori test (wave-uniform); the optimistic form then runs the bounded-score loop anyway
  if (!F16 && p.k2max && nb > 0 && !p.redo) {
    const float k2 = p.k2max[b * p.H + head];
    float qa = 0.f, qb = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float fa = (float)qfA[s][e], fb = (float)qfB[s][e];
        qa += fa * fa;
        qb += fb * fb;
      }
    qa += __shfl_xor(qa, 32, 64);
    qb += __shfl_xor(qb, 32, 64);
    fast = __all(fmaxf(qa, qb) * k2 <= A64_BOUND2);
  }
  const bool sure = fast;  // inside the a-priori bound: nothing to test afterwards
  if (!F16 && p.optim) fast = !p.redo;
  // static priority for the second-dispatched half (MI355X_MICROARCH.md, two waves per SIMD, item 4): the younger
  // wave of a SIMD loses every VALU arbitration at equal priority
  if (p.prio && wave >= NW / 2) __builtin_amdgcn_s_setprio(1);
  if constexpr (F16) {       // online-max loop only (see a64_mfma)
    if (nb == 2) A64_SWEEP(false, 2) else if (nb == 1) A64_SWEEP(false, 1) else A64_SWEEP(false, 0)
  } else if (nb == 2) {
    if (fast) A64_SWEEP(true, 2) else A64_SWEEP(false, 2)
  } else if (nb == 1) {
    if (fast) A64_SWEEP(true, 1) else A64_SWEEP(false, 1)
  } else {
    A64_SWEEP(true, 0)
  }

  if (!F16 && p.optim && !p.redo) {     // acceptance test of the optimistic bounded-score loop (workgroup-uniform branch)
    bool bad = false;
    if (nb > 0 && !sure) bad = a64_reject(lA + laccA[0], oA);
    if (nb > 1 && !sure) bad = bad || a64_reject(lB + laccB[0], oB);
    if (__syncthreads_or(bad)) {
      if (tid == 0) *a64_mark_ptr(p, b, qb, head, NW * 64) = A64_MARK;
      return;
    }
  }
  // finalize both blocks
#pragma unroll
  for (int blk = 0; blk < 2; ++blk) {
    const float lsum = blk ? lB + laccB[0] : lA + laccA[0];
    const float inv = 1.0f / (lsum + __shfl_xor(lsum, 32, 64));
    const int row = q0 + 32 * blk + r;
    if (row < S) {
      bf16_t* optr = p.o + (long)b * p.o_batch_stride + (long)row * p.o_tok_stride + head * 64;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x16& ov = blk ? oB[dt] : oA[dt];
          u32x2 w;
          w[0] = a64_pack<F16>(ov[4 * g + 0] * inv, ov[4 * g + 1] * inv);
          w[1] = a64_pack<F16>(ov[4 * g + 2] * inv, ov[4 * g + 3] * inv);
          *(u32x2*)(optr + 32 * dt + 8 * g + 4 * h) = w;
        }
    }
  }
  // which softmax loop this wave ran (diagnostic, off unless the caller registered a counter block): one no-return
  // atomic per wave after its stores, spread over 32 slots so that same-address atomics do not queue up in L2
  if (p.stats && lane == 0 && nb > 0)
    atomicAdd(p.stats + (NW == 8 ? 0 : 64) + (fast ? 0 : 32) + (blockIdx.x & 31), 1u);
}

template <int NW, bool GLDS = false, bool MSUM = false, bool F16 = false>
__global__ __launch_bounds__(NW * 64, (NW == 2 ? 4 : 2)) void attn_fwd64_kernel(Attn64Params p) {
  __shared__ __attribute__((aligned(16))) char lds[32768];
  a64_body<NW, GLDS, MSUM, F16>(p, lds, blockIdx.x);
}

// The follow-up launch of the optimistic form (p.redo = 1) on a SMALL grid: workgroup j looks at the marks of the primary
// launch's workgroups j, j + G, j + 2 G, ... in one batch of loads (thread t: candidate j + t G) and runs the online-max
// body for the marked ones.  With nothing rejected - the usual case - that is one load per workgroup of a 512-workgroup
// grid: 5.6 us on average (3.5-4 us at best) in the rocprofv3 trace of the bench where the full grid took 7.5-7.7 us of
// dependent-load rounds (94 attention calls per chunk: 0.7 -> 0.5 ms); with everything rejected the 512 workgroups keep
// the card as busy as the full grid would.  G is a multiple of 8, so a
// candidate stays on the XCD the primary launch ran it on (xcd_remap).  Spills in THIS instance do not matter.
template <int NW>
__global__ __launch_bounds__(NW * 64, 2) void attn_redo64_kernel(Attn64Params p) {
  __shared__ __attribute__((aligned(16))) char lds[32768];
  __shared__ unsigned char marked[NW * 64];
  const int nwg = p.nqb * p.H * p.B, G = (int)gridDim.x, tid = threadIdx.x;
  const int per = (nwg + G - 1) / G;              // <= NW * 64: the launcher sizes the grid
  bool m = false;
  if (tid < per) {
    const int c = (int)blockIdx.x + tid * G;
    if (c < nwg) {
      const int id = xcd_remap(c, nwg);
      m = __builtin_nontemporal_load(a64_mark_ptr(p, id / (p.nqb * p.H), id % p.nqb, (id / p.nqb) % p.H, NW * 64)) == A64_MARK;
    }
  }
  marked[tid] = m;
  if (!__syncthreads_or(m)) return;
  for (int t = 0; t < per; ++t)
    if (marked[t]) {                              // workgroup-uniform
      a64_body<NW, true, true, false>(p, lds, (int)blockIdx.x + t * G);
      __syncthreads();                            // the next candidate's staging must not overtake this one's last reads
    }
}

// Staging ring and tile macros of the hand-placed kernels: attn_fwd64b_kernel below and, in development builds,
// attn_fwd64a_kernel (attn64a_kernel.inc).  They expand inside the kernels, next to the locals they name.  The
// pipelined loop computes Q.K^T of tile t + 1 during tile t, so K is staged two tiles ahead and V one: the K ring is three
// slots deep (slot t % 3 at LDS offsets 0 / 8 192 / 32 768), the V ring two (16 384 + 8 192 (t & 1)).  A64A_BLOCK is one
// 32-row query block on one 64-key tile in C++ (the bounded-score form of a64_body's tile): tile 0 and the last three.
#define A64A_KSLOT(T) (((T) % 3) == 0 ? 0 : (((T) % 3) == 1 ? 8192 : 32768))
#define A64A_VSLOT(T) (16384 + ((T) & 1) * 8192)
#define A64A_LDSADDR(P) ((unsigned)(__UINTPTR_TYPE__)((__attribute__((address_space(3))) void*)(P)))
#define A64A_BLOCK(T, FIRST, LAST, QF, OACC, LSUM, LACC, MREF)                                                      \
  {                                                                                                               \
    f32x16 sc[2];                                                                                                 \
    bf16x8 pf[2][2];                                                                                              \
    _Pragma("unroll") for (int s = 0; s < 4; ++s) {                                                               \
      const int off = ((2 * s + h_) ^ kswz) << 4;                                                                 \
      const bf16x8 a0 = *(const bf16x8*)(kl + off);                                                               \
      const bf16x8 a1 = *(const bf16x8*)(kl + 32 * 128 + off);                                                    \
      sc[0] = a64_mfma<F16>(a0, QF[s], s == 0 ? (f32x16)(0.f) : sc[0]);                                           \
      sc[1] = a64_mfma<F16>(a1, QF[s], s == 0 ? (f32x16)(0.f) : sc[1]);                                           \
    }                                                                                                             \
    if ((LAST) && tail) { A64_MASK(T, sc, 2) }                                                                    \
    a64_softmax<FIRST, true, true, 2, F16>(sc, MREF, OACC, LSUM, LACC, pf);                                       \
    _Pragma("unroll") for (int kt = 0; kt < 2; ++kt)                                                              \
    _Pragma("unroll") for (int s2 = 0; s2 < 2; ++s2) {                                                            \
      const int row0 = 32 * kt + 16 * s2 + vrow_l;                                                                \
      _Pragma("unroll") for (int dt = 0; dt < 2; ++dt) {                                                          \
        const int ch = (4 * dt + vch_l) ^ vswz;                                                                   \
        const char* a = vl + row0 * 128 + (ch << 4) + vin_l;                                                      \
        const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)LDS_PTR(a)); \
        const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(                                               \
            (__attribute__((address_space(3))) bf16x4*)LDS_PTR(a + 8 * 128));                                     \
        OACC[dt] = a64_mfma<F16>(a64_cat4(lo, hi), pf[kt][s2], OACC[dt]);                                         \
      }                                                                                                           \
    }                                                                                                             \
  }

#ifdef PI3_DEV_VARIANTS   // knob attn_asm = 1 (development builds): measured 2.5 % behind attn_fwd64b_kernel, bit-identical
#include "attn64a_kernel.inc"
#endif   // PI3_DEV_VARIANTS

// ---------------------------------------------------------------------------------------------------------------------
// attn_fwd64b_kernel (round 5, late): the same hand-placed loop with ONE wave per SIMD - four waves per workgroup, 128 query
// rows (four 32-row blocks) per wave, the whole 512-register file per wave (launch bound 256 x 1).  Every K / V fragment
// read from LDS then feeds four MFMAs instead of two: half the fragment traffic per FLOP, which is what still pays in a
// power-limited loop (-2.3 ... -2.7 % in tools/micro/attn_loop_bench).  Generated by `tools/gen_attn_asm2.py 4 ... product`
// (attn64b_loop.inc): O and the row sums are "+a" operands, Q is loaded inside the block into a192..a255, the loop's
// state sits in v66..v253.  Same workgroup -> rows map (512 rows), same rings, same arithmetic in the same order per row
// as attn_fwd64a_kernel, so the results are bit-identical and a rejected workgroup's mark is found by the same follow-up
// launch.  Launched only for the optimistic form (knob attn_nomax = 2) and nt >= 8: there is no second body in here.
// ---------------------------------------------------------------------------------------------------------------------
#include <attn64b_loop.inc>
__global__ __launch_bounds__(256, 1) void attn_fwd64b_kernel(Attn64Params p) {
  __shared__ __attribute__((aligned(1024))) char lds[40960];
  constexpr bool F16 = false;
  const int tid = threadIdx.x, wave = tid >> 6;
  const int nwg = p.nqb * p.H * p.B;
  const int id = xcd_remap(blockIdx.x, nwg);
  const int qb = id % p.nqb;
  const int head = (id / p.nqb) % p.H;
  const int b = id / (p.nqb * p.H);
  const int S = p.S;
  const int nt = (S + A64_KT - 1) / A64_KT;
  const int q0 = qb * 512 + wave * 128;
  const bf16_t* qbase = p.q + (long)b * p.batch_stride + head * 64;
  const bf16_t* kbase = p.k + (long)b * p.batch_stride + head * 64;
  const bf16_t* vbase = p.v + (long)b * p.batch_stride + head * 64;
  const long tile_bytes = (long)A64_KT * p.tok_stride * 2;
  const bool tail = (S & (A64_KT - 1)) != 0;

  int kswz, krow_off, vrow_l, vch_l, vin_l, vswz, r_, h_, drow0, dpos;
#define A64B_LANE_CONSTS(LANE)                                                                                     \
  {                                                                                                               \
    r_ = (LANE) & 31; h_ = (LANE) >> 5;                                                                           \
    drow0 = wave * 16 + ((LANE) >> 3); dpos = (LANE) & 7;          /* pieces 2 wave, 2 wave + 1: rows drow0, drow0 + 8 */ \
    kswz = (r_ >> 1) & 7;                                                                                         \
    krow_off = r_ * 128;                                                                                          \
    const int gi = (LANE) & 15, gg = ((LANE) >> 4) & 1;                                                           \
    vrow_l = 4 * h_ + (gi >> 2);                                                                                  \
    const int vcol_l = 16 * gg + 4 * (gi & 3);                                                                    \
    vch_l = vcol_l >> 3;                                                                                          \
    vin_l = (vcol_l & 7) * 2;                                                                                     \
    vswz = ((vrow_l >> 1) & 1) << 2;                                                                              \
  }
  A64B_LANE_CONSTS(tid & 63)

  // a-priori test (the shortcut of the optimistic form: a workgroup wholly inside the bound is not tested afterwards)
  bool fast = false;
  if (p.k2max) {
    const float k2 = p.k2max[b * p.H + head];
    float qn = 0.f;
#pragma unroll
    for (int blk = 0; blk < 4; ++blk) {
      const bf16_t* pq = qbase + (long)min(q0 + 32 * blk + r_, S - 1) * p.tok_stride;
      float a = 0.f;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const bf16x8 f = *(const bf16x8*)(pq + 16 * s + 8 * h_);
#pragma unroll
        for (int e = 0; e < 8; ++e) a += (float)f[e] * (float)f[e];
      }
      a += __shfl_xor(a, 32, 64);
      qn = fmaxf(qn, a);
    }
    fast = __all(qn * k2 <= A64_BOUND2);
  }
  const bool sure = __syncthreads_and(fast) != 0;

  f32x16 o[4][2];
  f32x4 lacc[4];
  float msc[4], lsc[4];
#pragma unroll
  for (int blk = 0; blk < 4; ++blk) {
    o[blk][0] = o[blk][1] = (f32x16)(0.f);
    lacc[blk] = (f32x4)(0.f);
    msc[blk] = lsc[blk] = 0.f;
  }
  auto dma_k = [&](int T) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int drow = drow0 + 8 * i;
      int grow = T * A64_KT + drow;
      grow = grow < S ? grow : S - 1;                  // only the last, partial tile clamps
      a64_glds16((const char*)(kbase + (long)grow * p.tok_stride) + ((dpos ^ ((drow >> 1) & 7)) << 4),
                 lds + A64A_KSLOT(T) + (wave * 2 + i) * 1024);
    }
  };
  auto dma_v = [&](int T) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int drow = drow0 + 8 * i;
      int grow = T * A64_KT + drow;
      grow = grow < S ? grow : S - 1;
      a64_glds16((const char*)(vbase + (long)grow * p.tok_stride) + ((dpos ^ (((drow >> 1) & 1) << 2)) << 4),
                 lds + A64A_VSLOT(T) + (wave * 2 + i) * 1024);
    }
  };
  dma_k(0);
  dma_v(0);
  dma_k(1);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // one 64-key tile in C++ (four of ~1 000): the four blocks one after the other, Q fragments of a block loaded for it
#define A64B_TILE(T, FIRST, LAST)                                                                                  \
  {                                                                                                               \
    if ((T) + 1 < nt) dma_v((T) + 1);                                                                             \
    if ((T) + 2 < nt) dma_k((T) + 2);                                                                             \
    const char* kl = lds + A64A_KSLOT(T) + krow_off;                                                              \
    const char* vl = lds + A64A_VSLOT(T);                                                                         \
    _Pragma("unroll") for (int blk = 0; blk < 4; ++blk) {                                                         \
      bf16x8 qf[4];                                                                                               \
      const bf16_t* pq = qbase + (long)min(q0 + 32 * blk + r_, S - 1) * p.tok_stride;                             \
      _Pragma("unroll") for (int s = 0; s < 4; ++s) qf[s] = *(const bf16x8*)(pq + 16 * s + 8 * h_);               \
      A64A_BLOCK(T, FIRST, LAST, qf, o[blk], lsc[blk], lacc[blk], msc[blk])                                       \
      __builtin_amdgcn_sched_barrier(0);                                                                          \
    }                                                                                                             \
    if (!(LAST)) {                                                                                                \
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                            \
      __syncthreads();                                                                                            \
    }                                                                                                             \
  }
#define h h_      /* A64_MASK reads `h` */
  A64B_TILE(0, true, false)
  {
    const unsigned lds0 = A64A_LDSADDR(lds);
    const unsigned ka0 = lds0 + 8192 + krow_off + ((h_ ^ kswz) << 4);          // d-steps 1..3: ^ 32 s (inside the block)
    const unsigned va0 = lds0 + 16384 + vrow_l * 128 + ((vch_l ^ vswz) << 4) + vin_l;      // dt 1: ^ 64
    unsigned ksrc[2], vsrc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int drow = drow0 + 8 * i;
      ksrc[i] = (unsigned)(drow * p.tok_stride * 2) + ((dpos ^ ((drow >> 1) & 7)) << 4);
      vsrc[i] = (unsigned)(drow * p.tok_stride * 2) + ((dpos ^ (((drow >> 1) & 1) << 2)) << 4);
    }
    const bf16_t* qp[4];
#pragma unroll
    for (int blk = 0; blk < 4; ++blk) qp[blk] = qbase + (long)min(q0 + 32 * blk + r_, S - 1) * p.tok_stride + 8 * h_;
    const unsigned cnt = (unsigned)(nt - 4);
    const unsigned long long kg = (unsigned long long)(__UINTPTR_TYPE__)kbase + 3ull * (unsigned long long)tile_bytes;
    const unsigned long long vg = (unsigned long long)(__UINTPTR_TYPE__)vbase + 2ull * (unsigned long long)tile_bytes;
    const unsigned kg_lo = __builtin_amdgcn_readfirstlane((unsigned)kg), kg_hi = __builtin_amdgcn_readfirstlane((unsigned)(kg >> 32));
    const unsigned vg_lo = __builtin_amdgcn_readfirstlane((unsigned)vg), vg_hi = __builtin_amdgcn_readfirstlane((unsigned)(vg >> 32));
    const unsigned long long kgs = ((unsigned long long)kg_hi << 32) | kg_lo, vgs = ((unsigned long long)vg_hi << 32) | vg_lo;
    const unsigned tb = __builtin_amdgcn_readfirstlane((unsigned)tile_bytes);
    const unsigned kd0 = __builtin_amdgcn_readfirstlane(lds0 + wave * 2048);
    asm volatile(A64B4_LOOP_ASM
                 : [o00] "+a"(o[0][0]), [o01] "+a"(o[0][1]), [o10] "+a"(o[1][0]), [o11] "+a"(o[1][1]), [o20] "+a"(o[2][0]),
                   [o21] "+a"(o[2][1]), [o30] "+a"(o[3][0]), [o31] "+a"(o[3][1]), [l0] "+a"(lacc[0]), [l1] "+a"(lacc[1]),
                   [l2] "+a"(lacc[2]), [l3] "+a"(lacc[3])
                 : [ka0] "v"(ka0), [va0] "v"(va0), [ksrc0] "v"(ksrc[0]), [ksrc1] "v"(ksrc[1]), [vsrc0] "v"(vsrc[0]),
                   [vsrc1] "v"(vsrc[1]), [qp0] "v"(qp[0]), [qp1] "v"(qp[1]), [qp2] "v"(qp[2]), [qp3] "v"(qp[3]), [cnt] "s"(cnt),
                   [kg] "s"(kgs), [vg] "s"(vgs), [tb] "s"(tb), [kd0] "s"(kd0)
                 : "memory", "scc", "vcc", "m0", A64B4_CLOBBER_V, A64B4_CLOBBER_A, A64B4_CLOBBER_S);
  }
  {
    int lane2 = (int)(threadIdx.x & 63);
    asm volatile("" : "+v"(lane2));                    // opaque: nothing derived from the lane id before the loop stays live
    A64B_LANE_CONSTS(lane2)
  }
  A64B_TILE(nt - 3, false, false)
  A64B_TILE(nt - 2, false, false)
  A64B_TILE(nt - 1, false, true)
#undef h

  if (!sure) {         // acceptance test of the optimistic loop (a64_reject); workgroup-uniform
    bool bad = false;
#pragma unroll
    for (int blk = 0; blk < 4; ++blk) bad = bad || a64_reject(lsc[blk] + lacc[blk][0], o[blk]);
    if (__syncthreads_or(bad)) {
      if (tid == 0) *a64_mark_ptr(p, b, qb, head, 512) = A64_MARK;
      return;
    }
  }
  if (p.stats && (threadIdx.x & 63) == 0) atomicAdd(p.stats + 0 + (blockIdx.x & 31), 2u);      // two 64-row wave units per wave
#pragma unroll
  for (int blk = 0; blk < 4; ++blk) {
    const float lsum = lsc[blk] + lacc[blk][0];
    const float inv = 1.0f / (lsum + __shfl_xor(lsum, 32, 64));
    const int row = q0 + 32 * blk + r_;
    if (row < S) {
      bf16_t* optr = p.o + (long)b * p.o_batch_stride + (long)row * p.o_tok_stride + head * 64;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x16& ov = o[blk][dt];
          u32x2 w;
          w[0] = pack_bf16x2(ov[4 * g + 0] * inv, ov[4 * g + 1] * inv);
          w[1] = pack_bf16x2(ov[4 * g + 2] * inv, ov[4 * g + 3] * inv);
          *(u32x2*)(optr + 32 * dt + 8 * g + 4 * h_) = w;
        }
    }
  }
}

// max over keys of |k|^2 per (batch, head) for the bounded-score test; out must be zeroed (non-negative floats order
// like their bit patterns, so the reduction is an integer atomicMax)
#define A64_KNORM_BLOCKS 24   // blocks per (batch, head): 24 * 16 heads = 384 blocks, one atomic each
__global__ __launch_bounds__(256) void a64_knorm_kernel(const bf16_t* __restrict__ k, long tok_stride,
                                                        long batch_stride, int S, int H, float* __restrict__ out) {
  // 8 lanes per key row (16 bytes each: one full 128-byte line per row and instruction), 32 rows per pass; the block
  // strides over the sequence and issues ONE atomic (thousands of same-address atomics serialise in L2: the first
  // version spent 160 of its 190 us there)
  __shared__ float red[4];
  const int head = blockIdx.y, b = blockIdx.z;
  const int sub = threadIdx.x & 7, rl = threadIdx.x >> 3;
  const bf16_t* base = k + (long)b * batch_stride + head * 64 + sub * 8;
  float best = 0.f;
  for (int row0 = blockIdx.x * 128; row0 < S; row0 += A64_KNORM_BLOCKS * 128) {
    float s[4];
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
      const int row = row0 + pass * 32 + rl;
      s[pass] = 0.f;
      if (row < S) {
        const u32x4 w = *(const u32x4*)(base + (long)row * tok_stride);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float lo = __uint_as_float(w[j] << 16), hi = __uint_as_float(w[j] & 0xffff0000u);
          s[pass] += lo * lo + hi * hi;
        }
      }
    }
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
      float v = s[pass];
      v += __shfl_xor(v, 1, 64);
      v += __shfl_xor(v, 2, 64);
      v += __shfl_xor(v, 4, 64);
      best = fmaxf(best, v);
    }
  }
  best = wave_max(best);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0)
    atomicMax((unsigned*)&out[b * H + head], __float_as_uint(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]))));
}

// max_s |k[b, s, h, :]|^2 into out[B*H] (must be zeroed): the pre-pass of the bounded-score path, also used by the
// two-pass form of pi3_gemm_qkv.
int pi3_attention_knorm_launch(const void* k, long tok_stride, long batch_stride, int B, int S, int H, float* out,
                               hipStream_t stream) {
  hipLaunchKernelGGL(a64_knorm_kernel, dim3(A64_KNORM_BLOCKS, H, B), dim3(256), 0, stream, (const bf16_t*)k, tok_stride,
                     batch_stride, S, H, out);
  return pi3_check_launch("a64_knorm");
}

#ifdef PI3_DEV_VARIANTS
int pi3_attention64p_launch(const Attn64Params& p, long nwg, hipStream_t stream);   // attn64p.hip: software-pipelined form
#endif

// Diagnostic: counters of the softmax loop each wave of the 64-row kernel took.  counters = caller-owned DEVICE memory of
// 128 uint32, zeroed by the caller: [kind][path][32 slots], kind 0 = eight-wave workgroups (the long / global sequences),
// 1 = four- and two-wave workgroups (frame-wise sequences); path 0 = bounded-score loop (no running max), 1 = online-max
// loop.  Sum the 32 slots.  NULL switches it off (the default).  Process-wide; set it while no attention launch is in
// flight.  The pointer is read at launch time and NEVER while the launch stream is being captured: a captured hipGraph
// would keep the caller's pointer and write through it on every later replay, long after the caller freed the tensor.
static unsigned* g_attn_stats = nullptr;
extern "C" int pi3_attention_path_counters(unsigned int* counters) {
  g_attn_stats = counters;
  return PI3_OK;
}

static unsigned* a64_stats_for(hipStream_t stream) {
  if (!g_attn_stats) return nullptr;
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream, &st) != hipSuccess || st != hipStreamCaptureStatusNone) return nullptr;
  return g_attn_stats;
}


// Called by pi3_attention (attn.hip); same argument meaning, plus nw_req (0: 512-row workgroups, 4: four-wave workgroups).
// k2max_ws: caller-provided [B*H] floats (or null -> online-max loop); k2max_ready: already filled by the producer.
//
// The product library launches: attn_fwd64b_kernel (long sequences, optimistic bounded-score loop, knob attn_asm = 2, the
// default) or the compiler-scheduled attn_fwd64_kernel<8, true, true> (knob attn_asm = 0, knob attn_nomax = 0 / 1, and
// sequences of fewer than eight key tiles); attn_fwd64_kernel<4, true, true> for frame-wise sequences; the IEEE-half
// forms <8 / 4, true, false, true> for MoGe; attn_redo64_kernel<8 / 4> behind the optimistic form.  Everything else
// (attn_fwd64a_kernel = knob attn_asm 1, two-wave workgroups, LDS staging without DMA, vector-pipe row sums, wave
// priorities, the software-pipelined attn64p.hip) is a development variant: -DPI3_DEV_VARIANTS, make dev.
int pi3_attention64_launch(const void* q, const void* k, const void* v, long tok_stride, long batch_stride, void* o,
                           long o_tok_stride, long o_batch_stride, int B, int S, int H, float* k2max_ws,
                           int k2max_ready, int nw_req, hipStream_t stream, int f16) {
  Attn64Params p;
  p.q = (const bf16_t*)q; p.k = (const bf16_t*)k; p.v = (const bf16_t*)v;
  p.tok_stride = tok_stride; p.batch_stride = batch_stride;
  p.o = (bf16_t*)o; p.o_tok_stride = o_tok_stride; p.o_batch_stride = o_batch_stride;
  // development switches (constants in the product build, common.h): PI3_ATTN_NW 4 = 256-row workgroups for long sequences;
  // knob attn_frame_nw 2 = two-wave workgroups for frame-wise sequences (643 tokens are 10 full 64-row wave blocks + 3
  // rows: three four-wave workgroups give 12 wave slots of which the third workgroup's last half idles; six two-wave
  // workgroups end in a short one - measured slower); PI3_ATTN_GLDS 0 = staging through registers; PI3_ATTN_MSUM 0 = row
  // sums on the vector pipe; PI3_ATTN_PRIO 1 = s_setprio 1 for the second half of a workgroup's waves; PI3_ATTN_TAILOPT 0 =
  // every wave runs two query blocks and full key tiles; PI3_ATTN_PIPE 1 = attn64p.hip
  const int nw_long = PI3_DEV_ENV_INT("PI3_ATTN_NW", 8);
  const int nw_frame = (int)PI3_DEV_KNOB("attn_frame_nw", 4) == 2 ? 2 : 4;
  // nw_req = 4: the caller (short, frame-wise sequences) wants 256-row workgroups
  // the IEEE-half instances exist for eight and four waves only: the grid follows the instance that is launched
  const int nw = f16 ? (nw_req == 4 ? 4 : 8) : (nw_req == 4 ? nw_frame : nw_long);
  const int qrows = nw * 64;
  p.S = S; p.H = H; p.B = B; p.nqb = (S + qrows - 1) / qrows;
  const long nwg = (long)p.nqb * H * B;
  const int glds = PI3_DEV_ENV_INT("PI3_ATTN_GLDS", 1);
  const int msum = PI3_DEV_ENV_INT("PI3_ATTN_MSUM", 1);
  (void)glds; (void)msum;
  // knob attn_nomax (PI3_ATTN_NOMAX): 0 = always the online-max loop (A/B knob, how the tests reach that loop, and the
  // worst case bench.py reports beside the headline: real weights may not keep |q| max|k| inside the bound); 1 = the
  // a-priori test on max |k|^2; 2 (default) = optimistic bounded-score loop + acceptance test + follow-up launch
  const int nomax = (int)PI3_KNOB("attn_nomax", 2);
  p.k2max = nullptr;
  p.optim = nomax == 2;
  p.redo = 0;
  p.dbg = nullptr;
  p.stats = a64_stats_for(stream);
  p.prio = PI3_DEV_ENV_INT("PI3_ATTN_PRIO", 0);
  p.tailopt = PI3_DEV_ENV_INT("PI3_ATTN_TAILOPT", 1);

  if (f16) {      // IEEE-half operands: LDS-DMA staging, online-max loop, eight- or four-wave workgroups
    p.stats = nullptr;     // not a choice of path (half always takes the online-max loop): MoGe's launches stay out of pi3's counters
    if (nw == 4)
      hipLaunchKernelGGL((attn_fwd64_kernel<4, true, false, true>), dim3((unsigned)nwg), dim3(256), 0, stream, p);
    else
      hipLaunchKernelGGL((attn_fwd64_kernel<8, true, false, true>), dim3((unsigned)nwg), dim3(512), 0, stream, p);
    return pi3_check_launch("attn_fwd64 (f16)");
  }
  if (nomax && k2max_ws) {
    if (!k2max_ready) {
      if (hipMemsetAsync(k2max_ws, 0, (size_t)B * H * sizeof(float), stream) != hipSuccess) {
        pi3_set_error("attn_fwd64: hipMemsetAsync failed");
        return PI3_ERR_LAUNCH;
      }
      hipLaunchKernelGGL(a64_knorm_kernel, dim3(A64_KNORM_BLOCKS, H, B), dim3(256), 0, stream, p.k, tok_stride,
                         batch_stride, S, H, k2max_ws);
    }
    p.k2max = k2max_ws;
  }
#ifdef PI3_DEV_VARIANTS
  if (PI3_DEV_ENV_INT("PI3_ATTN_PIPE", 0) && nw == 8) return pi3_attention64p_launch(p, nwg, stream);
#endif
  // knob attn_asm (PI3_ATTN_ASM): the 512-row workgroups' kernel.  2 (default; any non-zero value in the product build) =
  // attn_fwd64b_kernel, the hand-placed loop with one wave per SIMD x 128 rows (optimistic form and >= 8 key tiles); 0 =
  // the compiler-scheduled kernel.  Development builds: 1 = attn_fwd64a_kernel, the same loop with two waves per SIMD x 64
  // rows (workgroups it does not cover run the compiler-scheduled body inside it).  Bit-identical results.
  const int asm_form = (int)PI3_KNOB("attn_asm", 2);
  const bool use_asm = asm_form != 0;
  const bool long_enough = S >= 8 * A64_KT - (A64_KT - 1);
  auto launch = [&](bool allow_asm) {
#ifdef PI3_DEV_VARIANTS
    if (nw == 8 && glds && msum && p.optim && allow_asm && asm_form == 2 && long_enough)
      hipLaunchKernelGGL(attn_fwd64b_kernel, dim3((unsigned)nwg), dim3(256), 0, stream, p);
    else if (nw == 8 && glds && msum && (p.k2max || p.optim) && allow_asm)
      hipLaunchKernelGGL(attn_fwd64a_kernel, dim3((unsigned)nwg), dim3(512), 0, stream, p);
    else if (nw == 8 && glds && msum)
      hipLaunchKernelGGL((attn_fwd64_kernel<8, true, true>), dim3((unsigned)nwg), dim3(512), 0, stream, p);
    else if (nw == 8 && glds)
      hipLaunchKernelGGL((attn_fwd64_kernel<8, true>), dim3((unsigned)nwg), dim3(512), 0, stream, p);
    else if (nw == 8)
      hipLaunchKernelGGL(attn_fwd64_kernel<8>, dim3((unsigned)nwg), dim3(512), 0, stream, p);
    else if (nw == 2)
      hipLaunchKernelGGL((attn_fwd64_kernel<2, true, true>), dim3((unsigned)nwg), dim3(128), 0, stream, p);
    else if (glds && msum)   // 4 waves: two independent workgroups per CU, the two waves of a SIMD drift out of phase
      hipLaunchKernelGGL((attn_fwd64_kernel<4, true, true>), dim3((unsigned)nwg), dim3(256), 0, stream, p);
    else
      hipLaunchKernelGGL(attn_fwd64_kernel<4>, dim3((unsigned)nwg), dim3(256), 0, stream, p);
#else
    if (nw == 8 && p.optim && allow_asm && long_enough)
      hipLaunchKernelGGL(attn_fwd64b_kernel, dim3((unsigned)nwg), dim3(256), 0, stream, p);
    else if (nw == 8)
      hipLaunchKernelGGL((attn_fwd64_kernel<8, true, true>), dim3((unsigned)nwg), dim3(512), 0, stream, p);
    else     // 4 waves: two independent workgroups per CU, the two waves of a SIMD drift out of phase
      hipLaunchKernelGGL((attn_fwd64_kernel<4, true, true>), dim3((unsigned)nwg), dim3(256), 0, stream, p);
#endif
  };
  launch(use_asm);
  if (p.optim) {        // the follow-up launch: workgroups that rejected the bounded-score loop run the online-max loop (a64_reject)
    p.redo = 1;
    if (glds != 0 && msum != 0 && (nw == 8 || nw == 4)) {
      const long threads = nw * 64;
      long grid = nwg < 512 ? nwg : 512;
      const long need = (nwg + threads - 1) / threads;          // at most one candidate per thread
      if (grid < need) grid = (need + 7) / 8 * 8;
      if (nw == 8) hipLaunchKernelGGL(attn_redo64_kernel<8>, dim3((unsigned)grid), dim3(512), 0, stream, p);
      else hipLaunchKernelGGL(attn_redo64_kernel<4>, dim3((unsigned)grid), dim3(256), 0, stream, p);
    } else {
      launch(false);
    }
  }
  return pi3_check_launch("attn_fwd64");
}
