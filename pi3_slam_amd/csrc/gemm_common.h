// Shared by gemm.hip (128x128 and narrow tiles) and gemm256.hip (256x256 pipelined tile, with gemm256_dev.inc): the
// parameter block GemmParams, the one launch path gemm_launch, the (out_dtype, act) -> template instance mapping
// gemm_dispatch, and the fused register-direct epilogue gemm_epilogue.
#pragma once
#include "common.h"

// Every field has a default: an entry point starts from GemmParams{} and sets what its own arguments supply, so no byte
// of a launched block is indeterminate and a new field needs no edit where it is not used.
struct GemmParams {
  const void* A = nullptr; long lda = 0;   // [M][K], element stride
  const void* W = nullptr; long ldw = 0;   // [N][K]
  int M = 0, N = 0, K = 0;
  const float* bias = nullptr;             // [N] or null
  const float* gamma = nullptr;            // [N] or null  (LayerScale)
  const float* resid = nullptr; long ldr = 0;  // fp32 [*][ldr] residual source (indexed by the remapped row) or null
  void* out = nullptr; long ldo = 0;       // bf16 or f32
  int rpg = 0, gstride = 0, goff = 0;      // row remap: orow = (m / rpg) * gstride + goff + (m % rpg); rpg == 0 -> orow = m
  const float* addtab = nullptr; long ldadd = 0;  // optional f32 table [rpg][ldadd], row (m % rpg), added after everything else
  float qscale = 1.f; int qcols = 0;       // columns n < qcols are multiplied by qscale (softmax scale folded into q)
  // implicit-GEMM 3x3 convolution, replicate padding (moge/model/modules.py:47-60): A is an NHWC image
  // [B][cH][cW][cC] (cC % 64 == 0), row m = pixel, K = 9 * cC with k = (ky*3 + kx) * cC + ci; cW == 0 -> plain GEMM
  int cH = 0, cW = 0, cC = 0;
  int f16 = 0;               // gemm.hip kernels only: the 16-bit operands (and a 16-bit output) are IEEE half, not bf16:
                             // v_mfma_f32_16x16x32_f16, same rate - MoGe, which the reference runs under fp16 autocast
  // the next five (and abl) are set in one place, pi3_gemm256_try (gemm256.hip), where the 256x256 launch is prepared
  int tile_gm = 0;           // gemm256: m-tiles per scheduling group (0 = default 8); consecutive ids walk a group's m-tiles
  int tile_order = 0;        // gemm256: 0 = m-tiles first inside a group, 1 = column tiles first
  int stagger_ns = 0;        // gemm256 (persistent form): workgroup b starts b * stagger_ns later (0 = all at once)
  int ilv_prio = 0;          // interleaved K loop (knob gemm_ilv = 2 / 3): 1 = waves 4-7 at priority 1, 2 = the two waves of a SIMD take turns
  int rpref = 0;             // gemm256, f32 output with a residual: touch the tile's residual lines during the last K tiles
#ifdef PI3_DEV_ABLATIONS
  int abl = 0;               // timing-only ablation bits (development builds; results are wrong)
#endif
  // fused q/k epilogue of the packed qkv projection (gemm256 only; FlashAttentionRope.forward,
  // pi3/models/layers/attention.py:323-334): columns [0, H*64) = q, [H*64, 2*H*64) = k, rest = v.  For q and k heads:
  // per-head LayerNorm(64) (optional: qk_w != null), RoPE-2D (optional), softmax scale folded into q, and max_s |k|^2
  // per (attention batch, head) for the bounded-score attention path (optional: k2max != null).
  int qk_mode = 0;           // 0 = off
  int qk_H = 0, qk_T = 0;    // heads; tokens per frame (row % T indexes pos)
  const int* qk_pos = nullptr;     // [T][2] (y, x) or null (no RoPE)
  const float* qk_cs = nullptr;    // [npos][16][2] (cos, sin)
  const float* qk_qw = nullptr; const float* qk_qb = nullptr; const float* qk_kw = nullptr; const float* qk_kb = nullptr;   // LayerNorm(64) affine or null
  float qk_eps = 0.f, qk_qscale = 0.f;
  float* qk_k2max = nullptr; int qk_attnS = 0;   // k2max[(row / attnS) * H + head]
};

// The one launch path: opts the kernel in to its LDS size (once per device; the mask is a static of this instantiation,
// one per kernel instance), launches it and checks the launch.  `what` names the family in the error texts.
template <void (*KERN)(GemmParams)>
static int gemm_launch(const char* what, int grid, int threads, int lds_bytes, const GemmParams& p, hipStream_t stream) {
  static unsigned long long optin = 0;
  if (int rc = pi3_lds_optin((const void*)KERN, lds_bytes, &optin, what)) return rc;
  hipLaunchKernelGGL(KERN, dim3(grid), dim3(threads), lds_bytes, stream, p);
  return pi3_check_launch(what);
}

// (out_dtype, act) -> template instance.  A kernel family lists the pairs it instantiates, OutActs<OutAct<OUT16, ACT>...>
// (OUT16: out_dtype == 0); gemm_dispatch calls launch(OutAct<...>{}), a generic lambda around the family's launcher
// (launch_x<oa.OUT16, oa.ACT, ...>(p, stream)), for the listed pair that matches and returns its code, or 1 - "not
// applicable", as pi3_gemm256_try - when none does.  (Deduced return type: a call instantiates its launchers where it
// stands, so a file's kernels are emitted in the order its entry points list them.)
template <bool OUT16_, int ACT_> struct OutAct { static constexpr bool OUT16 = OUT16_; static constexpr int ACT = ACT_; };
template <class... PAIRS> struct OutActs {};
template <class... PAIRS, class LAUNCH>
static auto gemm_dispatch(OutActs<PAIRS...>, int out_dtype, int act, LAUNCH launch) {
  int rc = 1;
  (void)(... || ((((out_dtype == 0) == PAIRS::OUT16) && act == PAIRS::ACT) && ((rc = launch(PAIRS{})), true)));
  return rc;
}

// Fused epilogue of one wave, swapped orientation (MFMA tile rows = n, cols = m): the lane owns output row m(mi) and,
// per n-tile ni, the 4 consecutive columns n0(ni) .. n0(ni)+3.  Per-column vectors (bias, LayerScale) are loaded once
// for all NI tiles; per-row operands (residual, table) once per row, all NI at a time, so each optional operand costs
// one uniform branch and one wait per row instead of one per tile.
// RT16: the 16-bit output type is a run-time choice (p.f16: IEEE half instead of bf16) - the kernels of gemm.hip; the
// 256x256 kernel of the pi3 hot path instantiates RT16 = false and pays nothing for it.
template <bool OUT_BF16, int ACT, int NI, int MI, bool RT16 = false>
__device__ __forceinline__ void gemm_epilogue(const GemmParams& p, f32x4 (&acc)[NI][MI], int m_base, int n_base,
                                              int lane) {
  const int frow = lane & 15;
  const int nq = (lane >> 4) * 4;
  f32x4 bias4[NI], gamma4[NI];
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) {
    bias4[ni] = (f32x4){0.f, 0.f, 0.f, 0.f};
    gamma4[ni] = (f32x4){1.f, 1.f, 1.f, 1.f};
  }
  if (p.bias) {
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) bias4[ni] = *(const f32x4*)(p.bias + n_base + ni * 16 + nq);
  }
  if (p.gamma) {
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) gamma4[ni] = *(const f32x4*)(p.gamma + n_base + ni * 16 + nq);
  }
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    const int m = m_base + mi * 16 + frow;
    if (m >= p.M) continue;
    long orow = m;
    int trow = 0;
    if (p.rpg > 0) {
      const int gq = m / p.rpg;
      trow = m - gq * p.rpg;
      orow = (long)gq * p.gstride + p.goff + trow;
    }
    f32x4 extra[NI];
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) extra[ni] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (p.resid) {
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) extra[ni] = *(const f32x4*)(p.resid + orow * p.ldr + n_base + ni * 16 + nq);
    }
    if (p.addtab) {
#pragma unroll
      for (int ni = 0; ni < NI; ++ni)
        extra[ni] += *(const f32x4*)(p.addtab + (long)trow * p.ldadd + n_base + ni * 16 + nq);
    }
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      const int n0 = n_base + ni * 16 + nq;
      f32x4 v = acc[ni][mi] + bias4[ni];
      if (n0 < p.qcols) v *= p.qscale;
      if constexpr (ACT == 1) {
        v = gelu_erf4(v);
      } else if constexpr (ACT == 3) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = gelu_erf_as(v[r]);
      } else if constexpr (ACT == 2) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
      }
      v = v * gamma4[ni] + extra[ni];
      if constexpr (OUT_BF16) {
        u32x2 o;
        if (RT16 && p.f16) {
          o[0] = pack_f16x2(v[0], v[1]);
          o[1] = pack_f16x2(v[2], v[3]);
        } else {
          o[0] = pack_bf16x2(v[0], v[1]);
          o[1] = pack_bf16x2(v[2], v[3]);
        }
        *(u32x2*)((bf16_t*)p.out + orow * p.ldo + n0) = o;
      } else {
        *(f32x4*)((float*)p.out + orow * p.ldo + n0) = v;
      }
    }
  }
}
