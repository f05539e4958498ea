// C[M][N] = act(A[M][K] . W[N][K]^T + bias) with fused LayerScale / residual / table-add epilogues.
//
// This is the Linear layer of every transformer block on the path (reference: torch.nn.Linear inside
// pi3/models/layers/block.py:310-335, pi3/models/dinov2/layers/mlp.py:34-40, pi3/models/layers/attention.py:325,345,
// pi3/models/layers/transformer_head.py:49,55,74, pi3/models/layers/camera_head.py:26-31).  Weights stay in the
// PyTorch [out][in] layout, so both operands are K-contiguous and feed MFMA fragments straight from 128-byte LDS rows.
//
// gfx950 design: 128x128 output tile per 256-thread workgroup (4 waves, 2x2, 64x64 each = 4x4 MFMA 16x16 tiles),
// K-step = one 128-byte row per operand row (64 bf16 / 32 f32), double-buffered LDS filled by global_load_lds dwordx4
// (lane-linear LDS image; the bank swizzle goes on the SOURCE address and on the fragment read).  MFMA operands are
// swapped (A-operand = weight rows, B-operand = activation rows) so that each lane ends up with 4 consecutive output
// columns of one output row: 8/16-byte stores and float4 bias loads in the epilogue.
// The f32 variant uses v_mfma_f32_16x16x4_f32 (exact fp32, runs at the vector rate) for the heads the reference
// computes with autocast disabled (pi3/models/pi3.py:192-209).
//
// Host side: pi3_gemm, pi3_gemm_qkv and pi3_conv3x3 check their arguments, fill a GemmParams that starts from its
// defaults and map (out_dtype, act) to an instance with gemm_dispatch; launch_gemm / launch_narrow size the grid and go
// through gemm_launch (gemm_common.h).  Large bf16 problems are offered to pi3_gemm256_try (gemm256.hip) first.
#include "gemm_common.h"
#include <stdlib.h>

#define BM 128
#define BN 128
#define TILE_BYTES (128 * 128)

// Swizzled LDS image of every kernel here: a 1 KiB segment is 8 tile rows of 128 B, lane l fills the 16-byte slot l & 7 of
// row seg * 8 + (l >> 3), and chunk c of row r lives in slot c ^ ((r >> 1) & 7): the source chunk that lands in l's slot
__device__ __forceinline__ int swz_src_chunk(int row, int lane) { return (lane & 7) ^ ((row >> 1) & 7); }

// 3x3 convolution: tap 0..8 -> (ky, kx) in -1..1
__device__ __forceinline__ void conv_tap_offsets(int tap, int& ky, int& kx) {
  ky = tap / 3 - 1;
  kx = tap - (tap / 3) * 3 - 1;
}

// K-step t of the convolution with cC % 64 == 0 covers one tap and one 64-channel block starting at channel c0
__device__ __forceinline__ void conv_kstep(const GemmParams& p, int t, int& c0, int& ky, int& kx) {
  const int cblocks = p.cC >> 6;
  const int tap = t / cblocks;
  c0 = (t - tap * cblocks) << 6;
  conv_tap_offsets(tap, ky, kx);
}

// Source pixel of output pixel m = (b * cH + y) * cW + x under tap (ky, kx): the neighbour, clamped to its own image
__device__ __forceinline__ long conv_src_pixel(const GemmParams& p, int m, int ky, int kx) {
  const int x = m % p.cW;
  const int by = m / p.cW;  // b * cH + y
  const int y = by % p.cH;
  int yy = y + ky, xx = x + kx;
  yy = yy < 0 ? 0 : (yy >= p.cH ? p.cH - 1 : yy);
  xx = xx < 0 ? 0 : (xx >= p.cW ? p.cW - 1 : xx);
  return (long)(by - y + yy) * p.cW + xx;
}

// One 32-deep MFMA step over NI x 4 tiles: fw weight rows x fa activation rows; p.f16 (wave-uniform): as IEEE half
template <int NI>
__device__ __forceinline__ void mfma_step16(const GemmParams& p, const bf16x8 (&fw)[NI], const bf16x8 (&fa)[4],
                                            f32x4 (&acc)[NI][4]) {
  if (p.f16) {
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
        acc[ni][mi] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, fw[ni]),
                                                             __builtin_bit_cast(f16x8, fa[mi]), acc[ni][mi], 0, 0, 0);
  } else {
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
        acc[ni][mi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw[ni], fa[mi], acc[ni][mi], 0, 0, 0);
  }
}

template <int ESZ>
__device__ __forceinline__ void stage_tile(const char* gbase, long ld_bytes, int row0, int rows, long k0_bytes,
                                           char* lds_tile, int wave, int lane) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int seg = wave * 4 + i;           // 1 KiB segment = 8 rows of 128 B
    const int row = seg * 8 + (lane >> 3);  // tile row 0..127
    const int c = swz_src_chunk(row, lane);
    int grow = row0 + row;
    grow = grow < rows ? grow : rows - 1;   // clamp: tail rows re-read the last valid row, results are discarded
    const char* src = gbase + (long)grow * ld_bytes + k0_bytes + c * 16;
    __builtin_amdgcn_global_load_lds(GLB_PTR(src), LDS_PTR(lds_tile + seg * 1024), 16, 0, 0);
  }
}

// A-operand staging for the 3x3 convolution: the K-step t covers one tap and one 64-channel block; the source row of
// tile row r is the replicate-clamped neighbour pixel of pixel (row0 + r).
__device__ __forceinline__ void stage_tile_conv(const GemmParams& p, int row0, int t, char* lds_tile, int wave,
                                                int lane) {
  int c0, ky, kx;
  conv_kstep(p, t, c0, ky, kx);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int seg = wave * 4 + i;
    const int row = seg * 8 + (lane >> 3);
    const int c = swz_src_chunk(row, lane);
    int m = row0 + row;
    m = m < p.M ? m : p.M - 1;
    const long pix = conv_src_pixel(p, m, ky, kx);
    const char* src = (const char*)p.A + (pix * p.lda + c0) * 2 + c * 16;
    __builtin_amdgcn_global_load_lds(GLB_PTR(src), LDS_PTR(lds_tile + seg * 1024), 16, 0, 0);
  }
}

template <bool IS_BF16, bool OUT_BF16, int ACT, bool CONV = false>
__global__ __launch_bounds__(256) void gemm_tn_kernel(GemmParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wn = wave & 1, wm = wave >> 1;
  constexpr int ESZ = IS_BF16 ? 2 : 4;
  constexpr int BK = 128 / ESZ;

  const int nbm = (p.M + BM - 1) / BM, nbn = p.N / BN;
  const int nwg = nbm * nbn;
  int id = xcd_remap(blockIdx.x, nwg);
  // groups of 8 row panels sweep the weight tiles together: the group's A panels + the current W tiles stay in L2
  constexpr int GM = 8;
  const int per_group = GM * nbn;
  const int g = id / per_group;
  const int gm = min(GM, nbm - g * GM);
  const int rem = id - g * per_group;
  const int bm = g * GM + rem % gm;
  const int bn = rem / gm;

  const char* Ab = (const char*)p.A;
  const char* Wb = (const char*)p.W;
  const long lda_b = p.lda * ESZ, ldw_b = p.ldw * ESZ;
  const int nk = p.K / BK;

  // LDS ring: buffer b holds the A tile at b * 2 * TILE_BYTES and the W tile right after it
#define LDS_A(b) (smem + (b) * 2 * TILE_BYTES)
#define LDS_W(b) (smem + (b) * 2 * TILE_BYTES + TILE_BYTES)

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  if constexpr (CONV) stage_tile_conv(p, bm * BM, 0, LDS_A(0), wave, lane);
  else stage_tile<ESZ>(Ab, lda_b, bm * BM, p.M, 0, LDS_A(0), wave, lane);
  stage_tile<ESZ>(Wb, ldw_b, bn * BN, p.N, 0, LDS_W(0), wave, lane);
  __syncthreads();  // drains the LDS-DMA (vmcnt(0)) and publishes the tile

  const int frow = lane & 15;
  const int swz = (lane >> 1) & 7;  // == ((row >> 1) & 7) for row = 16*i + (lane & 15)
  const int cq = lane >> 4;

  int cur = 0;
  for (int t = 0; t < nk; ++t) {
    if (t + 1 < nk) {
      if constexpr (CONV) stage_tile_conv(p, bm * BM, t + 1, LDS_A(cur ^ 1), wave, lane);
      else stage_tile<ESZ>(Ab, lda_b, bm * BM, p.M, (long)(t + 1) * 128, LDS_A(cur ^ 1), wave, lane);
      stage_tile<ESZ>(Wb, ldw_b, bn * BN, p.N, (long)(t + 1) * 128, LDS_W(cur ^ 1), wave, lane);
    }
    const char* la = LDS_A(cur) + (wm * 64 + frow) * 128;
    const char* lw = LDS_W(cur) + (wn * 64 + frow) * 128;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int off = ((cq + 4 * kk) ^ swz) << 4;
      if constexpr (IS_BF16) {
        bf16x8 fa[4], fw[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          fa[i] = *(const bf16x8*)(la + i * 16 * 128 + off);
          fw[i] = *(const bf16x8*)(lw + i * 16 * 128 + off);
        }
        mfma_step16<4>(p, fw, fa, acc);
      } else {
        f32x4 fa[4], fw[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          fa[i] = *(const f32x4*)(la + i * 16 * 128 + off);
          fw[i] = *(const f32x4*)(lw + i * 16 * 128 + off);
        }
        // lane group q of k-step s supplies k = 4*chunk + s for BOTH operands: a consistent k permutation
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int ni = 0; ni < 4; ++ni)
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
              acc[ni][mi] = __builtin_amdgcn_mfma_f32_16x16x4f32(fw[ni][s], fa[mi][s], acc[ni][mi], 0, 0, 0);
      }
    }
    __syncthreads();
    cur ^= 1;
  }

  // ---- epilogue: lane holds rows n = nb + 4*(lane>>4) + r (r = 0..3) of column m = mb + (lane & 15)
  gemm_epilogue<OUT_BF16, ACT, 4, 4, true>(p, acc, bm * BM + wm * 64, bn * BN + wn * 64, lane);
}

template <bool IS_BF16, bool OUT_BF16, int ACT, bool CONV = false>
static int launch_gemm(const GemmParams& p, hipStream_t stream) {
  const int nbm = (p.M + BM - 1) / BM, nbn = p.N / BN;
  return gemm_launch<gemm_tn_kernel<IS_BF16, OUT_BF16, ACT, CONV>>("gemm_tn", nbm * nbn, 256, 4 * TILE_BYTES, p, stream);
}

// ---------------------------------------------------------------------------------------------------------------
// Narrow-N variant (round 3): 256 rows x (16 NT) columns per workgroup, NT = 2 or 4, the four waves stacked along M (64
// rows each, all of them reading the whole W tile).  For the MoGe conv pyramid, whose finest levels are 32-channel maps
// of ~900 k pixels: padded to the 128-column tile of the kernel above they did 4x the MFMA work and, worse, wrote 4x
// the bytes (a 32-channel fp32 map as 128-float rows).  Same LDS image, swizzle and fragment reads as above.
// CONV with cC == 32: a 128-byte LDS row holds the 32 channels of TWO taps (K-step t = taps 2t and 2t + 1, k = tap * 32
// + ci; the weight rows carry zeros for the tenth tap, which is staged from tap 8 so that it is finite data): 5 K-steps
// instead of 9 half-empty ones.
// ---------------------------------------------------------------------------------------------------------------
#define NBM 256

template <int NT, bool CONV>
__device__ __forceinline__ void stage_narrow(const GemmParams& p, int row0, int n0, int t, char* lds_a, char* lds_w,
                                             int wave, int lane) {
  // ---- A: segments 8 wave .. 8 wave + 7 (8 rows of 128 B each)
  int c0 = 0, ky = 0, kx = 0;
  const bool half = CONV && p.cC == 32;
  if (CONV && !half) conv_kstep(p, t, c0, ky, kx);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int seg = wave * 8 + i;
    const int row = seg * 8 + (lane >> 3);
    const int c = swz_src_chunk(row, lane);
    int m = row0 + row;
    m = m < p.M ? m : p.M - 1;
    const char* src;
    if constexpr (CONV) {
      int cc = c;
      if (half) {      // chunks 0..3: the 32 channels of tap 2t, chunks 4..7: of tap 2t + 1
        conv_tap_offsets(min(2 * t + (c >> 2), 8), ky, kx);
        cc = c & 3;
      }
      const long pix = conv_src_pixel(p, m, ky, kx);
      src = (const char*)p.A + (pix * p.lda + c0) * 2 + cc * 16;
    } else {
      src = (const char*)p.A + ((long)m * p.lda + (long)t * 64) * 2 + c * 16;
    }
    __builtin_amdgcn_global_load_lds(GLB_PTR(src), LDS_PTR(lds_a + seg * 1024), 16, 0, 0);
  }
  // ---- W: 2 NT segments, wave w takes w (and w + 4)
#pragma unroll
  for (int i = 0; i < NT / 2; ++i) {
    const int seg = wave + 4 * i;
    if (seg < 2 * NT) {
      const int row = seg * 8 + (lane >> 3);
      const int c = swz_src_chunk(row, lane);
      const char* src = (const char*)p.W + ((long)(n0 + row) * p.ldw + (long)t * 64) * 2 + c * 16;
      __builtin_amdgcn_global_load_lds(GLB_PTR(src), LDS_PTR(lds_w + seg * 1024), 16, 0, 0);
    }
  }
}

template <int NT, bool OUT_BF16, int ACT, bool CONV>
__global__ __launch_bounds__(256) void gemm_narrow_kernel(GemmParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int A_BYTES = NBM * 128, STAGE = A_BYTES + 16 * NT * 128;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nbm = (p.M + NBM - 1) / NBM, nbn = p.N / (16 * NT);
  const int id = xcd_remap(blockIdx.x, nbm * nbn);
  const int bm = id / nbn, bn = id - bm * nbn;      // the (few) column tiles of a row panel run back to back
  const int nk = p.K / 64;

  f32x4 acc[NT][4];
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  stage_narrow<NT, CONV>(p, bm * NBM, bn * 16 * NT, 0, smem, smem + A_BYTES, wave, lane);
  __syncthreads();
  const int frow = lane & 15, swz = (lane >> 1) & 7, cq = lane >> 4;
  int cur = 0;
  for (int t = 0; t < nk; ++t) {
    if (t + 1 < nk)
      stage_narrow<NT, CONV>(p, bm * NBM, bn * 16 * NT, t + 1, smem + (cur ^ 1) * STAGE, smem + (cur ^ 1) * STAGE + A_BYTES,
                             wave, lane);
    const char* la = smem + cur * STAGE + (wave * 64 + frow) * 128;
    const char* lw = smem + cur * STAGE + A_BYTES + frow * 128;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int off = ((cq + 4 * kk) ^ swz) << 4;
      bf16x8 fa[4], fw[NT];
#pragma unroll
      for (int i = 0; i < 4; ++i) fa[i] = *(const bf16x8*)(la + i * 16 * 128 + off);
#pragma unroll
      for (int i = 0; i < NT; ++i) fw[i] = *(const bf16x8*)(lw + i * 16 * 128 + off);
      mfma_step16<NT>(p, fw, fa, acc);
    }
    __syncthreads();
    cur ^= 1;
  }
  gemm_epilogue<OUT_BF16, ACT, NT, 4, true>(p, acc, bm * NBM + wave * 64, bn * 16 * NT, lane);
}

template <bool OUT_BF16, int ACT, bool CONV>
static int launch_narrow(const GemmParams& p, hipStream_t stream) {
  const int nbm = (p.M + NBM - 1) / NBM;
  if (p.N % 64 == 0)
    return gemm_launch<gemm_narrow_kernel<4, OUT_BF16, ACT, CONV>>("gemm_narrow", nbm * (p.N / 64), 256,
                                                                   2 * (NBM * 128 + 64 * 128), p, stream);
  return gemm_launch<gemm_narrow_kernel<2, OUT_BF16, ACT, CONV>>("gemm_narrow", nbm * (p.N / 32), 256,
                                                                 2 * (NBM * 128 + 32 * 128), p, stream);
}

// ---- entry points.  The (out_dtype, act) pairs each kernel family instantiates (gemm_dispatch, gemm_common.h):
using Linear16Pairs = OutActs<OutAct<true, 0>, OutAct<true, 1>, OutAct<false, 0>, OutAct<false, 2>>;   // 16-bit operands
using LinearF32Pairs = OutActs<OutAct<false, 0>, OutAct<false, 2>, OutAct<true, 0>>;                   // fp32 operands
using ConvPairs = OutActs<OutAct<true, 0>, OutAct<false, 0>, OutAct<true, 2>>;                         // pi3_conv3x3

int pi3_gemm256_try(GemmParams p, int out_dtype, int act, hipStream_t stream);

// dtype code 2 = IEEE half: the bf16 code paths with the f16 MFMA / conversion selected at run time (GemmParams.f16).
// Folds the codes to 0 and returns the flag; a 16-bit output has the operands' format (one flag).
static int fold_half(int& in_dtype, int& out_dtype) {
  const int f16 = (in_dtype == 2 || out_dtype == 2) ? 1 : 0;
  if (in_dtype == 2) in_dtype = 0;
  if (out_dtype == 2) out_dtype = 0;
  return f16;
}

// the LDS-DMA moves 16 bytes per lane and the epilogues store 8 / 16 bytes per lane (esz: bytes per operand element)
static int check_aligned(const char* who, const void* A, long lda, const void* W, long ldw, int esz, const void* out,
                         long ldo) {
  if ((lda * esz) % 16 || (ldw * esz) % 16 || ((uintptr_t)A & 15) || ((uintptr_t)W & 15) || ((uintptr_t)out & 15) ||
      (ldo % 4)) {
    pi3_set_error("%s: operands must be 16-byte aligned with 16-byte-multiple row strides", who);
    return PI3_ERR_ARG;
  }
  return PI3_OK;
}

// in_dtype: 0 = bf16 operands, 1 = f32 operands.  out_dtype: 0 = bf16, 1 = f32.  act: 0 none, 1 GELU(erf), 2 ReLU.
extern "C" int pi3_gemm(const void* A, long lda, const void* W, long ldw, int M, int N, int K, int in_dtype,
                        const float* bias, const float* gamma, const float* resid, long ldr, void* out, long ldo,
                        int out_dtype, int act, int rpg, int gstride, int goff, const float* addtab, long ldadd,
                        float qscale, int qcols, void* stream) {
  // in_dtype 2 = IEEE-half operands, out_dtype 2 = IEEE-half output; half operands give a half or f32 output, never bf16
  if (in_dtype < 0 || in_dtype > 2 || out_dtype < 0 || out_dtype > 2 || (in_dtype == 2 && out_dtype == 0) ||
      (out_dtype == 2 && in_dtype != 2)) {
    pi3_set_error("pi3_gemm: unsupported dtypes in=%d out=%d (0 bf16, 1 f32, 2 f16; f16 operands give f16 or f32 output, "
                  "bf16 operands bf16 or f32)", in_dtype, out_dtype);
    return PI3_ERR_ARG;
  }
  const int f16 = fold_half(in_dtype, out_dtype);
  const int bk = in_dtype == 0 ? 64 : 32;
  const bool narrow = in_dtype == 0 && (N % BN) != 0 && (N % 32) == 0;     // bf16 operands, N = 32, 64, 96, 160, ...
  if (!A || !W || !out || M <= 0 || N <= 0 || K <= 0 || ((N % BN) != 0 && !narrow) || (K % bk) != 0 || act < 0 || act > 2) {
    pi3_set_error("pi3_gemm: bad arguments M=%d N=%d K=%d (N %% 128 == 0, or N %% 32 == 0 with bf16 operands; K %% %d == 0 required)",
                  M, N, K, bk);
    return PI3_ERR_ARG;
  }
  if (int rc = check_aligned("pi3_gemm", A, lda, W, ldw, in_dtype == 0 ? 2 : 4, out, ldo)) return rc;
  // the epilogues decide n < qcols once per group of 4 columns (one lane's f32x4): a boundary inside a group would
  // scale the whole group
  if (qcols < 0 || qcols > N || (qcols % 4) != 0) {
    pi3_set_error("pi3_gemm: qcols=%d must be a multiple of 4 in [0, N=%d]", qcols, N);
    return PI3_ERR_ARG;
  }
  GemmParams p{};
  p.A = A; p.lda = lda; p.W = W; p.ldw = ldw; p.M = M; p.N = N; p.K = K;
  p.bias = bias; p.gamma = gamma; p.resid = resid; p.ldr = ldr; p.out = out; p.ldo = ldo;
  p.rpg = rpg; p.gstride = gstride; p.goff = goff; p.addtab = addtab; p.ldadd = ldadd;
  p.qscale = qscale; p.qcols = qcols; p.f16 = f16;
  hipStream_t s = (hipStream_t)stream;
  if (narrow) {
    const int rc = gemm_dispatch(Linear16Pairs{}, out_dtype, act,
                                 [&](auto oa) { return launch_narrow<oa.OUT16, oa.ACT, false>(p, s); });
    if (rc == 1) {
      pi3_set_error("pi3_gemm: unsupported (out_dtype=%d, act=%d) for a narrow N", out_dtype, act);
      return PI3_ERR_ARG;
    }
    return rc;
  }
  int rc = 1;   // 1 = not served yet
  // large bf16 GEMMs: 256x256 pipelined kernel (development switch PI3_GEMM_IMPL=1, common.h, forces the 128x128 kernel)
  if (in_dtype == 0 && !f16 && PI3_DEV_ENV_INT("PI3_GEMM_IMPL", 0) != 1) rc = pi3_gemm256_try(p, out_dtype, act, s);
  if (rc == 1 && in_dtype == 0)
    rc = gemm_dispatch(Linear16Pairs{}, out_dtype, act, [&](auto oa) { return launch_gemm<true, oa.OUT16, oa.ACT>(p, s); });
  if (rc == 1 && in_dtype == 1)
    rc = gemm_dispatch(LinearF32Pairs{}, out_dtype, act, [&](auto oa) { return launch_gemm<false, oa.OUT16, oa.ACT>(p, s); });
  if (rc == 1) {
    pi3_set_error("pi3_gemm: unsupported (in_dtype=%d,out_dtype=%d,act=%d) combination", in_dtype, out_dtype, act);
    return PI3_ERR_ARG;
  }
  return rc;
}

// The packed qkv projection of a transformer block with what follows it on q and k fused into the epilogue
// (FlashAttentionRope.forward, pi3/models/layers/attention.py:323-334; BlockRope, layers/block.py:310-335):
//   qkv = x W^T + b  (bf16) ;  q, k <- LayerNorm_64(q), LayerNorm_64(k) per head (if qw) ;  q, k <- RoPE2D(q, k, pos)
//   (if pos) ;  q <- q * qscale ;  k2max[(row / attnS) * H + head] = max |k|^2 (if k2max: consumed by pi3_attention).
// Large problems run the 256x256 kernel with the fused epilogue (no second pass over the 395 MB qkv buffer); others
// run the plain GEMM followed by the stand-alone pi3_qknorm_rope pass (+ the key-norm pre-pass): same results up to
// fp32 summation order inside the LayerNorm statistic.
int pi3_qknorm_rope_launch(void* qkv, long rows, int H, int T, const int* pos, const float* cs, const float* qw,
                           const float* qb, const float* kw, const float* kb, float eps, float qscale, int do_rope,
                           hipStream_t stream);
int pi3_attention_knorm_launch(const void* k, long tok_stride, long batch_stride, int B, int S, int H, float* out,
                               hipStream_t stream);

extern "C" int pi3_gemm_qkv(const void* A, long lda, const void* W, long ldw, int M, int K, int H, const float* bias,
                            void* qkv, long ldo, int T, const int* pos, const float* cs, const float* qw,
                            const float* qb, const float* kw, const float* kb, float eps, float qscale,
                            float* k2max, int attn_B, int attn_S, void* stream) {
  const int N = 3 * H * 64;
  if (!A || !W || !qkv || M <= 0 || K <= 0 || H <= 0 || T <= 0 || (K % 64) || (N % BN) || ldo != N ||
      ((qw != nullptr) != (kw != nullptr)) || ((qw != nullptr) != (qb != nullptr)) || ((kw != nullptr) != (kb != nullptr)) ||
      ((pos != nullptr) != (cs != nullptr)) || (k2max && (attn_B <= 0 || attn_S <= 0 || (long)attn_B * attn_S != M))) {
    pi3_set_error("pi3_gemm_qkv: bad arguments M=%d K=%d H=%d T=%d (packed [M][3*H*64] output, K %% 64 == 0)", M, K, H, T);
    return PI3_ERR_ARG;
  }
  if (int rc = check_aligned("pi3_gemm_qkv", A, lda, W, ldw, 2, qkv, ldo)) return rc;   // (ldo == N: a multiple of 128)
  hipStream_t s = (hipStream_t)stream;
  if (k2max && hipMemsetAsync(k2max, 0, (size_t)attn_B * H * sizeof(float), s) != hipSuccess) {
    pi3_set_error("pi3_gemm_qkv: hipMemsetAsync failed");
    return PI3_ERR_LAUNCH;
  }
  GemmParams p{};          // the plain projection
  p.A = A; p.lda = lda; p.W = W; p.ldw = ldw; p.M = M; p.N = N; p.K = K; p.bias = bias; p.out = qkv; p.ldo = ldo;
  if (!qw && !pos) {       // no LayerNorm, no RoPE (encoder blocks): the q scale rides in the plain epilogue, as in pi3_gemm
    p.qscale = qscale;
    p.qcols = H * 64;
  }
  if (PI3_DEV_ENV_INT("PI3_QKV_FUSE", 1)) {    // development switch: 0 = always the two-pass form (both forms are correct)
    GemmParams f = p;      // the same projection with the fused q/k epilogue
    f.qk_mode = 1; f.qk_H = H; f.qk_T = T; f.qk_pos = pos; f.qk_cs = cs;
    f.qk_qw = qw; f.qk_qb = qb; f.qk_kw = kw; f.qk_kb = kb; f.qk_eps = eps; f.qk_qscale = qscale;
    f.qk_k2max = k2max; f.qk_attnS = attn_S > 0 ? attn_S : M;
    const int rc = pi3_gemm256_try(f, 0, 0, s);
    if (rc <= 0) return rc;
  }
  // two-pass form: plain projection, then the in-place q/k pass, then the key-norm pre-pass
  int rc = pi3_gemm256_try(p, 0, 0, s);
  if (rc > 0) rc = launch_gemm<true, true, 0>(p, s);
  if (rc != 0) return rc;
  if (qw || pos) {     // (without LayerNorm and RoPE the projection above has already folded the scale into q)
    rc = pi3_qknorm_rope_launch(qkv, M, H, T, pos, cs, qw, qb, kw, kb, eps, qscale, pos != nullptr, s);
    if (rc != 0) return rc;
  }
  if (k2max)
    return pi3_attention_knorm_launch((const char*)qkv + (size_t)H * 64 * 2, ldo, (long)attn_S * ldo, attn_B, attn_S, H,
                                      k2max, s);
  return PI3_OK;
}

// 3x3 convolution, stride 1, replicate padding, as an implicit GEMM on an NHWC bf16 image (nn.Conv2d(..., 3, padding=1,
// padding_mode='replicate') in moge/model/modules.py:47-60,146-164).  img: bf16 [B][H][W][ldc] with C % 64 == 0 used
// channels; wgt: bf16 [N][9*C], k = (ky*3 + kx)*C + ci; out rows = pixels.  Epilogue as pi3_gemm (bias, resid, act).
extern "C" int pi3_conv3x3(const void* img, long ldc, int B, int H, int W, int C, const void* wgt, int N,
                           const float* bias, const float* resid, long ldr, void* out, long ldo, int in_dtype,
                           int out_dtype, int act, void* stream) {
  // in_dtype: 0 = bf16 image and weights, 2 = IEEE half; out_dtype: 1 = f32, else the image's 16-bit type
  if ((in_dtype != 0 && in_dtype != 2) || (out_dtype != 1 && out_dtype != in_dtype)) {
    pi3_set_error("pi3_conv3x3: unsupported dtypes in=%d out=%d (in: 0 bf16 / 2 f16; out: 1 f32 or the input type)", in_dtype,
                  out_dtype);
    return PI3_ERR_ARG;
  }
  const int f16 = fold_half(in_dtype, out_dtype);
  const bool narrow = (N % BN) != 0 || C == 32;
  if (!img || !wgt || !out || B <= 0 || H <= 0 || W <= 0 || C <= 0 || ((C % 64) && C != 32) || N <= 0 || (N % 32) ||
      (ldc % 8) || ((uintptr_t)img & 15) || ((uintptr_t)wgt & 15) || ((uintptr_t)out & 15) || (ldo % 4) || act < 0 ||
      act > 2 || (long)B * H * W > 0x7fffffffL) {
    pi3_set_error("pi3_conv3x3: bad arguments B=%d H=%d W=%d C=%d N=%d (C %% 64 == 0 or C == 32, N %% 32 == 0)", B, H, W, C, N);
    return PI3_ERR_ARG;
  }
  GemmParams p{};
  // C == 32: weight rows are [10 taps][32] (the tenth tap zero), two taps per K-step
  const long kw = C == 32 ? 320 : 9L * C;
  p.A = img; p.lda = ldc; p.W = wgt; p.ldw = kw; p.M = B * H * W; p.N = N; p.K = (int)kw;
  p.bias = bias; p.resid = resid; p.ldr = ldr; p.out = out; p.ldo = ldo;
  p.cH = H; p.cW = W; p.cC = C; p.f16 = f16;
  hipStream_t s = (hipStream_t)stream;
  const int rc = narrow ? gemm_dispatch(ConvPairs{}, out_dtype, act,
                                        [&](auto oa) { return launch_narrow<oa.OUT16, oa.ACT, true>(p, s); })
                        : gemm_dispatch(ConvPairs{}, out_dtype, act,
                                        [&](auto oa) { return launch_gemm<true, oa.OUT16, oa.ACT, true>(p, s); });
  if (rc == 1) {
    pi3_set_error("pi3_conv3x3: unsupported (out_dtype=%d, act=%d)", out_dtype, act);
    return PI3_ERR_ARG;
  }
  return rc;
}
