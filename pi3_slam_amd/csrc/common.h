// Shared device helpers for the gfx950 (MI355X / CDNA4) kernels of the Pi3-SLAM hot path.
// Wave width is 64 everywhere; nothing in here is portable to 32-wide hardware and nothing tries to be.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef __bf16 bf16_t;
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

#define LDS_PTR(p) ((__attribute__((address_space(3))) void*)(p))
#define GLB_PTR(p) ((const __attribute__((address_space(1))) void*)(p))

// error codes returned through the C-ABI (include/pi3slam_hip.h)
enum {
  PI3_OK = 0,
  PI3_ERR_ARG = -1,      // bad shape / null pointer / unsupported size
  PI3_ERR_LAUNCH = -2,   // hipLaunch / runtime error (see pi3_last_error)
  PI3_ERR_WORKSPACE = -3 // caller workspace too small
};

void pi3_set_error(const char* fmt, ...);
int pi3_check_launch(const char* what);
// An entry point zeroes its own counters: n 64-bit words at ptr, on the stream.  PI3_OK, or PI3_ERR_LAUNCH with
// "<who>: hipMemsetAsync failed" in pi3_last_error().
int pi3_zero_words(const char* who, void* ptr, long n, void* stream);
// the argument test of a scale, a size or a tolerance: finite and > 0 (false for NaN)
inline bool positive_finite(double v) { return v > 0.0 && __builtin_isfinite(v); }
// Opt `kern` into `bytes` of dynamic LDS (above the 64 KB default) on the CURRENT device, once per device: the attribute
// is per device, so `done_mask` (one function-local static per kernel instance) carries one bit per device ordinal.
// Returns PI3_OK or PI3_ERR_LAUNCH with the runtime's message in pi3_last_error().
// run-time A/B knob (api.hip): pi3_set_knob value, else env PI3_<NAME>, else dflt.  Slots live in a static table, so a
// launch path resolves the name once (PI3_KNOB: a function-local static pointer) and then reads two words per launch.
struct Pi3Knob { char name[32]; long value; int state; };   // state 0 free, 1 unset, 2 has a value (release / acquire)
const Pi3Knob* pi3_knob_slot(const char* name);
long pi3_knob(const char* name, long dflt);
#define PI3_KNOB(NAME, DFLT)                                                     \
  ([]() -> long {                                                                \
    static const Pi3Knob* k_ = pi3_knob_slot(NAME);                              \
    return (k_ && __atomic_load_n(&k_->state, __ATOMIC_ACQUIRE) == 2)            \
               ? __atomic_load_n(&k_->value, __ATOMIC_RELAXED) : (long)(DFLT);   \
  }())
int pi3_lds_optin(const void* kern, int bytes, unsigned long long* done_mask, const char* what);

// Development variants.  The product library (make) carries ONE form of every kernel plus the run-time knobs listed in
// api.hip (pi3_set_knob refuses any other name).  Forms that were measured equal or slower - kept because their
// bit-identity against the shipped form is a race screen and a record of the experiment - compile only with
// -DPI3_DEV_VARIANTS (make dev -> libpi3slam_hip_dev.so), where the environment switches below are live.  In the
// product build PI3_DEV_ENV_INT is its default, a compile-time constant.
#ifdef PI3_DEV_VARIANTS
#include <stdlib.h>
#define PI3_DEV_ENV_INT(NAME, DFLT)            \
  ([]() -> int {                               \
    static int v_ = -0x7fffffff;               \
    if (v_ == -0x7fffffff) {                   \
      const char* e_ = getenv(NAME);           \
      v_ = e_ ? atoi(e_) : (int)(DFLT);        \
    }                                          \
    return v_;                                 \
  }())
#define PI3_DEV_KNOB(NAME, DFLT) PI3_KNOB(NAME, DFLT)
#else
#define PI3_DEV_ENV_INT(NAME, DFLT) ((int)(DFLT))
#define PI3_DEV_KNOB(NAME, DFLT) ((long)(DFLT))
#endif

// doubles per camera record of the map renderer (layout: render.hip; also read by render_shade in voxel_normals.hip)
constexpr int kCamDoubles = 20;

__device__ __forceinline__ float bf16_bits_to_f32(uint16_t b) {
  return __uint_as_float(((uint32_t)b) << 16);
}

// fp32 -> bf16 round-to-nearest-even through the compiler's cast (v_cvt_pk_bf16_f32 on gfx950; keeps NaN a NaN).
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
  bf16x2 v;
  v[0] = (bf16_t)lo;
  v[1] = (bf16_t)hi;
  return __builtin_bit_cast(uint32_t, v);
}

// fp32 -> IEEE half, round-to-nearest-even (v_cvt_pk_f16_f32 on gfx950); overflow -> inf like torch's .half()
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ uint32_t pack_f16x2(float lo, float hi) {
  f16x2 v;
  v[0] = (_Float16)lo;
  v[1] = (_Float16)hi;
  return __builtin_bit_cast(uint32_t, v);
}

// the 16-bit storage format as a run-time (wave-uniform) choice: the HBM-bound staging kernels of the MoGe path write
// bf16 or IEEE half with one code path
__device__ __forceinline__ uint32_t pack16x2(float lo, float hi, int f16) {
  return f16 ? pack_f16x2(lo, hi) : pack_bf16x2(lo, hi);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Bijective XCD-aware remap (8 XCDs, blocks dealt round-robin): consecutive logical ids land on one XCD so
// neighbouring tiles share that XCD's L2. Speed only; correctness never depends on placement.
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7;
  const int xcd = bid & 7, idx = bid >> 3;
  const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + idx;
}

// GELU(erf) = 0.5 x (1 + erf(x / sqrt 2)) = x Phi(x) (nn.GELU default, pi3/models/dinov2/layers/mlp.py:36).
//
// Round-4 form: with q = Phi(-|x|) the function is  relu(x) - |x| q  on both sides of zero, and log2 q is smooth, so
//   q = exp2(P8(|x|)),   P8 = degree-8 minimax fit of log2 Phi(-t) on [0, 5]  (max error 1.85e-6 in log2, i.e. 1.3e-6
//   RELATIVE in q: no 1 + erf cancellation in the negative tail, where fp32 erf formulas lose all digits)
// 8 FMAs + one v_exp_f32 + max + fma: no v_rcp, and the FMAs pack (v_pk_fma_f32) - 9.5 issue slots per element where
// the Abramowitz-Stegun form below takes 14.5; the fc1 epilogue runs with the matrix pipe idle, so VALU issue is its
// critical path.  Beyond t = 5 the polynomial keeps falling (leading coefficient < 0; checked to t = 40,
// then -inf), so q -> 0 and y -> relu(x) with no clamp; NaN in -> NaN out; |x| is clamped to 40 inside the product
// |x| q only (q = 0 there already), so that +-inf - an overflowed fc1 accumulator - gives relu(x) = +inf / 0 like the erf
// form and torch instead of inf * 0 = NaN (one v_pk_min_f32 per pair).
// Accuracy (tools/dev_gelu.py, 1e7 samples, bf16(y) against bf16 of the fp64 truth x Phi(x)): 9.6e-5 of N(0, 1) samples
// differ (torch's own fp32 gelu: 9.3e-5 - the floor set by fp32 rounding), 1.1e-3 of N(0, 2) samples (torch fp32: 1.8e-2,
// the A-S form: 1.4e-2); against bf16(torch fp32 gelu) on N(0, 1): 1.8e-4 (A-S form 1.3e-4), i.e. 99.98 % identical.
// Two elements at a time: written on <2 x float> so that the eight Horner steps and the final step are v_pk_fma_f32
// (hipcc's SLP pass packs the Abramowitz-Stegun form's independent multiplies by itself but leaves a chain of fmaf()
// calls scalar: 1 024 v_fma_f32 per tile instead of 512 v_pk_fma_f32).
__device__ __forceinline__ f32x2 gelu_erf2(f32x2 x) {
  const f32x2 t = __builtin_elementwise_abs(x);
  f32x2 p = (f32x2)(-2.927687888e-07f);
  p = __builtin_elementwise_fma(p, t, (f32x2)(4.067300779e-06f));
  p = __builtin_elementwise_fma(p, t, (f32x2)(1.347436773e-05f));
  p = __builtin_elementwise_fma(p, t, (f32x2)(-7.274326053e-04f));
  p = __builtin_elementwise_fma(p, t, (f32x2)(8.036931977e-03f));
  p = __builtin_elementwise_fma(p, t, (f32x2)(-5.337347835e-02f));
  p = __builtin_elementwise_fma(p, t, (f32x2)(-4.588178992e-01f));
  p = __builtin_elementwise_fma(p, t, (f32x2)(-1.151171446e+00f));
  p = __builtin_elementwise_fma(p, t, (f32x2)(-9.999981523e-01f));
  f32x2 q, r;
  q[0] = __builtin_amdgcn_exp2f(p[0]);
  q[1] = __builtin_amdgcn_exp2f(p[1]);
  r[0] = fmaxf(x[0], 0.0f);
  r[1] = fmaxf(x[1], 0.0f);
  const f32x2 tc = __builtin_elementwise_min(t, (f32x2)(40.0f));   // inf * 0 guard; the Horner chain keeps the true |x|
  return __builtin_elementwise_fma(tc, -q, r);       // the negation folds into the instruction's neg modifiers
}
__device__ __forceinline__ f32x4 gelu_erf4(f32x4 v) {
  const f32x2 a = gelu_erf2((f32x2){v[0], v[1]}), b = gelu_erf2((f32x2){v[2], v[3]});
  return (f32x4){a[0], a[1], b[0], b[1]};
}
__device__ __forceinline__ float gelu_erf(float x) {
  const float t = fabsf(x);
  float p = -2.927687888e-07f;
  p = fmaf(p, t, 4.067300779e-06f);
  p = fmaf(p, t, 1.347436773e-05f);
  p = fmaf(p, t, -7.274326053e-04f);
  p = fmaf(p, t, 8.036931977e-03f);
  p = fmaf(p, t, -5.337347835e-02f);
  p = fmaf(p, t, -4.588178992e-01f);
  p = fmaf(p, t, -1.151171446e+00f);
  p = fmaf(p, t, -9.999981523e-01f);
  const float q = __builtin_amdgcn_exp2f(p);
  return fmaf(-fminf(t, 40.0f), q, fmaxf(x, 0.0f));
}

// The round 1-3 form (Abramowitz-Stegun 7.1.26, |abs error of erf| <= 1.5e-7; one v_rcp, one v_exp and 11 regular vector
// operations): kept as the A/B partner of the form above (knob gelu_form = 1 in gemm256.hip; both are correct GELUs).
__device__ __forceinline__ float gelu_erf_as(float x) {
  const float ax = fabsf(x);
  const float t = __builtin_amdgcn_rcpf(fmaf(ax, 0.3275911f * 0.70710678118654752440f, 1.0f));
  const float poly = t * (0.254829592f + t * (-0.284496736f + t * (1.421413741f + t * (-1.453152027f + t * 1.061405429f))));
  const float z = ax * 0.84932180028801904272f;          // sqrt(log2(e) / 2): exp(-x^2 / 2) = exp2(-z^2)
  const float e = __builtin_amdgcn_exp2f(-z * z);
  const float hx = 0.5f * x;
  return fmaf(fabsf(hx), 1.0f - poly * e, hx);
}
