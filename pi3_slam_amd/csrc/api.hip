// C-ABI plumbing shared by every entry point: error string, launch checking, version.
// The boundary is declared in include/pi3slam_hip.h; nothing here depends on torch.
#include "common.h"
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static thread_local char g_err[512] = "";

void pi3_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int pi3_check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    pi3_set_error("%s: %s", what, hipGetErrorString(e));
    return PI3_ERR_LAUNCH;
  }
  return PI3_OK;
}

int pi3_zero_words(const char* who, void* ptr, long n, void* stream) {
  if (hipMemsetAsync(ptr, 0, (size_t)n * sizeof(unsigned long long), (hipStream_t)stream) == hipSuccess) return PI3_OK;
  pi3_set_error("%s: hipMemsetAsync failed", who);
  return PI3_ERR_LAUNCH;
}

int pi3_lds_optin(const void* kern, int bytes, unsigned long long* done_mask, const char* what) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) dev = 0;
  const unsigned long long bit = 1ull << (dev & 63);
  if (__atomic_load_n(done_mask, __ATOMIC_RELAXED) & bit) return PI3_OK;
  hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    pi3_set_error("%s: hipFuncSetAttribute(MaxDynamicSharedMemorySize = %d) on device %d: %s", what, bytes, dev,
                  hipGetErrorString(e));
    return PI3_ERR_LAUNCH;
  }
  __atomic_fetch_or(done_mask, bit, __ATOMIC_RELAXED);
  return PI3_OK;
}

// Run-time A/B knobs (all of them select CORRECT variants; speed only).  A knob's value is what pi3_set_knob() last
// stored, else the environment variable PI3_<NAME IN UPPER CASE> read once, else the caller's default.  The tools under
// tools/ use pi3_set_knob to interleave variants inside one process (perf deltas of a few per cent are only resolvable
// that way: the cards of the pool differ by +-4 %).
// The names a build knows are listed here; pi3_set_knob refuses any other (a knob of a development variant set on the
// product library would otherwise be accepted and silently do nothing):
//   attn_asm       0 = compiler-scheduled 512-row attention kernel, 2 (default) = hand-placed loop (attn_fwd64b_kernel)
//   attn_nomax     0 = online-max softmax loop everywhere, 1 = a-priori bound on max|k|^2, 2 (default) = optimistic form
//   gelu_form      1 = sigmoid form of the tanh approximation in the fc1 epilogue (default 0: erf)
//   ba_schur_rows  1 = the round-3 row kernel for the Schur complement (default 0: f64-MFMA tiles)
extern "C" const char* pi3_build_flavor(void);
static const char* const kKnobNames[] = {"attn_asm", "attn_nomax", "gelu_form", "ba_schur_rows",
#ifdef PI3_DEV_VARIANTS
                                         "attn_frame_nw", "gemm_4w", "gemm_ilv", "gemm_rpref", "gemm_stagger_ns", "gemm_mfma32",
#endif
#ifdef PI3_DEV_ABLATIONS
                                         "gemm_abl",
#endif
};
static bool knob_known(const char* name) {
  for (const char* k : kKnobNames)
    if (strcmp(k, name) == 0) return true;
  return false;
}
namespace {
typedef Pi3Knob Knob;
Knob g_knobs[64];
int g_knob_lock = 0;
struct KnobGuard {
  KnobGuard() { while (__atomic_exchange_n(&g_knob_lock, 1, __ATOMIC_ACQUIRE)) {} }
  ~KnobGuard() { __atomic_store_n(&g_knob_lock, 0, __ATOMIC_RELEASE); }
};
Knob* knob_slot(const char* name) {
  for (auto& k : g_knobs) {
    if (k.state && strncmp(k.name, name, sizeof(k.name)) == 0) return &k;
    if (!k.state) {
      strncpy(k.name, name, sizeof(k.name) - 1);
      char env[48] = "PI3_";
      size_t i = 4;
      for (const char* c = name; *c && i + 1 < sizeof(env); ++c, ++i) env[i] = (*c >= 'a' && *c <= 'z') ? *c - 32 : *c;
      env[i] = 0;
      const char* e = getenv(env);
      k.value = e ? atol(e) : 0;         // value, then state with release order: a lock-free reader (PI3_KNOB)
      __atomic_store_n(&k.state, e ? 2 : 1, __ATOMIC_RELEASE);   // acquires the state before it reads the value
      return &k;
    }
  }
  return nullptr;
}
}  // namespace

const Pi3Knob* pi3_knob_slot(const char* name) {
  KnobGuard g;
  return knob_slot(name);
}

long pi3_knob(const char* name, long dflt) {
  KnobGuard g;
  Knob* k = knob_slot(name);
  return (k && k->state == 2) ? k->value : dflt;
}

extern "C" int pi3_set_knob(const char* name, long value) {
  if (!name || !*name || strlen(name) >= sizeof(((Knob*)nullptr)->name)) {
    pi3_set_error("pi3_set_knob: bad knob name");
    return PI3_ERR_ARG;
  }
  if (!knob_known(name)) {
    pi3_set_error("pi3_set_knob: '%s' is not a knob of this build (%s library; development variants live in "
                  "libpi3slam_hip_dev.so, make dev)", name, pi3_build_flavor());
    return PI3_ERR_ARG;
  }
  KnobGuard g;
  Knob* k = knob_slot(name);
  if (!k) {
    pi3_set_error("pi3_set_knob: knob table full");
    return PI3_ERR_ARG;
  }
  k->value = value;
  __atomic_store_n(&k->state, 2, __ATOMIC_RELEASE);
  return PI3_OK;
}

// -> 1 and *value when the knob has a value (pi3_set_knob or its environment variable), 0 when it is unset (every launch
// path then uses its own default), PI3_ERR_ARG for a name this build does not know.
extern "C" int pi3_get_knob(const char* name, long* value) {
  if (!name || !knob_known(name)) {
    pi3_set_error("pi3_get_knob: '%s' is not a knob of this build", name ? name : "(null)");
    return PI3_ERR_ARG;
  }
  KnobGuard g;
  Knob* k = knob_slot(name);
  if (!k || k->state != 2) return 0;
  if (value) *value = k->value;
  return 1;
}

// Back to "unset": launch paths use their defaults again (the environment variable is NOT re-read).
extern "C" int pi3_unset_knob(const char* name) {
  if (!name || !knob_known(name)) {
    pi3_set_error("pi3_unset_knob: '%s' is not a knob of this build", name ? name : "(null)");
    return PI3_ERR_ARG;
  }
  KnobGuard g;
  Knob* k = knob_slot(name);
  if (k) __atomic_store_n(&k->state, 1, __ATOMIC_RELEASE);
  return PI3_OK;
}

extern "C" const char* pi3_last_error(void) { return g_err; }

// "product" (make) or "dev" (make dev: -DPI3_DEV_VARIANTS -DPI3_DEV_ABLATIONS, the measured-slower kernel forms and the
// timing ablations compiled in)
extern "C" const char* pi3_build_flavor(void) {
#ifdef PI3_DEV_VARIANTS
  return "dev";
#else
  return "product";
#endif
}

extern "C" int pi3_abi_version(void) { return 7; }   // 7: pi3_get_knob / pi3_unset_knob / pi3_build_flavor, pi3_set_knob refuses unknown names; 6: dtype code 2 = IEEE half through the MoGe entries (pi3_attention / pi3_conv3x3 / pi3_patch_gather / pi3_groupnorm_apply / pi3_convt_scatter take a dtype); 5: pi3_rope_2d (the reference's curope.rope_2d contract); 4: pi3_sim3_umeyama_weighted (real-valued pair weights); 2: caller-provided workspaces (attention, group-norm statistics); 3: narrow-N GEMM / conv forms, pi3_cast_rows_pad, 4-channel granularity of the MoGe staging kernels

// Number of visible devices (does not create a context); used by the loader to fail loudly on a box without a GPU.
extern "C" int pi3_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}
