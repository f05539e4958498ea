// Dense map -> camera views: a z-buffered splat renderer for the voxel map of voxel.hip.
//
// One thread per (voxel, camera): grid.x walks the voxels in blocks of 256, grid.y the cameras, so the 20 doubles of a
// camera are uniform per block (scalar loads).  A voxel is drawn as an axis-aligned square of half-width r pixels
// around its projection; every pixel of the square takes a 64-bit atomicMin of
//     (float_bits((float)zc) << 32) | row
// into a z-buffer that pi3_render_splat first fills with all ones (= empty).
// zc > 0, so the fp32 bit pattern orders like the value; equal depths resolve to the smaller row index.  min is
// commutative, associative and idempotent: the image does not depend on the order in which the atomics land, and the
// f64 numpy oracle (tests/render_ref.py) reproduces it bit for bit.
//
// Arithmetic per voxel (f64, no contraction; cam = world->camera 3x4 row-major, fx fy cx cy, ortho flag, 3 spare):
//   skip when a coordinate is not finite or weights[i] < min_weight
//   xc = ((r00 x + r01 y) + r02 z) + t0, likewise yc, zc;  skip unless near < zc <= far
//   perspective:  u = fx (xc / zc) + cx,  v = fy (yc / zc) + cy,  r = splat_scale voxel_size fx / zc
//   orthographic: u = fx xc + cx,         v = fy yc + cy,         r = splat_scale voxel_size fx
//   r = min(max(r, 0.5), 16); a clamp at 16 is counted in stats[1]
//   x0 = max(ceil(u - r), 0), x1 = min(floor(u + r), W - 1), same for y (pixel i has its centre at i);
//   an empty range (or a NaN) draws nothing and is counted in stats[0]
//
// Traffic: most atomics would lose (a footprint is ~8 x 8 pixels at 2 m and nearer voxels have already landed), so
// every pixel is first read with a plain relaxed agent-scope load and the atomic is issued only when the stored value
// is larger.  A wave whose 64 voxels all miss the frustum leaves before any footprint loop.
//
// stats (caller-owned device memory, 4 x uint64, ACCUMULATED - the caller zeroes them): [0] voxels that passed the
// depth test but touch no pixel, [1] radius clamps at 16, [2] non-empty pixels counted by pi3_render_resolve,
// [3] atomics issued (development build only: the timing tool's issued-vs-skipped figure; 0 in the product).
#include "common.h"
#include "wave_block.h"

#include <stdint.h>

namespace {

typedef unsigned long long u64;

constexpr u64 kEmptyPixel = ~0ull;
constexpr double kMinRadius = 0.5, kMaxRadius = 16.0;

__global__ __launch_bounds__(256) void render_splat_kernel(
    const float* __restrict__ points, const int* __restrict__ weights, long V, const double* __restrict__ cams, int H,
    int W, double sv, int min_weight, double near, double far, u64* __restrict__ zbuf, u64* __restrict__ stats) {
#pragma clang fp contract(off)
  const double* __restrict__ c = cams + (long)blockIdx.y * kCamDoubles;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63);
  bool draw = false, culled = false, clamped = false;
  int x0 = 0, x1 = -1, y0 = 0, y1 = -1;
  float zf = 0.0f;
  if (i < V && (!weights || weights[i] >= min_weight)) {
    const double x = (double)points[3 * i], y = (double)points[3 * i + 1], z = (double)points[3 * i + 2];
    if (__builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z)) {
      const double xc = ((c[0] * x + c[1] * y) + c[2] * z) + c[3];
      const double yc = ((c[4] * x + c[5] * y) + c[6] * z) + c[7];
      const double zc = ((c[8] * x + c[9] * y) + c[10] * z) + c[11];
      if (zc > near && zc <= far) {
        const double fx = c[12], fy = c[13], cx = c[14], cy = c[15];
        double u, v, r;
        if (c[16] != 0.0) {
          u = fx * xc + cx;
          v = fy * yc + cy;
          r = sv * fx;
        } else {
          u = fx * (xc / zc) + cx;
          v = fy * (yc / zc) + cy;
          r = sv * fx / zc;
        }
        if (r > kMaxRadius) {
          r = kMaxRadius;
          clamped = true;
        }
        if (!(r >= kMinRadius)) r = kMinRadius;
        double fx0 = ceil(u - r), fx1 = floor(u + r), fy0 = ceil(v - r), fy1 = floor(v + r);
        if (fx0 < 0.0) fx0 = 0.0;
        if (fy0 < 0.0) fy0 = 0.0;
        if (fx1 > (double)(W - 1)) fx1 = (double)(W - 1);
        if (fy1 > (double)(H - 1)) fy1 = (double)(H - 1);
        if (fx0 <= fx1 && fy0 <= fy1) {      // false for an empty range and for NaN: both bounds are in [0, W - 1] here
          draw = true;
          x0 = (int)fx0; x1 = (int)fx1; y0 = (int)fy0; y1 = (int)fy1;
          zf = (float)zc;
        } else {
          culled = true;
        }
      }
    }
  }
  const u64 nc = __ballot(culled), nk = __ballot(clamped);
  if (lane == 0) {
    if (nc) atomicAdd(stats + 0, (u64)__popcll(nc));
    if (nk) atomicAdd(stats + 1, (u64)__popcll(nk));
  }
  if (!__ballot(draw)) return;              // the whole wave is outside this camera's frustum
  u64 issued = 0;
  if (draw) {
    const u64 val = ((u64)__float_as_uint(zf) << 32) | (u64)(uint32_t)i;
    u64* __restrict__ img = zbuf + (long)blockIdx.y * H * W;
    for (int py = y0; py <= y1; ++py) {
      u64* row = img + (long)py * W;
      for (int px = x0; px <= x1; ++px) {
        if (__hip_atomic_load(row + px, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > val) {
          atomicMin(row + px, val);
          ++issued;
        }
      }
    }
  }
#ifdef PI3_DEV_VARIANTS
  issued = wave_sum_u64(issued);
  if (lane == 0 && issued) atomicAdd(stats + 3, issued);
#else
  (void)issued;
#endif
}

constexpr int kResolvePer = 8;              // pixels per thread: one counter atomic per 2048 pixels

__global__ __launch_bounds__(256) void render_resolve_kernel(const u64* __restrict__ zbuf,
                                                             const unsigned char* __restrict__ colors, long V, long n,
                                                             float* __restrict__ depth, unsigned char* __restrict__ color,
                                                             int* __restrict__ index, u64* __restrict__ stats) {
  const long p0 = (long)blockIdx.x * (256L * kResolvePer) + threadIdx.x;
  unsigned cnt = 0;
#pragma unroll
  for (int j = 0; j < kResolvePer; ++j) {
    const long p = p0 + 256L * j;
    if (p >= n) break;
    const u64 val = zbuf[p];
    const long row = (long)(val & 0xFFFFFFFFull);
    float d = 0.0f;
    int idx = -1;
    unsigned char r = 0, g = 0, b = 0;
    if (val != kEmptyPixel && row < V) {    // row < V: a z-buffer that this map did not write is never dereferenced
      d = __uint_as_float((uint32_t)(val >> 32));
      idx = (int)row;
      if (colors) {
        r = colors[3 * row];
        g = colors[3 * row + 1];
        b = colors[3 * row + 2];
      }
      ++cnt;
    }
    depth[p] = d;
    index[p] = idx;
    color[3 * p] = r;
    color[3 * p + 1] = g;
    color[3 * p + 2] = b;
  }
  wave_block::block_sum(cnt, stats + 2);
}

}  // namespace

extern "C" int pi3_render_splat(const float* points, const int* weights, long V, const double* cams, int M, int H, int W,
                                double voxel_size, double splat_scale, int min_weight, double near, double far,
                                unsigned long long* zbuf, unsigned long long* stats, void* stream) {
  if ((V > 0 && !points) || V < 0 || V >= (1L << 31) || !cams || !zbuf || !stats || M <= 0 || M > 65535 || H <= 0 ||
      W <= 0 || !positive_finite(voxel_size) || !positive_finite(splat_scale) || !(near >= 0.0) || far != far) {
    pi3_set_error("pi3_render_splat: bad arguments V=%ld M=%d H=%d W=%d voxel_size=%g splat_scale=%g near=%g far=%g", V,
                  M, H, W, voxel_size, splat_scale, near, far);
    return PI3_ERR_ARG;
  }
  if (hipMemsetAsync(zbuf, 0xFF, sizeof(u64) * (size_t)M * H * W, (hipStream_t)stream) != hipSuccess) {
    pi3_set_error("pi3_render_splat: hipMemsetAsync failed");
    return PI3_ERR_LAUNCH;
  }
  if (V == 0) return PI3_OK;
  hipLaunchKernelGGL(render_splat_kernel, dim3((unsigned)((V + 255) / 256), (unsigned)M), dim3(256), 0,
                     (hipStream_t)stream, points, weights, V, cams, H, W, splat_scale * voxel_size, min_weight, near, far,
                     (u64*)zbuf, (u64*)stats);
  return pi3_check_launch("render_splat");
}

extern "C" int pi3_render_resolve(const unsigned long long* zbuf, const unsigned char* colors, long V, int M, int H,
                                  int W, float* depth, unsigned char* color, int* index, unsigned long long* stats,
                                  void* stream) {
  if (!zbuf || (V > 0 && !colors) || V < 0 || V >= (1L << 31) || M <= 0 || H <= 0 || W <= 0 || !depth || !color ||
      !index || !stats) {
    pi3_set_error("pi3_render_resolve: bad arguments V=%ld M=%d H=%d W=%d", V, M, H, W);
    return PI3_ERR_ARG;
  }
  const long n = (long)M * H * W, span = 256L * kResolvePer;
  hipLaunchKernelGGL(render_resolve_kernel, dim3((unsigned)((n + span - 1) / span)), dim3(256), 0, (hipStream_t)stream,
                     (const u64*)zbuf, colors, V, n, depth, color, index, (u64*)stats);
  return pi3_check_launch("render_resolve");
}
