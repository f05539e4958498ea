// Surface normals for the dense voxel map of voxel.hip, and the shaded images of render.hip's views.
//
// The table's 64-byte slot is full, so the normals live beside it: nacc, caller-owned DEVICE memory of 4 x int64 per
// slot (Nx, Ny, Nz, cnt), parallel to the table and zeroed by the caller.  Every update is a 64-bit integer atomicAdd
// (the signed sums go through the unsigned atomic in two's complement), so the sums do not depend on the order in
// which the atomics land and the numpy oracle (tests/dense_normals_ref.py) reproduces every output byte for byte.
// Slots are looked up with slot_find (read-only, bounded by the capacity): nothing here claims a slot, the fusion
// kernels of voxel.hip ran first on the same inputs.
//
//   fuse_pixel_normals   stage 1: the normal of a pixel is the cross product of its neighbours' central differences,
//                        n = (P(y+1,x) - P(y-1,x)) x (P(y,x+1) - P(y,x-1)); with x right, y down, z forward it faces the
//                        camera that saw it.  q = rint((n / |n|) * 2^15) per axis is added to the pixel's voxel.
//   fuse_point_normals   stage 2: a chunk cloud's normals, rotated into the world frame and weighted by nweights.
//   extract_normals      one row per occupied (or kept) slot: key, N / |N| as fp32, min(cnt, 2^31 - 1).
//   render_shade         element-wise over render_resolve's index image: the normal in the camera's frame as RGB and a
//                        headlight shading along the optical axis.
//
// All arithmetic is f64 from the fp32 / int64 inputs, every operation rounded on its own in the order written (f64 add,
// multiply, divide and sqrt are correctly rounded on the device).  The Makefile compiles this file with
// -ffp-contract=off: under the library's -ffp-contract=fast the pragma alone is ignored.
//
// Contention: runs of equal keys among a wave's 64 consecutive candidates are merged in registers (wave_block.h,
// wave_merge_runs) and only the last lane of a run looks its slot up (one probe + up to four atomics).
//
// stats of the two fusion kernels (DEVICE uint64 [4], ACCUMULATED - the caller zeroes them): [0] contributions,
// [1] candidates that could not contribute (pixels: no full 4-neighbourhood; points: the point does not quantise),
// [2] degenerate normals (pixels: the cross product has no finite positive length; points: a zero or non-finite normal),
// [3] contributions whose slot was not found (0 whenever the matching fusion of voxel.hip ran first).
#include "common.h"
#include "voxel_table.h"
#include "wave_block.h"

#include <stdint.h>

namespace {

using namespace voxel_table;      // u64, kEmpty, point_key, slot_find, claim_rows, kExtractPer, pow2, blocks_for
using wave_block::block_sum;
using wave_block::wave_merge_runs;

typedef long long i64;

constexpr double kUnit = 32768.0;      // 2^15: one unit normal's fixed-point length

// fuse_pixels' predicate: mask, conf > thr, all three axes quantise
__device__ __forceinline__ bool candidate(const float* __restrict__ points, const float* __restrict__ conf,
                                          const unsigned char* __restrict__ masks, long i, float conf_thr, float inv_v,
                                          u64& key) {
  if (masks && !masks[i]) return false;
  if (conf && !(conf[i] > conf_thr)) return false;
  return point_key(points + 3 * i, inv_v, key);
}

// Every lane of the wave calls this (lanes without a voxel with valid = false).  v = Nx, Ny, Nz, cnt (two's complement)
// of this lane's pixel / row and 1 when it contributes, else all 0: the fifth word sums to the contributing pixels /
// rows of a run (cnt counts weights).  The last lane of a run of equal keys with one of them adds the run's totals to
// its slot of nacc.
__device__ __forceinline__ void wave_add_normals(const u64* __restrict__ table, u64 mask, u64* __restrict__ nacc,
                                                 bool valid, u64 key, u64 (&v)[5], bool contributes, bool skipped,
                                                 bool degenerate, u64* __restrict__ stats) {
  const bool tail = wave_merge_runs(valid, key, kEmpty, v);
  u64 lost = 0;
  if (valid && tail && v[4]) {
    const long s = slot_find(table, mask, key);
    if (s < 0) {
      lost = v[4];
    } else {
      u64* q = nacc + 4 * s;
      if (v[0]) atomicAdd(q + 0, v[0]);
      if (v[1]) atomicAdd(q + 1, v[1]);
      if (v[2]) atomicAdd(q + 2, v[2]);
      atomicAdd(q + 3, v[3]);
    }
  }
  lost = wave_sum_u64(lost);
  const u64 nc = __ballot(contributes), ns = __ballot(skipped), nd = __ballot(degenerate);
  if ((threadIdx.x & 63) == 0) {
    if (nc) atomicAdd(stats + 0, (u64)__popcll(nc));
    if (ns) atomicAdd(stats + 1, (u64)__popcll(ns));
    if (nd) atomicAdd(stats + 2, (u64)__popcll(nd));
    if (lost) atomicAdd(stats + 3, lost);
  }
}

__global__ __launch_bounds__(256) void fuse_pixel_normals_kernel(
    const u64* __restrict__ table, u64 mask, u64* __restrict__ nacc, const float* __restrict__ points,
    const float* __restrict__ conf, const unsigned char* __restrict__ masks, long n, int H, int W, float conf_thr,
    float inv_v, u64* __restrict__ stats) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  bool valid = false, contributes = false, skipped = false, degenerate = false;
  u64 key = kEmpty, v[5] = {0, 0, 0, 0, 0};
  if (i < n && candidate(points, conf, masks, i, conf_thr, inv_v, key)) {
    valid = true;
    // neighbours by (f, y, x): a wave may hold the end of one row and the start of the next, or of two frames
    const long row = i / W;
    const int x = (int)(i - row * W), y = (int)(row % H);
    u64 other;
    if (x >= 1 && x <= W - 2 && y >= 1 && y <= H - 2 && candidate(points, conf, masks, i - 1, conf_thr, inv_v, other) &&
        candidate(points, conf, masks, i + 1, conf_thr, inv_v, other) &&
        candidate(points, conf, masks, i - W, conf_thr, inv_v, other) &&
        candidate(points, conf, masks, i + W, conf_thr, inv_v, other)) {
      const float* l = points + 3 * (i - 1);
      const float* r = points + 3 * (i + 1);
      const float* u = points + 3 * (i - W);
      const float* d = points + 3 * (i + W);
      const double ax = (double)r[0] - (double)l[0], ay = (double)r[1] - (double)l[1], az = (double)r[2] - (double)l[2];
      const double bx = (double)d[0] - (double)u[0], by = (double)d[1] - (double)u[1], bz = (double)d[2] - (double)u[2];
      const double nx = by * az - bz * ay;
      const double ny = bz * ax - bx * az;
      const double nz = bx * ay - by * ax;
      const double l2 = (nx * nx + ny * ny) + nz * nz;
      if (l2 > 0.0 && __builtin_isfinite(l2)) {
        const double len = sqrt(l2);
        v[0] = (u64)(i64)rint((nx / len) * kUnit);
        v[1] = (u64)(i64)rint((ny / len) * kUnit);
        v[2] = (u64)(i64)rint((nz / len) * kUnit);
        v[3] = v[4] = 1ull;
        contributes = true;
      } else {
        degenerate = true;
      }
    } else {
      skipped = true;
    }
  }
  wave_add_normals(table, mask, nacc, valid, key, v, contributes, skipped, degenerate, stats);
}

// rint(x * 2^15) of one rotated component, kept within +-2^31 so that its product with a weight < 2^31 fits 63 bits
// (a unit normal gives |q| <= 2^15; a NaN from a non-finite rotation becomes -2^31, the same on every run)
__device__ __forceinline__ i64 fixed_component(double x) {
  double r = rint(x * kUnit);
  if (!(r >= -2147483648.0)) r = -2147483648.0;
  if (r > 2147483648.0) r = 2147483648.0;
  return (i64)r;
}

__global__ __launch_bounds__(256) void fuse_point_normals_kernel(
    const u64* __restrict__ table, u64 mask, u64* __restrict__ nacc, const float* __restrict__ points,
    const float* __restrict__ normals, const int* __restrict__ nweights, const double* __restrict__ rot, long n,
    float inv_v, u64* __restrict__ stats) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  bool valid = false, contributes = false, skipped = false, degenerate = false;
  u64 key = kEmpty, v[5] = {0, 0, 0, 0, 0};
  const int wi = i < n ? nweights[i] : 0;
  if (wi > 0) {
    const float fx = normals[3 * i], fy = normals[3 * i + 1], fz = normals[3 * i + 2];
    if (!(__builtin_isfinite(fx) && __builtin_isfinite(fy) && __builtin_isfinite(fz)) ||
        (fx == 0.0f && fy == 0.0f && fz == 0.0f)) {
      degenerate = true;
    } else if (!point_key(points + 3 * i, inv_v, key)) {
      skipped = true;
    } else {
      valid = contributes = true;
      const double nx = (double)fx, ny = (double)fy, nz = (double)fz;
      const i64 w = (i64)wi;
      v[0] = (u64)(w * fixed_component((rot[0] * nx + rot[1] * ny) + rot[2] * nz));
      v[1] = (u64)(w * fixed_component((rot[3] * nx + rot[4] * ny) + rot[5] * nz));
      v[2] = (u64)(w * fixed_component((rot[6] * nx + rot[7] * ny) + rot[8] * nz));
      v[3] = (u64)w;
      v[4] = 1ull;
    }
  }
  wave_add_normals(table, mask, nacc, valid, key, v, contributes, skipped, degenerate, stats);
}

// Occupied (kMasked: and kept) slots -> rows, claimed as voxel_extract_kernel's (claim_rows), so the two extractions
// of one table give the same rows in the same order of slots.  stats: [0] rows, [1] rows that did not fit max_out,
// [2] stored rows with a non-zero normal.
template <bool kMasked>
__global__ __launch_bounds__(256) void extract_normals_kernel(const u64* __restrict__ table, long capacity,
                                                              const i64* __restrict__ nacc,
                                                              const unsigned char* __restrict__ keep,
                                                              u64* __restrict__ keys, float* __restrict__ normals,
                                                              int* __restrict__ nweights, long max_out,
                                                              u64* __restrict__ stats) {
#pragma clang fp contract(off)
  const long s0 = (long)blockIdx.x * (256L * kExtractPer) + threadIdx.x;
  u64 at;
  const uint32_t occ = claim_rows<kMasked>(s0, table, capacity, keep, stats + 0, at);
  unsigned nonzero = 0, unstored = 0;
#pragma unroll 1
  for (int j = 0; j < kExtractPer; ++j) {
    if (!(occ >> j & 1u)) continue;
    if ((long)at >= max_out) {
      ++unstored;
      ++at;
      continue;
    }
    const long s = s0 + 256L * j;
    const i64* q = nacc + 4 * s;
    const i64 Nx = q[0], Ny = q[1], Nz = q[2], c = q[3];
    float ox = 0.0f, oy = 0.0f, oz = 0.0f;
    if (c != 0 && (Nx != 0 || Ny != 0 || Nz != 0)) {
      const double dx = (double)Nx, dy = (double)Ny, dz = (double)Nz;
      const double len = sqrt((dx * dx + dy * dy) + dz * dz);
      ox = (float)(dx / len);
      oy = (float)(dy / len);
      oz = (float)(dz / len);
      ++nonzero;
    }
    normals[3 * at] = ox;
    normals[3 * at + 1] = oy;
    normals[3 * at + 2] = oz;
    keys[at] = table[8 * s];
    nweights[at] = c > 0x7FFFFFFFll ? 0x7FFFFFFF : (c < 0 ? 0 : (int)c);
    ++at;
  }
  block_sum(nonzero, stats + 2);
  __syncthreads();                              // block_sum's LDS words are read by thread 0 until here
  block_sum(unstored, stats + 1);
}

constexpr int kShadePer = 8;                // pixels per thread: one counter atomic per 2048 pixels

// v rounded to an integer already: 0 for v <= 0 and for NaN, 255 for v >= 255
__device__ __forceinline__ unsigned char to_u8(double v) {
  if (!(v > 0.0)) return 0;
  return v >= 255.0 ? (unsigned char)255 : (unsigned char)v;
}

__global__ __launch_bounds__(256) void render_shade_kernel(const int* __restrict__ index,
                                                           const float* __restrict__ normals, long V,
                                                           const double* __restrict__ cams, long HW, long n,
                                                           unsigned char* __restrict__ normal_rgb,
                                                           unsigned char* __restrict__ shaded, u64* __restrict__ stats) {
#pragma clang fp contract(off)
  const long p0 = (long)blockIdx.x * (256L * kShadePer) + threadIdx.x;
  unsigned cnt = 0;
#pragma unroll
  for (int j = 0; j < kShadePer; ++j) {
    const long p = p0 + 256L * j;
    if (p >= n) break;
    const long idx = (long)index[p];
    unsigned char r = 0, g = 0, b = 0, s = 0;
    if (idx >= 0 && idx < V) {
      const float fx = normals[3 * idx], fy = normals[3 * idx + 1], fz = normals[3 * idx + 2];
      if (__builtin_isfinite(fx) && __builtin_isfinite(fy) && __builtin_isfinite(fz) &&
          (fx != 0.0f || fy != 0.0f || fz != 0.0f)) {
        const double* __restrict__ c = cams + (p / HW) * kCamDoubles;
        const double x = (double)fx, y = (double)fy, z = (double)fz;
        const double ncx = (c[0] * x + c[1] * y) + c[2] * z;
        const double ncy = (c[4] * x + c[5] * y) + c[6] * z;
        const double ncz = (c[8] * x + c[9] * y) + c[10] * z;
        r = to_u8(rint((ncx + 1.0) * 127.5));
        g = to_u8(rint((ncy + 1.0) * 127.5));
        b = to_u8(rint((ncz + 1.0) * 127.5));
        const double light = -ncz;                   // a headlight along the optical axis
        s = to_u8(rint(255.0 * (light > 0.0 ? light : 0.0)));
        ++cnt;
      }
    }
    normal_rgb[3 * p] = r;
    normal_rgb[3 * p + 1] = g;
    normal_rgb[3 * p + 2] = b;
    shaded[p] = s;
  }
  block_sum(cnt, stats + 0);
}

}  // namespace

extern "C" int pi3_voxel_fuse_pixel_normals(const void* table, long capacity, long long* nacc, const float* points,
                                            const float* conf, const unsigned char* masks, int N, int H, int W,
                                            float conf_logit_thr, float inv_voxel, unsigned long long* stats,
                                            void* stream) {
  const long n = (long)N * H * W;
  if (!table || !pow2(capacity) || !nacc || (n > 0 && !points) || !stats || N < 0 || H <= 0 || W <= 0 ||
      capacity < 2 * n || !positive_finite(inv_voxel)) {
    pi3_set_error("pi3_voxel_fuse_pixel_normals: bad arguments N=%d H=%d W=%d capacity=%ld inv_voxel=%g", N, H, W,
                  capacity, (double)inv_voxel);
    return PI3_ERR_ARG;
  }
  if (n == 0) return PI3_OK;
  hipLaunchKernelGGL(fuse_pixel_normals_kernel, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream,
                     (const u64*)table, (u64)(capacity - 1), (u64*)nacc, points, conf, masks, n, H, W, conf_logit_thr,
                     inv_voxel, (u64*)stats);
  return pi3_check_launch("voxel_fuse_pixel_normals");
}

extern "C" int pi3_voxel_fuse_point_normals(const void* table, long capacity, long long* nacc, const float* points,
                                            const float* normals, const int* nweights, const double* rot9, long n,
                                            float inv_voxel, unsigned long long* stats, void* stream) {
  if (!table || !pow2(capacity) || !nacc || (n > 0 && (!points || !normals || !nweights)) || !rot9 || !stats || n < 0 ||
      capacity < 2 * n || !positive_finite(inv_voxel)) {
    pi3_set_error("pi3_voxel_fuse_point_normals: bad arguments n=%ld capacity=%ld inv_voxel=%g", n, capacity,
                  (double)inv_voxel);
    return PI3_ERR_ARG;
  }
  if (n == 0) return PI3_OK;
  hipLaunchKernelGGL(fuse_point_normals_kernel, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream,
                     (const u64*)table, (u64)(capacity - 1), (u64*)nacc, points, normals, nweights, rot9, n, inv_voxel,
                     (u64*)stats);
  return pi3_check_launch("voxel_fuse_point_normals");
}

extern "C" int pi3_voxel_extract_normals(const void* table, long capacity, const long long* nacc,
                                         const unsigned char* keep_or_null, unsigned long long* keys, float* normals,
                                         int* nweights, long max_out, unsigned long long* stats, void* stream) {
  if (!table || !pow2(capacity) || !nacc || !keys || !normals || !nweights || !stats || max_out < 0) {
    pi3_set_error("pi3_voxel_extract_normals: bad arguments capacity=%ld max_out=%ld", capacity, max_out);
    return PI3_ERR_ARG;
  }
  if (pi3_zero_words("pi3_voxel_extract_normals", stats, 4, stream) != PI3_OK) return PI3_ERR_LAUNCH;
  const long span = 256L * kExtractPer;
  const dim3 grid((unsigned)((capacity + span - 1) / span));
  if (keep_or_null)
    hipLaunchKernelGGL(extract_normals_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, (const u64*)table,
                       capacity, (const i64*)nacc, keep_or_null, (u64*)keys, normals, nweights, max_out, (u64*)stats);
  else
    hipLaunchKernelGGL(extract_normals_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, (const u64*)table,
                       capacity, (const i64*)nacc, keep_or_null, (u64*)keys, normals, nweights, max_out, (u64*)stats);
  return pi3_check_launch("voxel_extract_normals");
}

extern "C" int pi3_render_shade(const int* index, const float* normals, long V, const double* cams, int M, int H, int W,
                                unsigned char* normal_rgb, unsigned char* shaded, unsigned long long* stats,
                                void* stream) {
  if (!index || (V > 0 && !normals) || V < 0 || V >= (1L << 31) || !cams || M <= 0 || H <= 0 || W <= 0 || !normal_rgb ||
      !shaded || !stats) {
    pi3_set_error("pi3_render_shade: bad arguments V=%ld M=%d H=%d W=%d", V, M, H, W);
    return PI3_ERR_ARG;
  }
  const long n = (long)M * H * W, span = 256L * kShadePer;
  hipLaunchKernelGGL(render_shade_kernel, dim3((unsigned)((n + span - 1) / span)), dim3(256), 0, (hipStream_t)stream,
                     index, normals, V, cams, (long)H * W, n, normal_rgb, shaded, (u64*)stats);
  return pi3_check_launch("render_shade");
}
