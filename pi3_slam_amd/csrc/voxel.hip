// Dense voxel map: confidence-filtered fusion of pi3's per-pixel pointmaps (and of whole chunk clouds) into one
// open-addressing hash table of voxels on the device (voxel_table.h: slot layout, quantisation, row claim).
//
// Integer accumulators only: the sums do not depend on the order in which the atomics land, so a run is bitwise
// reproducible and a float32 numpy oracle (tests/dense_map_ref.py) reproduces it bit for bit.
// Extraction: centroid = v * (k + U / (W * 2^24)) in f64, stored fp32;  colour = (C + W/2) / W;  weight = min(W, 2^31-1).
//
// Contention: runs of equal keys among a wave's 64 consecutive candidates are merged in registers (wave_block.h,
// wave_merge_runs); the last lane of each run does one probe + up to seven 64-bit atomic adds.  Capacity is a power of
// two >= 2 x the candidates since the last clear (the caller's rule), so the table never fills; every probe loop is
// bounded by the capacity anyway, and a candidate that finds no slot is counted in stats[1] instead of looping.
//
// stats (caller-owned device memory, 4 x uint64): [0] dropped points, [1] table overflows (0 under the capacity rule),
// [2] voxels written by the last extract, [3] voxels the last extract could not store (max_out too small).
#include "common.h"
#include "voxel_table.h"
#include "wave_block.h"

#include <stdint.h>

namespace {

using namespace voxel_table;      // u64, kEmpty, pack_key, quantise, slot_claim, slot_reset, slot_centre, slot_colour,
                                  // claim_rows, kExtractPer, pow2, blocks_for
using wave_block::block_sum;
using wave_block::wave_merge_runs;

// add (w, U, C) to the slot of `key`; false when no slot was found within `capacity` probes
__device__ __forceinline__ bool slot_add(u64* __restrict__ table, u64 mask, u64 key, u64 w, u64 u0, u64 u1, u64 u2,
                                         u64 c0, u64 c1, u64 c2) {
  bool fresh;
  const long h = slot_claim<8>(table, mask, mask, key, fresh);
  if (h < 0) return false;
  u64* s = table + 8 * h;
  atomicAdd(s + 1, w);
  if (u0) atomicAdd(s + 2, u0);
  if (u1) atomicAdd(s + 3, u1);
  if (u2) atomicAdd(s + 4, u2);
  if (c0) atomicAdd(s + 5, c0);
  if (c1) atomicAdd(s + 6, c1);
  if (c2) atomicAdd(s + 7, c2);
  return true;
}

// Every lane of the wave calls this (invalid lanes with valid = false).  v = w, U0 U1 U2, C0 C1 C2 of this lane's
// candidate; the last lane of each run of equal keys adds the run's totals to the table.
__device__ __forceinline__ void wave_fuse(u64* __restrict__ table, u64 mask, bool valid, u64 key, u64 (&v)[7],
                                          bool dropped, u64* __restrict__ stats) {
  const bool tail = wave_merge_runs(valid, key, kEmpty, v);
  bool lost = false;
  if (valid && tail) lost = !slot_add(table, mask, key, v[0], v[1], v[2], v[3], v[4], v[5], v[6]);
  const u64 nd = __ballot(dropped), nl = __ballot(lost);
  if ((threadIdx.x & 63) == 0) {
    if (nd) atomicAdd(stats + 0, (u64)__popcll(nd));
    if (nl) atomicAdd(stats + 1, (u64)__popcll(nl));
  }
}

__device__ __forceinline__ uint32_t colour_u8(float c) {
  const float v = c * 255.0f;            // then truncation, as the keypoint colours (post.hip, gather_keypoints)
  return v >= 255.0f ? 255u : (v > 0.0f ? (uint32_t)v : 0u);
}

__global__ __launch_bounds__(256) void voxel_clear_kernel(u64* __restrict__ table, long capacity,
                                                          u64* __restrict__ stats) {
  const long stride = (long)gridDim.x * 256;
  for (long s = (long)blockIdx.x * 256 + threadIdx.x; s < capacity; s += stride) slot_reset(table + 8 * s);
  if (stats && blockIdx.x == 0 && threadIdx.x < 4) stats[threadIdx.x] = 0ull;
}

__global__ __launch_bounds__(256) void voxel_fuse_pixels_kernel(
    u64* __restrict__ table, u64 mask, const float* __restrict__ points, const float* __restrict__ conf,
    const unsigned char* __restrict__ masks, const float* __restrict__ imgs, long n, long HW, float conf_thr,
    float inv_v, u64* __restrict__ stats) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  bool valid = false, dropped = false;
  u64 key = kEmpty, v[7] = {1, 0, 0, 0, 0, 0, 0};
  if (i < n && (!masks || masks[i]) && (!conf || conf[i] > conf_thr)) {
    uint32_t kx, ky, kz, ux, uy, uz;
    const float px = points[3 * i], py = points[3 * i + 1], pz = points[3 * i + 2];
    if (quantise(px, inv_v, kx, ux) && quantise(py, inv_v, ky, uy) && quantise(pz, inv_v, kz, uz)) {
      valid = true;
      key = pack_key(kx, ky, kz);
      v[1] = ux; v[2] = uy; v[3] = uz;
      if (imgs) {
        const long f = i / HW, p = i - f * HW;
        const float* im = imgs + 3 * f * HW + p;
        v[4] = colour_u8(im[0]);
        v[5] = colour_u8(im[HW]);
        v[6] = colour_u8(im[2 * HW]);
      }
    } else {
      dropped = true;
    }
  }
  wave_fuse(table, mask, valid, key, v, dropped, stats);
}

__global__ __launch_bounds__(256) void voxel_fuse_points_kernel(
    u64* __restrict__ table, u64 mask, const float* __restrict__ points, const unsigned char* __restrict__ colors,
    const int* __restrict__ weights, long n, float inv_v, u64* __restrict__ stats) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  bool valid = false, dropped = false;
  u64 key = kEmpty, v[7] = {0, 0, 0, 0, 0, 0, 0};
  const int wi = (i < n) ? (weights ? weights[i] : 1) : 0;
  if (wi > 0) {
    uint32_t kx, ky, kz, ux, uy, uz;
    const float px = points[3 * i], py = points[3 * i + 1], pz = points[3 * i + 2];
    if (quantise(px, inv_v, kx, ux) && quantise(py, inv_v, ky, uy) && quantise(pz, inv_v, kz, uz)) {
      valid = true;
      const u64 w = (u64)wi;
      key = pack_key(kx, ky, kz);
      v[0] = w;
      v[1] = w * ux; v[2] = w * uy; v[3] = w * uz;
      if (colors) {
        v[4] = w * colors[3 * i];
        v[5] = w * colors[3 * i + 1];
        v[6] = w * colors[3 * i + 2];
      }
    } else {
      dropped = true;
    }
  }
  wave_fuse(table, mask, valid, key, v, dropped, stats);
}

__global__ __launch_bounds__(256) void voxel_rehash_kernel(const u64* __restrict__ src, long src_capacity,
                                                           u64* __restrict__ dst, u64 dst_mask,
                                                           u64* __restrict__ stats) {
  const long s = (long)blockIdx.x * 256 + threadIdx.x;
  if (s >= src_capacity) return;
  const u64* q = src + 8 * s;
  if (q[0] == kEmpty) return;
  if (!slot_add(dst, dst_mask, q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7])) atomicAdd(stats + 1, 1ull);
}

// Occupied slots -> output rows (claim_rows: the workgroup's slots and its rows).
// kMasked: only the occupied slots with keep[slot] != 0 (pi3_voxel_extract_kept); the rows themselves are computed alike.
template <bool kMasked>
__global__ __launch_bounds__(256) void voxel_extract_kernel(const u64* __restrict__ table, long capacity,
                                                            const unsigned char* __restrict__ keep, double vsize,
                                                            u64* __restrict__ keys, float* __restrict__ points,
                                                            unsigned char* __restrict__ colors,
                                                            int* __restrict__ weights, long max_out,
                                                            u64* __restrict__ stats) {
#pragma clang fp contract(off)
  const long s0 = (long)blockIdx.x * (256L * kExtractPer) + threadIdx.x;
  u64 at;
  const uint32_t occ = claim_rows<kMasked>(s0, table, capacity, keep, stats + 2, at);
  unsigned unstored = 0;
#pragma unroll 1
  for (int j = 0; j < kExtractPer; ++j) {
    if (!(occ >> j & 1u)) continue;
    if ((long)at >= max_out) {
      ++unstored;
      ++at;
      continue;
    }
    const u64* q = table + 8 * (s0 + 256L * j);
    const u64 W = q[1];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      points[3 * at + a] = (float)(vsize * slot_centre(q, a));
      colors[3 * at + a] = (unsigned char)slot_colour(q, a);
    }
    keys[at] = q[0];
    weights[at] = W > 0x7FFFFFFFull ? 0x7FFFFFFF : (int)W;     // saturated (the centroid and colour use the full W)
    ++at;
  }
  block_sum(unstored, stats + 3);
}

}  // namespace

extern "C" int pi3_voxel_clear(void* table, long capacity, unsigned long long* stats, void* stream) {
  if (!table || !pow2(capacity)) {
    pi3_set_error("pi3_voxel_clear: bad arguments (capacity %ld must be a power of two)", capacity);
    return PI3_ERR_ARG;
  }
  long nb = (capacity + 255) / 256;
  if (nb > 65536) nb = 65536;
  hipLaunchKernelGGL(voxel_clear_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, (u64*)table, capacity,
                     (u64*)stats);
  return pi3_check_launch("voxel_clear");
}

extern "C" int pi3_voxel_fuse_pixels(void* table, long capacity, const float* points, const float* conf,
                                     const unsigned char* masks, const float* imgs, int N, int H, int W,
                                     float conf_logit_thr, float inv_voxel, unsigned long long* stats, void* stream) {
  const long n = (long)N * H * W;
  if (!table || !pow2(capacity) || (n > 0 && !points) || !stats || N < 0 || H <= 0 || W <= 0 || capacity < 2 * n ||
      !positive_finite(inv_voxel)) {
    pi3_set_error("pi3_voxel_fuse_pixels: bad arguments N=%d H=%d W=%d capacity=%ld inv_voxel=%g", N, H, W, capacity,
                  (double)inv_voxel);
    return PI3_ERR_ARG;
  }
  if (n == 0) return PI3_OK;
  hipLaunchKernelGGL(voxel_fuse_pixels_kernel, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, (u64*)table,
                     (u64)(capacity - 1), points, conf, masks, imgs, n, (long)H * W, conf_logit_thr, inv_voxel,
                     (u64*)stats);
  return pi3_check_launch("voxel_fuse_pixels");
}

extern "C" int pi3_voxel_fuse_points(void* table, long capacity, const float* points, const unsigned char* colors,
                                     const int* weights, long n, float inv_voxel, unsigned long long* stats,
                                     void* stream) {
  if (!table || !pow2(capacity) || (n > 0 && !points) || !stats || n < 0 || capacity < 2 * n ||
      !positive_finite(inv_voxel)) {
    pi3_set_error("pi3_voxel_fuse_points: bad arguments n=%ld capacity=%ld inv_voxel=%g", n, capacity,
                  (double)inv_voxel);
    return PI3_ERR_ARG;
  }
  if (n == 0) return PI3_OK;
  hipLaunchKernelGGL(voxel_fuse_points_kernel, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, (u64*)table,
                     (u64)(capacity - 1), points, colors, weights, n, inv_voxel, (u64*)stats);
  return pi3_check_launch("voxel_fuse_points");
}

extern "C" int pi3_voxel_rehash(const void* src_table, long src_capacity, void* dst_table, long dst_capacity,
                                unsigned long long* stats, void* stream) {
  if (!src_table || !dst_table || !stats || !pow2(src_capacity) || !pow2(dst_capacity) ||
      dst_capacity < src_capacity || src_table == dst_table) {
    pi3_set_error("pi3_voxel_rehash: bad arguments %ld -> %ld", src_capacity, dst_capacity);
    return PI3_ERR_ARG;
  }
  hipLaunchKernelGGL(voxel_rehash_kernel, dim3(blocks_for(src_capacity)), dim3(256), 0, (hipStream_t)stream,
                     (const u64*)src_table, src_capacity, (u64*)dst_table, (u64)(dst_capacity - 1), (u64*)stats);
  return pi3_check_launch("voxel_rehash");
}

namespace {

int extract_launch(const char* what, const void* table, long capacity, const unsigned char* keep, bool masked,
                   double voxel_size, unsigned long long* keys, float* points, unsigned char* colors, int* weights,
                   long max_out, unsigned long long* stats, void* stream) {
  if (!table || !pow2(capacity) || (masked && !keep) || !keys || !points || !colors || !weights || !stats ||
      max_out < 0 || !positive_finite(voxel_size)) {
    pi3_set_error("%s: bad arguments capacity=%ld max_out=%ld", what, capacity, max_out);
    return PI3_ERR_ARG;
  }
  if (pi3_zero_words(what, stats + 2, 2, stream) != PI3_OK) return PI3_ERR_LAUNCH;
  const long span = 256L * kExtractPer;
  const dim3 grid((unsigned)((capacity + span - 1) / span));
  if (masked)
    hipLaunchKernelGGL(voxel_extract_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, (const u64*)table, capacity,
                       keep, voxel_size, (u64*)keys, points, colors, weights, max_out, (u64*)stats);
  else
    hipLaunchKernelGGL(voxel_extract_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, (const u64*)table, capacity,
                       keep, voxel_size, (u64*)keys, points, colors, weights, max_out, (u64*)stats);
  return pi3_check_launch(what + 4);       // without the "pi3_" prefix, as the other entry points report
}

}  // namespace

extern "C" int pi3_voxel_extract(const void* table, long capacity, double voxel_size, unsigned long long* keys,
                                 float* points, unsigned char* colors, int* weights, long max_out,
                                 unsigned long long* stats, void* stream) {
  return extract_launch("pi3_voxel_extract", table, capacity, nullptr, false, voxel_size, keys, points, colors, weights,
                        max_out, stats, stream);
}

extern "C" int pi3_voxel_extract_kept(const void* table, long capacity, double voxel_size, unsigned long long* keys,
                                      float* points, unsigned char* colors, int* weights, long max_out,
                                      unsigned long long* stats, const unsigned char* keep, void* stream) {
  return extract_launch("pi3_voxel_extract_kept", table, capacity, keep, true, voxel_size, keys, points, colors, weights,
                        max_out, stats, stream);
}
