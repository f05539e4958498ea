// The voxel hash table: slot layout, quantisation of a point, key packing, hash, the slot claim and lookup, the walk
// over the cells around a key, a slot's centroid and colour, and the row claim of the extractions.  Shared by voxel.hip
// (fusion, extraction), voxel_normals.hip (the normals beside the table), voxel_clean.hip (neighbour-support and
// component filters), voxel_mesh.hip (surface nets; its cell table is claimed with the same loop), voxel_carve.hip
// (depth-keyframe carving), cloud_nn.hip (a cell grid in the table's form) and occupancy.hip (the quantiser alone: its
// grid is dense).
//
// Slot (64 B, 8 x uint64): key | W | U0 U1 U2 | C0 C1 C2.
//   key   the three voxel indices, each biased by 2^20 and packed at 21 bits (x << 42 | y << 21 | z); all ones = empty.
//         Slots are claimed with a 64-bit CAS; linear probing from mix64(key) & mask; capacity a power of two.
//   W     summed integer weight;  U = sum w * u with u = the fixed-point offset inside the voxel (24 fraction bits);
//   C     sum w * rgb (uint8 colours).
//
// Quantisation of one point p (per axis, fp32, no contraction):  s = p * inv_v;  k = floor(s);  f = s - k (exact);
//   u = min(trunc(f * 2^24), 2^24 - 1)   (an exact integer whenever |s| >= 1; the clamp catches s in (-2^-24, 0), where
//   s - k rounds to 1).  A point is dropped (and counted) when it is not finite or |k| >= 2^20.
#pragma once
#include "wave_block.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace voxel_table {

typedef unsigned long long u64;

constexpr u64 kEmpty = ~0ull;
constexpr int kBias = 1 << 20;
constexpr uint32_t kFieldMask = 0x1FFFFFu;      // one biased 21-bit index

__device__ __forceinline__ u64 mix64(u64 x) {     // splitmix64 finaliser: neighbouring keys land far apart
  x ^= x >> 30;
  x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27;
  x *= 0x94d049bb133111ebull;
  x ^= x >> 31;
  return x;
}

__device__ __forceinline__ u64 pack_key(uint32_t kx, uint32_t ky, uint32_t kz) {
  return ((u64)kx << 42) | ((u64)ky << 21) | (u64)kz;
}

// one axis: voxel index (biased) and fixed-point offset; false = drop
__device__ __forceinline__ bool quantise(float p, float inv_v, uint32_t& kb, uint32_t& u) {
#pragma clang fp contract(off)
  if (!__builtin_isfinite(p)) return false;
  float s = p * inv_v;
  asm volatile("" : "+v"(s));          // the rounded product, never an fma with the subtraction below
  const float k = floorf(s);
  if (!(fabsf(k) < 1048576.0f)) return false;
  const float f = s - k;
  const float uf = f * 16777216.0f;    // 2^24
  uint32_t ui = (uint32_t)uf;
  u = ui > 0xFFFFFFu ? 0xFFFFFFu : ui;
  kb = (uint32_t)((int)k + kBias);
  return true;
}

// the key of the point p[0..3) alone; false = drop
__device__ __forceinline__ bool point_key(const float* __restrict__ p, float inv_v, u64& key) {
  uint32_t kx, ky, kz, u;
  if (!(quantise(p[0], inv_v, kx, u) && quantise(p[1], inv_v, ky, u) && quantise(p[2], inv_v, kz, u))) return false;
  key = pack_key(kx, ky, kz);
  return true;
}

// the biased index of axis a (0 = x, 1 = y, 2 = z)
__device__ __forceinline__ uint32_t key_field(u64 key, int a) { return (uint32_t)(key >> (42 - 21 * a)) & kFieldMask; }

// A representable voxel index has |k| < 2^20, i.e. a biased field in 1 .. 2^21 - 1.  kb + d for a small offset d, tested
// on the field BEFORE a key is composed: an index that leaves the range names no voxel and never carries into the next
// field.
__device__ __forceinline__ bool field_offset(uint32_t kb, int d, uint32_t& out) {
  const int v = (int)kb + d;
  out = (uint32_t)v;
  return v >= 1 && v <= (int)kFieldMask;
}

// The cells around the voxel (kx, ky, kz) (biased fields) with max(|dx|, |dy|, |dz|) <= kRadius, the voxel itself only
// when kSelf, in x-major order (dx outermost, dz innermost): f(dx, dy, dz, key of the cell).  A cell whose index
// leaves the range on any axis is skipped.  The loops carry no unroll pragma: the callers' bodies are table lookups,
// and what the compiler makes of them rolled is what they were measured with (voxel_mesh.hip's vertex kernel, which
// needs dx, dy, dz as constants, keeps a written-out copy for that reason).
template <int kRadius, bool kSelf, typename F>
__device__ __forceinline__ void for_each_neighbour(uint32_t kx, uint32_t ky, uint32_t kz, F&& f) {
  for (int dx = -kRadius; dx <= kRadius; ++dx) {
    uint32_t nx, ny, nz;
    if (!field_offset(kx, dx, nx)) continue;
    for (int dy = -kRadius; dy <= kRadius; ++dy) {
      if (!field_offset(ky, dy, ny)) continue;
      for (int dz = -kRadius; dz <= kRadius; ++dz) {
        if ((!kSelf && (dx | dy | dz) == 0) || !field_offset(kz, dz, nz)) continue;
        f(dx, dy, dz, pack_key(nx, ny, nz));
      }
    }
  }
}

// Find or claim the slot of `key`: the only place a key word is written.  `keys` holds one key word every kStride
// words (8: a table of 64-byte slots; 1: a bare key array), linear probing from mix64(key) & mask, a relaxed load
// first and a 64-bit CAS only on an empty word.  Returns the slot, or -1 after last_probe + 1 probes (last_probe <= mask:
// a table without a free slot cannot make it spin); `fresh` says whether this call's CAS claimed it.
template <int kStride>
__device__ __forceinline__ long slot_claim(u64* __restrict__ keys, u64 mask, u64 last_probe, u64 key, bool& fresh) {
  fresh = false;
  u64 h = mix64(key) & mask;
  for (u64 probe = 0; probe <= last_probe; ++probe) {
    u64* s = keys + kStride * h;
    u64 cur = __hip_atomic_load(s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == kEmpty) {
      const u64 old = atomicCAS(s, kEmpty, key);
      fresh = old == kEmpty;
      cur = fresh ? key : old;
    }
    if (cur == key) return (long)h;
    h = (h + 1) & mask;
  }
  return -1;
}

// Read-only lookup: the slot that holds `key`, or -1.  Stops at the key, at an empty slot, or after `capacity` probes
// (a malformed table without an empty slot cannot make it spin).
__device__ __forceinline__ long slot_find(const u64* __restrict__ table, u64 mask, u64 key) {
  u64 h = mix64(key) & mask;
  for (u64 probe = 0; probe <= mask; ++probe) {
    const u64 cur = table[8 * h];
    if (cur == key) return (long)h;
    if (cur == kEmpty) return -1;
    h = (h + 1) & mask;
  }
  return -1;
}

// an empty slot with zero words
__device__ __forceinline__ void slot_reset(u64* __restrict__ slot) {
  ulonglong2* p = reinterpret_cast<ulonglong2*>(slot);
  p[0] = make_ulonglong2(kEmpty, 0ull);
  p[1] = make_ulonglong2(0ull, 0ull);
  p[2] = make_ulonglong2(0ull, 0ull);
  p[3] = make_ulonglong2(0ull, 0ull);
}

// The centroid of the occupied slot q on one axis, in voxel units: k + U / (W 2^24), f64, and its rounded colour
// (C + W / 2) / W.  A product that feeds a division, a division that feeds an add: there is no multiply-add to contract,
// so the bytes are the same under -ffp-contract=fast (voxel.hip) and =off (voxel_mesh.hip, voxel_carve.hip).
__device__ __forceinline__ double slot_centre(const u64* __restrict__ q, int axis) {
  const int k = (int)key_field(q[0], axis) - kBias;
  return (double)k + (double)q[2 + axis] / ((double)q[1] * 16777216.0);
}
__device__ __forceinline__ u64 slot_colour(const u64* __restrict__ q, int axis) {
  return (q[5 + axis] + q[1] / 2) / q[1];
}

constexpr int kExtractPer = 16;                 // slots per thread: one row-counter atomic per 4096 slots

// Occupied slots -> output rows, the part the extractions share.  A workgroup covers 256 x kExtractPer slots (coalesced:
// slot = s0 + j * 256 with s0 = block * 256 * kExtractPer + tid), counts its occupied ones (kMasked: those with
// keep[slot] != 0) and claims its rows with ONE atomicAdd on *row_counter.  Returns the thread's occupancy, bit j for
// slot s0 + j * 256, and in `at` the row of its first set bit; its further rows follow one by one.  The order of the
// rows is arbitrary (the host sorts by key).  Every thread of the workgroup calls this, once per kernel.
template <bool kMasked>
__device__ __forceinline__ uint32_t claim_rows(long s0, const u64* __restrict__ table, long capacity,
                                               const unsigned char* __restrict__ keep, u64* __restrict__ row_counter,
                                               u64& at) {
  __shared__ u64 block_base;
  uint32_t occ = 0;
#pragma unroll
  for (int j = 0; j < kExtractPer; ++j) {
    const long s = s0 + 256L * j;
    if (s < capacity && table[8 * s] != kEmpty && (!kMasked || keep[s])) occ |= 1u << j;
  }
  u64 tot;
  const u64 before = wave_block::block_exclusive_scan((u64)__popc(occ), tot);
  if (threadIdx.x == 0) block_base = tot ? atomicAdd(row_counter, tot) : 0ull;
  __syncthreads();
  at = block_base + before;
  return occ;
}

inline bool pow2(long c) { return c > 0 && (c & (c - 1)) == 0; }

inline unsigned blocks_for(long n) { return (unsigned)((n + 255) / 256); }

}  // namespace voxel_table
