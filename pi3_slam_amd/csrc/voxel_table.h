// The voxel hash table: slot layout, quantisation of a point, key packing, hash, lookup and the row claim of the
// extractions.  Shared by voxel.hip (fusion, extraction), voxel_normals.hip (the normals beside the table) and
// voxel_clean.hip (neighbour-support and component filters).
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
  __shared__ u64 wave_tot[4];
  __shared__ u64 block_base;
  const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
  uint32_t occ = 0;
#pragma unroll
  for (int j = 0; j < kExtractPer; ++j) {
    const long s = s0 + 256L * j;
    if (s < capacity && table[8 * s] != kEmpty && (!kMasked || keep[s])) occ |= 1u << j;
  }
  const u64 cnt = (u64)__popc(occ);
  u64 incl = cnt;                                  // inclusive prefix over the wave
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const u64 o = __shfl_up(incl, d, 64);
    if (lane >= d) incl += o;
  }
  if (lane == 63) wave_tot[wv] = incl;
  __syncthreads();
  if (tid == 0) {
    const u64 tot = wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
    block_base = tot ? atomicAdd(row_counter, tot) : 0ull;
  }
  __syncthreads();
  at = block_base + incl - cnt;
  for (int w = 0; w < wv; ++w) at += wave_tot[w];
  return occ;
}

inline bool pow2(long c) { return c > 0 && (c & (c - 1)) == 0; }

inline unsigned blocks_for(long n) { return (unsigned)((n + 255) / 256); }

}  // namespace voxel_table
