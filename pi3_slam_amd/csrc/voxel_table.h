// The voxel hash table's slot layout, key packing and hash, shared by voxel.hip (fusion, extraction) and
// voxel_clean.hip (neighbour-support and component filters).
//
// Slot (64 B, 8 x uint64): key | W | U0 U1 U2 | C0 C1 C2.  key = the three voxel indices, each biased by 2^20 and packed
// at 21 bits (x << 42 | y << 21 | z); all ones = empty.  Linear probing from mix64(key) & mask; capacity a power of two.
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

inline bool pow2(long c) { return c > 0 && (c & (c - 1)) == 0; }

inline unsigned blocks_for(long n) { return (unsigned)((n + 255) / 256); }

}  // namespace voxel_table
