// Which chunks see the same surface: the co-occupancy of the chunks' dense clouds on one coarse grid, the candidate
// search of loop closure (loop_closure.py).  Integers only: the result does not depend on the order in which the
// atomics land, and tests/loop_closure_ref.py reproduces it byte for byte.
//
// points f32 [P][3], all chunks' clouds in the world frame, chunk c's rows offsets[c] .. offsets[c + 1] - 1 (offsets
// DEVICE int64 [C + 1]; a row before offsets[0] or from offsets[C] on belongs to no chunk and counts as dropped).
// The table is the voxel table's form (voxel_table.h): 64-byte slots, key | seven 64-bit mask words, bit c of the
// masks = chunk c has a point in the cell: C <= 448 in one pass.
//   clear   every slot empty, masks zero.
//   pass 1  a thread per point: voxel_table::point_key (the voxel quantiser at inv_cell), voxel_table::slot_claim, a
//           relaxed load of the mask word and, when the bit is not there yet, one 64-bit atomic OR (a cell of 16 cm
//           holds tens of a chunk's 2 cm voxels: most points find their bit set).
//   pass 2  a workgroup scans 256 x 16 slots.  For an occupied slot and every pair i <= j of set bits: counts[i][j] and
//           counts[j][i] += 1 (the diagonal once).  C <= kLdsChunks: the pairs are counted in the workgroup's LDS
//           (uint32 [C][C] upper triangle, at most 4096 per entry) and flushed with one global atomic per non-zero
//           entry; larger C: global atomics straight away (65 536+ entries, few hits each).
// counters: dropped points, occupied cells, points without a slot, the most chunks in one cell.
#include "common.h"
#include "voxel_table.h"
#include "wave_block.h"

namespace {

using voxel_table::u64;

constexpr int kMaxChunks = 448;          // 7 mask words
constexpr int kWords = 7;
constexpr int kLdsChunks = 64;           // 64 x 64 uint32 = 16 KB of LDS
constexpr int kPer = 16;                 // slots per thread in pass 2

__global__ __launch_bounds__(256) void overlap_clear_kernel(u64* __restrict__ table, long capacity) {
  const long s = (long)blockIdx.x * 256 + threadIdx.x;
  if (s < capacity) voxel_table::slot_reset(table + 8 * s);
}

// the chunk of row i: the last c with offsets[c] <= i, or -1
__device__ __forceinline__ int chunk_of(const long* __restrict__ offsets, int C, long i) {
  if (i < offsets[0] || i >= offsets[C]) return -1;
  int lo = 0, hi = C;                    // offsets[lo] <= i < offsets[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (offsets[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void overlap_mark_kernel(const float* __restrict__ points, long P,
                                                           const long* __restrict__ offsets, int C, float inv_cell,
                                                           u64* __restrict__ table, u64 mask,
                                                           u64* __restrict__ counters) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  bool dropped = false, lost = false;
  if (i < P) {
    const int c = chunk_of(offsets, C, i);
    u64 key;
    if (c < 0 || !voxel_table::point_key(points + 3 * i, inv_cell, key)) {
      dropped = true;
    } else {
      bool fresh;
      const long slot = voxel_table::slot_claim<8>(table, mask, mask, key, fresh);
      if (slot < 0) {
        lost = true;
      } else {
        u64* w = table + 8 * slot + 1 + (c >> 6);
        const u64 bit = 1ull << (c & 63);
        if (!(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(w, bit);
      }
    }
  }
  const bool flag[2] = {dropped, lost};
  const int at[2] = {0, 2};
  wave_block::block_count(flag, counters, at);
}

// f(i, j) for every pair i <= j of set bits of the seven words, i ascending, then j ascending
template <typename F>
__device__ __forceinline__ void for_each_pair(const u64 (&w)[kWords], F&& f) {
  for (int wi = 0; wi < kWords; ++wi) {
    u64 mi = w[wi];
    while (mi) {
      const int bi = __builtin_ctzll(mi);
      mi &= mi - 1;
      for (int wj = wi; wj < kWords; ++wj) {
        u64 mj = wj == wi ? (w[wj] & (~0ull << bi)) : w[wj];
        while (mj) {
          const int bj = __builtin_ctzll(mj);
          mj &= mj - 1;
          f(64 * wi + bi, 64 * wj + bj);
        }
      }
    }
  }
}

template <bool kLds>
__global__ __launch_bounds__(256) void overlap_count_kernel(const u64* __restrict__ table, long capacity, int C,
                                                            u64* __restrict__ counts, u64* __restrict__ counters) {
  __shared__ unsigned pair_n[kLds ? kLdsChunks * kLdsChunks : 1];
  __shared__ unsigned most;
  const int tid = (int)threadIdx.x;
  if (kLds)
    for (int e = tid; e < C * C; e += 256) pair_n[e] = 0u;
  if (tid == 0) most = 0u;
  __syncthreads();
  const long s0 = (long)blockIdx.x * 256 * kPer + tid;
  unsigned cells = 0, mine = 0;
  for (int k = 0; k < kPer; ++k) {
    const long s = s0 + 256L * k;
    if (s >= capacity) break;
    const u64* __restrict__ q = table + 8 * s;
    if (q[0] == voxel_table::kEmpty) continue;
    u64 w[kWords];
    unsigned n = 0;
#pragma unroll
    for (int j = 0; j < kWords; ++j) {
      w[j] = q[1 + j];
      n += (unsigned)__popcll(w[j]);
    }
    ++cells;
    mine = n > mine ? n : mine;
    for_each_pair(w, [&](int i, int j) {
      if (j >= C) return;                // (no bit at or above C is ever set: chunk_of stays below C)
      if (kLds) {
        atomicAdd(&pair_n[i * C + j], 1u);
      } else {
        atomicAdd(counts + (long)i * C + j, 1ull);
        if (i != j) atomicAdd(counts + (long)j * C + i, 1ull);
      }
    });
  }
  if (mine) atomicMax(&most, mine);
  __syncthreads();
  if (kLds)
    for (int e = tid; e < C * C; e += 256) {
      const int i = e / C, j = e - i * C;
      const unsigned n = i <= j ? pair_n[e] : 0u;
      if (n) {
        atomicAdd(counts + (long)i * C + j, (u64)n);
        if (i != j) atomicAdd(counts + (long)j * C + i, (u64)n);
      }
    }
  if (tid == 0 && most) atomicMax(counters + 3, (u64)most);
  wave_block::block_sum(cells, counters + 1);
}

}  // namespace

extern "C" int pi3_chunk_cooccupancy(const float* points, long P, const long* offsets, int C, float inv_cell,
                                     void* table, long capacity, unsigned long long* counts,
                                     unsigned long long* counters, void* stream) {
  const bool work = P > 0 && C > 0;
  if (P < 0 || C < 0 || C > kMaxChunks || !counters || (C > 0 && !counts) ||
      (work && (!points || !offsets || !table || !positive_finite(inv_cell) || !voxel_table::pow2(capacity) ||
                capacity / 2 < P))) {
    pi3_set_error("pi3_chunk_cooccupancy: bad arguments P=%ld (>= 0) C=%d (0 .. %d) inv_cell=%g (finite, > 0) "
                  "capacity=%ld (a power of two, >= 2 P), or a null pointer", P, C, kMaxChunks, (double)inv_cell,
                  capacity);
    return PI3_ERR_ARG;
  }
  if (pi3_zero_words("pi3_chunk_cooccupancy", counters, 4, stream) != PI3_OK ||
      (C > 0 && pi3_zero_words("pi3_chunk_cooccupancy", counts, (long)C * C, stream) != PI3_OK))
    return PI3_ERR_LAUNCH;
  if (!work) return PI3_OK;
  hipStream_t st = (hipStream_t)stream;
  const dim3 block(256);
  u64* t = (u64*)table;
  hipLaunchKernelGGL(overlap_clear_kernel, dim3(voxel_table::blocks_for(capacity)), block, 0, st, t, capacity);
  hipLaunchKernelGGL(overlap_mark_kernel, dim3(voxel_table::blocks_for(P)), block, 0, st, points, P, offsets, C,
                     inv_cell, t, (u64)(capacity - 1), (u64*)counters);
  const dim3 grid((unsigned)((capacity + 256L * kPer - 1) / (256L * kPer)));
  if (C <= kLdsChunks)
    hipLaunchKernelGGL(overlap_count_kernel<true>, grid, block, 0, st, (const u64*)t, capacity, C, (u64*)counts,
                       (u64*)counters);
  else
    hipLaunchKernelGGL(overlap_count_kernel<false>, grid, block, 0, st, (const u64*)t, capacity, C, (u64*)counts,
                       (u64*)counters);
  return pi3_check_launch("chunk_cooccupancy");
}
