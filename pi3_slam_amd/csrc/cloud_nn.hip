// Exact radius-bounded nearest neighbour between two point clouds through a uniform cell grid: the distance search of
// map_eval.py (accuracy / completeness / F-score of a dense map against a reference cloud).
//
// The grid is a hash table of cells in the voxel table's form (voxel_table.h: the quantiser, the 21-bit key packing,
// mix64, linear probing, field_offset; 64-byte slots, so slot_find serves it as it is):
//   slot (8 x uint64)  key | count | start | fill | cursor (slot 0 only) | 3 spare
//   cells              n rows of 16 B: x, y, z as f32 bits and the point's original index (int32), grouped by cell; the
//                      rows of the cell in a slot are cells[start .. start + count).
// Index build (pi3_cloud_index_build), all on the stream, no allocation, no synchronisation:
//   clear   every slot empty with zero words;
//   (a)     every point finds or claims the slot of its cell key (slot_claim, as voxel.hip) and adds 1 to the slot's
//           count;
//   (b)     every occupied slot claims `count` contiguous rows: an exclusive scan of the counts over the workgroup and
//           ONE atomic add per workgroup on the cursor (word 4 of slot 0; after the pass it holds the number of rows);
//   (c)     every point finds its slot again, takes row start + atomicAdd(fill, 1) and writes its 16 bytes.
// The order of the rows inside a cell and of the cells in the array depends on the order the atomics land in; the query
// does not (below).  A point the quantiser drops (not finite, or |cell index| >= 2^20) gets no row.
//
// Query (pi3_cloud_nearest): one thread per query; it visits the 27 cells around its own (a cell whose index leaves
// |k| < 2^20 does not exist: field_offset) and, for every row p of them, in f64 with every operation rounded on its own
// (the Makefile compiles this file with -ffp-contract=off):
//   dx = (double)qx - (double)px, likewise dy, dz;   d2 = (dx dx + dy dy) + dz dz;
//   candidate when d2 <= max_dist max_dist (the product formed once, in f64);
//   result = the candidate with the smallest d2, among equal d2 the smallest original index: independent of the row
//   order, bitwise reproducible, and what tests/cloud_nn_ref.py computes by brute force.
// No candidate, or a dropped query: d2 = +inf, idx = -1.  NaN is written nowhere.
// A cell's list is read as whole 16-byte rows (one dwordx4 load per row and lane).  Lanes of a wave walk different
// lists, so the loads are gathers; queries that are neighbours in memory are usually neighbours in space (voxel rows in
// key order, pixels of a frame) and then share cells and cache lines.
#include "common.h"
#include "voxel_table.h"
#include "wave_block.h"

#include <stdint.h>

namespace {

using namespace voxel_table;
using wave_block::block_count;
using wave_block::block_exclusive_scan;

constexpr int kCursorAt = 4;            // word of slot 0 that holds the row cursor

__global__ __launch_bounds__(256) void cloud_clear_kernel(u64* __restrict__ table, long capacity) {
  const long s = (long)blockIdx.x * 256 + threadIdx.x;
  if (s < capacity) slot_reset(table + 8 * s);
}

// pass (a).  counters[0] += dropped points, counters[2] += points that found no slot within `capacity` probes
__global__ __launch_bounds__(256) void cloud_count_kernel(u64* __restrict__ table, u64 mask,
                                                          const float* __restrict__ points, long n, float inv_cell,
                                                          u64* __restrict__ counters) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  bool dropped = false, lost = false;
  if (i < n) {
    u64 key;
    if (point_key(points + 3 * i, inv_cell, key)) {
      bool fresh;
      const long h = slot_claim<8>(table, mask, mask, key, fresh);
      lost = h < 0;
      if (!lost) atomicAdd(table + 8 * h + 1, 1ull);
    } else {
      dropped = true;
    }
  }
  const bool flags[2] = {dropped, lost};
  const int at[2] = {0, 2};
  block_count<2>(flags, counters, at);
}

// pass (b): one thread per slot.  counters[1] += occupied slots, counters[3] = max(count)
__global__ __launch_bounds__(256) void cloud_offsets_kernel(u64* __restrict__ table, long capacity,
                                                            u64* __restrict__ counters) {
  __shared__ u64 wave_max[4];
  __shared__ u64 block_base;
  const int tid = (int)threadIdx.x;
  const long s = (long)blockIdx.x * 256 + tid;
  const bool occupied = s < capacity && table[8 * s] != kEmpty;
  const u64 cnt = occupied ? table[8 * s + 1] : 0ull;
  u64 big = cnt;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 other = __shfl_xor(big, o, 64);
    big = other > big ? other : big;
  }
  if ((tid & 63) == 0) wave_max[tid >> 6] = big;     // read after the scan's __syncthreads()
  u64 tot;
  const u64 before = block_exclusive_scan(cnt, tot);
  if (tid == 0) {
    block_base = tot ? atomicAdd(table + kCursorAt, tot) : 0ull;
    u64 m = wave_max[0];
    for (int w = 1; w < 4; ++w) m = wave_max[w] > m ? wave_max[w] : m;
    if (m) atomicMax(counters + 3, m);
  }
  __syncthreads();
  if (occupied) table[8 * s + 2] = block_base + before;     // fill (word 3) is still the zero of the clear
  const bool flags[1] = {occupied};
  const int at1[1] = {1};
  block_count<1>(flags, counters, at1);
}

// pass (c).  A point that pass (a) dropped or lost finds no key / no slot here either and writes nothing.
__global__ __launch_bounds__(256) void cloud_scatter_kernel(u64* __restrict__ table, u64 mask,
                                                            const float* __restrict__ points, long n, float inv_cell,
                                                            uint4* __restrict__ cells) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float* p = points + 3 * i;
  u64 key;
  if (!point_key(p, inv_cell, key)) return;
  const long h = slot_find(table, mask, key);
  if (h < 0) return;
  const u64 row = table[8 * h + 2] + atomicAdd(table + 8 * h + 3, 1ull);
  if (row >= (u64)n) return;           // cannot happen: the counts of pass (a) sum to at most n
  cells[row] = make_uint4(__float_as_uint(p[0]), __float_as_uint(p[1]), __float_as_uint(p[2]), (uint32_t)i);
}

// Why the 27 cells around a query's own hold every candidate.  The caller's cell edge is 1.25 max_dist and inv_cell is
// the fp32 nearest to 1 / edge, so max_dist * inv_cell <= 0.8 (1 + 2^-23) (the division in f64 and the rounding to fp32
// each add a relative error of at most 2^-24 and 2^-53).  The entry point does not take that on trust: it refuses
// max_dist * inv_cell > 0.9.  For a row p and a query q that both pass the quantiser, per axis:
//   s_p = fl(p inv_cell), s_q = fl(q inv_cell), both in [-2^20, 2^20), where an fp32 has an ulp of at most 2^-4: each
//   product is off by at most half of that, 2^-5 (round to nearest), the two together by at most 2^-4 = 0.0625;
//   |p - q| <= sqrt(d2).  d2 is computed from exact differences of doubles with three roundings, each 2^-53 relative, so
//   a candidate (d2 <= max_dist^2) has |p - q| <= max_dist (1 + 2^-51) per axis;
//   |s_p - s_q| <= |p - q| inv_cell + 0.0625 <= 0.9 (1 + 2^-51) + 0.0625 < 1, and two numbers less than 1 apart have
//   floors that differ by at most 1.
// So a candidate lies in a cell whose index differs by at most 1 per axis from the query's; with the caller's factor
// 1.25 the margin left is 1 - 0.8 - 0.0625 = 0.1375 cells, seven orders above the error of forming inv_cell.  A
// neighbour cell whose index would leave |k| < 2^20 holds no row (the quantiser dropped such points), so skipping it
// loses nothing.  (tests/test_map_eval_gpu.py runs the search at cell indices around 1.4e5, where the fp32 product has 6
// fraction bits left, against the brute-force oracle.)
//
// counters: [0] dropped queries, [1] matched, [2] beyond, [3] distance evaluations.  n == 0: every query is beyond.
__global__ __launch_bounds__(256) void cloud_nearest_kernel(const u64* __restrict__ table, u64 mask,
                                                            const uint4* __restrict__ cells, long n, float inv_cell,
                                                            const float* __restrict__ queries, long m, double r2,
                                                            double* __restrict__ d2_out, int* __restrict__ idx_out,
                                                            u64* __restrict__ counters) {
#pragma clang fp contract(off)      // the intent; what enforces it under the library's flags is the Makefile
  __shared__ u64 wave_evals[4];
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  bool dropped = false, matched = false, beyond = false;
  u64 evals = 0;
  if (i < m) {
    const float qxf = queries[3 * i], qyf = queries[3 * i + 1], qzf = queries[3 * i + 2];
    double best = __builtin_inf();
    int best_idx = -1;
    uint32_t kx, ky, kz, u;
    if (n == 0) {
      beyond = true;
    } else if (!(quantise(qxf, inv_cell, kx, u) && quantise(qyf, inv_cell, ky, u) && quantise(qzf, inv_cell, kz, u))) {
      dropped = true;
    } else {
      const double qx = (double)qxf, qy = (double)qyf, qz = (double)qzf;
      for_each_neighbour<1, true>(kx, ky, kz, [&](int, int, int, u64 cell) __attribute__((always_inline)) {
        const long h = slot_find(table, mask, cell);
        if (h < 0) return;
        const u64 start = table[8 * h + 2], count = table[8 * h + 1];
        if (start >= (u64)n || count > (u64)n - start) return;         // a table this index build did not write
        const uint4* __restrict__ row = cells + start;
        for (u64 j = 0; j < count; ++j) {
          const uint4 p = row[j];
          const double dx = qx - (double)__uint_as_float(p.x);
          const double dy = qy - (double)__uint_as_float(p.y);
          const double dz = qz - (double)__uint_as_float(p.z);
          const double d2 = (dx * dx + dy * dy) + dz * dz;
          const int pi = (int)p.w;
          if (d2 <= r2 && (d2 < best || (d2 == best && pi < best_idx))) {
            best = d2;
            best_idx = pi;
          }
        }
        evals += count;
      });
      matched = best_idx >= 0;
      beyond = !matched;
    }
    d2_out[i] = best;
    idx_out[i] = best_idx;
  }
  evals = wave_sum_u64(evals);
  if ((threadIdx.x & 63) == 0) wave_evals[threadIdx.x >> 6] = evals;
  __syncthreads();
  if (threadIdx.x == 0) {
    const u64 tot = wave_evals[0] + wave_evals[1] + wave_evals[2] + wave_evals[3];
    if (tot) atomicAdd(counters + 3, tot);
  }
  const bool flags[3] = {dropped, matched, beyond};
  const int at[3] = {0, 1, 2};
  block_count<3>(flags, counters, at);
}

}  // namespace

extern "C" int pi3_cloud_index_build(const float* points, long n, float inv_cell, void* table, long capacity,
                                     void* cells, unsigned long long* counters, void* stream) {
  if (!table || !pow2(capacity) || !counters || n < 0 || n >= (1L << 31) || (n > 0 && (!points || !cells)) ||
      !positive_finite((double)inv_cell)) {
    pi3_set_error("pi3_cloud_index_build: bad arguments n=%ld (0 <= n < 2^31) capacity=%ld (a power of two) "
                  "inv_cell=%g (finite, > 0), or a null pointer", n, capacity, (double)inv_cell);
    return PI3_ERR_ARG;
  }
  if (pi3_zero_words("pi3_cloud_index_build", counters, 4, stream) != PI3_OK) return PI3_ERR_LAUNCH;
  hipStream_t st = (hipStream_t)stream;
  u64* t = (u64*)table;
  const u64 mask = (u64)capacity - 1;
  hipLaunchKernelGGL(cloud_clear_kernel, dim3(blocks_for(capacity)), dim3(256), 0, st, t, capacity);
  if (n > 0) {
    hipLaunchKernelGGL(cloud_count_kernel, dim3(blocks_for(n)), dim3(256), 0, st, t, mask, points, n, inv_cell,
                       (u64*)counters);
    hipLaunchKernelGGL(cloud_offsets_kernel, dim3(blocks_for(capacity)), dim3(256), 0, st, t, capacity,
                       (u64*)counters);
    hipLaunchKernelGGL(cloud_scatter_kernel, dim3(blocks_for(n)), dim3(256), 0, st, t, mask, points, n, inv_cell,
                       (uint4*)cells);
  }
  return pi3_check_launch("cloud_index_build");
}

extern "C" int pi3_cloud_nearest(const void* table, long capacity, const void* cells, long n, float inv_cell,
                                 const float* queries, long m, double max_dist, double* d2, int* idx,
                                 unsigned long long* counters, void* stream) {
  if (!table || !pow2(capacity) || !counters || n < 0 || n >= (1L << 31) || (n > 0 && !cells) || m < 0 ||
      (m > 0 && (!queries || !d2 || !idx)) || !positive_finite((double)inv_cell) || !positive_finite(max_dist) ||
      !(max_dist * (double)inv_cell <= 0.9)) {
    pi3_set_error("pi3_cloud_nearest: bad arguments n=%ld (0 <= n < 2^31) m=%ld (>= 0) capacity=%ld (a power of two) "
                  "inv_cell=%g max_dist=%g (finite, > 0, max_dist * inv_cell <= 0.9: the 27-cell search is exact only "
                  "for cells of at least 1.112 max_dist), or a null pointer", n, m, capacity, (double)inv_cell, max_dist);
    return PI3_ERR_ARG;
  }
  if (pi3_zero_words("pi3_cloud_nearest", counters, 4, stream) != PI3_OK) return PI3_ERR_LAUNCH;
  if (m > 0)
    hipLaunchKernelGGL(cloud_nearest_kernel, dim3(blocks_for(m)), dim3(256), 0, (hipStream_t)stream, (const u64*)table,
                       (u64)capacity - 1, (const uint4*)cells, n, inv_cell, queries, m, max_dist * max_dist, d2, idx,
                       (u64*)counters);
  return pi3_check_launch("cloud_nearest");
}
