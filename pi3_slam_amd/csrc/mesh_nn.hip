// Exact radius-bounded nearest TRIANGLE of a mesh for a set of query points, through the uniform cell grid of
// cloud_nn.hip: the point-to-surface distance of map_eval.py when the target side of a comparison is a mesh.
//
// The grid is cloud_nn.hip's: a hash table of cells in the voxel table's form (voxel_table.h: quantiser, 21-bit key
// packing, slot_claim / slot_find, for_each_neighbour; 64-byte slots)
//   slot (8 x uint64)  key | count | start | fill | cursor (slot 0 only) | 3 spare
//   rows               int32 face indices grouped by cell: the triangles of the cell in a slot are
//                      rows[start .. start + count)
//   packed             f32 [F][12], caller-owned: a (3), b (3), c (3), 2 spare, and in the twelfth word the face index
//                      (int32; -1 = dropped).  Written once by the count call; the query reads a candidate as three
//                      16-byte loads.
// A triangle is DROPPED (counted, never indexed, never returned) when a vertex index is outside [0, V), a vertex is not
// finite or falls outside the quantiser's |k| < 2^20 on an axis, or n2 = 0 with, in f64, every operation rounded on its
// own (the Makefile compiles this file with -ffp-contract=off),
//   ab = b - a, ac = c - a;  nx = ab.y ac.z - ab.z ac.y,  ny = ab.z ac.x - ab.x ac.z,  nz = ab.x ac.y - ab.y ac.x;
//   n2 = (nx nx + ny ny) + nz nz.
//
// Index build.  A triangle gets a row in EVERY cell of its axis-aligned bounding box: per axis from the quantised
// minimum to the quantised maximum of its three fp32 coordinates (the quantiser is monotone, so these are the smallest
// and largest of the three quantised indices).  How many rows that makes is not known in advance, so the build is two
// calls with the host between them:
//   pi3_mesh_index_count   clear; (p) one thread per triangle validates, packs, and adds the number of cells of its box
//                          to counters[4] (a box of 2^32 cells or more counts as 2^32: the sum cannot wrap, and any such
//                          total is above every allowed max_rows); (a) every (triangle, cell) pair finds or claims the
//                          cell's slot and adds 1 to its count; the claims are counted (counters[1], the cells), so
//                          the host can tell a table that is too full to be searched quickly from one that is not.
//                          (a) starts by reading counters[4], which (p) finished: above max_rows it does nothing, so
//                          a mesh that cannot be indexed costs no table walk.
//   (host)                 reads counters[4], allocates rows
//   pi3_mesh_index_fill    (b) every occupied slot claims `count` rows: exclusive scan over the workgroup, ONE atomic per
//                          workgroup on the cursor; (c) every (triangle, cell) pair finds its slot again and writes its
//                          face index at start + atomicAdd(fill, 1).
// (a) and (c) enumerate a triangle's cells through the one function for_each_cell_of_triangles below, from the same
// packed words and the same inv_cell, so they meet the same cells.  The split of that work: a triangle of up to
// kLaneCells = 64 cells is walked by its own lane; larger ones are then taken one after the other by the whole wave,
// lane l visiting cells l, l + 64, ...  A wall of a room is thousands of cells (a 40^3 box 64 000); on one lane the
// other 63 would wait that long, while the wave form keeps all of them claiming slots and finishes a box in cells / 64
// steps.  Below 64 cells the wave form would idle lanes and a lane's own loop is no longer than one wave step per cell.
// There is no tighter cell test than the box: every cell of the box gets the row.
//
// Query (pi3_mesh_nearest): one thread per query point p (fp32, used as f64).  It visits the 27 cells around its own and
// for every row evaluates the closest point of the triangle (a, b, c) by the recipe of Ericson, Real-Time Collision
// Detection, 5.1.5, in f64, every operation rounded on its own, dot(u, v) = (u.x v.x + u.y v.y) + u.z v.z, vectors
// component by component, the tests in this order and the first that holds decides:
//   ab = b - a, ac = c - a, ap = p - a;  d1 = dot(ab, ap), d2 = dot(ac, ap)
//   A    d1 <= 0 and d2 <= 0                         q = a
//   bp = p - b;  d3 = dot(ab, bp), d4 = dot(ac, bp)
//   B    d3 >= 0 and d4 <= d3                        q = b
//   vc = d1 d4 - d3 d2
//   AB   vc <= 0 and d1 >= 0 and d3 <= 0             v = d1 / (d1 - d3);  q = a + ab v
//   cp = p - c;  d5 = dot(ab, cp), d6 = dot(ac, cp)
//   C    d6 >= 0 and d5 <= d6                        q = c
//   vb = d5 d2 - d1 d6
//   AC   vb <= 0 and d2 >= 0 and d6 <= 0             w = d2 / (d2 - d6);  q = a + ac w
//   va = d3 d6 - d5 d4;  s = d4 - d3, t = d5 - d6
//   BC   va <= 0 and s >= 0 and t >= 0               w = s / (s + t);     q = b + (c - b) w
//   interior                                         k = 1 / ((va + vb) + vc);  v = vb k, w = vc k;  q = (a + ab v) + ac w
//   e = p - q;  dist2 = (e.x e.x + e.y e.y) + e.z e.z
// A triangle is a candidate when dist2 <= max_dist max_dist (the product formed once, in f64); a dist2 that is not finite
// fails that test.  Result: the candidate with the smallest dist2, among equal dist2 the smallest face index, so the
// row order and a triangle met in several of the 27 cells do not matter: bitwise reproducible, and what
// tests/mesh_eval_ref.py computes by brute force.  Written per query: dist2 (f64), the face (int32) and q rounded to
// fp32.  No candidate, or a dropped query (not finite / outside the quantiser): +inf, -1, (0, 0, 0).  NaN is written
// nowhere.  Without any triangle (F == 0) every query is beyond, none dropped.
#include "common.h"
#include "voxel_table.h"
#include "wave_block.h"

#include <stdint.h>

namespace {

using namespace voxel_table;
using wave_block::block_count;
using wave_block::block_exclusive_scan;

constexpr int kCursorAt = 4;                 // word of slot 0 that holds the row cursor
constexpr uint32_t kLaneCells = 64;          // boxes up to this many cells stay on their lane
constexpr u64 kCellsCap = 1ull << 32;        // what one box adds to the row total at most
constexpr int kRowsAt = 4;                   // counters[4]: the row total

// *counter += the workgroup's sum of v: wave reduce, LDS, one atomic.  Every thread of the workgroup calls it; a kernel
// that calls it twice puts a __syncthreads() between the calls (wave_block.h's contract).
__device__ __forceinline__ void block_sum_u64(u64 v, u64* __restrict__ counter) {
  __shared__ u64 wave_v[4];
  v = wave_sum_u64(v);
  if ((threadIdx.x & 63) == 0) wave_v[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    const u64 tot = wave_v[0] + wave_v[1] + wave_v[2] + wave_v[3];
    if (tot) atomicAdd(counter, tot);
  }
}

// The box of the cells of a triangle given as 9 fp32 coordinates (a, b, c): lo = the biased index of the first cell per
// axis, n = the number of cells per axis.  false when a coordinate does not pass the quantiser.
__device__ __forceinline__ bool triangle_box(const float (&t)[9], float inv_cell, uint32_t (&lo)[3], uint32_t (&n)[3]) {
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    uint32_t k0 = 0, k1 = 0, k2 = 0, u;
    ok = quantise(t[a], inv_cell, k0, u) && ok;
    ok = quantise(t[3 + a], inv_cell, k1, u) && ok;
    ok = quantise(t[6 + a], inv_cell, k2, u) && ok;
    const uint32_t mn = min(k0, min(k1, k2)), mx = max(k0, max(k1, k2));
    lo[a] = mn;
    n[a] = mx - mn + 1;
  }
  return ok;
}

// the same from the packed words of face f; false for a face the count call dropped (or f >= F)
__device__ __forceinline__ bool packed_box(const float4* __restrict__ packed, long f, long F, float inv_cell,
                                           uint32_t (&lo)[3], uint32_t (&n)[3]) {
  if (f >= F) return false;
  const float4 p0 = packed[3 * f], p1 = packed[3 * f + 1], p2 = packed[3 * f + 2];
  if (__float_as_int(p2.w) != (int)f) return false;
  const float t[9] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w, p2.x};
  return triangle_box(t, inv_cell, lo, n);
}

// The ONE enumeration of (triangle, cell) pairs, used by the count pass and by the fill pass.  Every lane of a wave
// calls it with its own triangle (`valid`, face index `tri`, box lo / n); visit(key of the cell, face index) runs once
// for every cell of every valid box whose cell count is at most `limit` (< 2^31: the cell counter is 32 bits).  Boxes of
// up to kLaneCells cells are walked by their lane, the larger ones by the whole wave, one box after the other in lane
// order.  Which lane visits a pair differs between the two forms; which pairs are visited does not.
template <typename Visit>
__device__ __forceinline__ void for_each_cell_of_triangles(bool valid, int tri, const uint32_t (&lo)[3],
                                                           const uint32_t (&n)[3], uint32_t limit, Visit&& visit) {
  const u64 cells64 = valid ? (u64)n[0] * (u64)n[1] * (u64)n[2] : 0ull;
  const bool fits = cells64 <= (u64)limit;
  const uint32_t cells = fits ? (uint32_t)cells64 : 0u;
  const bool wide = cells > kLaneCells;
  if (!wide) {
    for (uint32_t c = 0; c < cells; ++c) {
      const uint32_t z = c % n[2], xy = c / n[2], y = xy % n[1], x = xy / n[1];
      visit(pack_key(lo[0] + x, lo[1] + y, lo[2] + z), tri);
    }
  }
  u64 todo = __ballot(wide);
  const uint32_t lane = threadIdx.x & 63;
  while (todo) {                               // uniform over the wave: every lane takes every turn
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const uint32_t lx = __shfl(lo[0], src, 64), ly = __shfl(lo[1], src, 64), lz = __shfl(lo[2], src, 64);
    const uint32_t ny = __shfl(n[1], src, 64), nz = __shfl(n[2], src, 64);
    const uint32_t total = __shfl(cells, src, 64);
    const int t = __shfl(tri, src, 64);
    for (uint32_t c = lane; c < total; c += 64) {
      const uint32_t z = c % nz, xy = c / nz, y = xy % ny, x = xy / ny;
      visit(pack_key(lx + x, ly + y, lz + z), t);
    }
  }
}

__global__ __launch_bounds__(256) void mesh_clear_kernel(u64* __restrict__ table, long capacity) {
  const long s = (long)blockIdx.x * 256 + threadIdx.x;
  if (s < capacity) slot_reset(table + 8 * s);
}

// pass (p): validate and pack.  counters[0] += dropped triangles, counters[4] += cells of the boxes (each capped)
__global__ __launch_bounds__(256) void mesh_pack_kernel(const float* __restrict__ vertices, long V,
                                                        const int* __restrict__ faces, long F, float inv_cell,
                                                        float4* __restrict__ packed, u64* __restrict__ counters) {
#pragma clang fp contract(off)      // the intent; what enforces it under the library's flags is the Makefile
  const long f = (long)blockIdx.x * 256 + threadIdx.x;
  bool dropped = false;
  u64 cells = 0;
  if (f < F) {
    const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    float t[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    bool ok = i0 >= 0 && i0 < V && i1 >= 0 && i1 < V && i2 >= 0 && i2 < V;
    if (ok) {
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        t[a] = vertices[3L * i0 + a];
        t[3 + a] = vertices[3L * i1 + a];
        t[6 + a] = vertices[3L * i2 + a];
      }
      uint32_t lo[3], n[3];
      ok = triangle_box(t, inv_cell, lo, n);
      if (ok) {
        const double abx = (double)t[3] - (double)t[0], aby = (double)t[4] - (double)t[1], abz = (double)t[5] - (double)t[2];
        const double acx = (double)t[6] - (double)t[0], acy = (double)t[7] - (double)t[1], acz = (double)t[8] - (double)t[2];
        const double nx = aby * acz - abz * acy, ny = abz * acx - abx * acz, nz = abx * acy - aby * acx;
        const double n2 = (nx * nx + ny * ny) + nz * nz;
        ok = n2 != 0.0;                           // finite inputs of |x| < 2^128 cannot overflow n2
        if (ok) {
          const u64 c = (u64)n[0] * (u64)n[1] * (u64)n[2];      // each factor <= 2^21: no wrap
          cells = c < kCellsCap ? c : kCellsCap;
        }
      }
    }
    dropped = !ok;
    if (dropped) {
#pragma unroll
      for (int j = 0; j < 9; ++j) t[j] = 0.0f;
    }
    packed[3 * f] = make_float4(t[0], t[1], t[2], t[3]);
    packed[3 * f + 1] = make_float4(t[4], t[5], t[6], t[7]);
    packed[3 * f + 2] = make_float4(t[8], 0.0f, 0.0f, __int_as_float(dropped ? -1 : (int)f));
  }
  block_sum_u64(cells, counters + kRowsAt);
  const bool flags[1] = {dropped};
  const int at[1] = {0};
  block_count<1>(flags, counters, at);
}

// pass (a).  counters[1] += cells (slots this pass claimed), counters[2] += (triangle, cell) pairs that found no slot
// within `capacity` probes
__global__ __launch_bounds__(256) void mesh_count_kernel(u64* __restrict__ table, u64 mask,
                                                         const float4* __restrict__ packed, long F, float inv_cell,
                                                         u64 max_rows, u64* __restrict__ counters) {
  const u64 total = counters[kRowsAt];               // pass (p) is complete: the previous launch on the stream
  u64 lost = 0, claimed = 0;
  if (total <= max_rows) {
    const long f = (long)blockIdx.x * 256 + threadIdx.x;
    uint32_t lo[3] = {0, 0, 0}, n[3] = {0, 0, 0};
    const bool valid = packed_box(packed, f, F, inv_cell, lo, n);
    for_each_cell_of_triangles(valid, (int)f, lo, n, (uint32_t)max_rows, [&](u64 key, int) {
      bool fresh;
      const long h = slot_claim<8>(table, mask, mask, key, fresh);
      if (h < 0) ++lost;
      else atomicAdd(table + 8 * h + 1, 1ull);
      claimed += fresh ? 1 : 0;
    });
  }
  block_sum_u64(lost, counters + 2);
  __syncthreads();
  block_sum_u64(claimed, counters + 1);
}

// pass (b): one thread per slot.  counters[3] = max(count)
__global__ __launch_bounds__(256) void mesh_offsets_kernel(u64* __restrict__ table, long capacity,
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
}

// pass (c).  A pair that pass (a) lost finds no slot here either and writes nothing.
__global__ __launch_bounds__(256) void mesh_scatter_kernel(u64* __restrict__ table, u64 mask,
                                                           const float4* __restrict__ packed, long F, float inv_cell,
                                                           int* __restrict__ rows, u64 n_rows) {
  const long f = (long)blockIdx.x * 256 + threadIdx.x;
  uint32_t lo[3] = {0, 0, 0}, n[3] = {0, 0, 0};
  const bool valid = packed_box(packed, f, F, inv_cell, lo, n);
  for_each_cell_of_triangles(valid, (int)f, lo, n, (uint32_t)n_rows, [&](u64 key, int tri) {
    const long h = slot_find(table, mask, key);
    if (h < 0) return;
    const u64 row = table[8 * h + 2] + atomicAdd(table + 8 * h + 3, 1ull);
    if (row < n_rows) rows[row] = tri;        // always, when n_rows is the count call's total
  });
}

// Why the 27 cells around a query's own hold every candidate.  As in cloud_nn.hip the caller's cell edge is 1.25
// max_dist, inv_cell the fp32 nearest to 1 / edge, and the entry point refuses max_dist * inv_cell > 0.9.  Take a query
// p that passes the quantiser and a triangle T with a row, and let x be the point of T closest to p.  Per axis:
//   x lies in the box of T: min <= x <= max over the three fp32 coordinates, so x inv_cell (exact) lies between
//   min inv_cell and max inv_cell, and those are within 2^-5 of s_min = fl(min inv_cell) and s_max = fl(max inv_cell)
//   (a product below 2^20 in magnitude has an fp32 ulp of at most 2^-4, round to nearest).  x' = x inv_cell clamped to
//   [s_min, s_max] therefore moves by at most 2^-5, and floor(x') is one of the box's cell indices floor(s_min) ..
//   floor(s_max).  (The same through the fp32 rounding of x, which lies in [min, max] too because rounding is monotone:
//   its product is one of the fl(.) the quantiser's monotonicity speaks of.)
//   s_p = fl(p inv_cell) is within 2^-5 of p inv_cell, and |p - x| <= dist(p, T).
//   |s_p - x'| <= dist(p, T) inv_cell + 2^-4, which for dist(p, T) <= max_dist (1 + 0.04) is below 0.9 * 1.04 + 0.0625
//   < 1: the floors differ by at most 1, so a cell of T's box is among the 27.
// With the caller's factor 1.25 the margin is 1 - 0.8 - 0.0625 = 0.1375 cells = 0.17 max_dist.  What it has to cover
// beyond the two products: the recipe's dist2 against the true squared distance.  q is a + ab v (+ ac w) with v, w from
// quotients of rounded dot products; in the vertex and edge regions 0 <= v, w <= 1 holds for the computed values (the
// tests above each quotient order numerator and denominator), so q is within a few ulp of f64 of the segment; in the
// interior v and w carry the cancellation of va, vb, vc, a relative 2^-50 times (longest edge)^2 / (2 area).  A
// candidate has |p - q| <= max_dist (1 + 2^-51), so dist(p, T) <= max_dist + dist(q, T), and the margin allows
// dist(q, T) of 0.04 max_dist even at the refusal limit: twelve orders above that error for any triangle a scan or a
// surface extraction produces (aspect up to 10^6).  A neighbour cell whose index would leave |k| < 2^20 holds no row.
//
// counters: [0] dropped queries, [1] matched, [2] beyond, [3] triangle evaluations.  F == 0: every query is beyond.
__global__ __launch_bounds__(256) void mesh_nearest_kernel(const u64* __restrict__ table, u64 mask,
                                                           const int* __restrict__ rows, u64 n_rows,
                                                           const float4* __restrict__ packed, long F, float inv_cell,
                                                           const float* __restrict__ queries, long m, double r2,
                                                           double* __restrict__ d2_out, int* __restrict__ face_out,
                                                           float* __restrict__ closest_out, u64* __restrict__ counters) {
#pragma clang fp contract(off)      // the intent; what enforces it under the library's flags is the Makefile
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  bool dropped = false, matched = false, beyond = false;
  u64 evals = 0;
  if (i < m) {
    const float pxf = queries[3 * i], pyf = queries[3 * i + 1], pzf = queries[3 * i + 2];
    double best = __builtin_inf();
    double bqx = 0.0, bqy = 0.0, bqz = 0.0;
    int best_face = -1;
    uint32_t kx, ky, kz, u;
    if (F == 0) {
      beyond = true;
    } else if (!(quantise(pxf, inv_cell, kx, u) && quantise(pyf, inv_cell, ky, u) && quantise(pzf, inv_cell, kz, u))) {
      dropped = true;
    } else {
      const double px = (double)pxf, py = (double)pyf, pz = (double)pzf;
      for_each_neighbour<1, true>(kx, ky, kz, [&](int, int, int, u64 cell) __attribute__((always_inline)) {
        const long h = slot_find(table, mask, cell);
        if (h < 0) return;
        const u64 start = table[8 * h + 2], count = table[8 * h + 1];
        if (start >= n_rows || count > n_rows - start) return;         // a table this index build did not write
        const int* __restrict__ row = rows + start;
        for (u64 j = 0; j < count; ++j) {
          const int f = row[j];
          if (f < 0 || f >= F) continue;
          const float4 p0 = packed[3L * f], p1 = packed[3L * f + 1], p2 = packed[3L * f + 2];
          const double ax = (double)p0.x, ay = (double)p0.y, az = (double)p0.z;
          const double bx = (double)p0.w, by = (double)p1.x, bz = (double)p1.y;
          const double cx = (double)p1.z, cy = (double)p1.w, cz = (double)p2.x;
          const double abx = bx - ax, aby = by - ay, abz = bz - az;
          const double acx = cx - ax, acy = cy - ay, acz = cz - az;
          const double apx = px - ax, apy = py - ay, apz = pz - az;
          const double d1 = (abx * apx + aby * apy) + abz * apz;
          const double d2 = (acx * apx + acy * apy) + acz * apz;
          double qx, qy, qz;
          if (d1 <= 0.0 && d2 <= 0.0) {
            qx = ax, qy = ay, qz = az;
          } else {
            const double bpx = px - bx, bpy = py - by, bpz = pz - bz;
            const double d3 = (abx * bpx + aby * bpy) + abz * bpz;
            const double d4 = (acx * bpx + acy * bpy) + acz * bpz;
            const double vc = d1 * d4 - d3 * d2;
            if (d3 >= 0.0 && d4 <= d3) {
              qx = bx, qy = by, qz = bz;
            } else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
              const double v = d1 / (d1 - d3);
              qx = ax + abx * v, qy = ay + aby * v, qz = az + abz * v;
            } else {
              const double cpx = px - cx, cpy = py - cy, cpz = pz - cz;
              const double d5 = (abx * cpx + aby * cpy) + abz * cpz;
              const double d6 = (acx * cpx + acy * cpy) + acz * cpz;
              const double vb = d5 * d2 - d1 * d6;
              const double va = d3 * d6 - d5 * d4;
              const double s = d4 - d3, t = d5 - d6;
              if (d6 >= 0.0 && d5 <= d6) {
                qx = cx, qy = cy, qz = cz;
              } else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
                const double w = d2 / (d2 - d6);
                qx = ax + acx * w, qy = ay + acy * w, qz = az + acz * w;
              } else if (va <= 0.0 && s >= 0.0 && t >= 0.0) {
                const double w = s / (s + t);
                qx = bx + (cx - bx) * w, qy = by + (cy - by) * w, qz = bz + (cz - bz) * w;
              } else {
                const double k = 1.0 / ((va + vb) + vc);
                const double v = vb * k, w = vc * k;
                qx = (ax + abx * v) + acx * w, qy = (ay + aby * v) + acy * w, qz = (az + abz * v) + acz * w;
              }
            }
          }
          const double ex = px - qx, ey = py - qy, ez = pz - qz;
          const double dist2 = (ex * ex + ey * ey) + ez * ez;
          if (dist2 <= r2 && (dist2 < best || (dist2 == best && f < best_face))) {
            best = dist2;
            best_face = f;
            bqx = qx, bqy = qy, bqz = qz;
          }
        }
        evals += count;
      });
      matched = best_face >= 0;
      beyond = !matched;
    }
    d2_out[i] = best;
    face_out[i] = best_face;
    closest_out[3 * i] = (float)bqx;
    closest_out[3 * i + 1] = (float)bqy;
    closest_out[3 * i + 2] = (float)bqz;
  }
  block_sum_u64(evals, counters + 3);
  const bool flags[3] = {dropped, matched, beyond};
  const int at[3] = {0, 1, 2};
  block_count<3>(flags, counters, at);
}

constexpr long kMaxRows = (1L << 31) - 1;

}  // namespace

extern "C" int pi3_mesh_index_count(const float* vertices, long V, const int* faces, long F, float inv_cell,
                                    void* table, long capacity, float* packed, long max_rows,
                                    unsigned long long* counters, void* stream) {
  if (!table || !pow2(capacity) || !counters || V < 0 || V >= (1L << 31) || F < 0 || F >= (1L << 31) ||
      (F > 0 && (!faces || !packed)) || (V > 0 && !vertices) || max_rows < 1 || max_rows > kMaxRows ||
      !positive_finite((double)inv_cell)) {
    pi3_set_error("pi3_mesh_index_count: bad arguments V=%ld F=%ld (0 <= V, F < 2^31) capacity=%ld (a power of two) "
                  "max_rows=%ld (1 .. 2^31 - 1) inv_cell=%g (finite, > 0), or a null pointer", V, F, capacity, max_rows,
                  (double)inv_cell);
    return PI3_ERR_ARG;
  }
  if (pi3_zero_words("pi3_mesh_index_count", counters, 8, stream) != PI3_OK) return PI3_ERR_LAUNCH;
  hipStream_t st = (hipStream_t)stream;
  u64* t = (u64*)table;
  hipLaunchKernelGGL(mesh_clear_kernel, dim3(blocks_for(capacity)), dim3(256), 0, st, t, capacity);
  if (F > 0) {
    hipLaunchKernelGGL(mesh_pack_kernel, dim3(blocks_for(F)), dim3(256), 0, st, vertices, V, faces, F, inv_cell,
                       (float4*)packed, (u64*)counters);
    hipLaunchKernelGGL(mesh_count_kernel, dim3(blocks_for(F)), dim3(256), 0, st, t, (u64)capacity - 1,
                       (const float4*)packed, F, inv_cell, (u64)max_rows, (u64*)counters);
  }
  return pi3_check_launch("mesh_index_count");
}

extern "C" int pi3_mesh_index_fill(void* table, long capacity, const float* packed, long F, float inv_cell, int* rows,
                                   long n_rows, unsigned long long* counters, void* stream) {
  if (!table || !pow2(capacity) || !counters || F < 0 || F >= (1L << 31) || (F > 0 && !packed) || n_rows < 0 ||
      n_rows > kMaxRows || (n_rows > 0 && !rows) || !positive_finite((double)inv_cell)) {
    pi3_set_error("pi3_mesh_index_fill: bad arguments F=%ld (0 <= F < 2^31) capacity=%ld (a power of two) n_rows=%ld "
                  "(0 .. 2^31 - 1) inv_cell=%g (finite, > 0), or a null pointer", F, capacity, n_rows, (double)inv_cell);
    return PI3_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  u64* t = (u64*)table;
  if (F > 0 && n_rows > 0) {
    hipLaunchKernelGGL(mesh_offsets_kernel, dim3(blocks_for(capacity)), dim3(256), 0, st, t, capacity, (u64*)counters);
    hipLaunchKernelGGL(mesh_scatter_kernel, dim3(blocks_for(F)), dim3(256), 0, st, t, (u64)capacity - 1,
                       (const float4*)packed, F, inv_cell, rows, (u64)n_rows);
  }
  return pi3_check_launch("mesh_index_fill");
}

extern "C" int pi3_mesh_nearest(const void* table, long capacity, const int* rows, long n_rows, const float* packed,
                                long F, float inv_cell, const float* queries, long m, double max_dist, double* d2,
                                int* face, float* closest, unsigned long long* counters, void* stream) {
  if (!table || !pow2(capacity) || !counters || F < 0 || F >= (1L << 31) || (F > 0 && !packed) || n_rows < 0 ||
      n_rows > kMaxRows || (n_rows > 0 && !rows) || m < 0 || (m > 0 && (!queries || !d2 || !face || !closest)) ||
      !positive_finite((double)inv_cell) || !positive_finite(max_dist) || !(max_dist * (double)inv_cell <= 0.9)) {
    pi3_set_error("pi3_mesh_nearest: bad arguments F=%ld (0 <= F < 2^31) n_rows=%ld (0 .. 2^31 - 1) m=%ld (>= 0) "
                  "capacity=%ld (a power of two) inv_cell=%g max_dist=%g (finite, > 0, max_dist * inv_cell <= 0.9: the "
                  "27-cell search is exact only for cells of at least 1.112 max_dist), or a null pointer", F, n_rows, m,
                  capacity, (double)inv_cell, max_dist);
    return PI3_ERR_ARG;
  }
  if (pi3_zero_words("pi3_mesh_nearest", counters, 4, stream) != PI3_OK) return PI3_ERR_LAUNCH;
  if (m > 0)
    hipLaunchKernelGGL(mesh_nearest_kernel, dim3(blocks_for(m)), dim3(256), 0, (hipStream_t)stream, (const u64*)table,
                       (u64)capacity - 1, rows, (u64)n_rows, (const float4*)packed, F, inv_cell, queries, m,
                       max_dist * max_dist, d2, face, closest, (u64*)counters);
  return pi3_check_launch("mesh_nearest");
}
