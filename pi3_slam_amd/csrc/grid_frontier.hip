// Frontiers of the occupancy grid (occupancy.hip's layout: state u8 [nz][ny][nx], x fastest, cell (ix, iy, iz) at the
// linear index (iz ny + iy) nx + ix): the free cells that border unknown space, grouped into connected surfaces and
// reduced to one row of figures per surface.  Integers only; tests/grid_frontier_ref.py reproduces every output byte
// for byte.
//
//   frontier  a cell with state == 1 of whose 6 face neighbours at least one is unknown (state == 0).  A neighbour
//             outside the grid counts as unknown: the box only bounds where points and cameras were, and nothing
//             beyond it was ever voted on.  label u32 per cell: 0xFFFFFFFF for a cell that is no frontier cell.
//   pi3_grid_frontier_mark   a thread per cell: label = the cell's own linear index when it is a frontier cell.
//                            Counted: the frontier cells and their unknown faces (1..6 each).
//   pi3_grid_frontier_sweep  one sweep of minimum-label propagation over plain 26-connectivity among the labelled
//                            cells (connectivity of a surface, not motion: no corner rule), in grid_tile.h's scheme
//                            (tiles of 8 x 8 x 8 cells, each relaxed in LDS to its own fixed point; the layout and why
//                            the order of the tiles does not matter are argued there; 0xFFFFFFFF outside the grid).
//                            That argument's step (1) here: every value ever stored in a labelled cell is the linear
//                            index of a cell of the same component, its own or a value taken from a labelled neighbour,
//                            which is such an index by induction.  So the cell m with the smallest index of its
//                            component keeps label m for ever (nothing in the component is smaller), and a state in
//                            which a sweep changes nothing has label[c] <= label[n] for every pair of labelled
//                            neighbours, in both directions: label is constant on the component, and the constant is
//                            label[m] = m.  A tile without a labelled cell returns after one load per thread and writes
//                            nothing.  The loop that repeats the launch lives with the caller (frontier.py).
//   pi3_grid_frontier_roots  compacts the cells with label[c] == c (after the fixed point: one per component), in any
//                            order: a workgroup scans its flags and claims its slots with one atomic add on *count.
//   pi3_grid_frontier_stats  a thread per cell; a frontier cell finds its row by binary search of its label in
//                            roots_sorted and reduces into it.  The lanes of a wave that share the wave's first label
//                            (a frontier is coherent along x: most of them) are merged in registers first and one lane
//                            adds for them; every other lane adds for itself.  All reductions are integer sums, minima
//                            and maxima, so the atomics give the same bytes in any order.
#include "common.h"
#include "grid_tile.h"
#include "voxel_table.h"
#include "wave_block.h"

#include <stdint.h>

namespace {

using grid_tile::grid_ok;
using grid_tile::kMaxIndex;
using voxel_table::u64;
using wave_block::block_count;
using wave_block::block_exclusive_scan;
using wave_block::block_sum;

typedef long long i64;

constexpr unsigned kNone = 0xFFFFFFFFu;
constexpr int kStats = 12;              // i64 per row
constexpr i64 kMinInit = 0x7FFFFFFFFFFFFFFFll;

// the unknown face neighbours of cell i = (x, y, z); outside the grid is unknown
__device__ __forceinline__ int unknown_faces(const unsigned char* __restrict__ state, int nx, int ny, int nz, int i,
                                             int x, int y, int z) {
  const int plane = nx * ny;
  int n = 0;
  n += (x == 0 || state[i - 1] == 0) ? 1 : 0;
  n += (x == nx - 1 || state[i + 1] == 0) ? 1 : 0;
  n += (y == 0 || state[i - nx] == 0) ? 1 : 0;
  n += (y == ny - 1 || state[i + nx] == 0) ? 1 : 0;
  n += (z == 0 || state[i - plane] == 0) ? 1 : 0;
  n += (z == nz - 1 || state[i + plane] == 0) ? 1 : 0;
  return n;
}

__global__ __launch_bounds__(256) void frontier_mark_kernel(const unsigned char* __restrict__ state, int nx, int ny,
                                                            int nz, int cells, unsigned* __restrict__ label,
                                                            u64* __restrict__ counters) {
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;      // cells <= 2^27
  int faces = 0;
  if (i < cells) {
    if (state[i] == 1) {
      const int line = i / nx;
      faces = unknown_faces(state, nx, ny, nz, i, i - line * nx, line % ny, line / ny);
    }
    label[i] = faces ? (unsigned)i : kNone;
  }
  const bool flags[1] = {faces != 0};
  const int at[1] = {0};
  block_count<1>(flags, counters, at);
  block_sum((unsigned)faces, counters + 1);
}

__global__ __launch_bounds__(grid_tile::kThreads) void frontier_sweep_kernel(int nx, int ny, int nz, int tx, int ty,
                                                                             unsigned* label,
                                                                             int* __restrict__ changed) {
  __shared__ unsigned sl[grid_tile::kLds];
  const grid_tile::Tile tile(nx, ny, nz, tx, ty);
  const unsigned first = tile.own ? label[tile.g] : kNone;    // == sl[c] once staged: nobody else writes this cell's word
  const bool labelled = first != kNone;
  if (!__syncthreads_or(labelled)) return;                    // no frontier here: nothing is written
  tile.stage(sl, (const unsigned*)label, kNone);
  __syncthreads();
  const int c = tile.c;
  grid_tile::settle(tile, sl, label, first, changed, [&](unsigned best) {
    if (labelled)
      grid_tile::for_hood([&](int, int, int, int off, int) {
        const unsigned l = sl[c + off];                       // 0xFFFFFFFF where there is no label
        if (l < best) best = l;
      });
    return best;
  });
}

__global__ __launch_bounds__(256) void frontier_roots_kernel(const unsigned* __restrict__ label, int cells,
                                                             long* __restrict__ roots, long cap,
                                                             u64* __restrict__ count) {
  __shared__ u64 base;
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
  const bool root = i < cells && label[i] == (unsigned)i;
  u64 total = 0;
  const u64 before = block_exclusive_scan(root ? 1ull : 0ull, total);
  if (threadIdx.x == 0 && total) base = atomicAdd(count, total);
  __syncthreads();
  if (root) {
    const u64 slot = base + before;
    if (slot < (u64)cap) roots[slot] = (long)i;
  }
}

__global__ __launch_bounds__(256) void frontier_rows_kernel(i64* __restrict__ stats, long K) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= K * kStats) return;
  const int f = (int)(j % kStats);
  stats[j] = f < 5 ? 0 : f < 8 ? kMinInit : f < 11 ? -1 : (i64)~0ull;
}

// the row of `l` in the ascending roots_sorted, -1 when it is not there
__device__ __forceinline__ long find_row(const long* __restrict__ roots, long K, unsigned l) {
  long lo = 0, hi = K;
  while (lo < hi) {
    const long mid = (lo + hi) >> 1;
    if (roots[mid] < (long)l) lo = mid + 1; else hi = mid;
  }
  return lo < K && roots[lo] == (long)l ? lo : -1;
}

__global__ __launch_bounds__(256) void frontier_stats_kernel(const unsigned char* __restrict__ state,
                                                             const unsigned* __restrict__ label,
                                                             const unsigned* __restrict__ dist, int nx, int ny, int nz,
                                                             int cells, const long* __restrict__ roots, long K,
                                                             i64* __restrict__ stats, u64* __restrict__ counters) {
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
  const int lane = (int)(threadIdx.x & 63);
  const unsigned mine = i < cells ? label[i] : kNone;
  const bool frontier = mine != kNone;
  int x = 0, y = 0, z = 0;
  unsigned faces = 0;
  u64 key = ~0ull;
  if (frontier) {
    const int line = i / nx;
    x = i - line * nx;
    y = line % ny;
    z = line / ny;
    faces = (unsigned)unknown_faces(state, nx, ny, nz, i, x, y, z);
    if (dist) {
      const unsigned d = dist[i];
      if (d != kNone) key = ((u64)d << 27) | (u64)i;          // d < 2^32, i < 2^27
    }
  }
  const bool reach = key != ~0ull;
  bool lost = false;
  const u64 todo = __ballot(frontier);
  if (todo) {                                                 // the same in every lane of the wave
    const unsigned l0 = __shfl(mine, __ffsll((long long)todo) - 1, 64);
    const bool in = frontier && mine == l0;
    const u64 same = __ballot(in);
    const int lead = __ffsll((long long)same) - 1;
    // the lanes that share the wave's first label, merged: x, y, z < 2^21 and 64 lanes, so 32 bits hold the sums
    unsigned f = in ? faces : 0u, sx = in ? (unsigned)x : 0u, sy = in ? (unsigned)y : 0u, sz = in ? (unsigned)z : 0u;
    int lx = in ? x : kMaxIndex, ly = in ? y : kMaxIndex, lz = in ? z : kMaxIndex;
    int hx = in ? x : -1, hy = in ? y : -1, hz = in ? z : -1;
    u64 k = in ? key : ~0ull;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      f += __shfl_xor(f, o, 64);
      sx += __shfl_xor(sx, o, 64);
      sy += __shfl_xor(sy, o, 64);
      sz += __shfl_xor(sz, o, 64);
      lx = min(lx, __shfl_xor(lx, o, 64));
      ly = min(ly, __shfl_xor(ly, o, 64));
      lz = min(lz, __shfl_xor(lz, o, 64));
      hx = max(hx, __shfl_xor(hx, o, 64));
      hy = max(hy, __shfl_xor(hy, o, 64));
      hz = max(hz, __shfl_xor(hz, o, 64));
      const u64 ok = __shfl_xor(k, o, 64);
      k = ok < k ? ok : k;
    }
    unsigned n = (unsigned)__popcll(same);
    if (frontier && !in) {                                    // a lane of another label adds for itself
      n = 1u;
      f = faces;
      sx = (unsigned)x, sy = (unsigned)y, sz = (unsigned)z;
      lx = hx = x, ly = hy = y, lz = hz = z;
      k = key;
    }
    if (frontier && (!in || lane == lead)) {
      const long row = find_row(roots, K, mine);
      if (row < 0) {
        lost = true;
      } else {
        i64* r = stats + row * kStats;
        atomicAdd((u64*)r + 0, (u64)n);
        atomicAdd((u64*)r + 1, (u64)f);
        atomicAdd((u64*)r + 2, (u64)sx);
        atomicAdd((u64*)r + 3, (u64)sy);
        atomicAdd((u64*)r + 4, (u64)sz);
        atomicMin(r + 5, (i64)lx);
        atomicMin(r + 6, (i64)ly);
        atomicMin(r + 7, (i64)lz);
        atomicMax(r + 8, (i64)hx);
        atomicMax(r + 9, (i64)hy);
        atomicMax(r + 10, (i64)hz);
        if (k != ~0ull) atomicMin((u64*)r + 11, k);
      }
    }
    const bool lead_lost = __shfl((int)lost, lead, 64) != 0;  // the merged lanes share their leader's fate
    if (in) lost = lead_lost;
  }
  const bool flags[3] = {frontier && !lost, lost, reach};
  const int at[3] = {0, 1, 2};
  block_count<3>(flags, counters, at);
}

}  // namespace

extern "C" int pi3_grid_frontier_mark(const unsigned char* state, int nx, int ny, int nz, unsigned* label,
                                      unsigned long long* counters, void* stream) {
  long cells = 0;
  if (!state || !label || !counters || !grid_ok(nx, ny, nz, cells)) {
    pi3_set_error("pi3_grid_frontier_mark: bad arguments dims=(%d, %d, %d) (1 .. 2^21 - 1 each, at most 2^27 cells), or "
                  "a null pointer", nx, ny, nz);
    return PI3_ERR_ARG;
  }
  if (pi3_zero_words("pi3_grid_frontier_mark", counters, 4, stream) != PI3_OK) return PI3_ERR_LAUNCH;
  hipLaunchKernelGGL(frontier_mark_kernel, dim3(voxel_table::blocks_for(cells)), dim3(256), 0, (hipStream_t)stream,
                     state, nx, ny, nz, (int)cells, label, (u64*)counters);
  return pi3_check_launch("grid_frontier_mark");
}

extern "C" int pi3_grid_frontier_sweep(int nx, int ny, int nz, unsigned* label, int* changed, void* stream) {
  long cells = 0;
  if (!label || !changed || !grid_ok(nx, ny, nz, cells)) {
    pi3_set_error("pi3_grid_frontier_sweep: bad arguments dims=(%d, %d, %d) (1 .. 2^21 - 1 each, at most 2^27 cells), "
                  "or a null pointer", nx, ny, nz);
    return PI3_ERR_ARG;
  }
  int tx, ty;
  const unsigned tiles = grid_tile::tiles(nx, ny, nz, tx, ty);
  hipLaunchKernelGGL(frontier_sweep_kernel, dim3(tiles), dim3(grid_tile::kThreads), 0, (hipStream_t)stream, nx, ny, nz,
                     tx, ty, label, changed);
  return pi3_check_launch("grid_frontier_sweep");
}

extern "C" int pi3_grid_frontier_roots(const unsigned* label, int nx, int ny, int nz, long* roots, long cap,
                                       long* count, void* stream) {
  long cells = 0;
  if (!label || !count || !grid_ok(nx, ny, nz, cells) || cap < 0 || (cap > 0 && !roots)) {
    pi3_set_error("pi3_grid_frontier_roots: bad arguments dims=(%d, %d, %d) (1 .. 2^21 - 1 each, at most 2^27 cells) "
                  "cap=%ld (>= 0; roots may be NULL at 0), or a null pointer", nx, ny, nz, cap);
    return PI3_ERR_ARG;
  }
  if (pi3_zero_words("pi3_grid_frontier_roots", count, 1, stream) != PI3_OK) return PI3_ERR_LAUNCH;
  hipLaunchKernelGGL(frontier_roots_kernel, dim3(voxel_table::blocks_for(cells)), dim3(256), 0, (hipStream_t)stream,
                     label, (int)cells, roots, cap, (u64*)count);
  return pi3_check_launch("grid_frontier_roots");
}

extern "C" int pi3_grid_frontier_stats(const unsigned char* state, const unsigned* label, const unsigned* dist, int nx,
                                       int ny, int nz, const long* roots_sorted, long K, long* stats,
                                       unsigned long long* counters, void* stream) {
  long cells = 0;
  if (!state || !label || !counters || !grid_ok(nx, ny, nz, cells) || K < 0 || K > cells ||
      (K > 0 && (!roots_sorted || !stats))) {
    pi3_set_error("pi3_grid_frontier_stats: bad arguments dims=(%d, %d, %d) (1 .. 2^21 - 1 each, at most 2^27 cells) "
                  "K=%ld (0 .. cells; roots_sorted and stats may be NULL at 0), or a null pointer", nx, ny, nz, K);
    return PI3_ERR_ARG;
  }
  static_assert(sizeof(long) == sizeof(i64), "stats rows are int64");
  if (pi3_zero_words("pi3_grid_frontier_stats", counters, 4, stream) != PI3_OK) return PI3_ERR_LAUNCH;
  if (K == 0) return PI3_OK;                  // no cluster: no kernel
  hipLaunchKernelGGL(frontier_rows_kernel, dim3(voxel_table::blocks_for(K * kStats)), dim3(256), 0, (hipStream_t)stream,
                     (i64*)stats, K);
  hipLaunchKernelGGL(frontier_stats_kernel, dim3(voxel_table::blocks_for(cells)), dim3(256), 0, (hipStream_t)stream,
                     state, label, dist, nx, ny, nz, (int)cells, roots_sorted, K, (i64*)stats, (u64*)counters);
  return pi3_check_launch("grid_frontier_stats");
}
