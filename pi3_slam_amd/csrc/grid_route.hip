// Routes through the occupancy grid (occupancy.hip's layout: state u8 [nz][ny][nx], x fastest, cell (ix, iy, iz) at the
// linear index (iz ny + iy) nx + ix): which cells a body can reach from a set of source cells, at what cost, and the
// cheapest way back from a goal.  Integers only; tests/grid_route_ref.py reproduces every output byte for byte.
//
//   graph   walk u8 per cell: 1 = traversable.  The 26 moves d in {-1, 0, 1}^3 \ {0} cost 12, 17, 21 for one, two, three
//           non-zero components (12 (1, sqrt 2, sqrt 3) rounded: +0.17 % / +1.04 %).  A move c -> c + d is allowed only
//           when every cell c + (a dx, b dy, e dz), a, b, e in {0, 1}, lies inside the grid and is traversable (2, 4 or
//           8 cells: no corner is cut).  The rule is symmetric, so the graph is undirected.  dist u32 per cell = the
//           cheapest move sequence from any source, 0xFFFFFFFF when there is none; at most 2^27 cells, so that the
//           longest simple path, 21 (cells - 1), stays below the far mark.
//   pi3_grid_route_init   a thread per cell: walk = (state == 1, or state != 2 with through_unknown) and, with a
//                         clearance field, d2 >= min_d2 (the field's far mark 0xFFFF passes); dist = far.  Then a thread
//                         per source: a linear index outside [0, cells) is counted as outside, one on a cell that is
//                         not traversable as such, every other gets dist = 0 (duplicates store the same word).
//   pi3_grid_route_sweep  one relaxation sweep in grid_tile.h's scheme (tiles of 8 x 8 x 8 cells, each relaxed in LDS to
//                         its own fixed point; the layout and why the order of the tiles does not matter are argued
//                         there).  Besides dist the tile's walk bytes are staged (outside the grid is not traversable),
//                         and every thread folds the 27 around its cell into the mask of its allowed moves once.  That
//                         argument's step (1) here: every value ever stored is the cost of a real move sequence from a
//                         source, a source's 0 or an allowed move added to such a value.  So no value ever drops below
//                         the shortest distance, and a state in which a sweep changes nothing satisfies
//                         dist[c] <= dist[n] + w for every allowed move: it is the unique shortest-distance field.  A
//                         tile with no traversable cell returns before it touches dist.  The loop that repeats the
//                         launch until a sweep changes nothing lives with the caller (grid_route.py).
//   pi3_grid_route_trace  one wave walks from the goal back to a source.  Lanes 0..25 each test one neighbour n, in the
//                         order of (dz, dy, dx): the move is allowed and dist[n] + w == dist[cur].  Inside the grid
//                         that order is the order of the linear indices, so the lowest qualifying lane holds the
//                         smallest index: one ballot.  dist falls by at least 12 per step, so the walk ends.  Two
//                         passes, the first only counts: a path that does not fit leaves `path` untouched.
#include "common.h"
#include "grid_tile.h"
#include "voxel_table.h"
#include "wave_block.h"

#include <stdint.h>

namespace {

using grid_tile::grid_ok;
using grid_tile::kLds;
using grid_tile::kPlane;
using grid_tile::kRow;
using voxel_table::u64;
using wave_block::block_count;

constexpr unsigned kFar = 0xFFFFFFFFu;
constexpr int kD2Far = 0xFFFF;
constexpr int kMaxMinD2 = 255 * 255;    // the clearance field's largest finite value

__host__ __device__ constexpr int move_cost(int dx, int dy, int dz) {
  const int n = (dx != 0) + (dy != 0) + (dz != 0);
  return n == 1 ? 12 : n == 2 ? 17 : 21;
}
// bit of the cell at offset (dx, dy, dz) in the 27-bit mask of a cell's 3 x 3 x 3 neighbourhood
__host__ __device__ constexpr unsigned hood_bit(int dx, int dy, int dz) {
  return 1u << ((dz + 1) * 9 + (dy + 1) * 3 + (dx + 1));
}
// the cells a move (dx, dy, dz) needs traversable: c + (a dx, b dy, e dz), a, b, e in {0, 1}
__host__ __device__ constexpr unsigned move_needs(int dx, int dy, int dz) {
  unsigned m = 0;
  for (int e = 0; e <= (dz != 0); ++e)
    for (int b = 0; b <= (dy != 0); ++b)
      for (int a = 0; a <= (dx != 0); ++a) m |= hood_bit(a * dx, b * dy, e * dz);
  return m;
}

__global__ __launch_bounds__(256) void route_init_kernel(const unsigned char* __restrict__ state,
                                                         const unsigned short* __restrict__ d2, int min_d2,
                                                         int through_unknown, int cells,
                                                         unsigned char* __restrict__ walk, unsigned* __restrict__ dist,
                                                         u64* __restrict__ counters) {
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;      // cells <= 2^27
  bool open = false;
  if (i < cells) {
    const unsigned char s = state[i];
    open = through_unknown ? s != 2 : s == 1;
    if (d2) open = open && (int)d2[i] >= min_d2;
    walk[i] = open ? 1 : 0;
    dist[i] = kFar;
  }
  const bool flags[1] = {open};
  const int at[1] = {0};
  block_count<1>(flags, counters, at);
}

__global__ __launch_bounds__(256) void route_sources_kernel(const long* __restrict__ sources, long Ns, int cells,
                                                            const unsigned char* __restrict__ walk,
                                                            unsigned* __restrict__ dist, u64* __restrict__ counters) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  bool accepted = false, blocked = false, outside = false;
  if (j < Ns) {
    const long s = sources[j];
    if (s < 0 || s >= (long)cells) {
      outside = true;
    } else if (!walk[s]) {
      blocked = true;
    } else {
      dist[s] = 0u;
      accepted = true;
    }
  }
  const bool flags[3] = {accepted, blocked, outside};
  const int at[3] = {1, 2, 3};
  block_count<3>(flags, counters, at);
}

__global__ __launch_bounds__(grid_tile::kThreads) void route_sweep_kernel(const unsigned char* __restrict__ walk, int nx,
                                                                          int ny, int nz, int tx, int ty, unsigned* dist,
                                                                          int* __restrict__ changed) {
  __shared__ unsigned sd[kLds];
  __shared__ unsigned char sw[kLds];
  const grid_tile::Tile tile(nx, ny, nz, tx, ty);
  const int c = tile.c;
  tile.stage(sw, walk, (unsigned char)0);
  __syncthreads();
  const bool open = sw[c] != 0;                               // 0 outside the grid: `own` is implied
  if (!__syncthreads_or(open)) return;                        // nothing to relax here: dist is not touched
  tile.stage(sd, (const unsigned*)dist, kFar);
  // the allowed moves of this cell: the 27 walk bytes around it, once
  unsigned moves = 0;
  if (open) {
    unsigned hood = 0;
#pragma unroll
    for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx)
          if (sw[c + dz * kPlane + dy * kRow + dx]) hood |= hood_bit(dx, dy, dz);
    // for_hood's walk and numbering, written out: as a lambda here the compiler waits for the 27 byte reads above in
    // batches of 8 instead of issuing them together (24 for 43 VGPRs, and a sweep measured 1 % slower)
    int k = 0;
#pragma unroll
    for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          if (dx == 0 && dy == 0 && dz == 0) continue;
          const unsigned need = move_needs(dx, dy, dz);
          if ((hood & need) == need) moves |= 1u << k;
          ++k;
        }
  }
  __syncthreads();
  grid_tile::settle(tile, sd, dist, sd[c], changed, [&](unsigned best) {
    grid_tile::for_hood([&](int dx, int dy, int dz, int off, int k) {
      if (moves & (1u << k)) {
        const unsigned d = sd[c + off];
        const unsigned cand = d + (unsigned)move_cost(dx, dy, dz);
        if (d != kFar && cand < best) best = cand;            // far + w would wrap
      }
    });
    return best;
  });
}

__global__ __launch_bounds__(64) void route_trace_kernel(const unsigned char* __restrict__ walk,
                                                         const unsigned* __restrict__ dist, int nx, int ny, int nz,
                                                         int goal, long* __restrict__ path, long cap,
                                                         long* __restrict__ length) {
  const int lane = (int)threadIdx.x;
  const int k = lane < 13 ? lane : lane + 1;                  // the 27 offsets in (dz, dy, dx) order without the centre
  const int dx = k % 3 - 1, dy = (k / 3) % 3 - 1, dz = k / 9 - 1;
  const unsigned w = (unsigned)move_cost(dx, dy, dz);
  const unsigned d_goal = dist[goal];
  if (!walk[goal] || d_goal == kFar) {
    if (lane == 0) *length = 0;
    return;
  }
  for (int pass = 0; pass < 2; ++pass) {
    int cur = goal;
    unsigned dcur = d_goal;
    long n = 1;
    if (pass && lane == 0) path[0] = goal;
    while (dcur != 0u) {
      const int line = cur / nx;
      const int cx = cur - line * nx, cy = line % ny, cz = line / ny;
      const int ax = cx + dx, ay = cy + dy, az = cz + dz;
      bool ok = lane < 26 && ax >= 0 && ax < nx && ay >= 0 && ay < ny && az >= 0 && az < nz;
      int at = 0;
      unsigned dn = kFar;
      if (ok) {                                               // the cells between lie inside when the far one does
        for (int e = 0; e <= (dz != 0); ++e)
          for (int b = 0; b <= (dy != 0); ++b)
            for (int a = 0; a <= (dx != 0); ++a)
              ok = ok && walk[((cz + e * dz) * ny + (cy + b * dy)) * nx + (cx + a * dx)] != 0;
        at = (az * ny + ay) * nx + ax;
        dn = dist[at];
        ok = ok && dn != kFar && dn + w == dcur;
      }
      const unsigned long long who = __ballot(ok);
      if (!who) {                                             // dist is no fixed point of the sweep: no path
        if (lane == 0) *length = 0;
        return;
      }
      const int src = __ffsll((long long)who) - 1;
      cur = __shfl(at, src, 64);
      dcur = __shfl(dn, src, 64);                             // < the previous dcur: the walk ends
      if (pass && lane == 0) path[n] = cur;
      ++n;
    }
    if (!pass && n > cap) {
      if (lane == 0) *length = -n;
      return;
    }
    if (pass && lane == 0) *length = n;
  }
}

}  // namespace

extern "C" int pi3_grid_route_init(const unsigned char* state, const unsigned short* d2, int min_d2, int through_unknown,
                                   int nx, int ny, int nz, const long* sources, long Ns, unsigned char* walk,
                                   unsigned* dist, unsigned long long* counters, void* stream) {
  long cells = 0;
  if (!state || !walk || !dist || !counters || !grid_ok(nx, ny, nz, cells) || min_d2 < 0 || min_d2 > kMaxMinD2 ||
      (min_d2 > 0 && !d2) || Ns < 0 || Ns >= (1L << 39) || (Ns > 0 && !sources)) {
    pi3_set_error("pi3_grid_route_init: bad arguments dims=(%d, %d, %d) (1 .. 2^21 - 1 each, at most 2^27 cells) "
                  "min_d2=%d (0 .. %d, 0 without d2) Ns=%ld (0 .. 2^39 - 1), or a null pointer", nx, ny, nz, min_d2,
                  kMaxMinD2, Ns);
    return PI3_ERR_ARG;
  }
  static_assert(kD2Far > kMaxMinD2, "the clearance field's far mark passes every min_d2");
  if (pi3_zero_words("pi3_grid_route_init", counters, 4, stream) != PI3_OK) return PI3_ERR_LAUNCH;
  hipLaunchKernelGGL(route_init_kernel, dim3(voxel_table::blocks_for(cells)), dim3(256), 0, (hipStream_t)stream, state,
                     d2, min_d2, through_unknown ? 1 : 0, (int)cells, walk, dist, (u64*)counters);
  if (Ns > 0)
    hipLaunchKernelGGL(route_sources_kernel, dim3(voxel_table::blocks_for(Ns)), dim3(256), 0, (hipStream_t)stream,
                       sources, Ns, (int)cells, (const unsigned char*)walk, dist, (u64*)counters);
  return pi3_check_launch("grid_route_init");
}

extern "C" int pi3_grid_route_sweep(const unsigned char* walk, int nx, int ny, int nz, unsigned* dist, int* changed,
                                    void* stream) {
  long cells = 0;
  if (!walk || !dist || !changed || !grid_ok(nx, ny, nz, cells)) {
    pi3_set_error("pi3_grid_route_sweep: bad arguments dims=(%d, %d, %d) (1 .. 2^21 - 1 each, at most 2^27 cells), or "
                  "a null pointer", nx, ny, nz);
    return PI3_ERR_ARG;
  }
  int tx, ty;
  const unsigned tiles = grid_tile::tiles(nx, ny, nz, tx, ty);
  hipLaunchKernelGGL(route_sweep_kernel, dim3(tiles), dim3(grid_tile::kThreads), 0, (hipStream_t)stream, walk, nx, ny,
                     nz, tx, ty, dist, changed);
  return pi3_check_launch("grid_route_sweep");
}

extern "C" int pi3_grid_route_trace(const unsigned char* walk, const unsigned* dist, int nx, int ny, int nz, long goal,
                                    long* path, long cap, long* length, void* stream) {
  long cells = 0;
  if (!walk || !dist || !path || !length || !grid_ok(nx, ny, nz, cells) || goal < 0 || goal >= cells || cap < 1) {
    pi3_set_error("pi3_grid_route_trace: bad arguments dims=(%d, %d, %d) (1 .. 2^21 - 1 each, at most 2^27 cells) "
                  "goal=%ld (0 .. cells - 1) cap=%ld (>= 1), or a null pointer", nx, ny, nz, goal, cap);
    return PI3_ERR_ARG;
  }
  hipLaunchKernelGGL(route_trace_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, walk, dist, nx, ny, nz, (int)goal,
                     path, cap, length);
  return pi3_check_launch("grid_route_trace");
}
