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
//   pi3_grid_route_init_stand  the same for a body that stands (grid_stand.hip's height u8 per cell): walk also needs
//                         h_lo <= height <= h_hi, and counters[4] counts the cells that only the band closed.
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
//
// Several fields over one walk (the tour of the views, view_tour.py): dist u32 [K][cells], field f from sources[f] alone.
// They live in this file, not in a header of shared pieces: move_cost, hood_bit, move_needs, the fold of a cell's
// allowed moves, the relaxation step and the trace walk are each written once here, as __device__ functions that the
// single-field and the batched kernels both call.
//   pi3_grid_route_fields_init  a thread per word sets every field far, then a thread per field applies the source
//                               rule above to sources[f] and field f; a field whose source is refused stays all far.
//   pi3_grid_route_sweep_many   one workgroup per (tile, group of `group` entries of `active`): the tile's walk bytes
//                               are staged and every thread's moves mask folded ONCE, then field after field of the
//                               group is staged into the same LDS block, relaxed by settle and written back.  A field
//                               whose staged block (tile and halo) holds no finite value is skipped before the
//                               relaxation: nothing can get lower there.  Fields share nothing but walk, so the
//                               argument above holds per field, and changed[f] is that field's own word.
//   pi3_grid_route_trace_many   one wave per leg l: the walk above over field field_of[l] from goal[l], into
//                               path[offset[l] .. offset[l + 1]).
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
constexpr int kMaxFields = 65535;       // fields of one batch: a launch grid's y extent
constexpr int kMaxStandHeight = 254;    // grid_stand.hip's largest height of a verified support

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

// The allowed moves of the cell at LDS index c, bit k for move k of for_hood's numbering: the 27 walk bytes around it.
// for_hood's walk and numbering, written out: as a lambda here the compiler waits for the 27 byte reads in batches of
// 8 instead of issuing them together (24 for 43 VGPRs, and a sweep measured 1 % slower)
__device__ __forceinline__ unsigned fold_moves(const unsigned char* sw, int c) {
  unsigned hood = 0, moves = 0;
#pragma unroll
  for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx)
        if (sw[c + dz * kPlane + dy * kRow + dx]) hood |= hood_bit(dx, dy, dz);
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
  return moves;
}

// settle's step: the lowest of `best` and what the allowed moves' neighbours in sd allow the cell at c
__device__ __forceinline__ unsigned relax_step(const unsigned* sd, int c, unsigned moves, unsigned best) {
  grid_tile::for_hood([&](int dx, int dy, int dz, int off, int k) {
    if (moves & (1u << k)) {
      const unsigned d = sd[c + off];
      const unsigned cand = d + (unsigned)move_cost(dx, dy, dz);
      if (d != kFar && cand < best) best = cand;              // far + w would wrap
    }
  });
  return best;
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

// route_init_kernel with the band of a body that stands: height u8 per cell (grid_stand.hip), open also needs
// h_lo <= height <= h_hi; counters[4] counts the cells the rule above alone would have opened and the band closed
__global__ __launch_bounds__(256) void route_init_stand_kernel(const unsigned char* __restrict__ state,
                                                               const unsigned short* __restrict__ d2, int min_d2,
                                                               int through_unknown,
                                                               const unsigned char* __restrict__ height, int h_lo,
                                                               int h_hi, int cells, unsigned char* __restrict__ walk,
                                                               unsigned* __restrict__ dist, u64* __restrict__ counters) {
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;      // cells <= 2^27
  bool open = false, off_band = false;
  if (i < cells) {
    const unsigned char s = state[i];
    open = through_unknown ? s != 2 : s == 1;
    if (d2) open = open && (int)d2[i] >= min_d2;
    const int h = height[i];
    off_band = open && (h < h_lo || h > h_hi);
    open = open && !off_band;
    walk[i] = open ? 1 : 0;
    dist[i] = kFar;
  }
  const bool flags[2] = {open, off_band};
  const int at[2] = {0, 4};
  block_count<2>(flags, counters, at);
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
  const unsigned moves = open ? fold_moves(sw, c) : 0u;       // the allowed moves of this cell, once
  __syncthreads();
  grid_tile::settle(tile, sd, dist, sd[c], changed, [&](unsigned best) { return relax_step(sd, c, moves, best); });
}

// The trace: this wave walks from `goal` back to the field's source (every lane of the wave calls this)
__device__ __forceinline__ void trace_walk(const unsigned char* __restrict__ walk, const unsigned* __restrict__ dist,
                                           int nx, int ny, int nz, int goal, long* __restrict__ path, long cap,
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

__global__ __launch_bounds__(64) void route_trace_kernel(const unsigned char* __restrict__ walk,
                                                         const unsigned* __restrict__ dist, int nx, int ny, int nz,
                                                         int goal, long* __restrict__ path, long cap,
                                                         long* __restrict__ length) {
  trace_walk(walk, dist, nx, ny, nz, goal, path, cap, length);
}

// ---- several fields over one walk
__global__ __launch_bounds__(256) void route_fields_far_kernel(int cells, unsigned* __restrict__ dist) {
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;      // cells <= 2^27; blockIdx.y = the field
  if (i < cells) dist[(size_t)blockIdx.y * (size_t)cells + i] = kFar;
}

__global__ __launch_bounds__(256) void route_fields_sources_kernel(const long* __restrict__ sources, int K, int cells,
                                                                   const unsigned char* __restrict__ walk,
                                                                   unsigned* __restrict__ dist,
                                                                   u64* __restrict__ counters) {
  const int f = (int)blockIdx.x * 256 + (int)threadIdx.x;
  bool accepted = false, blocked = false, outside = false;
  if (f < K) {
    const long s = sources[f];
    if (s < 0 || s >= (long)cells) {
      outside = true;
    } else if (!walk[s]) {
      blocked = true;
    } else {
      dist[(size_t)f * (size_t)cells + (size_t)s] = 0u;
      accepted = true;
    }
  }
  const bool flags[3] = {accepted, blocked, outside};
  const int at[3] = {0, 1, 2};
  block_count<3>(flags, counters, at);
}

// blockIdx.x = the tile (grid_tile::Tile reads it), blockIdx.y = the group of `group` entries of active[A].  One LDS
// block of words serves the group's fields one after the other: settle ends on a barrier after its last LDS read, so
// the next field may be staged over it.  LDS 8.4 KB and 8 waves per workgroup: the 32 waves of a CU are reached with 4
// workgroups at 34 KB, so a second block of words (to overlap a field's staging with its predecessor's relaxation)
// would buy no occupancy and cost a barrier protocol; the loop is the plain one.
// amdgpu_waves_per_eu(8): left alone the compiler takes 104 SGPRs for the loop's uniform values, which caps a SIMD at 7
// waves, 3 workgroups per CU instead of 4.  Held to 8 waves it keeps 78 and moves 26 into lanes of one more VGPR (42;
// no scratch), and the batched sweeps measured 13 to 18 % faster.
__global__ __launch_bounds__(grid_tile::kThreads) __attribute__((amdgpu_waves_per_eu(8)))
void route_sweep_many_kernel(const unsigned char* __restrict__ walk, int nx, int ny, int nz, int tx, int ty, size_t cells,
                             unsigned* dist, int K, const int* __restrict__ active, int A, int group,
                             int* __restrict__ changed) {
  __shared__ unsigned sd[kLds];
  __shared__ unsigned char sw[kLds];
  const grid_tile::Tile tile(nx, ny, nz, tx, ty);
  const int c = tile.c;
  tile.stage(sw, walk, (unsigned char)0);
  __syncthreads();
  const bool open = sw[c] != 0;                               // 0 outside the grid: `own` is implied
  if (!__syncthreads_or(open)) return;                        // nothing to relax here: no field is touched
  const unsigned moves = open ? fold_moves(sw, c) : 0u;       // once for every field of the group
  // the two words of the block that Tile::stage has this thread store (entries t and t + 512 of the 1 000)
  constexpr int kBlock = grid_tile::kH * grid_tile::kH * grid_tile::kH;
  static_assert(kBlock <= 2 * grid_tile::kThreads, "a thread stages at most two entries");
  const auto lds_of = [](int j) {
    return (j / (grid_tile::kH * grid_tile::kH)) * kPlane + ((j / grid_tile::kH) % grid_tile::kH) * kRow + j % grid_tile::kH;
  };
  const int mine0 = lds_of(tile.t);
  const int mine1 = tile.t + grid_tile::kThreads < kBlock ? lds_of(tile.t + grid_tile::kThreads) : mine0;
  const int first = (int)blockIdx.y * group;
  const int last = min(first + group, A);
  for (int a = first; a < last; ++a) {
    const int f = active[a];
    if (f < 0 || f >= K) continue;                            // not a field: nothing is read or written (uniform)
    unsigned* field = dist + (size_t)f * cells;
    tile.stage(sd, (const unsigned*)field, kFar);
    const bool finite = sd[mine0] != kFar || sd[mine1] != kFar;
    // the barrier publishes the staged words; an all-far block has nothing to lower, and nobody reads it again
    if (!__syncthreads_or(finite)) continue;
    grid_tile::settle(tile, sd, field, sd[c], changed + f, [&](unsigned best) { return relax_step(sd, c, moves, best); });
  }
}

// one wave per leg; a leg whose field or goal is none has no way
__global__ __launch_bounds__(64) void route_trace_many_kernel(const unsigned char* __restrict__ walk,
                                                              const unsigned* __restrict__ dist, int nx, int ny, int nz,
                                                              size_t cells, int K, const int* __restrict__ field_of,
                                                              const long* __restrict__ goal,
                                                              const long* __restrict__ offset, long* __restrict__ path,
                                                              long* __restrict__ length) {
  const int l = (int)blockIdx.x;
  const int f = field_of[l];
  const long g = goal[l];
  if (f < 0 || f >= K || g < 0 || g >= (long)cells) {
    if (threadIdx.x == 0) length[l] = 0;
    return;
  }
  trace_walk(walk, dist + (size_t)f * cells, nx, ny, nz, (int)g, path + offset[l], offset[l + 1] - offset[l], length + l);
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

extern "C" int pi3_grid_route_init_stand(const unsigned char* state, const unsigned short* d2, int min_d2,
                                         int through_unknown, const unsigned char* height, int h_lo, int h_hi, int nx,
                                         int ny, int nz, const long* sources, long Ns, unsigned char* walk, unsigned* dist,
                                         unsigned long long* counters, void* stream) {
  long cells = 0;
  if (!state || !height || !walk || !dist || !counters || !grid_ok(nx, ny, nz, cells) || min_d2 < 0 ||
      min_d2 > kMaxMinD2 || (min_d2 > 0 && !d2) || h_lo < 1 || h_hi < h_lo || h_hi > kMaxStandHeight || Ns < 0 ||
      Ns >= (1L << 39) || (Ns > 0 && !sources)) {
    pi3_set_error("pi3_grid_route_init_stand: bad arguments dims=(%d, %d, %d) (1 .. 2^21 - 1 each, at most 2^27 cells) "
                  "min_d2=%d (0 .. %d, 0 without d2) band=(%d, %d) (1 <= h_lo <= h_hi <= %d) Ns=%ld (0 .. 2^39 - 1), or a "
                  "null pointer", nx, ny, nz, min_d2, kMaxMinD2, h_lo, h_hi, kMaxStandHeight, Ns);
    return PI3_ERR_ARG;
  }
  if (pi3_zero_words("pi3_grid_route_init_stand", counters, 5, stream) != PI3_OK) return PI3_ERR_LAUNCH;
  hipLaunchKernelGGL(route_init_stand_kernel, dim3(voxel_table::blocks_for(cells)), dim3(256), 0, (hipStream_t)stream,
                     state, d2, min_d2, through_unknown ? 1 : 0, height, h_lo, h_hi, (int)cells, walk, dist,
                     (u64*)counters);
  if (Ns > 0)
    hipLaunchKernelGGL(route_sources_kernel, dim3(voxel_table::blocks_for(Ns)), dim3(256), 0, (hipStream_t)stream,
                       sources, Ns, (int)cells, (const unsigned char*)walk, dist, (u64*)counters);
  return pi3_check_launch("grid_route_init_stand");
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

extern "C" int pi3_grid_route_fields_init(const unsigned char* walk, int nx, int ny, int nz, const long* sources, int K,
                                          unsigned* dist, unsigned long long* counters, void* stream) {
  long cells = 0;
  if (!walk || !sources || !dist || !counters || !grid_ok(nx, ny, nz, cells) || K < 1 || K > kMaxFields) {
    pi3_set_error("pi3_grid_route_fields_init: bad arguments dims=(%d, %d, %d) (1 .. 2^21 - 1 each, at most 2^27 cells) "
                  "K=%d (1 .. %d), or a null pointer", nx, ny, nz, K, kMaxFields);
    return PI3_ERR_ARG;
  }
  if (pi3_zero_words("pi3_grid_route_fields_init", counters, 3, stream) != PI3_OK) return PI3_ERR_LAUNCH;
  hipLaunchKernelGGL(route_fields_far_kernel, dim3(voxel_table::blocks_for(cells), (unsigned)K), dim3(256), 0,
                     (hipStream_t)stream, (int)cells, dist);
  hipLaunchKernelGGL(route_fields_sources_kernel, dim3(voxel_table::blocks_for(K)), dim3(256), 0, (hipStream_t)stream,
                     sources, K, (int)cells, walk, dist, (u64*)counters);
  return pi3_check_launch("grid_route_fields_init");
}

extern "C" int pi3_grid_route_sweep_many(const unsigned char* walk, int nx, int ny, int nz, unsigned* dist, int K,
                                         const int* active, int A, int group, int* changed, void* stream) {
  long cells = 0;
  if (!walk || !dist || !changed || !grid_ok(nx, ny, nz, cells) || K < 1 || K > kMaxFields || A < 0 || A > K ||
      (A > 0 && !active) || group < 1) {
    pi3_set_error("pi3_grid_route_sweep_many: bad arguments dims=(%d, %d, %d) (1 .. 2^21 - 1 each, at most 2^27 cells) "
                  "K=%d (1 .. %d) A=%d (0 .. K) group=%d (>= 1), or a null pointer", nx, ny, nz, K, kMaxFields, A,
                  group);
    return PI3_ERR_ARG;
  }
  if (A == 0) return PI3_OK;                                  // no field is listed: nothing to sweep
  int tx, ty;
  const unsigned tiles = grid_tile::tiles(nx, ny, nz, tx, ty);
  const int per = group < A ? group : A;                      // more than A means A
  const unsigned groups = (unsigned)((A + per - 1) / per);    // <= K <= 65 535: a launch grid's y extent
  hipLaunchKernelGGL(route_sweep_many_kernel, dim3(tiles, groups), dim3(grid_tile::kThreads), 0, (hipStream_t)stream,
                     walk, nx, ny, nz, tx, ty, (size_t)cells, dist, K, active, A, per, changed);
  return pi3_check_launch("grid_route_sweep_many");
}

extern "C" int pi3_grid_route_trace_many(const unsigned char* walk, const unsigned* dist, int nx, int ny, int nz, int K,
                                         const int* field_of, const long* goal, const long* offset, long* path,
                                         long* length, int L, void* stream) {
  long cells = 0;
  if (!walk || !dist || !grid_ok(nx, ny, nz, cells) || K < 1 || K > kMaxFields || L < 0 ||
      (L > 0 && (!field_of || !goal || !offset || !path || !length))) {
    pi3_set_error("pi3_grid_route_trace_many: bad arguments dims=(%d, %d, %d) (1 .. 2^21 - 1 each, at most 2^27 cells) "
                  "K=%d (1 .. %d) L=%d (>= 0), or a null pointer", nx, ny, nz, K, kMaxFields, L);
    return PI3_ERR_ARG;
  }
  if (L == 0) return PI3_OK;                                  // no leg: nothing to trace
  hipLaunchKernelGGL(route_trace_many_kernel, dim3((unsigned)L), dim3(64), 0, (hipStream_t)stream, walk, dist, nx, ny,
                     nz, (size_t)cells, K, field_of, goal, offset, path, length);
  return pi3_check_launch("grid_route_trace_many");
}
