// Routes for a body that stands (occupancy.hip's layout: state u8 [nz][ny][nx], x fastest, cell (ix, iy, iz) at the linear
// index (iz ny + iy) nx + ix; 0 unknown, 1 free, 2 occupied): how high above something to stand on is a cell?  Integers
// only; tests/grid_stand_ref.py reproduces every output byte for byte.
//
//   up        s e_k, one of the six signed axes (up_axis k in 0 .. 2 = x, y, z; up_sign s = +-1).
//   passable  state == 1, or with through_unknown state != 2.  A cell that is not passable, and the first cell outside
//             the grid, is a stop.
//   height    u8 per cell, whatever the cell's own state: the first stop among c - j up, j = 1 .. 254.  An occupied cell
//             gives j; an unknown cell or the grid's border gives 0 (no verified support); none within 254 gives 255.
//
//   pi3_grid_stand_height  one pass, every direction reads state along x and writes every byte once.
//     along y, z   a workgroup is 64 cells of x by 4 lines of the third axis, a thread walks kSeg cells of its column from
//                  the -up side.  It carries (j, kind) of the last stop and first finds them by looking back from its
//                  segment, 254 cells at most (the rule reaches no further), so columns are cut into segments that fill
//                  the card whatever the grid's height.
//     along x      a wave takes 64 consecutive cells of a row: one ballot of "stops here", one of "is occupied".  For the
//                  lane at l the highest set bit of the stop ballot below l (up = +x; the lowest above l for -x) gives j
//                  and the kind; a lane with none takes the wave-uniform carry, the distance from the chunk's first cell
//                  in scan order to the last stop before it and that stop's kind.  A wave walks kChunks chunks of its row
//                  in scan order and first finds its carry in the kChunks chunks before them (256 >= 254 cells).  Lanes
//                  past the row's end are stops of the border's kind.
//   pi3_grid_view_candidates_stand  pi3_grid_view_candidates (grid_view.hip) with the lattice of a standing planner: on
//                  the two axes other than up's the absolute index is a multiple of stride, along up the lattice follows
//                  the floor, (height - h_lo) mod stride == 0.
#include "common.h"
#include "grid_tile.h"
#include "voxel_table.h"
#include "wave_block.h"

#include <stdint.h>

namespace {

using grid_tile::grid_ok;
using voxel_table::u64;
using wave_block::block_exclusive_scan;

constexpr int kMaxHeight = 254;         // the rule's reach in cells
constexpr int kFarHeight = 255;         // no stop within reach
constexpr int kSeg = 32;                // cells of a column per thread
constexpr int kChunks = 4;              // 64-cell chunks of a row per wave, and the chunks its carry is looked for in
constexpr int kNoCarry = 512;           // a carry beyond any reach
constexpr unsigned kUnreached = 0xFFFFFFFFu;      // grid_route.hip's mark of a cell no route reaches
static_assert(kChunks * 64 >= kMaxHeight, "the look-back covers the rule's reach");

__device__ __forceinline__ bool is_stop(unsigned char s, int through_unknown) { return through_unknown ? s == 2 : s != 1; }

__device__ __forceinline__ unsigned char height_of(int j, bool occupied) {
  return (unsigned char)(j > kMaxHeight ? kFarHeight : occupied ? j : 0);
}

// blockIdx.x = (segment, group of 4 lines, chunk of 64 x), the chunk fastest.  t counts the column's cells from the -up
// side: cell t lies at col[t step].
__global__ __launch_bounds__(256) void stand_height_columns_kernel(const unsigned char* __restrict__ state, int nx,
                                                                   int n_line, int n_scan, long line_stride,
                                                                   long scan_stride, int up_sign, int through_unknown,
                                                                   int x_chunks, int line_groups,
                                                                   unsigned char* __restrict__ height) {
  unsigned b = blockIdx.x;
  const int xc = (int)(b % (unsigned)x_chunks);
  b /= (unsigned)x_chunks;
  const int lg = (int)(b % (unsigned)line_groups), seg = (int)(b / (unsigned)line_groups);
  const int x = xc * 64 + (int)(threadIdx.x & 63), line = lg * 4 + (int)(threadIdx.x >> 6);
  if (x >= nx || line >= n_line) return;
  const long base = (long)line * line_stride + x + (up_sign > 0 ? 0 : (long)(n_scan - 1) * scan_stride);
  const long step = up_sign > 0 ? scan_stride : -scan_stride;
  const unsigned char* col = state + base;
  unsigned char* out = height + base;
  const int t0 = seg * kSeg, t1 = min(t0 + kSeg, n_scan);
  int j = kFarHeight;
  bool occupied = false;
  for (int back = 1; back <= kMaxHeight; ++back) {            // the last stop before the segment
    const int t = t0 - back;
    if (t < 0) {                                              // the border
      j = back;
      break;
    }
    const unsigned char s = col[t * step];
    if (is_stop(s, through_unknown)) {
      j = back;
      occupied = s == 2;
      break;
    }
  }
#pragma unroll 4
  for (int t = t0; t < t1; ++t) {
    const unsigned char s = col[t * step];
    out[t * step] = height_of(j, occupied);
    if (is_stop(s, through_unknown)) {
      j = 1;
      occupied = s == 2;
    } else {
      j = min(j + 1, kFarHeight);
    }
  }
}

// the two ballots of chunk c of a row of nx cells; a lane past the row's end is a stop that is not occupied
__device__ __forceinline__ void chunk_ballots(const unsigned char* __restrict__ row, int nx, int c, int lane,
                                              int through_unknown, u64& stop, u64& occupied) {
  const int x = c * 64 + lane;
  bool st = true, oc = false;
  if (x < nx) {
    const unsigned char s = row[x];
    st = is_stop(s, through_unknown);
    oc = s == 2;
  }
  stop = __ballot(st);
  occupied = __ballot(oc);
}

// the carry a chunk with a stop leaves: the distance from the next chunk's first cell in scan order to the chunk's last
// stop in scan order, and that stop's kind
__device__ __forceinline__ void carry_of(u64 stop, u64 occupied, int up_sign, int& cj, bool& coc) {
  const int at = up_sign > 0 ? 63 - __clzll((long long)stop) : __ffsll((long long)stop) - 1;
  cj = up_sign > 0 ? 64 - at : at + 1;
  coc = (occupied >> at) & 1ull;
}

// a wave per (row, segment of kChunks chunks); 4 waves per workgroup
__global__ __launch_bounds__(256) void stand_height_rows_kernel(const unsigned char* __restrict__ state, int nx, long rows,
                                                                int up_sign, int through_unknown, int segs,
                                                                unsigned char* __restrict__ height) {
  const long w = (long)blockIdx.x * 4 + (long)(threadIdx.x >> 6);
  const int lane = (int)(threadIdx.x & 63);
  const long r = w / segs;
  if (r >= rows) return;                                      // the whole wave
  const int seg = (int)(w - r * segs);
  const unsigned char* row = state + r * nx;
  unsigned char* out = height + r * nx;
  const int n_chunks = (nx + 63) / 64;
  const int k0 = seg * kChunks, k1 = min(k0 + kChunks, n_chunks);   // chunks in scan order: k is chunk k, or its mirror
  u64 stop, occupied;
  int cj = kNoCarry;
  bool coc = false;
  for (int back = 1; back <= kChunks; ++back) {               // uniform over the wave
    const int k = k0 - back;
    if (k < 0) {                                              // the border next to the first chunk
      cj = (back - 1) * 64 + 1;
      break;
    }
    chunk_ballots(row, nx, up_sign > 0 ? k : n_chunks - 1 - k, lane, through_unknown, stop, occupied);
    if (stop) {
      carry_of(stop, occupied, up_sign, cj, coc);
      cj += (back - 1) * 64;
      break;
    }
  }
  for (int k = k0; k < k1; ++k) {
    const int c = up_sign > 0 ? k : n_chunks - 1 - k;
    chunk_ballots(row, nx, c, lane, through_unknown, stop, occupied);
    // the stops on the -up side of this lane: below it for +x, above it for -x
    const u64 side = up_sign > 0 ? stop & ((1ull << lane) - 1ull) : stop & ~((2ull << lane) - 1ull);
    int j = cj + (up_sign > 0 ? lane : 63 - lane);
    bool oc = coc;
    if (side) {
      const int at = up_sign > 0 ? 63 - __clzll((long long)side) : __ffsll((long long)side) - 1;
      j = up_sign > 0 ? lane - at : at - lane;
      oc = (occupied >> at) & 1ull;
    }
    const int x = c * 64 + lane;
    if (x < nx) out[x] = height_of(j, oc);
    if (stop)
      carry_of(stop, occupied, up_sign, cj, coc);
    else
      cj = min(cj + 64, kNoCarry);
  }
}

__device__ __forceinline__ int floor_mod(long v, int m) {
  const int r = (int)(v % m);
  return r < 0 ? r + m : r;
}

__global__ __launch_bounds__(256) void stand_candidates_kernel(const unsigned* __restrict__ dist,
                                                               const unsigned char* __restrict__ height, int nx, int ny,
                                                               int cells, int ox, int oy, int oz, int stride,
                                                               unsigned max_cost, int up_axis, int h_lo,
                                                               long* __restrict__ out, long cap, u64* __restrict__ count) {
  __shared__ u64 base;
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;      // cells <= 2^27
  bool on = false;
  if (i < cells) {
    const unsigned d = dist[i];
    if (d != kUnreached && d <= max_cost) {
      const int line = i / nx;
      const int x = i - line * nx, y = line % ny, z = line / ny;
      const int along = floor_mod((long)height[i] - h_lo, stride);
      on = (up_axis == 0 ? along : floor_mod((long)ox + x, stride)) == 0 &&
           (up_axis == 1 ? along : floor_mod((long)oy + y, stride)) == 0 &&
           (up_axis == 2 ? along : floor_mod((long)oz + z, stride)) == 0;
    }
  }
  u64 total = 0;
  const u64 before = block_exclusive_scan(on ? 1ull : 0ull, total);
  if (threadIdx.x == 0 && total) base = atomicAdd(count, total);
  __syncthreads();
  if (on) {
    const u64 slot = base + before;
    if (slot < (u64)cap) out[slot] = (long)i;
  }
}

}  // namespace

extern "C" int pi3_grid_stand_height(const unsigned char* state, int nx, int ny, int nz, int up_axis, int up_sign,
                                     int through_unknown, unsigned char* height, void* stream) {
  long cells = 0;
  if (!state || !height || !grid_ok(nx, ny, nz, cells) || up_axis < 0 || up_axis > 2 || (up_sign != 1 && up_sign != -1)) {
    pi3_set_error("pi3_grid_stand_height: bad arguments dims=(%d, %d, %d) (1 .. 2^21 - 1 each, at most 2^27 cells) "
                  "up_axis=%d (0 .. 2) up_sign=%d (1 or -1), or a null pointer", nx, ny, nz, up_axis, up_sign);
    return PI3_ERR_ARG;
  }
  const int tu = through_unknown ? 1 : 0;
  if (up_axis == 0) {
    const long rows = (long)ny * nz;
    const int segs = ((nx + 63) / 64 + kChunks - 1) / kChunks;
    const long waves = rows * segs;                           // <= cells
    hipLaunchKernelGGL(stand_height_rows_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       state, nx, rows, up_sign, tu, segs, height);
  } else {
    // the scan axis and the third one, whose lines a workgroup takes four of
    const int n_scan = up_axis == 1 ? ny : nz, n_line = up_axis == 1 ? nz : ny;
    const long scan_stride = up_axis == 1 ? (long)nx : (long)nx * ny;
    const long line_stride = up_axis == 1 ? (long)nx * ny : (long)nx;
    const int x_chunks = (nx + 63) / 64, line_groups = (n_line + 3) / 4, segments = (n_scan + kSeg - 1) / kSeg;
    const long blocks = (long)x_chunks * line_groups * segments;        // every one holds a cell: <= 2^27
    hipLaunchKernelGGL(stand_height_columns_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, state, nx,
                       n_line, n_scan, line_stride, scan_stride, up_sign, tu, x_chunks, line_groups, height);
  }
  return pi3_check_launch("grid_stand_height");
}

extern "C" int pi3_grid_view_candidates_stand(const unsigned* dist, const unsigned char* height, int nx, int ny, int nz,
                                              int ox, int oy, int oz, int stride, long max_cost, int up_axis, int h_lo,
                                              long* cells_out, long cap, long* count, void* stream) {
  long cells = 0;
  if (!dist || !height || !count || !grid_ok(nx, ny, nz, cells) || stride < 1 || max_cost < 0 || up_axis < 0 ||
      up_axis > 2 || h_lo < 1 || h_lo > kMaxHeight || cap < 0 || (cap > 0 && !cells_out)) {
    pi3_set_error("pi3_grid_view_candidates_stand: bad arguments dims=(%d, %d, %d) (1 .. 2^21 - 1 each, at most 2^27 "
                  "cells) stride=%d (>= 1) max_cost=%ld (>= 0) up_axis=%d (0 .. 2) h_lo=%d (1 .. %d) cap=%ld (>= 0; cells "
                  "may be NULL at 0), or a null pointer", nx, ny, nz, stride, max_cost, up_axis, h_lo, kMaxHeight, cap);
    return PI3_ERR_ARG;
  }
  if (pi3_zero_words("pi3_grid_view_candidates_stand", count, 1, stream) != PI3_OK) return PI3_ERR_LAUNCH;
  const unsigned limit = max_cost >= (long)kUnreached ? kUnreached - 1u : (unsigned)max_cost;       // that mark never passes
  hipLaunchKernelGGL(stand_candidates_kernel, dim3(voxel_table::blocks_for(cells)), dim3(256), 0, (hipStream_t)stream,
                     dist, height, nx, ny, (int)cells, ox, oy, oz, stride, limit, up_axis, h_lo, cells_out, cap,
                     (u64*)count);
  return pi3_check_launch("grid_view_candidates_stand");
}
