// Line of sight between cells of the route graph (grid_route.hip's walk u8 [nz][ny][nx], 1 = traversable): can a body go
// straight from the centre of cell a to the centre of cell b?  Integers only, no scratch, no atomics;
// tests/grid_sight_ref.py reproduces every output byte for byte.
//
//   sight   a SEES b when every cell whose closed cube meets the segment between the two centres is traversable: the
//           closed supercover of the segment.  With o = b - a, (ax, ay, az) = |o|, m* = max(a*, 1) and the common
//           denominator 2 mx my mz, the segment crosses its k-th x plane at the key (2k - 1) my mz: kx starts at my mz and
//           grows by 2 my mz per crossing (y and z alike; an axis with a* = 0 never steps, its key is kNever).  A step
//           takes m = min(kx, ky, kz) and every axis whose key equals m steps together: grid_view_ray::ray_arrives_from's keys.
//           The difference is the tie: with s = 2 or 3 axes stepping the segment runs through an edge or a corner, and
//           all 2^s cells at + (a sx, b sy, e sz), a, b, e in {0, 1} over the stepping axes, are touched, not only the
//           diagonal one.  For a unit offset that is grid_route.hip's move rule of 2, 4 or 8 cells, so two consecutive
//           cells of a trace always see each other.  The rule is symmetric in a and b, the end cell is touched like any
//           other, and a == b touches the one cell.
//   bounds  every touched cell lies inside the bounding box of a and b, so two ends inside the grid need no bounds test
//           on the way.
//   32 bits (ax + 1)(ay + 1)(az + 1) <= cells <= 2^27 (grid_tile::kMaxCells), so mx my mz <= 2^27, a key's increment
//           2 m m <= 2^28 and every key that is still waiting lies below 2 mx my mz <= 2^28 < kNever = 2^30.  An axis that
//           has made its last crossing holds (2 a* + 1) m m <= 2^28 + 2^27: above every waiting key, below kNever, and
//           the walk ends on its count of crossings.  The offset (511, 511, 511) reaches 266 604 541.
//   pi3_grid_route_sight_paths  the cells of `legs` ways one after the other (way l is cells[offsets[l] .. offsets[l + 1])):
//           bit k of row p of vis u64 [P][ceil(span / 64)] is set when p and p + 1 + k lie in the same way, k < span, and
//           cells[p] sees cells[p + 1 + k]; every other bit is written 0.  One wave per (row, word): lane k walks its own
//           segment (it stops at the first blocked cell) and the wave's ballot is the stored word.  The partners of a
//           wave are consecutive along a way, so their walks have similar length and share their first cells.
//   pi3_grid_route_sight_pairs  arbitrary pairs, a lane each.  The whole segment is walked even after a blocked cell:
//           sees, touched = the supercover's cell count, min_d2 = the smallest d2 (pi3_grid_edt's field) over the touched
//           cells, 0xFFFF without d2.  An end outside [0, cells) gives 0, 0, 0xFFFF.
// walk is read with plain byte loads: the touched cells of one wave lie in one small box and hit the caches (DESIGN 7l
// has the timing that decided against staging that box as bits in LDS).
#include "common.h"
#include "grid_tile.h"
#include "grid_view_ray.h"
#include "voxel_table.h"

#include <stdint.h>

namespace {

using grid_tile::grid_ok;
using grid_view_ray::kNever;
using voxel_table::u64;

constexpr int kD2Far = 0xFFFF;
constexpr int kMaxSpan = 4096;
static_assert(2 * grid_tile::kMaxCells < (long)kNever, "every waiting key stays below kNever");
static_assert(3 * grid_tile::kMaxCells < (1L << 31), "a key after its axis' last crossing fits 32 bits");

// The closed supercover of the segment between the centres of the cells a and b (linear indices inside the grid): does
// a see b?  kWhole: the walk goes on after a blocked cell, `touched` counts the cells and min_d2 takes the smallest
// d2 over them (d2 may be NULL); otherwise it stops at the first blocked cell and the two are not meaningful.
template <bool kWhole>
__device__ __forceinline__ bool sight_walk(const unsigned char* __restrict__ walk, const unsigned short* __restrict__ d2,
                                           int nx, int ny, int a, int b, int& touched, int& min_d2) {
  const int la = a / nx, lb = b / nx;
  const int ox = (b - lb * nx) - (a - la * nx), oy = lb % ny - la % ny, oz = lb / ny - la / ny;
  const int ax = abs(ox), ay = abs(oy), az = abs(oz);
  const int mx = max(ax, 1), my = max(ay, 1), mz = max(az, 1);
  const int px = 2 * my * mz, py = 2 * mx * mz, pz = 2 * mx * my;       // a key grows by 2 P per crossing
  int kx = ax ? (px >> 1) : kNever, ky = ay ? (py >> 1) : kNever, kz = az ? (pz >> 1) : kNever;
  const int sx = ox > 0 ? 1 : -1, sy = oy > 0 ? nx : -nx, sz = oz > 0 ? nx * ny : -(nx * ny);
  int at = a;
  int left = ax + ay + az;                                    // crossings to go; 0 at b
  bool sees = true;
  touched = 0, min_d2 = kD2Far;
  const auto touch = [&](int c) {
    if (!walk[c]) sees = false;
    if (kWhole) {
      ++touched;
      if (d2) min_d2 = min(min_d2, (int)d2[c]);
    }
  };
  touch(at);
  while (left > 0 && (kWhole || sees)) {
    const int m = min(kx, min(ky, kz));
    const int dx = kx == m ? sx : 0, dy = ky == m ? sy : 0, dz = kz == m ? sz : 0;
    // the 2^s cells over the stepping axes, without `at` itself
    if (dx) touch(at + dx);
    if (dy) {
      touch(at + dy);
      if (dx) touch(at + dx + dy);
    }
    if (dz) {
      touch(at + dz);
      if (dx) touch(at + dx + dz);
      if (dy) {
        touch(at + dy + dz);
        if (dx) touch(at + dx + dy + dz);
      }
    }
    at += dx + dy + dz;
    if (dx) kx += px, --left;
    if (dy) ky += py, --left;
    if (dz) kz += pz, --left;
  }
  return sees;
}

// wave v of the launch = (row p, word w) = (v / W, v % W); four waves per workgroup
__global__ __launch_bounds__(256) void sight_paths_kernel(const unsigned char* __restrict__ walk, int nx, int ny,
                                                          int cells, const long* __restrict__ path, long P,
                                                          const long* __restrict__ offsets, int legs, int span, int W,
                                                          u64* __restrict__ vis) {
  const long v = (long)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
  if (v >= P * W) return;                                     // the whole wave
  const int lane = (int)threadIdx.x & 63;
  const long p = v / W;
  const int w = (int)(v - p * W);
  // the way that holds row p: the first l with p < offsets[l + 1]; its end bounds the partners
  int lo = 0, hi = legs;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (offsets[mid + 1] <= p) lo = mid + 1; else hi = mid;
  }
  const long end = lo < legs && offsets[lo] <= p ? min(offsets[lo + 1], P) : 0;
  const int k = w * 64 + lane;
  const long q = p + 1 + k;
  bool sees = false;
  if (k < span && q < end) {
    const long a = path[p], b = path[q];
    if (a >= 0 && a < (long)cells && b >= 0 && b < (long)cells) {
      int touched, min_d2;
      sees = sight_walk<false>(walk, nullptr, nx, ny, (int)a, (int)b, touched, min_d2);
    }
  }
  const u64 word = __ballot(sees);
  if (lane == 0) vis[v] = word;
}

__global__ __launch_bounds__(256) void sight_pairs_kernel(const unsigned char* __restrict__ walk,
                                                          const unsigned short* __restrict__ d2, int nx, int ny,
                                                          int cells, const long* __restrict__ a,
                                                          const long* __restrict__ b, long N,
                                                          unsigned char* __restrict__ sees, int* __restrict__ touched,
                                                          unsigned short* __restrict__ min_d2) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const long ca = a[i], cb = b[i];
  bool s = false;
  int n = 0, low = kD2Far;
  if (ca >= 0 && ca < (long)cells && cb >= 0 && cb < (long)cells)
    s = sight_walk<true>(walk, d2, nx, ny, (int)ca, (int)cb, n, low);
  sees[i] = s ? 1 : 0;
  touched[i] = n;
  min_d2[i] = (unsigned short)low;
}

}  // namespace

extern "C" int pi3_grid_route_sight_paths(const unsigned char* walk, int nx, int ny, int nz, const long* cells, long P,
                                          const long* offsets, int legs, int span, unsigned long long* vis,
                                          void* stream) {
  long n_cells = 0;
  const bool some = P > 0 && legs > 0;
  if (!walk || !grid_ok(nx, ny, nz, n_cells) || P < 0 || P >= (1L << 31) || legs < 0 || span < 1 || span > kMaxSpan ||
      (some && (!cells || !offsets || !vis))) {
    pi3_set_error("pi3_grid_route_sight_paths: bad arguments dims=(%d, %d, %d) (1 .. 2^21 - 1 each, at most 2^27 cells) "
                  "P=%ld (0 .. 2^31 - 1) legs=%d (>= 0) span=%d (1 .. %d), or a null pointer", nx, ny, nz, P, legs, span,
                  kMaxSpan);
    return PI3_ERR_ARG;
  }
  if (!some) return PI3_OK;                                   // no row or no way: nothing to test
  const int W = (span + 63) / 64;
  const long blocks = (P * W + 3) / 4;                        // < 2^31 x 64 / 4
  if (blocks >= (1L << 31)) {
    pi3_set_error("pi3_grid_route_sight_paths: P=%ld rows of %d words need %ld workgroups (fewer than 2^31)", P, W,
                  blocks);
    return PI3_ERR_ARG;
  }
  hipLaunchKernelGGL(sight_paths_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, walk, nx, ny,
                     (int)n_cells, cells, P, offsets, legs, span, W, (u64*)vis);
  return pi3_check_launch("grid_route_sight_paths");
}

extern "C" int pi3_grid_route_sight_pairs(const unsigned char* walk, const unsigned short* d2, int nx, int ny, int nz,
                                          const long* a, const long* b, long N, unsigned char* sees, int* touched,
                                          unsigned short* min_d2, void* stream) {
  long n_cells = 0;
  if (!walk || !grid_ok(nx, ny, nz, n_cells) || N < 0 || N >= (1L << 39) ||
      (N > 0 && (!a || !b || !sees || !touched || !min_d2))) {
    pi3_set_error("pi3_grid_route_sight_pairs: bad arguments dims=(%d, %d, %d) (1 .. 2^21 - 1 each, at most 2^27 cells) "
                  "N=%ld (0 .. 2^39 - 1), or a null pointer", nx, ny, nz, N);
    return PI3_ERR_ARG;
  }
  if (N == 0) return PI3_OK;                                  // no pair: nothing to test
  hipLaunchKernelGGL(sight_pairs_kernel, dim3(voxel_table::blocks_for(N)), dim3(256), 0, (hipStream_t)stream, walk, d2, nx,
                     ny, (int)n_cells, a, b, N, sees, touched, min_d2);
  return pi3_check_launch("grid_route_sight_pairs");
}
