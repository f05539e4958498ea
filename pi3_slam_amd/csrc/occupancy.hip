// Occupancy grid and clearance field of the dense map: the complement of the surface.  A regular grid of cells of edge
// c, integer origin (ox, oy, oz), dimensions (nx, ny, nz), cell (ix, iy, iz) at the linear index (iz ny + iy) nx + ix
// (x fastest), one state byte per cell: 0 unknown, 1 free, 2 occupied.
//
//   pi3_occupancy_mark     a thread per map point (the f32 rows of the extracted map): every axis through the voxel
//                          quantiser (voxel_table.h: quantise, at inv_v = (float)(1 / c)), the unbiased index minus the
//                          origin; state = 2 when the cell is inside the grid.  The call zeroes the grid first.  Many
//                          threads may write the same byte with the same value; that is the only overlap.
//   pi3_occupancy_observe  a thread per cell; an occupied cell is left alone.  The cell's centre X = c ((double)(o + i) +
//                          0.5) per axis is projected into every depth keyframe with the carver's arithmetic, operation
//                          for operation (voxel_carve.hip): the 20-double camera row, the depth scale in slot 17, rint of
//                          u inv_s, the fp16 gather, the same "no vote" cases.  lim = rel_tol zo + margin;  r < -lim is a
//                          free vote (the view measured a surface behind the centre: it looked through the cell),
//                          |r| <= lim a hit vote.  state = 1 when free >= min_free_views and free > hit, else 0.
//                          Then the cameras' own cells: a view cannot see the place it stands in (zc is about 0 there)
//                          and no other view need look through it, yet a camera stood there.  One thread walks the
//                          views in order: centre = -R^T t of the view's row, cell = floor(centre / c) per axis; a
//                          cell inside the grid that is unknown becomes free and moves from the unknown to the free
//                          count (counters[5] counts them).  The votes are not touched.
//                          f64 without contraction (the Makefile compiles this file with -ffp-contract=off):
//                          tests/occupancy_ref.py reproduces state, votes and counters byte for byte.
//                          Consecutive x in a wave: the 64 projections of a view lie next to each other in its plane; the
//                          camera rows are wave-uniform loads.  The gather is in bounds by construction: pu and pv are
//                          tested against the plane's size as doubles before they become indices.
//   pi3_grid_edt           the exact squared Euclidean distance transform of the grid, truncated at R cells (1..255):
//                          d2 u16 per cell = the squared distance in cells to the nearest site when it is <= R^2, else
//                          0xFFFF.  Sites: state == 2, and state == 0 too when unknown_is_obstacle.  Three separable
//                          passes x, y, z, each  out[i] = min over |d| <= R of in[i + d] + d^2  in integers, values above
//                          R^2 clamped to 0xFFFF after each pass (later passes only add: nothing is lost, and every
//                          intermediate fits u16).  The x pass reads the state bytes; the passes ping-pong between the
//                          output and one workspace of the same size, never in place: x -> d2, y -> work, z -> d2.
//                          A line segment and its halo are staged in LDS; d is scanned outwards from 0 and the scan stops
//                          once d^2 >= the best so far, so the cost follows the actual distance.  The y and z passes take
//                          tiles of 64 consecutive x, so global traffic stays coalesced.
#include "common.h"
#include "voxel_table.h"
#include "wave_block.h"

#include <stdint.h>

namespace {

using voxel_table::u64;
using wave_block::block_count;

constexpr int kDepthScaleAt = 17;       // the spare camera slot that carries the view's depth scale
constexpr int kMaxRadius = 255;         // R^2 = 65 025 < 0xFFFF
constexpr int kFar = 0xFFFF;
constexpr int kTile = 64;               // outputs along the axis per tile of the y and z passes
constexpr long kMaxCells = 1L << 40;
constexpr int kMaxIndex = 1 << 21;      // |origin| and every dimension stay below: o + i never overflows an int

__global__ __launch_bounds__(256) void occupancy_mark_kernel(const float* __restrict__ points, long P, float inv_v,
                                                             int ox, int oy, int oz, int nx, int ny, int nz,
                                                             unsigned char* __restrict__ state,
                                                             u64* __restrict__ counters) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  bool marked = false, dropped = false, outside = false;
  if (i < P) {
    const float* p = points + 3 * i;
    uint32_t kx, ky, kz, u;
    if (!(voxel_table::quantise(p[0], inv_v, kx, u) && voxel_table::quantise(p[1], inv_v, ky, u) &&
          voxel_table::quantise(p[2], inv_v, kz, u))) {
      dropped = true;
    } else {
      const int ix = ((int)kx - voxel_table::kBias) - ox;
      const int iy = ((int)ky - voxel_table::kBias) - oy;
      const int iz = ((int)kz - voxel_table::kBias) - oz;
      if (ix >= 0 && ix < nx && iy >= 0 && iy < ny && iz >= 0 && iz < nz) {
        state[((long)iz * ny + iy) * nx + ix] = 2;
        marked = true;
      } else {
        outside = true;
      }
    }
  }
  const bool flags[3] = {marked, dropped, outside};
  const int at[3] = {0, 1, 2};
  block_count<3>(flags, counters, at);
}

__global__ __launch_bounds__(256) void occupancy_observe_kernel(
    unsigned char* __restrict__ state, long cells, int nx, int ny, int ox, int oy, int oz, double cell,
    const double* __restrict__ views, int M, const _Float16* __restrict__ planes, int Hp, int Wp, double inv_s,
    double rel_tol, double margin, unsigned min_free, unsigned* __restrict__ free_out, unsigned* __restrict__ hit_out,
    u64* __restrict__ counters) {
#pragma clang fp contract(off)      // the intent; what enforces it under the library's flags is the Makefile
  const long s = (long)blockIdx.x * 256 + threadIdx.x;
  const bool inside = s < cells;
  bool occupied = false;
  double x = 0.0, y = 0.0, z = 0.0;
  if (inside) {
    occupied = state[s] == 2;
    const long line = s / nx;
    const int ix = (int)(s - line * nx), iy = (int)(line % ny), iz = (int)(line / ny);
    x = cell * ((double)(ox + ix) + 0.5);
    y = cell * ((double)(oy + iy) + 0.5);
    z = cell * ((double)(oz + iz) + 0.5);
  }
  const bool open = inside && !occupied;
  unsigned nfree = 0, nhit = 0;
  if (__ballot(open)) {                   // a wave without an open cell skips the views
    const long per = (long)Hp * Wp;
    const double wmax = (double)(Wp - 1), hmax = (double)(Hp - 1);
    for (int m = 0; m < M; ++m) {
      const double* __restrict__ c = views + (long)m * kCamDoubles;
      const double xc = ((c[0] * x + c[1] * y) + c[2] * z) + c[3];
      const double yc = ((c[4] * x + c[5] * y) + c[6] * z) + c[7];
      const double zc = ((c[8] * x + c[9] * y) + c[10] * z) + c[11];
      if (!open || !(zc > 0.0) || !__builtin_isfinite(xc) || !__builtin_isfinite(yc) || !__builtin_isfinite(zc))
        continue;
      const double u = c[12] * (xc / zc) + c[14];
      const double v = c[13] * (yc / zc) + c[15];
      const double pu = rint(u * inv_s), pv = rint(v * inv_s);      // inv_s = 1, 1/2 or 1/4: the product is the quotient
      if (!(pu >= 0.0 && pu <= wmax && pv >= 0.0 && pv <= hmax)) continue;     // NaN falls out
      const double zo = c[kDepthScaleAt] * (double)planes[m * per + (long)(int)pv * Wp + (int)pu];
      if (zo == 0.0 || !__builtin_isfinite(zo)) continue;
      const double r = zc - zo, lim = rel_tol * zo + margin;
      if (fabs(r) <= lim)
        ++nhit;
      else if (r < -lim)
        ++nfree;
    }
  }
  const bool is_free = open && nfree >= min_free && nfree > nhit;
  if (inside) {
    if (!occupied) state[s] = is_free ? 1 : 0;
    if (free_out) free_out[s] = nfree;
    if (hit_out) hit_out[s] = nhit;
  }
  const bool flags[5] = {inside, occupied, is_free, open && !is_free, open && nfree + nhit == 0};
  const int at[5] = {0, 1, 2, 3, 4};
  block_count<5>(flags, counters, at);         // every thread of the workgroup arrives here: the loop only continues
}

// The cells the cameras stand in, after the vote: serial (M is hundreds; several views may share a cell), so the counts
// need no atomics.  centre_j = -((r0j t0 + r1j t1) + r2j t2), k = floor(centre / cell), in f64 in this order.
__global__ void occupancy_cameras_kernel(unsigned char* __restrict__ state, int nx, int ny, int nz, int ox, int oy,
                                         int oz, double cell, const double* __restrict__ views, int M,
                                         u64* __restrict__ counters) {
#pragma clang fp contract(off)
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  u64 freed = 0;
  for (int m = 0; m < M; ++m) {
    const double* __restrict__ c = views + (long)m * kCamDoubles;
    const double kx = floor(-((c[0] * c[3] + c[4] * c[7]) + c[8] * c[11]) / cell);
    const double ky = floor(-((c[1] * c[3] + c[5] * c[7]) + c[9] * c[11]) / cell);
    const double kz = floor(-((c[2] * c[3] + c[6] * c[7]) + c[10] * c[11]) / cell);
    if (!(fabs(kx) < 1048576.0 && fabs(ky) < 1048576.0 && fabs(kz) < 1048576.0)) continue;     // NaN falls out
    const int ix = (int)kx - ox, iy = (int)ky - oy, iz = (int)kz - oz;
    if (ix < 0 || ix >= nx || iy < 0 || iy >= ny || iz < 0 || iz >= nz) continue;
    unsigned char* at = state + ((long)iz * ny + iy) * nx + ix;
    if (*at == 0) {
      *at = 1;
      ++freed;
    }
  }
  if (freed) {
    counters[2] += freed;
    counters[3] -= freed;
    counters[5] = freed;
  }
}

// min over |d| <= R of g[d] + d^2 around the LDS entry g[0], entries `step` apart, clamped: scanned outwards, stopped
// once d^2 can no longer improve on the best.  0xFFFF + d^2 > R^2 for every d: the far mark needs no case of its own.
__device__ __forceinline__ unsigned short edt_scan(const unsigned short* g, int step, int R) {
  int best = g[0];
  for (int d = 1; d <= R; ++d) {
    const int dd = d * d;
    if (dd >= best) break;
    const int a = g[-d * step], b = g[d * step];
    const int cand = (a < b ? a : b) + dd;
    best = cand < best ? cand : best;
  }
  return (unsigned short)(best > R * R ? kFar : best);
}

// x pass: a wave per segment of 64 consecutive x of one line, four segments per workgroup; LDS (dynamic) u16
// [4][64 + 2 R].  Reads the state bytes: a site is 0, everything else far.
__global__ __launch_bounds__(256) void edt_x_kernel(const unsigned char* __restrict__ state, int nx, long lines,
                                                    int segs_per_line, int R, int unknown_is_site,
                                                    unsigned short* __restrict__ out) {
  extern __shared__ unsigned short lds[];
  const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6);
  const int span = 64 + 2 * R;
  unsigned short* g = lds + wv * span;
  const long seg = (long)blockIdx.x * 4 + wv;
  const long line = seg / segs_per_line;
  const int x0 = (int)(seg - line * segs_per_line) * 64;
  const bool live = line < lines;
  if (live) {
    const unsigned char* row = state + line * nx;
    for (int j = lane; j < span; j += 64) {
      const int xs = x0 - R + j;
      unsigned short v = kFar;
      if (xs >= 0 && xs < nx) {
        const unsigned char b = row[xs];
        v = (b == 2 || (unknown_is_site && b == 0)) ? 0 : kFar;
      }
      g[j] = v;
    }
  }
  __syncthreads();
  if (live && x0 + lane < nx) out[line * nx + x0 + lane] = edt_scan(g + R + lane, 1, R);
}

// y or z pass: a tile of 64 consecutive x by kTile cells along the axis (stride `astride`, length na) at one
// coordinate of the third axis (stride `ostride`, count no); LDS (dynamic) u16 [kTile + 2 R][64].
__global__ __launch_bounds__(256) void edt_axis_kernel(const unsigned short* __restrict__ in, int nx, int na,
                                                       long astride, int no, long ostride, int xtiles, int atiles,
                                                       int R, unsigned short* __restrict__ out) {
  extern __shared__ unsigned short lds[];
  const int lane = (int)(threadIdx.x & 63), grp = (int)(threadIdx.x >> 6);
  long b = blockIdx.x;
  const int xt = (int)(b % xtiles);
  b /= xtiles;
  const int at = (int)(b % atiles);
  const long o = b / atiles;                  // < no by the grid's size
  const int x = xt * 64 + lane, a0 = at * kTile;
  const long base = o * ostride + x;
  const bool col = x < nx && o < no;
  const int rows = kTile + 2 * R;
  for (int r = grp; r < rows; r += 4) {
    const int a = a0 - R + r;
    lds[r * 64 + lane] = (col && a >= 0 && a < na) ? in[base + a * astride] : (unsigned short)kFar;
  }
  __syncthreads();
  if (col)
    for (int j = grp; j < kTile && a0 + j < na; j += 4)
      out[base + (a0 + j) * astride] = edt_scan(lds + (R + j) * 64 + lane, 64, R);
}

inline bool grid_ok(int nx, int ny, int nz, int ox, int oy, int oz, long& cells) {
  if (nx <= 0 || ny <= 0 || nz <= 0 || nx >= kMaxIndex || ny >= kMaxIndex || nz >= kMaxIndex) return false;
  if (ox <= -kMaxIndex || ox >= kMaxIndex || oy <= -kMaxIndex || oy >= kMaxIndex || oz <= -kMaxIndex || oz >= kMaxIndex)
    return false;
  cells = (long)nx * ny;                      // < 2^42
  if (cells > kMaxCells / nz) return false;
  cells *= nz;
  return true;
}

}  // namespace

extern "C" int pi3_occupancy_mark(const float* points, long P, float inv_cell, int ox, int oy, int oz, int nx, int ny,
                                  int nz, unsigned char* state, unsigned long long* counters, void* stream) {
  long cells = 0;
  if (P < 0 || P >= (1L << 39) || (P > 0 && !points) || !positive_finite(inv_cell) || !state || !counters ||
      !grid_ok(nx, ny, nz, ox, oy, oz, cells)) {
    pi3_set_error("pi3_occupancy_mark: bad arguments P=%ld (0 .. 2^39 - 1) inv_cell=%g (finite, > 0) origin=(%d, %d, %d) "
                  "(|o| < 2^21) dims=(%d, %d, %d) (1 .. 2^21 - 1 each, at most 2^40 cells), or a null pointer", P,
                  (double)inv_cell, ox, oy, oz, nx, ny, nz);
    return PI3_ERR_ARG;
  }
  if (pi3_zero_words("pi3_occupancy_mark", counters, 4, stream) != PI3_OK) return PI3_ERR_LAUNCH;
  if (hipMemsetAsync(state, 0, (size_t)cells, (hipStream_t)stream) != hipSuccess) {
    pi3_set_error("pi3_occupancy_mark: hipMemsetAsync failed");
    return PI3_ERR_LAUNCH;
  }
  if (P == 0) return PI3_OK;
  hipLaunchKernelGGL(occupancy_mark_kernel, dim3(voxel_table::blocks_for(P)), dim3(256), 0, (hipStream_t)stream, points,
                     P, inv_cell, ox, oy, oz, nx, ny, nz, state, (u64*)counters);
  return pi3_check_launch("occupancy_mark");
}

extern "C" int pi3_occupancy_observe(unsigned char* state, int nx, int ny, int nz, int ox, int oy, int oz, double cell,
                                     const double* views, int M, const unsigned short* planes, int Hp, int Wp,
                                     int pixel_stride, double rel_tol, double margin, int min_free_views,
                                     unsigned* free_votes, unsigned* hit_votes, unsigned long long* counters,
                                     void* stream) {
  long cells = 0;
  if (!state || !counters || !grid_ok(nx, ny, nz, ox, oy, oz, cells) || cells > 0x7fffffffL * 256 || M < 0 ||
      (M > 0 && (!views || !planes)) || Hp <= 0 || Wp <= 0 ||
      (pixel_stride != 1 && pixel_stride != 2 && pixel_stride != 4) || !positive_finite(cell) ||
      !positive_finite(rel_tol) || !(margin >= 0.0) || !__builtin_isfinite(margin) || min_free_views < 1) {
    pi3_set_error("pi3_occupancy_observe: bad arguments dims=(%d, %d, %d) (1 .. 2^21 - 1 each, at most 2^39 cells) "
                  "origin=(%d, %d, %d) (|o| < 2^21) cell=%g (finite, > 0) M=%d Hp=%d Wp=%d pixel_stride=%d (1, 2 or 4) "
                  "rel_tol=%g (finite, > 0) margin=%g (finite, >= 0) min_free_views=%d (>= 1), or a null pointer", nx,
                  ny, nz, ox, oy, oz, cell, M, Hp, Wp, pixel_stride, rel_tol, margin, min_free_views);
    return PI3_ERR_ARG;
  }
  if (pi3_zero_words("pi3_occupancy_observe", counters, 8, stream) != PI3_OK) return PI3_ERR_LAUNCH;
  hipLaunchKernelGGL(occupancy_observe_kernel, dim3(voxel_table::blocks_for(cells)), dim3(256), 0, (hipStream_t)stream,
                     state, cells, nx, ny, ox, oy, oz, cell, views, M, (const _Float16*)planes, Hp, Wp,
                     1.0 / (double)pixel_stride, rel_tol, margin, (unsigned)min_free_views, free_votes, hit_votes,
                     (u64*)counters);
  if (M > 0)
    hipLaunchKernelGGL(occupancy_cameras_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, nx, ny, nz, ox, oy,
                       oz, cell, views, M, (u64*)counters);
  return pi3_check_launch("occupancy_observe");
}

extern "C" int pi3_grid_edt(const unsigned char* state, int nx, int ny, int nz, int radius, int unknown_is_obstacle,
                            unsigned short* d2, unsigned short* workspace, void* stream) {
  long cells = 0;
  if (!state || !d2 || !workspace || d2 == workspace || radius < 1 || radius > kMaxRadius ||
      !grid_ok(nx, ny, nz, 0, 0, 0, cells)) {
    pi3_set_error("pi3_grid_edt: bad arguments dims=(%d, %d, %d) (1 .. 2^21 - 1 each, at most 2^40 cells) radius=%d "
                  "(1 .. %d), a null pointer, or the workspace is the output", nx, ny, nz, radius, kMaxRadius);
    return PI3_ERR_ARG;
  }
  const long lines = (long)ny * nz;
  const int xsegs = (nx + 63) / 64;
  const long xblocks = (lines * xsegs + 3) / 4;
  const int ytiles = (ny + kTile - 1) / kTile, ztiles = (nz + kTile - 1) / kTile;
  const long yblocks = (long)xsegs * ytiles * nz, zblocks = (long)xsegs * ztiles * ny;
  if (xblocks > 0x7fffffffL || yblocks > 0x7fffffffL || zblocks > 0x7fffffffL) {
    pi3_set_error("pi3_grid_edt: grid too large (%d, %d, %d)", nx, ny, nz);
    return PI3_ERR_ARG;
  }
  const int axis_lds = (kTile + 2 * radius) * 64 * (int)sizeof(unsigned short);
  static unsigned long long optin = 0;
  if (int rc = pi3_lds_optin((const void*)edt_axis_kernel, (kTile + 2 * kMaxRadius) * 64 * (int)sizeof(unsigned short),
                             &optin, "grid_edt"))
    return rc;
  hipStream_t st = (hipStream_t)stream;
  const long plane = (long)nx * ny;
  hipLaunchKernelGGL(edt_x_kernel, dim3((unsigned)xblocks), dim3(256),
                     4 * (64 + 2 * radius) * sizeof(unsigned short), st, state, nx, lines, xsegs, radius,
                     unknown_is_obstacle ? 1 : 0, d2);
  hipLaunchKernelGGL(edt_axis_kernel, dim3((unsigned)yblocks), dim3(256), axis_lds, st, (const unsigned short*)d2, nx,
                     ny, (long)nx, nz, plane, xsegs, ytiles, radius, workspace);
  hipLaunchKernelGGL(edt_axis_kernel, dim3((unsigned)zblocks), dim3(256), axis_lds, st,
                     (const unsigned short*)workspace, nx, nz, plane, ny, (long)nx, xsegs, ztiles, radius, d2);
  return pi3_check_launch("grid_edt");
}
