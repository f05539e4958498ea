// Moving a chunk's dense cloud with the views that saw it: stage 2's answer to a bundle adjustment that moved the views of
// a chunk one by one (dense_map.MapFollower).  A cloud lives in its chunk file's frame; so do the chunk's created poses
// and its depth keyframes (dense_filter.hip: pi3_dense_depth_planes).  Every keyframe m has a move D_m (3x4, f64) that
// takes a point of that frame to where the view's pixels ended up; a point follows a blend of the moves of the keyframes
// that agree with it in depth, found with the carver's projection and agreement test (voxel_carve.hip).
//
// Per point X = (x, y, z) (fp32, widened to f64) and, with normals, n = (nx, ny, nz):
//   X not finite: the outputs are the inputs, level 0, support 0, counter [0];
//   else for m = 0 .. M-1 in order, with d = moves[m] (12 doubles) and c = views[m] (20 doubles, render.hip's layout:
//   rigid frame->camera 3x4 row-major, fx fy cx cy, ortho flag, [17] = the unit of the view's plane in the cloud's units):
//     Y  = (((d0 x + d1 y) + d2 z) + d3, ((d4 x + d5 y) + d6 z) + d7, ((d8 x + d9 y) + d10 z) + d11);
//     Nn = ((d0 nx + d1 ny) + d2 nz, (d4 nx + d5 ny) + d6 nz, (d8 nx + d9 ny) + d10 nz);
//     level 3 takes every view:  S3 += Y, N3 += Nn;
//     xc = ((c0 x + c1 y) + c2 z) + c3, likewise yc, zc;  next view unless zc > 0 and all three finite;
//     u = c12 (xc / zc) + c14, v = c13 (yc / zc) + c15;  pu = rint(u / S), pv = rint(v / S) (half to even; S = 1, 2 or 4,
//     so the division is exact);  next view outside [0, W' - 1] x [0, H' - 1];
//     w = 1.0 / (zc zc);  level 2:  S2 += w Y, W2 += w, N2 += w Nn, ++n2;
//     zo = c17 * plane[m][pv][pu];  next view when zo is 0 or not finite;
//     |zc - zo| <= rel_tol zo + margin:  level 1:  S1 += w Y, W1 += w, N1 += w Nn, ++n1;
//   level = 1 when n1 > 0, else 2 when n2 > 0, else 3;
//   out = S_l / W_l per component (level 3: S3 / (double)M), rounded to fp32;
//   normal = N_l / sqrt((Nx Nx + Ny Ny) + Nz Nz) when that sum is positive and finite, else 0, rounded to fp32;
//   support = n1;  counters [1..3] count the points per level.
// f64 without contraction (the Makefile compiles this file with -ffp-contract=off), every product and sum rounded on
// its own in the order written: tests/dense_follow_ref.py reproduces every output byte for byte.
//
// One thread per point, 256-thread workgroups.  All lanes of a wave read the same view and move row, uniform loads
// that go through the scalar cache, so the only divergent memory access per view is the 2-byte gather from its plane.
// The gather is in bounds by construction: pu and pv are tested against the plane's size as doubles before they become
// indices.  A thread reads its own point (and normal) before the loop and writes it after: out_points may be points,
// out_normals may be normals.  Counters (caller-owned device memory, 4 x uint64, zeroed by the call): [0] points that
// are not finite, [1..3] points per level; summed per workgroup (wave_block.h, block_count), the only atomics.
#include "common.h"
#include "wave_block.h"

#include <stdint.h>

namespace {

using wave_block::block_count;
using wave_block::u64;

constexpr int kDepthScaleAt = 17;       // the spare camera slot that carries the unit of the view's plane
constexpr int kMoveDoubles = 12;

struct Sum {                            // one level's sums: the moved point, the weight, the moved normal
  double s[3], w, n[3];
};

template <bool NRM>
__device__ __forceinline__ void add_weighted(Sum& a, double w, const double (&Y)[3], const double (&Nn)[3]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int j = 0; j < 3; ++j) a.s[j] += w * Y[j];
  a.w += w;
  if (NRM) {
#pragma unroll
    for (int j = 0; j < 3; ++j) a.n[j] += w * Nn[j];
  }
}

template <bool NRM>
__global__ __launch_bounds__(256) void cloud_follow_kernel(
    const float* points, const float* normals, long P, const double* __restrict__ views,
    const double* __restrict__ moves, int M, const _Float16* __restrict__ planes, int Hp, int Wp, double inv_s,
    double rel_tol, double margin, float* out_points, float* out_normals, unsigned char* __restrict__ level_out,
    int* __restrict__ support_out, u64* __restrict__ counters) {
#pragma clang fp contract(off)      // the intent; what enforces it under the library's flags is the Makefile (see above)
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const bool inside = i < P;
  float xf = 0.f, yf = 0.f, zf = 0.f, nxf = 0.f, nyf = 0.f, nzf = 0.f;
  if (inside) {
    xf = points[3 * i], yf = points[3 * i + 1], zf = points[3 * i + 2];
    if (NRM) nxf = normals[3 * i], nyf = normals[3 * i + 1], nzf = normals[3 * i + 2];
  }
  const double x = (double)xf, y = (double)yf, z = (double)zf;
  const double nx = (double)nxf, ny = (double)nyf, nz = (double)nzf;
  const bool live = inside && __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z);
  Sum a1 = {}, a2 = {}, a3 = {};
  unsigned n1 = 0, n2 = 0;
  if (__ballot(live)) {                   // a wave without a point to move skips the views
    const long per = (long)Hp * Wp;
    const double wmax = (double)(Wp - 1), hmax = (double)(Hp - 1);
    for (int m = 0; m < M; ++m) {
      const double* __restrict__ d = moves + (long)m * kMoveDoubles;
      const double* __restrict__ c = views + (long)m * kCamDoubles;
      const double Y[3] = {((d[0] * x + d[1] * y) + d[2] * z) + d[3], ((d[4] * x + d[5] * y) + d[6] * z) + d[7],
                           ((d[8] * x + d[9] * y) + d[10] * z) + d[11]};
      double Nn[3] = {0.0, 0.0, 0.0};
      if (NRM) {
        Nn[0] = (d[0] * nx + d[1] * ny) + d[2] * nz;
        Nn[1] = (d[4] * nx + d[5] * ny) + d[6] * nz;
        Nn[2] = (d[8] * nx + d[9] * ny) + d[10] * nz;
      }
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        a3.s[j] += Y[j];
        if (NRM) a3.n[j] += Nn[j];
      }
      const double xc = ((c[0] * x + c[1] * y) + c[2] * z) + c[3];
      const double yc = ((c[4] * x + c[5] * y) + c[6] * z) + c[7];
      const double zc = ((c[8] * x + c[9] * y) + c[10] * z) + c[11];
      if (!live || !(zc > 0.0) || !__builtin_isfinite(xc) || !__builtin_isfinite(yc) || !__builtin_isfinite(zc))
        continue;
      const double u = c[12] * (xc / zc) + c[14];
      const double v = c[13] * (yc / zc) + c[15];
      const double pu = rint(u * inv_s), pv = rint(v * inv_s);      // inv_s = 1, 1/2 or 1/4: the product is the quotient
      if (!(pu >= 0.0 && pu <= wmax && pv >= 0.0 && pv <= hmax)) continue;     // NaN falls out
      const double w = 1.0 / (zc * zc);
      add_weighted<NRM>(a2, w, Y, Nn);
      ++n2;
      const double zo = c[kDepthScaleAt] * (double)planes[m * per + (long)(int)pv * Wp + (int)pu];
      if (zo == 0.0 || !__builtin_isfinite(zo)) continue;
      if (fabs(zc - zo) <= rel_tol * zo + margin) {
        add_weighted<NRM>(a1, w, Y, Nn);
        ++n1;
      }
    }
  }
  const int level = !live ? 0 : n1 > 0 ? 1 : n2 > 0 ? 2 : 3;
  if (inside) {
    float o[3] = {xf, yf, zf}, on[3] = {nxf, nyf, nzf};
    if (live) {
      // the level's sums, chosen value by value (a reference to one of three structs would put them into memory)
      const double wl = level == 1 ? a1.w : level == 2 ? a2.w : (double)M;
      double nl[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        o[j] = (float)((level == 1 ? a1.s[j] : level == 2 ? a2.s[j] : a3.s[j]) / wl);
        nl[j] = level == 1 ? a1.n[j] : level == 2 ? a2.n[j] : a3.n[j];
      }
      if (NRM) {
        const double q = (nl[0] * nl[0] + nl[1] * nl[1]) + nl[2] * nl[2];
        const bool ok = q > 0.0 && __builtin_isfinite(q);
        const double len = sqrt(q);
#pragma unroll
        for (int j = 0; j < 3; ++j) on[j] = ok ? (float)(nl[j] / len) : 0.f;
      }
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) out_points[3 * i + j] = o[j];
    if (NRM) {
#pragma unroll
      for (int j = 0; j < 3; ++j) out_normals[3 * i + j] = on[j];
    }
    if (level_out) level_out[i] = (unsigned char)level;
    if (support_out) support_out[i] = (int)n1;
  }
  const bool flags[4] = {inside && !live, level == 1, level == 2, level == 3};
  const int at[4] = {0, 1, 2, 3};
  block_count<4>(flags, counters, at);         // every thread of the workgroup arrives here: the loop only continues
}

}  // namespace

extern "C" int pi3_cloud_follow_views(const float* points, const float* normals, long P, const double* views,
                                      const double* moves, int M, const unsigned short* planes, int Hp, int Wp,
                                      int pixel_stride, double rel_tol, double margin, float* out_points,
                                      float* out_normals, unsigned char* level, int* support,
                                      unsigned long long* counters, void* stream) {
  if (P < 0 || P >= (1L << 39) || M < 1 || !views || !moves || !planes || !counters || (P > 0 && (!points || !out_points)) ||
      (normals == nullptr) != (out_normals == nullptr) || Hp <= 0 || Wp <= 0 ||
      (pixel_stride != 1 && pixel_stride != 2 && pixel_stride != 4) || !positive_finite(rel_tol) || !(margin >= 0.0) ||
      !__builtin_isfinite(margin)) {
    pi3_set_error("pi3_cloud_follow_views: bad arguments P=%ld M=%d (>= 1) Hp=%d Wp=%d pixel_stride=%d (1, 2 or 4) "
                  "rel_tol=%g (finite, > 0) margin=%g (finite, >= 0), a null pointer, or exactly one of normals and "
                  "out_normals", P, M, Hp, Wp, pixel_stride, rel_tol, margin);
    return PI3_ERR_ARG;
  }
  if (pi3_zero_words("pi3_cloud_follow_views", counters, 4, stream) != PI3_OK) return PI3_ERR_LAUNCH;
  if (P == 0) return PI3_OK;
  const dim3 grid((unsigned)((P + 255) / 256)), block(256);
  const double inv_s = 1.0 / (double)pixel_stride;
  if (normals)
    hipLaunchKernelGGL(cloud_follow_kernel<true>, grid, block, 0, (hipStream_t)stream, points, normals, P, views, moves, M,
                       (const _Float16*)planes, Hp, Wp, inv_s, rel_tol, margin, out_points, out_normals, level, support,
                       (u64*)counters);
  else
    hipLaunchKernelGGL(cloud_follow_kernel<false>, grid, block, 0, (hipStream_t)stream, points, normals, P, views, moves,
                       M, (const _Float16*)planes, Hp, Wp, inv_s, rel_tol, margin, out_points, out_normals, level, support,
                       (u64*)counters);
  return pi3_check_launch("cloud_follow");
}
