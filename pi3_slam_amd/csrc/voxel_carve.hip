// Carving the fused dense map with depth keyframes: a per-voxel decision on the world-frame hash table
// (voxel_table.h), taken after every chunk cloud is fused and before the cleaner (voxel_clean.hip) and the extraction.
//
// Stage 1 keeps a few sub-sampled fp16 depth planes per chunk (dense_filter.hip: pi3_dense_depth_planes).  Here every
// voxel is projected into every such view, of every chunk:
//   X        the extraction's centroid voxel_size (k + U / (W 2^24)), f64, rounded to fp32 and widened again (so that an
//            oracle can start from the extracted rows);
//   view m   20 doubles in render.hip's camera layout: rigid world->camera 3x4 row-major, fx fy cx cy, the ortho flag
//            (0 here), and in spare slot 17 the depth scale s of the view's chunk (a plane is in chunk units);
//   xc = ((r00 x + r01 y) + r02 z) + t0, likewise yc, zc;  no vote unless zc > 0 and all three finite;
//   u = fx (xc / zc) + cx, v = fy (yc / zc) + cy;  pu = rint(u / S), pv = rint(v / S) (half to even; S = 1, 2 or 4, so
//   the division is exact);  no vote outside [0, W' - 1] x [0, H' - 1];
//   zo = s * plane[m][pv][pu];  no vote when zo is 0 or not finite;
//   r = zc - zo, lim = rel_tol zo + margin:  |r| <= lim agrees;  r < -lim conflicts (the view measured a surface behind
//   the voxel: it looked through it);  else the voxel is occluded in that view: no vote;
//   carved = conflict >= min_conflicts && conflict > agree.
// f64 without contraction (the Makefile compiles this file with -ffp-contract=off), every product and sum rounded on
// its own in the order written: tests/dense_carve_ref.py reproduces carved, agree, conflict and the counters byte for
// byte.
//
// One thread per slot, 256-thread workgroups; the table is read only.  The loop over the views is bounded by M; all
// lanes of a wave read the same camera row, a uniform load that goes through the scalar cache, so the only divergent
// memory access per view is the 2-byte gather from its plane.  The gather is in bounds by construction: pu and pv are
// tested against the plane's size as doubles before they become indices.  Counters (caller-owned device memory,
// 4 x uint64, zeroed by the call): [0] occupied slots, [1] carved, [2] occupied slots no view voted on; summed per
// workgroup (wave_block.h, block_count).
#include "common.h"
#include "voxel_table.h"
#include "wave_block.h"

#include <stdint.h>

namespace {

using namespace voxel_table;
using wave_block::block_count;

constexpr int kDepthScaleAt = 17;       // the spare camera slot that carries the view's depth scale

__global__ __launch_bounds__(256) void voxel_carve_kernel(
    const u64* __restrict__ table, long capacity, double vsize, const double* __restrict__ views, int M,
    const _Float16* __restrict__ planes, int Hp, int Wp, double inv_s, double rel_tol, double margin,
    unsigned min_conflicts, unsigned char* __restrict__ carved, unsigned* __restrict__ agree_out,
    unsigned* __restrict__ conflict_out, u64* __restrict__ counters) {
#pragma clang fp contract(off)      // the intent; what enforces it under the library's flags is the Makefile (see above)
  const long s = (long)blockIdx.x * 256 + threadIdx.x;
  bool occupied = false;
  double x = 0.0, y = 0.0, z = 0.0;
  if (s < capacity) {
    const u64* q = table + 8 * s;
    occupied = q[0] != kEmpty;
    if (occupied) {
      x = (double)(float)(vsize * slot_centre(q, 0));
      y = (double)(float)(vsize * slot_centre(q, 1));
      z = (double)(float)(vsize * slot_centre(q, 2));
    }
  }
  unsigned agree = 0, conflict = 0;
  if (__ballot(occupied)) {               // a wave without a voxel skips the views
    const long per = (long)Hp * Wp;
    const double wmax = (double)(Wp - 1), hmax = (double)(Hp - 1);
    for (int m = 0; m < M; ++m) {
      const double* __restrict__ c = views + (long)m * kCamDoubles;
      const double xc = ((c[0] * x + c[1] * y) + c[2] * z) + c[3];
      const double yc = ((c[4] * x + c[5] * y) + c[6] * z) + c[7];
      const double zc = ((c[8] * x + c[9] * y) + c[10] * z) + c[11];
      if (!occupied || !(zc > 0.0) || !__builtin_isfinite(xc) || !__builtin_isfinite(yc) || !__builtin_isfinite(zc))
        continue;
      const double u = c[12] * (xc / zc) + c[14];
      const double v = c[13] * (yc / zc) + c[15];
      const double pu = rint(u * inv_s), pv = rint(v * inv_s);      // inv_s = 1, 1/2 or 1/4: the product is the quotient
      if (!(pu >= 0.0 && pu <= wmax && pv >= 0.0 && pv <= hmax)) continue;     // NaN falls out
      const double zo = c[kDepthScaleAt] * (double)planes[m * per + (long)(int)pv * Wp + (int)pu];
      if (zo == 0.0 || !__builtin_isfinite(zo)) continue;
      const double r = zc - zo, lim = rel_tol * zo + margin;
      if (fabs(r) <= lim)
        ++agree;
      else if (r < -lim)
        ++conflict;
    }
  }
  const bool cut = occupied && conflict >= min_conflicts && conflict > agree;
  if (s < capacity) {
    carved[s] = cut ? 1 : 0;
    if (agree_out) agree_out[s] = agree;
    if (conflict_out) conflict_out[s] = conflict;
  }
  const bool flags[3] = {occupied, cut, occupied && agree + conflict == 0};
  const int at[3] = {0, 1, 2};
  block_count<3>(flags, counters, at);         // every thread of the workgroup arrives here: the loop only continues
}

}  // namespace

extern "C" int pi3_voxel_carve(const void* table, long capacity, double voxel_size, const double* views, int M,
                               const unsigned short* planes, int Hp, int Wp, int pixel_stride, double rel_tol,
                               double margin, int min_conflicts, unsigned char* carved, unsigned* agree,
                               unsigned* conflict, unsigned long long* counters, void* stream) {
  if (!table || !pow2(capacity) || !carved || !counters || M < 0 || (M > 0 && (!views || !planes)) || Hp <= 0 ||
      Wp <= 0 || (pixel_stride != 1 && pixel_stride != 2 && pixel_stride != 4) || !positive_finite(voxel_size) ||
      !positive_finite(rel_tol) || !(margin >= 0.0) || !__builtin_isfinite(margin) || min_conflicts < 1) {
    pi3_set_error("pi3_voxel_carve: bad arguments capacity=%ld M=%d Hp=%d Wp=%d pixel_stride=%d (1, 2 or 4) "
                  "voxel_size=%g rel_tol=%g (finite, > 0) margin=%g (finite, >= 0) min_conflicts=%d (>= 1), or a null "
                  "pointer", capacity, M, Hp, Wp, pixel_stride, voxel_size, rel_tol, margin, min_conflicts);
    return PI3_ERR_ARG;
  }
  if (pi3_zero_words("pi3_voxel_carve", counters, 4, stream) != PI3_OK) return PI3_ERR_LAUNCH;
  hipLaunchKernelGGL(voxel_carve_kernel, dim3(blocks_for(capacity)), dim3(256), 0, (hipStream_t)stream,
                     (const u64*)table, capacity, voxel_size, views, M, (const _Float16*)planes, Hp, Wp,
                     1.0 / (double)pixel_stride, rel_tol, margin, (unsigned)min_conflicts, carved, agree, conflict,
                     (u64*)counters);
  return pi3_check_launch("voxel_carve");
}
