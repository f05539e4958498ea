// Multi-view depth consistency of one chunk's dense pointmaps: a pixel mask for the dense voxel map (voxel.hip).
//
// A pointmap network puts confident points into free space (depth discontinuities, specular surfaces, single frames).
// Every candidate pixel of frame i is projected into the neighbouring frames j = i +- s * stride, s = 1..radius, of the
// same chunk and compared with the depth frame j predicted at that pixel:
//   agree     |zc - zo| <= rel_tol * zo      the neighbour saw the same surface
//   conflict  zc - zo  < -rel_tol * zo       the point lies in front of what j saw there: j looked through it
//   neither   the point is behind j's surface (occluded): no vote
// and is kept when agree >= min_views && conflict <= agree.
//
// Two passes:
//   A  (coalesced) candidate test -> zplane[i] = local z of a candidate, else 0.  A candidate has mask != 0, conf above
//      the threshold, three finite world coordinates and a finite positive local z.
//   B  one thread per source pixel.  Neighbouring source pixels project to neighbouring target pixels, so the one 4-byte
//      gather per neighbour from zplane is coherent; without pass A it would be three strided gathers (masks, conf,
//      local_points).  A frame's pose and intrinsics are wave-uniform unless the wave straddles two frames (H W is not a
//      multiple of 64): the uniform wave reads them through the scalar cache, the straddling wave per lane; both run
//      the same arithmetic.
//
// All arithmetic is fp32 without contraction, every product and sum rounded on its own in the order written below, so
// a numpy float32 oracle (tests/dense_consistency_ref.py) reproduces mask, counts and stats byte for byte.  The Makefile
// compiles this file with -ffp-contract=off: under the library's -ffp-contract=fast the compiler ignores
// `#pragma clang fp contract(off)` and fuses the rotation's and the projection's multiply-adds.
//
// Depth keyframes (pi3_dense_depth_planes): the candidate test of pass A on every `every`-th frame and every
// `pixel_stride`-th row and column, the local z written as fp16 (round to nearest even; 0 for a non-candidate and for a
// value that rounds to 0 or inf).  Stage 2 carves the fused map with them (voxel_carve.hip);
// tests/dense_carve_ref.py reproduces the planes byte for byte.
#include "common.h"
#include "wave_block.h"

#include <stdint.h>

namespace {

typedef unsigned long long u64;

// the candidate test of both entry points: mask, confidence, a finite world point, a finite positive local z
__device__ __forceinline__ float candidate_z(const float* __restrict__ points, const float* __restrict__ local_points,
                                             const float* __restrict__ conf, const unsigned char* __restrict__ masks,
                                             long i, float conf_thr) {
  if ((!masks || masks[i]) && (!conf || conf[i] > conf_thr)) {
    const float px = points[3 * i], py = points[3 * i + 1], pz = points[3 * i + 2];
    const float lz = local_points[3 * i + 2];
    if (__builtin_isfinite(px) && __builtin_isfinite(py) && __builtin_isfinite(pz) && __builtin_isfinite(lz) &&
        lz > 0.0f)
      return lz;
  }
  return 0.0f;
}

__global__ __launch_bounds__(256) void dense_candidates_kernel(
    const float* __restrict__ points, const float* __restrict__ local_points, const float* __restrict__ conf,
    const unsigned char* __restrict__ masks, long n, float conf_thr, float* __restrict__ zplane) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  zplane[i] = candidate_z(points, local_points, conf, masks, i, conf_thr);
}

// One thread per sample (k, y', x') of the planes: frame k * every, pixel (S y', S x').  fp16 bits through _Float16
// (v_cvt_f16_f32: round to nearest even, overflow to inf, underflow through the subnormals to 0).
__global__ __launch_bounds__(256) void dense_depth_planes_kernel(
    const float* __restrict__ points, const float* __restrict__ local_points, const float* __restrict__ conf,
    const unsigned char* __restrict__ masks, long n_out, int H, int W, int Hp, int Wp, int every, int S, float conf_thr,
    unsigned short* __restrict__ depth, u64* __restrict__ count) {
  const long o = (long)blockIdx.x * 256 + threadIdx.x;
  unsigned nz = 0;
  if (o < n_out) {
    const long per = (long)Hp * Wp;
    const long k = o / per, r = o - k * per;
    const int yp = (int)(r / Wp), xp = (int)(r - (long)yp * Wp);
    const long i = (k * every * H + (long)yp * S) * W + (long)xp * S;       // yp S <= H - 1, xp S <= W - 1
    const float z = candidate_z(points, local_points, conf, masks, i, conf_thr);
    const _Float16 h = (_Float16)z;
    unsigned short bits = __builtin_bit_cast(unsigned short, h);
    if (bits == 0x7C00u) bits = 0;                                         // rounded to inf: no opinion
    depth[o] = bits;
    nz = bits != 0;
  }
  wave_block::block_sum(nz, count);
}

enum { kNoVote = 0, kAgree = 1, kConflict = 2 };

// The vote of view j (pose P = cam->world 4x4 row-major, K = fx fy cx cy, zj = its depth plane) on the world point X.
__device__ __forceinline__ int vote(const float* __restrict__ P, const float* __restrict__ K,
                                    const float* __restrict__ zj, int H, int W, float X, float Y, float Z,
                                    float rel_tol) {
#pragma clang fp contract(off)      // the intent; what enforces it under the library's flags is the Makefile (see above)
  const float dx = X - P[3], dy = Y - P[7], dz = Z - P[11];
  const float xc = (P[0] * dx + P[4] * dy) + P[8] * dz;      // R^T d: the head's rotation is SO(3), no inverse
  const float yc = (P[1] * dx + P[5] * dy) + P[9] * dz;
  const float zc = (P[2] * dx + P[6] * dy) + P[10] * dz;
  if (!(zc > 0.0f) || !__builtin_isfinite(xc) || !__builtin_isfinite(yc) || !__builtin_isfinite(zc)) return kNoVote;
  const float u = K[0] * (xc / zc) + K[2];
  const float v = K[1] * (yc / zc) + K[3];
  const float pu = rintf(u), pv = rintf(v);
  if (!(pu >= 0.0f && pu <= (float)(W - 1) && pv >= 0.0f && pv <= (float)(H - 1))) return kNoVote;     // NaN falls out
  const float zo = zj[(long)(int)pv * W + (int)pu];
  if (zo == 0.0f) return kNoVote;
  const float r = zc - zo, lim = rel_tol * zo;
  return fabsf(r) <= lim ? kAgree : (r < -lim ? kConflict : kNoVote);
}

__global__ __launch_bounds__(256) void dense_consistency_kernel(
    const float* __restrict__ points, const float* __restrict__ zplane, const float* __restrict__ poses,
    const float* __restrict__ fxfycxcy, long n, int N, int H, int W, int radius, int stride, int min_views,
    float rel_tol, unsigned char* __restrict__ out_mask, unsigned char* __restrict__ counts,
    u64* __restrict__ stats) {
  const long HW = (long)H * W;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const bool in = i < n;
  const int frame = (int)((in ? i : n - 1) / HW);
  const bool cand = in && zplane[i] != 0.0f;
  int agree = 0, conflict = 0;
  float X = 0.0f, Y = 0.0f, Z = 0.0f;
  if (cand) {
    X = points[3 * i];
    Y = points[3 * i + 1];
    Z = points[3 * i + 2];
  }
  const int first = __builtin_amdgcn_readfirstlane(frame);
  if (__all(frame == first)) {
    // the whole wave looks at one frame: j, the pose and the intrinsics are scalars
    for (int s = 1; s <= radius; ++s) {
#pragma unroll
      for (int sg = -1; sg <= 1; sg += 2) {
        const long j = (long)first + (long)sg * s * stride;
        if (j < 0 || j >= N) continue;
        const int c = cand ? vote(poses + 16 * j, fxfycxcy + 4 * j, zplane + j * HW, H, W, X, Y, Z, rel_tol) : kNoVote;
        agree += c == kAgree;
        conflict += c == kConflict;
      }
    }
  } else if (cand) {
    for (int s = 1; s <= radius; ++s) {
#pragma unroll
      for (int sg = -1; sg <= 1; sg += 2) {
        const long j = (long)frame + (long)sg * s * stride;
        if (j < 0 || j >= N) continue;
        const int c = vote(poses + 16 * j, fxfycxcy + 4 * j, zplane + j * HW, H, W, X, Y, Z, rel_tol);
        agree += c == kAgree;
        conflict += c == kConflict;
      }
    }
  }
  const bool keep = cand && agree >= min_views && conflict <= agree;
  if (in) {
    out_mask[i] = keep ? 1 : 0;
    if (counts) {
      uchar2 c;
      c.x = (unsigned char)(agree > 255 ? 255 : agree);
      c.y = (unsigned char)(conflict > 255 ? 255 : conflict);
      reinterpret_cast<uchar2*>(counts)[i] = c;
    }
  }
  const u64 nc = __ballot(cand), nk = __ballot(keep);
  if ((threadIdx.x & 63) == 0) {
    if (nc) atomicAdd(stats + 0, (u64)__popcll(nc));
    if (nk) atomicAdd(stats + 1, (u64)__popcll(nk));
  }
}

}  // namespace

extern "C" int pi3_dense_consistency(const float* points, const float* local_points, const float* conf,
                                     const unsigned char* masks, const float* poses, const float* fxfycxcy, int N,
                                     int H, int W, float conf_logit_thr, int radius, int stride, int min_views,
                                     float rel_tol, float* zplane, unsigned char* out_mask, unsigned char* counts,
                                     unsigned long long* stats, void* stream) {
  const long n = (long)N * H * W;
  if (!points || !local_points || !poses || !fxfycxcy || !zplane || !out_mask || !stats || N < 0 || H <= 0 ||
      W <= 0 || n > 0x7fffffffL || radius < 1 || radius > 16 || stride < 1 || min_views < 1 ||
      min_views > 2 * radius || !positive_finite(rel_tol)) {
    pi3_set_error("pi3_dense_consistency: bad arguments N=%d H=%d W=%d radius=%d (1..16) stride=%d (>= 1) "
                  "min_views=%d (1..2 radius) rel_tol=%g (finite, > 0), or a null pointer",
                  N, H, W, radius, stride, min_views, (double)rel_tol);
    return PI3_ERR_ARG;
  }
  if (pi3_zero_words("pi3_dense_consistency", stats, 2, stream) != PI3_OK) return PI3_ERR_LAUNCH;
  if (N == 0) return PI3_OK;
  const unsigned nb = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(dense_candidates_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, points, local_points, conf,
                     masks, n, conf_logit_thr, zplane);
  hipLaunchKernelGGL(dense_consistency_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, points,
                     (const float*)zplane, poses, fxfycxcy, n, N, H, W, radius, stride, min_views, rel_tol, out_mask,
                     counts, (u64*)stats);
  return pi3_check_launch("dense_consistency");
}

extern "C" int pi3_dense_depth_planes(const float* points, const float* local_points, const float* conf,
                                      const unsigned char* masks, int N, int H, int W, float conf_logit_thr, int every,
                                      int pixel_stride, unsigned short* depth, unsigned long long* count, void* stream) {
  const long n = (long)N * H * W;
  if (!points || !local_points || !depth || !count || N < 0 || H <= 0 || W <= 0 || n > 0x7fffffffL || every < 1 ||
      (pixel_stride != 1 && pixel_stride != 2 && pixel_stride != 4)) {
    pi3_set_error("pi3_dense_depth_planes: bad arguments N=%d H=%d W=%d every=%d (>= 1) pixel_stride=%d (1, 2 or 4), or "
                  "a null pointer", N, H, W, every, pixel_stride);
    return PI3_ERR_ARG;
  }
  if (pi3_zero_words("pi3_dense_depth_planes", count, 1, stream) != PI3_OK) return PI3_ERR_LAUNCH;
  if (N == 0) return PI3_OK;
  const int Nk = (int)(((long)N + every - 1) / every);
  const int Hp = (H + pixel_stride - 1) / pixel_stride, Wp = (W + pixel_stride - 1) / pixel_stride;
  const long n_out = (long)Nk * Hp * Wp;
  hipLaunchKernelGGL(dense_depth_planes_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     points, local_points, conf, masks, n_out, H, W, Hp, Wp, every, pixel_stride, conf_logit_thr, depth,
                     (u64*)count);
  return pi3_check_launch("dense_depth_planes");
}
