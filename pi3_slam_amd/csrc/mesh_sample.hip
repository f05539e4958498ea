// Area-weighted sampling of a triangle mesh's surface: the points a mesh is scored by when it is the QUERY side of a
// comparison (map_eval.py).  Deterministic: the samples are a function of the mesh, the spacing S and a 64-bit seed,
// bit for bit, and tests/mesh_eval_ref.py restates every line below in numpy.  f64 throughout, every operation rounded
// on its own (the Makefile compiles this file with -ffp-contract=off); a, b, c are the fp32 vertices of a face as f64.
//
// Hash.  mix64 is voxel_table.h's splitmix64 finaliser; + is addition modulo 2^64.
//   s0      = mix64(seed + 0x9E3779B97F4A7C15)
//   h(f)    = mix64(s0 + f)                                 the face's stream
//   u_f     = unit(mix64(h(f)))                             the face's count dither
//   r_k(f, j) = unit(mix64(h(f) + (2 j + k + 1)))           coordinate k = 0, 1 of sample j = 0, 1, ... of the face
//   unit(x) = (double)(x >> 11) * 2^-53                     in [0, 1), exact
//
// A face is DROPPED (counted, no samples) when a vertex index is outside [0, V), a coordinate is not finite, or n2 = 0:
//   ab = b - a, ac = c - a;  nx = ab.y ac.z - ab.z ac.y,  ny = ab.z ac.x - ab.x ac.z,  nz = ab.x ac.y - ab.y ac.x;
//   n2 = (nx nx + ny ny) + nz nz        (mesh_nn.hip's test; there is no cell grid here, so no quantiser range)
//
// pi3_mesh_sample_counts, per face:  l = sqrt(n2);  A = 0.5 l;  t = A / (S S) + u_f;  count = floor(t), limited to
//   2^31 - 1.  On average one sample per S^2 of area, and a triangle smaller than S^2 still gets its share.
// The host forms the exclusive prefix sum of the counts in face order (offsets, int64 [F + 1]); sample number
// offsets[f] + j is sample j of face f, so the order of the output is fixed.
// pi3_mesh_sample_points, one thread per sample: the face by binary search in offsets, then
//   r1 = r_0(f, j), r2 = r_1(f, j);  if r1 + r2 > 1:  r1 = 1 - r1, r2 = 1 - r2
//   p = (a + ab r1) + ac r2             stored as fp32
//   normal = (nx / l, ny / l, nz / l)   stored as fp32: the unit face normal, by the winding a -> b -> c
// and the face index.
#include "common.h"
#include "voxel_table.h"
#include "wave_block.h"

#include <stdint.h>

namespace {

using voxel_table::blocks_for;
using voxel_table::mix64;
using voxel_table::u64;
using wave_block::block_count;

constexpr u64 kGolden = 0x9E3779B97F4A7C15ull;

// s0 = mix64(seed + kGolden) on the host: mix64 as voxel_table.h writes it for the device
inline u64 seed_stream(u64 seed) {
  u64 x = seed + kGolden;
  x ^= x >> 30;
  x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27;
  x *= 0x94d049bb133111ebull;
  x ^= x >> 31;
  return x;
}

__device__ __forceinline__ double unit(u64 x) { return (double)(x >> 11) * 0x1.0p-53; }

struct Face {
  double ax, ay, az, abx, aby, abz, acx, acy, acz, nx, ny, nz, n2;
};

// false = drop
__device__ __forceinline__ bool load_face(const float* __restrict__ vertices, long V, const int* __restrict__ faces,
                                          long f, Face& t) {
#pragma clang fp contract(off)      // the intent; what enforces it under the library's flags is the Makefile
  const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
  if (!(i0 >= 0 && i0 < V && i1 >= 0 && i1 < V && i2 >= 0 && i2 < V)) return false;
  float v[9];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    v[a] = vertices[3L * i0 + a];
    v[3 + a] = vertices[3L * i1 + a];
    v[6 + a] = vertices[3L * i2 + a];
  }
  bool finite = true;
#pragma unroll
  for (int j = 0; j < 9; ++j) finite = finite && __builtin_isfinite(v[j]);
  if (!finite) return false;
  t.ax = (double)v[0], t.ay = (double)v[1], t.az = (double)v[2];
  t.abx = (double)v[3] - t.ax, t.aby = (double)v[4] - t.ay, t.abz = (double)v[5] - t.az;
  t.acx = (double)v[6] - t.ax, t.acy = (double)v[7] - t.ay, t.acz = (double)v[8] - t.az;
  t.nx = t.aby * t.acz - t.abz * t.acy;
  t.ny = t.abz * t.acx - t.abx * t.acz;
  t.nz = t.abx * t.acy - t.aby * t.acx;
  t.n2 = (t.nx * t.nx + t.ny * t.ny) + t.nz * t.nz;
  return t.n2 != 0.0;               // fp32 inputs: n2 below 2^518, never inf or NaN
}

// counters[0] += dropped faces
__global__ __launch_bounds__(256) void mesh_sample_counts_kernel(const float* __restrict__ vertices, long V,
                                                                 const int* __restrict__ faces, long F, double s2, u64 s0,
                                                                 long long* __restrict__ counts,
                                                                 u64* __restrict__ counters) {
#pragma clang fp contract(off)
  const long f = (long)blockIdx.x * 256 + threadIdx.x;
  bool dropped = false;
  if (f < F) {
    Face t;
    long long n = 0;
    if (load_face(vertices, V, faces, f, t)) {
      const double area = 0.5 * sqrt(t.n2);
      const double x = area / s2 + unit(mix64(mix64(s0 + (u64)f)));
      n = x < 2147483647.0 ? (long long)floor(x) : 2147483647ll;
    } else {
      dropped = true;
    }
    counts[f] = n;
  }
  const bool flags[1] = {dropped};
  const int at[1] = {0};
  block_count<1>(flags, counters, at);
}

__global__ __launch_bounds__(256) void mesh_sample_points_kernel(const float* __restrict__ vertices, long V,
                                                                 const int* __restrict__ faces, long F,
                                                                 const long long* __restrict__ offsets, long n, u64 s0,
                                                                 float* __restrict__ points, int* __restrict__ face_out,
                                                                 float* __restrict__ normals) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  long lo = 0, hi = F;                       // the face with offsets[f] <= i < offsets[f + 1]
  while (hi - lo > 1) {
    const long mid = lo + (hi - lo) / 2;
    if (offsets[mid] <= (long long)i) lo = mid; else hi = mid;
  }
  const long f = lo;
  const long long j = (long long)i - offsets[f];
  Face t;
  float px = 0.0f, py = 0.0f, pz = 0.0f, ux = 0.0f, uy = 0.0f, uz = 0.0f;
  int fo = -1;
  // offsets that are not the prefix sums of this mesh's counts name a dropped face or a sample past a face's count:
  // such a row gets zeros and face -1
  if (j >= 0 && j < offsets[f + 1] - offsets[f] && load_face(vertices, V, faces, f, t)) {
    const u64 h = mix64(s0 + (u64)f);
    double r1 = unit(mix64(h + (2ull * (u64)j + 1ull)));
    double r2 = unit(mix64(h + (2ull * (u64)j + 2ull)));
    if (r1 + r2 > 1.0) {
      r1 = 1.0 - r1;
      r2 = 1.0 - r2;
    }
    const double l = sqrt(t.n2);
    px = (float)((t.ax + t.abx * r1) + t.acx * r2);
    py = (float)((t.ay + t.aby * r1) + t.acy * r2);
    pz = (float)((t.az + t.abz * r1) + t.acz * r2);
    ux = (float)(t.nx / l), uy = (float)(t.ny / l), uz = (float)(t.nz / l);
    fo = (int)f;
  }
  points[3 * i] = px, points[3 * i + 1] = py, points[3 * i + 2] = pz;
  normals[3 * i] = ux, normals[3 * i + 1] = uy, normals[3 * i + 2] = uz;
  face_out[i] = fo;
}

}  // namespace

extern "C" int pi3_mesh_sample_counts(const float* vertices, long V, const int* faces, long F, double spacing,
                                      unsigned long long seed, long long* counts, unsigned long long* counters,
                                      void* stream) {
  const double s2 = spacing * spacing;
  if (!counters || V < 0 || V >= (1L << 31) || F < 0 || F >= (1L << 31) || (F > 0 && (!faces || !counts)) ||
      (V > 0 && !vertices) || !positive_finite(spacing) || !positive_finite(s2)) {
    pi3_set_error("pi3_mesh_sample_counts: bad arguments V=%ld F=%ld (0 <= V, F < 2^31) spacing=%g (finite, > 0, and "
                  "so its square), or a null pointer", V, F, spacing);
    return PI3_ERR_ARG;
  }
  if (pi3_zero_words("pi3_mesh_sample_counts", counters, 4, stream) != PI3_OK) return PI3_ERR_LAUNCH;
  if (F > 0)
    hipLaunchKernelGGL(mesh_sample_counts_kernel, dim3(blocks_for(F)), dim3(256), 0, (hipStream_t)stream, vertices, V,
                       faces, F, s2, seed_stream(seed), counts, (u64*)counters);
  return pi3_check_launch("mesh_sample_counts");
}

extern "C" int pi3_mesh_sample_points(const float* vertices, long V, const int* faces, long F, const long long* offsets,
                                      long n, unsigned long long seed, float* points, int* face, float* normals,
                                      void* stream) {
  if (V < 0 || V >= (1L << 31) || F < 1 || F >= (1L << 31) || !faces || !offsets || (V > 0 && !vertices) || n < 0 ||
      n >= (1L << 31) || (n > 0 && (!points || !face || !normals))) {
    pi3_set_error("pi3_mesh_sample_points: bad arguments V=%ld (0 <= V < 2^31) F=%ld (1 <= F < 2^31) n=%ld "
                  "(0 <= n < 2^31), or a null pointer", V, F, n);
    return PI3_ERR_ARG;
  }
  if (n > 0)
    hipLaunchKernelGGL(mesh_sample_points_kernel, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, vertices, V,
                       faces, F, offsets, n, seed_stream(seed), points, face, normals);
  return pi3_check_launch("mesh_sample_points");
}
