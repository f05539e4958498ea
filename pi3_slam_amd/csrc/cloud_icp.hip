// The normal equations of one ICP step between two point clouds: the reduction that follows pi3_cloud_nearest in
// map_eval.icp_refine (the alignment of a dense map on its reference cloud is refined on the geometry before scoring).
//
// Pair i = (p, q): p = queries[i] (the estimate, already moved by the current transform: the rows the search was given),
// q = points[idx[i]].  With x = p - centre and e = p - q (f64) the small motion about `centre` is
//   p' = p + w x x + l x + t,   J = [ -[x]x | x | I ]  (3 x 7; parameters w (3), l, t (3)).
//   mode 0 (point to point):   A += J^T J,  b += J^T e,  r2 += e.e
//   mode 1, 2 (point to plane): j = J^T n = (x x n, x.n, n),  r = n.e:   A += j j^T,  b += j r,  r2 += r r
// n: mode 1 normals[idx[i]] (the target's), mode 2 Rn normals[i] (the source's, rotated by the current transform);
// normalised in f64.  J^T J is written out: ww = |x|^2 I - x x^T, wl = 0, wt = [x]x, ll = x.x, lt = x, tt = I.
// A pair takes part when 0 <= idx[i] < n, d2[i] <= trim_dist^2 (inclusive) and, in modes 1 and 2, its normal has a
// finite non-zero length.  Every product and sum rounds on its own (the Makefile compiles this file with
// -ffp-contract=off).
//
// The sums are bitwise reproducible: no floating-point atomics.  A workgroup of 256 threads covers kSpan consecutive
// queries, lane t the queries t, t + 256, ... of the span in that order, 37 sums in f64 registers; a fixed
// xor-butterfly over the wave; the four waves through LDS as ((w0 + w1) + w2) + w3; one row of 40 doubles per workgroup
// with plain stores into the caller's workspace.  A second launch of one workgroup adds the rows: slice s of kSlices
// takes rows s, s + kSlices, ... in order, then the slices are added in order.  The grid depends on m alone.
// The counters are integers: per-lane counts, one atomic per workgroup and counter (wave_block::block_sum).
#include "common.h"
#include "wave_block.h"

#include <stdint.h>

namespace {

using wave_block::block_sum;
using wave_block::u64;

constexpr int kPerLane = 16;
constexpr long kSpan = 256 * kPerLane;   // queries per workgroup; ops.CLOUD_ICP_SPAN restates it
constexpr int kSums = 37;                // A (28), b (7), r2, sum of e.e
constexpr int kRow = 40;                 // doubles per row of partials and in `out`
constexpr int kSlices = 6;               // kSlices * kRow <= 256 threads of the second launch

struct PairFrame {
  double c[3];       // centre
  double R[9];       // Rn, row-major
  double trim2;
  int rotate;        // mode 2 with Rn given
};

template <int MODE>
__global__ __launch_bounds__(256) void pair_equations_kernel(const float* __restrict__ queries, long m,
                                                             const float* __restrict__ points, long n,
                                                             const int* __restrict__ idx, const double* __restrict__ d2,
                                                             const float* __restrict__ normals, PairFrame f,
                                                             double* __restrict__ partials, u64* __restrict__ counters) {
#pragma clang fp contract(off)      // the intent; what enforces it under the library's flags is the Makefile
  __shared__ double wave_part[4][kRow];
  double acc[kSums];
#pragma unroll
  for (int j = 0; j < kSums; ++j) acc[j] = 0.0;
  unsigned used = 0, unmatched = 0, trimmed = 0, rejected = 0;
  const int tid = (int)threadIdx.x;
  const long base = (long)blockIdx.x * kSpan + tid;
  for (int k = 0; k < kPerLane; ++k) {
    const long i = base + (long)k * 256;
    if (i >= m) break;
    // the pair's class first, in branches that touch no sum: the 37 accumulators then cross one branch per pair
    const int row = idx[i];
    const bool matched = row >= 0 && (long)row < n;
    bool near = false, good = true;
    double n0 = 0.0, n1 = 0.0, n2 = 0.0;
    if (matched) {
      near = d2[i] <= f.trim2;
      if (MODE != 0 && near) {
        const float* __restrict__ nr = normals + 3 * (MODE == 1 ? (long)row : i);
        double a0 = (double)nr[0], a1 = (double)nr[1], a2 = (double)nr[2];
        if (MODE == 2 && f.rotate) {
          const double r0 = (f.R[0] * a0 + f.R[1] * a1) + f.R[2] * a2;
          const double r1 = (f.R[3] * a0 + f.R[4] * a1) + f.R[5] * a2;
          const double r2 = (f.R[6] * a0 + f.R[7] * a1) + f.R[8] * a2;
          a0 = r0, a1 = r1, a2 = r2;
        }
        const double l2 = (a0 * a0 + a1 * a1) + a2 * a2;
        good = l2 > 0.0 && l2 < __builtin_inf();       // not zero, NaN or inf
        if (good) {
          const double l = sqrt(l2);
          n0 = a0 / l, n1 = a1 / l, n2 = a2 / l;
        }
      }
    }
    unmatched += !matched;
    trimmed += matched && !near;
    rejected += matched && near && !good;
    if (!(matched && near && good)) continue;
    ++used;
    const double p0 = (double)queries[3 * i], p1 = (double)queries[3 * i + 1], p2 = (double)queries[3 * i + 2];
    const float* __restrict__ qr = points + 3 * (long)row;
    const double e0 = p0 - (double)qr[0], e1 = p1 - (double)qr[1], e2 = p2 - (double)qr[2];
    const double x0 = p0 - f.c[0], x1 = p1 - f.c[1], x2 = p2 - f.c[2];
    const double ee = (e0 * e0 + e1 * e1) + e2 * e2;
    acc[36] += ee;
    if (MODE == 0) {
      // upper triangle, row-major: row 0 at 0..6, row 1 at 7..12, row 2 at 13..17, row 3 at 18..21, 4 at 22..24, 5 at
      // 25..26, 6 at 27.  Entries that are zero for every pair are never touched.
      const double s0 = x0 * x0, s1 = x1 * x1, s2 = x2 * x2;
      acc[0] += s1 + s2;
      acc[1] -= x0 * x1;
      acc[2] -= x0 * x2;
      acc[5] -= x2;
      acc[6] += x1;
      acc[7] += s0 + s2;
      acc[8] -= x1 * x2;
      acc[10] += x2;
      acc[12] -= x0;
      acc[13] += s0 + s1;
      acc[15] -= x1;
      acc[16] += x0;
      acc[18] += (s0 + s1) + s2;
      acc[19] += x0;
      acc[20] += x1;
      acc[21] += x2;
      acc[22] += 1.0;
      acc[25] += 1.0;
      acc[27] += 1.0;
      acc[28] += x1 * e2 - x2 * e1;
      acc[29] += x2 * e0 - x0 * e2;
      acc[30] += x0 * e1 - x1 * e0;
      acc[31] += (x0 * e0 + x1 * e1) + x2 * e2;
      acc[32] += e0;
      acc[33] += e1;
      acc[34] += e2;
      acc[35] += ee;
    } else {
      const double j[7] = {x1 * n2 - x2 * n1, x2 * n0 - x0 * n2, x0 * n1 - x1 * n0, (x0 * n0 + x1 * n1) + x2 * n2,
                           n0, n1, n2};
      const double r = (n0 * e0 + n1 * e1) + n2 * e2;
      int t = 0;
#pragma unroll
      for (int a = 0; a < 7; ++a) {
#pragma unroll
        for (int b = a; b < 7; ++b) acc[t++] += j[a] * j[b];
      }
#pragma unroll
      for (int a = 0; a < 7; ++a) acc[28 + a] += j[a] * r;
      acc[35] += r * r;
    }
  }
#pragma unroll
  for (int j = 0; j < kSums; ++j) acc[j] = wave_sum_f64(acc[j]);
  if ((tid & 63) == 0) {
#pragma unroll
    for (int j = 0; j < kSums; ++j) wave_part[tid >> 6][j] = acc[j];
  }
  __syncthreads();
  if (tid < kRow)
    partials[(long)blockIdx.x * kRow + tid] =
        tid < kSums ? ((wave_part[0][tid] + wave_part[1][tid]) + wave_part[2][tid]) + wave_part[3][tid] : 0.0;
  block_sum(used, counters + 0);
  __syncthreads();
  block_sum(unmatched, counters + 1);
  __syncthreads();
  block_sum(trimmed, counters + 2);
  __syncthreads();
  block_sum(rejected, counters + 3);
}

// one workgroup: out[c] = the sum over the rows of partials[.][c], in an order that depends on `rows` alone
__global__ __launch_bounds__(256) void pair_equations_sum_kernel(const double* __restrict__ partials, long rows,
                                                                 double* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double part[kSlices][kRow];
  const int tid = (int)threadIdx.x, s = tid / kRow, c = tid % kRow;
  if (s < kSlices) {
    double v = 0.0;
    for (long r = s; r < rows; r += kSlices) v += partials[r * kRow + c];
    part[s][c] = v;
  }
  __syncthreads();
  if (tid < kRow) {
    double v = part[0][tid];
#pragma unroll
    for (int k = 1; k < kSlices; ++k) v += part[k][tid];
    out[tid] = v;
  }
}

inline bool finite_all(const double* v, int count) {
  for (int k = 0; k < count; ++k)
    if (!__builtin_isfinite(v[k])) return false;
  return true;
}

}  // namespace

extern "C" int pi3_cloud_pair_equations(const float* queries, long m, const float* points, long n, const int* idx,
                                        const double* d2, double trim_dist, const double* centre, const float* normals,
                                        int normals_of, const double* Rn, double* partials, long partial_rows,
                                        double* out, unsigned long long* counters, void* stream) {
  if (m < 0 || n < 0 || n >= (1L << 31) || normals_of < 0 || normals_of > 2 || !out || !counters || !centre ||
      !finite_all(centre, 3) || !(trim_dist >= 0.0 && __builtin_isfinite(trim_dist)) || partial_rows < 0 ||
      (m > 0 && (!queries || !idx || !d2 || !partials || (n > 0 && !points))) ||
      (m > 0 && normals_of == 1 && n > 0 && !normals) || (m > 0 && normals_of == 2 && !normals) ||
      (normals_of == 2 && Rn && !finite_all(Rn, 9))) {
    pi3_set_error("pi3_cloud_pair_equations: bad arguments m=%ld (>= 0) n=%ld (0 <= n < 2^31) normals_of=%d (0, 1, 2) "
                  "trim_dist=%g (finite, >= 0), a centre or Rn that is not finite, or a null pointer", m, n, normals_of,
                  trim_dist);
    return PI3_ERR_ARG;
  }
  const long rows = (m + kSpan - 1) / kSpan;
  if (rows > partial_rows) {
    pi3_set_error("pi3_cloud_pair_equations: m=%ld needs %ld rows of %d doubles in partials, the caller has %ld", m,
                  rows, kRow, partial_rows);
    return PI3_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  if (pi3_zero_words("pi3_cloud_pair_equations", counters, 4, stream) != PI3_OK ||
      (m == 0 && pi3_zero_words("pi3_cloud_pair_equations", out, kRow, stream) != PI3_OK))
    return PI3_ERR_LAUNCH;
  if (m > 0) {
    PairFrame f;
    for (int k = 0; k < 3; ++k) f.c[k] = centre[k];
    f.rotate = normals_of == 2 && Rn;
    for (int k = 0; k < 9; ++k) f.R[k] = f.rotate ? Rn[k] : (k % 4 == 0 ? 1.0 : 0.0);
    f.trim2 = trim_dist * trim_dist;
    const dim3 grid((unsigned)rows), block(256);
    if (normals_of == 0)
      hipLaunchKernelGGL(pair_equations_kernel<0>, grid, block, 0, st, queries, m, points, n, idx, d2, normals, f,
                         partials, (u64*)counters);
    else if (normals_of == 1)
      hipLaunchKernelGGL(pair_equations_kernel<1>, grid, block, 0, st, queries, m, points, n, idx, d2, normals, f,
                         partials, (u64*)counters);
    else
      hipLaunchKernelGGL(pair_equations_kernel<2>, grid, block, 0, st, queries, m, points, n, idx, d2, normals, f,
                         partials, (u64*)counters);
    hipLaunchKernelGGL(pair_equations_sum_kernel, dim3(1), block, 0, st, (const double*)partials, rows, out);
  }
  return pi3_check_launch("cloud_pair_equations");
}
