// Views that see farther: the three ray kernels of grid_view.hip at a range of up to 64 cells.  The rules
// (between, visible, target, cone, per candidate; mark's "only when the bit reads clear", owner and counters) are
// grid_view.hip's, unchanged; tests/grid_view_ref.py and tests/grid_cover_ref.py reproduce every output byte for byte.
//
//   octant    a ray from v to u = v + o only touches cells whose offset from v lies, on every axis a, between 0 and o_a:
//             it never leaves the closed octant of its target.  So a workgroup does not stage the (2R + 1)^3 box but one
//             of its eight octant boxes of W = R + 1 cells per axis: octant q (bit a of q set: axis a negative) covers
//             the offsets 0 .. R on a positive axis and -R .. 0 on a negative one, and the pose sits at box coordinate 0
//             or R.  At R = 64 that is 65^3 bits, the 34.3 KB the near form stages at R = 32.
//   ownership a target o belongs to exactly one octant: axis a is positive when o_a >= 0.  A negative octant stages its
//             o_a = 0 plane, because its rays pass through it, and never casts at a cell of that plane (Octant::owns).
//   grid      (poses, 8): a workgroup of 256 threads per pose and octant, so that a single pose (cover marks one view
//             per round) still fills eight workgroups.  The looping form (one workgroup, eight octants in turn) was not
//             measured; this is the only form.
//   sums      every workgroup adds its LDS tally to gain[v][h], visible[v] and the counters with integer atomics: order
//             free, so the bytes are fixed.  The entry point zeroes them first, on the stream; octant 0 alone counts the
//             pose; view_best_kernel, a thread per pose, writes best afterwards.  mark needs no finishing.
//
// Arithmetic at R = 64: a DDA key grows by 2 P <= 2 * 64 * 64 = 8192 per crossing and an axis is crossed at most 64
// times, so a key stays below 2 * 64 * 8192 = 2^20 < kNever = 2^30; the bit index stays below 65^3 = 274 625; box
// coordinates 0 .. 64 fit the queue's 7-bit fields.  The cone test forms (o.a)^2 den <= R^2 |a|^2 den in 64 bits: the
// entry points refuse a call whose range^2 max|a|^2 den reaches 2^63 (the planner's |a|^2 <= 3 and den = 2^20 are far
// inside).  No float, no scratch, no inline assembly.
#include "common.h"
#include "grid_view_ray.h"
#include "voxel_table.h"

#include <stdint.h>

namespace {

using grid_view_ray::Headings;
using grid_view_ray::kFarMaxRange;
using grid_view_ray::kMarkRows;
using grid_view_ray::kMarkTally;
using grid_view_ray::kMaxAxis;
using grid_view_ray::kMaxHeadings;
using grid_view_ray::kQueue;
using grid_view_ray::kTally;
using grid_view_ray::MarkRows;
using voxel_table::u64;

// One octant box of the pose as 256 threads walk it, 256 cells per pass in box order (z, y, x): grid_view_ray::Box with
// W = R + 1 and the pose in a corner.
struct Octant {
  int R, W, W2, passes, dx, dy, dz;
  int px, py, pz;                                             // the pose's box coordinate: 0 on a positive axis, R on a negative
  __device__ __forceinline__ Octant(int R_, int q) : R(R_), W(R_ + 1) {
    W2 = W * W;
    passes = (W2 * W + 255) >> 8;                              // the box has at most 65^3 cells
    dx = 256 % W, dy = (256 / W) % W, dz = 256 / W2;
    px = (q & 1) ? R : 0, py = (q & 2) ? R : 0, pz = (q & 4) ? R : 0;
  }
  __device__ __forceinline__ void first(int t, int& bx, int& by, int& bz) const { bx = t % W, by = (t / W) % W, bz = t / W2; }
  __device__ __forceinline__ void next(int& bx, int& by, int& bz) const {
    grid_view_ray::box_advance(bx, by, bz, dx, dy, dz, W);
  }
  __device__ __forceinline__ int pose_cell() const { return (pz * W + py) * W + px; }
  // THE ownership rule: offset o_a = b_a - p_a belongs to the positive side of axis a when o_a >= 0, so a negative
  // octant (p_a = R) owns b_a < R only.  Its plane b_a = R (o_a = 0) is staged, rays pass through it, but a cell of
  // it is never a target here: the octant that is positive on that axis casts at it.  Every offset of the ball, the
  // axes and planes included, is therefore cast at once.
  __device__ __forceinline__ bool owns(int bx, int by, int bz) const {
    return (px == 0 || bx < R) && (py == 0 || by < R) && (pz == 0 || bz < R);
  }
  // no cell this octant owns lies inside the grid: the pose stands on the border its negative axis points across
  __device__ __forceinline__ bool empty(int vx, int vy, int vz) const {
    return (px && vx == 0) || (py && vy == 0) || (pz && vz == 0);
  }
};

// stage_occupied for an octant box: thread t of pass i owns box cell 256 i + t, the wave's ballot is two whole words
// (no LDS atomic), a cell outside the grid is not occupied.  The caller's __syncthreads() follows.
__device__ __forceinline__ void stage_octant(const Octant& b, const unsigned char* __restrict__ state, int nx, int ny,
                                             int nz, int vx, int vy, int vz, int t, unsigned* bits) {
  const int lane = t & 63;
  int bx, by, bz;
  b.first(t, bx, by, bz);
  for (int p = 0; p < b.passes; ++p) {
    const int gx = vx - b.px + bx, gy = vy - b.py + by, gz = vz - b.pz + bz;
    bool occ = false;
    if (bz < b.W && gx >= 0 && gx < nx && gy >= 0 && gy < ny && gz >= 0 && gz < nz)
      occ = state[((long)gz * ny + gy) * nx + gx] == 2;
    const unsigned long long m = __ballot(occ);
    if (lane == 0) {
      const int w = ((p << 8) + t) >> 5;                      // the wave's 64 cells are two whole words
      bits[w] = (unsigned)m;
      bits[w + 1] = (unsigned)(m >> 32);
    }
    b.next(bx, by, bz);
  }
}

// is box cell (bx, by, bz) of the octant a target of the pose?  Inside the box, owned, in the ball, inside the grid and
// unknown; u is its linear index then.
__device__ __forceinline__ bool octant_target(const Octant& b, const unsigned char* __restrict__ state, int nx, int ny,
                                              int nz, int vx, int vy, int vz, int bx, int by, int bz, long& u) {
  const int ox = bx - b.px, oy = by - b.py, oz = bz - b.pz;
  const int gx = vx + ox, gy = vy + oy, gz = vz + oz;
  const int o2 = ox * ox + oy * oy + oz * oz;
  if (!(bz < b.W && b.owns(bx, by, bz) && o2 != 0 && o2 <= b.R * b.R && gx >= 0 && gx < nx && gy >= 0 && gy < ny &&
        gz >= 0 && gz < nz))
    return false;
  u = ((long)gz * ny + gy) * nx + gx;
  return state[u] == 0;
}

// view_gain_kernel per (pose, octant): blockIdx.x is the pose, blockIdx.y the octant.  gain, visible and the counters
// were zeroed by the entry point and take atomic sums; best is view_best_kernel's.
template <bool kUnseen>
__global__ __launch_bounds__(256) void view_gain_far_kernel(const unsigned char* __restrict__ state, int nx, int ny, int nz,
                                                            const unsigned* __restrict__ seen,
                                                            const long* __restrict__ candidates, int R, int H,
                                                            const Headings hd, long long den, unsigned* gain,
                                                            unsigned* visible, u64* counters) {
  extern __shared__ unsigned lds[];                           // kTally words, a queue per wave, the octant's occupied bits
  unsigned* tally = lds;
  unsigned* queue = lds + kTally;
  unsigned* bits = queue + 4 * kQueue;
  const int t = (int)threadIdx.x, lane = t & 63;
  const long v = candidates[blockIdx.x];
  const long cells = (long)nx * ny * nz;
  if (v < 0 || v >= cells) return;                            // the same in every thread: zeros, and best = -1
  const int line = (int)v / nx;
  const int vx = (int)v - line * nx, vy = line % ny, vz = line / ny;
  const Octant box(R, (int)blockIdx.y);
  if (blockIdx.y == 0 && t == 0) atomicAdd(counters + 0, 1ull);        // the pose is counted once, not per octant
  if (box.empty(vx, vy, vz)) return;                          // the same in every thread
  if (t < kTally) tally[t] = 0u;

  // (1) the occupied bits
  stage_octant(box, state, nx, ny, nz, vx, vy, vz, t, bits);
  __syncthreads();

  // (2) the same walk finds the targets; a wave queues them (box coordinates, 7 bits each) and walks 64 at a time,
  // (3) then the cones of those that arrive.  Pass `passes` only empties the queue.
  const int home = box.pose_cell();
  unsigned* mine = queue + (t >> 6) * kQueue;                 // this wave's queue; the wave alone reads and writes it
  int queued = 0;                                             // the same in every lane of the wave; < 64 between passes
  int bx, by, bz;
  box.first(t, bx, by, bz);
  for (int p = 0; p <= box.passes; ++p) {
    if (p < box.passes) {
      long u = 0;
      bool cast = octant_target(box, state, nx, ny, nz, vx, vy, vz, bx, by, bz, u);
      if (kUnseen) cast = cast && !((seen[u >> 5] >> (u & 31)) & 1u);      // lanes along x read the same word
      grid_view_ray::queue_push(mine, queued, cast, lane, bx, by, bz);
      box.next(bx, by, bz);
    }
    if (queued < 64 && !(p == box.passes && queued > 0)) continue;
    int ox, oy, oz;
    bool holds;
    const int take = grid_view_ray::queue_take(mine, queued, lane, 0, holds, ox, oy, oz);      // box coordinates
    ox -= box.px, oy -= box.py, oz -= box.pz;
    bool arrived = false;
    if (holds) arrived = grid_view_ray::ray_arrives_from(bits, home, box.W, box.W2, ox, oy, oz);
    const u64 arrived_b = __ballot(arrived);
    if (arrived_b) {                                          // the same in every lane of the wave
      const long long o2l = ox * ox + oy * oy + oz * oz;
      for (int h = 0; h < H; ++h) {
        const u64 b = __ballot(grid_view_ray::in_cone(hd, h, den, ox, oy, oz, o2l) && arrived);
        if (lane == 0 && b) atomicAdd(&tally[h], (unsigned)__popcll(b));
      }
    }
    if (lane == 0) {
      const unsigned n = (unsigned)__popcll(arrived_b);
      atomicAdd(&tally[kMaxHeadings], n);
      atomicAdd(&tally[kMaxHeadings + 1], (unsigned)take);
      atomicAdd(&tally[kMaxHeadings + 2], (unsigned)take - n);
    }
  }
  __syncthreads();
  if (t < H && tally[t]) atomicAdd(&gain[(long)blockIdx.x * H + t], tally[t]);
  if (t == 0) {
    if (tally[kMaxHeadings]) atomicAdd(&visible[blockIdx.x], tally[kMaxHeadings]);
    if (tally[kMaxHeadings + 1]) atomicAdd(counters + 1, (u64)tally[kMaxHeadings + 1]);
    if (tally[kMaxHeadings + 2]) atomicAdd(counters + 2, (u64)tally[kMaxHeadings + 2]);
    if (tally[kMaxHeadings]) atomicAdd(counters + 3, (u64)tally[kMaxHeadings]);
  }
}

// a thread per pose, after the octants' sums: the smallest heading of the largest gain, -1 for a pose outside the grid
__global__ __launch_bounds__(256) void view_best_kernel(const long* __restrict__ candidates, long V, long cells, int H,
                                                        const unsigned* __restrict__ gain, int* __restrict__ best) {
  const long i = (long)blockIdx.x * 256 + (long)threadIdx.x;
  if (i >= V) return;
  const long v = candidates[i];
  int first = -1;
  if (v >= 0 && v < cells) {
    first = 0;
    for (int h = 1; h < H; ++h)
      if (gain[i * H + h] > gain[i * H + first]) first = h;
  }
  best[i] = first;
}

// view_mark_kernel per (row, octant)
__global__ __launch_bounds__(256) void view_mark_far_kernel(const unsigned char* __restrict__ state, int nx, int ny, int nz,
                                                            unsigned* seen, const long* __restrict__ cells_in,
                                                            const MarkRows rows, int same, int R, int H,
                                                            const Headings hd, long long den, short* owner, int tag,
                                                            u64* counters) {
  extern __shared__ unsigned lds[];                           // kMarkTally words, a queue per wave, the occupied bits
  unsigned* tally = lds;
  unsigned* queue = lds + kMarkTally;
  unsigned* bits = queue + 4 * kQueue;
  const int t = (int)threadIdx.x, lane = t & 63;
  const long v = cells_in[blockIdx.x];
  const long cells = (long)nx * ny * nz;
  if (v < 0 || v >= cells) return;                            // the same in every thread: no view
  const int heading = rows.heading[same ? 0 : blockIdx.x];
  const int line = (int)v / nx;
  const int vx = (int)v - line * nx, vy = line % ny, vz = line / ny;
  const Octant box(R, (int)blockIdx.y);
  if (blockIdx.y == 0 && t == 0) atomicAdd(counters + 0, 1ull);        // the view is counted once, not per octant
  if (box.empty(vx, vy, vz)) return;                          // the same in every thread
  if (t < kMarkTally) tally[t] = 0u;
  stage_octant(box, state, nx, ny, nz, vx, vy, vz, t, bits);
  __syncthreads();

  const int home = box.pose_cell();
  unsigned* mine = queue + (t >> 6) * kQueue;
  int queued = 0;
  int bx, by, bz;
  box.first(t, bx, by, bz);
  for (int p = 0; p <= box.passes; ++p) {
    if (p < box.passes) {
      long u = 0;
      const bool cast = octant_target(box, state, nx, ny, nz, vx, vy, vz, bx, by, bz, u);
      grid_view_ray::queue_push(mine, queued, cast, lane, bx, by, bz);
      box.next(bx, by, bz);
    }
    if (queued < 64 && !(p == box.passes && queued > 0)) continue;
    int ox, oy, oz;
    bool holds;
    const int take = grid_view_ray::queue_take(mine, queued, lane, 0, holds, ox, oy, oz);      // box coordinates
    ox -= box.px, oy -= box.py, oz -= box.pz;
    bool arrived = false;
    if (holds) arrived = grid_view_ray::ray_arrives_from(bits, home, box.W, box.W2, ox, oy, oz);
    const u64 arrived_b = __ballot(arrived);
    bool in = false, fresh = false;
    if (arrived_b) {                                          // the same in every lane of the wave
      const long long o2l = ox * ox + oy * oy + oz * oz;
      if (heading >= 0) {
        in = grid_view_ray::in_cone(hd, heading, den, ox, oy, oz, o2l) && arrived;
      } else {
        for (int h = 0; h < H; ++h) in = in || (grid_view_ray::in_cone(hd, h, den, ox, oy, oz, o2l) && arrived);
      }
      if (in) {                                               // a target: inside the grid, so u < cells
        const long u = ((long)(vz + oz) * ny + (vy + oy)) * nx + (vx + ox);
        const unsigned bit = 1u << (u & 31);
        unsigned* word = seen + (u >> 5);
        if (!(__atomic_load_n(word, __ATOMIC_RELAXED) & bit)) {
          fresh = !(atomicOr(word, bit) & bit);
          if (fresh && owner) owner[u] = (short)tag;
        }
      }
    }
    const u64 in_b = __ballot(in), fresh_b = __ballot(fresh);
    if (lane == 0) {
      atomicAdd(&tally[0], (unsigned)take);
      if (arrived_b) atomicAdd(&tally[1], (unsigned)__popcll(arrived_b));
      if (in_b) atomicAdd(&tally[2], (unsigned)__popcll(in_b));
      if (fresh_b) atomicAdd(&tally[3], (unsigned)__popcll(fresh_b));
    }
  }
  __syncthreads();
  if (t == 0)
    for (int i = 0; i < kMarkTally; ++i)
      if (tally[i]) atomicAdd(counters + 1 + i, (u64)tally[i]);
}

// the words of an octant's occupied bits: grid_view_ray::box_words for W = R + 1 (35.7 KB with the queues at R = 64)
int octant_words(int R) {
  const int W = R + 1;
  return 8 * ((W * W * W + 255) / 256);
}

// The far form's own rule: (o.a)^2 den <= range^2 |a|^2 den must stay below 2^63.  range^2 |a|^2 <= 2^12 * 3 * 2^20
// fits easily; the last product is compared by division instead of being formed.
bool cone_fits(int range, const Headings& hd, int H, long cos2_den) {
  long long most = 0;
  for (int h = 0; h < H; ++h) {
    long long n2 = 0;
    for (int a = 0; a < 3; ++a) n2 += (long long)hd.axis[h][a] * hd.axis[h][a];
    most = n2 > most ? n2 : most;
  }
  return (long long)range * range * most <= 0x7FFFFFFFFFFFFFFFll / (long long)cos2_den;
}

const char* const kConeRule = "the cone test's 64 bits: range^2 * max |axis|^2 * den < 2^63";

// pi3_grid_view_gain_far (seen == nullptr, unseen false) and pi3_grid_view_gain_unseen_far
int view_gain_far(const char* who, bool unseen, const unsigned char* state, int nx, int ny, int nz, const unsigned* seen,
                  const long* candidates, long V, int range, const int* headings, int H, long cos2_num, long cos2_den,
                  unsigned* gain, unsigned* visible, int* best, unsigned long long* counters, void* stream) {
  long cells = 0;
  Headings hd = {};
  const bool ok = grid_view_ray::view_rays_ok(state, nx, ny, nz, cells, V, range, kFarMaxRange, headings, H, cos2_num,
                                              cos2_den, counters, hd) &&
                  (V == 0 || (candidates && gain && visible && best)) && (!unseen || seen);
  if (!ok || !cone_fits(range, hd, H, cos2_den)) {
    pi3_set_error("%s: bad arguments dims=(%d, %d, %d) (1 .. 2^21 - 1 each, at most 2^27 cells) V=%ld "
                  "(0 .. 2^31 - 1) range=%d (1 .. %d) H=%d (1 .. %d; every axis non-zero, components within +-%d) "
                  "cos2=%ld/%ld (0 <= num <= den, 0 < den < 2^31; %s), or a null pointer", who, nx, ny, nz, V, range,
                  kFarMaxRange, H, kMaxHeadings, kMaxAxis, cos2_num, cos2_den, kConeRule);
    return PI3_ERR_ARG;
  }
  const hipStream_t s = (hipStream_t)stream;
  if (pi3_zero_words(who, counters, 4, stream) != PI3_OK) return PI3_ERR_LAUNCH;
  if (V == 0) return PI3_OK;                  // no candidate: no kernel
  if (hipMemsetAsync(gain, 0, (size_t)V * H * sizeof(unsigned), s) != hipSuccess ||
      hipMemsetAsync(visible, 0, (size_t)V * sizeof(unsigned), s) != hipSuccess) {
    pi3_set_error("%s: hipMemsetAsync failed", who);
    return PI3_ERR_LAUNCH;
  }
  const size_t bytes = (size_t)(kTally + 4 * kQueue + octant_words(range)) * sizeof(unsigned);
  const dim3 grid((unsigned)V, 8);
  if (unseen)
    hipLaunchKernelGGL(view_gain_far_kernel<true>, grid, dim3(256), bytes, s, state, nx, ny, nz, seen, candidates, range,
                       H, hd, (long long)cos2_den, gain, visible, (u64*)counters);
  else
    hipLaunchKernelGGL(view_gain_far_kernel<false>, grid, dim3(256), bytes, s, state, nx, ny, nz,
                       (const unsigned*)nullptr, candidates, range, H, hd, (long long)cos2_den, gain, visible,
                       (u64*)counters);
  const int rc = pi3_check_launch(who + 4);   // without "pi3_"
  if (rc != PI3_OK) return rc;
  hipLaunchKernelGGL(view_best_kernel, dim3(voxel_table::blocks_for(V)), dim3(256), 0, s, candidates, V, cells, H,
                     (const unsigned*)gain, best);
  return pi3_check_launch(who + 4);
}

}  // namespace

extern "C" int pi3_grid_view_gain_far(const unsigned char* state, int nx, int ny, int nz, const long* candidates, long V,
                                      int range, const int* headings, int H, long cos2_num, long cos2_den,
                                      unsigned* gain, unsigned* visible, int* best, unsigned long long* counters,
                                      void* stream) {
  return view_gain_far("pi3_grid_view_gain_far", false, state, nx, ny, nz, nullptr, candidates, V, range, headings, H,
                       cos2_num, cos2_den, gain, visible, best, counters, stream);
}

extern "C" int pi3_grid_view_gain_unseen_far(const unsigned char* state, int nx, int ny, int nz, const unsigned* seen,
                                             const long* candidates, long V, int range, const int* headings, int H,
                                             long cos2_num, long cos2_den, unsigned* gain, unsigned* visible, int* best,
                                             unsigned long long* counters, void* stream) {
  return view_gain_far("pi3_grid_view_gain_unseen_far", true, state, nx, ny, nz, seen, candidates, V, range, headings, H,
                       cos2_num, cos2_den, gain, visible, best, counters, stream);
}

extern "C" int pi3_grid_view_mark_far(const unsigned char* state, int nx, int ny, int nz, unsigned* seen,
                                      const long* cells_in, const int* heading_of, long V, int range, const int* headings,
                                      int H, long cos2_num, long cos2_den, short* owner, int tag,
                                      unsigned long long* counters, void* stream) {
  long cells = 0;
  Headings hd = {};
  bool ok = grid_view_ray::view_rays_ok(state, nx, ny, nz, cells, V, range, kFarMaxRange, headings, H, cos2_num, cos2_den,
                                        counters, hd) &&
            seen && (V == 0 || (cells_in && heading_of)) && tag >= 0 && tag < 32768 && (!owner || V == 1);
  for (long i = 0; ok && i < V; ++i) ok = heading_of[i] >= -1 && heading_of[i] < H;
  if (!ok || !cone_fits(range, hd, H, cos2_den)) {
    pi3_set_error("pi3_grid_view_mark_far: bad arguments dims=(%d, %d, %d) (1 .. 2^21 - 1 each, at most 2^27 cells) "
                  "V=%ld (0 .. 2^31 - 1; 1 with an owner) range=%d (1 .. %d) H=%d (1 .. %d; every axis non-zero, "
                  "components within +-%d; every row's heading in -1 .. H - 1) cos2=%ld/%ld (0 <= num <= den, 0 < den < "
                  "2^31; %s) tag=%d (0 .. 32767), or a null pointer", nx, ny, nz, V, range, kFarMaxRange, H, kMaxHeadings,
                  kMaxAxis, cos2_num, cos2_den, kConeRule, tag);
    return PI3_ERR_ARG;
  }
  if (pi3_zero_words("pi3_grid_view_mark_far", counters, 1 + kMarkTally, stream) != PI3_OK) return PI3_ERR_LAUNCH;
  const size_t bytes = (size_t)(kMarkTally + 4 * kQueue + octant_words(range)) * sizeof(unsigned);
  // the rows' headings travel by value, as in pi3_grid_view_mark: one launch when all rows share a heading, else
  // kMarkRows rows per launch
  bool same = true;
  for (long i = 1; same && i < V; ++i) same = heading_of[i] == heading_of[0];
  const long step = same ? V : kMarkRows;
  MarkRows rows;
  for (long base = 0; base < V; base += step) {
    const long n = V - base < step ? V - base : step;
    for (int i = 0; i < kMarkRows; ++i) rows.heading[i] = (signed char)(i < n ? heading_of[base + i] : -1);
    hipLaunchKernelGGL(view_mark_far_kernel, dim3((unsigned)n, 8), dim3(256), bytes, (hipStream_t)stream, state, nx, ny,
                       nz, seen, cells_in + base, rows, same ? 1 : 0, range, H, hd, (long long)cos2_den, owner, tag,
                       (u64*)counters);
    const int rc = pi3_check_launch("grid_view_mark_far");
    if (rc != PI3_OK) return rc;
  }
  return PI3_OK;
}
