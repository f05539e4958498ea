// Views of the occupancy grid (occupancy.hip's layout: state u8 [nz][ny][nx], x fastest, cell (ix, iy, iz) at the linear
// index (iz ny + iy) nx + ix; 0 unknown, 1 free, 2 occupied): how much unknown space does a pose see, and in which
// direction?  Integers only; tests/grid_view_ref.py reproduces every output byte for byte.
//
//   between   cell m lies between v and u when the open segment between their centres meets m's open interior; v and u
//             never count, and a cell the segment only touches at a face, edge or corner does not either.  That is the
//             integer DDA from v along o = u - v: axis a has its k-th crossing at t = (2k - 1) / (2 |o_a|); always the
//             smallest t, all axes tied at that t step at once, stop at u.  Over the common denominator 2 |o_x o_y o_z|
//             (a zero length counts as 1) the crossing is the integer key_a = (2k - 1) P_a, P_a = the product of the
//             other two lengths: at most 63 * 32 * 32, compared exactly.
//   visible   u is visible from v when no cell between them is occupied.  Unknown and free cells are transparent.
//   target    of candidate v at range R: u != v inside the grid with |u - v|^2 <= R^2 and state[u] == 0.
//   cone      offset o lies in heading a's cone when o.a > 0 and (o.a)^2 den >= num |o|^2 |a|^2, in 64 bits (|o_i| <= 32,
//             |a_i| <= 1024, den < 2^31: the left side stays below 2^10 * 3 * 2^20 * 2^31 < 2^63).
//
//   pi3_grid_view_candidates  a thread per cell of a settled route field: the reachable cells within max_cost on the
//                             lattice of the absolute index, compacted in any order like pi3_grid_frontier_roots.
//   pi3_grid_view_gain        a workgroup of 256 threads per candidate.  (1) The occupied bits of the (2R + 1)^3 box around
//                             the candidate go to LDS, one bit per cell in box order (z, y, x): thread t of pass i owns
//                             box cell 256 i + t, reads its state byte (rows along x: coalesced; outside the grid: not
//                             occupied) and the wave's ballot is stored as two words, so no LDS atomic is needed and the
//                             bit of box cell j is bit j & 31 of word j >> 5.  (2) The same walk over the box again
//                             finds the targets: a cell of the ball that is unknown.  Few lanes of a wave hold one
//                             (3.4 of 64 per pass on tools/view_timing.py's flat at R = 32), so a wave does not walk
//                             them where they are found: it appends them to its own queue in LDS (ballot ranks, no
//                             atomic; the wave alone touches its queue, so a wave-level fence orders it) and walks 64
//                             at a time: the DDA above on the LDS bits (a step is one ds_read_b32 and a handful of
//                             integer operations, the box index moves by +-1, +-W, +-W^2).  (3) After the wave's rays
//                             have ended, every heading is a ballot over the lanes whose ray arrived, and one lane
//                             adds the count to the heading's LDS word.  Integer sums only: the bytes do not depend on
//                             the order.
//
// Views that cover (tests/grid_cover_ref.py): seen is a bit per cell, cell c at bit c & 31 of word c >> 5, for "a kept
// view sees it".
//   pi3_grid_view_gain_unseen the same kernel, instantiated with one more condition in (2): the cell's bit of seen is
//                             clear.  Lanes along x read the same word: one broadcast load next to the state byte.
//   pi3_grid_view_mark        a workgroup per row (cell, heading): (1) and (2) with every unknown cell of the ball a
//                             target, then a lane whose ray arrived inside the heading's cone (-1: any heading's) ORs
//                             its cell's bit into seen.  The pieces the two kernels share are in grid_view_ray.h.
#include "common.h"
#include "grid_tile.h"
#include "grid_view_ray.h"
#include "voxel_table.h"
#include "wave_block.h"

#include <stdint.h>

namespace {

using grid_tile::grid_ok;
using grid_view_ray::Box;
using grid_view_ray::Headings;
using grid_view_ray::kMarkRows;
using grid_view_ray::kMarkTally;
using grid_view_ray::kMaxAxis;
using grid_view_ray::kMaxHeadings;
using grid_view_ray::kMaxRange;
using grid_view_ray::kQueue;
using grid_view_ray::kTally;
using grid_view_ray::MarkRows;
using grid_view_ray::view_rays_ok;
using voxel_table::u64;
using wave_block::block_exclusive_scan;

constexpr unsigned kFar = 0xFFFFFFFFu;

__device__ __forceinline__ int floor_mod(long v, int m) {
  const int r = (int)(v % m);
  return r < 0 ? r + m : r;
}

__global__ __launch_bounds__(256) void view_candidates_kernel(const unsigned* __restrict__ dist, int nx, int ny, int cells,
                                                              int ox, int oy, int oz, int stride, unsigned max_cost,
                                                              long* __restrict__ out, long cap, u64* __restrict__ count) {
  __shared__ u64 base;
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;      // cells <= 2^27
  bool on = false;
  if (i < cells) {
    const unsigned d = dist[i];
    if (d != kFar && d <= max_cost) {
      const int line = i / nx;
      const int x = i - line * nx, y = line % ny, z = line / ny;
      on = floor_mod((long)ox + x, stride) == 0 && floor_mod((long)oy + y, stride) == 0 &&
           floor_mod((long)oz + z, stride) == 0;
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

// kUnseen: a cell is a target only when its bit of `seen` is clear (pi3_grid_view_gain_unseen); `seen` is not read otherwise
template <bool kUnseen>
__global__ __launch_bounds__(256) void view_gain_kernel(const unsigned char* __restrict__ state, int nx, int ny, int nz,
                                                        const unsigned* __restrict__ seen,
                                                        const long* __restrict__ candidates, int R, int H,
                                                        const Headings hd, long long den, unsigned* __restrict__ gain,
                                                        unsigned* __restrict__ visible, int* __restrict__ best,
                                                        u64* __restrict__ counters) {
  extern __shared__ unsigned lds[];                           // kTally words, a queue per wave, the box's occupied bits
  unsigned* tally = lds;
  unsigned* queue = lds + kTally;
  unsigned* bits = queue + 4 * kQueue;
  const int t = (int)threadIdx.x, lane = t & 63;
  const long v = candidates[blockIdx.x];
  const long cells = (long)nx * ny * nz;
  if (v < 0 || v >= cells) {                                  // the same in every thread
    if (t < H) gain[(long)blockIdx.x * H + t] = 0u;
    if (t == 0) visible[blockIdx.x] = 0u, best[blockIdx.x] = -1;
    return;
  }
  const int line = (int)v / nx;
  const int vx = (int)v - line * nx, vy = line % ny, vz = line / ny;
  const Box box(R);
  if (t < kTally) tally[t] = 0u;

  // (1) the occupied bits
  grid_view_ray::stage_occupied(box, state, nx, ny, nz, vx, vy, vz, t, bits);
  __syncthreads();

  // (2) the same walk finds the targets; a wave queues them (box offsets + R, 7 bits each) and walks 64 at a time,
  // (3) then the cones of those that arrive.  Pass `passes` only empties the queue.
  const int R2 = R * R;
  unsigned* mine = queue + (t >> 6) * kQueue;                 // this wave's queue; the wave alone reads and writes it
  int queued = 0;                                             // the same in every lane of the wave; < 64 between passes
  int bx, by, bz;
  box.first(t, bx, by, bz);
  for (int p = 0; p <= box.passes; ++p) {
    if (p < box.passes) {
      const int ox = bx - R, oy = by - R, oz = bz - R;
      const int gx = vx + ox, gy = vy + oy, gz = vz + oz;
      const int o2 = ox * ox + oy * oy + oz * oz;
      bool cast = false;
      if (bz < box.W && o2 != 0 && o2 <= R2 && gx >= 0 && gx < nx && gy >= 0 && gy < ny && gz >= 0 && gz < nz) {
        const long u = ((long)gz * ny + gy) * nx + gx;
        cast = state[u] == 0;
        if (kUnseen) cast = cast && !((seen[u >> 5] >> (u & 31)) & 1u);     // lanes along x read the same word
      }
      grid_view_ray::queue_push(mine, queued, cast, lane, bx, by, bz);
      box.next(bx, by, bz);
    }
    if (queued < 64 && !(p == box.passes && queued > 0)) continue;
    int ox, oy, oz;
    bool holds;
    const int take = grid_view_ray::queue_take(mine, queued, lane, R, holds, ox, oy, oz);
    bool arrived = false;
    if (holds) arrived = grid_view_ray::ray_arrives(bits, R, box.W, box.W2, ox, oy, oz);
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
  if (t < H) gain[(long)blockIdx.x * H + t] = tally[t];
  if (t == 0) {
    int first = 0;
    for (int h = 1; h < H; ++h)
      if (tally[h] > tally[first]) first = h;                 // the smallest heading of the largest gain
    best[blockIdx.x] = first;
    visible[blockIdx.x] = tally[kMaxHeadings];
    atomicAdd(counters + 0, 1ull);
    if (tally[kMaxHeadings + 1]) atomicAdd(counters + 1, (u64)tally[kMaxHeadings + 1]);
    if (tally[kMaxHeadings + 2]) atomicAdd(counters + 2, (u64)tally[kMaxHeadings + 2]);
    if (tally[kMaxHeadings]) atomicAdd(counters + 3, (u64)tally[kMaxHeadings]);
  }
}

// A workgroup per row (cells[i], rows.heading[same ? 0 : i]): the gain kernel's box, queue and DDA with every unknown cell of the
// ball a target (the mask does not thin the rays).  A lane whose ray arrived inside the row's cone reads the cell's
// word of `seen` and, only when the bit is clear, ORs it in; the bit is new when the returned word had it clear, so of
// several rows that race for one cell exactly one counts it.  owner is written by that lane alone.
__global__ __launch_bounds__(256) void view_mark_kernel(const unsigned char* __restrict__ state, int nx, int ny, int nz,
                                                        unsigned* seen, const long* __restrict__ cells_in,
                                                        const MarkRows rows, int same, int R, int H, const Headings hd,
                                                        long long den, short* owner, int tag,
                                                        u64* __restrict__ counters) {
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
  const Box box(R);
  if (t < kMarkTally) tally[t] = 0u;
  grid_view_ray::stage_occupied(box, state, nx, ny, nz, vx, vy, vz, t, bits);
  __syncthreads();

  const int R2 = R * R;
  unsigned* mine = queue + (t >> 6) * kQueue;
  int queued = 0;
  int bx, by, bz;
  box.first(t, bx, by, bz);
  for (int p = 0; p <= box.passes; ++p) {
    if (p < box.passes) {
      const int ox = bx - R, oy = by - R, oz = bz - R;
      const int gx = vx + ox, gy = vy + oy, gz = vz + oz;
      const int o2 = ox * ox + oy * oy + oz * oz;
      bool cast = false;
      if (bz < box.W && o2 != 0 && o2 <= R2 && gx >= 0 && gx < nx && gy >= 0 && gy < ny && gz >= 0 && gz < nz)
        cast = state[((long)gz * ny + gy) * nx + gx] == 0;
      grid_view_ray::queue_push(mine, queued, cast, lane, bx, by, bz);
      box.next(bx, by, bz);
    }
    if (queued < 64 && !(p == box.passes && queued > 0)) continue;
    int ox, oy, oz;
    bool holds;
    const int take = grid_view_ray::queue_take(mine, queued, lane, R, holds, ox, oy, oz);
    bool arrived = false;
    if (holds) arrived = grid_view_ray::ray_arrives(bits, R, box.W, box.W2, ox, oy, oz);
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
  if (t == 0) {
    atomicAdd(counters + 0, 1ull);
    for (int i = 0; i < kMarkTally; ++i)
      if (tally[i]) atomicAdd(counters + 1 + i, (u64)tally[i]);
  }
}

// pi3_grid_view_gain (seen == nullptr, unseen false) and pi3_grid_view_gain_unseen
int view_gain(const char* who, bool unseen, const unsigned char* state, int nx, int ny, int nz, const unsigned* seen,
              const long* candidates, long V, int range, const int* headings, int H, long cos2_num, long cos2_den,
              unsigned* gain, unsigned* visible, int* best, unsigned long long* counters, void* stream) {
  long cells = 0;
  Headings hd = {};
  const bool ok = view_rays_ok(state, nx, ny, nz, cells, V, range, kMaxRange, headings, H, cos2_num, cos2_den, counters,
                               hd) &&
                  (V == 0 || (candidates && gain && visible && best)) && (!unseen || seen);
  if (!ok) {
    pi3_set_error("%s: bad arguments dims=(%d, %d, %d) (1 .. 2^21 - 1 each, at most 2^27 cells) V=%ld "
                  "(0 .. 2^31 - 1) range=%d (1 .. %d) H=%d (1 .. %d; every axis non-zero, components within +-%d) "
                  "cos2=%ld/%ld (0 <= num <= den, 0 < den < 2^31), or a null pointer", who, nx, ny, nz, V, range,
                  kMaxRange, H, kMaxHeadings, kMaxAxis, cos2_num, cos2_den);
    return PI3_ERR_ARG;
  }
  if (pi3_zero_words(who, counters, 4, stream) != PI3_OK) return PI3_ERR_LAUNCH;
  if (V == 0) return PI3_OK;                  // no candidate: no kernel
  const size_t bytes = (size_t)(kTally + 4 * kQueue + grid_view_ray::box_words(range)) * sizeof(unsigned);
  if (unseen)
    hipLaunchKernelGGL(view_gain_kernel<true>, dim3((unsigned)V), dim3(256), bytes, (hipStream_t)stream, state, nx, ny,
                       nz, seen, candidates, range, H, hd, (long long)cos2_den, gain, visible, best, (u64*)counters);
  else
    hipLaunchKernelGGL(view_gain_kernel<false>, dim3((unsigned)V), dim3(256), bytes, (hipStream_t)stream, state, nx, ny,
                       nz, (const unsigned*)nullptr, candidates, range, H, hd, (long long)cos2_den, gain, visible, best,
                       (u64*)counters);
  return pi3_check_launch(who + 4);           // without "pi3_"
}

}  // namespace

extern "C" int pi3_grid_view_candidates(const unsigned* dist, int nx, int ny, int nz, int ox, int oy, int oz, int stride,
                                        long max_cost, long* cells_out, long cap, long* count, void* stream) {
  long cells = 0;
  if (!dist || !count || !grid_ok(nx, ny, nz, cells) || stride < 1 || max_cost < 0 || cap < 0 || (cap > 0 && !cells_out)) {
    pi3_set_error("pi3_grid_view_candidates: bad arguments dims=(%d, %d, %d) (1 .. 2^21 - 1 each, at most 2^27 cells) "
                  "stride=%d (>= 1) max_cost=%ld (>= 0) cap=%ld (>= 0; cells may be NULL at 0), or a null pointer", nx,
                  ny, nz, stride, max_cost, cap);
    return PI3_ERR_ARG;
  }
  if (pi3_zero_words("pi3_grid_view_candidates", count, 1, stream) != PI3_OK) return PI3_ERR_LAUNCH;
  const unsigned limit = max_cost >= (long)kFar ? kFar - 1u : (unsigned)max_cost;       // the far mark never passes
  hipLaunchKernelGGL(view_candidates_kernel, dim3(voxel_table::blocks_for(cells)), dim3(256), 0, (hipStream_t)stream,
                     dist, nx, ny, (int)cells, ox, oy, oz, stride, limit, cells_out, cap, (u64*)count);
  return pi3_check_launch("grid_view_candidates");
}

extern "C" int pi3_grid_view_gain(const unsigned char* state, int nx, int ny, int nz, const long* candidates, long V,
                                  int range, const int* headings, int H, long cos2_num, long cos2_den, unsigned* gain,
                                  unsigned* visible, int* best, unsigned long long* counters, void* stream) {
  return view_gain("pi3_grid_view_gain", false, state, nx, ny, nz, nullptr, candidates, V, range, headings, H, cos2_num,
                   cos2_den, gain, visible, best, counters, stream);
}

extern "C" int pi3_grid_view_gain_unseen(const unsigned char* state, int nx, int ny, int nz, const unsigned* seen,
                                         const long* candidates, long V, int range, const int* headings, int H,
                                         long cos2_num, long cos2_den, unsigned* gain, unsigned* visible, int* best,
                                         unsigned long long* counters, void* stream) {
  return view_gain("pi3_grid_view_gain_unseen", true, state, nx, ny, nz, seen, candidates, V, range, headings, H,
                   cos2_num, cos2_den, gain, visible, best, counters, stream);
}

extern "C" int pi3_grid_view_mark(const unsigned char* state, int nx, int ny, int nz, unsigned* seen, const long* cells_in,
                                  const int* heading_of, long V, int range, const int* headings, int H, long cos2_num,
                                  long cos2_den, short* owner, int tag, unsigned long long* counters, void* stream) {
  long cells = 0;
  Headings hd = {};
  bool ok = view_rays_ok(state, nx, ny, nz, cells, V, range, kMaxRange, headings, H, cos2_num, cos2_den, counters, hd) && seen &&
            (V == 0 || (cells_in && heading_of)) && tag >= 0 && tag < 32768 && (!owner || V == 1);
  for (long i = 0; ok && i < V; ++i) ok = heading_of[i] >= -1 && heading_of[i] < H;
  if (!ok) {
    pi3_set_error("pi3_grid_view_mark: bad arguments dims=(%d, %d, %d) (1 .. 2^21 - 1 each, at most 2^27 cells) V=%ld "
                  "(0 .. 2^31 - 1; 1 with an owner) range=%d (1 .. %d) H=%d (1 .. %d; every axis non-zero, components "
                  "within +-%d; every row's heading in -1 .. H - 1) cos2=%ld/%ld (0 <= num <= den, 0 < den < 2^31) "
                  "tag=%d (0 .. 32767), or a null pointer", nx, ny, nz, V, range, kMaxRange, H, kMaxHeadings, kMaxAxis,
                  cos2_num, cos2_den, tag);
    return PI3_ERR_ARG;
  }
  if (pi3_zero_words("pi3_grid_view_mark", counters, 1 + kMarkTally, stream) != PI3_OK) return PI3_ERR_LAUNCH;
  const size_t bytes = (size_t)(kMarkTally + 4 * kQueue + grid_view_ray::box_words(range)) * sizeof(unsigned);
  // The rows' headings travel by value.  One heading for all rows (a single view, the seeable pass) is one launch;
  // else kMarkRows rows per launch, which costs a large batch the balance of one grid over all its rows.
  bool same = true;
  for (long i = 1; same && i < V; ++i) same = heading_of[i] == heading_of[0];
  const long step = same ? V : kMarkRows;
  MarkRows rows;
  for (long base = 0; base < V; base += step) {
    const long n = V - base < step ? V - base : step;
    for (int i = 0; i < kMarkRows; ++i) rows.heading[i] = (signed char)(i < n ? heading_of[base + i] : -1);
    hipLaunchKernelGGL(view_mark_kernel, dim3((unsigned)n), dim3(256), bytes, (hipStream_t)stream, state, nx, ny, nz,
                       seen, cells_in + base, rows, same ? 1 : 0, range, H, hd, (long long)cos2_den, owner, tag,
                       (u64*)counters);
    const int rc = pi3_check_launch("grid_view_mark");
    if (rc != PI3_OK) return rc;
  }
  return PI3_OK;
}
