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
#include "common.h"
#include "grid_tile.h"
#include "voxel_table.h"
#include "wave_block.h"

#include <stdint.h>

namespace {

using grid_tile::grid_ok;
using voxel_table::u64;
using wave_block::block_exclusive_scan;

constexpr unsigned kFar = 0xFFFFFFFFu;
constexpr int kMaxRange = 32;
constexpr int kMaxHeadings = 32;
constexpr int kMaxAxis = 1024;          // per component of a heading
constexpr int kNever = 1 << 30;         // the key of an axis the ray does not move along
constexpr int kTally = kMaxHeadings + 3;                 // LDS words: a gain per heading, visible, targets, blocked
constexpr int kQueue = 128;             // LDS words per wave: fewer than 64 targets waiting + the 64 of one pass

struct Headings {
  int axis[kMaxHeadings][3];
  long long norm[kMaxHeadings];         // num |a|^2
};

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

// this thread's box cell moves on by 256 cells: (bx, by, bz) += (dx, dy, dz) with carries, 256 = (dz W + dy) W + dx
__device__ __forceinline__ void box_advance(int& bx, int& by, int& bz, int dx, int dy, int dz, int W) {
  bx += dx;
  if (bx >= W) bx -= W, ++by;
  by += dy;
  if (by >= W) by -= W, ++bz;
  bz += dz;
}

// orders this wave's LDS stores and loads around a hand-over between its lanes (LDS operations of one wave run in
// order; this keeps the compiler from moving them)
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(256) void view_gain_kernel(const unsigned char* __restrict__ state, int nx, int ny, int nz,
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
  const int W = 2 * R + 1, W2 = W * W, box = W2 * W;          // <= 65^3
  const int dx = 256 % W, dy = (256 / W) % W, dz = 256 / W2;
  const int passes = (box + 255) >> 8;
  if (t < kTally) tally[t] = 0u;

  // (1) the occupied bits
  int bx = t % W, by = (t / W) % W, bz = t / W2;
  for (int p = 0; p < passes; ++p) {
    const int gx = vx - R + bx, gy = vy - R + by, gz = vz - R + bz;
    bool occ = false;
    if (bz < W && gx >= 0 && gx < nx && gy >= 0 && gy < ny && gz >= 0 && gz < nz)
      occ = state[((long)gz * ny + gy) * nx + gx] == 2;
    const u64 b = __ballot(occ);
    if (lane == 0) {
      const int w = ((p << 8) + t) >> 5;                      // the wave's 64 cells are two whole words
      bits[w] = (unsigned)b;
      bits[w + 1] = (unsigned)(b >> 32);
    }
    box_advance(bx, by, bz, dx, dy, dz, W);
  }
  __syncthreads();

  // (2) the same walk finds the targets; a wave queues them (box offsets + R, 7 bits each) and walks 64 at a time,
  // (3) then the cones of those that arrive.  Pass `passes` only empties the queue.
  const int R2 = R * R;
  unsigned* mine = queue + (t >> 6) * kQueue;                 // this wave's queue; the wave alone reads and writes it
  int queued = 0;                                             // the same in every lane of the wave; < 64 between passes
  bx = t % W, by = (t / W) % W, bz = t / W2;
  for (int p = 0; p <= passes; ++p) {
    if (p < passes) {
      const int ox = bx - R, oy = by - R, oz = bz - R;
      const int gx = vx + ox, gy = vy + oy, gz = vz + oz;
      const int o2 = ox * ox + oy * oy + oz * oz;
      bool cast = false;
      if (bz < W && o2 != 0 && o2 <= R2 && gx >= 0 && gx < nx && gy >= 0 && gy < ny && gz >= 0 && gz < nz)
        cast = state[((long)gz * ny + gy) * nx + gx] == 0;
      const u64 cast_b = __ballot(cast);
      if (cast) mine[queued + __popcll(cast_b & ((1ull << lane) - 1ull))] = (unsigned)(bx | (by << 7) | (bz << 14));
      queued += __popcll(cast_b);
      box_advance(bx, by, bz, dx, dy, dz, W);
    }
    if (queued < 64 && !(p == passes && queued > 0)) continue;
    const int take = min(queued, 64);
    queued -= take;
    wave_lds_fence();                                         // the lanes' stores above, before other lanes read them
    const bool cast = lane < take;
    const unsigned e = cast ? mine[queued + lane] : 0u;
    wave_lds_fence();                                         // and these reads before the next pass stores there
    const int ox = (int)(e & 127u) - R, oy = (int)((e >> 7) & 127u) - R, oz = (int)(e >> 14) - R;
    bool seen = false;
    if (cast) {
      const int ax = abs(ox), ay = abs(oy), az = abs(oz);
      const int mx = max(ax, 1), my = max(ay, 1), mz = max(az, 1);
      const int px = 2 * my * mz, py = 2 * mx * mz, pz = 2 * mx * my;       // a key grows by 2 P per crossing
      int kx = ax ? (px >> 1) : kNever, ky = ay ? (py >> 1) : kNever, kz = az ? (pz >> 1) : kNever;
      const int sx = ox > 0 ? 1 : -1, sy = oy > 0 ? W : -W, sz = oz > 0 ? W2 : -W2;
      int at = (R * W + R) * W + R;                           // the candidate's own box cell
      int left = ax + ay + az;                                // crossings to go; 0 at u
      for (;;) {
        const int m = min(kx, min(ky, kz));
        if (kx == m) at += sx, kx += px, --left;
        if (ky == m) at += sy, ky += py, --left;
        if (kz == m) at += sz, kz += pz, --left;
        if (left == 0) {
          seen = true;
          break;
        }
        if ((bits[at >> 5] >> (at & 31)) & 1u) break;         // an occupied cell between v and u
      }
    }
    const u64 seen_b = __ballot(seen);
    if (seen_b) {                                             // the same in every lane of the wave
      const long long o2l = ox * ox + oy * oy + oz * oz;
      for (int h = 0; h < H; ++h) {
        const long long dot = (long long)ox * hd.axis[h][0] + (long long)oy * hd.axis[h][1] + (long long)oz * hd.axis[h][2];
        const bool in = seen && dot > 0 && dot * dot * den >= hd.norm[h] * o2l;
        const u64 b = __ballot(in);
        if (lane == 0 && b) atomicAdd(&tally[h], (unsigned)__popcll(b));
      }
    }
    if (lane == 0) {
      const unsigned arrived = (unsigned)__popcll(seen_b);
      atomicAdd(&tally[kMaxHeadings], arrived);
      atomicAdd(&tally[kMaxHeadings + 1], (unsigned)take);
      atomicAdd(&tally[kMaxHeadings + 2], (unsigned)take - arrived);
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
  long cells = 0;
  bool ok = state && counters && headings && grid_ok(nx, ny, nz, cells) && V >= 0 && V <= 0x7FFFFFFFl && range >= 1 &&
            range <= kMaxRange && H >= 1 && H <= kMaxHeadings && cos2_den > 0 && cos2_den < (1l << 31) && cos2_num >= 0 &&
            cos2_num <= cos2_den && (V == 0 || (candidates && gain && visible && best));
  Headings hd = {};
  for (int h = 0; ok && h < H; ++h) {
    long long n2 = 0;
    for (int a = 0; a < 3; ++a) {
      const int c = headings[3 * h + a];
      ok = ok && c >= -kMaxAxis && c <= kMaxAxis;
      hd.axis[h][a] = c;
      n2 += (long long)c * c;
    }
    ok = ok && n2 != 0;
    hd.norm[h] = n2 * cos2_num;
  }
  if (!ok) {
    pi3_set_error("pi3_grid_view_gain: bad arguments dims=(%d, %d, %d) (1 .. 2^21 - 1 each, at most 2^27 cells) V=%ld "
                  "(0 .. 2^31 - 1) range=%d (1 .. %d) H=%d (1 .. %d; every axis non-zero, components within +-%d) "
                  "cos2=%ld/%ld (0 <= num <= den, 0 < den < 2^31), or a null pointer", nx, ny, nz, V, range, kMaxRange, H,
                  kMaxHeadings, kMaxAxis, cos2_num, cos2_den);
    return PI3_ERR_ARG;
  }
  if (pi3_zero_words("pi3_grid_view_gain", counters, 4, stream) != PI3_OK) return PI3_ERR_LAUNCH;
  if (V == 0) return PI3_OK;                  // no candidate: no kernel
  const int W = 2 * range + 1;
  const int words = kTally + 4 * kQueue + 8 * ((W * W * W + 255) / 256);      // 8 whole words per pass: 35.7 KB at 32
  hipLaunchKernelGGL(view_gain_kernel, dim3((unsigned)V), dim3(256), (size_t)words * sizeof(unsigned),
                     (hipStream_t)stream, state, nx, ny, nz, candidates, range, H, hd, (long long)cos2_den, gain, visible,
                     best, (u64*)counters);
  return pi3_check_launch("grid_view_gain");
}
