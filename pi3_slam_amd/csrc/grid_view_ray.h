// What the ray kernels of grid_view.hip share (view_gain_kernel and view_mark_kernel): a workgroup of 256 threads per
// view pose, the occupied bits of the (2R + 1)^3 box around it in LDS, a queue of targets per wave and the integer DDA
// on those bits.  grid_view.hip states the rules; every function here is inlined into its kernel.  The far form
// (grid_view_far.hip: a workgroup per pose and octant, ranges up to 64) shares the queue, the DDA, the cone, the tallies
// and the argument check.
#pragma once
#include "grid_tile.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace grid_view_ray {

constexpr int kMaxRange = 32;
constexpr int kFarMaxRange = 64;        // grid_view_far.hip: one octant of W = R + 1 cells per axis is 65^3 bits again
constexpr int kMaxHeadings = 32;
constexpr int kMaxAxis = 1024;          // per component of a heading
constexpr int kNever = 1 << 30;         // the key of an axis the ray does not move along
constexpr int kQueue = 128;             // LDS words per wave: fewer than 64 targets waiting + the 64 of one pass

constexpr int kTally = kMaxHeadings + 3; // LDS words of a gain kernel: a gain per heading, visible, targets, blocked
constexpr int kMarkTally = 4;           // LDS words of a mark kernel: rays, rays visible, in the cone, new
constexpr int kMarkRows = 1024;         // rows of one mark launch

struct Headings {
  int axis[kMaxHeadings][3];
  long long norm[kMaxHeadings];         // num |a|^2
};

struct MarkRows {
  signed char heading[kMarkRows];       // -1: any of the H headings
};

// the arguments the ray entry points share (range in 1 .. max_range); fills hd
inline bool view_rays_ok(const unsigned char* state, int nx, int ny, int nz, long& cells, long V, int range, int max_range,
                         const int* headings, int H, long cos2_num, long cos2_den, const unsigned long long* counters,
                         Headings& hd) {
  bool ok = state && counters && headings && grid_tile::grid_ok(nx, ny, nz, cells) && V >= 0 && V <= 0x7FFFFFFFl &&
            range >= 1 && range <= max_range && H >= 1 && H <= kMaxHeadings && cos2_den > 0 && cos2_den < (1l << 31) &&
            cos2_num >= 0 && cos2_num <= cos2_den;
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
  return ok;
}

// the words of the box's occupied bits: 8 whole words per pass of 256 cells (35.7 KB with the queues at R = 32)
inline int box_words(int R) {
  const int W = 2 * R + 1;
  return 8 * ((W * W * W + 255) / 256);
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

// The box around (vx, vy, vz) as 256 threads walk it, 256 cells per pass in box order (z, y, x).
struct Box {
  int R, W, W2, passes, dx, dy, dz;
  __device__ __forceinline__ explicit Box(int R_) : R(R_), W(2 * R_ + 1) {
    W2 = W * W;
    passes = (W2 * W + 255) >> 8;                              // the box has at most 65^3 cells
    dx = 256 % W, dy = (256 / W) % W, dz = 256 / W2;
  }
  __device__ __forceinline__ void first(int t, int& bx, int& by, int& bz) const { bx = t % W, by = (t / W) % W, bz = t / W2; }
  __device__ __forceinline__ void next(int& bx, int& by, int& bz) const { box_advance(bx, by, bz, dx, dy, dz, W); }
};

// (1) The occupied bits of the box go to `bits`, one bit per cell in box order: thread t of pass i owns box cell
// 256 i + t, reads its state byte (outside the grid: not occupied) and the wave's ballot is stored as two words, so the
// bit of box cell j is bit j & 31 of word j >> 5.  The caller's __syncthreads() follows.
__device__ __forceinline__ void stage_occupied(const Box& b, const unsigned char* __restrict__ state, int nx, int ny,
                                               int nz, int vx, int vy, int vz, int t, unsigned* bits) {
  const int lane = t & 63;
  int bx, by, bz;
  b.first(t, bx, by, bz);
  for (int p = 0; p < b.passes; ++p) {
    const int gx = vx - b.R + bx, gy = vy - b.R + by, gz = vz - b.R + bz;
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

// (2) A wave's queue of targets (box offsets + R, 7 bits each).  `queued` is the same in every lane and < 64 between
// passes; the wave alone reads and writes its queue, so a wave-level fence orders it.
__device__ __forceinline__ void queue_push(unsigned* mine, int& queued, bool cast, int lane, int bx, int by, int bz) {
  const unsigned long long cast_b = __ballot(cast);
  if (cast) mine[queued + __popcll(cast_b & ((1ull << lane) - 1ull))] = (unsigned)(bx | (by << 7) | (bz << 14));
  queued += __popcll(cast_b);
}

// takes up to 64 targets off the queue's end: a lane that `holds` one has its offset from the pose in (ox, oy, oz)
__device__ __forceinline__ int queue_take(unsigned* mine, int& queued, int lane, int R, bool& holds, int& ox, int& oy,
                                          int& oz) {
  const int take = min(queued, 64);
  queued -= take;
  wave_lds_fence();                                           // the lanes' stores, before other lanes read them
  holds = lane < take;
  const unsigned e = holds ? mine[queued + lane] : 0u;
  wave_lds_fence();                                           // and these reads before the next pass stores there
  ox = (int)(e & 127u) - R, oy = (int)((e >> 7) & 127u) - R, oz = (int)(e >> 14) - R;
  return take;
}

// The DDA from the pose's own box cell `at` along (ox, oy, oz) != 0 on the box's bits: does the ray arrive?  A step is
// one LDS word and a handful of integer operations; the box index moves by +-1, +-W, +-W^2.  Up to |o_a| = 64: a key
// grows by 2 P <= 8192 per crossing, at most 64 times per axis, and stays below 2^20 < kNever.
__device__ __forceinline__ bool ray_arrives_from(const unsigned* bits, int at, int W, int W2, int ox, int oy, int oz) {
  const int ax = abs(ox), ay = abs(oy), az = abs(oz);
  const int mx = max(ax, 1), my = max(ay, 1), mz = max(az, 1);
  const int px = 2 * my * mz, py = 2 * mx * mz, pz = 2 * mx * my;       // a key grows by 2 P per crossing
  int kx = ax ? (px >> 1) : kNever, ky = ay ? (py >> 1) : kNever, kz = az ? (pz >> 1) : kNever;
  const int sx = ox > 0 ? 1 : -1, sy = oy > 0 ? W : -W, sz = oz > 0 ? W2 : -W2;
  int left = ax + ay + az;                                    // crossings to go; 0 at u
  bool arrives = false;
  for (;;) {
    const int m = min(kx, min(ky, kz));
    if (kx == m) at += sx, kx += px, --left;
    if (ky == m) at += sy, ky += py, --left;
    if (kz == m) at += sz, kz += pz, --left;
    if (left == 0) {
      arrives = true;
      break;
    }
    if ((bits[at >> 5] >> (at & 31)) & 1u) break;             // an occupied cell between v and u
  }
  return arrives;
}

// the pose in the centre of the (2R + 1)^3 box
__device__ __forceinline__ bool ray_arrives(const unsigned* bits, int R, int W, int W2, int ox, int oy, int oz) {
  return ray_arrives_from(bits, (R * W + R) * W + R, W, W2, ox, oy, oz);
}

// offset o with |o|^2 = o2 lies in heading h's cone: o.a > 0 and (o.a)^2 den >= num |a|^2 |o|^2, in 64 bits
__device__ __forceinline__ bool in_cone(const Headings& hd, int h, long long den, int ox, int oy, int oz, long long o2) {
  const long long dot = (long long)ox * hd.axis[h][0] + (long long)oy * hd.axis[h][1] + (long long)oz * hd.axis[h][2];
  return dot > 0 && dot * dot * den >= hd.norm[h] * o2;
}

}  // namespace grid_view_ray
