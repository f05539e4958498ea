// The ray-casting skeleton of grid_view.hip's gain and mark kernels, each piece once: a workgroup of 256 threads stages
// the occupied bits of a box around a view pose in LDS, walks the box for targets, queues them per wave and runs the
// integer DDA on the bits, 64 rays at a time.  grid_view.hip states the rules (between, visible, target, cone); every
// function here is inlined into its kernel.  The box has two forms, chosen at compile time (kFar):
//
//   near      the whole (2R + 1)^3 box with the pose in the centre, R <= 32: a workgroup per pose casts at every target.
//   octant    a ray from v to u = v + o only touches cells whose offset from v lies, on every axis a, between 0 and o_a:
//             it never leaves the closed octant of its target.  So the far form stages one of the eight octant boxes of
//             W = R + 1 cells per axis: octant q (bit a of q set: axis a negative) covers the offsets 0 .. R on a
//             positive axis and -R .. 0 on a negative one, and the pose sits at box coordinate 0 or R.  At R = 64 that
//             is 65^3 bits, the 34.3 KB the near form stages at R = 32.
//   ownership a target o belongs to exactly one octant: axis a is positive when o_a >= 0.  A negative octant stages its
//             o_a = 0 plane, because its rays pass through it, and never casts at a cell of that plane (RayBox::owns).
//
// Arithmetic at R = 64: a DDA key grows by 2 P <= 2 * 64 * 64 = 8192 per crossing and an axis is crossed at most 64
// times, so a key stays below 2 * 64 * 8192 = 2^20 < kNever = 2^30; the bit index stays below 65^3 = 274 625; box
// coordinates 0 .. 64 fit the queue's 7-bit fields.  No float, no scratch, no inline assembly.
//
// The depth form (kDepth; either box form): a ray also ends when more than K cells between its ends are
// unknown.  The box then has two bit planes, occupied and unknown (state 0 inside the grid), staged from the one read of
// each state byte and interleaved word by word: words 2w and 2w + 1 are the occupied and the unknown bits of box cells
// 32w .. 32w + 31, so a DDA step is one aligned 8-byte LDS read and lane 0 stages a wave's 64 cells with one 16-byte
// write.  The second walk takes its targets from the unknown plane and reads no state byte again.  The count of
// unknown cells is one more register; keys, bit indices and queue fields are those above.  kApart (development build
// only): the two planes one behind the other, two reads per step, the form that was measured against this one.
#pragma once
#include "grid_tile.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace grid_view_ray {

constexpr int kMaxRange = 32;
constexpr int kFarMaxRange = 64;        // one octant of W = R + 1 cells per axis is 65^3 bits again
constexpr int kMaxDepth = 255;          // the depth form: unknown cells a ray may cross
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

// The frustum form's table: a heading is a frame of two orthogonal integer vectors, f forward and r right,
// components within +-kMaxFrame; u = f x r is up or down (its sign squares away).  Offset o lies in the frustum when
//   o.f > 0,  (o.r)^2 |f|^2 hd <= hn (o.f)^2 |r|^2,  (o.u)^2 vd <= vn (o.f)^2 |r|^2   (|u|^2 = |f|^2 |r|^2 divided out)
// with tan^2 of the half angles hn / hd and vn / vd; the faces are inclusive.  A row holds the three constants that
// depend on the frame; vd travels in the kernels' `den`.
constexpr int kMaxFrame = 64;           // per component of f and r
constexpr long kMaxTan2 = 1l << 20;     // the largest numerator and denominator of a tan^2 fraction

struct Frames {
  int f[kMaxHeadings][3], r[kMaxHeadings][3], u[kMaxHeadings][3];
  long long fhd[kMaxHeadings];          // |f|^2 hd
  long long hnr[kMaxHeadings];          // hn |r|^2
  long long vnr[kMaxHeadings];          // vn |r|^2
};

struct MarkRows {
  signed char heading[kMarkRows];       // -1: any of the H headings
};

// the arguments every ray entry point has, cones or frusta (range in 1 .. max_range)
inline bool view_grid_ok(const unsigned char* state, int nx, int ny, int nz, long& cells, long V, int range, int max_range,
                         const unsigned long long* counters) {
  return state && counters && grid_tile::grid_ok(nx, ny, nz, cells) && V >= 0 && V <= 0x7FFFFFFFl && range >= 1 &&
         range <= max_range;
}

// the arguments the cone entry points share (range in 1 .. max_range); fills hd
inline bool view_rays_ok(const unsigned char* state, int nx, int ny, int nz, long& cells, long V, int range, int max_range,
                         const int* headings, int H, long cos2_num, long cos2_den, const unsigned long long* counters,
                         Headings& hd) {
  bool ok = view_grid_ok(state, nx, ny, nz, cells, V, range, max_range, counters) && headings && H >= 1 &&
            H <= kMaxHeadings && cos2_den > 0 && cos2_den < (1l << 31) && cos2_num >= 0 && cos2_num <= cos2_den;
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

// The cone test forms (o.a)^2 den <= range^2 |a|^2 den in 64 bits, so range^2 max |a|^2 den must stay below 2^63 (hd
// as view_rays_ok filled it).  range^2 |a|^2 <= 2^12 * 3 * 2^20 fits easily; the last product is compared by division
// instead of being formed.  Only a range above 32 can fail it: up to there the product is at most 32^2 * 3 * 2^20 *
// 2^31 = 3 * 2^61 < 2^63, so the one host path applies the rule to both forms and only the far messages name it.
inline bool cone_fits(int range, const Headings& hd, int H, long cos2_den) {
  long long most = 0;
  for (int h = 0; h < H; ++h) {
    long long n2 = 0;
    for (int a = 0; a < 3; ++a) n2 += (long long)hd.axis[h][a] * hd.axis[h][a];
    most = n2 > most ? n2 : most;
  }
  return (long long)range * range * most <= 0x7FFFFFFFFFFFFFFFll / (long long)cos2_den;
}

// The frames of the frustum entry points: H rows of f then r, with the checks of the table above; fills fr.
// Why 64 bits hold both sides of both tests without a run-time check: |o|^2 <= 64^2 = 2^12, |f|^2, |r|^2 <= 3 * 64^2 =
// 12288, so (o.r)^2 <= |o|^2 |r|^2 <= 2^12 * 12288 and (o.r)^2 |f|^2 hd <= 2^12 * 12288 * 12288 * 2^20 = 2.25 * 2^58;
// (o.u)^2 vd <= |o|^2 |f|^2 |r|^2 vd is the same figure, and so is either right-hand side, hn (o.f)^2 |r|^2 <=
// 2^20 * 2^12 * 12288 * 12288.  2.25 * 2^58 < 2^63.  The dots fit an int: |o.u| <= 64 * 12288 < 2^20.
inline bool view_frames_ok(const int* frames, int H, long hn, long hd, long vn, long vd, Frames& fr) {
  bool ok = frames && H >= 1 && H <= kMaxHeadings && hn >= 0 && hn <= kMaxTan2 && hd >= 1 && hd <= kMaxTan2 && vn >= 0 &&
            vn <= kMaxTan2 && vd >= 1 && vd <= kMaxTan2;
  for (int h = 0; ok && h < H; ++h) {
    const int* f = frames + 6 * h;
    const int* r = f + 3;
    long long f2 = 0, r2 = 0, fr_dot = 0;
    for (int a = 0; a < 3; ++a) {
      ok = ok && f[a] >= -kMaxFrame && f[a] <= kMaxFrame && r[a] >= -kMaxFrame && r[a] <= kMaxFrame;
      fr.f[h][a] = f[a], fr.r[h][a] = r[a];
      f2 += (long long)f[a] * f[a], r2 += (long long)r[a] * r[a], fr_dot += (long long)f[a] * r[a];
    }
    ok = ok && f2 != 0 && r2 != 0 && fr_dot == 0;
    if (!ok) break;
    fr.u[h][0] = f[1] * r[2] - f[2] * r[1], fr.u[h][1] = f[2] * r[0] - f[0] * r[2], fr.u[h][2] = f[0] * r[1] - f[1] * r[0];
    fr.fhd[h] = f2 * hd, fr.hnr[h] = hn * r2, fr.vnr[h] = vn * r2;
  }
  return ok;
}

// cells per axis of the staged box
__host__ __device__ constexpr int box_width(bool far, int R) { return far ? R + 1 : 2 * R + 1; }

// the words of the box's occupied bits: 8 whole words per pass of 256 cells (W = 65, either form at its largest range:
// 35.7 KB with the queues)
__host__ __device__ inline int box_words(int W) { return 8 * ((W * W * W + 255) / 256); }

// The linear index of cell (gx, gy, gz) inside the grid.  A grid has at most 2^27 cells (grid_tile::grid_ok), so 32
// bits hold it; the two loops that call this wait for the load it addresses once per pass, and a 64-bit product there
// is three dependent v_mad_u64_u32 in front of every load.
__device__ __forceinline__ long cell_index(int nx, int ny, int gx, int gy, int gz) { return (gz * ny + gy) * nx + gx; }

// orders this wave's LDS stores and loads around a hand-over between its lanes (LDS operations of one wave run in
// order; this keeps the compiler from moving them)
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The box of a pose as 256 threads walk it, 256 cells per pass in box order (z, y, x).  Near: the box around the pose.
// Far: octant q of it, the pose in a corner.
template <bool kFar>
struct RayBox {
  int R, W, W2, passes, dx, dy, dz;
  int px, py, pz;                                             // the pose's box coordinate; far: 0 or R (a negative axis)
  __device__ __forceinline__ RayBox(int R_, int q) : R(R_), W(box_width(kFar, R_)) {
    W2 = W * W;
    passes = (W2 * W + 255) >> 8;                              // the box has at most 65^3 cells
    dx = 256 % W, dy = (256 / W) % W, dz = 256 / W2;
    px = (!kFar || (q & 1)) ? R : 0, py = (!kFar || (q & 2)) ? R : 0, pz = (!kFar || (q & 4)) ? R : 0;
  }
  __device__ __forceinline__ void first(int t, int& bx, int& by, int& bz) const {
    bx = t % W, by = (t / W) % W, bz = t / W2;
  }
  // this thread's box cell moves on by 256 cells: (bx, by, bz) += (dx, dy, dz) with carries, 256 = (dz W + dy) W + dx
  __device__ __forceinline__ void next(int& bx, int& by, int& bz) const {
    bx += dx;
    if (bx >= W) bx -= W, ++by;
    by += dy;
    if (by >= W) by -= W, ++bz;
    bz += dz;
  }
  __device__ __forceinline__ int pose_cell() const { return (pz * W + py) * W + px; }
  // THE ownership rule: offset o_a = b_a - p_a belongs to the positive side of axis a when o_a >= 0, so a negative
  // octant (p_a = R) owns b_a < R only.  Its plane b_a = R (o_a = 0) is staged, rays pass through it, but a cell of
  // it is never a target here: the octant that is positive on that axis casts at it.  Every offset of the ball, the
  // axes and planes included, is therefore cast at once.  The near box owns all its cells.
  __device__ __forceinline__ bool owns(int bx, int by, int bz) const {
    return !kFar || ((px == 0 || bx < R) && (py == 0 || by < R) && (pz == 0 || bz < R));
  }
  // no cell this octant owns lies inside the grid: the pose stands on the border its negative axis points across
  __device__ __forceinline__ bool empty(int vx, int vy, int vz) const {
    return kFar && ((px && vx == 0) || (py && vy == 0) || (pz && vz == 0));
  }
};

// the occupied and the unknown word of box cell j's 32 cells in the depth form (`words`: those of one plane)
template <bool kApart>
__device__ __forceinline__ uint2 plane_words(const unsigned* bits, int words, int j) {
  if (kApart) return make_uint2(bits[j >> 5], bits[words + (j >> 5)]);
  return *reinterpret_cast<const uint2*>(bits + ((j >> 5) << 1));        // bits is 16-byte aligned: one ds_read_b64
}

// (1) The occupied bits of the box go to `bits`, one bit per cell in box order: thread t of pass i owns box cell
// 256 i + t, reads its state byte (rows along x: coalesced; outside the grid: not occupied) and the wave's ballot is
// stored as two words, so no LDS atomic is needed and the bit of box cell j is bit j & 31 of word j >> 5.  The
// caller's __syncthreads() follows.  kDepth: the same byte also gives the unknown ballot (outside the grid: not
// unknown), and the wave's four words go out in one 16-byte store (plane_words is the layout's other end).
template <bool kFar, bool kDepth = false, bool kApart = false>
__device__ __forceinline__ void stage_occupied(const RayBox<kFar>& b, const unsigned char* __restrict__ state, int nx,
                                               int ny, int nz, int vx, int vy, int vz, int t, unsigned* bits) {
  const int lane = t & 63;
  int bx, by, bz;
  b.first(t, bx, by, bz);
  for (int p = 0; p < b.passes; ++p) {
    const int gx = vx - b.px + bx, gy = vy - b.py + by, gz = vz - b.pz + bz;
    if constexpr (!kDepth) {
      bool occ = false;
      if (bz < b.W && gx >= 0 && gx < nx && gy >= 0 && gy < ny && gz >= 0 && gz < nz)
        occ = state[cell_index(nx, ny, gx, gy, gz)] == 2;
      const unsigned long long m = __ballot(occ);
      if (lane == 0) {
        const int w = ((p << 8) + t) >> 5;                    // the wave's 64 cells are two whole words
        bits[w] = (unsigned)m;
        bits[w + 1] = (unsigned)(m >> 32);
      }
    } else {
      unsigned char s = 1;                                    // outside the box or the grid: neither plane has it
      if (bz < b.W && gx >= 0 && gx < nx && gy >= 0 && gy < ny && gz >= 0 && gz < nz)
        s = state[cell_index(nx, ny, gx, gy, gz)];
      const unsigned long long m = __ballot(s == 2), k = __ballot(s == 0);
      if (lane == 0) {
        const int w = ((p << 8) + t) >> 5;                    // even: the wave's 64 cells are two whole words per plane
        if (kApart) {
          unsigned* unknown = bits + 8 * b.passes;
          bits[w] = (unsigned)m, bits[w + 1] = (unsigned)(m >> 32);
          unknown[w] = (unsigned)k, unknown[w + 1] = (unsigned)(k >> 32);
        } else {
          *reinterpret_cast<uint4*>(bits + 2 * w) =
              make_uint4((unsigned)m, (unsigned)k, (unsigned)(m >> 32), (unsigned)(k >> 32));
        }
      }
    }
    b.next(bx, by, bz);
  }
}

// is box cell (bx, by, bz) a target of the pose?  Inside the box, owned, in the ball, inside the grid and unknown; u is
// its linear index then.
template <bool kFar>
__device__ __forceinline__ bool is_target(const RayBox<kFar>& b, const unsigned char* __restrict__ state, int nx, int ny,
                                          int nz, int vx, int vy, int vz, int bx, int by, int bz, long& u) {
  const int ox = bx - b.px, oy = by - b.py, oz = bz - b.pz;
  const int gx = vx + ox, gy = vy + oy, gz = vz + oz;
  const int o2 = ox * ox + oy * oy + oz * oz;
  if (!(bz < b.W && b.owns(bx, by, bz) && o2 != 0 && o2 <= b.R * b.R && gx >= 0 && gx < nx && gy >= 0 && gy < ny &&
        gz >= 0 && gz < nz))
    return false;
  u = cell_index(nx, ny, gx, gy, gz);
  return state[u] == 0;
}

// the depth form's is_target, from LDS: box cell j = (bx, by, bz) is owned, in the ball, not the pose, and its unknown
// bit is set, which already says "inside the box, inside the grid and state 0" (the bits behind the box's last cell are
// staged clear).  No state byte is read again.
template <bool kFar, bool kApart>
__device__ __forceinline__ bool is_target_bit(const RayBox<kFar>& b, const unsigned* bits, int words, int j, int bx,
                                              int by, int bz) {
  const int ox = bx - b.px, oy = by - b.py, oz = bz - b.pz;
  const int o2 = ox * ox + oy * oy + oz * oz;
  if (!(b.owns(bx, by, bz) && o2 != 0 && o2 <= b.R * b.R)) return false;
  return (plane_words<kApart>(bits, words, j).y >> (j & 31)) & 1u;
}

// (2) A wave's queue of targets (box coordinates, 7 bits each).  Few lanes of a wave hold a target (3.4 of 64 per pass
// on tools/view_timing.py's flat at R = 32), so a wave does not walk them where they are found: it appends them to its
// queue by ballot ranks and walks 64 at a time.  `queued` is the same in every lane and < 64 between passes; the wave
// alone reads and writes its queue, so a wave-level fence orders it and no atomic is needed.
__device__ __forceinline__ void queue_push(unsigned* mine, int& queued, bool cast, int lane, int bx, int by, int bz) {
  const unsigned long long cast_b = __ballot(cast);
  if (cast) mine[queued + __popcll(cast_b & ((1ull << lane) - 1ull))] = (unsigned)(bx | (by << 7) | (bz << 14));
  queued += __popcll(cast_b);
}

// takes up to 64 targets off the queue's end: a lane that `holds` one has its box coordinate in (bx, by, bz)
__device__ __forceinline__ int queue_take(unsigned* mine, int& queued, int lane, bool& holds, int& bx, int& by, int& bz) {
  const int take = min(queued, 64);
  queued -= take;
  wave_lds_fence();                                           // the lanes' stores, before other lanes read them
  holds = lane < take;
  const unsigned e = holds ? mine[queued + lane] : 0u;
  wave_lds_fence();                                           // and these reads before the next pass stores there
  bx = (int)(e & 127u), by = (int)((e >> 7) & 127u), bz = (int)(e >> 14);
  return take;
}

// The DDA from the pose's own box cell `at` along (ox, oy, oz) != 0 on the box's bits: does the ray arrive?  A step is
// one ds_read_b32 and a handful of integer operations; the box index moves by +-1, +-W, +-W^2.  kDepth: a step reads
// the cell's occupied and unknown word at once (plane_words); an unknown cell between the ends takes one off `spare`,
// which starts at the depth K, and the ray ends at the K + 1st.  The target's own bit is never read.
template <bool kDepth = false, bool kApart = false>
__device__ __forceinline__ bool ray_arrives_from(const unsigned* bits, int at, int W, int W2, int ox, int oy, int oz,
                                                 int words = 0, int spare = 0) {
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
    if constexpr (!kDepth) {
      if ((bits[at >> 5] >> (at & 31)) & 1u) break;           // an occupied cell between v and u
    } else {
      const uint2 w = plane_words<kApart>(bits, words, at);
      if ((w.x >> (at & 31)) & 1u) break;                     // an occupied cell between v and u
      spare -= (int)((w.y >> (at & 31)) & 1u);
      if (spare < 0) break;                                   // more than K unknown cells between them
    }
  }
  return arrives;
}

// offset o with |o|^2 = o2 lies in heading h's cone: o.a > 0 and (o.a)^2 den >= num |a|^2 |o|^2, in 64 bits
__device__ __forceinline__ bool in_cone(const Headings& hd, int h, long long den, int ox, int oy, int oz, long long o2) {
  const long long dot = (long long)ox * hd.axis[h][0] + (long long)oy * hd.axis[h][1] + (long long)oz * hd.axis[h][2];
  return dot > 0 && dot * dot * den >= hd.norm[h] * o2;
}

// offset o lies in frame h's frustum (Frames; vd is the vertical fraction's denominator): three dots, five 64-bit
// products, every constant wave-uniform in h.  view_frames_ok is why nothing overflows.
__device__ __forceinline__ bool in_frustum(const Frames& fr, int h, long long vd, int ox, int oy, int oz) {
  const int df = ox * fr.f[h][0] + oy * fr.f[h][1] + oz * fr.f[h][2];
  const int dr = ox * fr.r[h][0] + oy * fr.r[h][1] + oz * fr.r[h][2];
  const int du = ox * fr.u[h][0] + oy * fr.u[h][1] + oz * fr.u[h][2];
  const long long df2 = (long long)df * df;
  return df > 0 && (long long)dr * dr * fr.fhd[h] <= fr.hnr[h] * df2 && (long long)du * du * vd <= fr.vnr[h] * df2;
}

// the membership test of a kernel's table: the cone of a Headings row, the frustum of a Frames row (den: vd there)
__device__ __forceinline__ bool in_view(const Headings& hd, int h, long long den, int ox, int oy, int oz, long long o2) {
  return in_cone(hd, h, den, ox, oy, oz, o2);
}
__device__ __forceinline__ bool in_view(const Frames& fr, int h, long long den, int ox, int oy, int oz, long long) {
  return in_frustum(fr, h, den, ox, oy, oz);
}

// (2) and the DDA of (3), after stage_occupied and the caller's __syncthreads(): the same walk over the box finds the
// targets (kUnseen: only a cell whose bit of `seen` is clear; `seen` is not read otherwise), the wave queues them and,
// whenever 64 wait, takes them and casts their rays.  Pass `passes` only empties the queue.  on_batch(take, arrived,
// arrived_b, ox, oy, oz) gets each batch, every lane of the wave at once: `take` rays were cast, this lane's went along
// (ox, oy, oz) and `arrived` (false in a lane that held none), arrived_b is the ballot of that.
template <bool kFar, bool kUnseen, bool kDepth = false, bool kApart = false, class OnBatch>
__device__ __forceinline__ void cast_rays(const RayBox<kFar>& box, const unsigned char* __restrict__ state, int nx,
                                          int ny, int nz, const unsigned* __restrict__ seen, int vx, int vy, int vz,
                                          int t, unsigned* queue, const unsigned* bits, OnBatch on_batch, int depth = 0) {
  const int lane = t & 63;
  const int home = box.pose_cell();
  unsigned* mine = queue + (t >> 6) * kQueue;                 // this wave's queue; the wave alone reads and writes it
  const int words = 8 * box.passes;                           // of one plane (the depth form alone uses it)
  int queued = 0;                                             // the same in every lane of the wave; < 64 between passes
  int bx, by, bz;
  box.first(t, bx, by, bz);
  for (int p = 0; p <= box.passes; ++p) {
    if (p < box.passes) {
      long u = 0;
      bool cast = !kDepth && is_target(box, state, nx, ny, nz, vx, vy, vz, bx, by, bz, u);
      if (kUnseen && !kDepth) cast = cast && !((seen[u >> 5] >> (u & 31)) & 1u);     // lanes along x read the same word
      if constexpr (kDepth) {
        cast = is_target_bit<kFar, kApart>(box, bits, words, (p << 8) + t, bx, by, bz);
        if (kUnseen && cast) {                                // a target lies inside the grid
          u = cell_index(nx, ny, vx - box.px + bx, vy - box.py + by, vz - box.pz + bz);
          cast = !((seen[u >> 5] >> (u & 31)) & 1u);
        }
      }
      queue_push(mine, queued, cast, lane, bx, by, bz);
      box.next(bx, by, bz);
    }
    if (queued < 64 && !(p == box.passes && queued > 0)) continue;
    int ox, oy, oz;
    bool holds;
    const int take = queue_take(mine, queued, lane, holds, ox, oy, oz);
    ox -= box.px, oy -= box.py, oz -= box.pz;
    bool arrived = false;
    if (holds) arrived = ray_arrives_from<kDepth, kApart>(bits, home, box.W, box.W2, ox, oy, oz, words, depth);
    on_batch(take, arrived, (unsigned long long)__ballot(arrived), ox, oy, oz);
  }
}

}  // namespace grid_view_ray
