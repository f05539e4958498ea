// Views of the occupancy grid (occupancy.hip's layout: state u8 [nz][ny][nx], x fastest, cell (ix, iy, iz) at the linear
// index (iz ny + iy) nx + ix; 0 unknown, 1 free, 2 occupied): how much unknown space does a pose see, and in which
// direction?  Integers only; tests/grid_view_ref.py reproduces every output byte for byte.
//
//   between   cell m lies between v and u when the open segment between their centres meets m's open interior; v and u
//             never count, and a cell the segment only touches at a face, edge or corner does not either.  That is the
//             integer DDA from v along o = u - v: axis a has its k-th crossing at t = (2k - 1) / (2 |o_a|); always the
//             smallest t, all axes tied at that t step at once, stop at u.  Over the common denominator 2 |o_x o_y o_z|
//             (a zero length counts as 1) the crossing is the integer key_a = (2k - 1) P_a, P_a = the product of the
//             other two lengths, compared exactly.
//   visible   u is visible from v when no cell between them is occupied.  Unknown and free cells are transparent.
//   target    of candidate v at range R: u != v inside the grid with |u - v|^2 <= R^2 and state[u] == 0.
//   cone      offset o lies in heading a's cone when o.a > 0 and (o.a)^2 den >= num |o|^2 |a|^2, in 64 bits (|a_i| <=
//             1024, den < 2^31; grid_view_ray::cone_fits is the bound on the range that goes with them).
//
//   pi3_grid_view_candidates  a thread per cell of a settled route field: the reachable cells within max_cost on the
//                             lattice of the absolute index, compacted in any order like pi3_grid_frontier_roots.
//   pi3_grid_view_gain        a workgroup of 256 threads per candidate runs grid_view_ray.h's skeleton on the
//                             (2R + 1)^3 box around it, R <= 32: (1) the occupied bits of the box go to LDS, (2) the
//                             same walk over the box again finds the targets, which each wave queues and casts at 64 at
//                             a time with the DDA above on the LDS bits.  (3) After the wave's rays have ended, every
//                             heading is a ballot over the lanes whose ray arrived, and one lane adds the count to the
//                             heading's LDS word.  Integer sums only: the bytes do not depend on the order.
//
// Views that cover (tests/grid_cover_ref.py): seen is a bit per cell, cell c at bit c & 31 of word c >> 5, for "a kept
// view sees it".
//   pi3_grid_view_gain_unseen the same kernel, instantiated with one more condition in (2): the cell's bit of seen is
//                             clear.  Lanes along x read the same word: one broadcast load next to the state byte.
//   pi3_grid_view_mark        a workgroup per row (cell, heading): (1) and (2) with every unknown cell of the ball a
//                             target, then a lane whose ray arrived inside the heading's cone (-1: any heading's) ORs
//                             its cell's bit into seen.
//
// Views that see farther: the _far entry points run the same three kernels at a range of up to 64 cells on
// octant boxes (grid_view_ray.h: octant, ownership, the arithmetic at R = 64).  The rules above, mark's "only when the
// bit reads clear", owner and the counters are unchanged.
//   grid      (poses, 8): a workgroup of 256 threads per pose and octant, so that a single pose (cover marks one view
//             per round) still fills eight workgroups.  The looping form (one workgroup, eight octants in turn) was not
//             measured; this is the only form.
//   sums      every workgroup adds its LDS tally to gain[v][h], visible[v] and the counters with integer atomics: order
//             free, so the bytes are fixed.  The entry point zeroes them first, on the stream; octant 0 alone counts the
//             pose; view_best_kernel, a thread per pose, writes best afterwards.  mark needs no finishing.
//
// Unknown space that ends a ray (tests/grid_view_depth_ref.py): the _depth entry points run the same kernels,
// near (far = 0) or far (far = 1), with one more rule.
//   depth     K in 0 .. 255: u is visible from v when no cell between them is occupied and at most K cells between
//             them are unknown.  "Between" is the rule above; v and u never count, so the target's own state does not.
//             A ray has at most |o|_1 - 1 cells between its ends, 109 over the ball of 64 cells: K >= 110 gives the
//             transparent bytes.  Targets, ball, cone, best, seen, owner and the counters' layout are unchanged;
//             "blocked" is every ray that did not arrive, whichever rule ended it.
//   LDS       two bit planes (grid_view_ray.h), twice the box words: above 64 KB from W = 64 on (near R = 32, far
//             R >= 63), so those launches opt in to their LDS size first (pi3_lds_optin, a done-mask per kernel).
//   argument  the kernels keep their argument list: the depth form's `R` carries range | K << 8.
#include "common.h"
#include "grid_tile.h"
#include "grid_view_ray.h"
#include "voxel_table.h"
#include "wave_block.h"

#include <stdint.h>

namespace {

using grid_tile::grid_ok;
using grid_view_ray::Frames;
using grid_view_ray::Headings;
using grid_view_ray::kFarMaxRange;
using grid_view_ray::kMarkRows;
using grid_view_ray::kMarkTally;
using grid_view_ray::kMaxDepth;
using grid_view_ray::kMaxFrame;
using grid_view_ray::kMaxAxis;
using grid_view_ray::kMaxHeadings;
using grid_view_ray::kMaxRange;
using grid_view_ray::kQueue;
using grid_view_ray::kTally;
using grid_view_ray::MarkRows;
using grid_view_ray::RayBox;
using voxel_table::u64;
using wave_block::block_exclusive_scan;

constexpr unsigned kUnreached = 0xFFFFFFFFu;      // grid_route.hip's mark of a cell no route reaches

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
    if (d != kUnreached && d <= max_cost) {
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

// A workgroup per candidate (blockIdx.x), in the far form per candidate and octant (blockIdx.y).  kUnseen: a cell is a
// target only when its bit of `seen` is clear (pi3_grid_view_gain_unseen); `seen` is not read otherwise.  Near: gain,
// visible and best are stored.  Far: gain, visible and the counters were zeroed by the entry point and take atomic
// sums; best is view_best_kernel's.  kDepth: R carries range | K << 8, and the LDS holds two planes (kApart: one
// behind the other, development build only).  Table: Headings (cones) or Frames (frusta; `den` is then the
// vertical fraction's denominator); grid_view_ray::in_view is the only place where the two differ.
template <bool kUnseen, bool kFar, bool kDepth = false, bool kApart = false, class Table = Headings>
__global__ __launch_bounds__(256) void view_gain_kernel(const unsigned char* __restrict__ state, int nx, int ny, int nz,
                                                        const unsigned* __restrict__ seen,
                                                        const long* __restrict__ candidates, int R, int H,
                                                        const Table hd, long long den, unsigned* gain,
                                                        unsigned* visible, int* __restrict__ best, u64* counters) {
  extern __shared__ unsigned lds[];                           // kTally words, a queue per wave, the box's occupied bits
  const int range = kDepth ? R & 255 : R, depth = kDepth ? R >> 8 : 0;
  const int planes = kDepth ? 2 * grid_view_ray::box_words(grid_view_ray::box_width(kFar, range)) : 0;
  unsigned* tally = lds + planes;                             // depth: behind the two planes, which start the LDS
  unsigned* queue = tally + kTally;
  unsigned* bits = kDepth ? static_cast<unsigned*>(__builtin_assume_aligned(lds, 16)) : queue + 4 * kQueue;
  const int t = (int)threadIdx.x, lane = t & 63;
  const long v = candidates[blockIdx.x];
  const long cells = (long)nx * ny * nz;
  if (v < 0 || v >= cells) {                                  // the same in every thread
    if (!kFar) {                                              // far: the entry point's zeros stand, and best = -1
      if (t < H) gain[(long)blockIdx.x * H + t] = 0u;
      if (t == 0) visible[blockIdx.x] = 0u, best[blockIdx.x] = -1;
    }
    return;
  }
  const int line = (int)v / nx;
  const int vx = (int)v - line * nx, vy = line % ny, vz = line / ny;
  const RayBox<kFar> box(range, (int)blockIdx.y);
  if (kFar) {
    if (blockIdx.y == 0 && t == 0) atomicAdd(counters + 0, 1ull);      // the pose is counted once, not per octant
    if (box.empty(vx, vy, vz)) return;                        // the same in every thread
  }
  if (t < kTally) tally[t] = 0u;
  grid_view_ray::stage_occupied<kFar, kDepth, kApart>(box, state, nx, ny, nz, vx, vy, vz, t, bits);
  __syncthreads();

  // (3) the cones of the rays that arrived
  grid_view_ray::cast_rays<kFar, kUnseen, kDepth, kApart>(
      box, state, nx, ny, nz, seen, vx, vy, vz, t, queue, bits,
      [&](int take, bool arrived, u64 arrived_b, int ox, int oy, int oz) {
        if (arrived_b) {                                      // the same in every lane of the wave
          const long long o2l = ox * ox + oy * oy + oz * oz;
          for (int h = 0; h < H; ++h) {
            const u64 b = __ballot(grid_view_ray::in_view(hd, h, den, ox, oy, oz, o2l) && arrived);
            if (lane == 0 && b) atomicAdd(&tally[h], (unsigned)__popcll(b));
          }
        }
        if (lane == 0) {
          const unsigned n = (unsigned)__popcll(arrived_b);
          atomicAdd(&tally[kMaxHeadings], n);
          atomicAdd(&tally[kMaxHeadings + 1], (unsigned)take);
          atomicAdd(&tally[kMaxHeadings + 2], (unsigned)take - n);
        }
      },
      depth);
  __syncthreads();
  if (kFar) {
    if (t < H && tally[t]) atomicAdd(&gain[(long)blockIdx.x * H + t], tally[t]);
  } else {
    if (t < H) gain[(long)blockIdx.x * H + t] = tally[t];
  }
  if (t == 0) {
    if (kFar) {
      if (tally[kMaxHeadings]) atomicAdd(&visible[blockIdx.x], tally[kMaxHeadings]);
    } else {
      int first = 0;
      for (int h = 1; h < H; ++h)
        if (tally[h] > tally[first]) first = h;               // the smallest heading of the largest gain
      best[blockIdx.x] = first;
      visible[blockIdx.x] = tally[kMaxHeadings];
      atomicAdd(counters + 0, 1ull);
    }
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

// A workgroup per row (cells[i], rows.heading[same ? 0 : i]), in the far form per row and octant: the gain kernel's box,
// queue and DDA with every unknown cell of the ball a target (the mask does not thin the rays).  A lane whose ray
// arrived inside the row's cone reads the cell's word of `seen` and, only when the bit is clear, ORs it in; the bit is
// new when the returned word had it clear, so of several rows that race for one cell exactly one counts it.  owner is
// written by that lane alone.  kDepth, kApart and Table as the gain kernel's.
template <bool kFar, bool kDepth = false, bool kApart = false, class Table = Headings>
__global__ __launch_bounds__(256) void view_mark_kernel(const unsigned char* __restrict__ state, int nx, int ny, int nz,
                                                        unsigned* seen, const long* __restrict__ cells_in,
                                                        const MarkRows rows, int same, int R, int H, const Table hd,
                                                        long long den, short* owner, int tag, u64* counters) {
  extern __shared__ unsigned lds[];                           // kMarkTally words, a queue per wave, the occupied bits
  const int range = kDepth ? R & 255 : R, depth = kDepth ? R >> 8 : 0;
  const int planes = kDepth ? 2 * grid_view_ray::box_words(grid_view_ray::box_width(kFar, range)) : 0;
  unsigned* tally = lds + planes;                             // depth: behind the two planes, which start the LDS
  unsigned* queue = tally + kMarkTally;
  unsigned* bits = kDepth ? static_cast<unsigned*>(__builtin_assume_aligned(lds, 16)) : queue + 4 * kQueue;
  const int t = (int)threadIdx.x, lane = t & 63;
  const long v = cells_in[blockIdx.x];
  const long cells = (long)nx * ny * nz;
  if (v < 0 || v >= cells) return;                            // the same in every thread: no view
  const int heading = rows.heading[same ? 0 : blockIdx.x];
  const int line = (int)v / nx;
  const int vx = (int)v - line * nx, vy = line % ny, vz = line / ny;
  const RayBox<kFar> box(range, (int)blockIdx.y);
  if (kFar) {
    if (blockIdx.y == 0 && t == 0) atomicAdd(counters + 0, 1ull);      // the view is counted once, not per octant
    if (box.empty(vx, vy, vz)) return;                        // the same in every thread
  }
  if (t < kMarkTally) tally[t] = 0u;
  grid_view_ray::stage_occupied<kFar, kDepth, kApart>(box, state, nx, ny, nz, vx, vy, vz, t, bits);
  __syncthreads();

  grid_view_ray::cast_rays<kFar, false, kDepth, kApart>(
      box, state, nx, ny, nz, nullptr, vx, vy, vz, t, queue, bits,
      [&](int take, bool arrived, u64 arrived_b, int ox, int oy, int oz) {
        bool in = false, fresh = false;
        if (arrived_b) {                                      // the same in every lane of the wave
          const long long o2l = ox * ox + oy * oy + oz * oz;
          if (heading >= 0) {
            in = grid_view_ray::in_view(hd, heading, den, ox, oy, oz, o2l) && arrived;
          } else {
            for (int h = 0; h < H; ++h) in = in || (grid_view_ray::in_view(hd, h, den, ox, oy, oz, o2l) && arrived);
          }
          if (in) {                                           // a target: inside the grid, so u < cells
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
      },
      depth);
  __syncthreads();
  if (t == 0) {
    if (!kFar) atomicAdd(counters + 0, 1ull);
    for (int i = 0; i < kMarkTally; ++i)
      if (tally[i]) atomicAdd(counters + 1 + i, (u64)tally[i]);
  }
}

// What an entry point's form decides on the host: its name, its largest range, near or far, and what the far messages
// add about the cone (grid_view_ray::cone_fits is checked for both forms and can fail only above kMaxRange).
// The depth form (the _depth entry points) adds: its depth K, which its messages name, twice the box words, and the
// kernels' `R` argument as range | K << 8.  Every other entry point is not `deep`: transparent, and none of that.
struct Form {
  const char* who;
  bool far;
  bool deep = false;
  int depth = 0;
  char depth_text[48] = "";                                   // " depth=K (0 .. 255)" in the depth form's messages
  Form(const char* who_, bool far_) : who(who_), far(far_) {}
  Form(const char* who_, int far_, int depth_) : who(who_), far(far_ != 0), deep(true), depth(depth_) {
    snprintf(depth_text, sizeof depth_text, " depth=%d (0 .. %d)", depth, kMaxDepth);
  }
  // the frustum entry points' depth: -1 is the transparent form
  static Form or_transparent(const char* who_, int far_, int depth_) {
    Form form(who_, far_, depth_);
    form.deep = depth_ != -1;
    snprintf(form.depth_text, sizeof form.depth_text, " depth=%d (-1: transparent, else 0 .. %d)", depth_, kMaxDepth);
    return form;
  }
  bool depth_ok() const { return !deep || (depth >= 0 && depth <= kMaxDepth); }
  int max_range() const { return far ? kFarMaxRange : kMaxRange; }
  const char* cone_rule() const { return far ? "; the cone test's 64 bits: range^2 * max |axis|^2 * den < 2^63" : ""; }
  size_t lds_bytes(int tally, int range) const {              // the tally, a queue per wave, the box's bits
    const int words = grid_view_ray::box_words(grid_view_ray::box_width(far, range));
    return (size_t)(tally + 4 * kQueue + (deep ? 2 : 1) * words) * sizeof(unsigned);
  }
  int kernel_range(int range) const { return deep ? range | (depth << 8) : range; }
  dim3 grid(long n) const { return dim3((unsigned)n, far ? 8 : 1); }
};

// A depth kernel and the opt-in to its LDS size: above the 64 KB every kernel may have, the launch asks for the form's
// largest size first, once per device (the mask is a static of this instantiation, one per kernel instance).
constexpr size_t kLdsDefault = 64 * 1024;
template <auto KERN>
int depth_optin(size_t bytes, size_t most, const char* what) {
  static unsigned long long done = 0;
  return bytes <= kLdsDefault ? PI3_OK : pi3_lds_optin((const void*)KERN, (int)most, &done, what);
}
template <class Kernel>
struct DepthLaunch {
  Kernel kernel;
  int (*optin)(size_t bytes, size_t most, const char* what);
};
template <class Table>
using GainKernel = decltype(&view_gain_kernel<false, false, false, false, Table>);
template <class Table>
using MarkKernel = decltype(&view_mark_kernel<false, false, false, Table>);

template <class Table>
GainKernel<Table> plain_gain(bool unseen, bool far) {
  return far ? (unseen ? view_gain_kernel<true, true, false, false, Table> : view_gain_kernel<false, true, false, false, Table>)
             : (unseen ? view_gain_kernel<true, false, false, false, Table>
                       : view_gain_kernel<false, false, false, false, Table>);
}

template <class Table>
MarkKernel<Table> plain_mark(bool far) {
  return far ? view_mark_kernel<true, false, false, Table> : view_mark_kernel<false, false, false, Table>;
}

template <bool kApart, class Table>
DepthLaunch<GainKernel<Table>> depth_gain(bool unseen, bool far) {
#define PI3_VIEW_GAIN(U, F) DepthLaunch<GainKernel<Table>>{view_gain_kernel<U, F, true, kApart, Table>, depth_optin<view_gain_kernel<U, F, true, kApart, Table>>}
  return far ? (unseen ? PI3_VIEW_GAIN(true, true) : PI3_VIEW_GAIN(false, true))
             : (unseen ? PI3_VIEW_GAIN(true, false) : PI3_VIEW_GAIN(false, false));
#undef PI3_VIEW_GAIN
}

template <bool kApart, class Table>
DepthLaunch<MarkKernel<Table>> depth_mark(bool far) {
  if (far) return {view_mark_kernel<true, true, kApart, Table>, depth_optin<view_mark_kernel<true, true, kApart, Table>>};
  return {view_mark_kernel<false, true, kApart, Table>, depth_optin<view_mark_kernel<false, true, kApart, Table>>};
}

// the planes one behind the other: the development build alone has that form (PI3_VIEW_DEPTH_APART=1); the product
// library instantiates the interleaved kernels only
#ifdef PI3_DEV_VARIANTS
constexpr bool kDevVariants = true;
#else
constexpr bool kDevVariants = false;
#endif
bool planes_apart() { return PI3_DEV_ENV_INT("PI3_VIEW_DEPTH_APART", 0) != 0; }

// What an entry point tests the rays that arrived against, on the host: the kernels' table type, the checks that fill
// it (with the arguments every ray entry point has), the kernels' `den`, and its part of the error message (`rows`: what
// mark adds about its rows' headings).  Cones: every entry point but the _frustum ones.
struct Cones {
  using Table = Headings;
  const int* headings;
  int H;
  long num, den;
  bool ok(const Form& form, const unsigned char* state, int nx, int ny, int nz, long& cells, long V, int range,
          const unsigned long long* counters, Table& hd) const {
    return grid_view_ray::view_rays_ok(state, nx, ny, nz, cells, V, range, form.max_range(), headings, H, num, den,
                                       counters, hd) &&
           grid_view_ray::cone_fits(range, hd, H, den);
  }
  long long kernel_den() const { return den; }
  void rules(char* text, size_t n, const Form& form, const char* rows) const {
    snprintf(text, n, "H=%d (1 .. %d; every axis non-zero, components within +-%d%s) cos2=%ld/%ld (0 <= num <= den, "
             "0 < den < 2^31%s)", H, kMaxHeadings, kMaxAxis, rows, num, den, form.cone_rule());
  }
};

// Frusta: frames of f then r and the two tan^2 fractions; no rule depends on the range.
struct Frusta {
  using Table = Frames;
  const int* frames;
  int H;
  long hn, hd, vn, vd;
  bool ok(const Form& form, const unsigned char* state, int nx, int ny, int nz, long& cells, long V, int range,
          const unsigned long long* counters, Table& fr) const {
    return grid_view_ray::view_grid_ok(state, nx, ny, nz, cells, V, range, form.max_range(), counters) &&
           grid_view_ray::view_frames_ok(frames, H, hn, hd, vn, vd, fr);
  }
  long long kernel_den() const { return vd; }
  void rules(char* text, size_t n, const Form&, const char* rows) const {
    snprintf(text, n, "H=%d (1 .. %d; every frame f then r: both non-zero, f.r = 0, components within +-%d%s) "
             "tan2_h=%ld/%ld tan2_v=%ld/%ld (0 <= num <= 2^20, 1 <= den <= 2^20)", H, kMaxHeadings, kMaxFrame, rows, hn,
             hd, vn, vd);
  }
};

// every gain entry point: seen == nullptr unless unseen
template <class Shape>
int view_gain(Form form, bool unseen, const unsigned char* state, int nx, int ny, int nz, const unsigned* seen,
              const long* candidates, long V, int range, const Shape shape, unsigned* gain, unsigned* visible, int* best,
              unsigned long long* counters, void* stream) {
  using Table = typename Shape::Table;
  const char* who = form.who;
  const int H = shape.H;
  long cells = 0;
  Table hd = {};
  const bool ok = shape.ok(form, state, nx, ny, nz, cells, V, range, counters, hd) &&
                  (V == 0 || (candidates && gain && visible && best)) && (!unseen || seen) && form.depth_ok();
  if (!ok) {
    char rules[384];
    shape.rules(rules, sizeof rules, form, "");
    pi3_set_error("%s: bad arguments dims=(%d, %d, %d) (1 .. 2^21 - 1 each, at most 2^27 cells) V=%ld "
                  "(0 .. 2^31 - 1) range=%d (1 .. %d)%s %s, or a null pointer", who, nx, ny, nz, V, range,
                  form.max_range(), form.depth_text, rules);
    return PI3_ERR_ARG;
  }
  const hipStream_t s = (hipStream_t)stream;
  if (pi3_zero_words(who, counters, 4, stream) != PI3_OK) return PI3_ERR_LAUNCH;
  if (V == 0) return PI3_OK;                  // no candidate: no kernel
  if (form.far && (hipMemsetAsync(gain, 0, (size_t)V * H * sizeof(unsigned), s) != hipSuccess ||
                   hipMemsetAsync(visible, 0, (size_t)V * sizeof(unsigned), s) != hipSuccess)) {
    pi3_set_error("%s: hipMemsetAsync failed", who);
    return PI3_ERR_LAUNCH;
  }
  auto kernel = plain_gain<Table>(unseen, form.far);
  if (form.deep) {
    const auto deep = planes_apart() ? depth_gain<kDevVariants, Table>(unseen, form.far)
                                     : depth_gain<false, Table>(unseen, form.far);
    if (int rc = deep.optin(form.lds_bytes(kTally, range), form.lds_bytes(kTally, form.max_range()), who + 4)) return rc;
    kernel = deep.kernel;
  }
  hipLaunchKernelGGL(kernel, form.grid(V), dim3(256), form.lds_bytes(kTally, range), s, state, nx, ny, nz, seen,
                     candidates, form.kernel_range(range), H, hd, shape.kernel_den(), gain, visible, best,
                     (u64*)counters);
  const int rc = pi3_check_launch(who + 4);   // without "pi3_"
  if (rc != PI3_OK || !form.far) return rc;
  hipLaunchKernelGGL(view_best_kernel, dim3(voxel_table::blocks_for(V)), dim3(256), 0, s, candidates, V, cells, H,
                     (const unsigned*)gain, best);
  return pi3_check_launch(who + 4);
}

// every mark entry point
template <class Shape>
int view_mark(Form form, const unsigned char* state, int nx, int ny, int nz, unsigned* seen, const long* cells_in,
              const int* heading_of, long V, int range, const Shape shape, short* owner, int tag,
              unsigned long long* counters, void* stream) {
  using Table = typename Shape::Table;
  const int H = shape.H;
  long cells = 0;
  Table hd = {};
  bool ok = shape.ok(form, state, nx, ny, nz, cells, V, range, counters, hd) && seen &&
            (V == 0 || (cells_in && heading_of)) && tag >= 0 && tag < 32768 && (!owner || V == 1) && form.depth_ok();
  for (long i = 0; ok && i < V; ++i) ok = heading_of[i] >= -1 && heading_of[i] < H;
  if (!ok) {
    char rules[384];
    shape.rules(rules, sizeof rules, form, "; every row's heading in -1 .. H - 1");
    pi3_set_error("%s: bad arguments dims=(%d, %d, %d) (1 .. 2^21 - 1 each, at most 2^27 cells) V=%ld "
                  "(0 .. 2^31 - 1; 1 with an owner) range=%d (1 .. %d)%s %s tag=%d (0 .. 32767), or a null pointer",
                  form.who, nx, ny, nz, V, range, form.max_range(), form.depth_text, rules, tag);
    return PI3_ERR_ARG;
  }
  if (pi3_zero_words(form.who, counters, 1 + kMarkTally, stream) != PI3_OK) return PI3_ERR_LAUNCH;
  // The rows' headings travel by value.  One heading for all rows (a single view, the seeable pass) is one launch;
  // else kMarkRows rows per launch, which costs a large batch the balance of one grid over all its rows.
  bool same = true;
  for (long i = 1; same && i < V; ++i) same = heading_of[i] == heading_of[0];
  const long step = same ? V : kMarkRows;
  MarkRows rows;
  auto kernel = plain_mark<Table>(form.far);
  if (form.deep && V > 0) {
    const auto deep = planes_apart() ? depth_mark<kDevVariants, Table>(form.far) : depth_mark<false, Table>(form.far);
    if (int rc = deep.optin(form.lds_bytes(kMarkTally, range), form.lds_bytes(kMarkTally, form.max_range()), form.who + 4))
      return rc;
    kernel = deep.kernel;
  }
  for (long base = 0; base < V; base += step) {
    const long n = V - base < step ? V - base : step;
    for (int i = 0; i < kMarkRows; ++i) rows.heading[i] = (signed char)(i < n ? heading_of[base + i] : -1);
    hipLaunchKernelGGL(kernel, form.grid(n), dim3(256), form.lds_bytes(kMarkTally, range), (hipStream_t)stream, state,
                       nx, ny, nz, seen, cells_in + base, rows, same ? 1 : 0, form.kernel_range(range), H, hd,
                       shape.kernel_den(), owner, tag, (u64*)counters);
    const int rc = pi3_check_launch(form.who + 4);            // without "pi3_"
    if (rc != PI3_OK) return rc;
  }
  return PI3_OK;
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
  const unsigned limit = max_cost >= (long)kUnreached ? kUnreached - 1u : (unsigned)max_cost;       // that mark never passes
  hipLaunchKernelGGL(view_candidates_kernel, dim3(voxel_table::blocks_for(cells)), dim3(256), 0, (hipStream_t)stream,
                     dist, nx, ny, (int)cells, ox, oy, oz, stride, limit, cells_out, cap, (u64*)count);
  return pi3_check_launch("grid_view_candidates");
}

extern "C" int pi3_grid_view_gain(const unsigned char* state, int nx, int ny, int nz, const long* candidates, long V,
                                  int range, const int* headings, int H, long cos2_num, long cos2_den, unsigned* gain,
                                  unsigned* visible, int* best, unsigned long long* counters, void* stream) {
  return view_gain({"pi3_grid_view_gain", false}, false, state, nx, ny, nz, nullptr, candidates, V, range, Cones{headings, H, cos2_num, cos2_den}, gain, visible, best, counters, stream);
}

extern "C" int pi3_grid_view_gain_unseen(const unsigned char* state, int nx, int ny, int nz, const unsigned* seen,
                                         const long* candidates, long V, int range, const int* headings, int H,
                                         long cos2_num, long cos2_den, unsigned* gain, unsigned* visible, int* best,
                                         unsigned long long* counters, void* stream) {
  return view_gain({"pi3_grid_view_gain_unseen", false}, true, state, nx, ny, nz, seen, candidates, V, range, Cones{headings, H, cos2_num, cos2_den}, gain, visible, best, counters, stream);
}

extern "C" int pi3_grid_view_mark(const unsigned char* state, int nx, int ny, int nz, unsigned* seen, const long* cells_in,
                                  const int* heading_of, long V, int range, const int* headings, int H, long cos2_num,
                                  long cos2_den, short* owner, int tag, unsigned long long* counters, void* stream) {
  return view_mark({"pi3_grid_view_mark", false}, state, nx, ny, nz, seen, cells_in, heading_of, V, range, Cones{headings, H, cos2_num, cos2_den}, owner, tag, counters, stream);
}

extern "C" int pi3_grid_view_gain_far(const unsigned char* state, int nx, int ny, int nz, const long* candidates, long V,
                                      int range, const int* headings, int H, long cos2_num, long cos2_den,
                                      unsigned* gain, unsigned* visible, int* best, unsigned long long* counters,
                                      void* stream) {
  return view_gain({"pi3_grid_view_gain_far", true}, false, state, nx, ny, nz, nullptr, candidates, V, range, Cones{headings, H, cos2_num, cos2_den}, gain, visible, best, counters, stream);
}

extern "C" int pi3_grid_view_gain_unseen_far(const unsigned char* state, int nx, int ny, int nz, const unsigned* seen,
                                             const long* candidates, long V, int range, const int* headings, int H,
                                             long cos2_num, long cos2_den, unsigned* gain, unsigned* visible, int* best,
                                             unsigned long long* counters, void* stream) {
  return view_gain({"pi3_grid_view_gain_unseen_far", true}, true, state, nx, ny, nz, seen, candidates, V, range, Cones{headings, H, cos2_num, cos2_den}, gain, visible, best, counters, stream);
}

extern "C" int pi3_grid_view_mark_far(const unsigned char* state, int nx, int ny, int nz, unsigned* seen,
                                      const long* cells_in, const int* heading_of, long V, int range, const int* headings,
                                      int H, long cos2_num, long cos2_den, short* owner, int tag,
                                      unsigned long long* counters, void* stream) {
  return view_mark({"pi3_grid_view_mark_far", true}, state, nx, ny, nz, seen, cells_in, heading_of, V, range, Cones{headings, H, cos2_num, cos2_den}, owner, tag, counters, stream);
}

extern "C" int pi3_grid_view_gain_depth(const unsigned char* state, int nx, int ny, int nz, const unsigned* seen,
                                        const long* candidates, long V, int range, int depth, int far,
                                        const int* headings, int H, long cos2_num, long cos2_den, unsigned* gain,
                                        unsigned* visible, int* best, unsigned long long* counters, void* stream) {
  return view_gain({"pi3_grid_view_gain_depth", far, depth}, seen != nullptr, state, nx, ny, nz, seen, candidates, V,
                   range, Cones{headings, H, cos2_num, cos2_den}, gain, visible, best, counters, stream);
}

extern "C" int pi3_grid_view_mark_depth(const unsigned char* state, int nx, int ny, int nz, unsigned* seen,
                                        const long* cells_in, const int* heading_of, long V, int range, int depth, int far,
                                        const int* headings, int H, long cos2_num, long cos2_den, short* owner, int tag,
                                        unsigned long long* counters, void* stream) {
  return view_mark({"pi3_grid_view_mark_depth", far, depth}, state, nx, ny, nz, seen, cells_in, heading_of, V, range,
                   Cones{headings, H, cos2_num, cos2_den}, owner, tag, counters, stream);
}

extern "C" int pi3_grid_view_gain_frustum(const unsigned char* state, int nx, int ny, int nz, const unsigned* seen,
                                          const long* candidates, long V, int range, int depth, int far, const int* frames,
                                          int H, long tan2_h_num, long tan2_h_den, long tan2_v_num, long tan2_v_den,
                                          unsigned* gain, unsigned* visible, int* best, unsigned long long* counters,
                                          void* stream) {
  return view_gain(Form::or_transparent("pi3_grid_view_gain_frustum", far, depth), seen != nullptr, state, nx, ny, nz, seen,
                   candidates, V, range, Frusta{frames, H, tan2_h_num, tan2_h_den, tan2_v_num, tan2_v_den}, gain, visible,
                   best, counters, stream);
}

extern "C" int pi3_grid_view_mark_frustum(const unsigned char* state, int nx, int ny, int nz, unsigned* seen,
                                          const long* cells_in, const int* heading_of, long V, int range, int depth,
                                          int far, const int* frames, int H, long tan2_h_num, long tan2_h_den,
                                          long tan2_v_num, long tan2_v_den, short* owner, int tag,
                                          unsigned long long* counters, void* stream) {
  return view_mark(Form::or_transparent("pi3_grid_view_mark_frustum", far, depth), state, nx, ny, nz, seen, cells_in,
                   heading_of, V, range, Frusta{frames, H, tan2_h_num, tan2_h_den, tan2_v_num, tan2_v_den}, owner, tag,
                   counters, stream);
}
