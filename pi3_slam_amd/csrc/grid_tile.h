// The tile-wise fixed-point sweep over a field of 32-bit words on the occupancy grid (occupancy.hip's layout: [nz][ny][nx],
// x fastest, cell (ix, iy, iz) at the linear index (iz ny + iy) nx + ix), shared by grid_route.hip (costs) and
// grid_frontier.hip (labels).  Nothing here knows what the words mean: the caller brings the step that says which value
// a cell's 26 neighbours allow it.
//
// One sweep: a workgroup of 512 threads per tile of 8 x 8 x 8 cells, a thread per cell.  The tile and its one-cell halo
// are staged in LDS (10^3 entries; the caller names the value of a cell outside the grid), the tile's own cells are
// relaxed in LDS until no thread lowered anything (__syncthreads_or), only own cells that got lower are written back, as
// plain 32-bit stores, and *changed = 1 when any did.  The loop that repeats the launch until a sweep changes nothing
// lives with the caller (ops.sweep_until_quiet).
//
// Why the order of the tiles does not matter: a workgroup reads its halo while the neighbour that owns those cells may
// be writing them, and inside a tile a thread reads its neighbours' LDS words while they write them.  (1) is the
// caller's: every value ever stored is one that the field's meaning admits (a real cost, an index of the component).
// (2) A cell is written only by its own thread of its own workgroup, and only with a smaller value: values only
// decrease.  (3) A 32-bit word cannot tear: a reader sees the old or the new value, both of them admitted by (1).  So
// no value ever drops below the answer, and a state in which a sweep changes nothing satisfies the step's inequality
// between every cell and each of its neighbours, whatever order the tiles ran in and whichever halo values they read.
//
// LDS layout: the 10 x 10 x 10 block is stored with rows 16 entries and planes 168 entries apart (1 680 entries: 6.7 KB
// of words, 1.7 KB of bytes).  ds_read_b32 banks are (a / 4) mod 32 per 32-lane half; a half holds 8 x by 2 y by 2 z
// cells, whose words start at 0, 16, 168 = 8 and 184 = 24 (mod 32): the four rows of 8 tile the 32 banks, and a
// neighbour offset shifts them all alike, so all 26 reads are conflict free.  (Dense rows of 10 put the fourth row of
// any 8 x 4 arrangement on the first row's banks: 2-way on every read.)
#pragma once
#include <hip/hip_runtime.h>

namespace grid_tile {

constexpr long kMaxCells = 1L << 27;    // 21 (2^27 - 1) < 2^32 - 1: a route cost fits, and a label and a cost key share it
constexpr int kMaxIndex = 1 << 21;      // occupancy.hip's limit per dimension
constexpr int kT = 8;                   // tile edge
constexpr int kH = kT + 2;              // with the halo
constexpr int kRow = 16, kPlane = 168;  // LDS strides in entries (see above)
constexpr int kLds = kH * kPlane;
constexpr int kThreads = kT * kT * kT;  // a thread per cell of the tile

inline bool grid_ok(int nx, int ny, int nz, long& cells) {
  if (nx <= 0 || ny <= 0 || nz <= 0 || nx >= kMaxIndex || ny >= kMaxIndex || nz >= kMaxIndex) return false;
  cells = (long)nx * ny;                      // < 2^42
  if (cells > kMaxCells / nz) return false;
  cells *= nz;
  return true;
}

// the tiles along x and y, and the workgroups of one sweep (every tile holds a cell: <= 2^27)
inline unsigned tiles(int nx, int ny, int nz, int& tx, int& ty) {
  tx = (nx + kT - 1) / kT, ty = (ny + kT - 1) / kT;
  return (unsigned)((long)tx * ty * ((nz + kT - 1) / kT));
}

// this workgroup's tile and this thread's cell in it
struct Tile {
  int nx, ny, nz, x0, y0, z0;
  int t;        // the thread
  bool own;     // its cell lies inside the grid
  int g;        // then the cell's linear index, else 0
  int c;        // the cell's LDS index

  __device__ __forceinline__ Tile(int nx_, int ny_, int nz_, int tx, int ty) : nx(nx_), ny(ny_), nz(nz_) {
    t = (int)threadIdx.x;
    int b = (int)blockIdx.x;
    const int bx = b % tx;
    b /= tx;
    const int by = b % ty, bz = b / ty;                       // < the z tiles by the grid's size
    x0 = bx * kT, y0 = by * kT, z0 = bz * kT;
    // a 32-lane half = 8 x by 2 y by 2 z: rows at 0, 16, 168, 184 entries
    const int lx = t & 7, ly = ((t >> 3) & 1) | (((t >> 5) & 3) << 1), lz = ((t >> 4) & 1) | (((t >> 7) & 3) << 1);
    const int gx = x0 + lx, gy = y0 + ly, gz = z0 + lz;
    own = gx < nx && gy < ny && gz < nz;
    g = own ? (gz * ny + gy) * nx + gx : 0;
    c = (lz + 1) * kPlane + (ly + 1) * kRow + (lx + 1);
  }

  // the tile and its halo of `field` into lds[kLds]; a cell outside the grid reads as `outside`
  template <typename T>
  __device__ __forceinline__ void stage(T* lds, const T* field, T outside) const {
    for (int j = t; j < kH * kH * kH; j += kThreads) {
      const int hx = j % kH, hy = (j / kH) % kH, hz = j / (kH * kH);
      const int sx = x0 - 1 + hx, sy = y0 - 1 + hy, sz = z0 - 1 + hz;
      const bool in = sx >= 0 && sx < nx && sy >= 0 && sy < ny && sz >= 0 && sz < nz;
      lds[hz * kPlane + hy * kRow + hx] = in ? field[(sz * ny + sy) * nx + sx] : outside;
    }
  }
};

// f(dx, dy, dz, the neighbour's LDS offset, k) for the 26 neighbours, fully unrolled, in (dz, dy, dx) order: inside the
// grid that is the order of the linear indices, and k = 0 .. 25 numbers them
template <typename F>
__device__ __forceinline__ void for_hood(F f) {
  int k = 0;
#pragma unroll
  for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        if (dx == 0 && dy == 0 && dz == 0) continue;
        f(dx, dy, dz, dz * kPlane + dy * kRow + dx, k);
        ++k;
      }
}

// Relaxes the staged tile to its own fixed point and writes back: best(mine) is the lowest of `mine` and what the
// cell's neighbours in lds allow.  first = this cell's staged value (only this thread ever writes that word); a thread
// whose cell takes no part returns best(mine) = mine.  Every thread of the workgroup calls this, after the barrier that
// publishes the staged words.
template <typename F>
__device__ __forceinline__ void settle(const Tile& tile, unsigned* lds, unsigned* field, unsigned first, int* changed,
                                       F best) {
  unsigned mine = first;
  for (;;) {
    const unsigned b = best(mine);
    const bool lower = b < mine;
    if (lower) {
      mine = b;
      lds[tile.c] = b;
    }
    if (!__syncthreads_or(lower)) break;                      // the barrier also publishes this round's LDS stores
  }
  const bool lowered = mine < first;                          // then the cell takes part, so it lies inside the grid
  if (lowered) field[tile.g] = mine;
  if (__syncthreads_or(lowered) && tile.t == 0) *changed = 1;
}

}  // namespace grid_tile
