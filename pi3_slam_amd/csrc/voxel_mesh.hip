// A triangle mesh of the fused dense voxel map: an oriented-point signed field (Hoppe '92) on the lattice of the voxel
// table (voxel_table.h), meshed by surface nets.  Reads the table of voxel.hip and the normal sums of
// voxel_normals.hip (nacc), after the keep mask of voxel_clean.hip when one is given; writes nothing into them.
// tests/dense_mesh_ref.py reproduces every output byte for byte.
//
//   source voxel   an occupied slot with keep[slot] != 0 (when a mask is given), W >= 1, cnt > 0 and (Nx, Ny, Nz) != 0;
//                  c = k + U / (W 2^24) per axis in voxel units (voxel_extract_kernel's arithmetic),
//                  n = N / sqrt((Nx Nx + Ny Ny) + Nz Nz),  colour_u = (C + W / 2) / W.
//   cell           a voxel index i; its corners are the lattice points i .. i + 1, and corner g touches the 8 voxels
//                  g - 1 .. g, so a cell sees the 27 voxels i - 1 .. i + 1.  A cell whose biased index field leaves
//                  1 .. 2^21 - 1 does not exist (field_offset), and neither does such a voxel.
//   corner         f(g) = the mean over the source voxels among g - 1 .. g, in x-major order (dx outermost), of
//                  (nx (gx - cx) + ny (gy - cy)) + nz (gz - cz); undefined without one; negative = behind the surface
//                  (the normals face the camera).
//   edge           12 per cell, kEdge below: a crossing when both ends are defined and exactly one is negative, at
//                  t = f_a / (f_a - f_b) from its lower end.
//   vertex         a cell with a crossing: the mean of its crossings in edge order, times the voxel size, as fp32;
//                  normal = the normalised sum of the unit normals of the 27 voxels' sources (0 when they cancel);
//                  colour = (sum colour_u + cnt / 2) / cnt over the same voxels.
//   quad           the cell owns the three edges from its corner 0.  A crossing one, along axis a, gives a quad of the
//                  four cells around it: i - e_b - e_c, i - e_c, i, i - e_b with b = a + 1, c = a + 2 (mod 3), counter-
//                  clockwise seen from +a; `flip` (corner 0 is not negative: the surface faces -a) reverses it.  All four
//                  contain the edge and compute its ends from the same 8 voxels in the same order, so all four have a
//                  vertex; a quad one of whose cells does not exist is not emitted.  Row: owner key, axis | flip << 2.
//
// All arithmetic is f64 (and integers), every operation rounded on its own in the order written; f64 add, multiply,
// divide and sqrt are correctly rounded on the device.  The Makefile compiles this file with -ffp-contract=off.
//
// Kernels.  The cell table is a second hash table, caller-owned: `cells`, one u64 key per slot (all ones = empty,
// linear probing from mix64(key) & mask, 64-bit CAS claim, capacity a power of two), and `verts`, 8 x uint32 per slot.
//   mesh_cells      one thread per voxel slot: a source voxel inserts the keys of its 27 surrounding cells (only those
//                   can hold a vertex).  An insert that finds no slot within min(cell_capacity, kMaxProbe) probes is
//                   COUNTED, nothing is written for it (dense_map.MapMesher grows the table or raises).  The probe
//                   bound keeps a table that is far too small cheap: without it every insert into a full table would
//                   walk all of it.  Nothing looks a cell up later, so a bounded insert loses nothing: a key is found
//                   again on the same chain, at the probe where it was claimed.  cells = null: count sources only.
//   mesh_vertices   one thread per cell slot: 27 slot_find gathers into the table and nacc, the 8 corner sums in
//                   registers, then the masks, the vertex and the owned quads -> verts[slot] = x y z nx ny nz (fp32
//                   bits), rgb | flags << 24 (bit 0 vertex, bits 1-3 quad on axis 0-2, bit 4 flip), spare.
//   mesh_extract    cell slots -> vertex rows (key, xyz, normal, rgb) and quad rows; a workgroup covers
//                   256 x kExtractPer slots and claims its rows with one atomicAdd per counter (claim_rows' pattern:
//                   one block_exclusive_scan of both counts packed in a u64).  Row order is arbitrary: the host sorts.
// No atomics but the slot claim and the counters: everything else is a gather in a fixed order, so the rows do not
// depend on scheduling.  Every probe loop is bounded by its table's capacity and every store by its buffer's rows.
//
// stats (caller-owned DEVICE uint64 [12]; each entry point zeroes its own): mesh_cells [0] source voxels, [1] cells
// inserted, [2] inserts without a slot; mesh_vertices [3] vertices, [4] quads, [5] ambiguous faces (the cell faces
// through corner 0 whose four edges all cross: a non-manifold edge); mesh_extract [6] vertex rows, [7] quad rows,
// [8] vertex rows that did not fit, [9] quad rows that did not fit.
#include "common.h"
#include "voxel_table.h"
#include "wave_block.h"

#include <stdint.h>

namespace {

using namespace voxel_table;      // u64, kEmpty, kBias, pack_key, key_field, field_offset, for_each_neighbour, slot_claim,
                                  // slot_find, slot_centre, slot_colour, kExtractPer, pow2, blocks_for
using wave_block::block_exclusive_scan;
using wave_block::block_sum;

typedef long long i64;

constexpr uint32_t kVertex = 1u << 24, kQuad0 = 1u << 25, kFlip = 1u << 28;
constexpr u64 kMaxProbe = 256;         // a table at most half full has chains far shorter (mix64 spreads the keys)

// whether the occupied slot t holds a source voxel (keep = null: no mask)
__device__ __forceinline__ bool is_source(const u64* __restrict__ table, const i64* __restrict__ nacc,
                                          const unsigned char* __restrict__ keep, long t) {
  const i64* q = nacc + 4 * t;
  return (!keep || keep[t]) && table[8 * t + 1] >= 1ull && q[3] > 0 && (q[0] != 0 || q[1] != 0 || q[2] != 0);
}

// the slot of the voxel `key` when it is a source voxel, else -1
__device__ __forceinline__ long source_slot(const u64* __restrict__ table, u64 mask, const i64* __restrict__ nacc,
                                            const unsigned char* __restrict__ keep, u64 key) {
  const long t = slot_find(table, mask, key);
  return t >= 0 && is_source(table, nacc, keep, t) ? t : -1;
}

// claim the slot of `key` in the cell table: 1 = newly claimed, 0 = already there, -1 = no slot within the probe bound
__device__ __forceinline__ int cell_insert(u64* __restrict__ cells, u64 cmask, u64 key) {
  bool fresh;
  const long h = slot_claim<1>(cells, cmask, cmask < kMaxProbe ? cmask : kMaxProbe - 1, key, fresh);
  return h < 0 ? -1 : (int)fresh;
}

template <bool kMasked>
__global__ __launch_bounds__(256) void mesh_cells_kernel(const u64* __restrict__ table, long capacity,
                                                         const i64* __restrict__ nacc,
                                                         const unsigned char* __restrict__ keep, u64* __restrict__ cells,
                                                         u64 cmask, u64* __restrict__ stats) {
  const long s = (long)blockIdx.x * 256 + threadIdx.x;
  unsigned sources = 0, claimed = 0, lost = 0;
  if (s < capacity) {
    const u64 key = table[8 * s];
    if (key != kEmpty && is_source(table, nacc, kMasked ? keep : nullptr, s)) {
      sources = 1;
      if (cells) {
        for_each_neighbour<1, true>(key_field(key, 0), key_field(key, 1), key_field(key, 2),
                                    [&](int, int, int, u64 cell) __attribute__((always_inline)) {
          const int r = cell_insert(cells, cmask, cell);
          claimed += r > 0;
          lost += r < 0;
        });
      }
    }
  }
  block_sum(sources, stats + 0);
  __syncthreads();                              // block_sum's LDS words are read by thread 0 until here
  block_sum(claimed, stats + 1);
  __syncthreads();
  block_sum(lost, stats + 2);
}

// kEdge: the 12 edges of a cell as corner indices (4 a + 2 b + c): axis 0's four, axis 1's, axis 2's; lower end first

template <bool kMasked>
__global__ __launch_bounds__(256) void mesh_vertices_kernel(const u64* __restrict__ table, long capacity,
                                                            const i64* __restrict__ nacc,
                                                            const unsigned char* __restrict__ keep_or_null,
                                                            const u64* __restrict__ cells, long cell_capacity,
                                                            double vsize, uint32_t* __restrict__ verts,
                                                            u64* __restrict__ stats) {
#pragma clang fp contract(off)
  const long s = (long)blockIdx.x * 256 + threadIdx.x;
  const u64 mask = (u64)capacity - 1;
  const unsigned char* keep = kMasked ? keep_or_null : nullptr;
  unsigned has_vertex = 0, quads = 0, ambiguous = 0;
  const u64 key = s < cell_capacity ? cells[s] : kEmpty;
  if (key != kEmpty) {
    const uint32_t bi[3] = {key_field(key, 0), key_field(key, 1), key_field(key, 2)};
    const double i0[3] = {(double)((int)bi[0] - kBias), (double)((int)bi[1] - kBias), (double)((int)bi[2] - kBias)};
    double f[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int cn[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    double ns[3] = {0.0, 0.0, 0.0};
    u64 cs[3] = {0, 0, 0};
    int n27 = 0;
    // for_each_neighbour's walk (x-major: its order is the order of the sums), written out because it must be fully
    // unrolled here: dx, dy and dz are then constants and the corner tests below fold away.  Through the shared walk,
    // which the other kernels want rolled, this kernel took 17 more VGPRs and 7 % more time (430 k voxels, MI355X).
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      uint32_t vx, vy, vz;
      const bool okx = field_offset(bi[0], dx, vx);
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy) {
        const bool oky = field_offset(bi[1], dy, vy);
#pragma unroll
        for (int dz = -1; dz <= 1; ++dz) {
          if (!(okx && oky && field_offset(bi[2], dz, vz))) continue;
          const long t = source_slot(table, mask, nacc, keep, pack_key(vx, vy, vz));
          if (t < 0) continue;
          const u64* q = table + 8 * t;
          const i64* nq = nacc + 4 * t;
          const double c[3] = {slot_centre(q, 0), slot_centre(q, 1), slot_centre(q, 2)};
          const double d[3] = {(double)nq[0], (double)nq[1], (double)nq[2]};
          const double len = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
          const double u[3] = {d[0] / len, d[1] / len, d[2] / len};
#pragma unroll
          for (int a = 0; a < 2; ++a) {
            if (dx < a - 1 || dx > a) continue;
#pragma unroll
            for (int b = 0; b < 2; ++b) {
              if (dy < b - 1 || dy > b) continue;
#pragma unroll
              for (int e = 0; e < 2; ++e) {
                if (dz < e - 1 || dz > e) continue;
                const double gx = i0[0] + (double)a, gy = i0[1] + (double)b, gz = i0[2] + (double)e;
                const double term = (u[0] * (gx - c[0]) + u[1] * (gy - c[1])) + u[2] * (gz - c[2]);
                f[4 * a + 2 * b + e] = f[4 * a + 2 * b + e] + term;
                ++cn[4 * a + 2 * b + e];
              }
            }
          }
#pragma unroll
          for (int a = 0; a < 3; ++a) {
            ns[a] = ns[a] + u[a];
            cs[a] += slot_colour(q, a);
          }
          ++n27;
        }
      }
    }
    unsigned defined = 0, neg = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (cn[i] > 0) {
        f[i] = f[i] / (double)cn[i];
        defined |= 1u << i;
        if (f[i] < 0.0) neg |= 1u << i;
      }
    }
    constexpr int kEdgeLo[12] = {0, 1, 2, 3, 0, 1, 4, 5, 0, 2, 4, 6};
    constexpr int kEdgeHi[12] = {4, 5, 6, 7, 2, 3, 6, 7, 1, 3, 5, 7};
    double ps[3] = {0.0, 0.0, 0.0};
    int ncross = 0;
    unsigned crossing = 0;
#pragma unroll
    for (int e = 0; e < 12; ++e) {
      const int lo = kEdgeLo[e], hi = kEdgeHi[e], axis = e >> 2;
      if (!((defined >> lo) & (defined >> hi) & 1u) || !(((neg >> lo) ^ (neg >> hi)) & 1u)) continue;
      crossing |= 1u << e;
      const double t = f[lo] / (f[lo] - f[hi]);
      double p[3] = {i0[0] + (double)(lo >> 2), i0[1] + (double)((lo >> 1) & 1), i0[2] + (double)(lo & 1)};
      p[axis] = p[axis] + t;
      ps[0] = ps[0] + p[0];
      ps[1] = ps[1] + p[1];
      ps[2] = ps[2] + p[2];
      ++ncross;
    }
    uint32_t out[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (ncross > 0) {
      has_vertex = 1;
      const double l2 = (ns[0] * ns[0] + ns[1] * ns[1]) + ns[2] * ns[2];
      const double len = l2 > 0.0 ? sqrt(l2) : 1.0;
      uint32_t word = kVertex;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        out[a] = __float_as_uint((float)(vsize * (ps[a] / (double)ncross)));
        out[3 + a] = __float_as_uint(l2 > 0.0 ? (float)(ns[a] / len) : 0.0f);
        word |= (uint32_t)((cs[a] + (u64)(n27 / 2)) / (u64)n27) << (8 * a);
      }
      // the owned edges: kEdge 0, 4, 8 run from corner 0 along axis 0, 1, 2
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        uint32_t other;
        if ((crossing >> (4 * a) & 1u) && field_offset(bi[(a + 1) % 3], -1, other) &&
            field_offset(bi[(a + 2) % 3], -1, other)) {
          word |= kQuad0 << a;
          ++quads;
        }
      }
      if (!(neg & 1u)) word |= kFlip;
      out[6] = word;
    }
    // the faces through corner 0, perpendicular to axis 0, 1, 2: corners in a ring
    constexpr int ring[3][4] = {{0, 2, 3, 1}, {0, 4, 5, 1}, {0, 4, 6, 2}};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const unsigned all = (1u << ring[a][0]) | (1u << ring[a][1]) | (1u << ring[a][2]) | (1u << ring[a][3]);
      const unsigned n0 = neg >> ring[a][0] & 1u, n1 = neg >> ring[a][1] & 1u, n2 = neg >> ring[a][2] & 1u,
                     n3 = neg >> ring[a][3] & 1u;
      if ((defined & all) == all && n0 == n2 && n1 == n3 && n0 != n1) ++ambiguous;
    }
    uint4* dst = reinterpret_cast<uint4*>(verts + 8 * s);
    dst[0] = make_uint4(out[0], out[1], out[2], out[3]);
    dst[1] = make_uint4(out[4], out[5], out[6], out[7]);
  }
  block_sum(has_vertex, stats + 3);
  __syncthreads();
  block_sum(quads, stats + 4);
  __syncthreads();
  block_sum(ambiguous, stats + 5);
}

__global__ __launch_bounds__(256) void mesh_extract_kernel(const u64* __restrict__ cells, long cell_capacity,
                                                           const uint32_t* __restrict__ verts, u64* __restrict__ vkeys,
                                                           float* __restrict__ vxyz, float* __restrict__ vnrm,
                                                           unsigned char* __restrict__ vrgb, long max_vertices,
                                                           u64* __restrict__ qkeys, int* __restrict__ qcodes,
                                                           long max_quads, u64* __restrict__ stats) {
  __shared__ u64 base_v, base_q;
  const int tid = (int)threadIdx.x;
  const long s0 = (long)blockIdx.x * (256L * kExtractPer) + tid;
  // this thread's rows: vertices in the low half, quads in the high half (a workgroup has at most 4096 and 12288)
  uint32_t occ = 0;
  u64 cnt = 0;
#pragma unroll
  for (int j = 0; j < kExtractPer; ++j) {
    const long s = s0 + 256L * j;
    if (s < cell_capacity && cells[s] != kEmpty) {
      const uint32_t w = verts[8 * s + 6];
      if (w & kVertex) {
        occ |= 1u << j;
        cnt += 1ull + ((u64)__popc(w >> 25 & 7u) << 32);
      }
    }
  }
  u64 tot;
  const u64 excl = block_exclusive_scan(cnt, tot);
  if (tid == 0) {
    const u64 tv = tot & 0xFFFFFFFFull, tq = tot >> 32;
    base_v = tv ? atomicAdd(stats + 6, tv) : 0ull;
    base_q = tq ? atomicAdd(stats + 7, tq) : 0ull;
  }
  __syncthreads();
  u64 at_v = base_v + (excl & 0xFFFFFFFFull), at_q = base_q + (excl >> 32);
  unsigned unstored_v = 0, unstored_q = 0;
#pragma unroll 1
  for (int j = 0; j < kExtractPer; ++j) {
    if (!(occ >> j & 1u)) continue;
    const long s = s0 + 256L * j;
    const uint4 lo = reinterpret_cast<const uint4*>(verts + 8 * s)[0];
    const uint4 hi = reinterpret_cast<const uint4*>(verts + 8 * s)[1];
    const u64 key = cells[s];
    if ((long)at_v < max_vertices) {
      vkeys[at_v] = key;
      vxyz[3 * at_v] = __uint_as_float(lo.x);
      vxyz[3 * at_v + 1] = __uint_as_float(lo.y);
      vxyz[3 * at_v + 2] = __uint_as_float(lo.z);
      vnrm[3 * at_v] = __uint_as_float(lo.w);
      vnrm[3 * at_v + 1] = __uint_as_float(hi.x);
      vnrm[3 * at_v + 2] = __uint_as_float(hi.y);
      vrgb[3 * at_v] = (unsigned char)(hi.z & 0xFFu);
      vrgb[3 * at_v + 1] = (unsigned char)(hi.z >> 8 & 0xFFu);
      vrgb[3 * at_v + 2] = (unsigned char)(hi.z >> 16 & 0xFFu);
    } else {
      ++unstored_v;
    }
    ++at_v;
    const int flip = (hi.z & kFlip) ? 4 : 0;
    for (int a = 0; a < 3; ++a) {
      if (!(hi.z & (kQuad0 << a))) continue;
      if ((long)at_q < max_quads) {
        qkeys[at_q] = key;
        qcodes[at_q] = a | flip;
      } else {
        ++unstored_q;
      }
      ++at_q;
    }
  }
  block_sum(unstored_v, stats + 8);
  __syncthreads();
  block_sum(unstored_q, stats + 9);
}

}  // namespace

extern "C" int pi3_voxel_mesh_cells(const void* table, long capacity, const long long* nacc,
                                    const unsigned char* keep_or_null, unsigned long long* cells_or_null,
                                    long cell_capacity, unsigned long long* stats, void* stream) {
  if (!table || !pow2(capacity) || !nacc || !stats || (cells_or_null && !pow2(cell_capacity))) {
    pi3_set_error("pi3_voxel_mesh_cells: bad arguments capacity=%ld cell_capacity=%ld", capacity, cell_capacity);
    return PI3_ERR_ARG;
  }
  if (pi3_zero_words("pi3_voxel_mesh_cells", stats, 3, stream) != PI3_OK) return PI3_ERR_LAUNCH;
  if (cells_or_null && hipMemsetAsync(cells_or_null, 0xFF, (size_t)cell_capacity * sizeof(unsigned long long),
                                      (hipStream_t)stream) != hipSuccess) {
    pi3_set_error("pi3_voxel_mesh_cells: hipMemsetAsync failed");
    return PI3_ERR_LAUNCH;
  }
  const u64 cmask = cells_or_null ? (u64)(cell_capacity - 1) : 0ull;
  if (keep_or_null)
    hipLaunchKernelGGL(mesh_cells_kernel<true>, dim3(blocks_for(capacity)), dim3(256), 0, (hipStream_t)stream,
                       (const u64*)table, capacity, (const i64*)nacc, keep_or_null, (u64*)cells_or_null, cmask,
                       (u64*)stats);
  else
    hipLaunchKernelGGL(mesh_cells_kernel<false>, dim3(blocks_for(capacity)), dim3(256), 0, (hipStream_t)stream,
                       (const u64*)table, capacity, (const i64*)nacc, keep_or_null, (u64*)cells_or_null, cmask,
                       (u64*)stats);
  return pi3_check_launch("voxel_mesh_cells");
}

extern "C" int pi3_voxel_mesh_vertices(const void* table, long capacity, const long long* nacc,
                                       const unsigned char* keep_or_null, const unsigned long long* cells,
                                       long cell_capacity, double voxel_size, unsigned* verts,
                                       unsigned long long* stats, void* stream) {
  if (!table || !pow2(capacity) || !nacc || !cells || !pow2(cell_capacity) || !verts || !stats ||
      !positive_finite(voxel_size)) {
    pi3_set_error("pi3_voxel_mesh_vertices: bad arguments capacity=%ld cell_capacity=%ld voxel_size=%g", capacity,
                  cell_capacity, voxel_size);
    return PI3_ERR_ARG;
  }
  if (pi3_zero_words("pi3_voxel_mesh_vertices", stats + 3, 3, stream) != PI3_OK) return PI3_ERR_LAUNCH;
  if (keep_or_null)
    hipLaunchKernelGGL(mesh_vertices_kernel<true>, dim3(blocks_for(cell_capacity)), dim3(256), 0, (hipStream_t)stream,
                       (const u64*)table, capacity, (const i64*)nacc, keep_or_null, (const u64*)cells, cell_capacity,
                       voxel_size, verts, (u64*)stats);
  else
    hipLaunchKernelGGL(mesh_vertices_kernel<false>, dim3(blocks_for(cell_capacity)), dim3(256), 0, (hipStream_t)stream,
                       (const u64*)table, capacity, (const i64*)nacc, keep_or_null, (const u64*)cells, cell_capacity,
                       voxel_size, verts, (u64*)stats);
  return pi3_check_launch("voxel_mesh_vertices");
}

extern "C" int pi3_voxel_mesh_extract(const unsigned long long* cells, long cell_capacity, const unsigned* verts,
                                      unsigned long long* vkeys, float* vxyz, float* vnrm, unsigned char* vrgb,
                                      long max_vertices, unsigned long long* qkeys, int* qcodes, long max_quads,
                                      unsigned long long* stats, void* stream) {
  if (!cells || !pow2(cell_capacity) || !verts || !stats || max_vertices < 0 || max_quads < 0 ||
      (max_vertices > 0 && (!vkeys || !vxyz || !vnrm || !vrgb)) || (max_quads > 0 && (!qkeys || !qcodes))) {
    pi3_set_error("pi3_voxel_mesh_extract: bad arguments cell_capacity=%ld max_vertices=%ld max_quads=%ld",
                  cell_capacity, max_vertices, max_quads);
    return PI3_ERR_ARG;
  }
  if (pi3_zero_words("pi3_voxel_mesh_extract", stats + 6, 4, stream) != PI3_OK) return PI3_ERR_LAUNCH;
  const long span = 256L * kExtractPer;
  hipLaunchKernelGGL(mesh_extract_kernel, dim3((unsigned)((cell_capacity + span - 1) / span)), dim3(256), 0,
                     (hipStream_t)stream, (const u64*)cells, cell_capacity, verts, (u64*)vkeys, vxyz, vnrm, vrgb,
                     max_vertices, (u64*)qkeys, qcodes, max_quads, (u64*)stats);
  return pi3_check_launch("voxel_mesh_extract");
}
