// Cleaning the fused dense map: a keep / drop decision per voxel of the world-frame hash table (voxel_table.h), taken
// on the device after every chunk cloud is fused and before the extraction.  No new geometry, integer arithmetic only:
// tests/dense_clean_ref.py reproduces every array byte for byte.
//
//   eligible     an occupied slot whose full 64-bit weight W >= min_weight;
//   support(v)   the number of eligible voxels u != v with max(|dx|, |dy|, |dz|) <= R in voxel indices, R = 1 or 2
//                (26 or 124 candidate cells).  A cell whose index on any axis leaves |k| < 2^20 does not exist: the
//                biased 21-bit field is tested before a key is composed, so +1 never carries into the next field;
//   stage A      survivors = eligible voxels with support >= min_support;
//   stage B      26-connected components of the survivors; label = the component's smallest key, size = its voxel
//                count; kept = survivors whose component has size >= min_component.
// One pass of each stage, in this order: stage A is not repeated on what stage B leaves.
//
// Kernels: one thread per slot, 256-thread workgroups; a slot that holds no voxel of the stage at hand leaves at once.
// The table is read only; every lookup goes through slot_find, which is bounded by the capacity, and every other loop
// in this file has a constant bound.
//
// Labelling.  label[slot] (u64) starts as the slot's own key for a survivor and as all ones elsewhere.  A sweep gives
// every survivor m = min(its label, the labels of its 26 neighbours) (an all-ones label never wins a minimum, so the
// labels alone tell who survives), shortens the chain m <- label[slot_find(m)] a bounded number of hops, and, when m is
// smaller than the slot's label L, atomicMins m into label[slot] and into label[slot_find(L)] (the slot's previous
// root) and raises the sweep's `changed` word.
// Invariant: a label is always the key of a survivor of the same component, and labels only decrease.  (Initially the
// own key; a sweep only ever copies a label of the same component - a neighbour's, or the label of the voxel a label
// names - into a slot of that component, through atomicMin.)  Hence, whatever order the atomics land in and however
// stale a relaxed load inside a launch is: a sweep that changes nothing has label[v] <= label[u] for every pair of
// neighbours, so the label is constant on a component; the voxel with the component's smallest key can only carry that
// key (its label is a key of the component and <= its own); so the only fixed point is "every voxel carries its
// component's smallest key".  A sweep reads at least what the previous launch wrote, so plain neighbour propagation
// alone ends within (survivors) sweeps: the host loop's bound.  The host (dense_map.MapCleaner) runs a few sweeps, reads
// their `changed` words, and stops at the first sweep that changed nothing.
//
// Sizes are uint32 atomic counts at the root's slot, so two runs give the same bytes.  Counters (caller-owned device
// memory, 8 x uint64, zeroed by pi3_voxel_support): [0] occupied slots, [1] eligible, [2] after support, [3] after
// components, [4] components found, [5] components kept, [6] (pi3_voxel_support_excluding) the occupied slots its exclude
// mask names.  Every counter is summed per workgroup (wave_block.h, block_count).
//
// Excluded slots (pi3_voxel_support_excluding; the carved voxels of voxel_carve.hip): exclude[slot] != 0 makes an occupied
// slot not eligible and nobody's neighbour, so stage A counts its support without them, and stage B, which starts from
// stage A's mask, its components.  The same kernel with a template flag.
#include "common.h"
#include "voxel_table.h"
#include "wave_block.h"

#include <stdint.h>

namespace {

using namespace voxel_table;
using wave_block::block_count;

constexpr int kHops = 8;              // chain-shortening hops per sweep and slot

__device__ __forceinline__ u64 load_relaxed(const u64* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Stage A.  kRadius = 1 or 2.  probe = false (min_support == 0 and nobody asks for the counts): eligibility only.
// kExcl: the slots that `exclude` names are neither eligible nor counted as anybody's neighbour.
template <int kRadius, bool kExcl>
__global__ __launch_bounds__(256) void voxel_support_kernel(const u64* __restrict__ table, long capacity, u64 min_weight,
                                                            int min_support, bool probe,
                                                            const unsigned char* __restrict__ exclude,
                                                            unsigned char* __restrict__ keep, int* __restrict__ support,
                                                            u64* __restrict__ counters) {
  const long s = (long)blockIdx.x * 256 + threadIdx.x;
  const u64 mask = (u64)capacity - 1;
  bool occupied = false, eligible = false, kept = false, excluded = false;
  if (s < capacity) {
    const u64 key = table[8 * s];
    occupied = key != kEmpty;
    if (kExcl) excluded = occupied && exclude[s];
    eligible = occupied && !excluded && table[8 * s + 1] >= min_weight;
    int n = -1;
    if (eligible && probe) {
      n = 0;
      for_each_neighbour<kRadius, false>(key_field(key, 0), key_field(key, 1), key_field(key, 2),
                                         [&](int, int, int, u64 other) __attribute__((always_inline)) {
        const long t = slot_find(table, mask, other);
        if (t >= 0 && table[8 * t + 1] >= min_weight && (!kExcl || !exclude[t])) ++n;
      });
    }
    kept = eligible && (!probe || n >= min_support);
    keep[s] = kept ? 1 : 0;
    if (support) support[s] = n;
  }
  if constexpr (kExcl) {
    const bool flags[4] = {occupied, eligible, kept, excluded};
    const int at[4] = {0, 1, 2, 6};
    block_count<4>(flags, counters, at);
  } else {
    const bool flags[3] = {occupied, eligible, kept};
    const int at[3] = {0, 1, 2};
    block_count<3>(flags, counters, at);
  }
}

__global__ __launch_bounds__(256) void voxel_label_init_kernel(const u64* __restrict__ table, long capacity,
                                                               const unsigned char* __restrict__ keep,
                                                               u64* __restrict__ label) {
  const long s = (long)blockIdx.x * 256 + threadIdx.x;
  if (s >= capacity) return;
  const u64 key = table[8 * s];
  label[s] = (key != kEmpty && keep[s]) ? key : kEmpty;
}

__global__ __launch_bounds__(256) void voxel_label_sweep_kernel(const u64* __restrict__ table, long capacity,
                                                                u64* label, int* changed) {
  const long s = (long)blockIdx.x * 256 + threadIdx.x;
  const u64 mask = (u64)capacity - 1;
  bool lowered = false;
  const u64 own = s < capacity ? load_relaxed(label + s) : kEmpty;
  if (own != kEmpty) {                                   // a survivor (empty and dropped slots carry all ones)
    const u64 key = table[8 * s];
    u64 m = own;
    for_each_neighbour<1, false>(key_field(key, 0), key_field(key, 1), key_field(key, 2),
                                 [&](int, int, int, u64 other) __attribute__((always_inline)) {
      const long t = slot_find(table, mask, other);
      if (t < 0) return;
      const u64 l = load_relaxed(label + t);
      m = l < m ? l : m;
    });
    for (int hop = 0; hop < kHops; ++hop) {              // m names a voxel of this component: follow its label
      const long r = slot_find(table, mask, m);
      if (r < 0) break;
      const u64 l = load_relaxed(label + r);
      if (l >= m) break;                                 // l == m: a root
      m = l;
    }
    if (m < own) {
      atomicMin(label + s, m);
      if (own != key) {
        const long r0 = slot_find(table, mask, own);     // the previous root hooks on as well
        if (r0 >= 0) atomicMin(label + r0, m);
      }
      lowered = true;
    }
  }
  const u64 any = __ballot(lowered);
  if (any && (int)(threadIdx.x & 63) == __ffsll((long long)any) - 1) atomicExch(changed, 1);
}

// size[root slot] += 1 for every survivor.  The lanes of a wave that share a label add once (a large component would
// otherwise put 64 atomics per wave on one address); the label most lanes are likely to share, the wave's first, is
// merged over the workgroup's four waves in LDS first.
__global__ __launch_bounds__(256) void voxel_component_sizes_kernel(const u64* __restrict__ table, long capacity,
                                                                    const u64* __restrict__ label,
                                                                    unsigned* __restrict__ size) {
  __shared__ u64 first_label[4];
  __shared__ unsigned first_count[4];
  const long s = (long)blockIdx.x * 256 + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6);
  const u64 mask = (u64)capacity - 1;
  const u64 mine = s < capacity ? label[s] : kEmpty;
  u64 todo = __ballot(mine != kEmpty);
  {                                                       // round 0: the wave's first label, through LDS
    u64 l = kEmpty;
    unsigned n = 0;
    if (todo) {
      l = __shfl(mine, __ffsll((long long)todo) - 1, 64);
      const u64 same = __ballot(mine == l);
      n = (unsigned)__popcll(same);
      todo &= ~same;
    }
    if (lane == 0) {
      first_label[wv] = l;
      first_count[wv] = n;
    }
  }
  __syncthreads();
  if (threadIdx.x < 4 && first_label[threadIdx.x] != kEmpty) {
    const int w = (int)threadIdx.x;
    bool leader = true;                                   // the first wave that holds this label adds for all four
    unsigned n = 0;
    for (int o = 0; o < 4; ++o) {
      if (first_label[o] != first_label[w]) continue;
      if (o < w) leader = false;
      n += first_count[o];
    }
    if (leader) {
      const long r = slot_find(table, mask, first_label[w]);
      if (r >= 0) atomicAdd(size + r, n);
    }
  }
  for (int round = 0; round < 64 && todo; ++round) {      // the wave's other labels: at most 63 of them
    const u64 l = __shfl(mine, __ffsll((long long)todo) - 1, 64);
    const u64 same = __ballot(mine == l) & todo;
    if (lane == __ffsll((long long)same) - 1) {
      const long r = slot_find(table, mask, l);
      if (r >= 0) atomicAdd(size + r, (unsigned)__popcll(same));
    }
    todo &= ~same;
  }
}

// Stage B's decision: keep[slot] &= size[root] >= min_component; counts the survivors kept, the roots and the roots kept.
__global__ __launch_bounds__(256) void voxel_component_filter_kernel(const u64* __restrict__ table, long capacity,
                                                                     const u64* __restrict__ label,
                                                                     const unsigned* __restrict__ size,
                                                                     unsigned min_component,
                                                                     unsigned char* __restrict__ keep,
                                                                     u64* __restrict__ counters) {
  const long s = (long)blockIdx.x * 256 + threadIdx.x;
  const u64 mask = (u64)capacity - 1;
  bool kept = false, root = false, root_kept = false;
  const u64 l = s < capacity ? label[s] : kEmpty;
  if (l != kEmpty) {
    const long r = slot_find(table, mask, l);
    kept = r >= 0 && size[r] >= min_component;
    root = r == s;
    root_kept = root && kept;
    if (!kept) keep[s] = 0;
  }
  const bool flags[3] = {kept, root, root_kept};
  const int at[3] = {3, 4, 5};
  block_count<3>(flags, counters, at);
}

}  // namespace

namespace {

template <bool kExcl>
int support_launch(const char* what, const void* table, long capacity, unsigned long long min_weight, int radius,
                   int min_support, const unsigned char* exclude, unsigned char* keep, int* support,
                   unsigned long long* counters, void* stream) {
  const int cells = (2 * radius + 1) * (2 * radius + 1) * (2 * radius + 1) - 1;
  if (!table || !pow2(capacity) || !keep || !counters || (kExcl && !exclude) || (radius != 1 && radius != 2) ||
      min_support < 0 || min_support > cells) {
    pi3_set_error("%s: bad arguments capacity=%ld radius=%d min_support=%d", what, capacity, radius, min_support);
    return PI3_ERR_ARG;
  }
  if (pi3_zero_words(what, counters, 8, stream) != PI3_OK) return PI3_ERR_LAUNCH;
  const bool probe = min_support > 0 || support != nullptr;
  if (radius == 1)
    hipLaunchKernelGGL((voxel_support_kernel<1, kExcl>), dim3(blocks_for(capacity)), dim3(256), 0, (hipStream_t)stream,
                       (const u64*)table, capacity, (u64)min_weight, min_support, probe, exclude, keep, support,
                       (u64*)counters);
  else
    hipLaunchKernelGGL((voxel_support_kernel<2, kExcl>), dim3(blocks_for(capacity)), dim3(256), 0, (hipStream_t)stream,
                       (const u64*)table, capacity, (u64)min_weight, min_support, probe, exclude, keep, support,
                       (u64*)counters);
  return pi3_check_launch(what + 4);       // without the "pi3_" prefix, as the other entry points report
}

}  // namespace

extern "C" int pi3_voxel_support(const void* table, long capacity, unsigned long long min_weight, int radius,
                                 int min_support, unsigned char* keep, int* support, unsigned long long* counters,
                                 void* stream) {
  return support_launch<false>("pi3_voxel_support", table, capacity, min_weight, radius, min_support, nullptr, keep,
                               support, counters, stream);
}

extern "C" int pi3_voxel_support_excluding(const void* table, long capacity, unsigned long long min_weight, int radius,
                                           int min_support, unsigned char* keep, int* support,
                                           unsigned long long* counters, const unsigned char* exclude, void* stream) {
  return support_launch<true>("pi3_voxel_support_excluding", table, capacity, min_weight, radius, min_support, exclude,
                              keep, support, counters, stream);
}

extern "C" int pi3_voxel_label_init(const void* table, long capacity, const unsigned char* keep,
                                    unsigned long long* label, void* stream) {
  if (!table || !pow2(capacity) || !keep || !label) {
    pi3_set_error("pi3_voxel_label_init: bad arguments capacity=%ld", capacity);
    return PI3_ERR_ARG;
  }
  hipLaunchKernelGGL(voxel_label_init_kernel, dim3(blocks_for(capacity)), dim3(256), 0, (hipStream_t)stream,
                     (const u64*)table, capacity, keep, (u64*)label);
  return pi3_check_launch("voxel_label_init");
}

extern "C" int pi3_voxel_label_sweep(const void* table, long capacity, unsigned long long* label, int* changed,
                                     void* stream) {
  if (!table || !pow2(capacity) || !label || !changed) {
    pi3_set_error("pi3_voxel_label_sweep: bad arguments capacity=%ld", capacity);
    return PI3_ERR_ARG;
  }
  hipLaunchKernelGGL(voxel_label_sweep_kernel, dim3(blocks_for(capacity)), dim3(256), 0, (hipStream_t)stream,
                     (const u64*)table, capacity, (u64*)label, changed);
  return pi3_check_launch("voxel_label_sweep");
}

extern "C" int pi3_voxel_component_sizes(const void* table, long capacity, const unsigned long long* label,
                                         unsigned* size, void* stream) {
  if (!table || !pow2(capacity) || !label || !size) {
    pi3_set_error("pi3_voxel_component_sizes: bad arguments capacity=%ld", capacity);
    return PI3_ERR_ARG;
  }
  if (hipMemsetAsync(size, 0, (size_t)capacity * sizeof(unsigned), (hipStream_t)stream) != hipSuccess) {
    pi3_set_error("pi3_voxel_component_sizes: hipMemsetAsync failed");
    return PI3_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(voxel_component_sizes_kernel, dim3(blocks_for(capacity)), dim3(256), 0, (hipStream_t)stream,
                     (const u64*)table, capacity, (const u64*)label, size);
  return pi3_check_launch("voxel_component_sizes");
}

extern "C" int pi3_voxel_component_filter(const void* table, long capacity, const unsigned long long* label,
                                          const unsigned* size, long min_component, unsigned char* keep,
                                          unsigned long long* counters, void* stream) {
  if (!table || !pow2(capacity) || !label || !size || !keep || !counters || min_component < 0 ||
      min_component > 0xFFFFFFFFl) {
    pi3_set_error("pi3_voxel_component_filter: bad arguments capacity=%ld min_component=%ld", capacity, min_component);
    return PI3_ERR_ARG;
  }
  if (pi3_zero_words("pi3_voxel_component_filter", counters + 3, 3, stream) != PI3_OK) return PI3_ERR_LAUNCH;
  hipLaunchKernelGGL(voxel_component_filter_kernel, dim3(blocks_for(capacity)), dim3(256), 0, (hipStream_t)stream,
                     (const u64*)table, capacity, (const u64*)label, size, (unsigned)min_component, keep,
                     (u64*)counters);
  return pi3_check_launch("voxel_component_filter");
}
