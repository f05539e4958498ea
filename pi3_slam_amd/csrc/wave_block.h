// Wave (64 lanes) and workgroup (256 threads = 4 waves) helpers shared by the voxel, cloud and render kernels: the merge
// of runs of equal keys over a wave, the per-workgroup counters and the workgroup's exclusive scan.  Nothing here knows
// a table or an image.
//
// Counters: a count is summed per workgroup in LDS and costs ONE global atomic per workgroup and counter (a per-wave
// atomic on one address once serialised voxel_extract at ~700 k voxels).  block_count and block_sum keep their LDS
// words in function-local __shared__ arrays and end on the threads that read them: a kernel that calls the same one
// twice puts a __syncthreads() between the calls.  Every thread of the workgroup calls them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wave_block {

typedef unsigned long long u64;

// one workgroup's flags -> LDS -> one global atomic per counter: counters[at[i]] += the threads with flag[i]
template <int N>
__device__ __forceinline__ void block_count(const bool (&flag)[N], u64* __restrict__ counters, const int (&at)[N]) {
  __shared__ unsigned tot[N];
  const int tid = (int)threadIdx.x;
  if (tid < N) tot[tid] = 0u;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const u64 b = __ballot(flag[i]);
    if ((tid & 63) == 0 && b) atomicAdd(&tot[i], (unsigned)__popcll(b));
  }
  __syncthreads();
  if (tid < N && tot[tid]) atomicAdd(counters + at[tid], (u64)tot[tid]);
}

// the same for a per-thread integer: *counter += the workgroup's sum of n (wave reduce, LDS, one atomic when non-zero)
__device__ __forceinline__ void block_sum(unsigned n, u64* __restrict__ counter) {
  __shared__ unsigned wave_n[4];
  const int tid = (int)threadIdx.x;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if ((tid & 63) == 0) wave_n[tid >> 6] = n;
  __syncthreads();
  if (tid == 0) {
    const unsigned tot = wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
    if (tot) atomicAdd(counter, (u64)tot);
  }
}

// The workgroup-exclusive prefix of cnt in thread order (the sum over the threads before this one), and in `total` the
// workgroup's sum, the same in every thread: what a kernel needs to hand each thread its rows after ONE atomic per
// workgroup on the row counter (that atomic, by thread 0 and only when total != 0, stays with the caller).  The same
// LDS contract as block_count and block_sum: the per-wave totals are read after the one __syncthreads() inside, so a
// kernel that calls this twice puts a __syncthreads() between the calls.  Every thread of the workgroup calls this.
__device__ __forceinline__ u64 block_exclusive_scan(u64 cnt, u64& total) {
  __shared__ u64 wave_tot[4];
  const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
  u64 incl = cnt;                                  // inclusive prefix over the wave
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const u64 o = __shfl_up(incl, d, 64);
    if (lane >= d) incl += o;
  }
  if (lane == 63) wave_tot[wv] = incl;
  __syncthreads();
  u64 before = incl - cnt;
  for (int w = 0; w < wv; ++w) before += wave_tot[w];
  total = wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
  return before;
}

// Contention scheme of the fusion kernels: a wave's 64 lanes hold 64 consecutive candidates (for the pixel forms: 64
// neighbouring pixels of a row, which at 1-6 m depth and centimetre voxels mostly share voxels).  Runs of consecutive
// lanes with the same key are merged in registers by a segmented inclusive scan over the wave, and only the last lane
// of each run touches memory (one probe + a few 64-bit atomic adds).
//
// Every lane of the wave calls this.  A lane that is not `valid` gets key = no_key, so it ends the run before it and
// joins none of a valid lane's (no_key is a key that no valid lane carries).  v[0..K) becomes the sum over the lanes of
// this lane's run up to and including this lane; the return value says whether this lane is the last of its run, where
// v holds the run's totals.
template <int K>
__device__ __forceinline__ bool wave_merge_runs(bool valid, u64& key, u64 no_key, u64 (&v)[K]) {
  const int lane = (int)(threadIdx.x & 63);
  if (!valid) key = no_key;
  const u64 prev = __shfl_up(key, 1, 64);
  const u64 next = __shfl_down(key, 1, 64);
  const bool head = lane == 0 || prev != key;
  const bool tail = lane == 63 || next != key;
  const u64 heads = __ballot(head);
  const u64 upto = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
  const int seg = 63 - __clzll(heads & upto);          // first lane of this lane's run
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int oseg = __shfl_up(seg, d, 64);
    u64 ov[K];
#pragma unroll
    for (int j = 0; j < K; ++j) ov[j] = __shfl_up(v[j], d, 64);
    if (lane >= d && oseg == seg) {
#pragma unroll
      for (int j = 0; j < K; ++j) v[j] += ov[j];
    }
  }
  return tail;
}

}  // namespace wave_block
