// The launches the union-find labellers share: cc_kernels.hip (affinity graphs) and label_cc_kernels.hip (id volumes) both leave a
// parent array in the form cc_core.h describes and then flatten, rank, scan and number it with the kernels below.  They were moved
// here from cc_kernels.hip as they stood; `static` is the one addition (two translation units of one library include this header).
// The launch order and what each launch may read and write is told at the top of cc_kernels.hip.
#pragma once
#include <cstdint>

#include "cc_core.h"
#include "pytc_common.h"

namespace pytc {

using namespace cc;

constexpr int CC_THREADS = 256;
constexpr int CC_PER_THREAD = TILE / CC_THREADS;
constexpr int CC_SCAN_THREADS = 1024;
static_assert(TILE % CC_THREADS == 0 && RANK_BLOCK % CC_THREADS == 0, "whole passes");
static_assert(TX * 4 == 128, "a tile row of labels is one 128-byte line");

// ------------------------------------------------------------------------------------------------------------- memories of cc_core.h
struct LdsLabels {                                         // a tile's labels: local indices, workgroup scope
  uint32_t* lab;
  __device__ __forceinline__ uint32_t load(uint32_t i) { return __hip_atomic_load(lab + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
  __device__ __forceinline__ uint32_t atomic_min(uint32_t i, uint32_t v) {
    return __hip_atomic_fetch_min(lab + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
};

struct AgentParents {                                      // the parent array while other workgroups lower it (cc_merge, cc_flatten)
  uint32_t* parent;
  __device__ __forceinline__ uint32_t load(uint32_t i) { return __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ __forceinline__ uint32_t atomic_min(uint32_t i, uint32_t v) {
    return __hip_atomic_fetch_min(parent + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};

// ----------------------------------------------------------------------------------------------------------------------- cc_flatten
static __global__ void __launch_bounds__(CC_THREADS) cc_flatten_kernel(uint32_t* parent, long V, int edge_offset) {
  const long v = (long)blockIdx.x * CC_THREADS + threadIdx.x;
  if (v >= V) return;
  AgentParents m{parent};
  const uint32_t p = m.load((uint32_t)v);
  if (p == BACKGROUND) return;
  if (p == (uint32_t)v) {                                  // a root: only this thread stores here; a walk that reads the tag ends at v
    parent[v] = root_slot((uint32_t)v, edge_offset);
    return;
  }
  // roots do not change in this launch: whatever mixture of old parents and already stored roots the walk reads, it ends at the root
  const uint32_t r = find(m, p);
  if (r != p) parent[v] = r;                               // its own voxel: no other thread stores here
}

// -------------------------------------------------------------------------------------------------------------------------- scans
// Exclusive prefix sum of one int per thread over a workgroup of THREADS threads, in thread order; total = the sum.  wave_sums:
// THREADS / WAVE ints of LDS; the closing barrier leaves them free for the next call.
template <int THREADS>
__device__ __forceinline__ int block_exclusive_scan(int c, int* wave_sums, int& total) {
  const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
  int incl = c;
#pragma unroll
  for (int o = 1; o < WAVE; o <<= 1) {
    const int n = __shfl_up(incl, o, WAVE);
    if (lane >= o) incl += n;
  }
  if (lane == WAVE - 1) wave_sums[wave] = incl;
  __syncthreads();
  int before = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < THREADS / WAVE; ++w) {
    const int s = wave_sums[w];
    before += w < wave ? s : 0;
    total += s;
  }
  __syncthreads();
  return before + incl - c;
}

constexpr int RANK_PER = RANK_BLOCK / CC_THREADS;          // a thread takes RANK_PER consecutive voxels, so thread order is raster order

static __global__ void __launch_bounds__(CC_THREADS) cc_rank_kernel(const uint32_t* __restrict__ parent, uint8_t* __restrict__ edges,
                                                                    int32_t* __restrict__ counts, long V) {
  __shared__ int wave_sums[CC_THREADS / WAVE];
  const long first = (long)blockIdx.x * RANK_BLOCK + (long)threadIdx.x * RANK_PER;
  int c = 0;
#pragma unroll
  for (int j = 0; j < RANK_PER; ++j) {
    const long v = first + j;
    if (v >= V) continue;
    const uint32_t p = parent[v];
    if (p == BACKGROUND) continue;
    if ((parent[root_of(p, (uint32_t)v)] & ~TAG) == (uint32_t)v) {        // every component has a seed: no root slot is empty any more
      edges[v] |= (uint8_t)EDGE_HEAD;
      ++c;
    }
  }
  int total;
  block_exclusive_scan<CC_THREADS>(c, wave_sums, total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// counts[b] -> the heads of the blocks before b; count[0] = K.  One workgroup; the carry runs through registers.
static __global__ void __launch_bounds__(CC_SCAN_THREADS) cc_scan_kernel(int32_t* __restrict__ counts, int32_t* __restrict__ count, int blocks) {
  __shared__ int wave_sums[CC_SCAN_THREADS / WAVE];
  int carry = 0;
  for (int base = 0; base < blocks; base += CC_SCAN_THREADS) {
    const int i = base + threadIdx.x;
    const int c = i < blocks ? counts[i] : 0;
    int total;
    const int before = block_exclusive_scan<CC_SCAN_THREADS>(c, wave_sums, total);
    if (i < blocks) counts[i] = carry + before;
    carry += total;
  }
  if (threadIdx.x == 0) count[0] = carry;
}

static __global__ void __launch_bounds__(CC_THREADS) cc_number_kernel(uint32_t* parent, const uint8_t* __restrict__ edges,
                                                                      const int32_t* __restrict__ offsets, long V) {
  __shared__ int wave_sums[CC_THREADS / WAVE];
  const long first = (long)blockIdx.x * RANK_BLOCK + (long)threadIdx.x * RANK_PER;
  bool head[RANK_PER];
  int c = 0;
#pragma unroll
  for (int j = 0; j < RANK_PER; ++j) {
    head[j] = first + j < V && (edges[first + j] & EDGE_HEAD);
    c += head[j] ? 1 : 0;
  }
  int total;
  int id = offsets[blockIdx.x] + block_exclusive_scan<CC_THREADS>(c, wave_sums, total) + 1;
#pragma unroll
  for (int j = 0; j < RANK_PER; ++j) {
    if (!head[j]) continue;
    const uint32_t v = (uint32_t)(first + j);
    // a head that is no root reads its own slot (an index nobody writes now) and writes its root's, which only this thread touches
    parent[root_of(parent[v], v)] = TAG | (uint32_t)id++;
  }
}

static bool ranges_overlap(const void* a, long a_bytes, const void* b, long b_bytes) {
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return pa < pb + b_bytes && pb < pa + a_bytes;
}

}  // namespace pytc
