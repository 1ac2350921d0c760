// Connected components of a thresholded affinity graph on the MI355X: the reference's decode_affinity_cc (decoding/decoders/
// segmentation.py, segmentation_kernels.py connected_components_affinity_3d_numba), which it runs as a serial flood fill on the CPU or
// as min-label sweeps with a host read per iteration.  Here: union-find, eight or nine launches on one stream, no convergence loop and no host
// read.  Integers only; the result is the reference's ids bit for bit.
//
// Volume (A0, A1, A2), v = (i0 A1 + i1) A2 + i2 < 2^31 - 1.  hard[a][v] = aff[a][v] > threshold (strict; NaN is false).  Voxels v and
// v + unit_a are joined iff v + unit_a lies inside and hard[a][v + edge_offset unit_a].  A voxel is foreground iff any hard[a][v] or it
// ends an edge; it is a SEED iff any hard[a][v]: the reference's serial flood fill starts a component only there, so it numbers the
// components 1 .. K in raster order of their smallest seed, the component's HEAD.  With edge_offset 0 the head is the smallest voxel;
// with edge_offset 1 an edge is stored at its far end and the smallest voxel of a component need not be a seed.  Background is 0.
//
// INVARIANT.  While unions run (cc_local's LDS labels, the global parent array through cc_merge) parent[i] <= i at all times, and a
// value only ever decreases.  Every find (cc_core.h) walks on only while the loaded parent is smaller, so it falls strictly and ends
// whatever it reads; every union lowers the larger of two roots.  From cc_flatten on a root's slot holds a tagged value (>= 2^31),
// which ends a walk just as parent[r] == r did.  No loop of this file has an iteration cap, none waits for another thread or workgroup,
// and nothing spins.
//
// TILE.  cc_local works on 8 x 8 x 32 voxels (cc_core.h TZ, TY, TX): 32 uint32 labels along x are one 128-byte line (whole lines
// where A2 is a multiple of 32; any A2 is correct).  A tile's local order (lz, ly, lx) is the order of its global indices, so the
// smallest local index of a set is its smallest global index.
//
// LAUNCHES, in order:
//   cc_edges    the three channel planes -> one byte per voxel: bits 0..2 the edge to +axis a (bounds and edge_offset applied), bit 3
//               foreground, bit 4 seed, from the source values at v and at v -/+ unit_a (no second pass).
//   cc_local    a workgroup stages a tile's edge bytes, unions the edges inside the tile in LDS (atomicMin on local indices) and writes
//               parent[v] = the global index of the tile-local root, 0xFFFFFFFF for background.
//   cc_merge    every edge across a tile face: union of its endpoints in global memory.  The only store to parent in this launch is
//               atomicMin at agent scope and every read of parent is an agent-scope atomic load: the L2s of the eight XCDs are not
//               coherent with each other inside a launch, the atomics are performed where they are.  A stale load would still be an
//               ancestor, and the value atomicMin returns decides how a union goes on.  No flag, no wait.
//   cc_flatten  (a new launch: the kernel boundary makes the merges visible) every foreground voxel follows parent to its root and
//               stores it.  Roots do not change in this launch; a voxel another thread has already rewritten reads as its root instead
//               of an older ancestor of the same set, both lead to the same root.  A root replaces its own slot by a tagged value:
//               TAG | itself with edge_offset 0 (it is the head), "no head yet" with edge_offset 1.
//   cc_vote     (edge_offset 1 only) a seed that no edge joins to a smaller seed offers itself to its root's slot with atomicMin at
//               agent scope; one that reads a smaller candidate there stays silent (a stale read only costs an atomic).  The smallest
//               seed of a component has no smaller seed beside it, so it always votes, and it is what is left: the head.
//   cc_rank     v is a head iff the slot of its root names v.  Per block of 2048 consecutive voxels: the number of heads; bit 5 of a
//               head's own edge byte is set (slots are only read here).
//   cc_scan     one workgroup turns the block counts into exclusive offsets, chunk after chunk with a running carry, and writes K.
//               Not a decoupled look-back: that spins on other workgroups.
//   cc_number   per block again: a head's id = offset of its block + heads before it in the block + 1, stored as TAG | id in the slot
//               of its root (heads are read from the edge bytes: no thread reads a slot another one writes).
//   cc_apply    label[v] = the id in the slot of v's root as int32, 0 for background.
//
// MEMORY.  1 byte (edges) + 4 (parent) + 4 (labels) per voxel and 4 bytes per 2048 voxels (counts), all the caller's.
#include "cc_shared.h"

namespace pytc {

struct CcGeo {
  int A0, A1, A2, t0, t1, t2;                              // t*: tiles per axis
  long V;
};
// ------------------------------------------------------------------------------------------------------------------------- cc_edges
template <typename T>
__global__ void __launch_bounds__(CC_THREADS) cc_edges_kernel(const T* __restrict__ c0, const T* __restrict__ c1, const T* __restrict__ c2,
                                                              uint8_t* __restrict__ edges, CcGeo g, float threshold, int edge_offset) {
  const long v = (long)blockIdx.x * CC_THREADS + threadIdx.x;
  if (v >= g.V) return;
  const long plane = (long)g.A1 * g.A2;
  const int i0 = (int)(v / plane);
  const int rem = (int)(v - (long)i0 * plane);
  const int i1 = rem / g.A2, i2 = rem - i1 * g.A2;
  const T* src[3] = {c0, c1, c2};
  const long unit[3] = {plane, (long)g.A2, 1};
  const int at_i[3] = {i0, i1, i2}, dim[3] = {g.A0, g.A1, g.A2};
  bool at[3], other[3], in_plus[3], in_minus[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    in_plus[a] = at_i[a] + 1 < dim[a];
    in_minus[a] = at_i[a] > 0;
    at[a] = (float)src[a][v] > threshold;
    const bool there = edge_offset ? in_plus[a] : in_minus[a];
    other[a] = there && (float)src[a][edge_offset ? v + unit[a] : v - unit[a]] > threshold;
  }
  edges[v] = (uint8_t)edge_byte(at, other, in_plus, in_minus, edge_offset);
}

// ------------------------------------------------------------------------------------------------------------------------- cc_local
__global__ void __launch_bounds__(CC_THREADS) cc_local_kernel(const uint8_t* __restrict__ edges, uint32_t* __restrict__ parent, CcGeo g) {
  __shared__ uint32_t lab[TILE];
  __shared__ uint8_t edge[TILE];
  int b = blockIdx.x;
  const int x0 = (b % g.t2) * TX;
  b /= g.t2;
  const int y0 = (b % g.t1) * TY, z0 = (b / g.t1) * TZ;
  // local index li = (lz TY + ly) TX + lx; a wave covers two rows of 32 voxels along x
  long at[CC_PER_THREAD];                                  // the global index of the thread's voxels, -1 outside the volume
#pragma unroll
  for (int k = 0; k < CC_PER_THREAD; ++k) {
    const int li = k * CC_THREADS + threadIdx.x;
    const int lx = li % TX, ly = (li / TX) % TY, lz = li / (TX * TY);
    const int z = z0 + lz, y = y0 + ly, x = x0 + lx;
    const bool in = z < g.A0 && y < g.A1 && x < g.A2;
    at[k] = in ? ((long)z * g.A1 + y) * g.A2 + x : -1;
    edge[li] = in ? edges[at[k]] : (uint8_t)0;
    lab[li] = li;
  }
  __syncthreads();
  LdsLabels m{lab};
#pragma unroll
  for (int k = 0; k < CC_PER_THREAD; ++k) {
    const int li = k * CC_THREADS + threadIdx.x;
    const int lx = li % TX, ly = (li / TX) % TY, lz = li / (TX * TY);
    const unsigned e = edge[li];                           // an edge bit implies that the neighbour lies inside the volume
    if ((e & 1) && lz + 1 < TZ) unite(m, (uint32_t)li, (uint32_t)(li + TX * TY));
    if ((e & 2) && ly + 1 < TY) unite(m, (uint32_t)li, (uint32_t)(li + TX));
    if ((e & 4) && lx + 1 < TX) unite(m, (uint32_t)li, (uint32_t)(li + 1));
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < CC_PER_THREAD; ++k) {
    if (at[k] < 0) continue;
    const int li = k * CC_THREADS + threadIdx.x;
    uint32_t out = BACKGROUND;
    if (edge[li] & EDGE_FG) {
      const int r = (int)find(m, (uint32_t)li);            // labels are final: no union runs any more
      const int rx = r % TX, ry = (r / TX) % TY, rz = r / (TX * TY);
      out = (uint32_t)(((long)(z0 + rz) * g.A1 + (y0 + ry)) * g.A2 + (x0 + rx));
    }
    parent[at[k]] = out;
  }
}

// ------------------------------------------------------------------------------------------------------------------------- cc_merge
__global__ void __launch_bounds__(CC_THREADS) cc_merge_kernel(const uint8_t* __restrict__ edges, uint32_t* parent, CcGeo g) {
  const long v = (long)blockIdx.x * CC_THREADS + threadIdx.x;
  if (v >= g.V) return;
  const unsigned e = edges[v];
  if (!(e & 7)) return;
  const long plane = (long)g.A1 * g.A2;
  const int i0 = (int)(v / plane);
  const int rem = (int)(v - (long)i0 * plane);
  const int i1 = rem / g.A2, i2 = rem - i1 * g.A2;
  AgentParents m{parent};
  // the edge leaves the tile of v: its other end is the first voxel of the next tile along the axis
  if ((e & 1) && i0 % TZ == TZ - 1) unite(m, (uint32_t)v, (uint32_t)(v + plane));
  if ((e & 2) && i1 % TY == TY - 1) unite(m, (uint32_t)v, (uint32_t)(v + g.A2));
  if ((e & 4) && i2 % TX == TX - 1) unite(m, (uint32_t)v, (uint32_t)(v + 1));
}
// -------------------------------------------------------------------------------------------------------------------------- cc_vote
__global__ void __launch_bounds__(CC_THREADS) cc_vote_kernel(const uint8_t* __restrict__ edges, uint32_t* parent, CcGeo g) {
  const long v = (long)blockIdx.x * CC_THREADS + threadIdx.x;
  if (v >= g.V || !(edges[v] & EDGE_SEED)) return;
  const long unit[3] = {(long)g.A1 * g.A2, (long)g.A2, 1};
  if (!may_be_head(edges, v, unit)) return;
  AgentParents m{parent};
  const uint32_t r = root_of(m.load((uint32_t)v), (uint32_t)v);          // a seed is foreground: its slot is a root index or a tag
  const uint32_t mine = head_candidate((uint32_t)v);
  if (mine < m.load(r)) m.atomic_min(r, mine);
}

// ------------------------------------------------------------------------------------------------------------------------- cc_apply
__global__ void __launch_bounds__(CC_THREADS) cc_apply_kernel(const uint32_t* __restrict__ parent, int32_t* __restrict__ labels, long V) {
  const long v = (long)blockIdx.x * CC_THREADS + threadIdx.x;
  if (v >= V) return;
  const uint32_t p = parent[v];
  labels[v] = p == BACKGROUND ? 0 : (int32_t)(parent[root_of(p, (uint32_t)v)] & ~TAG);
}

template <typename T>
static void launch_edges(const void* c0, const void* c1, const void* c2, uint8_t* edges, const CcGeo& g, float threshold, int edge_offset,
                         hipStream_t st) {
  hipLaunchKernelGGL((cc_edges_kernel<T>), dim3(ceil_div(g.V, CC_THREADS)), dim3(CC_THREADS), 0, st, static_cast<const T*>(c0),
                     static_cast<const T*>(c1), static_cast<const T*>(c2), edges, g, threshold, edge_offset);
}

}  // namespace pytc

using namespace pytc;

extern "C" int pytc_affinity_cc_tile(int axis) { return axis == 0 ? TZ : (axis == 1 ? TY : (axis == 2 ? TX : 0)); }

extern "C" int64_t pytc_affinity_cc_blocks(int64_t voxels) { return voxels < 1 ? 0 : (voxels + RANK_BLOCK - 1) / RANK_BLOCK; }

extern "C" int pytc_affinity_cc(const void* c0, const void* c1, const void* c2, int dtype, float threshold, int edge_offset, void* edges,
                                void* parent, int32_t* counts, int32_t* labels, int32_t* count, int A0, int A1, int A2, void* stream) {
  const char* what = "affinity_cc";
  PYTC_REQUIRE(c0 && c1 && c2 && edges && parent && counts && labels && count, "%s: the three channels, edges, parent, counts, labels and "
               "count are required", what);
  PYTC_REQUIRE(A0 >= 1 && A1 >= 1 && A2 >= 1, "%s: bad shape (%d, %d, %d)", what, A0, A1, A2);
  const long V = (long)A0 * A1 * A2;
  PYTC_REQUIRE(V < 0x7fffffffL, "%s: %ld voxels; ids and indices are 31 bits and 2^31 - 1 is kept for the background", what, V);
  PYTC_REQUIRE(edge_offset == 0 || edge_offset == 1, "%s: edge_offset %d is neither 0 nor 1", what, edge_offset);
  PYTC_REQUIRE(dtype == PYTC_F16 || dtype == PYTC_F32 || dtype == PYTC_BF16, "%s: bad dtype %d", what, dtype);
  const int width = dtype == PYTC_F32 ? 4 : 2;
  const void* ch[3] = {c0, c1, c2};
  for (int a = 0; a < 3; ++a)
    PYTC_REQUIRE(reinterpret_cast<uintptr_t>(ch[a]) % width == 0, "%s: channel %d is not aligned to its %d-byte elements", what, a, width);
  PYTC_REQUIRE(reinterpret_cast<uintptr_t>(parent) % 4 == 0 && reinterpret_cast<uintptr_t>(counts) % 4 == 0 &&
               reinterpret_cast<uintptr_t>(labels) % 4 == 0 && reinterpret_cast<uintptr_t>(count) % 4 == 0,
               "%s: parent, counts, labels and count must be 4-byte aligned", what);
  const long blocks = (long)pytc_affinity_cc_blocks(V);
  const void* outs[5] = {edges, parent, counts, labels, count};
  const long out_bytes[5] = {V, 4 * V, 4 * blocks, 4 * V, 4};
  const char* out_names[5] = {"edges", "parent", "counts", "labels", "count"};
  for (int i = 0; i < 5; ++i) {
    for (int a = 0; a < 3; ++a)
      PYTC_REQUIRE(!ranges_overlap(outs[i], out_bytes[i], ch[a], V * width), "%s: %s must not alias channel %d", what, out_names[i], a);
    for (int j = 0; j < i; ++j)
      PYTC_REQUIRE(!ranges_overlap(outs[i], out_bytes[i], outs[j], out_bytes[j]), "%s: %s must not alias %s", what, out_names[i], out_names[j]);
  }
  CcGeo g{A0, A1, A2, ceil_div(A0, TZ), ceil_div(A1, TY), ceil_div(A2, TX), V};
  const long tiles = (long)g.t0 * g.t1 * g.t2;
  PYTC_REQUIRE(tiles <= 0x7fffffffL, "%s: %ld tiles", what, tiles);
  hipStream_t st = (hipStream_t)stream;
  uint8_t* e8 = static_cast<uint8_t*>(edges);
  uint32_t* par = static_cast<uint32_t*>(parent);
  const dim3 per_voxel(ceil_div(V, CC_THREADS)), threads(CC_THREADS);
  if (dtype == PYTC_F16)                                   // the one entry that reads fp16 predictions; the other codes take the one dispatch
    launch_edges<_Float16>(c0, c1, c2, e8, g, threshold, edge_offset, st);
  else
    PYTC_DISPATCH_DTYPE(dtype, what, T, launch_edges<T>(c0, c1, c2, e8, g, threshold, edge_offset, st));
  PYTC_LAUNCH_CHECK("affinity_cc (edges)");
  hipLaunchKernelGGL(cc_local_kernel, dim3((unsigned)tiles), threads, 0, st, e8, par, g);
  PYTC_LAUNCH_CHECK("affinity_cc (local)");
  hipLaunchKernelGGL(cc_merge_kernel, per_voxel, threads, 0, st, e8, par, g);
  PYTC_LAUNCH_CHECK("affinity_cc (merge)");
  hipLaunchKernelGGL(cc_flatten_kernel, per_voxel, threads, 0, st, par, V, edge_offset);
  PYTC_LAUNCH_CHECK("affinity_cc (flatten)");
  if (edge_offset) {
    hipLaunchKernelGGL(cc_vote_kernel, per_voxel, threads, 0, st, e8, par, g);
    PYTC_LAUNCH_CHECK("affinity_cc (vote)");
  }
  hipLaunchKernelGGL(cc_rank_kernel, dim3((unsigned)blocks), threads, 0, st, par, e8, counts, V);
  PYTC_LAUNCH_CHECK("affinity_cc (rank)");
  hipLaunchKernelGGL(cc_scan_kernel, dim3(1), dim3(CC_SCAN_THREADS), 0, st, counts, count, (int)blocks);
  PYTC_LAUNCH_CHECK("affinity_cc (scan)");
  hipLaunchKernelGGL(cc_number_kernel, dim3((unsigned)blocks), threads, 0, st, par, e8, counts, V);
  PYTC_LAUNCH_CHECK("affinity_cc (number)");
  hipLaunchKernelGGL(cc_apply_kernel, per_voxel, threads, 0, st, par, labels, V);
  PYTC_LAUNCH_CHECK("affinity_cc (apply)");
  return PYTC_OK;
}
