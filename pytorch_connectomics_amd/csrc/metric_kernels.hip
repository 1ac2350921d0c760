// The evaluation metrics (jaccard, dice, accuracy; binary and multi-class) on the MI355X: one streaming pass that turns logits and
// labels into a K x K table of integer counts.  Every metric is a function of that table (training/metrics.py), and the counts add
// across batches and ranks exactly, so the kernels know nothing of the metrics.
//
//   counts[t * K + p] += the voxels with target class t and predicted class p;   counts[K * K] += the voxels whose index target lies
//   outside [0, K): they enter no cell.   K = max(C, 2).
//
// x is fp32 (N, C, R) addressed by (stride_n, stride_c, stride_r) as in softmax_loss_kernels.hip: a channels-last output, a plain NCDHW
// tensor or a channel slice of a wider tensor, none of them copied.  Predicted class: C == 1: x > pred_threshold (strict; NaN -> 0);
// C >= 2: the first index of the maximum with NaN counting as the maximum (torch.argmax on the CPU: [inf, nan, inf] -> 1).  Target
// class: an index (fp32 truncated toward zero, int64 or uint8), a threshold (C == 1: t > target_threshold) or the argmax of a dense
// fp32 (N, C, R) target by the same rule.
//
// Work split.  A workgroup of 256 threads takes CC_TILE = 4096 consecutive voxels of one sample; a lane owns whole voxels, so the
// argmax is a running (best, index) pair in two registers for any C.  Three load forms, chosen on the host from strides and alignment:
//   VPL = 4  stride_r == 1 (NCDHW): a lane takes four consecutive voxels and reads each channel as one 16-byte vector (a uint8 label
//            as one dword), consecutive lanes consecutive vectors;
//   CVEC     stride_c == 1, C % 4 == 0 (channels-last): a lane reads its voxel's channels as 16-byte vectors;
//   scalar   everything else: one dword per (voxel, channel); with stride_r == 1 consecutive lanes still read consecutive voxels.
// Counting.  K == 2: four __ballot masks per voxel step (target bit, prediction bit, valid, active) and popcounts of their
// intersections, accumulated in wave-uniform registers: no LDS traffic in the loop.  K > 2: one LDS table per workgroup with
// wave-aggregated adds: the wave loops over the DISTINCT cells it holds, and the leader lane of each adds popc(ballot(cell ==
// leader's cell)) with one LDS atomic; a segmentation volume puts most of a wave into cell (0, 0), which costs one add, not 64
// serialised ones.  A tile's row of K * K + 1 counts is written with plain stores; a second launch adds the rows in int64 into
// `counts` (integer adds: any order gives the same table).  No float arithmetic on a count anywhere, no host synchronisation.
//
// Invariant: a partial cell counts voxels of ONE tile, so it never exceeds CC_TILE = 4096 < 2^31 and uint32 cannot wrap; everything
// summed over more than one tile is int64.
#include <cmath>
#include <cstdint>

#include "pytc_common.h"

namespace pytc {

constexpr int CC_THREADS = 256;
constexpr int CC_TILE = 4096;            // voxels per workgroup = voxels per partial row (pytc_confusion_tiles)
constexpr int CC_MAX_C = 32;
constexpr int CC_NW = CC_THREADS / WAVE;
constexpr int CC_FLIGHT = 8;             // voxels a lane loads before it counts any of them
static_assert(CC_TILE % (CC_THREADS * 4) == 0, "a tile is a whole number of passes in every load form");

struct CcGeo {
  long R;
  int C, K, tiles;
  long xs[3], ts[3];
  int tdtype, tmode;
  float pthr, tthr;
};

// v[j] = p[j * stride] for j < live (0 beyond); four live values of a VPL = 4 lane are one aligned vector (the host checked
// stride == 1 and the alignment of every such address before choosing VPL = 4)
template <typename T, int VPL>
__device__ __forceinline__ void cc_load(const T* __restrict__ p, long stride, int live, T (&v)[VPL]) {
  if (VPL == 4 && live == 4) {
    typedef T vec_t __attribute__((ext_vector_type(4)));
    const vec_t q = *reinterpret_cast<const vec_t*>(p);
#pragma unroll
    for (int j = 0; j < VPL; ++j) v[j] = q[j];
  } else {
#pragma unroll
    for (int j = 0; j < VPL; ++j) v[j] = j < live ? p[j * stride] : T(0);
  }
}

// first index of the maximum, NaN counting as the maximum: once `best` is NaN nothing replaces it
__device__ __forceinline__ void cc_take(float v, int c, float& best, int& bi) {
  if (best == best && (v > best || v != v)) {
    best = v;
    bi = c;
  }
}

// A lane works on U groups of VPL consecutive voxels at once (group u has live[u] voxels inside the sample, 0 beyond it), and every
// loop over channels loads for all U groups before it compares: U * VPL independent loads in flight per lane.

// cls[u][j] = argmax over the C channels of voxel j of group u; p[u] points at channel 0 of the group's first voxel
template <int VPL, int U, bool CVEC>
__device__ __forceinline__ void cc_argmax(const float* const (&p)[U], long sc, long sr, int C, const int (&live)[U], int (&cls)[U][VPL]) {
  float best[U][VPL];
  if (CVEC) {                                             // VPL == 1, sc == 1, C % 4 == 0
#pragma unroll
    for (int u = 0; u < U; ++u) {
      best[u][0] = -INFINITY;
      cls[u][0] = 0;
    }
    for (int c = 0; c < C; c += 4) {
      f32x4_t v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) v[u] = live[u] ? *reinterpret_cast<const f32x4_t*>(p[u] + c) : f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (c == 0) best[u][0] = v[u][0];                 // (channel 0 starts the running maximum, whatever its value)
#pragma unroll
        for (int k = 0; k < 4; ++k) cc_take(v[u][k], c + k, best[u][0], cls[u][0]);
      }
    }
    return;
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    cc_load<float, VPL>(p[u], sr, live[u], best[u]);
#pragma unroll
    for (int j = 0; j < VPL; ++j) cls[u][j] = 0;
  }
  for (int c = 1; c < C; ++c) {
    float v[U][VPL];
#pragma unroll
    for (int u = 0; u < U; ++u) cc_load<float, VPL>(p[u] + c * sc, sr, live[u], v[u]);
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int j = 0; j < VPL; ++j) cc_take(v[u][j], c, best[u][j], cls[u][j]);
  }
}

// the class of one label: index mode -> [0, K) or -1 (invalid); threshold mode -> t > target_threshold
__device__ __forceinline__ int cc_label_class(float v, const CcGeo& g) {
  if (g.tmode == 1) return v > g.tthr ? 1 : 0;
  return (v > -1.f && v < (float)g.K) ? (int)v : -1;      // truncation toward zero: (-1, 0) -> 0; false for NaN
}
__device__ __forceinline__ int cc_label_class(long v, const CcGeo& g) {
  if (g.tmode == 1) return (float)v > g.tthr ? 1 : 0;
  return (v >= 0 && v < g.K) ? (int)v : -1;
}
__device__ __forceinline__ int cc_label_class(uint8_t v, const CcGeo& g) { return cc_label_class((long)v, g); }

template <typename T, int VPL, int U>
__device__ __forceinline__ void cc_label_classes(const void* __restrict__ target, const long (&off)[U], const CcGeo& g,
                                                 const int (&live)[U], int (&cls)[U][VPL]) {
  T v[U][VPL];
#pragma unroll
  for (int u = 0; u < U; ++u) cc_load<T, VPL>(static_cast<const T*>(target) + off[u], g.ts[2], live[u], v[u]);
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int j = 0; j < VPL; ++j) cls[u][j] = cc_label_class(v[u][j], g);
}

// cell[u][j] = t * K + p of voxel r0[u] + j of sample n; K * K for an invalid label; -1 beyond the sample
template <int VPL, int U, bool CVEC>
__device__ __forceinline__ void cc_cells(const float* __restrict__ x, const void* __restrict__ target, const CcGeo& g, int n,
                                         const long (&r0)[U], int (&cell)[U][VPL]) {
  int live[U], p[U][VPL], t[U][VPL];
  long toff[U];
  const float* px[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    live[u] = r0[u] >= g.R ? 0 : (g.R - r0[u] < VPL ? (int)(g.R - r0[u]) : VPL);
    const long r = live[u] ? r0[u] : 0;                   // a group beyond the sample loads nothing; its addresses stay inside
    px[u] = x + n * g.xs[0] + r * g.xs[2];
    toff[u] = n * g.ts[0] + r * g.ts[2];
  }
  if (g.C == 1) {
    float v[U][VPL];
#pragma unroll
    for (int u = 0; u < U; ++u) cc_load<float, VPL>(px[u], g.xs[2], live[u], v[u]);
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int j = 0; j < VPL; ++j) p[u][j] = v[u][j] > g.pthr ? 1 : 0;
  } else {
    cc_argmax<VPL, U, CVEC>(px, g.xs[1], g.xs[2], g.C, live, p);
  }
  if (g.tmode == 2) {
    const float* pt[U];
#pragma unroll
    for (int u = 0; u < U; ++u) pt[u] = static_cast<const float*>(target) + toff[u];
    cc_argmax<VPL, U, false>(pt, g.ts[1], g.ts[2], g.C, live, t);
  } else if (g.tdtype == PYTC_TARGET_F32) {
    cc_label_classes<float, VPL, U>(target, toff, g, live, t);
  } else if (g.tdtype == PYTC_TARGET_I64) {
    cc_label_classes<long, VPL, U>(target, toff, g, live, t);
  } else {
    cc_label_classes<uint8_t, VPL, U>(target, toff, g, live, t);
  }
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int j = 0; j < VPL; ++j) cell[u][j] = j < live[u] ? (t[u][j] < 0 ? g.K * g.K : t[u][j] * g.K + p[u][j]) : -1;
}

template <int VPL, bool CVEC, bool K2>
__global__ void __launch_bounds__(CC_THREADS) confusion_tile_kernel(const float* __restrict__ x, const void* __restrict__ target,
                                                                    uint32_t* __restrict__ partial, CcGeo g) {
  constexpr int HIST = K2 ? CC_NW * 5 : CC_MAX_C * CC_MAX_C + 1;
  __shared__ uint32_t hist[HIST];
  const int n = blockIdx.y, wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
  const int rowlen = g.K * g.K + 1;
  const long tile0 = (long)blockIdx.x * CC_TILE;
  if (!K2) {
    for (int i = threadIdx.x; i < rowlen; i += CC_THREADS) hist[i] = 0;
    __syncthreads();
  }
  uint32_t w00 = 0, w01 = 0, w10 = 0, w11 = 0, wbad = 0;  // K == 2: this wave's counts, the same value in every lane
  // every lane runs every pass (the ballots below want whole waves); a lane beyond the sample holds cell = -1 and loads nothing.
  // The cells of CC_FLIGHT voxels per lane are formed before any of them is counted: their loads do not wait for the ballots and
  // LDS adds of the voxel before (one voxel in flight per lane left the kernel waiting on load latency, not on HBM)
  constexpr int PASSES = CC_TILE / (CC_THREADS * VPL), U = CC_FLIGHT / VPL;
  static_assert(PASSES % U == 0, "whole batches of passes");
  for (int it0 = 0; it0 < PASSES; it0 += U) {
    int cell[U][VPL];
    long r0[U];
#pragma unroll
    for (int u = 0; u < U; ++u) r0[u] = tile0 + ((long)(it0 + u) * CC_THREADS + threadIdx.x) * VPL;
    cc_cells<VPL, U, CVEC>(x, target, g, n, r0, cell);
#pragma unroll
    for (int q = 0; q < U * VPL; ++q) {
      const int c = cell[q / VPL][q % VPL];
      if (K2) {
        const unsigned long long ba = __ballot(c >= 0), bv = __ballot(c >= 0 && c < 4);
        const unsigned long long bt = __ballot(c >= 0 && (c & 2)) & bv, bp = __ballot(c >= 0 && (c & 1)) & bv;
        w11 += __popcll(bt & bp);
        w10 += __popcll(bt & ~bp);
        w01 += __popcll(~bt & bp & bv);
        w00 += __popcll(~bt & ~bp & bv);
        wbad += __popcll(ba & ~bv);
      } else {
        unsigned long long todo = __ballot(c >= 0);       // wave-uniform: the loop below does not diverge
        while (todo) {
          const int leader = __ffsll((long long)todo) - 1;
          const int lc = __shfl(c, leader, WAVE);
          const unsigned long long same = __ballot(c == lc);
          if (lane == leader) atomicAdd(&hist[lc], (uint32_t)__popcll(same));   // one add per distinct cell of the wave
          todo &= ~same;
        }
      }
    }
  }
  uint32_t* row = partial + ((long)n * g.tiles + blockIdx.x) * rowlen;
  if (K2) {
    if (lane == 0) {
      hist[wave * 5 + 0] = w00;
      hist[wave * 5 + 1] = w01;
      hist[wave * 5 + 2] = w10;
      hist[wave * 5 + 3] = w11;
      hist[wave * 5 + 4] = wbad;
    }
    __syncthreads();
    if (threadIdx.x < 5) {
      uint32_t a = 0;
#pragma unroll
      for (int q = 0; q < CC_NW; ++q) a += hist[q * 5 + threadIdx.x];
      row[threadIdx.x] = a;
    }
  } else {
    __syncthreads();
    for (int i = threadIdx.x; i < rowlen; i += CC_THREADS) row[i] = hist[i];
  }
}

// counts[e] += the sum over the partial rows of cell e, in int64: one column of workgroups per cell, the rows strided over the
// column's workgroups and threads (neighbouring cells' workgroups share the 64-byte lines they read through L2), then the shared
// workgroup reduction and one integer atomic per workgroup
__global__ void __launch_bounds__(CC_THREADS) confusion_sum_kernel(const uint32_t* __restrict__ partial, long long* __restrict__ counts,
                                                                   long rows, int rowlen) {
  __shared__ long long red[CC_THREADS];
  const int e = blockIdx.x;
  long long a = 0;
  for (long r = (long)blockIdx.y * CC_THREADS + threadIdx.x; r < rows; r += (long)gridDim.y * CC_THREADS) a += partial[r * rowlen + e];
  a = block_sum<CC_THREADS>(a, red);
  if (threadIdx.x == 0 && a != 0) atomicAdd(reinterpret_cast<unsigned long long*>(counts + e), (unsigned long long)a);
}

// every address a VPL = 4 lane reads as a vector of four `elem`-byte values is aligned: the base, and the strides that move it
// (the sample stride with more than one sample, the channel stride where channels are walked)
static bool cc_vec4_ok(const void* p, int elem, long s0, bool use_s0, long s1, bool use_s1, long s2) {
  return s2 == 1 && (reinterpret_cast<uintptr_t>(p) % (4 * elem)) == 0 && (!use_s0 || s0 % 4 == 0) && (!use_s1 || s1 % 4 == 0);
}

}  // namespace pytc

using namespace pytc;

extern "C" int pytc_confusion_tiles(int64_t R) { return R >= 1 ? ceil_div((long)R, CC_TILE) : 0; }

#define CC_LAUNCH(VPL, CVEC)                                                                                               \
  do {                                                                                                                     \
    if (g.K == 2)                                                                                                          \
      hipLaunchKernelGGL((confusion_tile_kernel<VPL, CVEC, true>), grid, dim3(CC_THREADS), 0, st, x, target, partial, g);  \
    else                                                                                                                   \
      hipLaunchKernelGGL((confusion_tile_kernel<VPL, CVEC, false>), grid, dim3(CC_THREADS), 0, st, x, target, partial, g); \
  } while (0)

extern "C" int pytc_confusion_counts(const float* x, const void* target, uint32_t* partial, int64_t* counts, int N, int C, int64_t R,
                                     const int64_t* x_strides, const int64_t* t_strides, int target_dtype, int target_mode,
                                     float pred_threshold, float target_threshold, void* stream) {
  const char* what = "confusion_counts";
  PYTC_REQUIRE(N >= 1 && C >= 1 && R >= 1, "%s: bad shape N %d, C %d, R %ld", what, N, C, (long)R);
  if (C > CC_MAX_C) {
    set_error("%s: C = %d; the count kernels cover 1 <= C <= %d", what, C, CC_MAX_C);
    return PYTC_ERR_UNSUPPORTED;
  }
  PYTC_REQUIRE(x && target && partial && counts && x_strides && t_strides, "%s: x, target, partial, counts and the strides are required",
               what);
  PYTC_REQUIRE(target_dtype == PYTC_TARGET_F32 || target_dtype == PYTC_TARGET_I64 || target_dtype == PYTC_TARGET_U8,
               "%s: unknown target_dtype %d", what, target_dtype);
  PYTC_REQUIRE(target_mode >= 0 && target_mode <= 2, "%s: unknown target_mode %d", what, target_mode);
  PYTC_REQUIRE(target_mode != 1 || C == 1, "%s: a threshold target needs C == 1, got C = %d", what, C);
  PYTC_REQUIRE(target_mode != 2 || (C >= 2 && target_dtype == PYTC_TARGET_F32), "%s: a dense target needs C >= 2 and fp32", what);
  PYTC_REQUIRE(N <= 65535, "%s: %d samples", what, N);
  PYTC_REQUIRE(((long)R + CC_TILE - 1) / CC_TILE <= 0x7fffffffL, "%s: %ld voxels per sample", what, (long)R);
  CcGeo g;
  g.R = R;
  g.C = C;
  g.K = C > 2 ? C : 2;
  g.tiles = ceil_div((long)R, CC_TILE);
  for (int i = 0; i < 3; ++i) {
    g.xs[i] = x_strides[i];
    g.ts[i] = t_strides[i];
    PYTC_REQUIRE(g.xs[i] >= 0 && g.ts[i] >= 0, "%s: negative stride", what);
  }
  g.tdtype = target_dtype;
  g.tmode = target_mode;
  g.pthr = pred_threshold;
  g.tthr = target_threshold;
  const int telem = target_dtype == PYTC_TARGET_U8 ? 1 : (target_dtype == PYTC_TARGET_I64 ? 8 : 4);
  const bool vpl4 = cc_vec4_ok(x, 4, g.xs[0], N > 1, g.xs[1], C > 1, g.xs[2]) &&
                    cc_vec4_ok(target, telem, g.ts[0], N > 1, g.ts[1], target_mode == 2, g.ts[2]);
  const bool cvec = C >= 4 && C % 4 == 0 && g.xs[1] == 1 && (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (N == 1 || g.xs[0] % 4 == 0) &&
                    (R == 1 || g.xs[2] % 4 == 0);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(g.tiles, N);
  if (vpl4)
    CC_LAUNCH(4, false);
  else if (cvec)
    CC_LAUNCH(1, true);
  else
    CC_LAUNCH(1, false);
  PYTC_LAUNCH_CHECK("confusion_counts");
  const long rows = (long)N * g.tiles;
  const int slabs = (int)(rows / (CC_THREADS * 16) < 1 ? 1 : (rows / (CC_THREADS * 16) > 256 ? 256 : rows / (CC_THREADS * 16)));
  hipLaunchKernelGGL(confusion_sum_kernel, dim3(g.K * g.K + 1, slabs), dim3(CC_THREADS), 0, st, partial,
                     reinterpret_cast<long long*>(counts), rows, g.K * g.K + 1);
  PYTC_LAUNCH_CHECK("confusion_counts_sum");
  return PYTC_OK;
}
