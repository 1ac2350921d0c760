// The softmax losses (CrossEntropyLoss, softmax Dice, DiceCE, GeneralizedDice) on the MI355X: one kernel pair for all of them.  The
// forward reads every voxel's C logits once, forms the softmax over the channel axis and reduces eight sums per (sample, class);
// the backward recomputes the softmax from the operands and writes dx from d loss / d sums.  Everything a loss does with the sums
// (Dice ratios, class weights, label smoothing, reductions) is torch on the (N, C, 8) tensor: the kernels know nothing of it.
//
//   sums[n][c][0..7] = sum over voxels of  p t,  p,  p^2,  t,  t^2,  valid t (-logp),  valid (-logp),  valid t
//
// x is fp32 (N, C, R) addressed by (stride_n, stride_c, stride_r): the channels-last network output, a plain NCDHW tensor or a
// channel slice of a wider channels-last tensor, none of them copied.  The target is dense fp32 (N, C, R), a class index as fp32
// (N, R) (truncated toward zero) or as int64 (N, R); for an index target t = onehot(y), and a voxel with y == ignore_index is
// "CE-invalid" (valid = 0) with t = 0 in every channel.  A label outside [0, C) that is not ignore_index traps nothing: it puts NaN
// into column 5 of every class of its sample, and the loss built on the sums is then not finite.
//
// mask (nullable, C channels or one through a channel stride of 0): where mask <= 0 the logit reads as `fill` and a dense target
// as 0; an index label reads as 0 (class 0) unless every channel of its voxel is valid.  The voxel still counts in the sums (with
// p = 1 / C where all channels are masked); dx is 0 at every masked element.
//
// Work split.  A workgroup of 256 threads takes SL_TILE = 2048 consecutive voxels of one sample.  L = 1, 2 or 4 adjacent lanes own
// one voxel and CPL = 2, 4 or 8 channels each (C <= 2: 2 x 1, <= 4: 4 x 1, <= 8: 8 x 1, <= 16: 8 x 2, <= 32: 8 x 4), so a lane keeps
// its logits and its 8 CPL running sums in registers and the channel reduction crosses at most four lanes.  With stride_c == 1 and
// 16-byte alignment a lane loads its channels as 16-byte vectors (whole vectors inside [0, C) only).  The tile's sums are reduced
// across lanes by shuffles and across the four waves through LDS in a fixed order, written as one partial per tile, and a second
// launch adds the tiles of a sample (one wave per sum, a fixed order): no atomics, two runs give the same bits.
#include <cmath>
#include <cstdint>

#include "pytc_common.h"

#pragma clang fp contract(off)

namespace pytc {

constexpr int SL_THREADS = 256;
constexpr int SL_TILE = 2048;            // voxels per workgroup: also the voxels per partial of pytc_softmax_loss_tiles
constexpr int SL_COLS = 8;
constexpr int SL_MAX_C = 32;

struct SlGeo {
  long R;
  int C, tiles;
  long xs[3], ts[3], ms[3], ds[3];
  int target_kind;
  long ignore_index;
  float fill;
};

template <int L>
__device__ __forceinline__ float sl_lane_sum(float v) {
#pragma unroll
  for (int o = 1; o < L; o <<= 1) v += __shfl_xor(v, o, WAVE);
  return v;
}

template <int L>
__device__ __forceinline__ float sl_lane_max(float v) {
#pragma unroll
  for (int o = 1; o < L; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, WAVE));
  return v;
}

template <int L>
__device__ __forceinline__ int sl_lane_and(int v) {
#pragma unroll
  for (int o = 1; o < L; o <<= 1) v &= __shfl_xor(v, o, WAVE);
  return v;
}

// One voxel's channels [c0, c0 + CPL) of this lane: x (masked -> fill), t, valid; p and -logp.  All lanes of a voxel call this together.
template <int CPL, int L, bool VEC>
struct SlVoxel {
  float p[CPL], nlogp[CPL], t[CPL];
  bool live[CPL];          // the element is not masked (its dx may be non-zero)
  float valid;             // 1 where the voxel enters the CE columns
  bool bad;                // an index label outside [0, C) that is not ignore_index

  __device__ __forceinline__ void load(const float* __restrict__ x, const void* __restrict__ target, const float* __restrict__ mask,
                                       const SlGeo& g, int n, long r, int c0) {
    float xv[CPL];
    const float* px = x + n * g.xs[0] + r * g.xs[2];
    const float* pm = mask ? mask + n * g.ms[0] + r * g.ms[2] : nullptr;
#pragma unroll
    for (int q = 0; q < CPL; q += 4) {
      if (VEC && CPL >= 4 && c0 + q + 4 <= g.C) {
        const f32x4_t v = *reinterpret_cast<const f32x4_t*>(px + c0 + q);
#pragma unroll
        for (int j = 0; j < 4 && q + j < CPL; ++j) xv[q + j] = v[j];
      } else {
#pragma unroll
        for (int j = 0; j < 4 && q + j < CPL; ++j) xv[q + j] = c0 + q + j < g.C ? px[(c0 + q + j) * g.xs[1]] : 0.f;
      }
    }
    int all_live = 1;
    const bool one = g.ms[1] == 0;                        // a one-channel mask: one load per voxel
    const bool live0 = (pm && one) ? pm[0] > 0.f : true;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      live[j] = live0;
      if (pm && !one && c0 + j < g.C) live[j] = pm[(c0 + j) * g.ms[1]] > 0.f;
      if (!live[j]) {
        xv[j] = g.fill;
        all_live = 0;
      }
    }
    bad = false;
    valid = 1.f;
    if (g.target_kind == 0) {
      const float* pt = static_cast<const float*>(target) + n * g.ts[0] + r * g.ts[2];
#pragma unroll
      for (int j = 0; j < CPL; ++j) t[j] = (c0 + j < g.C && live[j]) ? pt[(c0 + j) * g.ts[1]] : 0.f;
    } else {
      long y;
      bool finite = true;
      if (g.target_kind == 1) {
        const float fy = static_cast<const float*>(target)[n * g.ts[0] + r * g.ts[2]];
        finite = fy > -9.0e18f && fy < 9.0e18f;          // false for NaN too
        y = finite ? (long)fy : 0;
      } else {
        y = static_cast<const long*>(target)[n * g.ts[0] + r * g.ts[2]];
      }
      if (pm && !sl_lane_and<L>(all_live)) {
        y = 0;
        finite = true;
      }
      const bool ignored = finite && y == g.ignore_index;
      if (ignored) valid = 0.f;
      bad = !finite || (!ignored && (y < 0 || y >= g.C));
#pragma unroll
      for (int j = 0; j < CPL; ++j) t[j] = (!ignored && !bad && y == c0 + j) ? 1.f : 0.f;
    }
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < CPL; ++j)
      if (c0 + j < g.C) m = fmaxf(m, xv[j]);
    m = sl_lane_max<L>(m);
    float e[CPL], s = 0.f;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      e[j] = c0 + j < g.C ? expf(xv[j] - m) : 0.f;
      s += e[j];
    }
    s = sl_lane_sum<L>(s);
    const float ls = logf(s), inv = 1.f / s;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      nlogp[j] = c0 + j < g.C ? ls - (xv[j] - m) : 0.f;
      p[j] = e[j] * inv;
    }
  }
};

template <int CPL, int L, bool VEC>
__global__ void __launch_bounds__(SL_THREADS) softmax_loss_forward_kernel(const float* __restrict__ x, const void* __restrict__ target,
                                                                          const float* __restrict__ mask, float* __restrict__ partial,
                                                                          SlGeo g) {
  constexpr int VOX = SL_THREADS / L;                    // voxels per pass of the workgroup
  constexpr int NW = SL_THREADS / WAVE;
  __shared__ float red[NW][L * CPL * SL_COLS];
  const int n = blockIdx.y, sub = threadIdx.x % L, c0 = sub * CPL;
  const long base = (long)blockIdx.x * SL_TILE + threadIdx.x / L;
  float acc[CPL][SL_COLS];
#pragma unroll
  for (int j = 0; j < CPL; ++j)
#pragma unroll
    for (int k = 0; k < SL_COLS; ++k) acc[j][k] = 0.f;
  bool bad = false;
  for (int it = 0; it < SL_TILE / VOX; ++it) {
    const long r = base + (long)it * VOX;
    if (r >= g.R) break;                                 // the L lanes of a voxel leave together
    SlVoxel<CPL, L, VEC> v;
    v.load(x, target, mask, g, n, r, c0);
    bad |= v.bad;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      const float p = v.p[j], t = v.t[j];
      acc[j][0] += p * t;
      acc[j][1] += p;
      acc[j][2] += p * p;
      acc[j][3] += t;
      acc[j][4] += t * t;
      acc[j][5] += v.valid * (t * v.nlogp[j]);
      acc[j][6] += v.valid * v.nlogp[j];
      acc[j][7] += v.valid * t;
    }
  }
  if (bad) {
#pragma unroll
    for (int j = 0; j < CPL; ++j) acc[j][5] = NAN;
  }
  // lanes of one sub-index across the wave, then the waves in order
  const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
#pragma unroll
  for (int j = 0; j < CPL; ++j)
#pragma unroll
    for (int k = 0; k < SL_COLS; ++k) {
      float a = acc[j][k];
#pragma unroll
      for (int o = L; o < WAVE; o <<= 1) a += __shfl_xor(a, o, WAVE);
      if (lane < L) red[wave][(sub * CPL + j) * SL_COLS + k] = a;
    }
  __syncthreads();
  for (int i = threadIdx.x; i < L * CPL * SL_COLS; i += SL_THREADS) {
    const int c = i / SL_COLS;
    if (c < g.C) {
      float a = red[0][i];
#pragma unroll
      for (int w = 1; w < NW; ++w) a += red[w][i];
      partial[(((long)n * g.tiles + blockIdx.x) * g.C + c) * SL_COLS + (i - c * SL_COLS)] = a;
    }
  }
}

// sums[n][c][k] = the tiles of sample n: one wave per (n, c, k); lane l adds tiles l, l + 64, ... in order, then a fixed shuffle tree
__global__ void __launch_bounds__(SL_THREADS) softmax_loss_sum_kernel(const float* __restrict__ partial, float* __restrict__ sums, int N,
                                                                      int row, int tiles) {
  const long i = (long)blockIdx.x * (SL_THREADS / WAVE) + threadIdx.x / WAVE;
  if (i >= (long)N * row) return;                        // the whole wave leaves together
  const int lane = threadIdx.x % WAVE;
  const long n = i / row, e = i - n * row;
  float a = 0.f;
  for (int tl = lane; tl < tiles; tl += WAVE) a += partial[(n * tiles + tl) * row + e];
#pragma unroll
  for (int o = WAVE / 2; o > 0; o >>= 1) a += __shfl_xor(a, o, WAVE);
  if (lane == 0) sums[i] = a;
}

template <int CPL, int L, bool VEC>
__global__ void __launch_bounds__(SL_THREADS) softmax_loss_backward_kernel(const float* __restrict__ x, const void* __restrict__ target,
                                                                           const float* __restrict__ mask,
                                                                           const float* __restrict__ gsums, float* __restrict__ dx,
                                                                           SlGeo g) {
  constexpr int VOX = SL_THREADS / L;
  const int n = blockIdx.y, sub = threadIdx.x % L, c0 = sub * CPL;
  const long base = (long)blockIdx.x * SL_TILE + threadIdx.x / L;
  float g0[CPL], g1[CPL], g2[CPL], g5[CPL], g6[CPL];
#pragma unroll
  for (int j = 0; j < CPL; ++j) {
    const bool in = c0 + j < g.C;
    const float* gs = gsums + ((long)n * g.C + (in ? c0 + j : 0)) * SL_COLS;
    g0[j] = in ? gs[0] : 0.f;
    g1[j] = in ? gs[1] : 0.f;
    g2[j] = in ? 2.f * gs[2] : 0.f;
    g5[j] = in ? gs[5] : 0.f;
    g6[j] = in ? gs[6] : 0.f;
  }
  for (int it = 0; it < SL_TILE / VOX; ++it) {
    const long r = base + (long)it * VOX;
    if (r >= g.R) break;
    SlVoxel<CPL, L, VEC> v;
    v.load(x, target, mask, g, n, r, c0);
    float u[CPL], h[CPL], A = 0.f, H = 0.f;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      u[j] = g0[j] * v.t[j] + g1[j] + g2[j] * v.p[j];
      h[j] = v.valid * (g5[j] * v.t[j] + g6[j]);
      A += v.p[j] * u[j];                                // p = 0, u = 0, h = 0 beyond C
      H += h[j];
    }
    A = sl_lane_sum<L>(A);
    H = sl_lane_sum<L>(H);
    float d[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) d[j] = v.live[j] ? v.p[j] * (u[j] - A) + (v.p[j] * H - h[j]) : 0.f;
    float* pd = dx + n * g.ds[0] + r * g.ds[2];
#pragma unroll
    for (int q = 0; q < CPL; q += 4) {
      if (VEC && CPL >= 4 && c0 + q + 4 <= g.C) {
        f32x4_t o;
#pragma unroll
        for (int j = 0; j < 4 && q + j < CPL; ++j) o[j] = d[q + j];
        *reinterpret_cast<f32x4_t*>(pd + c0 + q) = o;
      } else {
#pragma unroll
        for (int j = 0; j < 4 && q + j < CPL; ++j)
          if (c0 + q + j < g.C) pd[(c0 + q + j) * g.ds[1]] = d[q + j];
      }
    }
  }
}

static bool sl_vec_ok(const float* p, const long* s) {
  return p == nullptr || ((reinterpret_cast<uintptr_t>(p) & 15) == 0 && s[1] == 1 && s[0] % 4 == 0 && s[2] % 4 == 0);
}

static int sl_geo(const char* what, const float* x, const void* target, const float* mask, int N, int C, long R, const int64_t* xs,
                  const int64_t* ts, const int64_t* ms, const int64_t* ds, int target_kind, long ignore_index, float fill, SlGeo& g) {
  PYTC_REQUIRE(N >= 1 && C >= 1 && R >= 1, "%s: bad shape N %d, C %d, R %ld", what, N, C, R);
  if (C < 2 || C > SL_MAX_C) {
    set_error("%s: C = %d; the softmax-loss kernels cover 2 <= C <= %d", what, C, SL_MAX_C);
    return PYTC_ERR_UNSUPPORTED;
  }
  PYTC_REQUIRE(x && target && xs && ts, "%s: x, target and their strides are required", what);
  PYTC_REQUIRE(!mask || ms, "%s: a mask needs its strides", what);
  PYTC_REQUIRE(target_kind >= 0 && target_kind <= 2, "%s: unknown target_kind %d", what, target_kind);
  PYTC_REQUIRE(N <= 65535, "%s: %d samples", what, N);
  PYTC_REQUIRE((R + SL_TILE - 1) / SL_TILE <= 0x7fffffffL, "%s: %ld voxels per sample", what, R);
  g.R = R;
  g.C = C;
  g.tiles = ceil_div(R, SL_TILE);
  for (int i = 0; i < 3; ++i) {
    g.xs[i] = xs[i];
    g.ts[i] = ts[i];
    g.ms[i] = mask ? ms[i] : 0;
    g.ds[i] = ds ? ds[i] : 0;
    PYTC_REQUIRE(g.xs[i] >= 0 && g.ts[i] >= 0 && g.ms[i] >= 0 && g.ds[i] >= 0, "%s: negative stride", what);
  }
  g.target_kind = target_kind;
  g.ignore_index = ignore_index;
  g.fill = fill;
  return PYTC_OK;
}

}  // namespace pytc

using namespace pytc;

extern "C" int pytc_softmax_loss_tiles(int64_t R) { return R >= 1 ? ceil_div((long)R, SL_TILE) : 0; }

#define SL_LAUNCH(KERNEL, CPL, L, grid, ...)                                                                  \
  do {                                                                                                        \
    if (vec)                                                                                                  \
      hipLaunchKernelGGL((KERNEL<CPL, L, true>), grid, dim3(SL_THREADS), 0, st, __VA_ARGS__);                 \
    else                                                                                                      \
      hipLaunchKernelGGL((KERNEL<CPL, L, false>), grid, dim3(SL_THREADS), 0, st, __VA_ARGS__);                \
  } while (0)

#define SL_DISPATCH(KERNEL, grid, ...)                     \
  do {                                                     \
    if (C <= 2)                                            \
      SL_LAUNCH(KERNEL, 2, 1, grid, __VA_ARGS__);          \
    else if (C <= 4)                                       \
      SL_LAUNCH(KERNEL, 4, 1, grid, __VA_ARGS__);          \
    else if (C <= 8)                                       \
      SL_LAUNCH(KERNEL, 8, 1, grid, __VA_ARGS__);          \
    else if (C <= 16)                                      \
      SL_LAUNCH(KERNEL, 8, 2, grid, __VA_ARGS__);          \
    else                                                   \
      SL_LAUNCH(KERNEL, 8, 4, grid, __VA_ARGS__);          \
  } while (0)

extern "C" int pytc_softmax_loss_forward(const float* x, const void* target, const float* mask, float* partial, float* sums, int N, int C,
                                         int64_t R, const int64_t* x_strides, const int64_t* t_strides, const int64_t* m_strides,
                                         int target_kind, int64_t ignore_index, float fill, void* stream) {
  SlGeo g;
  if (int s = sl_geo("softmax_loss_forward", x, target, mask, N, C, (long)R, x_strides, t_strides, m_strides, nullptr, target_kind,
                     (long)ignore_index, fill, g))
    return s;
  PYTC_REQUIRE(partial && sums, "softmax_loss_forward: partial and sums are required");
  const bool vec = C >= 4 && sl_vec_ok(x, g.xs);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(g.tiles, N);
  SL_DISPATCH(softmax_loss_forward_kernel, grid, x, target, mask, partial, g);
  PYTC_LAUNCH_CHECK("softmax_loss_forward");
  const int row = C * SL_COLS;
  hipLaunchKernelGGL(softmax_loss_sum_kernel, dim3(ceil_div((long)N * row, SL_THREADS / WAVE)), dim3(SL_THREADS), 0, st, partial, sums, N, row,
                     g.tiles);
  PYTC_LAUNCH_CHECK("softmax_loss_forward_sum");
  return PYTC_OK;
}

extern "C" int pytc_softmax_loss_backward(const float* x, const void* target, const float* mask, const float* gsums, float* dx, int N,
                                          int C, int64_t R, const int64_t* x_strides, const int64_t* t_strides, const int64_t* m_strides,
                                          const int64_t* d_strides, int target_kind, int64_t ignore_index, float fill, void* stream) {
  SlGeo g;
  PYTC_REQUIRE(d_strides != nullptr, "softmax_loss_backward: dx needs its strides");
  if (int s = sl_geo("softmax_loss_backward", x, target, mask, N, C, (long)R, x_strides, t_strides, m_strides, d_strides, target_kind,
                     (long)ignore_index, fill, g))
    return s;
  PYTC_REQUIRE(gsums && dx && dx != x, "softmax_loss_backward: null or aliased pointer");
  PYTC_REQUIRE(g.ds[1] >= 1 && g.ds[2] >= 1 && g.ds[0] >= 1, "softmax_loss_backward: dx may not broadcast");
  const bool vec = C >= 4 && sl_vec_ok(x, g.xs) && sl_vec_ok(dx, g.ds);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(g.tiles, N);
  SL_DISPATCH(softmax_loss_backward_kernel, grid, x, target, mask, gsums, dx, g);
  PYTC_LAUNCH_CHECK("softmax_loss_backward");
  return PYTC_OK;
}
