// Soft skeleton of the clDice topology loss on the MI355X: the iterated soft erosion, the skeleton chain with its weighted sums, and
// the reverse sweep of its gradient -- for 5-D (N, C, D, H, W) and 4-D (N, C, H, W) fp32 volumes, any number of iterations.
//
// Reference: connectomics/models/losses/losses.py:47-85 (_soft_erode_pool, _soft_dilate_pool, _soft_open_pool,
// _soft_skeletonize_pool) and :456-721 (SoftClDiceLoss).  With p_0 the probability volume and E the soft erosion,
//   p_{j+1} = E(p_j)                      E = min(min(minpool_d, minpool_h), minpool_w)  (2-D: min(minpool_h, minpool_w))
//   d_j = relu(p_j - Dil(p_{j+1}))        Dil = 3^3 max-pool (2-D: 3^2), the opening of p_j is Dil(E(p_j)) = Dil(p_{j+1})
//   s_0 = d_0,  s_j = s_{j-1} + relu(d_j - s_{j-1} d_j)            j = 1 .. n, the skeleton is s_n
// The reference evaluates E 2n + 1 times; here every p_j is computed once (pytc_cldice_erode, n + 1 launches) and kept.
//
// Rounding: every product and difference is rounded on its own, as torch's eager ops do (no contraction into FMAs), and the
// pools select values, so the skeleton is bit-identical to the reference's.
//
// Gradient: torch autograd's routing on ties, in gather form (each voxel collects from the voxels that selected it, in a fixed
// order; no atomics): a max-pool sends the whole gradient to the first maximum of its window in scan order (d, h, w), padding
// never selected; torch.minimum splits a tie in halves; relu passes where its result is > 0.  The chain kernel recomputes d_j
// and the first-max position of every dilation window (one byte per voxel and level) and turns dL/ds_n into the gradient of each
// relu(p_j - Dil(p_{j+1})); the sweep then walks j = n + 1 .. 0, collecting at p_j the direct term, the dilation of level j - 1
// and the erosion into p_{j+1}.  Sums of the loss are per-tile partials reduced in a fixed order.
#include <algorithm>

#include "pytc_common.h"

#pragma clang fp contract(off)

namespace pytc {

constexpr int CLD_THREADS = 256;
constexpr int CLD_TILE = 1024;          // voxels of one volume per block of the skeleton kernel (4 per thread)

struct CldGeo {
  int D, H, W;
  long V;                               // D H W
  int is2d;
};

__device__ __forceinline__ float cld_relu(float x) { return x > 0.f ? x : 0.f; }

// first minimum of the 3-window along one axis (scan order c - 1, c, c + 1, out-of-range taps skipped): value and offset
__device__ __forceinline__ float axis_min(const float* __restrict__ p, long u, int c, int L, long st, int& off) {
  float best;
  if (c > 0) {
    best = p[u - st];
    off = -1;
    const float v = p[u];
    if (v < best) { best = v; off = 0; }
  } else {
    best = p[u];
    off = 0;
  }
  if (c + 1 < L) {
    const float v = p[u + st];
    if (v < best) { best = v; off = 1; }
  }
  return best;
}

// soft erosion at voxel u = (z, y, x) of one volume; m[3] = the axis minima (m[0] unused in 2-D), o[3] their offsets
__device__ __forceinline__ float erode_at(const float* __restrict__ p, long u, int z, int y, int x, const CldGeo& g, float (&m)[3],
                                          int (&o)[3]) {
  m[1] = axis_min(p, u, y, g.H, g.W, o[1]);
  m[2] = axis_min(p, u, x, g.W, 1, o[2]);
  if (g.is2d) {
    o[0] = 0;
    m[0] = m[1];
    return m[1] < m[2] ? m[1] : m[2];
  }
  m[0] = axis_min(p, u, z, g.D, (long)g.H * g.W, o[0]);
  const float q = m[0] < m[1] ? m[0] : m[1];
  return q < m[2] ? q : m[2];
}

// d(erosion)/d(axis minimum) under torch.minimum's tie rule: c[i] in {0, 1/4, 1/2, 1}
__device__ __forceinline__ void erode_coef(const float (&m)[3], int is2d, float (&c)[3]) {
  auto share = [](float a, float b) { return a < b ? 1.f : (a == b ? 0.5f : 0.f); };
  if (is2d) {
    c[0] = 0.f;
    c[1] = share(m[1], m[2]);
    c[2] = share(m[2], m[1]);
    return;
  }
  const float q = m[0] < m[1] ? m[0] : m[1];
  const float cq = share(q, m[2]);
  c[0] = cq * share(m[0], m[1]);
  c[1] = cq * share(m[1], m[0]);
  c[2] = share(m[2], q);
}

// 3^3 (2-D: 3^2) max-pool at voxel u with the first maximum's window code (dz + 1) 9 + (dy + 1) 3 + (dx + 1)
__device__ __forceinline__ float dilate_at(const float* __restrict__ p, long u, int z, int y, int x, const CldGeo& g, int& code) {
  float best = 0.f;
  code = -1;
  const long sz = (long)g.H * g.W;
  for (int dz = -1; dz <= 1; ++dz) {
    if (z + dz < 0 || z + dz >= g.D) continue;
    for (int dy = -1; dy <= 1; ++dy) {
      if (y + dy < 0 || y + dy >= g.H) continue;
      for (int dx = -1; dx <= 1; ++dx) {
        if (x + dx < 0 || x + dx >= g.W) continue;
        const float v = p[u + dz * sz + dy * (long)g.W + dx];
        if (code < 0 || v > best) {
          best = v;
          code = (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1);
        }
      }
    }
  }
  return best;
}

__device__ __forceinline__ void cld_coords(int i, const CldGeo& g, int& z, int& y, int& x) {
  x = i % g.W;
  const int r = i / g.W;
  y = r % g.H;
  z = r / g.H;
}

__device__ __forceinline__ const float* level(const float* p0, const float* P, int j, long total) {
  return j == 0 ? p0 : P + (long)(j - 1) * total;
}

// dst = E(src) over nvol volumes
__global__ void __launch_bounds__(CLD_THREADS) cldice_erode_kernel(const float* __restrict__ src, float* __restrict__ dst, CldGeo g,
                                                                   long total) {
  const int i = blockIdx.x * CLD_THREADS + threadIdx.x, vol = blockIdx.y;
  if (i >= g.V) return;
  const long t = (long)vol * g.V + i;
  int z, y, x;
  cld_coords(i, g, z, y, x);
  float m[3];
  int o[3];
  dst[t] = erode_at(src, t, z, y, x, g, m, o);
}

// skeleton s_n of every voxel (written when skel is non-null) and, when other is non-null, the tile partials
//   partial[(vol tiles + tile) 2 + 0] = sum (s w)(other w),   [.. + 1] = sum s w        (w = 1 when weight is null)
__global__ void __launch_bounds__(CLD_THREADS) cldice_skeleton_kernel(const float* __restrict__ p0, const float* __restrict__ P,
                                                                      float* __restrict__ skel, const float* __restrict__ other,
                                                                      const float* __restrict__ weight, float* __restrict__ partial,
                                                                      CldGeo g, long total, int n, int tiles) {
  __shared__ float red[CLD_THREADS];
  const int vol = blockIdx.y, tile = blockIdx.x;
  float acc0 = 0.f, acc1 = 0.f;
  for (int k = 0; k < CLD_TILE / CLD_THREADS; ++k) {
    const int i = tile * CLD_TILE + k * CLD_THREADS + threadIdx.x;
    if (i >= g.V) break;
    const long t = (long)vol * g.V + i;
    int z, y, x, code;
    cld_coords(i, g, z, y, x);
    float s = 0.f;
    for (int j = 0; j <= n; ++j) {
      const float o = dilate_at(level(p0, P, j + 1, total), t, z, y, x, g, code);
      const float d = cld_relu(level(p0, P, j, total)[t] - o);
      if (j == 0) {
        s = d;
      } else {
        const float sd = s * d;
        s = s + cld_relu(d - sd);
      }
    }
    if (skel) skel[t] = s;
    if (other) {
      const float w = weight ? weight[t] : 1.f;
      const float se = weight ? s * w : s;
      const float oe = weight ? other[t] * w : other[t];
      acc0 += se * oe;
      acc1 += se;
    }
  }
  if (!other) return;
  acc0 = block_sum<CLD_THREADS>(acc0, red);
  acc1 = block_sum<CLD_THREADS>(acc1, red);
  if (threadIdx.x == 0) {
    partial[((long)vol * tiles + tile) * 2 + 0] = acc0;
    partial[((long)vol * tiles + tile) * 2 + 1] = acc1;
  }
}

// sums[vol 2 + k] = the tile partials of vol, in a fixed order
__global__ void __launch_bounds__(CLD_THREADS) cldice_sum_kernel(const float* __restrict__ partial, float* __restrict__ sums, int tiles) {
  __shared__ float red[CLD_THREADS];
  const int vol = blockIdx.x;
  float a0 = 0.f, a1 = 0.f;
  for (int t = threadIdx.x; t < tiles; t += CLD_THREADS) {
    a0 += partial[((long)vol * tiles + t) * 2 + 0];
    a1 += partial[((long)vol * tiles + t) * 2 + 1];
  }
  a0 = block_sum<CLD_THREADS>(a0, red);
  a1 = block_sum<CLD_THREADS>(a1, red);
  if (threadIdx.x == 0) {
    sums[vol * 2 + 0] = a0;
    sums[vol * 2 + 1] = a1;
  }
}

// Backward, step 1.  g_n = dL/ds_n = (alpha (t w) + beta) w per voxel, alpha / beta per volume (coef[vol], coef[nvol + vol]).
// Writes gdiff[j] = dL/d(p_j - Dil(p_{j+1})) through relu, and arg[j] = the first-max code of the dilation window, j = 0 .. n.
// gdiff[j] holds d_j until the backward chain overwrites it (s_{j-1} is recomputed from d_0 .. d_{j-1}).
__global__ void __launch_bounds__(CLD_THREADS) cldice_chain_bwd_kernel(const float* __restrict__ p0, const float* __restrict__ P,
                                                                       const float* __restrict__ target, const float* __restrict__ weight,
                                                                       const float* __restrict__ coef, float* __restrict__ gdiff,
                                                                       unsigned char* __restrict__ arg, CldGeo g, long total, int nvol,
                                                                       int n) {
  const int i = blockIdx.x * CLD_THREADS + threadIdx.x, vol = blockIdx.y;
  if (i >= g.V) return;
  const long t = (long)vol * g.V + i;
  int z, y, x, code;
  cld_coords(i, g, z, y, x);
  for (int j = 0; j <= n; ++j) {
    const float o = dilate_at(level(p0, P, j + 1, total), t, z, y, x, g, code);
    gdiff[(long)j * total + t] = cld_relu(level(p0, P, j, total)[t] - o);
    arg[(long)j * total + t] = (unsigned char)code;
  }
  const float w = weight ? weight[t] : 1.f;
  const float te = weight ? target[t] * w : target[t];
  float gs = (coef[vol] * te + coef[nvol + vol]) * w;
  for (int j = n; j >= 1; --j) {
    float s = gdiff[t];                                         // s_{j-1} from d_0 .. d_{j-1}
    for (int k = 1; k < j; ++k) {
      const float d = gdiff[(long)k * total + t];
      const float sd = s * d;
      s = s + cld_relu(d - sd);
    }
    const float d = gdiff[(long)j * total + t];
    const float sd = s * d;
    const float gu = (d - sd) > 0.f ? gs : 0.f;                 // relu(d - s d)
    const float gd = gu + (-gu) * s;                            // d (d - s d) / d d
    gs = gs + (-gu) * d;                                        // the add's identity path + d (d - s d) / d s
    gdiff[(long)j * total + t] = d > 0.f ? gd : 0.f;            // relu(p_j - o_j)
  }
  const float d0 = gdiff[t];
  gdiff[t] = d0 > 0.f ? gs : 0.f;
}

// Backward, step 2 (one launch per level j = n + 1 .. 0):
//   a_j = [j <= n] gdiff_j + [j >= 1] sum over the dilation windows of level j - 1 whose first max is this voxel of -gdiff_{j-1}
//       + [j <= n] sum over the erosion windows at p_j that selected this voxel of (tie share) a_{j+1}
// and at j = 0 also gamma (s_t w) w (gamma per volume at coef[2 nvol + vol]; skipped when skel_t is null).
__global__ void __launch_bounds__(CLD_THREADS) cldice_sweep_kernel(const float* __restrict__ p0, const float* __restrict__ P,
                                                                   const float* __restrict__ gdiff, const unsigned char* __restrict__ arg,
                                                                   const float* __restrict__ a_next, float* __restrict__ a_out,
                                                                   const float* __restrict__ skel_t, const float* __restrict__ weight,
                                                                   const float* __restrict__ coef, CldGeo g, long total, int nvol, int n,
                                                                   int j) {
  const int i = blockIdx.x * CLD_THREADS + threadIdx.x, vol = blockIdx.y;
  if (i >= g.V) return;
  const long t = (long)vol * g.V + i;
  int z, y, x;
  cld_coords(i, g, z, y, x);
  const long sz = (long)g.H * g.W;
  float acc = j <= n ? gdiff[(long)j * total + t] : 0.f;
  if (j >= 1) {
    const float* gd = gdiff + (long)(j - 1) * total;
    const unsigned char* ag = arg + (long)(j - 1) * total;
    for (int dz = -1; dz <= 1; ++dz) {
      if (z + dz < 0 || z + dz >= g.D) continue;
      for (int dy = -1; dy <= 1; ++dy) {
        if (y + dy < 0 || y + dy >= g.H) continue;
        for (int dx = -1; dx <= 1; ++dx) {
          if (x + dx < 0 || x + dx >= g.W) continue;
          const long u = t + dz * sz + dy * (long)g.W + dx;
          if (ag[u] == (1 - dz) * 9 + (1 - dy) * 3 + (1 - dx)) acc += -gd[u];      // u's window max sits at u - (dz, dy, dx)
        }
      }
    }
  }
  if (j <= n) {
    const float* p = level(p0, P, j, total);
    float m[3], c[3];
    int o[3];
    // u = this voxel: every axis whose minimum sits at offset 0
    erode_at(p, t, z, y, x, g, m, o);
    erode_coef(m, g.is2d, c);
    float e = 0.f;
    for (int a = g.is2d ? 1 : 0; a < 3; ++a)
      if (o[a] == 0) e += c[a];
    acc += e * a_next[t];
    // u = this voxel -/+ one step along an axis: that axis's minimum must sit at offset +/-1
    const int lo = g.is2d ? 1 : 0;
    for (int a = lo; a < 3; ++a) {
      const int cc = a == 0 ? z : (a == 1 ? y : x);
      const int L = a == 0 ? g.D : (a == 1 ? g.H : g.W);
      const long st = a == 0 ? sz : (a == 1 ? (long)g.W : 1);
      for (int s = -1; s <= 1; s += 2) {
        if (cc + s < 0 || cc + s >= L) continue;
        const long u = t + s * st;
        const int uz = a == 0 ? z + s : z, uy = a == 1 ? y + s : y, ux = a == 2 ? x + s : x;
        erode_at(p, u, uz, uy, ux, g, m, o);
        if (o[a] != -s) continue;
        erode_coef(m, g.is2d, c);
        acc += c[a] * a_next[u];
      }
    }
  }
  if (j == 0 && skel_t) {
    const float w = weight ? weight[t] : 1.f;
    const float se = weight ? skel_t[t] * w : skel_t[t];
    acc += coef[2 * nvol + vol] * se * w;
  }
  a_out[t] = acc;
}

static int cld_geo(const char* what, int nvol, int D, int H, int W, int is2d, CldGeo& g, long& total) {
  PYTC_REQUIRE(nvol >= 1 && nvol <= 65535 && D >= 1 && H >= 1 && W >= 1, "%s: bad shape nvol %d, (%d, %d, %d)", what, nvol, D, H, W);
  PYTC_REQUIRE(!is2d || D == 1, "%s: a 2-D volume has D = 1, got %d", what, D);
  g.D = D;
  g.H = H;
  g.W = W;
  g.V = (long)D * H * W;
  g.is2d = is2d ? 1 : 0;
  total = g.V * nvol;
  PYTC_REQUIRE(g.V <= 0x7fffffffL - CLD_TILE, "%s: %ld voxels per volume", what, g.V);
  return PYTC_OK;
}

}  // namespace pytc

using namespace pytc;

extern "C" int pytc_cldice_tiles(int64_t voxels) { return ceil_div((long)voxels, CLD_TILE); }

extern "C" int pytc_cldice_erode(const float* src, float* dst, int nvol, int D, int H, int W, int is2d, void* stream) {
  CldGeo g;
  long total;
  if (int s = cld_geo("cldice_erode", nvol, D, H, W, is2d, g, total)) return s;
  PYTC_REQUIRE(src && dst && src != dst, "cldice_erode: null or aliased pointer");
  hipLaunchKernelGGL(cldice_erode_kernel, dim3(ceil_div(g.V, CLD_THREADS), nvol), dim3(CLD_THREADS), 0, (hipStream_t)stream, src, dst, g,
                     total);
  PYTC_LAUNCH_CHECK("cldice_erode");
  return PYTC_OK;
}

extern "C" int pytc_cldice_skeleton(const float* p0, const float* P, float* skel, const float* other, const float* weight,
                                    float* partial, float* sums, int nvol, int D, int H, int W, int n_iters, int is2d, void* stream) {
  CldGeo g;
  long total;
  if (int s = cld_geo("cldice_skeleton", nvol, D, H, W, is2d, g, total)) return s;
  PYTC_REQUIRE(n_iters >= 0 && p0 && P, "cldice_skeleton: n_iters %d, p0 and P (n_iters + 1 eroded levels) are required", n_iters);
  PYTC_REQUIRE(skel || other, "cldice_skeleton: nothing to write");
  PYTC_REQUIRE(!other || (partial && sums), "cldice_skeleton: sums need the partial workspace");
  const int tiles = ceil_div(g.V, CLD_TILE);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(cldice_skeleton_kernel, dim3(tiles, nvol), dim3(CLD_THREADS), 0, st, p0, P, skel, other, weight, partial, g, total,
                     n_iters, tiles);
  PYTC_LAUNCH_CHECK("cldice_skeleton");
  if (other) {
    hipLaunchKernelGGL(cldice_sum_kernel, dim3(nvol), dim3(CLD_THREADS), 0, st, partial, sums, tiles);
    PYTC_LAUNCH_CHECK("cldice_skeleton_sum");
  }
  return PYTC_OK;
}

extern "C" int pytc_cldice_chain_bwd(const float* p0, const float* P, const float* target, const float* weight, const float* coef,
                                     float* gdiff, uint8_t* arg, int nvol, int D, int H, int W, int n_iters, int is2d, void* stream) {
  CldGeo g;
  long total;
  if (int s = cld_geo("cldice_chain_bwd", nvol, D, H, W, is2d, g, total)) return s;
  PYTC_REQUIRE(n_iters >= 0 && p0 && P && target && coef && gdiff && arg, "cldice_chain_bwd: null pointer");
  hipLaunchKernelGGL(cldice_chain_bwd_kernel, dim3(ceil_div(g.V, CLD_THREADS), nvol), dim3(CLD_THREADS), 0, (hipStream_t)stream, p0, P,
                     target, weight, coef, gdiff, arg, g, total, nvol, n_iters);
  PYTC_LAUNCH_CHECK("cldice_chain_bwd");
  return PYTC_OK;
}

extern "C" int pytc_cldice_sweep_bwd(const float* p0, const float* P, const float* gdiff, const uint8_t* arg, const float* a_next,
                                     float* a_out, const float* skel_t, const float* weight, const float* coef, int nvol, int D, int H,
                                     int W, int n_iters, int level, int is2d, void* stream) {
  CldGeo g;
  long total;
  if (int s = cld_geo("cldice_sweep_bwd", nvol, D, H, W, is2d, g, total)) return s;
  PYTC_REQUIRE(n_iters >= 0 && level >= 0 && level <= n_iters + 1, "cldice_sweep_bwd: level %d of %d", level, n_iters + 1);
  PYTC_REQUIRE(p0 && P && gdiff && arg && a_out && coef && (level > n_iters || (a_next && a_next != a_out)),
               "cldice_sweep_bwd: null or aliased pointer");
  hipLaunchKernelGGL(cldice_sweep_kernel, dim3(ceil_div(g.V, CLD_THREADS), nvol), dim3(CLD_THREADS), 0, (hipStream_t)stream, p0, P, gdiff,
                     arg, a_next, a_out, skel_t, weight, coef, g, total, nvol, n_iters, level);
  PYTC_LAUNCH_CHECK("cldice_sweep_bwd");
  return PYTC_OK;
}
