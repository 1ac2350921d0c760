// The regularisation losses of connectomics/models/losses/regularization.py on the MI355X: BinaryRegularization,
// ForegroundDistanceConsistency, ContourDistanceConsistency, NonOverlapRegularization (a streaming pair: one sum forward, every
// operand's gradient backward) and ForegroundContourConsistency (a stencil pair).  fp32, contiguous, nothing saved between forward
// and backward but the one-byte code map of the stencil pair; every sum comes from fixed-order partials (no atomics).
//
// Streaming pair.  A workgroup of 256 threads takes RG_TILE = 4096 consecutive voxels of one volume (sample, channel): four 16-byte
// vectors per thread and operand when V % 4 == 0 and every pointer is 16-byte aligned (then every volume starts on a vector), else
// sixteen coalesced scalars.  Per voxel (s = sigmoid, t = tanh b, sp = softplus):
//   BINARY      d = |s(a) - 0.5| = 0.5 tanh(|a| / 2) = -0.5 em / (2 + em) with em = expm1(-|a|): no cancellation near a = 0, where
//               the loss 1 / max(d, thr) and its gradient -sign(a) s (1 - s) / d^2 (0 where d < thr) are largest.
//   FG_DIST     sp(-a) max(t, 0) + sp(a) max(-t, 0); d/da = -s(-a) max(t, 0) + s(a) max(-t, 0), d/db = (1 - t^2) ([t >= 0] sp(-a) -
//               [t <= 0] sp(a)) (both clamps pass at t = 0, as torch's do).
//   CT_DIST     u^2, u = s(a) |t|; d/da = 2 u |t| s(a) s(-a), d/db = 2 u s(a) sign(t) (1 - t^2).
//   NONOVERLAP  s(a0) s(a1) [s(a2)] on channels 0, 1 [, 2] of one (N, C, V) tensor; the gradient is written for all C channels, zero
//               outside channels 0 and 1 (a2 is detached in the reference).
// The mask (nullable) has C channels or one; the one-channel mask is indexed per sample inside the kernel.
//
// Stencil pair.  Tile = 32 x 64 voxels (y, x) of one z-plane; sigmoid(fg) is staged in LDS with a halo (rows of 72 floats: 4 columns
// left and right of the tile), the clamped edge magnitude e is formed in LDS from it and pooled from LDS.  Forward: halo 2 (e at
// halo 1).  Backward: the pooled output o needs e at its code position, the edge voxel u gathers from the outputs o of its 3 x 3
// window whose code names u, the voxel v gathers from the edge voxels v +- 1 along x and y: halo 4 of sigmoid(fg), 3 of e, 2 of the
// per-output factor G = coef mask 2 (E - s(contour)), 1 of the edge gradients.  All arrays share one (row, column) indexing.
#include <algorithm>

#include "pytc_common.h"

#pragma clang fp contract(off)

namespace pytc {

constexpr int RG_THREADS = 256;
constexpr int RG_PER_THREAD = 16;
constexpr int RG_TILE = RG_THREADS * RG_PER_THREAD;      // 4096 voxels per workgroup: also the voxels per partial of pytc_reg_tiles

struct RgGeo {
  long V;
  int C, wC;
  float param;
  int flag;
};

// s = sigmoid(x), sc = sigmoid(-x), both without cancellation
__device__ __forceinline__ void rg_sig2(float x, float& s, float& sc) {
  const float e = expf(-fabsf(x));
  const float big = 1.f / (1.f + e), small = e * big;
  s = x >= 0.f ? big : small;
  sc = x >= 0.f ? small : big;
}

__device__ __forceinline__ float rg_sigmoid(float x) {
  float s, sc;
  rg_sig2(x, s, sc);
  return s;
}

// d = |p - 0.5|, sgn = sign(p - 0.5), ps = dp / da of BinaryRegularization
__device__ __forceinline__ void rg_binary_terms(float a, int apply_sigmoid, float& d, float& sgn, float& ps) {
  if (apply_sigmoid) {
    const float em = expm1f(-fabsf(a)), den = 2.f + em;
    d = -0.5f * em / den;
    ps = (1.f + em) / (den * den);
    sgn = a > 0.f ? 1.f : (a < 0.f ? -1.f : 0.f);
  } else {
    const float c = a - 0.5f;
    d = fabsf(c);
    ps = 1.f;
    sgn = c > 0.f ? 1.f : (c < 0.f ? -1.f : 0.f);
  }
}

template <int KIND>
__device__ __forceinline__ float rg_loss(float a, float b, float c, bool has_c, const RgGeo& g) {
  if (KIND == PYTC_REG_BINARY) {
    float d, sgn, ps;
    rg_binary_terms(a, g.flag, d, sgn, ps);
    return 1.f / fmaxf(d, g.param);
  } else if (KIND == PYTC_REG_FG_DIST) {
    const float t = tanhf(b), l = log1pf(expf(-fabsf(a)));
    const float spn = fmaxf(-a, 0.f) + l, spp = fmaxf(a, 0.f) + l;
    return spn * fmaxf(t, 0.f) + spp * fmaxf(-t, 0.f);
  } else if (KIND == PYTC_REG_CT_DIST) {
    const float u = rg_sigmoid(a) * fabsf(tanhf(b));
    return u * u;
  } else {
    float l = rg_sigmoid(a) * rg_sigmoid(b);
    if (has_c) l = l * rg_sigmoid(c);
    return l;
  }
}

// the gradients of one voxel's loss in a and b, times gm (= coef x mask)
template <int KIND>
__device__ __forceinline__ void rg_grad(float a, float b, float c, bool has_c, const RgGeo& g, float gm, float& da, float& db) {
  if (KIND == PYTC_REG_BINARY) {
    float d, sgn, ps;
    rg_binary_terms(a, g.flag, d, sgn, ps);
    da = d >= g.param ? gm * (-sgn * ps / (d * d)) : 0.f;
    db = 0.f;
  } else if (KIND == PYTC_REG_FG_DIST) {
    const float t = tanhf(b), e = expf(-fabsf(a)), l = log1pf(e);
    const float spn = fmaxf(-a, 0.f) + l, spp = fmaxf(a, 0.f) + l;
    const float big = 1.f / (1.f + e), small = e * big;
    const float s = a >= 0.f ? big : small, sc = a >= 0.f ? small : big;
    da = gm * (s * fmaxf(-t, 0.f) - sc * fmaxf(t, 0.f));
    db = gm * ((1.f - t * t) * ((t >= 0.f ? spn : 0.f) - (t <= 0.f ? spp : 0.f)));
  } else if (KIND == PYTC_REG_CT_DIST) {
    float s, sc;
    rg_sig2(a, s, sc);
    const float t = tanhf(b), at = fabsf(t), u = s * at;
    const float sgn = t > 0.f ? 1.f : (t < 0.f ? -1.f : 0.f);
    da = gm * (2.f * u * at * (s * sc));
    db = gm * (2.f * u * s * sgn * (1.f - t * t));
  } else {
    float s0, c0, s1, c1;
    rg_sig2(a, s0, c0);
    rg_sig2(b, s1, c1);
    const float s2 = has_c ? rg_sigmoid(c) : 1.f;
    da = gm * (s1 * s2 * (s0 * c0));
    db = gm * (s0 * s2 * (s1 * c1));
  }
}

// the operand rows of one volume: a, b, c (NONOVERLAP: channels 0, 1, 2 of sample `vol`) and the mask row
template <int KIND>
__device__ __forceinline__ void rg_rows(const float* a, const float* b, const float* mask, int vol, const RgGeo& g, const float*& pa,
                                        const float*& pb, const float*& pc, const float*& pm) {
  pb = pc = pm = nullptr;
  if (KIND == PYTC_REG_NONOVERLAP) {
    pa = a + (long)vol * g.C * g.V;
    pb = pa + g.V;
    if (g.flag && g.C >= 3) pc = pa + 2 * g.V;
  } else {
    pa = a + (long)vol * g.V;
    if (KIND != PYTC_REG_BINARY) pb = b + (long)vol * g.V;
    if (mask) {
      const int n = vol / g.C, c = vol - n * g.C;
      pm = mask + ((long)n * g.wC + (g.wC == 1 ? 0 : c)) * g.V;
    }
  }
}

template <int KIND, int VEC>
__global__ void __launch_bounds__(RG_THREADS) reg_forward_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                 const float* __restrict__ mask, float* __restrict__ partial, RgGeo g) {
  __shared__ float red[RG_THREADS];
  const float *pa, *pb, *pc, *pm;
  rg_rows<KIND>(a, b, mask, blockIdx.y, g, pa, pb, pc, pm);
  const long base = (long)blockIdx.x * RG_TILE;
  float s = 0.f;
  if (VEC) {
#pragma unroll
    for (int k = 0; k < RG_PER_THREAD / 4; ++k) {
      const long i = base + ((long)k * RG_THREADS + threadIdx.x) * 4;
      if (i < g.V) {                                                       // V % 4 == 0: the whole vector is inside
        const f32x4_t z = {0.f, 0.f, 0.f, 0.f}, one = {1.f, 1.f, 1.f, 1.f};
        const f32x4_t va = *reinterpret_cast<const f32x4_t*>(pa + i);
        const f32x4_t vb = pb ? *reinterpret_cast<const f32x4_t*>(pb + i) : z;
        const f32x4_t vc = pc ? *reinterpret_cast<const f32x4_t*>(pc + i) : z;
        const f32x4_t vm = pm ? *reinterpret_cast<const f32x4_t*>(pm + i) : one;
#pragma unroll
        for (int j = 0; j < 4; ++j) s += rg_loss<KIND>(va[j], vb[j], vc[j], pc != nullptr, g) * vm[j];
      }
    }
  } else {
#pragma unroll 4
    for (int k = 0; k < RG_PER_THREAD; ++k) {
      const long i = base + (long)k * RG_THREADS + threadIdx.x;
      if (i < g.V) s += rg_loss<KIND>(pa[i], pb ? pb[i] : 0.f, pc ? pc[i] : 0.f, pc != nullptr, g) * (pm ? pm[i] : 1.f);
    }
  }
  s = block_sum<RG_THREADS>(s, red);
  if (threadIdx.x == 0) partial[(long)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

// sum[0] = the n partials in a fixed order (one workgroup)
__global__ void __launch_bounds__(RG_THREADS) reg_sum_kernel(const float* __restrict__ partial, float* __restrict__ sum, long n) {
  __shared__ float red[RG_THREADS];
  float s = 0.f;
  for (long i = threadIdx.x; i < n; i += RG_THREADS) s += partial[i];
  s = block_sum<RG_THREADS>(s, red);
  if (threadIdx.x == 0) sum[0] = s;
}

// blockIdx.y = the volume; NONOVERLAP: sample n = y / (C - 1), j = y % (C - 1): j = 0 writes channels 0 and 1, j >= 1 zeroes channel j + 1
template <int KIND, int VEC>
__global__ void __launch_bounds__(RG_THREADS) reg_backward_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                  const float* __restrict__ mask, const float* __restrict__ coef,
                                                                  float* __restrict__ da, float* __restrict__ db, RgGeo g) {
  const float *pa, *pb, *pc, *pm;
  float *qa, *qb = nullptr;
  bool zero_only = false;
  if (KIND == PYTC_REG_NONOVERLAP) {
    const int n = blockIdx.y / (g.C - 1), j = blockIdx.y - n * (g.C - 1);
    rg_rows<KIND>(a, b, mask, n, g, pa, pb, pc, pm);
    qa = da + (long)n * g.C * g.V;
    if (j == 0) {
      qb = qa + g.V;
    } else {
      qa += (long)(j + 1) * g.V;
      zero_only = true;
    }
  } else {
    rg_rows<KIND>(a, b, mask, blockIdx.y, g, pa, pb, pc, pm);
    qa = da + (long)blockIdx.y * g.V;
    if (KIND != PYTC_REG_BINARY) qb = db + (long)blockIdx.y * g.V;
  }
  const float cf = coef[0];
  const long base = (long)blockIdx.x * RG_TILE;
  if (VEC) {
#pragma unroll
    for (int k = 0; k < RG_PER_THREAD / 4; ++k) {
      const long i = base + ((long)k * RG_THREADS + threadIdx.x) * 4;
      if (i < g.V) {
        const f32x4_t z = {0.f, 0.f, 0.f, 0.f}, one = {1.f, 1.f, 1.f, 1.f};
        if (zero_only) {
          *reinterpret_cast<f32x4_t*>(qa + i) = z;
          continue;
        }
        const f32x4_t va = *reinterpret_cast<const f32x4_t*>(pa + i);
        const f32x4_t vb = pb ? *reinterpret_cast<const f32x4_t*>(pb + i) : z;
        const f32x4_t vc = pc ? *reinterpret_cast<const f32x4_t*>(pc + i) : z;
        const f32x4_t vm = pm ? *reinterpret_cast<const f32x4_t*>(pm + i) : one;
        f32x4_t ga, gb;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float x, y;
          rg_grad<KIND>(va[j], vb[j], vc[j], pc != nullptr, g, cf * vm[j], x, y);
          ga[j] = x;
          gb[j] = y;
        }
        *reinterpret_cast<f32x4_t*>(qa + i) = ga;
        if (qb) *reinterpret_cast<f32x4_t*>(qb + i) = gb;
      }
    }
  } else {
#pragma unroll 4
    for (int k = 0; k < RG_PER_THREAD; ++k) {
      const long i = base + (long)k * RG_THREADS + threadIdx.x;
      if (i < g.V) {
        if (zero_only) {
          qa[i] = 0.f;
          continue;
        }
        float x, y;
        rg_grad<KIND>(pa[i], pb ? pb[i] : 0.f, pc ? pc[i] : 0.f, pc != nullptr, g, cf * (pm ? pm[i] : 1.f), x, y);
        qa[i] = x;
        if (qb) qb[i] = y;
      }
    }
  }
}

// ---- ForegroundContourConsistency ------------------------------------------------------------------------------------------------
constexpr int FC_THREADS = 256;
constexpr int FC_TX = 64, FC_TY = 32;
constexpr int FC_PAD = 4;                            // staged columns left and right of the tile (>= the widest halo)
constexpr int FC_ROW = FC_TX + 2 * FC_PAD;           // 72 floats

struct FcGeo {
  int D, H, W;
  long V;
  int ny, nx;
  float eps, hi;                                     // the clamp bounds eps and 1 - eps (rounded once from double, as torch does)
};

__device__ __forceinline__ void fc_tile_origin(int tile, const FcGeo& g, int& z, int& y0, int& x0) {
  const int tx = tile % g.nx, rem = tile / g.nx;
  x0 = tx * FC_TX;
  y0 = (rem % g.ny) * FC_TY;
  z = rem / g.ny;
}

// P = sigmoid(fg) over the tile and HALO rows above and below (all FC_ROW columns), zero outside the plane
template <int HALO>
__device__ __forceinline__ void fc_stage_prob(const float* __restrict__ plane, const FcGeo& g, int y0, int x0, float* P) {
  constexpr int ROWS = FC_TY + 2 * HALO;
  for (int it = threadIdx.x; it < ROWS * FC_ROW; it += FC_THREADS) {
    const int ry = it / FC_ROW, rc = it - ry * FC_ROW;
    const int gy = y0 - HALO + ry, gx = x0 - FC_PAD + rc;
    float p = 0.f;
    if (gy >= 0 && gy < g.H && gx >= 0 && gx < g.W) p = rg_sigmoid(plane[(long)gy * g.W + gx]);
    P[it] = p;
  }
}

// ex, ey and the unclamped magnitude of the edge voxel at LDS position o (its four neighbours are staged)
__device__ __forceinline__ float fc_edge(const float* P, int o, float eps, float& ex, float& ey) {
  ex = P[o - 1] - P[o + 1];
  ey = P[o - FC_ROW] - P[o + FC_ROW];
  return sqrtf(ex * ex + ey * ey + eps);
}

// E = the clamped magnitude over rows [HALO - EH, ...) i.e. the tile and EH voxels around it; 0 outside the plane (e >= eps > 0 inside)
template <int HALO, int EH>
__device__ __forceinline__ void fc_stage_edge(const float* P, const FcGeo& g, int y0, int x0, float* E) {
  constexpr int NR = FC_TY + 2 * EH, NC = FC_TX + 2 * EH;
  for (int it = threadIdx.x; it < NR * NC; it += FC_THREADS) {
    const int r = it / NC, c = it - r * NC;
    const int ry = HALO - EH + r, rc = FC_PAD - EH + c;
    const int gy = y0 - HALO + ry, gx = x0 - FC_PAD + rc;
    float e = 0.f;
    if (gy >= 0 && gy < g.H && gx >= 0 && gx < g.W) {
      float ex, ey;
      e = fminf(fmaxf(fc_edge(P, ry * FC_ROW + rc, g.eps, ex, ey), g.eps), g.hi);
    }
    E[ry * FC_ROW + rc] = e;
  }
}

__global__ void __launch_bounds__(FC_THREADS) fgcontour_forward_kernel(const float* __restrict__ fg, const float* __restrict__ ct,
                                                                       const float* __restrict__ mask, uint8_t* __restrict__ code,
                                                                       float* __restrict__ partial, FcGeo g) {
  constexpr int HALO = 2, ROWS = FC_TY + 2 * HALO;
  __shared__ __align__(16) float P[ROWS * FC_ROW];
  __shared__ __align__(16) float E[ROWS * FC_ROW];
  __shared__ float red[FC_THREADS];
  int z, y0, x0;
  fc_tile_origin(blockIdx.x, g, z, y0, x0);
  const long plane = (long)blockIdx.y * g.V + (long)z * g.H * g.W;
  fc_stage_prob<HALO>(fg + plane, g, y0, x0, P);
  __syncthreads();
  fc_stage_edge<HALO, 1>(P, g, y0, x0, E);
  __syncthreads();
  const int lx = threadIdx.x & 63, ly0 = (threadIdx.x >> 6) * 8, gx = x0 + lx;
  float s = 0.f;
  if (gx < g.W) {
    for (int ly = ly0; ly < ly0 + 8; ++ly) {
      const int gy = y0 + ly;
      if (gy >= g.H) break;
      const int o = (ly + HALO) * FC_ROW + lx + FC_PAD;
      float best = 0.f;
      int cd = 4;
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          const float v = E[o + dy * FC_ROW + dx];
          const bool gt = v > best;                   // strict: the first maximum in (y, x) scan order; the zeros outside never win
          best = gt ? v : best;
          cd = gt ? (dy + 1) * 3 + (dx + 1) : cd;
        }
      }
      const long i = plane + (long)gy * g.W + gx;
      code[i] = (uint8_t)cd;
      const float d = best - rg_sigmoid(ct[i]);
      s += (d * d) * (mask ? mask[i] : 1.f);
    }
  }
  s = block_sum<FC_THREADS>(s, red);
  if (threadIdx.x == 0) partial[(long)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

__global__ void __launch_bounds__(FC_THREADS) fgcontour_backward_kernel(const float* __restrict__ fg, const float* __restrict__ ct,
                                                                        const float* __restrict__ mask, const uint8_t* __restrict__ code,
                                                                        const float* __restrict__ coef, float* __restrict__ dfg,
                                                                        float* __restrict__ dct, FcGeo g) {
  constexpr int HALO = 4, ROWS = FC_TY + 2 * HALO;
  __shared__ __align__(16) float P[ROWS * FC_ROW];
  __shared__ __align__(16) float E[ROWS * FC_ROW];        // e through phase 3, then the edge gradient along x
  __shared__ __align__(16) float G[ROWS * FC_ROW];
  __shared__ __align__(16) float GY[ROWS * FC_ROW];
  __shared__ uint8_t CD[ROWS * FC_ROW];
  int z, y0, x0;
  fc_tile_origin(blockIdx.x, g, z, y0, x0);
  const long plane = (long)blockIdx.y * g.V + (long)z * g.H * g.W;
  const float cf = coef[0];
  fc_stage_prob<HALO>(fg + plane, g, y0, x0, P);
  __syncthreads();
  fc_stage_edge<HALO, 3>(P, g, y0, x0, E);
  __syncthreads();
  {                                                       // phase 3: G and the code of every output within 2 of the tile
    constexpr int NR = FC_TY + 4, NC = FC_TX + 4;
    for (int it = threadIdx.x; it < NR * NC; it += FC_THREADS) {
      const int r = it / NC, c = it - r * NC;
      const int ry = HALO - 2 + r, rc = FC_PAD - 2 + c;
      const int gy = y0 - HALO + ry, gx = x0 - FC_PAD + rc;
      float gv = 0.f;
      int cd = 255;                                       // names no voxel
      if (gy >= 0 && gy < g.H && gx >= 0 && gx < g.W) {
        const long i = plane + (long)gy * g.W + gx;
        const int k = code[i];
        if (k <= 8) {
          cd = k;
          const float e = E[(ry + k / 3 - 1) * FC_ROW + rc + k % 3 - 1];
          float q, qc;
          rg_sig2(ct[i], q, qc);
          gv = cf * (mask ? mask[i] : 1.f) * (2.f * (e - q));
          if (r >= 2 && r < NR - 2 && c >= 2 && c < NC - 2) dct[i] = -gv * (q * qc);
        } else if (r >= 2 && r < NR - 2 && c >= 2 && c < NC - 2) {
          dct[i] = 0.f;
        }
      }
      G[ry * FC_ROW + rc] = gv;
      CD[ry * FC_ROW + rc] = (uint8_t)cd;
    }
  }
  __syncthreads();
  {                                                       // phase 4: every edge voxel within 1 of the tile gathers, then splits along x and y
    constexpr int NR = FC_TY + 2, NC = FC_TX + 2;
    for (int it = threadIdx.x; it < NR * NC; it += FC_THREADS) {
      const int r = it / NC, c = it - r * NC;
      const int ry = HALO - 1 + r, rc = FC_PAD - 1 + c;
      const int gy = y0 - HALO + ry, gx = x0 - FC_PAD + rc;
      const int o = ry * FC_ROW + rc;
      float vx = 0.f, vy = 0.f;
      if (gy >= 0 && gy < g.H && gx >= 0 && gx < g.W) {
        float acc = 0.f;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
          for (int dx = -1; dx <= 1; ++dx) {
            const int q = o + dy * FC_ROW + dx;           // the output u + d chose u when its code is that of -d
            if ((int)CD[q] == (1 - dy) * 3 + (1 - dx)) acc += G[q];
          }
        }
        float ex, ey;
        const float raw = fc_edge(P, o, g.eps, ex, ey);
        if (raw >= g.eps && raw <= g.hi) {
          vx = acc * ex / raw;
          vy = acc * ey / raw;
        }
      }
      E[o] = vx;
      GY[o] = vy;
    }
  }
  __syncthreads();
  const int lx = threadIdx.x & 63, ly0 = (threadIdx.x >> 6) * 8, gx = x0 + lx;
  if (gx < g.W) {
    for (int ly = ly0; ly < ly0 + 8; ++ly) {
      const int gy = y0 + ly;
      if (gy >= g.H) break;
      const int o = (ly + HALO) * FC_ROW + lx + FC_PAD;
      const float dp = ((E[o + 1] - E[o - 1]) + GY[o + FC_ROW]) - GY[o - FC_ROW];
      const float p = P[o];
      dfg[plane + (long)gy * g.W + gx] = dp * (p * (1.f - p));
    }
  }
}

static int fc_geo(const char* what, int N, int D, int H, int W, double eps, FcGeo& g) {
  PYTC_REQUIRE(N >= 1 && N <= 65535 && D >= 1 && H >= 1 && W >= 1, "%s: bad shape N %d, (%d, %d, %d)", what, N, D, H, W);
  PYTC_REQUIRE(eps > 0.0 && eps < 0.5, "%s: eps %g outside (0, 0.5)", what, eps);
  g.D = D;
  g.H = H;
  g.W = W;
  g.V = (long)D * H * W;
  PYTC_REQUIRE((long)H * W <= 0x7fffffffL, "%s: %ld voxels per plane", what, (long)H * W);
  g.ny = ceil_div(H, FC_TY);
  g.nx = ceil_div(W, FC_TX);
  PYTC_REQUIRE((long)D * g.ny * g.nx <= 0x7fffffffL, "%s: %ld tiles per volume", what, (long)D * g.ny * g.nx);
  g.eps = (float)eps;
  g.hi = (float)(1.0 - eps);
  PYTC_REQUIRE(g.eps > 0.f, "%s: eps %g is zero in fp32", what, eps);
  return PYTC_OK;
}

static bool rg_aligned(const void* p) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static int rg_geo(const char* what, int kind, const float* a, const float* b, const float* mask, int N, int C, int wC, long V, float param,
                  int flag, RgGeo& g, int& nvol) {
  PYTC_REQUIRE(kind >= PYTC_REG_BINARY && kind <= PYTC_REG_NONOVERLAP, "%s: unknown kind %d", what, kind);
  PYTC_REQUIRE(N >= 1 && C >= 1 && V >= 1, "%s: bad shape N %d, C %d, V %ld", what, N, C, V);
  PYTC_REQUIRE(a != nullptr, "%s: operand a is required", what);
  if (kind == PYTC_REG_NONOVERLAP) {
    PYTC_REQUIRE(C >= 2, "%s: NONOVERLAP needs at least 2 channels, got %d", what, C);
    PYTC_REQUIRE(b == nullptr && mask == nullptr, "%s: NONOVERLAP takes one operand and no mask", what);
    nvol = N;
  } else {
    PYTC_REQUIRE((kind == PYTC_REG_BINARY) == (b == nullptr), "%s: kind %d takes %s", what, kind,
                 kind == PYTC_REG_BINARY ? "one operand" : "two operands");
    PYTC_REQUIRE(!mask || wC == C || wC == 1, "%s: the mask has %d channels, expected %d or 1", what, wC, C);
    PYTC_REQUIRE((long)N * C <= 65535, "%s: %ld volumes", what, (long)N * C);
    nvol = N * C;
  }
  PYTC_REQUIRE((long)N * (C > 1 ? C - 1 : 1) <= 65535, "%s: %ld volumes", what, (long)N * C);
  PYTC_REQUIRE((V + RG_TILE - 1) / RG_TILE <= 0x7fffffffL, "%s: %ld voxels per volume", what, V);
  g.V = V;
  g.C = C;
  g.wC = mask ? wC : C;
  g.param = param;
  g.flag = flag;
  return PYTC_OK;
}

}  // namespace pytc

using namespace pytc;

extern "C" int pytc_reg_tiles(int64_t voxels) { return ceil_div((long)voxels, RG_TILE); }

#define RG_DISPATCH(KERNEL, grid, ...)                                                                                          \
  do {                                                                                                                          \
    switch (kind * 2 + vec) {                                                                                                   \
      case 0: hipLaunchKernelGGL((KERNEL<PYTC_REG_BINARY, 0>), grid, dim3(RG_THREADS), 0, st, __VA_ARGS__); break;              \
      case 1: hipLaunchKernelGGL((KERNEL<PYTC_REG_BINARY, 1>), grid, dim3(RG_THREADS), 0, st, __VA_ARGS__); break;              \
      case 2: hipLaunchKernelGGL((KERNEL<PYTC_REG_FG_DIST, 0>), grid, dim3(RG_THREADS), 0, st, __VA_ARGS__); break;             \
      case 3: hipLaunchKernelGGL((KERNEL<PYTC_REG_FG_DIST, 1>), grid, dim3(RG_THREADS), 0, st, __VA_ARGS__); break;             \
      case 4: hipLaunchKernelGGL((KERNEL<PYTC_REG_CT_DIST, 0>), grid, dim3(RG_THREADS), 0, st, __VA_ARGS__); break;             \
      case 5: hipLaunchKernelGGL((KERNEL<PYTC_REG_CT_DIST, 1>), grid, dim3(RG_THREADS), 0, st, __VA_ARGS__); break;             \
      case 6: hipLaunchKernelGGL((KERNEL<PYTC_REG_NONOVERLAP, 0>), grid, dim3(RG_THREADS), 0, st, __VA_ARGS__); break;          \
      default: hipLaunchKernelGGL((KERNEL<PYTC_REG_NONOVERLAP, 1>), grid, dim3(RG_THREADS), 0, st, __VA_ARGS__); break;         \
    }                                                                                                                           \
  } while (0)

extern "C" int pytc_reg_pointwise_forward(int kind, const float* a, const float* b, const float* mask, float* partial, float* sum, int N,
                                          int C, int wC, int64_t V, float param, int flag, void* stream) {
  RgGeo g;
  int nvol;
  if (int s = rg_geo("reg_pointwise_forward", kind, a, b, mask, N, C, wC, (long)V, param, flag, g, nvol)) return s;
  PYTC_REQUIRE(partial && sum, "reg_pointwise_forward: partial and sum are required");
  const int vec = (V % 4 == 0 && rg_aligned(a) && rg_aligned(b) && rg_aligned(mask)) ? 1 : 0;
  const int slots = pytc_reg_tiles(V);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(slots, nvol);
  RG_DISPATCH(reg_forward_kernel, grid, a, b, mask, partial, g);
  PYTC_LAUNCH_CHECK("reg_pointwise_forward");
  hipLaunchKernelGGL(reg_sum_kernel, dim3(1), dim3(RG_THREADS), 0, st, partial, sum, (long)slots * nvol);
  PYTC_LAUNCH_CHECK("reg_pointwise_forward_sum");
  return PYTC_OK;
}

extern "C" int pytc_reg_pointwise_backward(int kind, const float* a, const float* b, const float* mask, const float* coef, float* da,
                                           float* db, int N, int C, int wC, int64_t V, float param, int flag, void* stream) {
  RgGeo g;
  int nvol;
  if (int s = rg_geo("reg_pointwise_backward", kind, a, b, mask, N, C, wC, (long)V, param, flag, g, nvol)) return s;
  const bool two = kind == PYTC_REG_FG_DIST || kind == PYTC_REG_CT_DIST;
  PYTC_REQUIRE(coef && da && da != a && two == (db != nullptr) && (!db || (db != b && db != da)),
               "reg_pointwise_backward: null, surplus or aliased pointer");
  const int vec = (V % 4 == 0 && rg_aligned(a) && rg_aligned(b) && rg_aligned(mask) && rg_aligned(da) && rg_aligned(db)) ? 1 : 0;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(pytc_reg_tiles(V), kind == PYTC_REG_NONOVERLAP ? N * (C - 1) : nvol);
  RG_DISPATCH(reg_backward_kernel, grid, a, b, mask, coef, da, db, g);
  PYTC_LAUNCH_CHECK("reg_pointwise_backward");
  return PYTC_OK;
}

extern "C" int pytc_fgcontour_tiles(int D, int H, int W) {
  if (D < 1 || H < 1 || W < 1) return 0;
  const long n = (long)D * ceil_div(H, FC_TY) * ceil_div(W, FC_TX);
  return n <= 0x7fffffffL ? (int)n : 0;
}

extern "C" int pytc_fgcontour_forward(const float* fg, const float* contour, const float* mask, uint8_t* code, float* partial, float* sum,
                                      int N, int D, int H, int W, double eps, void* stream) {
  FcGeo g;
  if (int s = fc_geo("fgcontour_forward", N, D, H, W, eps, g)) return s;
  PYTC_REQUIRE(fg && contour && code && partial && sum, "fgcontour_forward: fg, contour, code, partial and sum are required");
  const int tiles = pytc_fgcontour_tiles(D, H, W);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(fgcontour_forward_kernel, dim3(tiles, N), dim3(FC_THREADS), 0, st, fg, contour, mask, code, partial, g);
  PYTC_LAUNCH_CHECK("fgcontour_forward");
  hipLaunchKernelGGL(reg_sum_kernel, dim3(1), dim3(RG_THREADS), 0, st, partial, sum, (long)tiles * N);
  PYTC_LAUNCH_CHECK("fgcontour_forward_sum");
  return PYTC_OK;
}

extern "C" int pytc_fgcontour_backward(const float* fg, const float* contour, const float* mask, const uint8_t* code, const float* coef,
                                       float* dfg, float* dcontour, int N, int D, int H, int W, double eps, void* stream) {
  FcGeo g;
  if (int s = fc_geo("fgcontour_backward", N, D, H, W, eps, g)) return s;
  PYTC_REQUIRE(fg && contour && code && coef && dfg && dcontour && dfg != fg && dcontour != contour && dfg != dcontour,
               "fgcontour_backward: null or aliased pointer");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(fgcontour_backward_kernel, dim3(pytc_fgcontour_tiles(D, H, W), N), dim3(FC_THREADS), 0, st, fg, contour, mask, code,
                     coef, dfg, dcontour, g);
  PYTC_LAUNCH_CHECK("fgcontour_backward");
  return PYTC_OK;
}
