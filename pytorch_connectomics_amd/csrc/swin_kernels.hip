// Token-layout kernels of MONAI SwinUNETR's Swin encoder on the MI355X: window partition / reverse (zero pad, cyclic roll, crop,
// fused residual), the 2x2x2 space-to-depth of the patch embedding and of PatchMerging, and a LayerNorm for any width that is a
// multiple of 16 (up to 6144), with or without affine parameters -- forward and backward.
//
// Reference: monai.networks.nets.swin_unetr (MONAI 1.3): window_partition / window_reverse, SwinTransformerBlock.forward_part1
// (F.pad, torch.roll, crop), PatchEmbed (Conv3d k 2 s 2), PatchMerging ("merging", v1), proj_out (F.layer_norm without affine),
// the encoder of the reference's `monai_swin_unetr` (connectomics/models/architectures/monai_models.py:297-334).  The window
// attention itself is csrc/transformer_kernels.hip (pytc_window_attention_*).
//
// Layouts: activations are channels-last token matrices (B * D * H * W, C), row-major over (b, d, h, w).  The window matrix has
// rows ((b * nW + window) * n + token): windows row-major over the padded grid's (D_p / ws_d, H_p / ws_h, W_p / ws_w), tokens
// row-major inside a window.  One wave per row, lanes over channels; every output element has one writer, every sum a fixed order.
#include <algorithm>

#include "pytc_common.h"

namespace pytc {

// grid (3), window (3), padded grid (3), shift (3)
struct WinGeo {
  int G[3], ws[3], P[3], sh[3];
};

// dir 0 (partition): dst window row r = src token at the padded, rolled position of r, or zeros in the padding.
// dir 1 (reverse):   dst token t = src window row holding t (+ res[t] when res is non-null): roll back and crop.
template <typename T>
__global__ void __launch_bounds__(256) window_gather_kernel(const T* __restrict__ src, T* __restrict__ dst, const T* __restrict__ res,
                                                            WinGeo g, long rows, int C, int dir) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const int nw1 = g.P[1] / g.ws[1], nw2 = g.P[2] / g.ws[2], nw0 = g.P[0] / g.ws[0];
  long other;       // the row of the other matrix, -1 for a padding row
  if (dir == 0) {
    const int n = g.ws[0] * g.ws[1] * g.ws[2];
    const int i = (int)(row % n);
    const long w = row / n;
    const int wl = (int)(w % ((long)nw0 * nw1 * nw2));
    const long b = w / ((long)nw0 * nw1 * nw2);
    const int pd = (wl / (nw1 * nw2)) * g.ws[0] + i / (g.ws[1] * g.ws[2]);
    const int ph = (wl / nw2 % nw1) * g.ws[1] + i / g.ws[2] % g.ws[1];
    const int pw = (wl % nw2) * g.ws[2] + i % g.ws[2];
    const int z = (pd + g.sh[0]) % g.P[0], y = (ph + g.sh[1]) % g.P[1], x = (pw + g.sh[2]) % g.P[2];
    other = (z < g.G[0] && y < g.G[1] && x < g.G[2]) ? ((b * g.G[0] + z) * g.G[1] + y) * g.G[2] + x : -1;
  } else {
    const int x = (int)(row % g.G[2]);
    long t = row / g.G[2];
    const int y = (int)(t % g.G[1]);
    t /= g.G[1];
    const int z = (int)(t % g.G[0]);
    const long b = t / g.G[0];
    const int pd = (z - g.sh[0] + g.P[0]) % g.P[0], ph = (y - g.sh[1] + g.P[1]) % g.P[1], pw = (x - g.sh[2] + g.P[2]) % g.P[2];
    const int wl = ((pd / g.ws[0]) * nw1 + ph / g.ws[1]) * nw2 + pw / g.ws[2];
    const int i = ((pd % g.ws[0]) * g.ws[1] + ph % g.ws[1]) * g.ws[2] + pw % g.ws[2];
    other = (b * ((long)nw0 * nw1 * nw2) + wl) * ((long)g.ws[0] * g.ws[1] * g.ws[2]) + i;
  }
  T* d = dst + row * C;
  if (other < 0) {
    for (int c = lane; c < C; c += 64) d[c] = from_f32<T>(0.f);
    return;
  }
  const T* s = src + other * C;
  if (res) {
    const T* r = res + row * C;
    for (int c = lane; c < C; c += 64) d[c] = from_f32<T>(to_f32<T>(s[c]) + to_f32<T>(r[c]));
  } else {
    for (int c = lane; c < C; c += 64) d[c] = s[c];
  }
}

// 2x2x2 space-to-depth: column block `slot` of an output row holds the voxel at offset s2d_off(order, slot) of its 2^3 cell.
// order 0: (kd, kh, kw) row-major, the Conv3d(k 2, s 2) weight's tap order; order 1: MONAI PatchMerging v1's x0..x7 list, which
// reads (0,1,0) and (0,0,1) twice and never (1,1,0) or (0,1,1).
__device__ __forceinline__ int s2d_off(int order, int slot) {   // bits: d << 2 | h << 1 | w
  constexpr int v1[8] = {0, 4, 2, 1, 5, 2, 1, 7};
  return order == 0 ? slot : v1[slot];
}

// dir 0: cols (B * D/2 * H/2 * W/2, 8 C) from x (B, D, H, W, C), one wave per output row.
// dir 1: dx (B, D, H, W, C) = the sum over the slots that read each voxel (slot order), zero where none does, one wave per voxel.
template <typename T>
__global__ void __launch_bounds__(256) s2d_kernel(const T* __restrict__ src, T* __restrict__ dst, int D, int H, int W, int C, long rows,
                                                  int order, int dir) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const int h2 = H >> 1, w2 = W >> 1, d2 = D >> 1;
  if (dir == 0) {
    const int x = (int)(row % w2);
    long t = row / w2;
    const int y = (int)(t % h2);
    t /= h2;
    const int z = (int)(t % d2);
    const long b = t / d2;
    T* o = dst + row * 8L * C;
    for (int slot = 0; slot < 8; ++slot) {
      const int off = s2d_off(order, slot);
      const T* s = src + (((b * D + 2 * z + (off >> 2)) * H + 2 * y + ((off >> 1) & 1)) * W + 2 * x + (off & 1)) * C;
      for (int c = lane; c < C; c += 64) o[slot * C + c] = s[c];
    }
  } else {
    const int x = (int)(row % W);
    long t = row / W;
    const int y = (int)(t % H);
    t /= H;
    const int z = (int)(t % D);
    const long b = t / D;
    const int mine = ((z & 1) << 2) | ((y & 1) << 1) | (x & 1);
    const T* s = src + (((b * d2 + (z >> 1)) * h2 + (y >> 1)) * w2 + (x >> 1)) * 8L * C;
    T* o = dst + row * C;
    for (int c = lane; c < C; c += 64) {
      float v = 0.f;
      for (int slot = 0; slot < 8; ++slot)
        if (s2d_off(order, slot) == mine) v += to_f32<T>(s[slot * C + c]);
      o[c] = from_f32<T>(v);
    }
  }
}

// ------------------------------------------------------------------------------------------------ LayerNorm, any width
// one wave per row; two-pass statistics (mean, then the centred sum of squares) over the row, re-read from cache
template <typename T>
__device__ __forceinline__ void ln_row_stats(const T* xr, int C, int lane, float& mean, float& rstd, float eps) {
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += to_f32<T>(xr[c]);
  mean = wave_sum(s) / (float)C;
  float q = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float v = to_f32<T>(xr[c]) - mean;
    q += v * v;
  }
  rstd = rsqrtf(wave_sum(q) / (float)C + eps);
}

template <typename T>
__global__ void __launch_bounds__(256) layernorm_any_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, const float* gamma,
                                                                const float* beta, long rows, int C, float eps) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const T* xr = x + row * C;
  float mean, rstd;
  ln_row_stats(xr, C, lane, mean, rstd, eps);
  T* yr = y + row * C;
  for (int c = lane; c < C; c += 64) {
    float v = (to_f32<T>(xr[c]) - mean) * rstd;
    if (gamma) v = v * gamma[c] + beta[c];
    yr[c] = from_f32<T>(v);
  }
}

// dx = rstd (g - mean(g) - xhat mean(g xhat)), g = dy * gamma (dy without affine); stats[row] = (mean, rstd) for the parameter pass
template <typename T>
__global__ void __launch_bounds__(256) layernorm_any_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ x, const float* gamma,
                                                                T* __restrict__ dx, float2* __restrict__ stats, long rows, int C, float eps) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const T* xr = x + row * C;
  const T* gr = dy + row * C;
  float mean, rstd;
  ln_row_stats(xr, C, lane, mean, rstd, eps);
  float s1 = 0.f, s2 = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float g = to_f32<T>(gr[c]) * (gamma ? gamma[c] : 1.f);
    s1 += g;
    s2 += g * (to_f32<T>(xr[c]) - mean) * rstd;
  }
  s1 = wave_sum(s1) / (float)C;
  s2 = wave_sum(s2) / (float)C;
  T* dr = dx + row * C;
  for (int c = lane; c < C; c += 64) {
    const float g = to_f32<T>(gr[c]) * (gamma ? gamma[c] : 1.f);
    dr[c] = from_f32<T>(rstd * (g - s1 - (to_f32<T>(xr[c]) - mean) * rstd * s2));
  }
  if (stats && lane == 0) stats[row] = make_float2(mean, rstd);
}

constexpr int LNA_ROWS_PER_SLOT = 256;
// the parameter kernel's slots are gridDim.y; 65535 is a conservative constant (the smallest y limit HIP devices report), not read
// from the device
constexpr int LNA_MAX_SLOTS = 65535;

// partial[slot][0][c] = sum dy xhat, partial[slot][1][c] = sum dy over the slot's rows (ascending); grid (ceil(C / 256), slots)
template <typename T>
__global__ void layernorm_any_param_kernel(const T* __restrict__ dy, const T* __restrict__ x, const float2* __restrict__ stats,
                                           float* __restrict__ partial, long rows, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const long r0 = (long)blockIdx.y * LNA_ROWS_PER_SLOT, r1 = std::min<long>(rows, r0 + LNA_ROWS_PER_SLOT);
  float pg = 0.f, pb = 0.f;
  for (long r = r0; r < r1; ++r) {
    const float2 st = stats[r];
    const float g = to_f32<T>(dy[r * C + c]);
    pg += g * (to_f32<T>(x[r * C + c]) - st.x) * st.y;
    pb += g;
  }
  partial[((long)blockIdx.y * 2 + 0) * C + c] = pg;
  partial[((long)blockIdx.y * 2 + 1) * C + c] = pb;
}

__global__ void layernorm_any_reduce_kernel(const float* __restrict__ partial, float* dgamma, float* dbeta, int slots, int C) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 2 * C) return;
  const int which = i / C, c = i % C;
  float s = 0.f;
  for (int b = 0; b < slots; ++b) s += partial[((long)b * 2 + which) * C + c];
  (which == 0 ? dgamma : dbeta)[c] = s;
}

}  // namespace pytc

using namespace pytc;

// ------------------------------------------------------------------------------------------------------------ C ABI
static int win_geo(const char* what, const int* geom, WinGeo* g) {
  PYTC_REQUIRE(geom, "%s: null geometry", what);
  for (int a = 0; a < 3; ++a) {
    g->G[a] = geom[a]; g->ws[a] = geom[3 + a]; g->P[a] = geom[6 + a]; g->sh[a] = geom[9 + a];
    PYTC_REQUIRE(g->G[a] >= 1 && g->ws[a] >= 1 && g->P[a] >= g->G[a] && g->P[a] % g->ws[a] == 0 && g->P[a] - g->G[a] < g->ws[a] &&
                 g->sh[a] >= 0 && g->sh[a] < g->ws[a],
                 "%s: axis %d: grid %d, window %d, padded %d, shift %d is not a window partition", what, a, g->G[a], g->ws[a], g->P[a],
                 g->sh[a]);
  }
  return PYTC_OK;
}

extern "C" int pytc_window_partition(const void* src, void* dst, const void* res, const int* geom, int B, int C, int reverse, int dtype,
                                     void* stream) {
  WinGeo g;
  if (int s = win_geo("window_partition", geom, &g)) return s;
  PYTC_REQUIRE(src && dst && B >= 1 && C >= 1 && (!res || reverse), "window_partition: bad arguments");
  const long rows = reverse ? (long)B * g.G[0] * g.G[1] * g.G[2] : (long)B * g.P[0] * g.P[1] * g.P[2];
  hipStream_t st = (hipStream_t)stream;
  dim3 grid(ceil_div(rows, 4));
  PYTC_DISPATCH_DTYPE(dtype, "window_partition", T,
                      hipLaunchKernelGGL(window_gather_kernel<T>, grid, dim3(256), 0, st, (const T*)src, (T*)dst, (const T*)res, g, rows, C,
                                         reverse));
  PYTC_LAUNCH_CHECK("window_partition");
  return PYTC_OK;
}

extern "C" int pytc_space_to_depth2(const void* src, void* dst, int B, int D, int H, int W, int C, int order, int scatter, int dtype,
                                    void* stream) {
  PYTC_REQUIRE(src && dst && B >= 1 && C >= 1 && D >= 2 && H >= 2 && W >= 2 && D % 2 == 0 && H % 2 == 0 && W % 2 == 0,
               "space_to_depth2: grid (%d, %d, %d) is not a whole number of 2^3 cells", D, H, W);
  PYTC_REQUIRE(order == 0 || order == 1, "space_to_depth2: order %d (0: conv taps, 1: PatchMerging v1)", order);
  const long rows = scatter ? (long)B * D * H * W : (long)B * (D / 2) * (H / 2) * (W / 2);
  hipStream_t st = (hipStream_t)stream;
  dim3 grid(ceil_div(rows, 4));
  PYTC_DISPATCH_DTYPE(dtype, "space_to_depth2", T,
                      hipLaunchKernelGGL(s2d_kernel<T>, grid, dim3(256), 0, st, (const T*)src, (T*)dst, D, H, W, C, rows, order, scatter));
  PYTC_LAUNCH_CHECK("space_to_depth2");
  return PYTC_OK;
}

static int ln_any_check(const char* what, int64_t rows, int C, int dtype) {
  PYTC_REQUIRE(rows >= 1 && C >= 16 && C <= 6144 && C % 16 == 0, "%s: C = %d must be a multiple of 16 in [16, 6144]", what, C);
  PYTC_CHECK_DTYPE(dtype, what);
  return PYTC_OK;
}

extern "C" int pytc_layernorm_any(const void* x, void* y, const float* gamma, const float* beta, int64_t rows, int C, float eps, int dtype,
                                  void* stream) {
  if (int s = ln_any_check("layernorm_any", rows, C, dtype)) return s;
  PYTC_REQUIRE(x && y && !gamma == !beta, "layernorm_any: null pointer (gamma and beta are both given or both null)");
  hipStream_t st = (hipStream_t)stream;
  dim3 grid(ceil_div(rows, 4));
  PYTC_DISPATCH_DTYPE(dtype, "layernorm_any", T,
                      hipLaunchKernelGGL(layernorm_any_fwd_kernel<T>, grid, dim3(256), 0, st, (const T*)x, (T*)y, gamma, beta, (long)rows, C, eps));
  PYTC_LAUNCH_CHECK("layernorm_any");
  return PYTC_OK;
}

extern "C" int pytc_layernorm_any_bwd_slots(int64_t rows) { return ceil_div(rows, LNA_ROWS_PER_SLOT); }

// stats: 2 rows floats; partial: 2 C pytc_layernorm_any_bwd_slots(rows) floats; both only read / written when dgamma is non-null
extern "C" int pytc_layernorm_any_bwd(const void* dy, const void* x, const float* gamma, void* dx, float* stats, float* partial,
                                      float* dgamma, float* dbeta, int64_t rows, int C, float eps, int dtype, void* stream) {
  if (int s = ln_any_check("layernorm_any_bwd", rows, C, dtype)) return s;
  PYTC_REQUIRE(dy && x && dx && (!dgamma || (gamma && dbeta && stats && partial)), "layernorm_any_bwd: null pointer");
  // layernorm_any_param_kernel has its row slots on gridDim.y: past the device's limit the launch would be rejected without a name
  const long param_slots = ((long)rows + LNA_ROWS_PER_SLOT - 1) / LNA_ROWS_PER_SLOT;          // in long: ceil_div narrows to int
  PYTC_REQUIRE(!dgamma || param_slots <= LNA_MAX_SLOTS,
               "layernorm_any_bwd: %ld rows are %ld parameter slots of %d rows, over the %d slots one launch takes: split the rows",
               (long)rows, param_slots, LNA_ROWS_PER_SLOT, LNA_MAX_SLOTS);
  hipStream_t st = (hipStream_t)stream;
  dim3 grid(ceil_div(rows, 4));
  float2* s2 = dgamma ? reinterpret_cast<float2*>(stats) : nullptr;
  const int slots = ceil_div(rows, LNA_ROWS_PER_SLOT);
  dim3 pg(ceil_div(C, 256), slots);
  PYTC_DISPATCH_DTYPE(dtype, "layernorm_any_bwd", T,
    hipLaunchKernelGGL(layernorm_any_bwd_kernel<T>, grid, dim3(256), 0, st, (const T*)dy, (const T*)x, gamma, (T*)dx, s2, (long)rows, C, eps);
    if (dgamma)
      hipLaunchKernelGGL(layernorm_any_param_kernel<T>, pg, dim3(256), 0, st, (const T*)dy, (const T*)x, (const float2*)s2, partial,
                         (long)rows, C));
  if (dgamma)
    hipLaunchKernelGGL(layernorm_any_reduce_kernel, dim3(ceil_div(2 * C, 256)), dim3(256), 0, st, (const float*)partial, dgamma, dbeta,
                       slots, C);
  PYTC_LAUNCH_CHECK("layernorm_any_bwd");
  return PYTC_OK;
}
