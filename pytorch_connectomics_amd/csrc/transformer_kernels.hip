// ViT encoder of MONAI UNETR on the MI355X: multi-head self-attention, wide-row LayerNorm, patch gather, and the linear layers
// with their epilogues, forward and backward.
//
// Reference: monai.networks.nets.UNETR (MONAI 1.3) -> ViT -> PatchEmbeddingBlock / TransformerBlock (SABlock, MLPBlock,
// nn.LayerNorm), the encoder of the reference's `monai_unetr` (connectomics/models/architectures/monai_models.py:253-294).
//
// Layouts: tokens are rows of (B * N, h) matrices, row-major; qkv is the (B * N, 3 h) output of the qkv linear layer with its
// columns in MONAI's (qkv, head, d) order, so head `hd`'s Q / K / V are column blocks hd * d, h + hd * d, 2 h + hd * d of it.
// Storage bf16 or fp32, accumulation fp32.  No atomics anywhere: every reduction has a fixed order, every output element one
// writer, so results are bit-reproducible run to run.
//
// Attention (softmax(Q K^T * d^-0.5) V per (batch, head)) works on 64 x 64 tiles with 256 threads.  Thread (ti, tj) of the
// 16 x 16 grid owns rows ti + 16 r and columns tj + 16 s (r, s < 4) of a tile, so the 16 owners of a row are 16 consecutive lanes
// of one wave and a row's max / sum is a 4-step xor shuffle.  Operands are staged in LDS as fp32 rows padded to d + 1 floats
// (the 16 column owners read 16 distinct banks, the row owners broadcast).
//   forward : per query tile, loop over key tiles with an online softmax; O = acc / l, lse = m + log l saved for the backward.
//   backward: Dv = rowsum(dO * O) (attn_bwd_dvec_kernel); dK, dV per KEY tile looping over query tiles (attn_bwd_dkv_kernel);
//             dQ per QUERY tile looping over key tiles (attn_bwd_dq_kernel).  P is recomputed from Q, K and lse in both.
//   WIN = true: MONAI SwinUNETR's shifted-window attention (pytc_window_attention_*): windows as the batch, the relative-position
//             bias and shift mask added to every score (WinArgs), d = 16 / 32; the bias-table gradient is win_attn_dbias_kernel's
//             fixed-slot per-window-group partials, summed in a fixed order by win_attn_table_grad_kernel.
//
// Linear layers: C[M][N] = sum_k A(m, k) B(k, n), one LDS-tiled FMA kernel with transposition flags for the three products
// (Y = f(X) W^T, dX = dY W, dW = dY^T f(X)), f = GELU (erf form, pytc_common.h gelu_erf) applied to an operand as it is loaded
// (the MLP's second layer reads the stored pre-activation, as the pointwise MFMA GEMM's pre_act prologue does).  Epilogue:
// + bias[n], + pos[m % P][n] (the position embedding, broadcast over the batch), then + res[m][n] or * gelu'(res[m][n]) (the data
// gradient through the GELU).  The UNETR path uses it where the MFMA GEMM of csrc/pw_gemm_kernels.hip does not apply: fp32, widths
// outside that kernel's rules, and the patch embedding's position-embedding epilogue.
#include <algorithm>

#include "pytc_common.h"

namespace pytc {

// ------------------------------------------------------------------------------------------------------ linear (GEMM)
struct LinParams {
  const void* A;
  const void* B;
  void* C;
  const float* bias;   // [N] or null
  const float* pos;    // [P][N] or null
  const void* res;     // [M][N] (C's type) or null
  int M, N, K, lda, ldb, ldc, P;
  int gelu_a, gelu_b;  // GELU on the A / B operand as it is loaded
  int res_gelu_bwd;    // 0: C = acc (+ res); 1: C = acc * gelu'(res)
};

constexpr int LG_BM = 64, LG_BN = 64, LG_BK = 32;

// gelu_erf / gelu_erf_grad / wave_sum: pytc_common.h

// A(m, k) = A_T ? A[k * lda + m] : A[m * lda + k];  B(k, n) = B_T ? B[n * ldb + k] : B[k * ldb + n]
template <typename TA, typename TB, typename TC, bool A_T, bool B_T>
__global__ void __launch_bounds__(256) linear_gemm_kernel(LinParams p) {
  __shared__ float sA[LG_BK][LG_BM + 4];
  __shared__ float sB[LG_BK][LG_BN + 4];
  const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
  const int m0 = blockIdx.y * LG_BM, n0 = blockIdx.x * LG_BN;
  const TA* A = reinterpret_cast<const TA*>(p.A);
  const TB* B = reinterpret_cast<const TB*>(p.B);
  float acc[4][4] = {};
  for (int k0 = 0; k0 < p.K; k0 += LG_BK) {
#pragma unroll
    for (int q = 0; q < LG_BM * LG_BK / 256; ++q) {
      const int e = tid + 256 * q;
      int mm, kk;
      if (A_T) { mm = e % LG_BM; kk = e / LG_BM; } else { kk = e % LG_BK; mm = e / LG_BK; }
      const int m = m0 + mm, k = k0 + kk;
      float v = 0.f;
      if (m < p.M && k < p.K) v = to_f32<TA>(A_T ? A[(long)k * p.lda + m] : A[(long)m * p.lda + k]);
      sA[kk][mm] = p.gelu_a ? gelu_erf(v) : v;
      int nn, kb;
      if (B_T) { kb = e % LG_BK; nn = e / LG_BK; } else { nn = e % LG_BN; kb = e / LG_BN; }
      const int n = n0 + nn, kB = k0 + kb;
      float w = 0.f;
      if (n < p.N && kB < p.K) w = to_f32<TB>(B_T ? B[(long)n * p.ldb + kB] : B[(long)kB * p.ldb + n]);
      sB[kb][nn] = p.gelu_b ? gelu_erf(w) : w;
    }
    __syncthreads();
#pragma unroll 8
    for (int k = 0; k < LG_BK; ++k) {
      float a[4], b[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) a[r] = sA[k][ti + 16 * r];
#pragma unroll
      for (int s = 0; s < 4; ++s) b[s] = sB[k][tj + 16 * s];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[r][s] = fmaf(a[r], b[s], acc[r][s]);
    }
    __syncthreads();
  }
  TC* C = reinterpret_cast<TC*>(p.C);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = m0 + ti + 16 * r;
    if (m >= p.M) continue;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int n = n0 + tj + 16 * s;
      if (n >= p.N) continue;
      float v = acc[r][s];
      if (p.bias) v += p.bias[n];
      if (p.pos) v += p.pos[(long)(m % p.P) * p.N + n];
      if (p.res) {
        const float r = to_f32<TC>(reinterpret_cast<const TC*>(p.res)[(long)m * p.ldc + n]);
        v = p.res_gelu_bwd ? v * gelu_erf_grad(r) : v + r;
      }
      C[(long)m * p.ldc + n] = from_f32<TC>(v);
    }
  }
}

// out[q][c] = sum_{b < M / P} X[b * P + q][c]: bias gradient (P = 1) and position-embedding gradient (P = tokens), fixed order
template <typename T>
__global__ void colsum_period_kernel(const T* __restrict__ x, float* __restrict__ out, int M, int C, int P) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)P * C) return;
  const int q = (int)(i / C), c = (int)(i % C);
  float s = 0.f;
  for (int m = q; m < M; m += P) s += to_f32<T>(x[(long)m * C + c]);
  out[i] = s;
}

// ------------------------------------------------------------------------------------------------- wide-row LayerNorm
// one wave per row of C = 64 * nv channels (nv <= 16): lane l holds channels k * 64 + l
constexpr int LN_MAXV = 16, LN_ROWS_PER_BLOCK = 32;

template <typename T>
__global__ void __launch_bounds__(256) layernorm_wide_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, const float* gamma,
                                                                 const float* beta, long rows, int C, float eps) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63, nv = C >> 6;
  if (row >= rows) return;
  const T* xr = x + row * C;
  float v[LN_MAXV];
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < LN_MAXV; ++k) {
    v[k] = k < nv ? to_f32<T>(xr[k * 64 + lane]) : 0.f;
    s += v[k];
  }
  const float mean = wave_sum(s) / (float)C;
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < LN_MAXV; ++k)
    if (k < nv) q += (v[k] - mean) * (v[k] - mean);
  const float rstd = rsqrtf(wave_sum(q) / (float)C + eps);
  T* yr = y + row * C;
#pragma unroll
  for (int k = 0; k < LN_MAXV; ++k)
    if (k < nv) {
      const int c = k * 64 + lane;
      yr[c] = from_f32<T>((v[k] - mean) * rstd * gamma[c] + beta[c]);
    }
}

// dx per row; partial[blk][0][c] = sum dy * xhat, partial[blk][1][c] = sum dy over the block's 32 rows (waves combined in order)
template <typename T>
__global__ void __launch_bounds__(256) layernorm_wide_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ x, const float* gamma,
                                                                 T* __restrict__ dx, float* __restrict__ partial, long rows, int C,
                                                                 float eps) {
  __shared__ float sg[4][2][1024];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nv = C >> 6;
  float pg[LN_MAXV] = {}, pb[LN_MAXV] = {};
  for (int it = 0; it < LN_ROWS_PER_BLOCK / 4; ++it) {
    const long row = (long)blockIdx.x * LN_ROWS_PER_BLOCK + it * 4 + wave;
    if (row >= rows) break;
    const T* xr = x + row * C;
    const T* gr = dy + row * C;
    float v[LN_MAXV], g[LN_MAXV];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < LN_MAXV; ++k) {
      v[k] = k < nv ? to_f32<T>(xr[k * 64 + lane]) : 0.f;
      g[k] = k < nv ? to_f32<T>(gr[k * 64 + lane]) : 0.f;
      s += v[k];
    }
    const float mean = wave_sum(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < LN_MAXV; ++k)
      if (k < nv) q += (v[k] - mean) * (v[k] - mean);
    const float rstd = rsqrtf(wave_sum(q) / (float)C + eps);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < LN_MAXV; ++k)
      if (k < nv) {
        const float xh = (v[k] - mean) * rstd;
        const float gg = g[k] * gamma[k * 64 + lane];
        v[k] = xh;
        s1 += gg;
        s2 += gg * xh;
        pg[k] += g[k] * xh;
        pb[k] += g[k];
      }
    s1 = wave_sum(s1) / (float)C;
    s2 = wave_sum(s2) / (float)C;
    T* dr = dx + row * C;
#pragma unroll
    for (int k = 0; k < LN_MAXV; ++k)
      if (k < nv) {
        const int c = k * 64 + lane;
        dr[c] = from_f32<T>(rstd * (g[k] * gamma[c] - s1 - v[k] * s2));
      }
  }
#pragma unroll
  for (int k = 0; k < LN_MAXV; ++k)
    if (k < nv) {
      sg[wave][0][k * 64 + lane] = pg[k];
      sg[wave][1][k * 64 + lane] = pb[k];
    }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    partial[((long)blockIdx.x * 2 + 0) * C + c] = ((sg[0][0][c] + sg[1][0][c]) + sg[2][0][c]) + sg[3][0][c];
    partial[((long)blockIdx.x * 2 + 1) * C + c] = ((sg[0][1][c] + sg[1][1][c]) + sg[2][1][c]) + sg[3][1][c];
  }
}

__global__ void layernorm_wide_reduce_kernel(const float* __restrict__ partial, float* dgamma, float* dbeta, int slots, int C) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 2 * C) return;
  const int which = i / C, c = i % C;
  float s = 0.f;
  for (int b = 0; b < slots; ++b) s += partial[((long)b * 2 + which) * C + c];
  float* out = which == 0 ? dgamma : dbeta;
  if (out) out[c] = s;
}

// ------------------------------------------------------------------------------------------------------ patch gather
// patches[(b * n_tok + t)][((p1 * 16 + p2) * 16 + p3) * C + c] = x[b][tz * 16 + p1][ty * 16 + p2][tx * 16 + p3][c]: MONAI's
// Rearrange("b c (h p1) (w p2) (d p3) -> b (h w d) (p1 p2 p3 c)") on channels-last x.  dir 0 gathers, dir 1 scatters back.
template <typename T>
__global__ void patch_gather_kernel(const T* __restrict__ src, T* __restrict__ dst, int B, int D, int H, int W, int C, int dir) {
  const int td = D >> 4, th = H >> 4, tw = W >> 4;
  const long cols = 4096L * C, total = (long)B * td * th * tw * cols;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const long row = e / cols;
    const int col = (int)(e % cols);
    const int c = col % C, p = col / C, p3 = p & 15, p2 = (p >> 4) & 15, p1 = p >> 8;
    const int tx = (int)(row % tw);
    long t = row / tw;
    const int ty = (int)(t % th);
    t /= th;
    const int tz = (int)(t % td);
    const int b = (int)(t / td);
    const long xi = ((((long)b * D + tz * 16 + p1) * H + ty * 16 + p2) * W + tx * 16 + p3) * C + c;
    if (dir == 0) dst[e] = src[xi];
    else dst[xi] = src[e];
  }
}

// --------------------------------------------------------------------------------------------------------- attention
constexpr int AT_T = 64;

// Shifted-window attention of MONAI's SwinUNETR (WIN = true): the "batch" is the window, N = n tokens of it, and every score gets
// S = q k^T * scale + table[rel(i, j)][head] (+ -100 where the shift-region labels of i and j differ).  rel(i, j) is MONAI's
// relative_position_index of the FULL 7^3 window sliced to [:n, :n]: with i's coordinates taken in the 7^3 grid,
// rel = c13(i) - c13(j) + 1098, c13(t) = (t / 49) * 169 + (t / 7 % 7) * 13 + t % 7.  The labels are compute_mask's, on the padded,
// rolled grid: per axis 0 below P - ws, 1 below P - s, else 2 (every coordinate 2 when that axis' shift is 0).
struct WinArgs {
  const float* table;          // (2197, heads) fp32 relative-position bias table
  int nw[3], ws[3], P[3], sh[3];  // windows per axis, window, padded grid, shift
  int masked;                  // any shift > 0
};

__device__ __forceinline__ int win_axis_label(int p, int P, int ws, int s) { return s == 0 ? 2 : (p < P - ws ? 0 : (p < P - s ? 1 : 2)); }

// c13[t] and label[t] of rows r0 + t (t < 64) of window `w` (global window index; w % windows-per-image locates it)
__device__ __forceinline__ void win_meta(const WinArgs& wa, int w, int r0, int N, int* c13, int* lab) {
  const int t = threadIdx.x;
  if (t >= AT_T) return;
  const int i = r0 + t;
  if (i >= N) {
    c13[t] = 0;
    lab[t] = 0;
    return;
  }
  c13[t] = (i / 49) * 169 + (i / 7 % 7) * 13 + i % 7;
  int l = 0;
  if (wa.masked) {
    const int wl = w % (wa.nw[0] * wa.nw[1] * wa.nw[2]);
    const int wd = wl / (wa.nw[1] * wa.nw[2]), wh = wl / wa.nw[2] % wa.nw[1], ww = wl % wa.nw[2];
    const int id = i / (wa.ws[1] * wa.ws[2]), ih = i / wa.ws[2] % wa.ws[1], iw = i % wa.ws[2];
    l = win_axis_label(wd * wa.ws[0] + id, wa.P[0], wa.ws[0], wa.sh[0]) * 9 +
        win_axis_label(wh * wa.ws[1] + ih, wa.P[1], wa.ws[1], wa.sh[1]) * 3 + win_axis_label(ww * wa.ws[2] + iw, wa.P[2], wa.ws[2], wa.sh[2]);
  }
  lab[t] = l;
}

// the additive term of score (i, j): sm = {c13 q, label q, c13 k, label k} staged by win_meta
__device__ __forceinline__ float win_add(const WinArgs& wa, const int* sm, int i, int j, int hd, int heads) {
  const float b = wa.table[(sm[i] - sm[2 * AT_T + j] + 1098) * heads + hd];
  return sm[AT_T + i] != sm[3 * AT_T + j] ? b - 100.f : b;
}

// The scaled score, rounded ONCE and never fused into a later add.  The forward builds its running maximum and the saved lse from this
// number and the backward recomputes P = expf(score - lse) from it: were the multiply contracted into the subtraction on one side
// only (scale = 32^-0.5 is not a power of two, so the product rounds), a row whose softmax is exactly one-hot would get
// P = expf(rounding error of the score) != 1 in the backward.
__device__ __forceinline__ float scaled_score(float s, float scale) {
#pragma clang fp contract(off)
  return s * scale;
}

template <typename T, int D>
__device__ __forceinline__ void attn_stage(float* s, const T* qkv, long row_stride, int col, int b, int N, int r0) {
  // s[i][c] (pitch D + 1) = qkv[(b * N + r0 + i) * row_stride + col + c], zero past N
  for (int e = threadIdx.x; e < AT_T * D; e += 256) {
    const int i = e / D, c = e % D;
    const int r = r0 + i;
    s[i * (D + 1) + c] = r < N ? to_f32<T>(qkv[((long)b * N + r) * row_stride + col + c]) : 0.f;
  }
}

// S[r][s] = sum_c X[ti + 16 r][c] * Y[tj + 16 s][c]
template <int D>
__device__ __forceinline__ void attn_dot(const float* X, const float* Y, float (&S)[4][4], int ti, int tj) {
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int s = 0; s < 4; ++s) S[r][s] = 0.f;
#pragma unroll 4
  for (int c = 0; c < D; ++c) {
    float a[4], b[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) a[r] = X[(ti + 16 * r) * (D + 1) + c];
#pragma unroll
    for (int s = 0; s < 4; ++s) b[s] = Y[(tj + 16 * s) * (D + 1) + c];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int s = 0; s < 4; ++s) S[r][s] = fmaf(a[r], b[s], S[r][s]);
  }
}

__device__ __forceinline__ float row16_max(float v) {
#pragma unroll
  for (int o = 8; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

__device__ __forceinline__ float row16_sum(float v) {
#pragma unroll
  for (int o = 8; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// grid (ceil(N / 64), heads, B); dynamic LDS: Q, K, V (64 x (D + 1)) and P (64 x 65) floats (+ 4 x 64 ints of window metadata)
template <typename T, int D, bool WIN = false>
__global__ void __launch_bounds__(256) attn_fwd_kernel(const T* __restrict__ qkv, T* __restrict__ out, float* __restrict__ lse, int N,
                                                       int heads, float scale, WinArgs wa) {
  extern __shared__ float smem[];
  constexpr int CU = D / 16;
  float* sQ = smem;
  float* sK = sQ + AT_T * (D + 1);
  float* sV = sK + AT_T * (D + 1);
  float* sP = sV + AT_T * (D + 1);
  int* sM = reinterpret_cast<int*>(sP + AT_T * (AT_T + 1));
  const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
  const int q0 = blockIdx.x * AT_T, hd = blockIdx.y, b = blockIdx.z;
  const int hid = heads * D;
  const long rs = 3L * hid;
  attn_stage<T, D>(sQ, qkv, rs, hd * D, b, N, q0);
  if constexpr (WIN) win_meta(wa, b, q0, N, sM, sM + AT_T);
  float m[4], l[4], acc[4][CU];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    m[r] = -INFINITY;
    l[r] = 0.f;
#pragma unroll
    for (int u = 0; u < CU; ++u) acc[r][u] = 0.f;
  }
  for (int j0 = 0; j0 < N; j0 += AT_T) {
    __syncthreads();
    attn_stage<T, D>(sK, qkv, rs, hid + hd * D, b, N, j0);
    attn_stage<T, D>(sV, qkv, rs, 2 * hid + hd * D, b, N, j0);
    if constexpr (WIN) win_meta(wa, b, j0, N, sM + 2 * AT_T, sM + 3 * AT_T);
    __syncthreads();
    float S[4][4];
    attn_dot<D>(sQ, sK, S, ti, tj);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float mx = -INFINITY;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        float sc = scaled_score(S[r][s], scale);
        if constexpr (WIN) sc += win_add(wa, sM, ti + 16 * r, tj + 16 * s, hd, heads);
        S[r][s] = j0 + tj + 16 * s < N ? sc : -INFINITY;
        mx = fmaxf(mx, S[r][s]);
      }
      const float mn = fmaxf(m[r], row16_max(mx));     // finite: key j0 < N is in every tile
      const float alpha = expf(m[r] - mn);
      float ps = 0.f;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const float pv = expf(S[r][s] - mn);
        sP[(ti + 16 * r) * (AT_T + 1) + tj + 16 * s] = pv;
        ps += pv;
      }
      l[r] = l[r] * alpha + row16_sum(ps);
      m[r] = mn;
#pragma unroll
      for (int u = 0; u < CU; ++u) acc[r][u] *= alpha;
    }
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < AT_T; ++j) {
      float v[CU];
#pragma unroll
      for (int u = 0; u < CU; ++u) v[u] = sV[j * (D + 1) + tj + 16 * u];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float pv = sP[(ti + 16 * r) * (AT_T + 1) + j];
#pragma unroll
        for (int u = 0; u < CU; ++u) acc[r][u] = fmaf(pv, v[u], acc[r][u]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = q0 + ti + 16 * r;
    if (i >= N) continue;
    const float inv = 1.f / l[r];
#pragma unroll
    for (int u = 0; u < CU; ++u) out[((long)b * N + i) * hid + hd * D + tj + 16 * u] = from_f32<T>(acc[r][u] * inv);
    if (tj == 0) lse[((long)b * heads + hd) * N + i] = m[r] + logf(l[r]);
  }
}

// dvec[(b * heads + hd) * N + i] = sum_c dO[b * N + i][hd * D + c] * O[...]
template <typename T>
__global__ void attn_bwd_dvec_kernel(const T* __restrict__ dout, const T* __restrict__ out, float* __restrict__ dvec, int B, int N,
                                     int heads, int D) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)B * heads * N) return;
  const int n = (int)(i % N);
  const long t = i / N;
  const int hd = (int)(t % heads), b = (int)(t / heads);
  const long base = ((long)b * N + n) * heads * D + (long)hd * D;
  float s = 0.f;
  for (int c = 0; c < D; ++c) s += to_f32<T>(dout[base + c]) * to_f32<T>(out[base + c]);
  dvec[i] = s;
}

// P and dS of one (query tile, key tile) pair into sP / sS ([query][key], pitch 65).  sX = Q rows, sY = K rows, sdO, sV as staged.
template <int D, bool WIN = false>
__device__ __forceinline__ void attn_p_ds(const float* sQ, const float* sK, const float* sdO, const float* sV, const float* slse,
                                          const float* sdv, float* sP, float* sS, int ti, int tj, int q0, int j0, int N, float scale,
                                          const WinArgs& wa, const int* sM, int hd, int heads) {
  float S[4][4], dP[4][4];
  attn_dot<D>(sQ, sK, S, ti, tj);
  attn_dot<D>(sdO, sV, dP, ti, tj);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = ti + 16 * r;
    const bool qok = q0 + i < N;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int j = tj + 16 * s;
      float sc = scaled_score(S[r][s], scale);
      if constexpr (WIN) sc += win_add(wa, sM, i, j, hd, heads);
      const float pv = (qok && j0 + j < N) ? expf(sc - slse[i]) : 0.f;
      sP[i * (AT_T + 1) + j] = pv;
      sS[i * (AT_T + 1) + j] = pv * (dP[r][s] - sdv[i]);
    }
  }
}

// grid (ceil(N / 64) key tiles, heads, B); LDS: K, V, Q, dO (64 x (D + 1)), P, dS (64 x 65), lse, dvec (64) (+ 4 x 64 window ints)
template <typename T, int D, bool WIN = false>
__global__ void __launch_bounds__(256) attn_bwd_dkv_kernel(const T* __restrict__ qkv, const T* __restrict__ dout,
                                                           const float* __restrict__ lse, const float* __restrict__ dvec,
                                                           T* __restrict__ dqkv, int N, int heads, float scale, WinArgs wa) {
  extern __shared__ float smem[];
  constexpr int CU = D / 16, PD = AT_T * (D + 1), PP = AT_T * (AT_T + 1);
  float* sK = smem;
  float* sV = sK + PD;
  float* sQ = sV + PD;
  float* sdO = sQ + PD;
  float* sP = sdO + PD;
  float* sS = sP + PP;
  float* slse = sS + PP;
  float* sdv = slse + AT_T;
  int* sM = reinterpret_cast<int*>(sdv + AT_T);
  const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
  const int j0 = blockIdx.x * AT_T, hd = blockIdx.y, b = blockIdx.z;
  const int hid = heads * D;
  const long rs = 3L * hid;
  attn_stage<T, D>(sK, qkv, rs, hid + hd * D, b, N, j0);
  attn_stage<T, D>(sV, qkv, rs, 2 * hid + hd * D, b, N, j0);
  if constexpr (WIN) win_meta(wa, b, j0, N, sM + 2 * AT_T, sM + 3 * AT_T);
  float dK[4][CU], dV[4][CU];       // keys ti + 16 r, channels tj + 16 u
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int u = 0; u < CU; ++u) dK[r][u] = dV[r][u] = 0.f;
  const long sb = ((long)b * heads + hd) * N;
  for (int q0 = 0; q0 < N; q0 += AT_T) {
    __syncthreads();
    attn_stage<T, D>(sQ, qkv, rs, hd * D, b, N, q0);
    attn_stage<T, D>(sdO, dout, hid, hd * D, b, N, q0);
    if (tid < AT_T) {
      slse[tid] = q0 + tid < N ? lse[sb + q0 + tid] : 0.f;
      sdv[tid] = q0 + tid < N ? dvec[sb + q0 + tid] : 0.f;
    }
    if constexpr (WIN) win_meta(wa, b, q0, N, sM, sM + AT_T);
    __syncthreads();
    attn_p_ds<D, WIN>(sQ, sK, sdO, sV, slse, sdv, sP, sS, ti, tj, q0, j0, N, scale, wa, sM, hd, heads);
    __syncthreads();
#pragma unroll 4
    for (int i = 0; i < AT_T; ++i) {
      float dov[CU], qv[CU];
#pragma unroll
      for (int u = 0; u < CU; ++u) {
        dov[u] = sdO[i * (D + 1) + tj + 16 * u];
        qv[u] = sQ[i * (D + 1) + tj + 16 * u];
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float pv = sP[i * (AT_T + 1) + ti + 16 * r];
        const float dsv = sS[i * (AT_T + 1) + ti + 16 * r];
#pragma unroll
        for (int u = 0; u < CU; ++u) {
          dV[r][u] = fmaf(pv, dov[u], dV[r][u]);
          dK[r][u] = fmaf(dsv, qv[u], dK[r][u]);
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int j = j0 + ti + 16 * r;
    if (j >= N) continue;
    T* row = dqkv + ((long)b * N + j) * rs;
#pragma unroll
    for (int u = 0; u < CU; ++u) {
      row[hid + hd * D + tj + 16 * u] = from_f32<T>(dK[r][u] * scale);
      row[2 * hid + hd * D + tj + 16 * u] = from_f32<T>(dV[r][u]);
    }
  }
}

// grid (ceil(N / 64) query tiles, heads, B); LDS as attn_bwd_dkv_kernel
template <typename T, int D, bool WIN = false>
__global__ void __launch_bounds__(256) attn_bwd_dq_kernel(const T* __restrict__ qkv, const T* __restrict__ dout,
                                                          const float* __restrict__ lse, const float* __restrict__ dvec,
                                                          T* __restrict__ dqkv, int N, int heads, float scale, WinArgs wa) {
  extern __shared__ float smem[];
  constexpr int CU = D / 16, PD = AT_T * (D + 1), PP = AT_T * (AT_T + 1);
  float* sK = smem;
  float* sV = sK + PD;
  float* sQ = sV + PD;
  float* sdO = sQ + PD;
  float* sP = sdO + PD;
  float* sS = sP + PP;
  float* slse = sS + PP;
  float* sdv = slse + AT_T;
  int* sM = reinterpret_cast<int*>(sdv + AT_T);
  const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
  const int q0 = blockIdx.x * AT_T, hd = blockIdx.y, b = blockIdx.z;
  const int hid = heads * D;
  const long rs = 3L * hid;
  const long sb = ((long)b * heads + hd) * N;
  attn_stage<T, D>(sQ, qkv, rs, hd * D, b, N, q0);
  attn_stage<T, D>(sdO, dout, hid, hd * D, b, N, q0);
  if (tid < AT_T) {
    slse[tid] = q0 + tid < N ? lse[sb + q0 + tid] : 0.f;
    sdv[tid] = q0 + tid < N ? dvec[sb + q0 + tid] : 0.f;
  }
  if constexpr (WIN) win_meta(wa, b, q0, N, sM, sM + AT_T);
  float dQ[4][CU];                  // queries ti + 16 r, channels tj + 16 u
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int u = 0; u < CU; ++u) dQ[r][u] = 0.f;
  for (int j0 = 0; j0 < N; j0 += AT_T) {
    __syncthreads();
    attn_stage<T, D>(sK, qkv, rs, hid + hd * D, b, N, j0);
    attn_stage<T, D>(sV, qkv, rs, 2 * hid + hd * D, b, N, j0);
    if constexpr (WIN) win_meta(wa, b, j0, N, sM + 2 * AT_T, sM + 3 * AT_T);
    __syncthreads();
    attn_p_ds<D, WIN>(sQ, sK, sdO, sV, slse, sdv, sP, sS, ti, tj, q0, j0, N, scale, wa, sM, hd, heads);
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < AT_T; ++j) {
      float kv[CU];
#pragma unroll
      for (int u = 0; u < CU; ++u) kv[u] = sK[j * (D + 1) + tj + 16 * u];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float dsv = sS[(ti + 16 * r) * (AT_T + 1) + j];
#pragma unroll
        for (int u = 0; u < CU; ++u) dQ[r][u] = fmaf(dsv, kv[u], dQ[r][u]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = q0 + ti + 16 * r;
    if (i >= N) continue;
    T* row = dqkv + ((long)b * N + i) * rs;
#pragma unroll
    for (int u = 0; u < CU; ++u) row[hd * D + tj + 16 * u] = from_f32<T>(dQ[r][u] * scale);
  }
}

// Bias-table gradient, stage 1: partial[g][hd][i][j] = sum over windows w = g, g + G, g + 2 G, ... (in that order) of dS[w][hd][i][j],
// dS = P (dP - dvec), P recomputed as in the backward kernels.  grid (ceil(N / 64) query tiles, ceil(N / 64) key tiles, heads * G);
// LDS as attn_bwd_dkv_kernel.  Every partial element has one writer: no atomics.
template <typename T, int D>
__global__ void __launch_bounds__(256) win_attn_dbias_kernel(const T* __restrict__ qkv, const T* __restrict__ dout,
                                                             const float* __restrict__ lse, const float* __restrict__ dvec,
                                                             float* __restrict__ partial, int nwin, int N, int heads, int G, float scale,
                                                             WinArgs wa) {
  extern __shared__ float smem[];
  constexpr int PD = AT_T * (D + 1), PP = AT_T * (AT_T + 1);
  float* sK = smem;
  float* sV = sK + PD;
  float* sQ = sV + PD;
  float* sdO = sQ + PD;
  float* sP = sdO + PD;
  float* sS = sP + PP;
  float* slse = sS + PP;
  float* sdv = slse + AT_T;
  int* sM = reinterpret_cast<int*>(sdv + AT_T);
  const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
  const int q0 = blockIdx.x * AT_T, j0 = blockIdx.y * AT_T, hd = blockIdx.z % heads, g = blockIdx.z / heads;
  const int hid = heads * D;
  const long rs = 3L * hid;
  float acc[4][4] = {};
  for (int w = g; w < nwin; w += G) {
    __syncthreads();
    attn_stage<T, D>(sQ, qkv, rs, hd * D, w, N, q0);
    attn_stage<T, D>(sdO, dout, hid, hd * D, w, N, q0);
    attn_stage<T, D>(sK, qkv, rs, hid + hd * D, w, N, j0);
    attn_stage<T, D>(sV, qkv, rs, 2 * hid + hd * D, w, N, j0);
    const long sb = ((long)w * heads + hd) * N;
    if (tid < AT_T) {
      slse[tid] = q0 + tid < N ? lse[sb + q0 + tid] : 0.f;
      sdv[tid] = q0 + tid < N ? dvec[sb + q0 + tid] : 0.f;
    }
    win_meta(wa, w, q0, N, sM, sM + AT_T);
    win_meta(wa, w, j0, N, sM + 2 * AT_T, sM + 3 * AT_T);
    __syncthreads();
    attn_p_ds<D, true>(sQ, sK, sdO, sV, slse, sdv, sP, sS, ti, tj, q0, j0, N, scale, wa, sM, hd, heads);
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int s = 0; s < 4; ++s) acc[r][s] += sS[(ti + 16 * r) * (AT_T + 1) + tj + 16 * s];     // this thread's own writes
  }
  float* out = partial + ((long)g * heads + hd) * N * N;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = q0 + ti + 16 * r;
    if (i >= N) continue;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int j = j0 + tj + 16 * s;
      if (j < N) out[(long)i * N + j] = acc[r][s];
    }
  }
}

// Stage 2: dtable[r][hd] = sum over query rows i (ascending) of the key j with rel(i, j) = r, j < N, of sum_g partial[g][hd][i][j]
// (g ascending).  rel is one-to-one in j for fixed i, so each (i, r) names at most one key.  One thread per table entry.
__global__ void win_attn_table_grad_kernel(const float* __restrict__ partial, float* __restrict__ dtable, int N, int heads, int G) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= 2197 * heads) return;
  const int r = e / heads, hd = e % heads;
  const int od = r / 169 - 6, oh = r / 13 % 13 - 6, ow = r % 13 - 6;
  const long plane = (long)heads * N * N;
  float s = 0.f;
  for (int i = 0; i < N; ++i) {
    const int jd = i / 49 - od, jh = i / 7 % 7 - oh, jw = i % 7 - ow;
    if (jd < 0 || jd > 6 || jh < 0 || jh > 6 || jw < 0 || jw > 6) continue;
    const int j = jd * 49 + jh * 7 + jw;
    if (j >= N) continue;
    const float* p = partial + ((long)hd * N + i) * N + j;
    for (int g = 0; g < G; ++g) s += p[g * plane];
  }
  dtable[e] = s;
}

}  // namespace pytc

using namespace pytc;

// ------------------------------------------------------------------------------------------------------------ C ABI
// linear_launch puts the M tiles on gridDim.y: past the device's limit the launch itself would be rejected without a name
constexpr int LG_MAX_M_TILES = 65535;      // conservative: the smallest y limit HIP devices report, not read from the device
static int linear_m_tiles_check(const char* what, int M) {
  const long tiles = ((long)M + LG_BM - 1) / LG_BM;
  PYTC_REQUIRE(tiles <= LG_MAX_M_TILES, "%s: %d rows are %ld row tiles of %d, over the %d tiles one launch takes: split the rows",
               what, M, tiles, LG_BM, LG_MAX_M_TILES);
  return PYTC_OK;
}

template <typename TA, typename TB, typename TC, bool A_T, bool B_T>
static void linear_launch(const LinParams& p, hipStream_t st) {
  dim3 grid(ceil_div(p.N, LG_BN), ceil_div(p.M, LG_BM));
  hipLaunchKernelGGL((linear_gemm_kernel<TA, TB, TC, A_T, B_T>), grid, dim3(256), 0, st, p);
}

extern "C" int pytc_linear_fwd(const void* x, const float* w, const float* bias, const float* pos, int pos_rows, const void* res,
                               void* y, int M, int N, int K, int x_gelu, int dtype, void* stream) {
  PYTC_REQUIRE(x && w && y && M >= 1 && N >= 1 && K >= 1, "linear_fwd: bad arguments");
  PYTC_REQUIRE(!pos || (pos_rows >= 1 && M % pos_rows == 0), "linear_fwd: %d rows are not a whole number of %d-row position blocks",
               M, pos_rows);
  PYTC_CHECK_DTYPE(dtype, "linear_fwd");
  if (int s = linear_m_tiles_check("linear_fwd", M)) return s;
  LinParams p;
  memset(&p, 0, sizeof(p));
  p.A = x; p.B = w; p.C = y; p.bias = bias; p.pos = pos; p.P = pos ? pos_rows : 1; p.res = res; p.gelu_a = x_gelu;
  p.M = M; p.N = N; p.K = K; p.lda = K; p.ldb = K; p.ldc = N;
  hipStream_t st = (hipStream_t)stream;
  PYTC_DISPATCH_DTYPE(dtype, "linear_fwd", T, linear_launch<T, float, T, false, true>(p, st));
  PYTC_LAUNCH_CHECK("linear_fwd");
  return PYTC_OK;
}

extern "C" int pytc_linear_bwd_data(const void* dy, const float* w, const void* x_gelu, void* dx, int M, int N, int K, int dtype,
                                    void* stream) {
  PYTC_REQUIRE(dy && w && dx && M >= 1 && N >= 1 && K >= 1, "linear_bwd_data: bad arguments");
  PYTC_CHECK_DTYPE(dtype, "linear_bwd_data");
  if (int s = linear_m_tiles_check("linear_bwd_data", M)) return s;
  LinParams p;
  memset(&p, 0, sizeof(p));
  // dx[M][K] = dy[M][N] . w[N][K]: the GEMM's (M, N, K) are (M, K, N)
  p.A = dy; p.B = w; p.C = dx; p.M = M; p.N = K; p.K = N; p.lda = N; p.ldb = K; p.ldc = K; p.P = 1;
  p.res = x_gelu; p.res_gelu_bwd = x_gelu ? 1 : 0;
  hipStream_t st = (hipStream_t)stream;
  PYTC_DISPATCH_DTYPE(dtype, "linear_bwd_data", T, linear_launch<T, float, T, false, false>(p, st));
  PYTC_LAUNCH_CHECK("linear_bwd_data");
  return PYTC_OK;
}

extern "C" int pytc_linear_wgrad(const void* dy, const void* x, float* dw, float* db, float* dpos, int pos_rows, int M, int N, int K,
                                 int x_gelu, int dtype, void* stream) {
  PYTC_REQUIRE(dy && x && M >= 1 && N >= 1 && K >= 1, "linear_wgrad: bad arguments");
  PYTC_REQUIRE(!dpos || (pos_rows >= 1 && M % pos_rows == 0), "linear_wgrad: bad position-block rows %d", pos_rows);
  PYTC_CHECK_DTYPE(dtype, "linear_wgrad");
  if (int s = linear_m_tiles_check("linear_wgrad", N)) return s;      // the weight-gradient GEMM's M is the output features
  hipStream_t st = (hipStream_t)stream;
  if (dw) {
    // dw[N][K] = sum_m dy[m][n] x[m][k]: A(n, m) = dy[m][n] (transposed), B(m, k) = x[m][k]; one thread owns each output, K = M
    // summed in order -- no split, no atomics
    LinParams p;
    memset(&p, 0, sizeof(p));
    p.A = dy; p.B = x; p.C = dw; p.M = N; p.N = K; p.K = M; p.lda = N; p.ldb = K; p.ldc = K; p.P = 1; p.gelu_b = x_gelu;
    PYTC_DISPATCH_DTYPE(dtype, "linear_wgrad", T, linear_launch<T, T, float, true, false>(p, st));
  }
  const int blk = 256;
  const long n = (long)pos_rows * N;
  PYTC_DISPATCH_DTYPE(dtype, "linear_wgrad", T,
    if (db) hipLaunchKernelGGL(colsum_period_kernel<T>, dim3(ceil_div(N, blk)), dim3(blk), 0, st, (const T*)dy, db, M, N, 1);
    if (dpos) hipLaunchKernelGGL(colsum_period_kernel<T>, dim3(ceil_div(n, blk)), dim3(blk), 0, st, (const T*)dy, dpos, M, N, pos_rows));
  PYTC_LAUNCH_CHECK("linear_wgrad");
  return PYTC_OK;
}

static int ln_wide_check(const char* what, int64_t rows, int C, int dtype) {
  PYTC_REQUIRE(rows >= 1 && C >= 64 && C <= 64 * LN_MAXV && C % 64 == 0, "%s: C = %d must be a multiple of 64 in [64, %d]", what, C,
               64 * LN_MAXV);
  PYTC_CHECK_DTYPE(dtype, what);
  return PYTC_OK;
}

extern "C" int pytc_layernorm_wide(const void* x, void* y, const float* gamma, const float* beta, int64_t rows, int C, float eps,
                                   int dtype, void* stream) {
  if (int s = ln_wide_check("layernorm_wide", rows, C, dtype)) return s;
  PYTC_REQUIRE(x && y && gamma && beta, "layernorm_wide: null pointer");
  hipStream_t st = (hipStream_t)stream;
  dim3 grid(ceil_div(rows, 4));
  PYTC_DISPATCH_DTYPE(dtype, "layernorm_wide", T,
                      hipLaunchKernelGGL(layernorm_wide_fwd_kernel<T>, grid, dim3(256), 0, st, (const T*)x, (T*)y, gamma, beta, (long)rows, C, eps));
  PYTC_LAUNCH_CHECK("layernorm_wide");
  return PYTC_OK;
}

extern "C" int pytc_layernorm_wide_bwd_slots(int64_t rows) { return ceil_div(rows, LN_ROWS_PER_BLOCK); }

extern "C" int pytc_layernorm_wide_bwd(const void* dy, const void* x, const float* gamma, void* dx, float* partial, float* dgamma,
                                       float* dbeta, int64_t rows, int C, float eps, int dtype, void* stream) {
  if (int s = ln_wide_check("layernorm_wide_bwd", rows, C, dtype)) return s;
  PYTC_REQUIRE(dy && x && gamma && dx && partial, "layernorm_wide_bwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int slots = ceil_div(rows, LN_ROWS_PER_BLOCK);
  PYTC_DISPATCH_DTYPE(dtype, "layernorm_wide_bwd", T,
                      hipLaunchKernelGGL(layernorm_wide_bwd_kernel<T>, dim3(slots), dim3(256), 0, st, (const T*)dy, (const T*)x, gamma, (T*)dx,
                                         partial, (long)rows, C, eps));
  if (dgamma || dbeta)
    hipLaunchKernelGGL(layernorm_wide_reduce_kernel, dim3(ceil_div(2 * C, 256)), dim3(256), 0, st, (const float*)partial, dgamma, dbeta,
                       slots, C);
  PYTC_LAUNCH_CHECK("layernorm_wide_bwd");
  return PYTC_OK;
}

extern "C" int pytc_patch_gather16(const void* src, void* dst, int B, int D, int H, int W, int C, int scatter, int dtype, void* stream) {
  PYTC_REQUIRE(src && dst && B >= 1 && C >= 1 && D >= 16 && H >= 16 && W >= 16 && D % 16 == 0 && H % 16 == 0 && W % 16 == 0,
               "patch_gather16: grid (%d, %d, %d) is not a whole number of 16^3 patches", D, H, W);
  hipStream_t st = (hipStream_t)stream;
  const long total = (long)B * D * H * W * C;
  const int grid = (int)std::min<long>((total + 255) / 256, 16384);
  PYTC_DISPATCH_DTYPE(dtype, "patch_gather16", T,
                      hipLaunchKernelGGL(patch_gather_kernel<T>, dim3(grid), dim3(256), 0, st, (const T*)src, (T*)dst, B, D, H, W, C, scatter));
  PYTC_LAUNCH_CHECK("patch_gather16");
  return PYTC_OK;
}

extern "C" int pytc_attention_supported(int d_head) { return d_head == 32 || d_head == 64; }

static int attn_check(const char* what, int B, int N, int heads, int d_head, int dtype) {
  PYTC_REQUIRE(B >= 1 && N >= 1 && heads >= 1, "%s: bad sizes", what);
  PYTC_REQUIRE(pytc_attention_supported(d_head), "%s: head width %d has no kernel (32, 64)", what, d_head);
  PYTC_CHECK_DTYPE(dtype, what);
  return PYTC_OK;
}

template <typename T, int D>
static void attn_fwd_launch(const void* qkv, void* out, float* lse, int B, int N, int heads, float scale, hipStream_t st) {
  const size_t lds = (3 * AT_T * (D + 1) + AT_T * (AT_T + 1)) * sizeof(float);
  const void* k = reinterpret_cast<const void*>(&attn_fwd_kernel<T, D>);
  if (!ensure_dynamic_lds(k, lds, "attention_fwd")) return;
  hipLaunchKernelGGL((attn_fwd_kernel<T, D>), dim3(ceil_div(N, AT_T), heads, B), dim3(256), lds, st, (const T*)qkv, (T*)out, lse, N,
                     heads, scale, WinArgs{});
}

extern "C" int pytc_attention_fwd(const void* qkv, void* out, float* lse, int B, int N, int heads, int d_head, float scale, int dtype,
                                  void* stream) {
  if (int s = attn_check("attention_fwd", B, N, heads, d_head, dtype)) return s;
  PYTC_REQUIRE(qkv && out && lse, "attention_fwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  PYTC_DISPATCH_DTYPE(dtype, "attention_fwd", T,
                      if (d_head == 64) attn_fwd_launch<T, 64>(qkv, out, lse, B, N, heads, scale, st);
                      else attn_fwd_launch<T, 32>(qkv, out, lse, B, N, heads, scale, st));
  PYTC_LAUNCH_CHECK("attention_fwd");
  return PYTC_OK;
}

template <typename T, int D>
static void attn_bwd_launch(const void* qkv, const void* out, const void* dout, const float* lse, float* dvec, void* dqkv, int B, int N,
                            int heads, float scale, hipStream_t st) {
  const size_t lds = (4 * AT_T * (D + 1) + 2 * AT_T * (AT_T + 1) + 2 * AT_T) * sizeof(float);
  const long rows = (long)B * heads * N;
  hipLaunchKernelGGL(attn_bwd_dvec_kernel<T>, dim3(ceil_div(rows, 256)), dim3(256), 0, st, (const T*)dout, (const T*)out, dvec, B, N,
                     heads, D);
  const void* kkv = reinterpret_cast<const void*>(&attn_bwd_dkv_kernel<T, D>);
  const void* kq = reinterpret_cast<const void*>(&attn_bwd_dq_kernel<T, D>);
  if (!ensure_dynamic_lds(kkv, lds, "attention_bwd") || !ensure_dynamic_lds(kq, lds, "attention_bwd")) return;
  dim3 grid(ceil_div(N, AT_T), heads, B);
  hipLaunchKernelGGL((attn_bwd_dkv_kernel<T, D>), grid, dim3(256), lds, st, (const T*)qkv, (const T*)dout, lse, (const float*)dvec,
                     (T*)dqkv, N, heads, scale, WinArgs{});
  hipLaunchKernelGGL((attn_bwd_dq_kernel<T, D>), grid, dim3(256), lds, st, (const T*)qkv, (const T*)dout, lse, (const float*)dvec,
                     (T*)dqkv, N, heads, scale, WinArgs{});
}

extern "C" int pytc_attention_bwd(const void* qkv, const void* out, const void* dout, const float* lse, float* dvec, void* dqkv, int B,
                                  int N, int heads, int d_head, float scale, int dtype, void* stream) {
  if (int s = attn_check("attention_bwd", B, N, heads, d_head, dtype)) return s;
  PYTC_REQUIRE(qkv && out && dout && lse && dvec && dqkv, "attention_bwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  PYTC_DISPATCH_DTYPE(dtype, "attention_bwd", T,
                      if (d_head == 64) attn_bwd_launch<T, 64>(qkv, out, dout, lse, dvec, dqkv, B, N, heads, scale, st);
                      else attn_bwd_launch<T, 32>(qkv, out, dout, lse, dvec, dqkv, B, N, heads, scale, st));
  PYTC_LAUNCH_CHECK("attention_bwd");
  return PYTC_OK;
}

// ------------------------------------------------------------------------------------------ shifted-window attention (Swin)
extern "C" int pytc_window_attention_supported(int d_head) { return d_head == 16 || d_head == 32; }

// G window groups of the bias-table gradient: enough (query tile, key tile, head, group) blocks to fill the GPU, at most nwin
extern "C" int pytc_window_attention_bias_groups(int nwin, int N, int heads) {
  const int tiles = ceil_div(N, AT_T) * ceil_div(N, AT_T) * std::max(heads, 1);
  return std::max(1, std::min(nwin, ceil_div(2048, tiles)));
}

// geom = {windows per axis (3), window (3), padded grid (3), shift (3)} of one image; nwin = images * windows per image
static int win_args(const char* what, const float* table, const int* geom, int nwin, int N, int heads, int d_head, int dtype,
                    WinArgs* wa) {
  PYTC_REQUIRE(table && geom && nwin >= 1 && heads >= 1, "%s: bad arguments", what);
  PYTC_REQUIRE(pytc_window_attention_supported(d_head), "%s: head width %d has no kernel (16, 32)", what, d_head);
  PYTC_CHECK_DTYPE(dtype, what);
  memset(wa, 0, sizeof(*wa));
  wa->table = table;
  int per_img = 1, n = 1;
  for (int a = 0; a < 3; ++a) {
    wa->nw[a] = geom[a]; wa->ws[a] = geom[3 + a]; wa->P[a] = geom[6 + a]; wa->sh[a] = geom[9 + a];
    PYTC_REQUIRE(wa->ws[a] >= 1 && wa->ws[a] <= 7 && wa->nw[a] >= 1 && wa->nw[a] * wa->ws[a] == wa->P[a] && wa->sh[a] >= 0 &&
                 wa->sh[a] < wa->ws[a], "%s: axis %d: %d windows of %d over a padded %d with shift %d is not a window grid", what, a,
                 wa->nw[a], wa->ws[a], wa->P[a], wa->sh[a]);
    per_img *= wa->nw[a];
    n *= wa->ws[a];
    wa->masked |= wa->sh[a] > 0;
  }
  PYTC_REQUIRE(n == N && nwin % per_img == 0, "%s: %d windows of %d tokens do not fit the geometry (%d-token windows, %d per image)",
               what, nwin, N, n, per_img);
  return PYTC_OK;
}

static size_t win_fwd_lds(int D) { return (3 * AT_T * (D + 1) + AT_T * (AT_T + 1) + 4 * AT_T) * sizeof(float); }
static size_t win_bwd_lds(int D) { return (4 * AT_T * (D + 1) + 2 * AT_T * (AT_T + 1) + 2 * AT_T + 4 * AT_T) * sizeof(float); }

template <typename T, int D>
static void win_fwd_launch(const void* qkv, void* out, float* lse, int nwin, int N, int heads, float scale, const WinArgs& wa,
                           hipStream_t st) {
  const size_t lds = win_fwd_lds(D);
  const void* k = reinterpret_cast<const void*>(&attn_fwd_kernel<T, D, true>);
  if (!ensure_dynamic_lds(k, lds, "window_attention_fwd")) return;
  hipLaunchKernelGGL((attn_fwd_kernel<T, D, true>), dim3(ceil_div(N, AT_T), heads, nwin), dim3(256), lds, st, (const T*)qkv, (T*)out,
                     lse, N, heads, scale, wa);
}

extern "C" int pytc_window_attention_fwd(const void* qkv, const float* table, const int* geom, void* out, float* lse, int nwin, int N,
                                         int heads, int d_head, float scale, int dtype, void* stream) {
  WinArgs wa;
  if (int s = win_args("window_attention_fwd", table, geom, nwin, N, heads, d_head, dtype, &wa)) return s;
  PYTC_REQUIRE(qkv && out && lse, "window_attention_fwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  PYTC_DISPATCH_DTYPE(dtype, "window_attention_fwd", T,
                      if (d_head == 16) win_fwd_launch<T, 16>(qkv, out, lse, nwin, N, heads, scale, wa, st);
                      else win_fwd_launch<T, 32>(qkv, out, lse, nwin, N, heads, scale, wa, st));
  PYTC_LAUNCH_CHECK("window_attention_fwd");
  return PYTC_OK;
}

template <typename T, int D>
static void win_bwd_launch(const void* qkv, const void* out, const void* dout, const float* lse, float* dvec, void* dqkv, float* partial,
                           float* dtable, int nwin, int N, int heads, float scale, const WinArgs& wa, hipStream_t st) {
  const size_t lds = win_bwd_lds(D);
  const long rows = (long)nwin * heads * N;
  hipLaunchKernelGGL(attn_bwd_dvec_kernel<T>, dim3(ceil_div(rows, 256)), dim3(256), 0, st, (const T*)dout, (const T*)out, dvec, nwin, N,
                     heads, D);
  const void* kkv = reinterpret_cast<const void*>(&attn_bwd_dkv_kernel<T, D, true>);
  const void* kq = reinterpret_cast<const void*>(&attn_bwd_dq_kernel<T, D, true>);
  const void* kb = reinterpret_cast<const void*>(&win_attn_dbias_kernel<T, D>);
  if (!ensure_dynamic_lds(kkv, lds, "window_attention_bwd") || !ensure_dynamic_lds(kq, lds, "window_attention_bwd") ||
      !ensure_dynamic_lds(kb, lds, "window_attention_bwd"))
    return;
  dim3 grid(ceil_div(N, AT_T), heads, nwin);
  hipLaunchKernelGGL((attn_bwd_dkv_kernel<T, D, true>), grid, dim3(256), lds, st, (const T*)qkv, (const T*)dout, lse, (const float*)dvec,
                     (T*)dqkv, N, heads, scale, wa);
  hipLaunchKernelGGL((attn_bwd_dq_kernel<T, D, true>), grid, dim3(256), lds, st, (const T*)qkv, (const T*)dout, lse, (const float*)dvec,
                     (T*)dqkv, N, heads, scale, wa);
  if (dtable) {
    const int G = pytc_window_attention_bias_groups(nwin, N, heads);
    hipLaunchKernelGGL((win_attn_dbias_kernel<T, D>), dim3(ceil_div(N, AT_T), ceil_div(N, AT_T), heads * G), dim3(256), lds, st,
                       (const T*)qkv, (const T*)dout, lse, (const float*)dvec, partial, nwin, N, heads, G, scale, wa);
    hipLaunchKernelGGL(win_attn_table_grad_kernel, dim3(ceil_div(2197L * heads, 256)), dim3(256), 0, st, (const float*)partial, dtable, N,
                       heads, G);
  }
}

extern "C" int pytc_window_attention_bwd(const void* qkv, const float* table, const int* geom, const void* out, const void* dout,
                                         const float* lse, float* dvec, void* dqkv, float* partial, float* dtable, int nwin, int N,
                                         int heads, int d_head, float scale, int dtype, void* stream) {
  WinArgs wa;
  if (int s = win_args("window_attention_bwd", table, geom, nwin, N, heads, d_head, dtype, &wa)) return s;
  PYTC_REQUIRE(qkv && out && dout && lse && dvec && dqkv && (!dtable || partial), "window_attention_bwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  PYTC_DISPATCH_DTYPE(dtype, "window_attention_bwd", T,
                      if (d_head == 16) win_bwd_launch<T, 16>(qkv, out, dout, lse, dvec, dqkv, partial, dtable, nwin, N, heads, scale, wa, st);
                      else win_bwd_launch<T, 32>(qkv, out, dout, lse, dvec, dqkv, partial, dtable, nwin, N, heads, scale, wa, st));
  PYTC_LAUNCH_CHECK("window_attention_bwd");
  return PYTC_OK;
}
