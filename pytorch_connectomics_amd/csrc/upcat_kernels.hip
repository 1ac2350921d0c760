// MONAI UpCat on the MI355X: ConvTranspose3d(k 2, s 2, p 0) + replicate pad to the skip's size + channel concat [skip, up], fused.
//
// Reference: monai.networks.nets.basic_unet.UpCat (UpSample(mode="deconv") -> F.pad(..., "replicate") -> torch.cat([x_e, x_0], 1)),
// the decoder block of the reference's `monai_basic_unet3d` (connectomics/models/architectures/monai_models.py:142-194).
//
// A k2/s2/p0 transposed conv has no overlapping taps: output voxel (2z+a, 2y+b, 2x+c) is ONE matrix product of the input row
// x_low[z,y,x,:] with the weight slice W[:, :, a, b, c].  So the whole up-sampling is one GEMM
//     G[r][j] = sum_i x_low[r][i] * W[i][o][par],     r = low voxel, j = par * C_u + o, par = 4a + 2b + c      (rows x 8 C_u)
// whose epilogue scatters column block `par` of row r to its output voxel, at channel offset C_e of the concat buffer (row stride
// C_e + C_u), and once more to the replicated face when the skip is one voxel longer on an axis (D = 2d + 1: plane 2d is a copy of
// plane 2d - 1, which is parity a = 1 of low plane d - 1).  Neither the up tensor nor a padded copy of it exists.
//
// Backward (the adjoint of each piece):
//   dx_e  = dcat[..., :C_e]                                               (upcat_copy_channels_kernel)
//   G'[r][j] = dcat[child(r, par), C_e + o] (+ the replicated faces' gradients folded into the last plane: at most 8 terms, summed
//              in a fixed order in fp32)                                  (gather prologue of the two GEMMs below)
//   dx_low = G' . W^T      rows x C_in, K = 8 C_u                          (upcat_gemm_kernel<DGRAD>)
//   dW     = x_low^T . G'  C_in x 8 C_u, K = rows: split-K partials over fixed row ranges, then a fixed-order reduction; an extra
//            all-ones row of x_low^T makes the same launch produce sum_r G' = the bias gradient's summands
//                                                                          (upcat_gemm_kernel<WGRAD> + upcat_wgrad_reduce_kernel)
// No atomics anywhere: every result is bit-reproducible.
//
// The GEMM: a workgroup (4 waves) owns a 64 (P) x 64 (Q) output tile, each wave 32 x 32 = 2 x 2 MFMA 16x16 tiles
// (v_mfma_f32_16x16x32_bf16 / 4 x v_mfma_f32_16x16x4f32).  Both operands are staged through LDS per k step (32 bf16 / 16 fp32 k),
// the loads of step k+1 held in registers during the MFMAs of step k.  Every operand load is masked, so C_in, C_e, C_u need not be
// multiples of anything: the K tail is zero-filled inside the kernel.  P is the MFMA A operand: a lane ends with 4 consecutive P
// indices of one Q index -- 4 consecutive up channels of one voxel (FWD), 4 consecutive input channels of one low row (DGRAD).
#include <algorithm>

#include "pw_common.h"

namespace pytc {

enum UpcatMode { UPCAT_FWD = 0, UPCAT_DGRAD = 1, UPCAT_WGRAD = 2 };

struct UpcatParams {
  const void* x_low;     // [rows][C_in] (FWD operand, WGRAD P operand)
  const float* w;        // ConvTranspose3d weight, fp32 [C_in][C_u][2][2][2]
  const float* bias;     // [C_u] or null (FWD)
  const void* dcat;      // [N*D*H*W][C_e + C_u] (DGRAD / WGRAD)
  void* out;             // FWD: cat; DGRAD: dx_low [rows][C_in]; WGRAD: fp32 partials [S][C_in + 1][8 C_u]
  int N, d, h, w_, D, H, W;
  int C_in, C_e, C_u;
  int up_off, Ct;        // channel offset of the up half and row stride of the concat buffer ([skip, up]: C_e, C_e + C_u)
  int rows;              // N * d * h * w
  int rows_per_split;    // WGRAD: K range of one split (multiple of the k step)
};

constexpr int UP_BP = 64, UP_BQ = 64;
// the forward and data-gradient launches put the row tiles on gridDim.y.  65535 is a conservative constant, the smallest y limit HIP
// devices report (maxGridSize[1]); it is not read from the device, so a device that would take more is refused as well
constexpr int UP_MAX_ROW_TILES = 65535;

// child voxel of low voxel r for parity (0, 0, 0), and the replicated-face flags (bit 0: z, 1: y, 2: x) of its last planes
__device__ __forceinline__ void upcat_row_info(const UpcatParams& p, int r, int& vbase, int& flags) {
  const unsigned ur = (unsigned)r;
  const unsigned x = ur % (unsigned)p.w_;
  unsigned t = ur / (unsigned)p.w_;
  const unsigned y = t % (unsigned)p.h;
  t /= (unsigned)p.h;
  const unsigned z = t % (unsigned)p.d;
  const unsigned n = t / (unsigned)p.d;
  vbase = (((int)n * p.D + 2 * (int)z) * p.H + 2 * (int)y) * p.W + 2 * (int)x;
  flags = ((int)z == p.d - 1 && p.D == 2 * p.d + 1 ? 1 : 0) | ((int)y == p.h - 1 && p.H == 2 * p.h + 1 ? 2 : 0) |
          ((int)x == p.w_ - 1 && p.W == 2 * p.w_ + 1 ? 4 : 0);
}

// gradient of the up tensor at (row, parity, channel o): the child's dcat plus the faces replicated from it, fixed order
template <typename T>
__device__ __forceinline__ float upcat_gather(const UpcatParams& p, int vbase, int flags, int par, int o) {
  const int a = par >> 2, b = (par >> 1) & 1, c = par & 1;
  const int Ct = p.Ct;
  const int HW = p.H * p.W;
  const int v = vbase + a * HW + b * p.W + c;
  const int ez = (a & flags) ? 1 : 0, ey = (b && (flags & 2)) ? 1 : 0, ex = (c && (flags & 4)) ? 1 : 0;
  const T* g = reinterpret_cast<const T*>(p.dcat) + p.up_off + o;
  float s = 0.f;
  for (int zz = 0; zz <= ez; ++zz)
    for (int yy = 0; yy <= ey; ++yy)
      for (int xx = 0; xx <= ex; ++xx) s += to_f32<T>(g[(long)(v + zz * HW + yy * p.W + xx) * Ct]);
  return s;
}

template <typename T, int MODE>
__global__ void __launch_bounds__(256, 2) upcat_gemm_kernel(UpcatParams p) {
  typedef Mma<T> M;
  constexpr int KS = M::KSTEP;                 // 32 (bf16) / 16 (fp32)
  constexpr int EPL = M::EPL;                  // 8 / 4
  constexpr int PITCH = KS + (sizeof(T) == 2 ? 8 : 4);   // 80-byte rows: the 16 rows of a fragment read hit distinct banks
  constexpr int PER = UP_BP * KS / 256;        // staged elements per thread and operand
  __shared__ __attribute__((aligned(16))) T sP[UP_BP * PITCH];
  __shared__ __attribute__((aligned(16))) T sQ[UP_BQ * PITCH];
  __shared__ int sVb[UP_BQ], sFl[UP_BQ];

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wp = wave & 1, wq = wave >> 1;
  const int r16 = lane & 15, kb = lane >> 4;
  const int Cu8 = 8 * p.C_u;
  // P / Q extents and the K range of this workgroup
  const int Pdim = MODE == UPCAT_FWD ? Cu8 : (MODE == UPCAT_DGRAD ? p.C_in : p.C_in + 1);
  const int Qdim = MODE == UPCAT_WGRAD ? Cu8 : p.rows;
  const int P0 = blockIdx.x * UP_BP, Q0 = blockIdx.y * UP_BQ;
  int k_begin = 0, k_end = MODE == UPCAT_FWD ? p.C_in : (MODE == UPCAT_DGRAD ? Cu8 : p.rows);
  if (MODE == UPCAT_WGRAD) {
    k_begin = blockIdx.z * p.rows_per_split;
    k_end = min(p.rows, k_begin + p.rows_per_split);
  }

  if (MODE != UPCAT_WGRAD) {           // the 64 low rows of this tile: voxel bases and face flags, once
    if (tid < UP_BQ) {
      const int r = Q0 + tid;
      int vb = 0, fl = 0;
      if (r < p.rows) upcat_row_info(p, r, vb, fl);
      sVb[tid] = vb;
      sFl[tid] = fl;
    }
    __syncthreads();
  }

  // ---- staging: element e = tid + 256 q of a 64 x KS tile.  k-fast (k = e % KS) where the operand is contiguous along k,
  // index-fast (idx = e % 64) where it is contiguous along the P / Q index (WGRAD: both operands run over rows along k)
  float pv[PER], qv[PER];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int e = tid + 256 * q;
      int ip, kk;
      if (MODE == UPCAT_WGRAD) { ip = e % UP_BP; kk = e / UP_BP; }
      else { kk = e % KS; ip = e / KS; }
      const int k = k0 + kk, P = P0 + ip, Q = Q0 + ip;
      float a = 0.f, b = 0.f;
      if (MODE == UPCAT_FWD) {
        if (k < k_end && P < Pdim) {
          const int par = P / p.C_u, o = P - par * p.C_u;
          a = p.w[((long)k * p.C_u + o) * 8 + par];
        }
        if (k < k_end && Q < Qdim) b = to_f32<T>(reinterpret_cast<const T*>(p.x_low)[(long)Q * p.C_in + k]);
      } else if (MODE == UPCAT_DGRAD) {
        const int par = k / p.C_u, o = k - par * p.C_u;
        if (k < k_end && P < Pdim) a = p.w[((long)P * p.C_u + o) * 8 + par];
        if (k < k_end && Q < Qdim) b = upcat_gather<T>(p, sVb[ip], sFl[ip], par, o);
      } else {
        if (k < k_end && P < Pdim) a = P < p.C_in ? to_f32<T>(reinterpret_cast<const T*>(p.x_low)[(long)k * p.C_in + P]) : 1.f;
        if (k < k_end && Q < Qdim) {
          int vb, fl;
          upcat_row_info(p, k, vb, fl);
          const int par = Q / p.C_u, o = Q - par * p.C_u;
          b = upcat_gather<T>(p, vb, fl, par, o);
        }
      }
      pv[q] = a;
      qv[q] = b;
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int e = tid + 256 * q;
      int ip, kk;
      if (MODE == UPCAT_WGRAD) { ip = e % UP_BP; kk = e / UP_BP; }
      else { kk = e % KS; ip = e / KS; }
      sP[ip * PITCH + kk] = from_f32<T>(pv[q]);
      sQ[ip * PITCH + kk] = from_f32<T>(qv[q]);
    }
  };

  f32x4_t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  if (k_begin < k_end) {
    fetch(k_begin);
    commit();
    __syncthreads();
    for (int k0 = k_begin; k0 < k_end; k0 += KS) {
      const bool more = k0 + KS < k_end;
      if (more) fetch(k0 + KS);
      typename M::frag_t af[2], bfr[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        af[t] = *reinterpret_cast<const typename M::frag_t*>(&sP[(wp * 32 + t * 16 + r16) * PITCH + kb * EPL]);
        bfr[t] = *reinterpret_cast<const typename M::frag_t*>(&sQ[(wq * 32 + t * 16 + r16) * PITCH + kb * EPL]);
      }
#pragma unroll
      for (int tp = 0; tp < 2; ++tp)
#pragma unroll
        for (int tq = 0; tq < 2; ++tq) acc[tp][tq] = M::mma(af[tp], bfr[tq], acc[tp][tq]);
      __syncthreads();
      if (more) {
        commit();
        __syncthreads();
      }
    }
  }

  // ---- epilogue: acc[tp][tq][v] = result (P = P0 + wp*32 + tp*16 + 4 kb + v, Q = Q0 + wq*32 + tq*16 + r16)
#pragma unroll
  for (int tq = 0; tq < 2; ++tq) {
    const int ql = wq * 32 + tq * 16 + r16;
    const int Q = Q0 + ql;
    if (Q >= Qdim) continue;
#pragma unroll
    for (int tp = 0; tp < 2; ++tp) {
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int P = P0 + wp * 32 + tp * 16 + 4 * kb + v;
        if (P >= Pdim) continue;
        const float val = acc[tp][tq][v];
        if (MODE == UPCAT_FWD) {
          const int par = P / p.C_u, o = P - par * p.C_u;
          const int a = par >> 2, b = (par >> 1) & 1, c = par & 1;
          const int fl = sFl[ql];
          const int HW = p.H * p.W, Ct = p.Ct;
          const int vx = sVb[ql] + a * HW + b * p.W + c;
          const int ez = (a & fl) ? 1 : 0, ey = (b && (fl & 2)) ? 1 : 0, ex = (c && (fl & 4)) ? 1 : 0;
          const T out = from_f32<T>(val + (p.bias ? p.bias[o] : 0.f));
          T* dst = reinterpret_cast<T*>(p.out) + p.up_off + o;
          for (int zz = 0; zz <= ez; ++zz)
            for (int yy = 0; yy <= ey; ++yy)
              for (int xx = 0; xx <= ex; ++xx) dst[(long)(vx + zz * HW + yy * p.W + xx) * Ct] = out;
        } else if (MODE == UPCAT_DGRAD) {
          reinterpret_cast<T*>(p.out)[(long)Q * p.C_in + P] = from_f32<T>(val);
        } else {
          reinterpret_cast<float*>(p.out)[((long)blockIdx.z * Pdim + P) * Cu8 + Q] = val;
        }
      }
    }
  }
}

// dst[v][dst_off + c] = src[v][src_off + c], c < C: the skip half of the concat buffer (forward) and dx_e (backward)
template <typename T>
__global__ void upcat_copy_channels_kernel(const T* __restrict__ src, T* __restrict__ dst, long voxels, int C, int src_stride,
                                           int src_off, int dst_stride, int dst_off) {
  const long total = voxels * C;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long v = i / C;
    const int c = (int)(i - v * C);
    dst[v * dst_stride + dst_off + c] = src[v * src_stride + src_off + c];
  }
}

// dW[i][o][par] = sum_s part[s][i][par * C_u + o];  db[o] = sum_par sum_s part[s][C_in][par * C_u + o]  (fixed orders)
__global__ void upcat_wgrad_reduce_kernel(const float* __restrict__ part, float* __restrict__ dw, float* __restrict__ db, int S,
                                          int C_in, int C_u) {
  const int Cu8 = 8 * C_u;
  const long nw = (long)C_in * Cu8;
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride_s = (long)(C_in + 1) * Cu8;
  if (t < nw) {
    const int i = (int)(t / Cu8), j = (int)(t - (long)i * Cu8);
    const int par = j / C_u, o = j - par * C_u;
    float s = 0.f;
    for (int k = 0; k < S; ++k) s += part[k * stride_s + t];
    dw[((long)i * C_u + o) * 8 + par] = s;
  } else if (db && t < nw + C_u) {
    const int o = (int)(t - nw);
    float s = 0.f;
    for (int par = 0; par < 8; ++par) {
      float sp = 0.f;
      for (int k = 0; k < S; ++k) sp += part[k * stride_s + (long)C_in * Cu8 + par * C_u + o];
      s += sp;
    }
    db[o] = s;
  }
}

}  // namespace pytc

using namespace pytc;

static int upcat_check(const char* what, int N, int d, int h, int w, int D, int H, int W, int C_in, int C_e, int C_u, int dtype) {
  PYTC_REQUIRE(N >= 1 && d >= 1 && h >= 1 && w >= 1 && C_in >= 1 && C_e >= 1 && C_u >= 1, "%s: bad sizes", what);
  PYTC_REQUIRE((D == 2 * d || D == 2 * d + 1) && (H == 2 * h || H == 2 * h + 1) && (W == 2 * w || W == 2 * w + 1),
               "%s: skip grid (%d, %d, %d) is neither twice nor twice + 1 the low grid (%d, %d, %d)", what, D, H, W, d, h, w);
  PYTC_REQUIRE((long)N * D * H * W < (1L << 31), "%s: too many voxels for 32-bit voxel indices", what);
  PYTC_CHECK_DTYPE(dtype, what);
  return PYTC_OK;
}

// the row tiles of the FWD / DGRAD launches are gridDim.y: past the device's limit the launch itself would be rejected without a name
static int upcat_row_tiles_check(const char* what, int N, int d, int h, int w) {
  const long rows = (long)N * d * h * w;
  const long tiles = (rows + UP_BQ - 1) / UP_BQ;          // in long: ceil_div narrows to int
  PYTC_REQUIRE(tiles <= UP_MAX_ROW_TILES,
               "%s: %ld low-resolution rows are %ld row tiles of %d, over the %d tiles one launch takes: split the batch", what, rows,
               tiles, UP_BQ, UP_MAX_ROW_TILES);
  return PYTC_OK;
}

static UpcatParams upcat_params(int N, int d, int h, int w, int D, int H, int W, int C_in, int C_e, int C_u) {
  UpcatParams p;
  memset(&p, 0, sizeof(p));
  p.N = N; p.d = d; p.h = h; p.w_ = w; p.D = D; p.H = H; p.W = W;
  p.C_in = C_in; p.C_e = C_e; p.C_u = C_u;
  p.up_off = C_e; p.Ct = C_e + C_u;
  p.rows = N * d * h * w;
  return p;
}

template <typename T>
static void upcat_copy(const void* src, void* dst, long voxels, int C, int ss, int so, int ds, int dof, hipStream_t st) {
  const long total = voxels * C;
  const int grid = (int)std::min<long>((total + 255) / 256, 8192);
  hipLaunchKernelGGL(upcat_copy_channels_kernel<T>, dim3(grid), dim3(256), 0, st, (const T*)src, (T*)dst, voxels, C, ss, so, ds, dof);
}

extern "C" int pytc_upcat_deconv2_fwd(const void* x_low, const float* w, const float* bias, const void* x_e, void* cat, int N, int d,
                                      int h, int wd, int D, int H, int W, int C_in, int C_e, int C_u, int dtype, void* stream) {
  if (int st = upcat_check("upcat_deconv2_fwd", N, d, h, wd, D, H, W, C_in, C_e, C_u, dtype)) return st;
  if (int st = upcat_row_tiles_check("upcat_deconv2_fwd", N, d, h, wd)) return st;
  PYTC_REQUIRE(x_low && w && x_e && cat, "upcat_deconv2_fwd: null pointer");
  UpcatParams p = upcat_params(N, d, h, wd, D, H, W, C_in, C_e, C_u);
  p.x_low = x_low; p.w = w; p.bias = bias; p.out = cat;
  hipStream_t st = (hipStream_t)stream;
  const long vox = (long)N * D * H * W;
  dim3 grid(ceil_div(8L * C_u, UP_BP), ceil_div(p.rows, UP_BQ));
  PYTC_DISPATCH_DTYPE(dtype, "upcat_deconv2_fwd", T,
                      upcat_copy<T>(x_e, cat, vox, C_e, C_e, 0, C_e + C_u, 0, st);
                      hipLaunchKernelGGL((upcat_gemm_kernel<T, UPCAT_FWD>), grid, dim3(256), 0, st, p));
  PYTC_LAUNCH_CHECK("upcat_deconv2_fwd");
  return PYTC_OK;
}

extern "C" int pytc_upcat_deconv2_bwd_data(const void* dcat, const float* w, void* dx_e, void* dx_low, int N, int d, int h, int wd,
                                           int D, int H, int W, int C_in, int C_e, int C_u, int dtype, void* stream) {
  if (int st = upcat_check("upcat_deconv2_bwd_data", N, d, h, wd, D, H, W, C_in, C_e, C_u, dtype)) return st;
  if (int st = upcat_row_tiles_check("upcat_deconv2_bwd_data", N, d, h, wd)) return st;
  PYTC_REQUIRE(dcat && w, "upcat_deconv2_bwd_data: null pointer");
  UpcatParams p = upcat_params(N, d, h, wd, D, H, W, C_in, C_e, C_u);
  p.w = w; p.dcat = dcat; p.out = dx_low;
  hipStream_t st = (hipStream_t)stream;
  const long vox = (long)N * D * H * W;
  dim3 grid(ceil_div(C_in, UP_BP), ceil_div(p.rows, UP_BQ));
  PYTC_DISPATCH_DTYPE(dtype, "upcat_deconv2_bwd_data", T,
                      if (dx_e) upcat_copy<T>(dcat, dx_e, vox, C_e, C_e + C_u, 0, C_e, 0, st);
                      if (dx_low) hipLaunchKernelGGL((upcat_gemm_kernel<T, UPCAT_DGRAD>), grid, dim3(256), 0, st, p));
  PYTC_LAUNCH_CHECK("upcat_deconv2_bwd_data");
  return PYTC_OK;
}

// split count of the weight-gradient GEMM: about 512 workgroups in all, at least one k step of rows per split, at most 64 splits
static int upcat_wgrad_splits(int rows, int C_in, int C_u, int ks) {
  const long tiles = (long)ceil_div(C_in + 1, UP_BP) * ceil_div(8L * C_u, UP_BQ);
  long s = (512 + tiles - 1) / tiles;
  s = std::min<long>(s, std::min<long>(64, ceil_div(rows, ks)));
  return (int)std::max<long>(s, 1);
}

extern "C" int64_t pytc_upcat_deconv2_wgrad_ws_elems(int rows, int C_in, int C_u, int dtype) {
  const int ks = mfma_kstep(dtype);
  return (int64_t)upcat_wgrad_splits(rows, C_in, C_u, ks) * (C_in + 1) * 8 * C_u;
}

extern "C" int pytc_upcat_deconv2_wgrad(const void* x_low, const void* dcat, float* workspace, float* dw, float* db, int N, int d, int h,
                                        int wd, int D, int H, int W, int C_in, int C_e, int C_u, int dtype, void* stream) {
  if (int st = upcat_check("upcat_deconv2_wgrad", N, d, h, wd, D, H, W, C_in, C_e, C_u, dtype)) return st;
  PYTC_REQUIRE(x_low && dcat && workspace && dw, "upcat_deconv2_wgrad: null pointer");
  UpcatParams p = upcat_params(N, d, h, wd, D, H, W, C_in, C_e, C_u);
  p.x_low = x_low; p.dcat = dcat; p.out = workspace;
  const int ks = mfma_kstep(dtype);
  const int S = upcat_wgrad_splits(p.rows, C_in, C_u, ks);
  p.rows_per_split = ceil_div(ceil_div(p.rows, S), ks) * ks;
  const int S_used = ceil_div(p.rows, p.rows_per_split);     // every split the reduction reads is written (the last may be short)
  hipStream_t st = (hipStream_t)stream;
  dim3 grid(ceil_div(C_in + 1, UP_BP), ceil_div(8L * C_u, UP_BQ), S_used);
  PYTC_DISPATCH_DTYPE(dtype, "upcat_deconv2_wgrad", T, hipLaunchKernelGGL((upcat_gemm_kernel<T, UPCAT_WGRAD>), grid, dim3(256), 0, st, p));
  const long n = (long)C_in * 8 * C_u + C_u;
  hipLaunchKernelGGL(upcat_wgrad_reduce_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, st, (const float*)workspace, dw, db, S_used,
                     C_in, C_u);
  PYTC_LAUNCH_CHECK("upcat_deconv2_wgrad");
  return PYTC_OK;
}

// ---- [up, skip] placement (MONAI UnetrUpBlock: torch.cat((transp_conv(inp), skip), 1)) and the plain k2/s2 deconv (C_e = 0:
// UnetrPrUpBlock chains).  The same GEMMs with the up half at channel offset 0 and the skip after it; the grids are exactly twice the
// low grid (no replicated faces).  The workspace of the weight gradient is sized by pytc_upcat_deconv2_wgrad_ws_elems.
static int upfirst_check(const char* what, int N, int d, int h, int w, int C_in, int C_e, int C_u, int dtype) {
  PYTC_REQUIRE(N >= 1 && d >= 1 && h >= 1 && w >= 1 && C_in >= 1 && C_e >= 0 && C_u >= 1, "%s: bad sizes", what);
  PYTC_REQUIRE((long)N * 8 * d * h * w < (1L << 31), "%s: too many voxels for 32-bit voxel indices", what);
  PYTC_CHECK_DTYPE(dtype, what);
  return PYTC_OK;
}

static UpcatParams upfirst_params(int N, int d, int h, int w, int C_in, int C_e, int C_u) {
  UpcatParams p = upcat_params(N, d, h, w, 2 * d, 2 * h, 2 * w, C_in, C_e, C_u);
  p.up_off = 0;
  return p;
}

extern "C" int pytc_deconv2_upfirst_fwd(const void* x_low, const float* w, const float* bias, const void* x_e, void* out, int N, int d,
                                        int h, int wd, int C_in, int C_e, int C_u, int dtype, void* stream) {
  if (int st = upfirst_check("deconv2_upfirst_fwd", N, d, h, wd, C_in, C_e, C_u, dtype)) return st;
  if (int st = upcat_row_tiles_check("deconv2_upfirst_fwd", N, d, h, wd)) return st;
  PYTC_REQUIRE(x_low && w && out && (C_e == 0 || x_e), "deconv2_upfirst_fwd: null pointer");
  UpcatParams p = upfirst_params(N, d, h, wd, C_in, C_e, C_u);
  p.x_low = x_low; p.w = w; p.bias = bias; p.out = out;
  hipStream_t st = (hipStream_t)stream;
  const long vox = 8L * N * d * h * wd;
  dim3 grid(ceil_div(8L * C_u, UP_BP), ceil_div(p.rows, UP_BQ));
  PYTC_DISPATCH_DTYPE(dtype, "deconv2_upfirst_fwd", T,
                      if (C_e) upcat_copy<T>(x_e, out, vox, C_e, C_e, 0, C_e + C_u, C_u, st);
                      hipLaunchKernelGGL((upcat_gemm_kernel<T, UPCAT_FWD>), grid, dim3(256), 0, st, p));
  PYTC_LAUNCH_CHECK("deconv2_upfirst_fwd");
  return PYTC_OK;
}

extern "C" int pytc_deconv2_upfirst_bwd_data(const void* dout, const float* w, void* dx_e, void* dx_low, int N, int d, int h, int wd,
                                             int C_in, int C_e, int C_u, int dtype, void* stream) {
  if (int st = upfirst_check("deconv2_upfirst_bwd_data", N, d, h, wd, C_in, C_e, C_u, dtype)) return st;
  if (int st = upcat_row_tiles_check("deconv2_upfirst_bwd_data", N, d, h, wd)) return st;
  PYTC_REQUIRE(dout && w, "deconv2_upfirst_bwd_data: null pointer");
  UpcatParams p = upfirst_params(N, d, h, wd, C_in, C_e, C_u);
  p.w = w; p.dcat = dout; p.out = dx_low;
  hipStream_t st = (hipStream_t)stream;
  const long vox = 8L * N * d * h * wd;
  dim3 grid(ceil_div(C_in, UP_BP), ceil_div(p.rows, UP_BQ));
  PYTC_DISPATCH_DTYPE(dtype, "deconv2_upfirst_bwd_data", T,
                      if (dx_e && C_e) upcat_copy<T>(dout, dx_e, vox, C_e, C_e + C_u, C_u, C_e, 0, st);
                      if (dx_low) hipLaunchKernelGGL((upcat_gemm_kernel<T, UPCAT_DGRAD>), grid, dim3(256), 0, st, p));
  PYTC_LAUNCH_CHECK("deconv2_upfirst_bwd_data");
  return PYTC_OK;
}

extern "C" int pytc_deconv2_upfirst_wgrad(const void* x_low, const void* dout, float* workspace, float* dw, float* db, int N, int d, int h,
                                          int wd, int C_in, int C_e, int C_u, int dtype, void* stream) {
  if (int st = upfirst_check("deconv2_upfirst_wgrad", N, d, h, wd, C_in, C_e, C_u, dtype)) return st;
  PYTC_REQUIRE(x_low && dout && workspace && dw, "deconv2_upfirst_wgrad: null pointer");
  UpcatParams p = upfirst_params(N, d, h, wd, C_in, C_e, C_u);
  p.x_low = x_low; p.dcat = dout; p.out = workspace;
  const int ks = mfma_kstep(dtype);
  const int S = upcat_wgrad_splits(p.rows, C_in, C_u, ks);
  p.rows_per_split = ceil_div(ceil_div(p.rows, S), ks) * ks;
  const int S_used = ceil_div(p.rows, p.rows_per_split);
  hipStream_t st = (hipStream_t)stream;
  dim3 grid(ceil_div(C_in + 1, UP_BP), ceil_div(8L * C_u, UP_BQ), S_used);
  PYTC_DISPATCH_DTYPE(dtype, "deconv2_upfirst_wgrad", T, hipLaunchKernelGGL((upcat_gemm_kernel<T, UPCAT_WGRAD>), grid, dim3(256), 0, st, p));
  const long n = (long)C_in * 8 * C_u + C_u;
  hipLaunchKernelGGL(upcat_wgrad_reduce_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, st, (const float*)workspace, dw, db, S_used,
                     C_in, C_u);
  PYTC_LAUNCH_CHECK("deconv2_upfirst_wgrad");
  return PYTC_OK;
}
