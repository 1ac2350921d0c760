// Same-Class Neighbor Penalization (ScnpLoss) on the MI355X: the neighbour-penalised logits z~, the five sums of the per-channel
// class-balanced BCE on them, and the input gradient -- for 5-D (N, C, D, H, W) and 4-D (N, C, H, W) fp32 volumes.
//
// Reference: connectomics/models/losses/losses.py:354-453 (ScnpLoss._scnp_logits, two gated max-pools) scored by
// PerChannelBCEWithLogitsLoss (:269-351).  With ns the window side, r = ns / 2, L = 9999, fg = t > 0.5 per voxel and channel:
//   fg centre:  z~ = min over the in-bounds window voxels u of (fg_u ? x_u : L)
//   bg centre:  z~ = max over the same window of (bg_u ? x_u : -L)         = -min of (bg_u ? -x_u : L)
// so one "first strict minimum in (z, y, x) scan order" serves both classes: the tile is staged twice in LDS, as
// A_u = fg_u ? x_u : L and B_u = bg_u ? -x_u : L (+inf outside the volume: torch pads its pools with -inf), and a centre scans the
// array of its own class.  The selected value is a stored logit (or +-L), so z~ is bit-identical to the reference's for finite logits;
// torch's pooling keeps the first maximum of a window, which the strict comparison in ascending scan order reproduces.
//
// Window code of the supplier: ((dz + r) ns + (dy + r)) ns + (dx + r), written per voxel to `arg`: one byte through ns = 5 (codes
// <= 124), two bytes at ns = 7 (codes <= 342).  2-D inputs (is2d, D = 1) scan dz = 0 only and keep the same code formula.
//
// Tile: 4 x 8 x 64 voxels (z, y, x) per pass of a 256-thread workgroup, 1 x 32 x 64 for 2-D inputs: lane = x (64 consecutive floats
// per wave: conflict-free ds_read_b32, 256-byte global rows), eight consecutive y rows of one z per wave.  The kernels are
// instantiated per (r, window radius along z), so all three window loops unroll.  The staged rows are 72 floats: 4 columns left
// and right of the tile, so that with W % 4 == 0 every global access of the staging is an aligned 16-byte vector (W-contiguous)
// and every LDS write a ds_write_b128; other widths take a scalar staging loop.  LDS per workgroup (3-D): (4 + 2r)(8 + 2r) rows
// x 72 x 8 bytes forward (34.6 / 55.3 / 80.6 KB at ns 3 / 5 / 7) and x 10 bytes backward (43.2 / 69.1 / 100.8 KB).
//
// Sums: per (workgroup, volume) five partials -- sum w [(1 - t) z~ + softplus(-z~)], sum w t softplus(-z~) (fp32) and the counts of
// w > 0, valid t > 0, valid t <= 0 (int32 in the same 4-byte slots) -- reduced by a second launch in a fixed order.  torch's BCE
// with pos_weight pw is (1 - t) x + (1 + (pw - 1) t) softplus(-x), i.e. the first sum + (pw - 1) x the second.  A workgroup walks the
// tiles blockIdx.x, blockIdx.x + gridDim.x, ... of its volume; gridDim.x = pytc_scnp_tiles(D H W) <= the number of tiles.
//
// Gradient, gather form (no atomics): voxel v visits the voxels u of its window in ascending scan order and, wherever arg_u names v
// and u is of v's class, adds g_u w_u [(1 - t_u) - (1 + (pw - 1) t_u) sigmoid(-x_v)] (z~_u = x_v there).  arg, the class bit and the
// two per-u factors are staged with halo in LDS; the fixed order makes the result bit-reproducible.
#include <algorithm>

#include "pytc_common.h"

#pragma clang fp contract(off)

namespace pytc {

constexpr int SC_THREADS = 256;
constexpr int SC_TX = 64, SC_ROWS = 32;                // a tile is SC_ROWS rows of SC_TX voxels: TZ x TY = 4 x 8, or 1 x 32 in 2-D
constexpr int SC_TILE = SC_ROWS * SC_TX;      // 2048 voxels: also the voxels per partial slot of pytc_scnp_tiles
constexpr int SC_PAD = 4;                           // staged columns left and right of the tile (>= r; keeps rows 16-byte aligned)
constexpr int SC_ROW = SC_TX + 2 * SC_PAD;          // 72 floats
constexpr float SC_LARGE = 9999.f;
constexpr int SC_TERMS = 5;

struct ScGeo {
  int D, H, W;
  long V;                                           // D H W
  int C, wC;                                        // channels of x / t and of the weight (C or 1)
  int zr;                                           // window radius along z: r, or 0 for 2-D inputs
  int tz, ty;                                       // tile extent along z and y: 4 x 8, or 1 x 32 for 2-D inputs
  int ny, nx, ntiles;                               // tiles along y and x, tiles per volume
  int vec;                                          // 1: W % 4 == 0 and 16-byte aligned pointers
};

template <int R>
struct ScArg { typedef unsigned char type; };
template <>
struct ScArg<3> { typedef unsigned short type; };

__device__ __forceinline__ void sc_tile_origin(int tile, const ScGeo& g, int& z0, int& y0, int& x0) {
  const int tx = tile % g.nx, rem = tile / g.nx;
  x0 = tx * SC_TX;
  y0 = (rem % g.ny) * g.ty;
  z0 = (rem / g.ny) * g.tz;
}

// the two staged values of one voxel
__device__ __forceinline__ void sc_gate(float x, float t, float& a, float& b) {
  const bool fg = t > 0.5f;
  a = fg ? x : SC_LARGE;
  b = fg ? SC_LARGE : -x;
}

template <int R, int ZR>
__global__ void __launch_bounds__(SC_THREADS) scnp_forward_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                                  const float* __restrict__ w,
                                                                  typename ScArg<R>::type* __restrict__ arg, float* __restrict__ zt,
                                                                  float* __restrict__ partial, ScGeo g, int valid_only) {
  constexpr int NS = 2 * R + 1, TZ = ZR == R ? 4 : 1, TY = SC_ROWS / TZ, NY = TY + 2 * R;
  extern __shared__ __align__(16) float sc_lds[];
  __shared__ float red[SC_THREADS];
  constexpr int rows = (TZ + 2 * ZR) * NY;
  float* A = sc_lds;
  float* B = sc_lds + rows * SC_ROW;
  const int vol = blockIdx.y, n = vol / g.C, c = vol - n * g.C;
  const float* xv = x + (long)vol * g.V;
  const float* tv = t + (long)vol * g.V;
  const float* wv = w ? w + ((long)n * g.wC + (g.wC == 1 ? 0 : c)) * g.V : nullptr;
  const float inf = __builtin_inff();
  const int lx = threadIdx.x & 63, row0 = (threadIdx.x >> 6) * 8, lz = row0 / TY, ly0 = row0 % TY;      // eight rows per wave
  float s0 = 0.f, s1 = 0.f;
  int n0 = 0, n1 = 0, n2 = 0;
  for (int tile = blockIdx.x; tile < g.ntiles; tile += gridDim.x) {
    int z0, y0, x0;
    sc_tile_origin(tile, g, z0, y0, x0);
    if (g.vec) {
      for (int it = threadIdx.x; it < rows * (SC_ROW / 4); it += SC_THREADS) {
        const int row = it / (SC_ROW / 4), q = it - row * (SC_ROW / 4);
        const int rz = row / NY, ry = row - rz * NY;
        const int gz = z0 - ZR + rz, gy = y0 - R + ry, gx = x0 - SC_PAD + 4 * q;
        f32x4_t a = {inf, inf, inf, inf}, b = {inf, inf, inf, inf};
        if (gz >= 0 && gz < g.D && gy >= 0 && gy < g.H && gx >= 0 && gx < g.W) {          // W % 4 == 0: the whole vector is inside
          const long off = ((long)gz * g.H + gy) * g.W + gx;
          const f32x4_t xx = *reinterpret_cast<const f32x4_t*>(xv + off);
          const f32x4_t tt = *reinterpret_cast<const f32x4_t*>(tv + off);
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            float ak, bk;
            sc_gate(xx[k], tt[k], ak, bk);
            a[k] = ak;
            b[k] = bk;
          }
        }
        *reinterpret_cast<f32x4_t*>(A + row * SC_ROW + 4 * q) = a;
        *reinterpret_cast<f32x4_t*>(B + row * SC_ROW + 4 * q) = b;
      }
    } else {
      for (int it = threadIdx.x; it < rows * SC_ROW; it += SC_THREADS) {
        const int row = it / SC_ROW, col = it - row * SC_ROW;
        const int rz = row / NY, ry = row - rz * NY;
        const int gz = z0 - ZR + rz, gy = y0 - R + ry, gx = x0 - SC_PAD + col;
        float a = inf, b = inf;
        if (gz >= 0 && gz < g.D && gy >= 0 && gy < g.H && gx >= 0 && gx < g.W) {
          const long off = ((long)gz * g.H + gy) * g.W + gx;
          sc_gate(xv[off], tv[off], a, b);
        }
        A[it] = a;
        B[it] = b;
      }
    }
    __syncthreads();
    const int gz = z0 + lz, gx = x0 + lx;
    if (gz < g.D && gx < g.W) {
      for (int ly = ly0; ly < ly0 + 8; ++ly) {
        const int gy = y0 + ly;
        if (gy >= g.H) break;
        const long i = ((long)gz * g.H + gy) * g.W + gx;
        const float tc = tv[i];
        const bool fg = tc > 0.5f;
        const float* P = (fg ? A : B) + ((lz + ZR) * NY + (ly + R)) * SC_ROW + lx + SC_PAD;
        float best = inf;
        int code = (R * NS + R) * NS + R;
#pragma unroll
        for (int dz = -ZR; dz <= ZR; ++dz) {
          const float* Pz = P + dz * (NY * SC_ROW);
          float pb = inf;
          int pc = 0;
#pragma unroll
          for (int dy = -R; dy <= R; ++dy) {
#pragma unroll
            for (int dx = -R; dx <= R; ++dx) {
              const float v = Pz[dy * SC_ROW + dx];
              const bool lt = v < pb;
              pb = lt ? v : pb;
              pc = lt ? (dy + R) * NS + (dx + R) : pc;
            }
          }
          if (pb < best) {
            best = pb;
            code = (dz + R) * (NS * NS) + pc;
          }
        }
        const float z = fg ? best : -best;
        arg[(long)vol * g.V + i] = (typename ScArg<R>::type)code;
        if (zt) zt[(long)vol * g.V + i] = z;
        if (partial) {
          const float wc = wv ? wv[i] : 1.f;
          const bool valid = wc > 0.f;
          const float we = (valid_only && !valid) ? 0.f : wc;
          const float sp = log1pf(expf(-fabsf(z))) + fmaxf(-z, 0.f);
          s0 += we * ((1.f - tc) * z + sp);
          s1 += we * (tc * sp);
          n0 += valid ? 1 : 0;
          n1 += (valid && tc > 0.f) ? 1 : 0;
          n2 += (valid && tc <= 0.f) ? 1 : 0;
        }
      }
    }
    __syncthreads();
  }
  if (!partial) return;
  s0 = block_sum<SC_THREADS>(s0, red);
  s1 = block_sum<SC_THREADS>(s1, red);
  int* redi = reinterpret_cast<int*>(red);
  n0 = block_sum<SC_THREADS>(n0, redi);
  n1 = block_sum<SC_THREADS>(n1, redi);
  n2 = block_sum<SC_THREADS>(n2, redi);
  if (threadIdx.x == 0) {
    float* p = partial + ((long)vol * gridDim.x + blockIdx.x) * SC_TERMS;
    p[0] = s0;
    p[1] = s1;
    p[2] = __int_as_float(n0);
    p[3] = __int_as_float(n1);
    p[4] = __int_as_float(n2);
  }
}

// sums[vol 5 + k] = the slot partials of vol in a fixed order: k = 0, 1 fp32 sums, k = 2 .. 4 int32 counts
__global__ void __launch_bounds__(SC_THREADS) scnp_sum_kernel(const float* __restrict__ partial, float* __restrict__ sums, int slots) {
  __shared__ float red[SC_THREADS];
  const int vol = blockIdx.x;
  float a0 = 0.f, a1 = 0.f;
  int c0 = 0, c1 = 0, c2 = 0;
  for (int s = threadIdx.x; s < slots; s += SC_THREADS) {
    const float* p = partial + ((long)vol * slots + s) * SC_TERMS;
    a0 += p[0];
    a1 += p[1];
    c0 += __float_as_int(p[2]);
    c1 += __float_as_int(p[3]);
    c2 += __float_as_int(p[4]);
  }
  a0 = block_sum<SC_THREADS>(a0, red);
  a1 = block_sum<SC_THREADS>(a1, red);
  int* redi = reinterpret_cast<int*>(red);
  c0 = block_sum<SC_THREADS>(c0, redi);
  c1 = block_sum<SC_THREADS>(c1, redi);
  c2 = block_sum<SC_THREADS>(c2, redi);
  if (threadIdx.x == 0) {
    float* o = sums + (long)vol * SC_TERMS;
    o[0] = a0;
    o[1] = a1;
    o[2] = __int_as_float(c0);
    o[3] = __int_as_float(c1);
    o[4] = __int_as_float(c2);
  }
}

// the staged values of one voxel u of the backward: fa = g w (1 - t), fb = g w (1 + (pw - 1) t), key = arg | class << 15
__device__ __forceinline__ void sc_bwd_gate(float t, float w, int a, float g, float pw, int valid_only, float& fa, float& fb,
                                            unsigned short& key) {
  const float we = (valid_only && !(w > 0.f)) ? 0.f : w;
  const float gw = g * we;
  fa = gw * (1.f - t);
  fb = gw * (1.f + (pw - 1.f) * t);
  key = (unsigned short)(a | (t > 0.5f ? 0x8000 : 0));
}

template <int R, int ZR>
__global__ void __launch_bounds__(SC_THREADS) scnp_backward_kernel(const float* __restrict__ x, const float* __restrict__ t,
                                                                   const float* __restrict__ w,
                                                                   const typename ScArg<R>::type* __restrict__ arg,
                                                                   const float* __restrict__ coef, const float* __restrict__ pos_weight,
                                                                   float* __restrict__ dx_out, ScGeo g, int valid_only) {
  typedef typename ScArg<R>::type arg_t;
  typedef arg_t arg4_t __attribute__((ext_vector_type(4)));
  constexpr int NS = 2 * R + 1, TZ = ZR == R ? 4 : 1, TY = SC_ROWS / TZ, NY = TY + 2 * R;
  constexpr unsigned short NOKEY = 0x7fff;                // no window code reaches it
  extern __shared__ __align__(16) float sc_lds[];
  constexpr int rows = (TZ + 2 * ZR) * NY;
  float* FA = sc_lds;
  float* FB = sc_lds + rows * SC_ROW;
  unsigned short* KEY = reinterpret_cast<unsigned short*>(sc_lds + 2 * rows * SC_ROW);
  const int vol = blockIdx.y, n = vol / g.C, c = vol - n * g.C;
  const float* xv = x + (long)vol * g.V;
  const float* tv = t + (long)vol * g.V;
  const float* wv = w ? w + ((long)n * g.wC + (g.wC == 1 ? 0 : c)) * g.V : nullptr;
  const arg_t* av = arg + (long)vol * g.V;
  const float gv = coef[vol], pw = pos_weight[vol];
  const int lx = threadIdx.x & 63, row0 = (threadIdx.x >> 6) * 8, lz = row0 / TY, ly0 = row0 % TY;      // eight rows per wave
  for (int tile = blockIdx.x; tile < g.ntiles; tile += gridDim.x) {
    int z0, y0, x0;
    sc_tile_origin(tile, g, z0, y0, x0);
    if (g.vec) {
      for (int it = threadIdx.x; it < rows * (SC_ROW / 4); it += SC_THREADS) {
        const int row = it / (SC_ROW / 4), q = it - row * (SC_ROW / 4);
        const int rz = row / NY, ry = row - rz * NY;
        const int gz = z0 - ZR + rz, gy = y0 - R + ry, gx = x0 - SC_PAD + 4 * q;
        f32x4_t fa = {0.f, 0.f, 0.f, 0.f}, fb = {0.f, 0.f, 0.f, 0.f};
        unsigned short key[4] = {NOKEY, NOKEY, NOKEY, NOKEY};
        typedef unsigned short key4_t __attribute__((ext_vector_type(4)));
        if (gz >= 0 && gz < g.D && gy >= 0 && gy < g.H && gx >= 0 && gx < g.W) {
          const long off = ((long)gz * g.H + gy) * g.W + gx;
          const f32x4_t tt = *reinterpret_cast<const f32x4_t*>(tv + off);
          f32x4_t ww = {1.f, 1.f, 1.f, 1.f};
          if (wv) ww = *reinterpret_cast<const f32x4_t*>(wv + off);
          const arg4_t aa = *reinterpret_cast<const arg4_t*>(av + off);
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            float fak, fbk;
            sc_bwd_gate(tt[k], ww[k], (int)aa[k], gv, pw, valid_only, fak, fbk, key[k]);
            fa[k] = fak;
            fb[k] = fbk;
          }
        }
        const int o = row * SC_ROW + 4 * q;
        *reinterpret_cast<f32x4_t*>(FA + o) = fa;
        *reinterpret_cast<f32x4_t*>(FB + o) = fb;
        *reinterpret_cast<key4_t*>(KEY + o) = (key4_t){key[0], key[1], key[2], key[3]};       // o % 4 == 0: one 8-byte store
      }
    } else {
      for (int it = threadIdx.x; it < rows * SC_ROW; it += SC_THREADS) {
        const int row = it / SC_ROW, col = it - row * SC_ROW;
        const int rz = row / NY, ry = row - rz * NY;
        const int gz = z0 - ZR + rz, gy = y0 - R + ry, gx = x0 - SC_PAD + col;
        float fa = 0.f, fb = 0.f;
        unsigned short key = NOKEY;
        if (gz >= 0 && gz < g.D && gy >= 0 && gy < g.H && gx >= 0 && gx < g.W) {
          const long off = ((long)gz * g.H + gy) * g.W + gx;
          sc_bwd_gate(tv[off], wv ? wv[off] : 1.f, (int)av[off], gv, pw, valid_only, fa, fb, key);
        }
        FA[it] = fa;
        FB[it] = fb;
        KEY[it] = key;
      }
    }
    __syncthreads();
    const int gz = z0 + lz, gx = x0 + lx;
    if (gz < g.D && gx < g.W) {
      for (int ly = ly0; ly < ly0 + 8; ++ly) {
        const int gy = y0 + ly;
        if (gy >= g.H) break;
        const long i = ((long)gz * g.H + gy) * g.W + gx;
        const int cls = tv[i] > 0.5f ? 0x8000 : 0;
        const float s = 1.f / (1.f + expf(xv[i]));                        // sigmoid(-x_v)
        const int centre = ((lz + ZR) * NY + (ly + R)) * SC_ROW + lx + SC_PAD;
        float acc = 0.f;
#pragma unroll
        for (int dz = -ZR; dz <= ZR; ++dz) {
          const int base = centre + dz * (NY * SC_ROW);
          const int want_z = ((R - dz) * (NS * NS)) | cls;                // u = v + d selected v: its code is that of -d
#pragma unroll
          for (int dy = -R; dy <= R; ++dy) {
#pragma unroll
            for (int dx = -R; dx <= R; ++dx) {
              const int o = base + dy * SC_ROW + dx;
              if ((int)KEY[o] - want_z == (R - dy) * NS + (R - dx)) acc += FA[o] - FB[o] * s;
            }
          }
        }
        dx_out[(long)vol * g.V + i] = acc;
      }
    }
    __syncthreads();
  }
}

static int sc_geo(const char* what, int N, int C, int wC, int D, int H, int W, int ns, int is2d, ScGeo& g) {
  PYTC_REQUIRE(N >= 1 && C >= 1 && (long)N * C <= 65535 && D >= 1 && H >= 1 && W >= 1, "%s: bad shape N %d, C %d, (%d, %d, %d)", what, N,
               C, D, H, W);
  PYTC_REQUIRE(wC == C || wC == 1, "%s: the weight has %d channels, expected %d or 1", what, wC, C);
  PYTC_REQUIRE(!is2d || D == 1, "%s: a 2-D volume has D = 1, got %d", what, D);
  if (ns != 1 && ns != 3 && ns != 5 && ns != 7) {
    set_error("%s: neighborhood_size %d has no kernel (1, 3, 5 and 7 are built)", what, ns);
    return PYTC_ERR_UNSUPPORTED;
  }
  g.D = D;
  g.H = H;
  g.W = W;
  g.V = (long)D * H * W;
  PYTC_REQUIRE(g.V <= 0x7fffffffL - SC_TILE, "%s: %ld voxels per volume", what, g.V);
  g.C = C;
  g.wC = wC;
  g.zr = is2d ? 0 : ns / 2;
  g.tz = g.zr == ns / 2 ? 4 : 1;                      // (ns = 1: r = 0 either way, the 3-D tile)
  g.ty = SC_ROWS / g.tz;
  g.ny = ceil_div(H, g.ty);
  g.nx = ceil_div(W, SC_TX);
  const long nt = (long)ceil_div(D, g.tz) * g.ny * g.nx;
  PYTC_REQUIRE(nt <= 0x7fffffffL, "%s: %ld tiles per volume", what, nt);
  g.ntiles = (int)nt;
  g.vec = 0;
  return PYTC_OK;
}

static bool sc_aligned(const void* p) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int R, int ZR>
static void sc_launch_forward(const float* x, const float* t, const float* w, void* arg, float* zt, float* partial, const ScGeo& g,
                              int valid_only, dim3 grid, hipStream_t st) {
  constexpr int TZ = ZR == R ? 4 : 1;
  const size_t lds = (size_t)(TZ + 2 * ZR) * (SC_ROWS / TZ + 2 * R) * SC_ROW * 8;
  if (lds > 64 * 1024 && !ensure_dynamic_lds(reinterpret_cast<const void*>(&scnp_forward_kernel<R, ZR>), lds, "scnp_forward")) return;
  hipLaunchKernelGGL((scnp_forward_kernel<R, ZR>), grid, dim3(SC_THREADS), lds, st, x, t, w, static_cast<typename ScArg<R>::type*>(arg), zt,
                     partial, g, valid_only);
}

template <int R, int ZR>
static void sc_launch_backward(const float* x, const float* t, const float* w, const void* arg, const float* coef, const float* pw,
                               float* dx, const ScGeo& g, int valid_only, dim3 grid, hipStream_t st) {
  constexpr int TZ = ZR == R ? 4 : 1;
  const size_t lds = (size_t)(TZ + 2 * ZR) * (SC_ROWS / TZ + 2 * R) * SC_ROW * 10;
  if (lds > 64 * 1024 && !ensure_dynamic_lds(reinterpret_cast<const void*>(&scnp_backward_kernel<R, ZR>), lds, "scnp_backward")) return;
  hipLaunchKernelGGL((scnp_backward_kernel<R, ZR>), grid, dim3(SC_THREADS), lds, st, x, t, w,
                     static_cast<const typename ScArg<R>::type*>(arg), coef, pw, dx, g, valid_only);
}

}  // namespace pytc

using namespace pytc;

extern "C" int pytc_scnp_tiles(int64_t voxels) { return ceil_div((long)voxels, SC_TILE); }

extern "C" int pytc_scnp_forward(const float* x, const float* t, const float* w, void* arg, float* zt, float* partial, float* sums,
                                 int N, int C, int wC, int D, int H, int W, int ns, int is2d, int valid_only, void* stream) {
  ScGeo g;
  if (int s = sc_geo("scnp_forward", N, C, w ? wC : C, D, H, W, ns, is2d, g)) return s;
  PYTC_REQUIRE(x && t && arg, "scnp_forward: x, t and arg are required");
  PYTC_REQUIRE((partial != nullptr) == (sums != nullptr), "scnp_forward: sums need the partial workspace, and the workspace the sums");
  g.vec = (W % 4 == 0 && sc_aligned(x) && sc_aligned(t)) ? 1 : 0;
  const int slots = pytc_scnp_tiles(g.V), nvol = N * C;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(slots, nvol);
#define SC_FWD(R)                                                                                     \
  do {                                                                                                \
    if (g.zr == R) sc_launch_forward<R, R>(x, t, w, arg, zt, partial, g, valid_only, grid, st);       \
    else sc_launch_forward<R, 0>(x, t, w, arg, zt, partial, g, valid_only, grid, st);                 \
  } while (0)
  switch (ns / 2) {
    case 0: SC_FWD(0); break;
    case 1: SC_FWD(1); break;
    case 2: SC_FWD(2); break;
    default: SC_FWD(3); break;
  }
  PYTC_LAUNCH_CHECK("scnp_forward");
  if (sums) {
    hipLaunchKernelGGL(scnp_sum_kernel, dim3(nvol), dim3(SC_THREADS), 0, st, partial, sums, slots);
    PYTC_LAUNCH_CHECK("scnp_forward_sum");
  }
  return PYTC_OK;
}

extern "C" int pytc_scnp_backward(const float* x, const float* t, const float* w, const void* arg, const float* coef,
                                  const float* pos_weight, float* dx, int N, int C, int wC, int D, int H, int W, int ns, int is2d,
                                  int valid_only, void* stream) {
  ScGeo g;
  if (int s = sc_geo("scnp_backward", N, C, w ? wC : C, D, H, W, ns, is2d, g)) return s;
  PYTC_REQUIRE(x && t && arg && coef && pos_weight && dx && dx != x, "scnp_backward: null or aliased pointer");
  g.vec = (W % 4 == 0 && sc_aligned(t) && sc_aligned(w) && sc_aligned(arg)) ? 1 : 0;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(pytc_scnp_tiles(g.V), N * C);
#define SC_BWD(R)                                                                                         \
  do {                                                                                                    \
    if (g.zr == R) sc_launch_backward<R, R>(x, t, w, arg, coef, pos_weight, dx, g, valid_only, grid, st); \
    else sc_launch_backward<R, 0>(x, t, w, arg, coef, pos_weight, dx, g, valid_only, grid, st);           \
  } while (0)
  switch (ns / 2) {
    case 0: SC_BWD(0); break;
    case 1: SC_BWD(1); break;
    case 2: SC_BWD(2); break;
    default: SC_BWD(3); break;
  }
  PYTC_LAUNCH_CHECK("scnp_backward");
  return PYTC_OK;
}
