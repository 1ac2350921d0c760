// Training targets from instance labels on the MI355X: the Kisuk-Lee border erosion of an id patch and the stacked target tensor
// (affinities at any offsets, binary, instance boundary, polarity) with its per-channel valid mask, the work the reference does in
// numpy on CPU workers (data/processing/segment.py, affinity.py, target.py, transforms.py MultiTaskLabelTransformd).
//
// Every id is an int32 and stays one: comparisons and parities only, no float touches an id.  Outputs are exact 0 / 1 (/ 2).
//
// seg_erode_kernel.  out[p] = seg[p] where seg[p] < 0 or the box window [p - h, p + h], clipped to the volume, holds exactly one
// distinct positive id (max over the window == min over its positive ids, and a positive id exists); else 0.  A workgroup takes an
// ER_TY x ER_TX tile of one z-plane.  For every plane of the z-window it stages the tile with its (hy, hx) halo in LDS (cells outside
// the volume read as 0: they add no positive id), reduces rows along x into the pair (max, min-positive) in LDS, and every thread folds
// the 2 hy + 1 rows of its four outputs into registers: a separable pass of 1 + (2 hx + 1) + 2 (2 hy + 1) LDS accesses per plane
// instead of (2 hx + 1)(2 hy + 1) gathers.  The stock half-size (0, 1, 1) stages one plane: the label comes from HBM once, halo re-reads
// are cache hits.  A z half-size restages 2 hz + 1 planes per output plane (from L2); the large windows are the rare ones.
//
// label_targets_kernel.  One launch for every channel.  The channel table (kind, source buffer, offsets / ids) and the source pointers
// are kernel arguments by value: no device allocation, no copy, no synchronisation.  A workgroup of 256 threads takes LT_TILE = 4096
// consecutive voxels of one sample; a lane owns four consecutive voxels (consecutive lanes consecutive 16 bytes).  When D H W is a
// multiple of 4 every group of every sample and channel is 16-byte aligned: the centre ids are one vector load per source, every
// channel's values one 16-byte store, its mask one dword (uint8) or 16-byte (fp32) store; W itself may be anything, a group that
// straddles a row carries its (z, y, x) over.  Otherwise the same code runs with scalar accesses and a partial last group.  Neighbour
// ids (the other endpoint of an affinity edge, the six boundary neighbours) are scalar loads that hit L1 / L2: HBM traffic is
// 4 sources + 4 C (+ C or 4 C for the mask) bytes per voxel.
#include <climits>
#include <cstdint>

#include "pytc_common.h"

namespace pytc {

// ---------------------------------------------------------------------------------------------------------------- erosion
constexpr int ER_THREADS = 256;
constexpr int ER_TX = 64, ER_TY = 16;
constexpr int ER_MAX_H = 10;
constexpr int ER_PER_THREAD = ER_TX * ER_TY / ER_THREADS;
static_assert(ER_TX == WAVE && ER_TY % (ER_THREADS / WAVE) == 0, "a wave is one tile row; the waves share the rows evenly");

struct ErGeo {
  int N, D, H, W, hz, hy, hx, tiles_x, tiles_y;
};

__global__ void __launch_bounds__(ER_THREADS) seg_erode_kernel(const int32_t* __restrict__ seg, int32_t* __restrict__ out, ErGeo g) {
  extern __shared__ int er_lds[];                          // sized by the launch for this halo: er_lds_bytes
  long b = blockIdx.x;
  const int tx = (int)(b % g.tiles_x);
  b /= g.tiles_x;
  const int ty = (int)(b % g.tiles_y);
  b /= g.tiles_y;
  const int z = (int)(b % g.D);
  const int n = (int)(b / g.D);
  const int x0 = tx * ER_TX, y0 = ty * ER_TY;
  const int rows = ER_TY + 2 * g.hy, pw = ER_TX + 2 * g.hx;
  int* raw = er_lds;                                       // rows x pw staged ids
  int* xmax = raw + rows * pw;                             // rows x ER_TX: the maximum of every row window
  int* xmin = xmax + rows * ER_TX;                         // rows x ER_TX: its minimum over positive ids
  const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
  const int32_t* vol = seg + (long)n * g.D * g.H * g.W;
  int M[ER_PER_THREAD], m[ER_PER_THREAD];
#pragma unroll
  for (int j = 0; j < ER_PER_THREAD; ++j) {
    M[j] = INT_MIN;
    m[j] = INT_MAX;
  }
  const int z_lo = z - g.hz < 0 ? 0 : z - g.hz, z_hi = z + g.hz > g.D - 1 ? g.D - 1 : z + g.hz;
  for (int zz = z_lo; zz <= z_hi; ++zz) {
    const int32_t* plane = vol + (long)zz * g.H * g.W;
    for (int i = threadIdx.x; i < rows * pw; i += ER_THREADS) {
      const int r = i / pw, c = i - r * pw;
      const int gy = y0 - g.hy + r, gx = x0 - g.hx + c;
      raw[i] = (gy >= 0 && gy < g.H && gx >= 0 && gx < g.W) ? plane[(long)gy * g.W + gx] : 0;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < rows * ER_TX; i += ER_THREADS) {
      const int r = i / ER_TX, c = i % ER_TX;
      int a = INT_MIN, p = INT_MAX;
      for (int k = 0; k <= 2 * g.hx; ++k) {
        const int v = raw[r * pw + c + k];
        a = v > a ? v : a;
        p = (v > 0 && v < p) ? v : p;
      }
      xmax[i] = a;
      xmin[i] = p;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < ER_PER_THREAD; ++j) {
      const int ry = wave * ER_PER_THREAD + j;             // output row of the tile; its window is staged rows ry .. ry + 2 hy
      for (int k = 0; k <= 2 * g.hy; ++k) {
        const int a = xmax[(ry + k) * ER_TX + lane], p = xmin[(ry + k) * ER_TX + lane];
        M[j] = a > M[j] ? a : M[j];
        m[j] = p < m[j] ? p : m[j];
      }
    }
    __syncthreads();                                       // the next plane overwrites raw / xmax / xmin
  }
#pragma unroll
  for (int j = 0; j < ER_PER_THREAD; ++j) {
    const int y = y0 + wave * ER_PER_THREAD + j, x = x0 + lane;
    if (y < g.H && x < g.W) {
      const long at = ((long)n * g.D + z) * g.H * g.W + (long)y * g.W + x;
      const int v = seg[at];
      out[at] = (v < 0 || (M[j] > 0 && M[j] == m[j])) ? v : 0;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- targets
constexpr int LT_THREADS = 256;
constexpr int LT_VPL = 4;                                  // voxels per lane and pass
constexpr int LT_TILE = 4096;                              // voxels per workgroup (pytc_label_targets_tile)
constexpr int LT_PASSES = LT_TILE / (LT_THREADS * LT_VPL);
static_assert(LT_TILE % (LT_THREADS * LT_VPL) == 0, "a tile is a whole number of passes");

struct LtChan {
  int8_t kind, source, flags, n_ids;
  int32_t v[PYTC_LABEL_MAX_IDS];                           // affinity: dz, dy, dx; binary: the segment ids
};

struct LtTable {
  const int32_t* src[PYTC_LABEL_MAX_SOURCES];
  LtChan ch[PYTC_LABEL_MAX_CHANNELS];
  int n_src, n_ch, D, H, W, mask_f32;
  long V;
};
static_assert(sizeof(LtTable) <= 2048, "the table travels as a kernel argument");

typedef int i32x4_t __attribute__((ext_vector_type(4)));
typedef unsigned char u8x4_t __attribute__((ext_vector_type(4)));

// (z, y, x) lies inside the volume
__device__ __forceinline__ bool lt_inside(const LtTable& t, int z, int y, int x) {
  return z >= 0 && z < t.D && y >= 0 && y < t.H && x >= 0 && x < t.W;
}

__device__ __forceinline__ bool lt_edge(int a, int b, int mode) {
  if (a == b) return false;
  if (mode == PYTC_LABEL_EDGE_ALL) return true;
  if (mode == PYTC_LABEL_EDGE_SEG_ALL) return a > 0 || b > 0;
  return a > 0 && b > 0;
}

// The other endpoint q of channel c's edge for the lane's four voxels: o[j] = the id at q, in[j] = q lies in the volume (an affinity
// channel; anything else, and c beyond the table, leaves 0 / false).  The kernel calls it one channel ahead, so that these loads are in
// flight while the channel before is compared and stored: a lane's channels are otherwise one load latency after the other.
__device__ __forceinline__ void lt_fetch(const LtTable& t, int c, int n, long p0, int live, long HW, const int (&z)[LT_VPL],
                                         const int (&y)[LT_VPL], const int (&x)[LT_VPL], int (&o)[LT_VPL], bool (&in)[LT_VPL]) {
#pragma unroll
  for (int j = 0; j < LT_VPL; ++j) {
    o[j] = 0;
    in[j] = false;
  }
  if (c >= t.n_ch || t.ch[c].kind != PYTC_LABEL_AFFINITY) return;
  const LtChan& ch = t.ch[c];
  const int32_t* vol = t.src[ch.source] + (long)n * t.V;
  const int sign = (ch.flags & PYTC_LABEL_FLAG_BANIS) ? 1 : -1;           // q = p + o (banis), p - o (deepem)
  const int dz = sign * ch.v[0], dy = sign * ch.v[1], dx = sign * ch.v[2];
  const long shift = (long)dz * HW + (long)dy * t.W + dx;
#pragma unroll
  for (int j = 0; j < LT_VPL; ++j) {
    in[j] = j < live && lt_inside(t, z[j] + dz, y[j] + dy, x[j] + dx);
    if (in[j]) o[j] = vol[p0 + j + shift];
  }
}

template <bool VEC>
__global__ void __launch_bounds__(LT_THREADS) label_targets_kernel(float* __restrict__ values, void* __restrict__ mask, LtTable t) {
  const int n = blockIdx.y;
  const long tile0 = (long)blockIdx.x * LT_TILE;
  const long HW = (long)t.H * t.W;
  for (int pass = 0; pass < LT_PASSES; ++pass) {
    const long p0 = tile0 + ((long)pass * LT_THREADS + threadIdx.x) * LT_VPL;
    if (p0 >= t.V) continue;
    const int live = t.V - p0 < LT_VPL ? (int)(t.V - p0) : LT_VPL;        // (VEC: always 4)
    int z[LT_VPL], y[LT_VPL], x[LT_VPL];
    z[0] = (int)(p0 / HW);
    const int rem = (int)(p0 - (long)z[0] * HW);
    y[0] = rem / t.W;
    x[0] = rem - y[0] * t.W;
#pragma unroll
    for (int j = 1; j < LT_VPL; ++j) {                     // carry (z, y, x) over a row / plane end; beyond the sample: unused
      x[j] = x[j - 1] + 1;
      y[j] = y[j - 1];
      z[j] = z[j - 1];
      if (x[j] == t.W) {
        x[j] = 0;
        if (++y[j] == t.H) {
          y[j] = 0;
          ++z[j];
        }
      }
    }
    // the centre ids of every source buffer
    int ctr[PYTC_LABEL_MAX_SOURCES][LT_VPL];
#pragma unroll
    for (int s = 0; s < PYTC_LABEL_MAX_SOURCES; ++s) {
      if (s < t.n_src) {
        const int32_t* q = t.src[s] + (long)n * t.V + p0;
        if (VEC) {
          const i32x4_t c4 = *reinterpret_cast<const i32x4_t*>(q);
#pragma unroll
          for (int j = 0; j < LT_VPL; ++j) ctr[s][j] = c4[j];
        } else {
#pragma unroll
          for (int j = 0; j < LT_VPL; ++j) ctr[s][j] = j < live ? q[j] : 0;
        }
      } else {
#pragma unroll
        for (int j = 0; j < LT_VPL; ++j) ctr[s][j] = 0;
      }
    }
    int o_next[LT_VPL];
    bool in_next[LT_VPL];
    lt_fetch(t, 0, n, p0, live, HW, z, y, x, o_next, in_next);
    for (int c = 0; c < t.n_ch; ++c) {                     // everything about a channel is wave-uniform
      const LtChan& ch = t.ch[c];
      const int32_t* vol = t.src[ch.source] + (long)n * t.V;
      int o_cur[LT_VPL];
      bool in_cur[LT_VPL];
#pragma unroll
      for (int j = 0; j < LT_VPL; ++j) {
        o_cur[j] = o_next[j];
        in_cur[j] = in_next[j];
      }
      lt_fetch(t, c + 1, n, p0, live, HW, z, y, x, o_next, in_next);
      int a[LT_VPL];
#pragma unroll
      for (int j = 0; j < LT_VPL; ++j)
        a[j] = ch.source == 0 ? ctr[0][j] : (ch.source == 1 ? ctr[1][j] : (ch.source == 2 ? ctr[2][j] : ctr[3][j]));
      float val[LT_VPL];
      bool ok[LT_VPL];
      if (ch.kind == PYTC_LABEL_AFFINITY) {
        const bool semantic = (ch.flags & PYTC_LABEL_FLAG_SEMANTIC) != 0;
#pragma unroll
        for (int j = 0; j < LT_VPL; ++j) {
          const bool in = in_cur[j];                       // fetched one channel ago (lt_fetch)
          int o = o_cur[j];
          int s = a[j];
          if (semantic) {
            o = o > 0 ? 1 : o;
            s = s > 0 ? 1 : s;
          }
          val[j] = (in && s == o && s > 0) ? 1.f : 0.f;
          ok[j] = in && s != -1 && o != -1;
        }
      } else if (ch.kind == PYTC_LABEL_BINARY) {
#pragma unroll
        for (int j = 0; j < LT_VPL; ++j) {
          bool hit = a[j] > 0;
          if (ch.n_ids > 0) {
            hit = false;
            for (int k = 0; k < ch.n_ids; ++k) hit = hit || a[j] == ch.v[k];
          }
          val[j] = hit ? 1.f : 0.f;
          ok[j] = a[j] != -1;
        }
      } else if (ch.kind == PYTC_LABEL_BOUNDARY) {
        const int mode = ch.flags & 3;
        const bool planar = (ch.flags & PYTC_LABEL_FLAG_2D) != 0;
#pragma unroll
        for (int j = 0; j < LT_VPL; ++j) {
          bool hit = false;
          if (j < live) {
            const long p = p0 + j;
            if (x[j] > 0) hit = hit || lt_edge(a[j], vol[p - 1], mode);
            if (x[j] < t.W - 1) hit = hit || lt_edge(a[j], vol[p + 1], mode);
            if (y[j] > 0) hit = hit || lt_edge(a[j], vol[p - t.W], mode);
            if (y[j] < t.H - 1) hit = hit || lt_edge(a[j], vol[p + t.W], mode);
            if (!planar) {
              if (z[j] > 0) hit = hit || lt_edge(a[j], vol[p - HW], mode);
              if (z[j] < t.D - 1) hit = hit || lt_edge(a[j], vol[p + HW], mode);
            }
          }
          val[j] = hit ? 1.f : 0.f;
          ok[j] = a[j] != -1;
        }
      } else {                                             // PYTC_LABEL_POLARITY
        const int what = ch.flags & 3;
#pragma unroll
        for (int j = 0; j < LT_VPL; ++j) {
          const bool fg = a[j] > 0, odd = (a[j] & 1) != 0;
          const bool pos = fg && odd, neg = fg && !odd;
          val[j] = what == PYTC_LABEL_POLARITY_POS ? (pos ? 1.f : 0.f)
                   : what == PYTC_LABEL_POLARITY_NEG ? (neg ? 1.f : 0.f)
                   : what == PYTC_LABEL_POLARITY_FG  ? (fg ? 1.f : 0.f)
                                                     : (pos ? 1.f : (neg ? 2.f : 0.f));
          ok[j] = a[j] != -1;
        }
      }
      const long at = ((long)n * t.n_ch + c) * t.V + p0;
      if (VEC) {
        *reinterpret_cast<f32x4_t*>(values + at) = f32x4_t{val[0], val[1], val[2], val[3]};
        if (mask) {
          if (t.mask_f32)
            *reinterpret_cast<f32x4_t*>(static_cast<float*>(mask) + at) =
                f32x4_t{ok[0] ? 1.f : 0.f, ok[1] ? 1.f : 0.f, ok[2] ? 1.f : 0.f, ok[3] ? 1.f : 0.f};
          else
            *reinterpret_cast<u8x4_t*>(static_cast<unsigned char*>(mask) + at) =
                u8x4_t{(unsigned char)ok[0], (unsigned char)ok[1], (unsigned char)ok[2], (unsigned char)ok[3]};
        }
      } else {
#pragma unroll
        for (int j = 0; j < LT_VPL; ++j) {
          if (j < live) {
            values[at + j] = val[j];
            if (mask) {
              if (t.mask_f32)
                static_cast<float*>(mask)[at + j] = ok[j] ? 1.f : 0.f;
              else
                static_cast<unsigned char*>(mask)[at + j] = (unsigned char)ok[j];
            }
          }
        }
      }
    }
  }
}

// LDS of one erosion workgroup: the staged tile with its halo and the two row-reduced planes.  4.6 KB + 9.2 KB at the stock halo
// (0, 1, 1), 30 KB at (10, 10); sized per launch so that the small halos keep eight workgroups on a CU
static size_t er_lds_bytes(int hy, int hx) { return sizeof(int) * (size_t)(ER_TY + 2 * hy) * ((ER_TX + 2 * hx) + 2 * ER_TX); }

static bool ranges_overlap(const void* a, long a_bytes, const void* b, long b_bytes) {
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return pa < pb + b_bytes && pb < pa + a_bytes;
}

}  // namespace pytc

using namespace pytc;

extern "C" int pytc_seg_erode_instance(const int32_t* seg, int32_t* out, int N, int D, int H, int W, int hz, int hy, int hx, void* stream) {
  const char* what = "seg_erode_instance";
  PYTC_REQUIRE(seg && out, "%s: seg and out are required", what);
  PYTC_REQUIRE(N >= 1 && D >= 1 && H >= 1 && W >= 1, "%s: bad shape N %d, D %d, H %d, W %d", what, N, D, H, W);
  PYTC_REQUIRE(hz >= 0 && hy >= 0 && hx >= 0, "%s: negative half-size (%d, %d, %d)", what, hz, hy, hx);
  const long total = (long)N * D * H * W;
  PYTC_REQUIRE((long)D * H * W <= 0x7fffffffL, "%s: %ld voxels per sample", what, (long)D * H * W);
  PYTC_REQUIRE(!ranges_overlap(seg, total * 4, out, total * 4), "%s: out must not alias seg (a voxel's window reads its neighbours' inputs)", what);
  if (hz > ER_MAX_H || hy > ER_MAX_H || hx > ER_MAX_H) {
    set_error("%s: half-size (%d, %d, %d); the erosion kernel covers 0 .. %d per axis", what, hz, hy, hx, ER_MAX_H);
    return PYTC_ERR_UNSUPPORTED;
  }
  ErGeo g{N, D, H, W, hz, hy, hx, ceil_div(W, ER_TX), ceil_div(H, ER_TY)};
  const long blocks = (long)N * D * g.tiles_x * g.tiles_y;
  PYTC_REQUIRE(blocks <= 0x7fffffffL, "%s: %ld tiles", what, blocks);
  hipLaunchKernelGGL(seg_erode_kernel, dim3((unsigned)blocks), dim3(ER_THREADS), er_lds_bytes(hy, hx), (hipStream_t)stream, seg, out, g);
  PYTC_LAUNCH_CHECK("seg_erode_instance");
  return PYTC_OK;
}

extern "C" int pytc_label_targets_tile(void) { return LT_TILE; }

extern "C" int pytc_label_targets(const int32_t* const* sources, int n_sources, const pytc_label_channel* channels, int n_channels,
                                  float* values, void* mask, int mask_dtype, int N, int D, int H, int W, void* stream) {
  const char* what = "label_targets";
  PYTC_REQUIRE(sources && channels && values, "%s: sources, channels and values are required", what);
  PYTC_REQUIRE(n_sources >= 1 && n_channels >= 1, "%s: %d sources, %d channels", what, n_sources, n_channels);
  if (n_sources > PYTC_LABEL_MAX_SOURCES || n_channels > PYTC_LABEL_MAX_CHANNELS) {
    set_error("%s: %d sources, %d channels; one launch covers at most %d sources and %d channels", what, n_sources, n_channels,
              PYTC_LABEL_MAX_SOURCES, PYTC_LABEL_MAX_CHANNELS);
    return PYTC_ERR_UNSUPPORTED;
  }
  PYTC_REQUIRE(N >= 1 && N <= 65535 && D >= 1 && H >= 1 && W >= 1, "%s: bad shape N %d, D %d, H %d, W %d", what, N, D, H, W);
  PYTC_REQUIRE((long)D * H * W <= 0x3fffffffL, "%s: %ld voxels per sample", what, (long)D * H * W);
  PYTC_REQUIRE(mask_dtype == PYTC_LABEL_MASK_U8 || mask_dtype == PYTC_LABEL_MASK_F32, "%s: unknown mask_dtype %d", what, mask_dtype);
  LtTable t;
  memset(&t, 0, sizeof(t));
  t.n_src = n_sources;
  t.n_ch = n_channels;
  t.D = D;
  t.H = H;
  t.W = W;
  t.V = (long)D * H * W;
  t.mask_f32 = mask_dtype == PYTC_LABEL_MASK_F32;
  bool vec = t.V % LT_VPL == 0 && (reinterpret_cast<uintptr_t>(values) & 15) == 0 &&
             (!mask || (reinterpret_cast<uintptr_t>(mask) & (t.mask_f32 ? 15 : 3)) == 0);
  for (int s = 0; s < n_sources; ++s) {
    PYTC_REQUIRE(sources[s], "%s: source %d is null", what, s);
    t.src[s] = sources[s];
    vec = vec && (reinterpret_cast<uintptr_t>(sources[s]) & 15) == 0;
  }
  for (int c = 0; c < n_channels; ++c) {
    const pytc_label_channel& in = channels[c];
    PYTC_REQUIRE(in.source >= 0 && in.source < n_sources, "%s: channel %d reads source %d of %d", what, c, in.source, n_sources);
    LtChan& ch = t.ch[c];
    ch.kind = (int8_t)in.kind;
    ch.source = (int8_t)in.source;
    ch.flags = (int8_t)in.flags;
    ch.n_ids = 0;
    switch (in.kind) {
      case PYTC_LABEL_AFFINITY:
        PYTC_REQUIRE((in.flags & ~(PYTC_LABEL_FLAG_BANIS | PYTC_LABEL_FLAG_SEMANTIC)) == 0, "%s: channel %d: affinity flags %d", what, c,
                     in.flags);
        for (int k = 0; k < 3; ++k) {
          // an offset as long as its axis already leaves the channel empty: larger ones are clamped to that, so a coordinate
          // plus an offset stays inside an int
          const int lim = k == 0 ? D : (k == 1 ? H : W);
          ch.v[k] = in.v[k] > lim ? lim : (in.v[k] < -lim ? -lim : in.v[k]);
        }
        break;
      case PYTC_LABEL_BINARY:
        PYTC_REQUIRE(in.flags == 0 && in.n_ids >= 0 && in.n_ids <= PYTC_LABEL_MAX_IDS, "%s: channel %d: binary with %d ids, flags %d",
                     what, c, in.n_ids, in.flags);
        ch.n_ids = (int8_t)in.n_ids;
        for (int k = 0; k < in.n_ids; ++k) ch.v[k] = in.v[k];
        break;
      case PYTC_LABEL_BOUNDARY:
        PYTC_REQUIRE((in.flags & ~(3 | PYTC_LABEL_FLAG_2D)) == 0 && (in.flags & 3) <= PYTC_LABEL_EDGE_SEG_NO_BG,
                     "%s: channel %d: boundary flags %d", what, c, in.flags);
        break;
      case PYTC_LABEL_POLARITY:
        PYTC_REQUIRE(in.flags >= 0 && in.flags <= PYTC_LABEL_POLARITY_EXCLUSIVE, "%s: channel %d: polarity form %d", what, c, in.flags);
        break;
      default:
        PYTC_REQUIRE(false, "%s: channel %d: unknown kind %d", what, c, in.kind);
    }
  }
  const long bytes_s = (long)N * t.V * 4, bytes_v = bytes_s * n_channels, bytes_m = mask ? (t.mask_f32 ? bytes_v : bytes_v / 4) : 0;
  for (int s = 0; s < n_sources; ++s)
    PYTC_REQUIRE(!ranges_overlap(sources[s], bytes_s, values, bytes_v) && (!mask || !ranges_overlap(sources[s], bytes_s, mask, bytes_m)),
                 "%s: values and mask must not alias source %d", what, s);
  PYTC_REQUIRE(!mask || !ranges_overlap(values, bytes_v, mask, bytes_m), "%s: mask must not alias values", what);
  const dim3 grid(ceil_div(t.V, LT_TILE), N);
  hipStream_t st = (hipStream_t)stream;
  if (vec)
    hipLaunchKernelGGL((label_targets_kernel<true>), grid, dim3(LT_THREADS), 0, st, values, mask, t);
  else
    hipLaunchKernelGGL((label_targets_kernel<false>), grid, dim3(LT_THREADS), 0, st, values, mask, t);
  PYTC_LAUNCH_CHECK("label_targets");
  return PYTC_OK;
}
