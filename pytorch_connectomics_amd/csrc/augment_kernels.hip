// Training augmentations on the MI355X: the flips, quarter turns and axis permutations of a batch as one signed axis permutation per
// sample, and the EM section defects of the image (filled slices and rectangles, shifted slabs, lost sections, one multiply-add) as a
// chain of op rows per sample, the work the reference does in numpy on CPU workers (data/augmentation/transforms.py, augment_ops.py).
// Everything is an index map or one multiply-add: outputs equal numpy's bit for bit.
//
// aug_permute_lines_kernel.  Samples whose permutation keeps x on x.  A workgroup of 256 threads takes AUG_TILE = 4096 consecutive
// output voxels of one (sample, channel); a lane owns four consecutive voxels.  With W a multiple of 4 and 16-byte aligned buffers the
// four lie in one line: one 16-byte load (taken from the mirrored position and reversed in registers when x is flipped) and one
// 16-byte store; otherwise scalar accesses.  The identity is the same code with positive unit steps: a copy.
//
// aug_permute_tiles_kernel.  Samples whose permutation moves x: the input x axis becomes output axis a (z or y), so output lines run
// along what was a strided axis.  A workgroup stages a 64 x 64 tile of the (output x, output a) plane in LDS, rows padded to 65 dwords:
// it reads the input along its x lines (a wave one 256-byte piece, backwards when that axis is flipped), and every wave then reads a
// tile COLUMN (dword address 65 lane + row: the 32 lanes of a half fall on 32 different banks) and writes it as one 256-byte piece of
// an output line.  A gather without the tile would read 4 bytes of every 128-byte line it touches.
//
// aug_defects_kernel.  One launch per batch.  A sample's rows are staged in LDS once per workgroup; every output voxel walks them
// backwards with a source coordinate (a shift moves it, a section copy changes z, a fill or a zero-filled shift ends the walk with a
// constant), loads the input there (shifts only offset the x lines a wave reads) and applies the multiply-adds behind the row that
// ended the walk in forward order, the product rounded before the sum: no contraction into a fused multiply-add.  An interpolated
// lost section evaluates the two neighbours' walks over the rows before its group.  A lane owns four consecutive voxels and stores
// them as one 16-byte vector when the sample's voxel count is a multiple of 4.
//
// The kernels decode tables from device memory; the launches check the caller's host copy of the same tables.  A kernel still refuses
// whatever it cannot index safely (a permutation that is none, coordinates outside the volume, offsets outside the table): it writes
// nothing, or zero, rather than read out of bounds.
#include <cstdint>

#include "pytc_common.h"

// numpy rounds the product and then the sum.  hipcc contracts a * b + c into one fused multiply-add by default, and this HIP's
// __fmul_rn / __fadd_rn are inline operators compiled under that default, which a pragma here cannot reach.  Contraction is off for
// this file and the arithmetic is written with plain operators: the listing of the defect kernels holds v_mul_f32 / v_add_f32 pairs
// and no v_fma / v_fmac on a loaded value (those it has belong to the 64-bit divisions).
#pragma clang fp contract(off)

namespace pytc {

constexpr int AUG_THREADS = 256;
constexpr int AUG_VPL = 4;                                 // voxels per lane and pass
constexpr int AUG_TILE = 4096;                             // voxels per workgroup (pytc_augment_tile)
constexpr int AUG_PASSES = AUG_TILE / (AUG_THREADS * AUG_VPL);
constexpr int AUG_TS = 64;                                 // side of the transposing tile
static_assert(AUG_TILE % (AUG_THREADS * AUG_VPL) == 0, "a tile is a whole number of passes");
static_assert(AUG_TS == WAVE && AUG_TS * AUG_TS == AUG_TILE, "a wave is one tile row; the tile is one workgroup's voxels");

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

struct AugGeo {
  int C, D, H, W;
  long V;
};

// A sample's signed permutation as index arithmetic: the input offset of output voxel (o0, o1, o2) is base + sum o_a step[a].
struct AugMap {
  long base, step[3];
  int src[3];
};

// false where v is no signed permutation or would change the shape (the launch has refused the same on the host copy)
__host__ __device__ inline bool aug_decode(const int32_t* v, int D, int H, int W, AugMap& m) {
  const int dims[3] = {D, H, W};
  const long stride[3] = {(long)H * W, (long)W, 1L};
  int seen = 0;
  m.base = 0;
  for (int a = 0; a < 3; ++a) {
    const bool flip = v[a] < 0;
    const int s = flip ? -1 - v[a] : v[a];
    if (s < 0 || s > 2 || dims[s] != dims[a]) return false;
    seen |= 1 << s;
    m.src[a] = s;
    m.step[a] = flip ? -stride[s] : stride[s];
    if (flip) m.base += (long)(dims[a] - 1) * stride[s];
  }
  return seen == 7;
}

template <bool VEC>
__global__ void __launch_bounds__(AUG_THREADS) aug_permute_lines_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                                        const int32_t* __restrict__ perm, AugGeo g) {
  const int nc = blockIdx.y;
  AugMap m;
  if (!aug_decode(perm + 3 * (nc / g.C), g.D, g.H, g.W, m) || m.src[2] != 2) return;      // x moves: the tile kernel's sample
  const uint32_t* src = in + (long)nc * g.V;
  uint32_t* dst = out + (long)nc * g.V;
  const long HW = (long)g.H * g.W;
  const bool flip_x = m.step[2] < 0;
  const long tile0 = (long)blockIdx.x * AUG_TILE;
  for (int pass = 0; pass < AUG_PASSES; ++pass) {
    const long p0 = tile0 + ((long)pass * AUG_THREADS + threadIdx.x) * AUG_VPL;
    if (p0 >= g.V) continue;
    if (VEC) {                                             // W % 4 == 0: the four voxels share (z, y)
      const int z = (int)(p0 / HW);
      const int rem = (int)(p0 - (long)z * HW);
      const int y = rem / g.W, x = rem - y * g.W;
      const long at = m.base + z * m.step[0] + y * m.step[1] + (flip_x ? -(long)x : (long)x);
      u32x4_t v;
      if (flip_x) {
        const u32x4_t r = *reinterpret_cast<const u32x4_t*>(src + at - 3);
        v = u32x4_t{r[3], r[2], r[1], r[0]};
      } else {
        v = *reinterpret_cast<const u32x4_t*>(src + at);
      }
      *reinterpret_cast<u32x4_t*>(dst + p0) = v;
    } else {
#pragma unroll
      for (int j = 0; j < AUG_VPL; ++j) {
        const long p = p0 + j;
        if (p < g.V) {
          const int z = (int)(p / HW);
          const int rem = (int)(p - (long)z * HW);
          const int y = rem / g.W, x = rem - y * g.W;
          dst[p] = src[m.base + z * m.step[0] + y * m.step[1] + x * m.step[2]];
        }
      }
    }
  }
}

__global__ void __launch_bounds__(AUG_THREADS) aug_permute_tiles_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                                        const int32_t* __restrict__ perm, AugGeo g, int tiles_w) {
  __shared__ uint32_t tile[AUG_TS][AUG_TS + 1];
  const int nc = blockIdx.z;
  AugMap m;
  if (!aug_decode(perm + 3 * (nc / g.C), g.D, g.H, g.W, m) || m.src[2] == 2) return;      // x stays: the line kernel's sample
  const int a = m.src[0] == 2 ? 0 : 1;                     // the output axis the input x axis lands on: its length is W
  const int b = 1 - a;                                     // the remaining output axis: one plane per blockIdx.y
  const int ob = blockIdx.y;
  if (ob >= (b == 0 ? g.D : g.H)) return;
  const int ox0 = (int)(blockIdx.x % tiles_w) * AUG_TS, oa0 = (int)(blockIdx.x / tiles_w) * AUG_TS;
  const long out_stride[2] = {(long)g.H * g.W, (long)g.W};
  const uint32_t* src = in + (long)nc * g.V + m.base + ob * m.step[b];
  uint32_t* dst = out + (long)nc * g.V + ob * out_stride[b];
  const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
  for (int i = wave; i < AUG_TS; i += AUG_THREADS / WAVE) {            // row i: output x = ox0 + i; lanes along output a = input x
    const int ox = ox0 + i, oa = oa0 + lane;
    if (ox < g.W && oa < g.W) tile[i][lane] = src[oa * m.step[a] + ox * m.step[2]];
  }
  __syncthreads();
  for (int r = wave; r < AUG_TS; r += AUG_THREADS / WAVE) {            // row r: output a = oa0 + r; lanes along output x
    const int oa = oa0 + r, ox = ox0 + lane;
    if (oa < g.W && ox < g.W) dst[oa * out_stride[a] + ox] = tile[lane][r];
  }
}

// ---------------------------------------------------------------------------------------------------------------- defects
// The value of voxel (z, y, x) after rows [0, k_end) of `ops`; rows of group `skip` are passed over (they read their group's input).
template <bool ALLOW_MEAN>
__device__ __forceinline__ float aug_eval(const float* __restrict__ vol, const int32_t* ops, int k_end, int skip, int z, int y, int x,
                                          const AugGeo& g) {
  float v = 0.f;
  bool constant = false;
  int k = k_end - 1;
  for (; k >= 0; --k) {
    const int32_t* r = ops + k * PYTC_AUG_ROW;
    const int kind = r[0], grp = r[1];
    if (kind == PYTC_AUG_MULADD || (grp != 0 && grp == skip)) continue;
    if (kind == PYTC_AUG_FILL) {
      if (z >= r[2] && z < r[3] && y >= r[4] && y < r[5] && x >= r[6] && x < r[7]) {
        v = __int_as_float(r[8]);
        constant = true;
        break;
      }
    } else if (kind == PYTC_AUG_MOVE) {
      const int axis = r[2];
      const int c = axis == 0 ? z : (axis == 1 ? y : x);
      if (c >= r[3] && c < r[4]) {
        const int nu = axis == 0 ? g.H : g.D, nv = axis == 2 ? g.H : g.W;
        int su = (axis == 0 ? y : z) - r[5], sv = (axis == 2 ? y : x) - r[6];
        if (r[7]) {
          su %= nu;
          sv %= nv;
          su += su < 0 ? nu : 0;
          sv += sv < 0 ? nv : 0;
        } else if (su < 0 || su >= nu || sv < 0 || sv >= nv) {
          constant = true;                                 // v = 0: what a zero-filled shift brings in from outside
          break;
        }
        if (axis == 0) {
          y = su;
          x = sv;
        } else if (axis == 1) {
          z = su;
          x = sv;
        } else {
          z = su;
          y = sv;
        }
      }
    } else if (kind == PYTC_AUG_COPY_SECTION && z == r[2]) {
      if (r[3] != 0) {
        z += r[3] < 0 ? -1 : 1;
        skip = grp;
      } else if (ALLOW_MEAN) {
        const float lo = aug_eval<false>(vol, ops, k, grp, z - 1, y, x, g), hi = aug_eval<false>(vol, ops, k, grp, z + 1, y, x, g);
        v = 0.5f * (lo + hi);
        constant = true;
        break;
      }
    }
  }
  if (!constant) {
    const bool inside = z >= 0 && z < g.D && y >= 0 && y < g.H && x >= 0 && x < g.W;       // a valid table never leaves the volume
    v = inside ? vol[((long)z * g.H + y) * g.W + x] : 0.f;
  }
  for (int j = k + 1; j < k_end; ++j) {
    const int32_t* r = ops + j * PYTC_AUG_ROW;
    if (r[0] == PYTC_AUG_MULADD) {
      const float product = v * __int_as_float(r[2]);      // rounded here ...
      v = product + __int_as_float(r[3]);                  // ... and again here: contraction is off
    }
  }
  return v;
}

template <bool VEC>
__global__ void __launch_bounds__(AUG_THREADS) aug_defects_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                                  const int32_t* __restrict__ ops, const int32_t* __restrict__ offsets,
                                                                  int total_rows, AugGeo g) {
  __shared__ int32_t rows[PYTC_AUG_MAX_OPS * PYTC_AUG_ROW];
  const int nc = blockIdx.y, n = nc / g.C;
  int first = offsets[n], count = offsets[n + 1] - first;
  if (first < 0 || count < 0 || count > PYTC_AUG_MAX_OPS || first > total_rows - count) count = 0;      // not the table the launch checked
  for (int i = threadIdx.x; i < count * PYTC_AUG_ROW; i += AUG_THREADS) rows[i] = ops[(long)first * PYTC_AUG_ROW + i];
  __syncthreads();
  const float* vol = in + (long)nc * g.V;
  float* dst = out + (long)nc * g.V;
  const long HW = (long)g.H * g.W;
  const long tile0 = (long)blockIdx.x * AUG_TILE;
  for (int pass = 0; pass < AUG_PASSES; ++pass) {
    const long p0 = tile0 + ((long)pass * AUG_THREADS + threadIdx.x) * AUG_VPL;
    if (p0 >= g.V) continue;
    if (VEC && count == 0) {                               // a sample without rows: a copy
      *reinterpret_cast<f32x4_t*>(dst + p0) = *reinterpret_cast<const f32x4_t*>(vol + p0);
      continue;
    }
    int z = (int)(p0 / HW);
    const int rem = (int)(p0 - (long)z * HW);
    int y = rem / g.W, x = rem - y * g.W;
    float v[AUG_VPL];
#pragma unroll
    for (int j = 0; j < AUG_VPL; ++j) {
      v[j] = p0 + j < g.V ? aug_eval<true>(vol, rows, count, 0, z, y, x, g) : 0.f;
      if (++x == g.W) {                                    // carry over a row / plane end
        x = 0;
        if (++y == g.H) {
          y = 0;
          ++z;
        }
      }
    }
    if (VEC) {
      *reinterpret_cast<f32x4_t*>(dst + p0) = f32x4_t{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
      for (int j = 0; j < AUG_VPL; ++j)
        if (p0 + j < g.V) dst[p0 + j] = v[j];
    }
  }
}

static bool aug_overlap(const void* a, const void* b, long bytes) {
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return pa < pb + bytes && pb < pa + bytes;
}

static bool aug_aligned16(const void* a, const void* b) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0;
}

}  // namespace pytc

using namespace pytc;

extern "C" int pytc_augment_tile(void) { return AUG_TILE; }

#define PYTC_AUG_SHAPE(what)                                                                                                       \
  PYTC_REQUIRE(N >= 1 && C >= 1 && D >= 1 && H >= 1 && W >= 1, "%s: bad shape N %d, C %d, D %d, H %d, W %d", what, N, C, D, H, W); \
  PYTC_REQUIRE((long)N * C <= 65535, "%s: N C = %ld exceeds 65535", what, (long)N * C);                                            \
  PYTC_REQUIRE((long)D * H * W <= 0x3fffffffL, "%s: %ld voxels per sample", what, (long)D * H * W)

extern "C" int pytc_augment_permute(const void* in, void* out, const int32_t* perm, const int32_t* perm_host, int N, int C, int D, int H,
                                    int W, void* stream) {
  const char* what = "augment_permute";
  PYTC_REQUIRE(in && out && perm && perm_host, "%s: in, out, perm and perm_host are required", what);
  PYTC_AUG_SHAPE(what);
  AugGeo g{C, D, H, W, (long)D * H * W};
  PYTC_REQUIRE(!aug_overlap(in, out, (long)N * C * g.V * 4), "%s: out must not alias in (a voxel reads another voxel's input)", what);
  bool lines = false, tiles = false;
  for (int n = 0; n < N; ++n) {
    const int32_t* v = perm_host + 3 * n;
    int seen = 0;
    for (int a = 0; a < 3; ++a) {
      const int s = v[a] < 0 ? -1 - v[a] : v[a];
      PYTC_REQUIRE(s >= 0 && s <= 2, "%s: sample %d: entry %d of (%d, %d, %d) names no axis", what, n, a, v[0], v[1], v[2]);
      seen |= 1 << s;
    }
    PYTC_REQUIRE(seen == 7, "%s: sample %d: (%d, %d, %d) is not a signed permutation of the axes", what, n, v[0], v[1], v[2]);
    AugMap m;
    if (!aug_decode(v, D, H, W, m)) {
      set_error("%s: sample %d: permutation (%d, %d, %d) moves an axis of a (%d, %d, %d) volume onto one of another length", what, n, v[0],
                v[1], v[2], D, H, W);
      return PYTC_ERR_UNSUPPORTED;
    }
    (m.src[2] == 2 ? lines : tiles) = true;
  }
  PYTC_REQUIRE(!tiles || (D > H ? D : H) <= 65535, "%s: %d planes for the tile kernel", what, D > H ? D : H);   // before any launch
  hipStream_t st = (hipStream_t)stream;
  const uint32_t* src = static_cast<const uint32_t*>(in);
  uint32_t* dst = static_cast<uint32_t*>(out);
  if (lines) {
    const dim3 grid(ceil_div(g.V, AUG_TILE), N * C);
    if (W % AUG_VPL == 0 && aug_aligned16(in, out))
      hipLaunchKernelGGL((aug_permute_lines_kernel<true>), grid, dim3(AUG_THREADS), 0, st, src, dst, perm, g);
    else
      hipLaunchKernelGGL((aug_permute_lines_kernel<false>), grid, dim3(AUG_THREADS), 0, st, src, dst, perm, g);
    PYTC_LAUNCH_CHECK("augment_permute");
  }
  if (tiles) {
    const int tiles_w = ceil_div(W, AUG_TS);
    const dim3 grid(tiles_w * tiles_w, D > H ? D : H, N * C);
    hipLaunchKernelGGL(aug_permute_tiles_kernel, grid, dim3(AUG_THREADS), 0, st, src, dst, perm, g, tiles_w);
    PYTC_LAUNCH_CHECK("augment_permute");
  }
  return PYTC_OK;
}

extern "C" int pytc_augment_defects(const float* in, float* out, const int32_t* ops, const int32_t* offsets, const int32_t* ops_host,
                                    const int32_t* offsets_host, int N, int C, int D, int H, int W, void* stream) {
  const char* what = "augment_defects";
  PYTC_REQUIRE(in && out && offsets && offsets_host, "%s: in, out, offsets and offsets_host are required", what);
  PYTC_AUG_SHAPE(what);
  AugGeo g{C, D, H, W, (long)D * H * W};
  PYTC_REQUIRE(!aug_overlap(in, out, (long)N * C * g.V * 4), "%s: out must not alias in (a voxel reads another voxel's input)", what);
  PYTC_REQUIRE(offsets_host[0] == 0, "%s: offsets start at %d, not 0", what, offsets_host[0]);
  const int total = offsets_host[N];
  PYTC_REQUIRE(total >= 0 && (total == 0 || (ops && ops_host)), "%s: %d rows need ops and ops_host", what, total);
  const int dims[3] = {D, H, W};
  for (int n = 0; n < N; ++n) {
    const int first = offsets_host[n], count = offsets_host[n + 1] - first;
    PYTC_REQUIRE(count >= 0, "%s: offsets decrease at sample %d", what, n);
    if (count > PYTC_AUG_MAX_OPS) {
      set_error("%s: sample %d has %d rows; one launch walks at most %d per sample", what, n, count, PYTC_AUG_MAX_OPS);
      return PYTC_ERR_UNSUPPORTED;
    }
    int mean_group = 0, mean_groups = 0;
    for (int k = first; k < first + count; ++k) {
      const int32_t* r = ops_host + (long)k * PYTC_AUG_ROW;
      const int32_t* p = r + 2;
      switch (r[0]) {
        case PYTC_AUG_FILL:
          for (int a = 0; a < 3; ++a)
            PYTC_REQUIRE(p[2 * a] >= 0 && p[2 * a] <= p[2 * a + 1] && p[2 * a + 1] <= dims[a],
                         "%s: row %d: fill box [%d, %d) along axis %d of length %d", what, k, p[2 * a], p[2 * a + 1], a, dims[a]);
          break;
        case PYTC_AUG_MOVE:
          PYTC_REQUIRE(p[0] >= 0 && p[0] <= 2, "%s: row %d: move along axis %d", what, k, p[0]);
          PYTC_REQUIRE(p[1] >= 0 && p[1] <= p[2] && p[2] <= dims[p[0]], "%s: row %d: slab [%d, %d) along axis %d of length %d", what, k,
                       p[1], p[2], p[0], dims[p[0]]);
          PYTC_REQUIRE(p[3] > -0x40000000 && p[3] < 0x40000000 && p[4] > -0x40000000 && p[4] < 0x40000000 && (p[5] == 0 || p[5] == 1),
                       "%s: row %d: shift (%d, %d), wrap %d", what, k, p[3], p[4], p[5]);
          break;
        case PYTC_AUG_COPY_SECTION:
          PYTC_REQUIRE(p[0] >= 1 && p[0] <= D - 2 && p[1] >= -1 && p[1] <= 1, "%s: row %d: section %d of %d from %d", what, k, p[0], D, p[1]);
          if (p[1] == 0 && (mean_groups == 0 || r[1] == 0 || r[1] != mean_group)) {
            ++mean_groups;
            mean_group = r[1];
          }
          break;
        case PYTC_AUG_MULADD:
          break;
        default:
          PYTC_REQUIRE(false, "%s: row %d: unknown op kind %d", what, k, r[0]);
      }
    }
    if (mean_groups > 1) {
      set_error("%s: sample %d interpolates sections in %d groups; one launch evaluates one level of means", what, n, mean_groups);
      return PYTC_ERR_UNSUPPORTED;
    }
  }
  const dim3 grid(ceil_div(g.V, AUG_TILE), N * C);
  hipStream_t st = (hipStream_t)stream;
  if (g.V % AUG_VPL == 0 && aug_aligned16(in, out))
    hipLaunchKernelGGL((aug_defects_kernel<true>), grid, dim3(AUG_THREADS), 0, st, in, out, ops, offsets, total, g);
  else
    hipLaunchKernelGGL((aug_defects_kernel<false>), grid, dim3(AUG_THREADS), 0, st, in, out, ops, offsets, total, g);
  PYTC_LAUNCH_CHECK("augment_defects");
  return PYTC_OK;
}
