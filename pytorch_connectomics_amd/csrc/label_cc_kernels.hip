// Connected components of an integer id volume on the MI355X: what cc3d.connected_components computes for the reference's
// RelabelConnectedComponentsd (data/processing/transforms.py:537-581) and its decoding postprocessing (decoding/stage.py:87-111),
// and the size filter of cc3d.dust.  The union-find of cc_kernels.hip with another edge rule: the same invariants, the same tile, the
// shared launches of cc_shared.h.  Integers only.
//
// N volumes (A0, A1, A2) in one buffer, N A0 A1 A2 < 2^31 - 1; g = n V + (i0 A1 + i1) A2 + i2 is a voxel's index in the batch.  Two
// voxels of one sample are joined iff they carry the same id, the id is not 0, and one is a 6- / 18- / 26-neighbour of the other.
// Negative ids are ids.  A component's HEAD is its smallest voxel, which is its root; components are numbered 1 .. K_n in raster order
// of their heads, anew in every sample.
//
// INVARIANT, as in cc_kernels.hip: parent[i] <= i while unions run and a value only decreases; every find falls strictly and ends
// whatever it reads; label_merge stores to parent only through agent-scope atomicMin and loads it through agent-scope atomic loads.
// No loop has an iteration cap, none waits for another workgroup, nothing is read back.
//
// EDGES are not stored.  A voxel compares its id with the ids at the offsets cc_core.h names (nb_wanted) and unites the forward edges
// needed_edges leaves: a diagonal edge whose ends a voxel between them already joins is left out.  The decision reads ids only, so
// label_local (ids staged in LDS, the neighbour inside the tile) and label_merge (global ids, the neighbour inside the sample but in
// another tile) make it alike, and every forward edge belongs to exactly one of the two launches.  A diagonal edge may leave a tile
// through an edge or a corner into a tile that shares no face with it: label_merge looks at a voxel's own offsets, not at tile faces,
// so each such pair is one forward offset of one voxel, taken once.
//
// LAUNCHES: label_local, label_merge, cc_flatten, cc_rank, cc_scan, cc_number (cc_shared.h, over the batch as one run of N V voxels,
// which numbers the heads of the whole batch 1 .. K), label_bases (bases[n] = the heads before sample n: the scanned count of the rank
// block that holds g = n V plus the heads of that block before g; count[n] = bases[n + 1] - bases[n]), label_apply
// (labels = the id in the root's slot - bases[n]).  Eight launches for any N.
// Dust: dust_clear (the first count[n] cells of sample n's table and kept[n]), dust_count (integer atomics, one per run of equal labels
// among a lane's 8 voxels, a lane's last run summed over the wave first), dust_kept, dust_apply.
//
// MEMORY.  1 byte (head flag) + 4 (parent) + 4 (labels) per voxel and 4 bytes per 2048 voxels, all the caller's.  The size table is
// N V int32, cell n V + label - 1: the parent array, dead after label_apply, serves.
#include "cc_shared.h"

namespace pytc {

struct LabelGeo {
  int A0, A1, A2, t0, t1, t2, N, level;                    // t*: tiles per axis of one sample
  long V, VT;                                              // voxels of a sample, of the batch
};

// ---------------------------------------------------------------------------------------------------------------------- label_local
__global__ void __launch_bounds__(CC_THREADS) label_local_kernel(const int32_t* __restrict__ ids, uint32_t* __restrict__ parent,
                                                                 uint8_t* __restrict__ flags, LabelGeo g) {
  __shared__ uint32_t lab[TILE];
  __shared__ int32_t idt[TILE];
  long b = blockIdx.x;
  const int x0 = (int)(b % g.t2) * TX;
  b /= g.t2;
  const int y0 = (int)(b % g.t1) * TY;
  b /= g.t1;
  const int z0 = (int)(b % g.t0) * TZ;
  const long base = (b / g.t0) * g.V;                      // the sample's first voxel
  long at[CC_PER_THREAD];                                  // the batch index of the thread's voxels, -1 outside the volume
#pragma unroll
  for (int k = 0; k < CC_PER_THREAD; ++k) {
    const int li = k * CC_THREADS + threadIdx.x;
    const int lx = li % TX, ly = (li / TX) % TY, lz = li / (TX * TY);
    const int z = z0 + lz, y = y0 + ly, x = x0 + lx;
    const bool in = z < g.A0 && y < g.A1 && x < g.A2;
    at[k] = in ? base + ((long)z * g.A1 + y) * g.A2 + x : -1;
    idt[li] = in ? ids[at[k]] : 0;                         // outside the volume: id 0 joins nothing
    lab[li] = li;
  }
  __syncthreads();
  LdsLabels m{lab};
#pragma unroll
  for (int k = 0; k < CC_PER_THREAD; ++k) {
    const int li = k * CC_THREADS + threadIdx.x;
    const int lx = li % TX, ly = (li / TX) % TY, lz = li / (TX * TY);
    const int32_t id = idt[li];
    if (id == 0) continue;
    uint32_t same = 0;
#pragma unroll
    for (int nb = 0; nb < NB_BITS; ++nb) {
      if (!nb_wanted(nb, g.level)) continue;
      int d0, d1, d2;
      nb_offset(nb, d0, d1, d2);
      const int nz = lz + d0, ny = ly + d1, nx = lx + d2;
      if (nz < TZ && ny >= 0 && ny < TY && nx >= 0 && nx < TX && idt[(nz * TY + ny) * TX + nx] == id) same |= 1u << nb;
    }
    const uint32_t need = needed_edges(same, g.level);
#pragma unroll
    for (int nb = NB_SELF + 1; nb < NB_BITS; ++nb) {
      if (!((need >> nb) & 1u)) continue;
      int d0, d1, d2;
      nb_offset(nb, d0, d1, d2);
      unite(m, (uint32_t)li, (uint32_t)(li + (d0 * TY + d1) * TX + d2));
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < CC_PER_THREAD; ++k) {
    if (at[k] < 0) continue;
    const int li = k * CC_THREADS + threadIdx.x;
    uint32_t out = BACKGROUND;
    if (idt[li] != 0) {
      const int r = (int)find(m, (uint32_t)li);            // labels are final: no union runs any more
      const int rx = r % TX, ry = (r / TX) % TY, rz = r / (TX * TY);
      out = (uint32_t)(base + ((long)(z0 + rz) * g.A1 + (y0 + ry)) * g.A2 + (x0 + rx));
    }
    parent[at[k]] = out;
    flags[at[k]] = idt[li] != 0 ? (uint8_t)EDGE_FG : (uint8_t)0;
  }
}

// ---------------------------------------------------------------------------------------------------------------------- label_merge
__global__ void __launch_bounds__(CC_THREADS) label_merge_kernel(const int32_t* __restrict__ ids, uint32_t* parent, LabelGeo g) {
  const long v = (long)blockIdx.x * CC_THREADS + threadIdx.x;
  if (v >= g.VT) return;
  const long plane = (long)g.A1 * g.A2;
  const long r = v % g.V;                                  // inside its sample
  const int i0 = (int)(r / plane);
  const int rem = (int)(r - (long)i0 * plane);
  const int i1 = rem / g.A2, i2 = rem - i1 * g.A2;
  const int lz = i0 % TZ, ly = i1 % TY, lx = i2 % TX;
  // a forward offset leaves the tile upwards along axis 0, either way along the other two (never with level 1)
  const bool up = lz == TZ - 1 || ly == TY - 1 || lx == TX - 1;
  if (!(up || (g.level > 1 && (ly == 0 || lx == 0)))) return;
  const int32_t id = ids[v];
  if (id == 0) return;
  uint32_t same = 0;
#pragma unroll
  for (int nb = 0; nb < NB_BITS; ++nb) {
    if (!nb_wanted(nb, g.level)) continue;
    int d0, d1, d2;
    nb_offset(nb, d0, d1, d2);
    const int n0 = i0 + d0, n1 = i1 + d1, n2 = i2 + d2;
    if (n0 < g.A0 && n1 >= 0 && n1 < g.A1 && n2 >= 0 && n2 < g.A2 && ids[v + d0 * plane + d1 * (long)g.A2 + d2] == id) same |= 1u << nb;
  }
  const uint32_t need = needed_edges(same, g.level);
  AgentParents m{parent};
#pragma unroll
  for (int nb = NB_SELF + 1; nb < NB_BITS; ++nb) {
    if (!((need >> nb) & 1u)) continue;
    int d0, d1, d2;
    nb_offset(nb, d0, d1, d2);
    const int nz = lz + d0, ny = ly + d1, nx = lx + d2;
    if (nz < TZ && ny >= 0 && ny < TY && nx >= 0 && nx < TX) continue;       // inside the tile: label_local's edge
    unite(m, (uint32_t)v, (uint32_t)(v + d0 * plane + d1 * (long)g.A2 + d2));
  }
}

// ---------------------------------------------------------------------------------------------------------------------- label_bases
// Workgroup n: the heads before sample n and before sample n + 1, each from the scanned count of the rank block that holds the
// sample's first voxel and the head flags of that block before it.  ktotal[0] = the heads of the batch.
__global__ void __launch_bounds__(CC_THREADS) label_bases_kernel(const uint8_t* __restrict__ flags, const int32_t* __restrict__ offsets,
                                                                 const int32_t* __restrict__ ktotal, int32_t* __restrict__ bases,
                                                                 int32_t* __restrict__ count, LabelGeo g) {
  __shared__ int wave_sums[CC_THREADS / WAVE];
  const int n = blockIdx.x;
  int before[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const long end = (long)(n + s) * g.V;                  // n + s == N: the end of the batch
    const long block = end / RANK_BLOCK, first = block * RANK_BLOCK + (long)threadIdx.x * RANK_PER;
    int c = 0;
#pragma unroll
    for (int j = 0; j < RANK_PER; ++j) c += (first + j < end && (flags[first + j] & EDGE_HEAD)) ? 1 : 0;
    int total;
    block_exclusive_scan<CC_THREADS>(c, wave_sums, total);
    before[s] = n + s == g.N ? ktotal[0] : offsets[block] + total;
  }
  if (threadIdx.x == 0) {
    bases[n] = before[0];
    count[n] = before[1] - before[0];
  }
}

// ---------------------------------------------------------------------------------------------------------------------- label_apply
__global__ void __launch_bounds__(CC_THREADS) label_apply_kernel(const uint32_t* __restrict__ parent, const int32_t* __restrict__ bases,
                                                                 int32_t* __restrict__ labels, LabelGeo g) {
  const long v = (long)blockIdx.x * CC_THREADS + threadIdx.x;
  if (v >= g.VT) return;
  const uint32_t p = parent[v];
  labels[v] = p == BACKGROUND ? 0 : (int32_t)(parent[root_of(p, (uint32_t)v)] & ~TAG) - bases[v / g.V];
}

// ----------------------------------------------------------------------------------------------------------------------------- dust
constexpr int DUST_RUN = 8;                                // consecutive voxels of a lane in dust_count: 32 bytes of labels

__global__ void __launch_bounds__(CC_THREADS) dust_clear_kernel(int32_t* __restrict__ table, int32_t* __restrict__ kept,
                                                                const int32_t* __restrict__ count, long V, long VT) {
  const long i = (long)blockIdx.x * CC_THREADS + threadIdx.x;
  if (i >= VT) return;
  const long n = i / V, j = i - n * V;
  if (j < count[n]) table[i] = 0;
  if (j == 0) kept[n] = 0;
}

// Sizes by integer atomics.  A lane walks DUST_RUN consecutive voxels and adds once per run of equal labels; its last run -- for a lane
// inside a large component its only one -- is first summed over the neighbouring lanes of the wave that end in the same cell (a
// segmented scan in lane order, six shuffle steps), and the last lane of such a stretch adds the sum.  One address takes one atomic per
// wave and component instead of one per lane (solid segments: 1.40 -> 0.27 ms at 165 x 1024 x 768; ids that change every voxel or two
// still pay close to one atomic per foreground voxel).
__global__ void __launch_bounds__(CC_THREADS) dust_count_kernel(const int32_t* __restrict__ labels, int32_t* table, long V, long VT) {
  const long first = ((long)blockIdx.x * CC_THREADS + threadIdx.x) * DUST_RUN;
  long n = first < VT ? first / V : 0;
  int cell = -1;                                           // the table cell of the run in hand (cells are indices below N V < 2^31)
  int run = 0;
#pragma unroll
  for (int j = 0; j < DUST_RUN; ++j) {
    const long v = first + j;
    if (v >= VT) break;
    while (v >= (n + 1) * V) ++n;                          // a lane's voxels may pass into the next samples
    const int32_t l = labels[v];
    const int c = (l <= 0 || l > V) ? -1 : (int)(n * V + l - 1);    // 1 .. count[n] <= V from label_cc; anything else has no cell
    if (c != cell) {
      if (cell >= 0) atomicAdd(table + cell, run);
      cell = c;
      run = 0;
    }
    ++run;
  }
  // every lane of the wave is here (none has returned): the shuffles below read all of them
  const int lane = threadIdx.x % WAVE;
  const int before = __shfl_up(cell, 1, WAVE), after = __shfl_down(cell, 1, WAVE);
  bool head = lane == 0 || before != cell;                 // the first lane of a stretch of equal cells
  const bool tail = lane == WAVE - 1 || after != cell;
  int sum = run;
#pragma unroll
  for (int o = 1; o < WAVE; o <<= 1) {
    const int s = __shfl_up(sum, o, WAVE);
    const bool h = __shfl_up((int)head, o, WAVE) != 0;
    if (lane >= o && !head) {
      sum += s;
      head = h;
    }
  }
  if (tail && cell >= 0) atomicAdd(table + cell, sum);
}

// kept[n] += the cells of sample n that hold min_size or more.  Lanes of a wave that share a sample add once.
__global__ void __launch_bounds__(CC_THREADS) dust_kept_kernel(const int32_t* __restrict__ table, const int32_t* __restrict__ count,
                                                               int32_t* kept, int min_size, long V, long VT) {
  const long i = (long)blockIdx.x * CC_THREADS + threadIdx.x;
  const bool in = i < VT;
  const int n = in ? (int)(i / V) : 0;
  bool pass = in && i - (long)n * V < count[n] && table[i] >= min_size;
  const int lane = threadIdx.x % WAVE;
  for (unsigned long long left = __ballot(pass); left; left = __ballot(pass)) {       // one round per sample the wave's lanes touch
    const int leader = __ffsll(left) - 1;
    const int ln = __shfl(n, leader, WAVE);
    const unsigned long long group = __ballot(pass && n == ln);
    if (lane == leader) atomicAdd(kept + ln, __popcll(group));
    if (n == ln) pass = false;
  }
}

__global__ void __launch_bounds__(CC_THREADS) dust_apply_kernel(const int32_t* labels, const int32_t* __restrict__ table, int32_t* out,
                                                                int min_size, long V, long VT) {
  const long v = (long)blockIdx.x * CC_THREADS + threadIdx.x;
  if (v >= VT) return;
  const int32_t l = labels[v];
  out[v] = (l <= 0 || l > V || table[(v / V) * V + l - 1] < min_size) ? 0 : l;
}

static bool label_cc_shape(const char* what, int N, int A0, int A1, int A2, long& V, long& VT, int& status) {
  status = PYTC_ERR_INVALID;
  if (!(N >= 1 && A0 >= 1 && A1 >= 1 && A2 >= 1)) {
    set_error("%s: bad shape %d x (%d, %d, %d)", what, N, A0, A1, A2);
    return false;
  }
  V = (long)A0 * A1 * A2;
  VT = V >= 0x7fffffffL ? V : V * N;
  if (VT >= 0x7fffffffL) {
    status = PYTC_ERR_UNSUPPORTED;
    set_error("%s: %d x %ld voxels; indices and component numbers are 31 bits and 2^31 - 1 is kept for the background", what, N, V);
    return false;
  }
  return true;
}

}  // namespace pytc

using namespace pytc;

extern "C" int pytc_label_cc_tile(int axis) { return axis == 0 ? TZ : (axis == 1 ? TY : (axis == 2 ? TX : 0)); }

extern "C" int64_t pytc_label_cc_rank_block(void) { return RANK_BLOCK; }

extern "C" int64_t pytc_label_cc_counts(int64_t samples, int64_t voxels) {
  if (samples < 1 || voxels < 1 || voxels >= 0x7fffffffL || samples * voxels >= 0x7fffffffL) return 0;
  return (samples * voxels + RANK_BLOCK - 1) / RANK_BLOCK + 1 + samples;
}

extern "C" int64_t pytc_label_cc_table(int64_t samples, int64_t voxels) {
  if (samples < 1 || voxels < 1 || voxels >= 0x7fffffffL || samples * voxels >= 0x7fffffffL) return 0;
  return samples * voxels;
}

extern "C" int pytc_label_cc(const int32_t* ids, int connectivity, void* flags, void* parent, int32_t* counts, int32_t* labels,
                             int32_t* count, int N, int A0, int A1, int A2, void* stream) {
  const char* what = "label_cc";
  PYTC_REQUIRE(ids && flags && parent && counts && labels && count, "%s: ids, flags, parent, counts, labels and count are required", what);
  long V, VT;
  int status;
  if (!label_cc_shape(what, N, A0, A1, A2, V, VT, status)) return status;
  const int level = connectivity_level(connectivity);
  if (!level) {
    set_error("%s: connectivity %d is none of 6, 18, 26", what, connectivity);
    return PYTC_ERR_UNSUPPORTED;
  }
  PYTC_REQUIRE(reinterpret_cast<uintptr_t>(ids) % 4 == 0 && reinterpret_cast<uintptr_t>(parent) % 4 == 0 &&
               reinterpret_cast<uintptr_t>(counts) % 4 == 0 && reinterpret_cast<uintptr_t>(labels) % 4 == 0 &&
               reinterpret_cast<uintptr_t>(count) % 4 == 0, "%s: ids, parent, counts, labels and count must be 4-byte aligned", what);
  const long blocks = ceil_div(VT, RANK_BLOCK);
  const void* bufs[6] = {ids, flags, parent, counts, labels, count};
  const long bytes[6] = {4 * VT, VT, 4 * VT, 4 * (long)pytc_label_cc_counts(N, V), 4 * VT, 4L * N};
  const char* names[6] = {"ids", "flags", "parent", "counts", "labels", "count"};
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < i; ++j)
      PYTC_REQUIRE(!ranges_overlap(bufs[i], bytes[i], bufs[j], bytes[j]), "%s: %s must not alias %s", what, names[i], names[j]);
  LabelGeo g{A0, A1, A2, ceil_div(A0, TZ), ceil_div(A1, TY), ceil_div(A2, TX), N, level, V, VT};
  const long tiles = (long)g.t0 * g.t1 * g.t2 * N;
  PYTC_REQUIRE(tiles <= 0x7fffffffL, "%s: %ld tiles", what, tiles);
  hipStream_t st = (hipStream_t)stream;
  uint8_t* f8 = static_cast<uint8_t*>(flags);
  uint32_t* par = static_cast<uint32_t*>(parent);
  int32_t* ktotal = counts + blocks;
  int32_t* bases = ktotal + 1;
  const dim3 per_voxel(ceil_div(VT, CC_THREADS)), threads(CC_THREADS);
  hipLaunchKernelGGL(label_local_kernel, dim3((unsigned)tiles), threads, 0, st, ids, par, f8, g);
  PYTC_LAUNCH_CHECK("label_cc (local)");
  hipLaunchKernelGGL(label_merge_kernel, per_voxel, threads, 0, st, ids, par, g);
  PYTC_LAUNCH_CHECK("label_cc (merge)");
  hipLaunchKernelGGL(cc_flatten_kernel, per_voxel, threads, 0, st, par, VT, 0);
  PYTC_LAUNCH_CHECK("label_cc (flatten)");
  hipLaunchKernelGGL(cc_rank_kernel, dim3((unsigned)blocks), threads, 0, st, par, f8, counts, VT);
  PYTC_LAUNCH_CHECK("label_cc (rank)");
  hipLaunchKernelGGL(cc_scan_kernel, dim3(1), dim3(CC_SCAN_THREADS), 0, st, counts, ktotal, (int)blocks);
  PYTC_LAUNCH_CHECK("label_cc (scan)");
  hipLaunchKernelGGL(cc_number_kernel, dim3((unsigned)blocks), threads, 0, st, par, f8, counts, VT);
  PYTC_LAUNCH_CHECK("label_cc (number)");
  hipLaunchKernelGGL(label_bases_kernel, dim3(N), threads, 0, st, f8, counts, ktotal, bases, count, g);
  PYTC_LAUNCH_CHECK("label_cc (bases)");
  hipLaunchKernelGGL(label_apply_kernel, per_voxel, threads, 0, st, par, bases, labels, g);
  PYTC_LAUNCH_CHECK("label_cc (apply)");
  return PYTC_OK;
}

extern "C" int pytc_label_cc_dust(const int32_t* labels, const int32_t* count, int min_size, int32_t* table, int32_t* out, int32_t* kept,
                                  int N, int A0, int A1, int A2, void* stream) {
  const char* what = "label_cc_dust";
  PYTC_REQUIRE(labels && count && table && out && kept, "%s: labels, count, table, out and kept are required", what);
  long V, VT;
  int status;
  if (!label_cc_shape(what, N, A0, A1, A2, V, VT, status)) return status;
  PYTC_REQUIRE(min_size >= 1, "%s: min_size %d removes nothing; the caller skips the call", what, min_size);
  PYTC_REQUIRE(reinterpret_cast<uintptr_t>(labels) % 4 == 0 && reinterpret_cast<uintptr_t>(count) % 4 == 0 &&
               reinterpret_cast<uintptr_t>(table) % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 4 == 0 &&
               reinterpret_cast<uintptr_t>(kept) % 4 == 0, "%s: every buffer must be 4-byte aligned", what);
  const void* bufs[5] = {labels, count, table, out, kept};
  const long bytes[5] = {4 * VT, 4L * N, 4 * VT, 4 * VT, 4L * N};
  const char* names[5] = {"labels", "count", "table", "out", "kept"};
  for (int i = 0; i < 5; ++i)
    for (int j = 0; j < i; ++j) {
      if (i == 3 && j == 0 && out == labels) continue;     // in place: dust_apply reads and writes a voxel in one thread
      PYTC_REQUIRE(!ranges_overlap(bufs[i], bytes[i], bufs[j], bytes[j]), "%s: %s must not alias %s", what, names[i], names[j]);
    }
  hipStream_t st = (hipStream_t)stream;
  const dim3 per_voxel(ceil_div(VT, CC_THREADS)), threads(CC_THREADS);
  hipLaunchKernelGGL(dust_clear_kernel, per_voxel, threads, 0, st, table, kept, count, V, VT);
  PYTC_LAUNCH_CHECK("label_cc_dust (clear)");
  hipLaunchKernelGGL(dust_count_kernel, dim3(ceil_div(VT, (long)CC_THREADS * DUST_RUN)), threads, 0, st, labels, table, V, VT);
  PYTC_LAUNCH_CHECK("label_cc_dust (count)");
  hipLaunchKernelGGL(dust_kept_kernel, per_voxel, threads, 0, st, table, count, kept, min_size, V, VT);
  PYTC_LAUNCH_CHECK("label_cc_dust (kept)");
  hipLaunchKernelGGL(dust_apply_kernel, per_voxel, threads, 0, st, labels, table, out, min_size, V, VT);
  PYTC_LAUNCH_CHECK("label_cc_dust (apply)");
  return PYTC_OK;
}
