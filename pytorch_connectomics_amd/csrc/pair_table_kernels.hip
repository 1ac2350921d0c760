// The label-pair table of two id volumes on the MI355X: n[g][s] = the number of voxels with ground-truth id g and segmentation id s,
// as a sparse open-addressing hash table, and from it the integers adapted Rand, VOI and instance matching are functions of
// (the reference's metrics/segmentation_numpy.py adapted_rand, voi, instance_matching, instance_matching_simple, which build a scipy
// sparse matrix from N ones and a dense n_true x n_pred overlap matrix on the host).  Integers only, apart from log2 in the VOI terms,
// which are rounded to fixed point before they are added: every cell of the record is the same from call to call.
//
// Two volumes of N < 2^31 - 1 ids, int32 or int64 in any combination, 0 <= id <= 2^31 - 2.  pair_table_core.h holds the table, the
// termination argument of its probe loop and every per-thread step; this file holds the memories and the launches.
//
// LAUNCHES.  pytc_pair_table_runs:
//   pt_runs       one streaming pass: U = the positions whose (gt, seg) differs from its predecessor in memory order, an upper bound
//                 of the number of distinct pairs, and a flag word (bit 0: gt, bit 1: seg holds an id outside the range).  The host
//                 reads both -- the one read before the build -- and sizes the table: cap = the smallest power of two >= 2 U.
// pytc_pair_table_build (refuses cap < 2 U):
//   pt_build      a lane reads LANE_RUN consecutive voxels of both volumes with 16-byte loads and merges equal neighbours in
//                 registers; its runs go to the workgroup's LDS table (LDS_SLOTS slots, direct-mapped: the smallest key offered to
//                 a free slot owns it, whichever lane came first), and straight to the global table when their slot is another
//                 key's.  A workgroup walks its spans one after the other and flushes its LDS table at the end: one global update
//                 per distinct pair it held.  The number of updates is therefore the same from call to call.  A global key is
//                 claimed by a 64-bit compare-exchange and the count added by a 64-bit fetch-add, both relaxed at agent scope, and
//                 keys are only ever read by agent-scope atomic loads: the L2s of the eight XCDs are not coherent with each other
//                 inside a launch.  No thread waits for another.
//   pt_marginals  (a new launch: the table is visible to plain loads) every occupied slot adds n to A[g] in the table of gt ids and
//                 Bfull[s] << 32 | B1[s] to the table of seg ids, through an LDS table with bounded probing.  Both tables have cap slots too:
//                 the distinct ids of either volume are no more than the distinct pairs.  Nothing is sized by the largest id.
//   pt_sums       the three tables -> the int64 record (pair_table_core.h Cell): register sums, a workgroup sum, one 64-bit integer
//                 atomic add per cell and workgroup.  Integer adds commute: the cells are exact and identical in any order.
//   pt_finish     one thread: the two VOI sums X_A - X_N and X_B - X_N.
// pytc_pair_table_matches:
//   pt_matches    every occupied slot with g, s >= 1 looks A[g] and Bfull[s] up and evaluates the float32 score rule; the passing
//                 pairs are counted and compacted (one atomic add per wave) into the caller's buffer, in no particular order.
//
// MEMORY.  48 bytes per slot (three tables of key and value), cap <= max(4 U, 256) slots, 128 bytes of record; no more per voxel.
#include <cstdint>

#include "pair_table_core.h"
#include "pytc_common.h"

namespace pytc {

using namespace pt;

typedef unsigned long long u64;
static_assert(sizeof(u64) == sizeof(uint64_t), "64-bit table words");
static_assert((LDS_SLOTS & (LDS_SLOTS - 1)) == 0 && LDS_SLOTS % THREADS == 0 && MIN_CAP % THREADS == 0, "whole passes");

// ------------------------------------------------------------------------------------------------- memories of pair_table_core.h
struct LdsTable {                                          // the workgroup's table: workgroup scope
  u64* keys;
  u64* vals;
  __device__ __forceinline__ uint64_t load_key(uint64_t i) { return __hip_atomic_load(keys + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
  __device__ __forceinline__ uint64_t claim(uint64_t i, uint64_t key) {
    u64 seen = EMPTY;
    __hip_atomic_compare_exchange_strong(keys + i, &seen, (u64)key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    return seen;
  }
  __device__ __forceinline__ void add(uint64_t i, uint64_t v) { __hip_atomic_fetch_add(vals + i, (u64)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
  __device__ __forceinline__ void min_key(uint64_t i, uint64_t v) { __hip_atomic_fetch_min(keys + i, (u64)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
  __device__ __forceinline__ void store_key(uint64_t i, uint64_t v) { __hip_atomic_store(keys + i, (u64)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
};

struct AgentTable {                                        // a global table while other workgroups insert: agent scope, atomics only
  u64* keys;
  u64* vals;
  __device__ __forceinline__ uint64_t load_key(uint64_t i) { return __hip_atomic_load(keys + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ __forceinline__ uint64_t claim(uint64_t i, uint64_t key) {
    u64 seen = EMPTY;
    __hip_atomic_compare_exchange_strong(keys + i, &seen, (u64)key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return seen;
  }
  __device__ __forceinline__ void add(uint64_t i, uint64_t v) { __hip_atomic_fetch_add(vals + i, (u64)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};

struct FinishedTable {                                     // a table of an earlier launch: plain loads
  const u64* keys;
  __device__ __forceinline__ uint64_t load_key(uint64_t i) { return keys[i]; }
};

// a lane's LANE_RUN ids from a 16-byte aligned address, as 16-byte loads
__device__ __forceinline__ void load_run(const int32_t* p, int64_t (&v)[LANE_RUN]) {
  const int4* q = reinterpret_cast<const int4*>(p);
#pragma unroll
  for (int j = 0; j < LANE_RUN / 4; ++j) {
    const int4 t = q[j];
    v[4 * j] = t.x;
    v[4 * j + 1] = t.y;
    v[4 * j + 2] = t.z;
    v[4 * j + 3] = t.w;
  }
}
__device__ __forceinline__ void load_run(const int64_t* p, int64_t (&v)[LANE_RUN]) {
  const longlong2* q = reinterpret_cast<const longlong2*>(p);
#pragma unroll
  for (int j = 0; j < LANE_RUN / 2; ++j) {
    const longlong2 t = q[j];
    v[2 * j] = t.x;
    v[2 * j + 1] = t.y;
  }
}

// The keys of the lane's voxels first .. first + m, m = min(LANE_RUN, n - first) >= 1; bad: bit 0 / 1 = a gt / seg id out of range.
template <typename TG, typename TS>
__device__ __forceinline__ int load_keys(const TG* __restrict__ gt, const TS* __restrict__ seg, long first, long n, uint64_t (&keys)[LANE_RUN],
                                         unsigned& bad) {
  int64_t g[LANE_RUN], s[LANE_RUN];
  int m = LANE_RUN;
  if (first + LANE_RUN <= n) {                             // first is a multiple of LANE_RUN and the volumes are 16-byte aligned
    load_run(gt + first, g);
    load_run(seg + first, s);
  } else {
    m = (int)(n - first);
#pragma unroll
    for (int i = 0; i < LANE_RUN; ++i) {
      g[i] = i < m ? (int64_t)gt[first + i] : 0;
      s[i] = i < m ? (int64_t)seg[first + i] : 0;
    }
  }
#pragma unroll
  for (int i = 0; i < LANE_RUN; ++i) {
    bad |= (id_bad(g[i]) ? 1u : 0u) | (id_bad(s[i]) ? 2u : 0u);
    keys[i] = pair_key((uint64_t)(uint32_t)g[i], (uint64_t)(uint32_t)s[i]);
  }
  return m;
}

// --------------------------------------------------------------------------------------------------------------------------- pt_runs
template <typename TG, typename TS>
__global__ void __launch_bounds__(THREADS) pt_runs_kernel(const TG* __restrict__ gt, const TS* __restrict__ seg, long n, long per_wg,
                                                          u64* bound) {
  __shared__ u64 red[THREADS];
  u64 changes = 0;
  unsigned bad = 0;
  for (long k = 0; k < per_wg; ++k) {
    const long first = ((long)blockIdx.x * per_wg + k) * SPAN + (long)threadIdx.x * LANE_RUN;
    if (first >= n) break;
    uint64_t keys[LANE_RUN];
    const int m = load_keys(gt, seg, first, n, keys, bad);
    uint64_t before = 0;
    if (first > 0) before = pair_key((uint64_t)(uint32_t)gt[first - 1], (uint64_t)(uint32_t)seg[first - 1]);
    changes += (u64)count_changes(keys, m, first > 0, before);
  }
  const u64 total = block_sum<THREADS>(changes, red);
  // the flag bits are or-ed, not summed: the number of lanes that saw one, per bit
  const u64 bad_gt = block_sum<THREADS>((u64)(bad & 1u), red), bad_seg = block_sum<THREADS>((u64)((bad >> 1) & 1u), red);
  if (threadIdx.x == 0) {
    if (total) __hip_atomic_fetch_add(bound, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const u64 word = (bad_gt ? 1u : 0u) | (bad_seg ? 2u : 0u);
    if (word) __hip_atomic_fetch_or(bound + 1, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// -------------------------------------------------------------------------------------------------------------------------- pt_build
__device__ __forceinline__ void lds_clear(u64* lkeys, u64* lvals) {
#pragma unroll
  for (int i = threadIdx.x; i < LDS_SLOTS; i += THREADS) {
    lkeys[i] = EMPTY;
    lvals[i] = 0;
  }
  __syncthreads();
}

template <typename TG, typename TS>
__global__ void __launch_bounds__(THREADS) pt_build_kernel(const TG* __restrict__ gt, const TS* __restrict__ seg, long n, long per_wg,
                                                           u64* keys_out, u64* vals_out, int log2_cap, u64* record) {
  __shared__ u64 lkeys[LDS_SLOTS];
  __shared__ u64 lvals[LDS_SLOTS];
  __shared__ u64 red[THREADS];
  lds_clear(lkeys, lvals);
  LdsTable lds{lkeys, lvals};
  AgentTable glob{keys_out, vals_out};
  Propose<LdsTable> offer(lds);
  Commit<LdsTable, AgentTable> emit(lds, glob, log2_cap);
  for (long k = 0; k < per_wg; ++k) {
    const long span_first = ((long)blockIdx.x * per_wg + k) * SPAN;
    if (span_first >= n) break;                            // the whole workgroup: the barriers below stay uniform
    const long first = span_first + (long)threadIdx.x * LANE_RUN;
    uint64_t keys[LANE_RUN];
    unsigned bad = 0;                                      // checked by pt_runs before this launch
    const int m = first < n ? load_keys(gt, seg, first, n, keys, bad) : 0;
    if (m) merge_runs(keys, m, offer);
    __syncthreads();                                       // every offer is in: the slots' keys stand for this span
    if (m) merge_runs(keys, m, emit);
    __syncthreads();                                       // every winner's bit is cleared before the next span offers
  }
  // the closing barrier of the last span: every lane's LDS adds are done, the flush reads plain
#pragma unroll 1
  for (int i = threadIdx.x; i < LDS_SLOTS; i += THREADS)
    if (lkeys[i] != EMPTY) emit.to_global(lkeys[i], lvals[i]);
  const u64 updates = block_sum<THREADS>((u64)emit.updates, red);
  const u64 lost = block_sum<THREADS>((u64)(emit.lost ? 1 : 0), red);
  if (threadIdx.x == 0) {
    __hip_atomic_fetch_add(record + C_UPDATES, updates, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (lost) __hip_atomic_fetch_add(record + C_LOST, lost, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---------------------------------------------------------------------------------------------------------------------- pt_marginals
constexpr uint64_t SEG_SIDE = uint64_t(1) << 32;           // the LDS table holds both sides: a seg id carries this bit

__global__ void __launch_bounds__(THREADS) pt_marginals_kernel(const u64* __restrict__ pkeys, const u64* __restrict__ pvals, u64* gkeys,
                                                               u64* gvals, u64* skeys, u64* svals, long cap, int log2_cap, u64* record) {
  __shared__ u64 lkeys[LDS_SLOTS];
  __shared__ u64 lvals[LDS_SLOTS];
  __shared__ u64 red[THREADS];
  lds_clear(lkeys, lvals);
  LdsTable lds{lkeys, lvals};
  AgentTable gtab{gkeys, gvals}, stab{skeys, svals};
  bool lost = false;
  auto to_global = [&](uint64_t tagged, uint64_t val) {
    const bool seg_side = (tagged & SEG_SIDE) != 0;
    if (!global_add(seg_side ? stab : gtab, tagged & 0xffffffffu, val, log2_cap)) lost = true;
  };
  for (long base = (long)blockIdx.x * THREADS; base < cap; base += (long)gridDim.x * THREADS) {
    const long i = base + threadIdx.x;                     // cap is a multiple of THREADS
    const uint64_t key = pkeys[i];
    if (key == EMPTY) continue;
    const uint64_t n = pvals[i], g = key >> 32, s = key & 0xffffffffu;
    if (!lds_add(lds, g, n)) to_global(g, n);
    const uint64_t sv = seg_marginal(g, n);
    if (!lds_add(lds, s | SEG_SIDE, sv)) to_global(s | SEG_SIDE, sv);
  }
  __syncthreads();
#pragma unroll 1
  for (int i = threadIdx.x; i < LDS_SLOTS; i += THREADS)
    if (lkeys[i] != EMPTY) to_global(lkeys[i], lvals[i]);
  const u64 any = block_sum<THREADS>((u64)(lost ? 1 : 0), red);
  if (threadIdx.x == 0 && any) __hip_atomic_fetch_add(record + C_LOST, any, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// --------------------------------------------------------------------------------------------------------------------------- pt_sums
__global__ void __launch_bounds__(THREADS) pt_sums_kernel(const u64* __restrict__ pkeys, const u64* __restrict__ pvals,
                                                          const u64* __restrict__ gkeys, const u64* __restrict__ gvals,
                                                          const u64* __restrict__ skeys, const u64* __restrict__ svals, long cap, u64* record) {
  __shared__ u64 red[THREADS];
  uint64_t a[RECORD_CELLS];
#pragma unroll
  for (int c = 0; c < RECORD_CELLS; ++c) a[c] = 0;
  for (long base = (long)blockIdx.x * THREADS; base < cap; base += (long)gridDim.x * THREADS) {
    const long i = base + threadIdx.x;
    const uint64_t pk = pkeys[i], gk = gkeys[i], sk = skeys[i];
    if (pk != EMPTY) sums_of_pair(pk, pvals[i], a);
    if (gk != EMPTY) sums_of_gt(gk, gvals[i], a);
    if (sk != EMPTY) sums_of_seg(sk, svals[i], a);
  }
#pragma unroll
  for (int c = 0; c < RECORD_CELLS; ++c) {
    if (c == C_UPDATES || c == C_LOST || c == C_SPLIT || c == C_MERGE) continue;      // not this launch's cells
    const u64 total = block_sum<THREADS>((u64)a[c], red);
    if (threadIdx.x == 0 && total) __hip_atomic_fetch_add(record + c, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ void pt_finish_kernel(u64* record) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  record[C_SPLIT] = record[C_XA] - record[C_XN];
  record[C_MERGE] = record[C_XB] - record[C_XN];
}

// ------------------------------------------------------------------------------------------------------------------------ pt_matches
__global__ void __launch_bounds__(THREADS) pt_matches_kernel(const u64* __restrict__ pkeys, const u64* __restrict__ pvals,
                                                             const u64* __restrict__ gkeys, const u64* __restrict__ gvals,
                                                             const u64* __restrict__ skeys, const u64* __restrict__ svals, long cap,
                                                             int log2_cap, float thresh, int32_t* __restrict__ pairs, long pairs_cap,
                                                             u64* count) {
  FinishedTable gtab{gkeys}, stab{skeys};
  for (long base = (long)blockIdx.x * THREADS; base < cap; base += (long)gridDim.x * THREADS) {
    const long i = base + threadIdx.x;                     // cap is a multiple of THREADS: whole waves, the ballot below is convergent
    const uint64_t key = pkeys[i];
    const uint64_t g = key >> 32, s = key & 0xffffffffu;
    bool pass = false, lost = false;
    if (key != EMPTY && g != 0 && s != 0) {
      const int64_t gi = global_find(gtab, g, log2_cap), si = global_find(stab, s, log2_cap);
      lost = gi < 0 || si < 0;                             // pt_marginals inserted both
      if (!lost) pass = pair_passes(pvals[i], gvals[gi], svals[si] >> 32, thresh);
    }
    const u64 mask = __ballot(pass);
    const u64 lost_mask = __ballot(lost);
    const int lane = threadIdx.x % WAVE;
    u64 first = 0;
    if (mask) {
      const int leader = __ffsll((long long)mask) - 1;
      if (lane == leader) first = __hip_atomic_fetch_add(count, (u64)__popcll(mask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      first = __shfl(first, leader, WAVE);
    }
    if (lost_mask && lane == 0) __hip_atomic_fetch_add(count + 1, (u64)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (pass) {
      const long at = (long)(first + (u64)__popcll(mask & ((u64(1) << lane) - 1)));
      if (at < pairs_cap) {                                // the count still says how many passed
        pairs[2 * at] = (int32_t)g;
        pairs[2 * at + 1] = (int32_t)s;
      }
    }
  }
}

static int log2_of(int64_t cap) {
  int l = 0;
  while ((int64_t(1) << l) < cap) ++l;
  return l;
}

static bool table_shape_ok(int64_t cap) { return cap >= MIN_CAP && cap <= (int64_t(1) << 40) && (cap & (cap - 1)) == 0; }

template <typename TG, typename TS>
static void launch_runs(const void* gt, const void* seg, long n, u64* bound, hipStream_t st) {
  hipLaunchKernelGGL((pt_runs_kernel<TG, TS>), dim3((unsigned)workgroups_of(n)), dim3(THREADS), 0, st, static_cast<const TG*>(gt),
                     static_cast<const TS*>(seg), n, (long)spans_per_wg(n), bound);
}

template <typename TG, typename TS>
static void launch_build(const void* gt, const void* seg, long n, u64* keys, u64* vals, int log2_cap, u64* record, hipStream_t st) {
  hipLaunchKernelGGL((pt_build_kernel<TG, TS>), dim3((unsigned)workgroups_of(n)), dim3(THREADS), 0, st, static_cast<const TG*>(gt),
                     static_cast<const TS*>(seg), n, (long)spans_per_wg(n), keys, vals, log2_cap, record);
}

// the four width combinations of the two volumes
#define PYTC_PT_DISPATCH(gt_bytes, seg_bytes, CALL)                     \
  do {                                                                  \
    if ((gt_bytes) == 4 && (seg_bytes) == 4) CALL(int32_t, int32_t);    \
    else if ((gt_bytes) == 4) CALL(int32_t, int64_t);                   \
    else if ((seg_bytes) == 4) CALL(int64_t, int32_t);                  \
    else CALL(int64_t, int64_t);                                        \
  } while (0)

static int check_volumes(const char* what, const void* gt, int gt_bytes, const void* seg, int seg_bytes, int64_t n) {
  PYTC_REQUIRE(gt && seg, "%s: gt and seg are required", what);
  PYTC_REQUIRE((gt_bytes == 4 || gt_bytes == 8) && (seg_bytes == 4 || seg_bytes == 8), "%s: ids are 4 or 8 bytes wide, got %d and %d", what,
               gt_bytes, seg_bytes);
  PYTC_REQUIRE(n >= 1 && n < ID_LIMIT, "%s: %lld voxels; a volume has 1 to 2^31 - 2", what, (long long)n);
  PYTC_REQUIRE(reinterpret_cast<uintptr_t>(gt) % 16 == 0 && reinterpret_cast<uintptr_t>(seg) % 16 == 0,
               "%s: gt and seg must be 16-byte aligned (they are read with 16-byte loads)", what);
  return PYTC_OK;
}

}  // namespace pytc

using namespace pytc;

extern "C" int64_t pytc_pair_table_lane_run(void) { return LANE_RUN; }
extern "C" int64_t pytc_pair_table_span(void) { return SPAN; }
extern "C" int64_t pytc_pair_table_lds_slots(void) { return LDS_SLOTS; }
extern "C" int64_t pytc_pair_table_record_cells(void) { return RECORD_CELLS; }
extern "C" int64_t pytc_pair_table_workgroups(int64_t voxels) { return workgroups_of(voxels); }
extern "C" int64_t pytc_pair_table_capacity(int64_t runs) { return runs < 1 || runs >= ID_LIMIT ? -1 : capacity_for(runs); }
extern "C" int64_t pytc_pair_hash(int64_t gt, int64_t seg, int log2_cap) {
  if (id_bad(gt) || id_bad(seg) || log2_cap < 1 || log2_cap > 40) return -1;
  return (int64_t)start_slot(pair_key((uint64_t)gt, (uint64_t)seg), log2_cap);
}

extern "C" int pytc_pair_table_runs(const void* gt, int gt_bytes, const void* seg, int seg_bytes, int64_t n, int64_t* bound, void* stream) {
  const char* what = "pair_table_runs";
  if (int rc = check_volumes(what, gt, gt_bytes, seg, seg_bytes, n)) return rc;
  PYTC_REQUIRE(bound && reinterpret_cast<uintptr_t>(bound) % 8 == 0, "%s: bound (two int64) is required, 8-byte aligned", what);
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(bound, 0, 16, st);
  if (e != hipSuccess) return hip_fail(e, "pair_table_runs (clear)");
  u64* b = reinterpret_cast<u64*>(bound);
#define PYTC_PT_CALL(TG, TS) launch_runs<TG, TS>(gt, seg, (long)n, b, st)
  PYTC_PT_DISPATCH(gt_bytes, seg_bytes, PYTC_PT_CALL);
#undef PYTC_PT_CALL
  PYTC_LAUNCH_CHECK("pair_table_runs");
  return PYTC_OK;
}

extern "C" int pytc_pair_table_build(const void* gt, int gt_bytes, const void* seg, int seg_bytes, int64_t n, int64_t runs, void* table,
                                     int64_t cap, int64_t* record, void* stream) {
  const char* what = "pair_table_build";
  if (int rc = check_volumes(what, gt, gt_bytes, seg, seg_bytes, n)) return rc;
  PYTC_REQUIRE(table && record && reinterpret_cast<uintptr_t>(table) % 8 == 0 && reinterpret_cast<uintptr_t>(record) % 8 == 0,
               "%s: table and record are required, 8-byte aligned", what);
  PYTC_REQUIRE(runs >= 1 && runs <= n, "%s: %lld runs in %lld voxels", what, (long long)runs, (long long)n);
  PYTC_REQUIRE(table_shape_ok(cap), "%s: capacity %lld is not a power of two from %d up", what, (long long)cap, MIN_CAP);
  PYTC_REQUIRE(cap >= 2 * runs, "%s: capacity %lld is below twice the %lld runs: the probe loop's bound would not hold", what, (long long)cap,
               (long long)runs);
  hipStream_t st = (hipStream_t)stream;
  // table: the keys of the pair, gt and seg tables (all ones = empty), then their values (zero), cap words each
  u64* keys = static_cast<u64*>(table);
  u64* vals = keys + 3 * cap;
  u64* rec = reinterpret_cast<u64*>(record);
  hipError_t e = hipMemsetAsync(keys, 0xff, (size_t)(3 * cap) * 8, st);
  if (e == hipSuccess) e = hipMemsetAsync(vals, 0, (size_t)(3 * cap) * 8, st);
  if (e == hipSuccess) e = hipMemsetAsync(rec, 0, RECORD_CELLS * 8, st);
  if (e != hipSuccess) return hip_fail(e, "pair_table_build (clear)");
  const int lc = log2_of(cap);
#define PYTC_PT_CALL(TG, TS) launch_build<TG, TS>(gt, seg, (long)n, keys, vals, lc, rec, st)
  PYTC_PT_DISPATCH(gt_bytes, seg_bytes, PYTC_PT_CALL);
#undef PYTC_PT_CALL
  PYTC_LAUNCH_CHECK("pair_table_build (build)");
  const long per_slot = cap / THREADS;
  hipLaunchKernelGGL(pt_marginals_kernel, dim3((unsigned)(per_slot < MAX_WGS ? per_slot : MAX_WGS)), dim3(THREADS), 0, st, keys, vals,
                     keys + cap, vals + cap, keys + 2 * cap, vals + 2 * cap, (long)cap, lc, rec);
  PYTC_LAUNCH_CHECK("pair_table_build (marginals)");
  hipLaunchKernelGGL(pt_sums_kernel, dim3((unsigned)(per_slot < 1024 ? per_slot : 1024)), dim3(THREADS), 0, st, keys, vals, keys + cap,
                     vals + cap, keys + 2 * cap, vals + 2 * cap, (long)cap, rec);
  PYTC_LAUNCH_CHECK("pair_table_build (sums)");
  hipLaunchKernelGGL(pt_finish_kernel, dim3(1), dim3(1), 0, st, rec);
  PYTC_LAUNCH_CHECK("pair_table_build (finish)");
  return PYTC_OK;
}

extern "C" int pytc_pair_table_matches(const void* table, int64_t cap, float thresh, int32_t* pairs, int64_t pairs_cap, int64_t* count,
                                       void* stream) {
  const char* what = "pair_table_matches";
  PYTC_REQUIRE(table && pairs && count && reinterpret_cast<uintptr_t>(table) % 8 == 0 && reinterpret_cast<uintptr_t>(count) % 8 == 0 &&
               reinterpret_cast<uintptr_t>(pairs) % 4 == 0, "%s: table, pairs and count (two int64) are required and aligned", what);
  PYTC_REQUIRE(table_shape_ok(cap), "%s: capacity %lld is not a power of two from %d up", what, (long long)cap, MIN_CAP);
  PYTC_REQUIRE(pairs_cap >= 1, "%s: room for %lld pairs", what, (long long)pairs_cap);
  PYTC_REQUIRE(thresh == thresh, "%s: the threshold is NaN", what);
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(count, 0, 16, st);
  if (e != hipSuccess) return hip_fail(e, "pair_table_matches (clear)");
  const u64* keys = static_cast<const u64*>(table);
  const u64* vals = keys + 3 * cap;
  const long per_slot = cap / THREADS;
  hipLaunchKernelGGL(pt_matches_kernel, dim3((unsigned)(per_slot < MAX_WGS ? per_slot : MAX_WGS)), dim3(THREADS), 0, st, keys, vals,
                     keys + cap, vals + cap, keys + 2 * cap, vals + 2 * cap, (long)cap, log2_of(cap), thresh, pairs, (long)pairs_cap,
                     reinterpret_cast<u64*>(count));
  PYTC_LAUNCH_CHECK("pair_table_matches");
  return PYTC_OK;
}
