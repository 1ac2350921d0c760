// The host-and-device core of the label-pair table (pair_table_kernels.hip): the contingency table n[g][s] of two id volumes as an
// open-addressing hash table, and everything the launches do per thread -- the walk over a lane's run of voxels, the insert, the
// lookup, the per-slot terms of the record, the match rule.  Everything here compiles as plain C++ too, so a host program can run the
// same functions over whole volumes (tools/pair_table_host_check.cpp).
//
// TABLE.  `cap` slots, a power of two; slot i holds a 64-bit key and a 64-bit value in two arrays.  An empty key is all ones: ids are
// below 2^31 - 1, so neither gt << 32 | seg nor a single id can be that.  A key is claimed once (compare-exchange EMPTY -> key) and
// never changes again; the value is only ever added to.
//
// TERMINATION of table_add.  The caller proves cap >= 2 K before the first insert, K the number of distinct keys that will ever be
// inserted (K <= U, the run count of pt_runs).  A probe starts at the key's slot and walks on, wrapping, while the slot holds ANOTHER
// key.  Slots are never freed, so at most K - 1 < cap / 2 slots hold another key at any time, whatever the other threads do: after at
// most K - 1 steps the walk reads its own key or EMPTY.  A claim of an EMPTY slot fails only when another thread claimed the same slot
// first; it then holds our key (done) or another one (one of the K - 1, walk on).  The loop is bounded by `probes` all the same and
// returns false when it runs out, which the kernels record (cell LOST) and Python turns into an error: nothing is dropped in silence.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PYTC_PT_HD __host__ __device__ __forceinline__
#else
#define PYTC_PT_HD inline
#endif

namespace pytc {
namespace pt {

constexpr int THREADS = 256;                               // lanes of a workgroup
constexpr int LANE_RUN = 16;                               // consecutive voxels a lane reads and merges in registers
constexpr int SPAN = THREADS * LANE_RUN;                   // consecutive voxels of a workgroup's pass
constexpr int MAX_WGS = 2048;                              // workgroups of pt_runs / pt_build: each takes whole spans, one after the other
constexpr int LDS_SLOTS = 2048;                            // the workgroup's own table (16 bytes a slot)
constexpr int LDS_PROBES = 8;                              // pt_marginals: after that many foreign keys the workgroup's table counts as full
constexpr int MIN_CAP = THREADS;                           // the smallest global table: one workgroup's worth of slots
constexpr uint64_t EMPTY = ~uint64_t(0);
constexpr int64_t ID_LIMIT = 0x7fffffff;                   // ids are 0 .. 2^31 - 2
constexpr int VOI_FRAC_BITS = 27;                          // x log2 x in fixed point: x < 2^31 gives x log2 x < 2^36, the sums too

// the record pt_sums writes, int64 cells
enum Cell {
  C_N = 0,        // voxels
  C_N1,           // voxels with gt >= 1
  C_SA,           // sum over g >= 1 of A[g]^2
  C_SB,           // sum over s >= 1 of B1[s]^2
  C_SAB,          // sum over g, s >= 1 of n^2
  C_C,            // sum over g >= 1 of n[g][0]
  C_NTRUE,        // distinct gt ids >= 1
  C_NPRED,        // distinct seg ids >= 1
  C_P,            // distinct pairs
  C_UPDATES,      // updates of the global pair table by pt_build (diagnostic)
  C_XN,           // fixed point: sum over g >= 1, all s of n log2 n
  C_XA,           // fixed point: sum over g >= 1 of A[g] log2 A[g]
  C_XB,           // fixed point: sum over all s of B1[s] log2 B1[s]
  C_LOST,         // non-zero: an insert or a lookup ran out of probes (a capacity below its bound: refused before the launch)
  C_SPLIT,        // fixed point: X_A - X_N = N1 H(seg | gt)
  C_MERGE,        // fixed point: X_B - X_N = N1 H(gt | seg)
  RECORD_CELLS
};

PYTC_PT_HD uint64_t mix64(uint64_t k) {                    // the 64-bit finaliser of MurmurHash3
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdULL;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ULL;
  k ^= k >> 33;
  return k;
}

PYTC_PT_HD uint64_t pair_key(uint64_t g, uint64_t s) { return (g << 32) | s; }
PYTC_PT_HD uint64_t start_slot(uint64_t key, int log2_cap) { return mix64(key) >> (64 - log2_cap); }   // the top bits
PYTC_PT_HD uint64_t lds_slot(uint64_t key) { return mix64(key) & (LDS_SLOTS - 1); }                    // the low bits
PYTC_PT_HD bool id_bad(int64_t v) { return v < 0 || v >= ID_LIMIT; }

// geometry of pt_runs and pt_build: whole spans per workgroup, at most MAX_WGS workgroups
PYTC_PT_HD int64_t spans_of(int64_t n) { return (n + SPAN - 1) / SPAN; }
PYTC_PT_HD int64_t spans_per_wg(int64_t n) { return (spans_of(n) + MAX_WGS - 1) / MAX_WGS; }
PYTC_PT_HD int64_t workgroups_of(int64_t n) { return n < 1 ? 0 : (spans_of(n) + spans_per_wg(n) - 1) / spans_per_wg(n); }

PYTC_PT_HD int64_t capacity_for(int64_t runs) {            // the smallest power of two >= 2 runs, at least MIN_CAP
  int64_t cap = MIN_CAP;
  while (cap < 2 * runs) cap <<= 1;
  return cap;
}

// Add val to the slot of key, claiming one when the key is new.  Tab: load_key(i), claim(i, key) -> the key the slot held before
// (EMPTY: this call claimed it), add(i, val).  false: `probes` slots held other keys.
template <class Tab>
PYTC_PT_HD bool table_add(Tab& t, uint64_t key, uint64_t val, uint64_t start, uint64_t mask, uint64_t probes) {
  uint64_t slot = start & mask;
  for (uint64_t p = 0; p < probes; ++p, slot = (slot + 1) & mask) {
    uint64_t cur = t.load_key(slot);
    if (cur == EMPTY) cur = t.claim(slot, key);
    if (cur == EMPTY || cur == key) {
      t.add(slot, val);
      return true;
    }
  }
  return false;
}

// The slot of a key in a finished table (a later launch: plain loads), -1 when it is absent.
template <class Tab>
PYTC_PT_HD int64_t table_find(Tab& t, uint64_t key, uint64_t start, uint64_t mask, uint64_t probes) {
  uint64_t slot = start & mask;
  for (uint64_t p = 0; p < probes; ++p, slot = (slot + 1) & mask) {
    const uint64_t cur = t.load_key(slot);
    if (cur == key) return (int64_t)slot;
    if (cur == EMPTY) return -1;
  }
  return -1;
}

template <class Tab>
PYTC_PT_HD bool lds_add(Tab& t, uint64_t key, uint64_t val) { return table_add(t, key, val, lds_slot(key), LDS_SLOTS - 1, LDS_PROBES); }
template <class Tab>
PYTC_PT_HD bool global_add(Tab& t, uint64_t key, uint64_t val, int log2_cap) {
  return table_add(t, key, val, start_slot(key, log2_cap), (uint64_t(1) << log2_cap) - 1, uint64_t(1) << log2_cap);
}
template <class Tab>
PYTC_PT_HD int64_t global_find(Tab& t, uint64_t key, int log2_cap) {
  return table_find(t, key, start_slot(key, log2_cap), (uint64_t(1) << log2_cap) - 1, uint64_t(1) << log2_cap);
}

// pt_build's use of the workgroup's table is DIRECT-MAPPED and decided by the keys alone, so that what reaches the global table -- and
// with it the update count of the record -- does not depend on which lane came first.  A span is walked twice.  PROPOSE: every run
// offers key | CONTESTED to the slot of its key with an atomic minimum.  A slot claimed in an earlier span holds its key without that
// bit, which is below every offer, and keeps it; an unclaimed slot ends up with the smallest key offered to it.  (A barrier.)  COMMIT:
// a run whose key is the slot's adds its count there and clears the bit (every such lane stores the same value); any other run goes
// straight to the global table.  (A barrier before the next span's offers.)
constexpr uint64_t CONTESTED = uint64_t(1) << 63;          // keys are below 2^63: ids are below 2^31 - 1

template <class Lds>
struct Propose {
  Lds& lds;
  PYTC_PT_HD explicit Propose(Lds& l) : lds(l) {}
  PYTC_PT_HD void operator()(uint64_t key, uint64_t) { lds.min_key(lds_slot(key), key | CONTESTED); }
};

// Tab (LDS side): load_key, min_key(i, v), store_key(i, v), add.  Counts what reaches the global table.
template <class Lds, class Glob>
struct Commit {
  Lds& lds;
  Glob& glob;
  int log2_cap;
  int64_t updates = 0;
  bool lost = false;
  PYTC_PT_HD Commit(Lds& l, Glob& g, int lc) : lds(l), glob(g), log2_cap(lc) {}
  PYTC_PT_HD void to_global(uint64_t key, uint64_t val) {
    ++updates;
    if (!global_add(glob, key, val, log2_cap)) lost = true;
  }
  PYTC_PT_HD void operator()(uint64_t key, uint64_t val) {
    const uint64_t slot = lds_slot(key), cur = lds.load_key(slot);
    if (cur == EMPTY || (cur & ~CONTESTED) != key) return to_global(key, val);
    if (cur & CONTESTED) lds.store_key(slot, key);
    lds.add(slot, val);
  }
};

// A lane's walk: keys[0 .. n), 1 <= n <= LANE_RUN, equal neighbours merged; emit(key, count) once per run.
template <class Emit>
PYTC_PT_HD void merge_runs(const uint64_t (&keys)[LANE_RUN], int n, Emit& emit) {
  uint64_t cur = keys[0], count = 1;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int i = 1; i < LANE_RUN; ++i) {
    if (i >= n) break;
    if (keys[i] == cur) {
      ++count;
    } else {
      emit(cur, count);
      cur = keys[i];
      count = 1;
    }
  }
  emit(cur, count);
}

// pt_runs: the positions of a lane's keys that differ from their predecessor in memory order (`before`: the key in front of keys[0];
// the first voxel of the volume has none and counts).
PYTC_PT_HD int count_changes(const uint64_t (&keys)[LANE_RUN], int n, bool has_before, uint64_t before) {
  int c = (!has_before || keys[0] != before) ? 1 : 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int i = 1; i < LANE_RUN; ++i) c += (i < n && keys[i] != keys[i - 1]) ? 1 : 0;
  return c;
}

// x log2 x in fixed point with VOI_FRAC_BITS fractional bits, rounded to nearest: |error| <= 2^-(VOI_FRAC_BITS + 1) from the rounding,
// plus the error of log2 and of the product, both relative to the term.  Integer sums of these are exact in any order.
PYTC_PT_HD int64_t xlog2x_fixed(uint64_t x) {
  if (x <= 1) return 0;
  return (int64_t)llrint((double)x * log2((double)x) * (double)(int64_t(1) << VOI_FRAC_BITS));
}

// The record's terms of one occupied slot of each table.  a: RECORD_CELLS accumulators.
PYTC_PT_HD void sums_of_pair(uint64_t key, uint64_t n, uint64_t* a) {
  const uint64_t g = key >> 32, s = key & 0xffffffffu;
  a[C_P] += 1;
  if (g == 0) return;
  a[C_XN] += (uint64_t)xlog2x_fixed(n);
  if (s == 0)
    a[C_C] += n;
  else
    a[C_SAB] += n * n;
}
PYTC_PT_HD void sums_of_gt(uint64_t g, uint64_t A, uint64_t* a) {
  a[C_N] += A;
  if (g == 0) return;
  a[C_N1] += A;
  a[C_SA] += A * A;
  a[C_NTRUE] += 1;
  a[C_XA] += (uint64_t)xlog2x_fixed(A);
}
// packed = Bfull[s] << 32 | B1[s]: both are below 2^31, so neither half carries into the other
PYTC_PT_HD void sums_of_seg(uint64_t s, uint64_t packed, uint64_t* a) {
  const uint64_t B1 = packed & 0xffffffffu;
  a[C_XB] += (uint64_t)xlog2x_fixed(B1);
  if (s == 0) return;
  a[C_SB] += B1 * B1;
  a[C_NPRED] += 1;
}

// pt_marginals: what one pair adds to the table of gt ids (A) and to the table of seg ids (Bfull << 32 | B1)
PYTC_PT_HD uint64_t seg_marginal(uint64_t g, uint64_t n) { return (n << 32) | (g ? n : 0); }

// pt_matches: the reference's float32 score of a pair g, s >= 1, float64 divide then one rounding, against the float32 threshold
PYTC_PT_HD bool pair_passes(uint64_t n, uint64_t A, uint64_t Bfull, float thresh) {
  return (float)((double)n / (double)(A + Bfull - n)) >= thresh;
}

}  // namespace pt
}  // namespace pytc
