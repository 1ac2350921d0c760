// The host-and-device core of the affinity connected components (cc_kernels.hip): the edge byte of a voxel, union-find over any
// memory that offers `load` and `atomic_min`, and the steps from a voxel to its root, its component's head and its id.  Everything here compiles as plain C++
// too, so a host program can run the same functions over a whole volume (tools/affinity_cc_host_check.cpp).
//
// Invariant of every parent array while unions run: parent[i] <= i at all times, and a value only ever decreases.  `find` therefore
// walks strictly downwards and ends without an iteration cap; `unite` lowers the larger of its two roots every round.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PYTC_CC_HD __host__ __device__ __forceinline__
#else
#define PYTC_CC_HD inline
#endif

namespace pytc {
namespace cc {

constexpr int TZ = 8, TY = 8, TX = 32;                     // the cc_local tile: TX uint32 labels = one 128-byte line
constexpr int TILE = TZ * TY * TX;
constexpr int RANK_BLOCK = 2048;                           // consecutive voxels whose roots one workgroup counts and ranks
constexpr uint32_t BACKGROUND = 0xFFFFFFFFu;               // parent of a voxel that belongs to no component; a root slot without a head yet
constexpr uint32_t TAG = 0x80000000u;                      // from cc_flatten on a root's slot holds TAG | payload (indices and ids < 2^31 - 1)
constexpr unsigned EDGE_FG = 8;                            // bits 0..2: the edge to +axis a; bit 3: foreground
constexpr unsigned EDGE_SEED = 16;                         // bit 4: a channel is hard AT the voxel: the reference's flood fill starts there
constexpr unsigned EDGE_HEAD = 32;                         // bit 5 (cc_rank): the smallest seed of its component, the voxel that orders the ids

// at[a] = hard[a][v].  other[a] = hard[a] at the second voxel the rules read: v + unit_a for edge_offset 1, v - unit_a for
// edge_offset 0, false where that voxel lies outside.  in_plus[a] / in_minus[a]: v + unit_a / v - unit_a lies inside the volume.
PYTC_CC_HD unsigned edge_byte(const bool (&at)[3], const bool (&other)[3], const bool (&in_plus)[3], const bool (&in_minus)[3],
                              int edge_offset) {
  unsigned bits = 0;
  bool fg = false;
  for (int a = 0; a < 3; ++a) {
    const bool plus = edge_offset ? other[a] : (in_plus[a] && at[a]);        // the edge v -- v + unit_a
    const bool minus = edge_offset ? (in_minus[a] && at[a]) : other[a];      // the edge v - unit_a -- v
    bits |= plus ? 1u << a : 0u;
    fg = fg || at[a] || plus || minus;
  }
  if (at[0] || at[1] || at[2]) bits |= EDGE_SEED;
  return bits | (fg ? EDGE_FG : 0u);
}

// The root of x.  A loaded parent is at most x (the invariant); the walk goes on only while it is smaller, so x falls strictly and
// the loop ends whatever the memory holds.  A stale load returns an older parent: an ancestor of x in the same set.
template <class Mem>
PYTC_CC_HD uint32_t find(Mem& m, uint32_t x) {
  for (uint32_t p = m.load(x); p < x; p = m.load(x)) x = p;
  return x;
}

// Join the sets of a and b.  The only store is atomic_min(hi, lo) with lo < hi, which keeps the invariant.  old == hi: hi was a
// root and now points to lo.  Otherwise hi had the parent old < hi already (a stale find, or another thread's union): whichever of
// old and lo is smaller is now its parent, and the other one is joined to lo in the next round.  max(a, b) falls every round.
template <class Mem>
PYTC_CC_HD void unite(Mem& m, uint32_t a, uint32_t b) {
  for (;;) {
    a = find(m, a);
    b = find(m, b);
    if (a == b) return;
    const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
    const uint32_t old = m.atomic_min(hi, lo);
    if (old == hi) return;
    a = old;
    b = lo;
  }
}

// From cc_flatten on: p = parent[v] of a foreground voxel is the index of its root, or TAG | payload where v is the root itself.
PYTC_CC_HD uint32_t root_of(uint32_t p, uint32_t v) { return (p & TAG) ? v : p; }

// The value cc_flatten leaves in a root's slot: with edge_offset 0 the root, the smallest voxel of its component, stores one of its
// own edges or has a hard channel, so it is the head; with edge_offset 1 an edge is stored at its far end and the head is voted.
PYTC_CC_HD uint32_t root_slot(uint32_t root, int edge_offset) { return edge_offset ? BACKGROUND : (TAG | root); }

// cc_vote: the candidate a seed s offers to its root's slot; the smallest one wins (atomic_min).
PYTC_CC_HD uint32_t head_candidate(uint32_t s) { return TAG | s; }

// cc_vote: a seed that an edge joins to a SMALLER seed cannot be the smallest seed of its component and keeps quiet.  The edge
// v - unit_a -- v is bit a of the byte at index v - unit_a, and that bit is set only where v really is that voxel's neighbour inside
// the volume, so no coordinates are needed.  In a dense volume almost every seed has such a neighbour: the votes that are left
// are the components' candidate heads, not every voxel of a large component on one address.
PYTC_CC_HD bool may_be_head(const uint8_t* edges, long v, const long (&unit)[3]) {
  for (int a = 0; a < 3; ++a) {
    const long n = v - unit[a];
    if (n < 0) continue;
    const unsigned nb = edges[n];
    if (((nb >> a) & 1u) && (nb & EDGE_SEED)) return false;
  }
  return true;
}

}  // namespace cc
}  // namespace pytc
