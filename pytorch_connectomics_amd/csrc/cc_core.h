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

// ---- id volumes (label_cc_kernels.hip): voxels are joined iff they carry the same non-zero id and are 6-, 18- or 26-neighbours.
// The neighbourhood a voxel looks at is the 17 offsets (d0, d1, d2) with d0 in {0, 1} and d1, d2 in {-1, 0, 1}, bit
// (d0 3 + d1 + 1) 3 + d2 + 1 of a mask; bit 4 is the voxel itself.  Bits 5 .. 17 are the 13 FORWARD offsets, the ones that lead to a
// larger index: every edge of the graph is the forward offset of exactly one of its two ends.  `level` is the largest number of
// non-zero components an offset may have: 1, 2, 3 for connectivity 6, 18, 26.
constexpr int NB_SELF = 4, NB_BITS = 18;

PYTC_CC_HD int connectivity_level(int connectivity) { return connectivity == 6 ? 1 : connectivity == 18 ? 2 : connectivity == 26 ? 3 : 0; }

PYTC_CC_HD int nb_bit(int d0, int d1, int d2) { return (d0 * 3 + d1 + 1) * 3 + d2 + 1; }

PYTC_CC_HD void nb_offset(int b, int& d0, int& d1, int& d2) {
  d0 = b / 9;
  d1 = (b / 3) % 3 - 1;
  d2 = b % 3 - 1;
}

// Offset b is one a voxel has to compare its id with: a forward offset within the level, and with diagonals (level > 1) the backward
// offsets of its own plane too, which lie between the voxel and a forward diagonal neighbour.
PYTC_CC_HD bool nb_wanted(int b, int level) {
  int d0, d1, d2;
  nb_offset(b, d0, d1, d2);
  const int nz = d0 + (d1 != 0) + (d2 != 0);
  return b != NB_SELF && nz <= level && (b > NB_SELF || level > 1);
}

// same: bit b set iff the voxel at offset b lies inside and carries the id of this voxel, for every wanted b.  -> the forward edges
// this voxel has to unite.  A diagonal edge v -- w is left out when a voxel m between them (every component of its offset is that of
// w or 0) carries the id too: v -- m and m -- w have fewer non-zero components each, are edges of the same graph, and are kept or
// left out by the same rule, which ends at the face edges: those are never left out.  The components are the same; the inside of a
// solid segment unites three face edges per voxel at any connectivity.
PYTC_CC_HD uint32_t needed_edges(uint32_t same, int level) {
  uint32_t out = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int b = NB_SELF + 1; b < NB_BITS; ++b) {
    int d0, d1, d2;
    nb_offset(b, d0, d1, d2);
    const int nz = d0 + (d1 != 0) + (d2 != 0);
    uint32_t between = 0;
    for (int s = 1; s < 7; ++s) {
      const int mb = nb_bit((s & 4) ? d0 : 0, (s & 2) ? d1 : 0, (s & 1) ? d2 : 0);
      if (mb != b && mb != NB_SELF) between |= 1u << mb;
    }
    if (nz <= level && ((same >> b) & 1u) && !(same & between)) out |= 1u << b;
  }
  return out;
}

}  // namespace cc
}  // namespace pytc
