// The build rule of lj_scene_rebuild_bvh_ex with LJ_BUILD_PLOC: parallel locally-ordered clustering (Meister & Bittner,
// "Parallel Locally-Ordered Clustering for Bounding Volume Hierarchy Construction", TVCG 2018) over the padded primitive boxes in the
// Morton order of drebuild.h.
//   start     cluster p of the n initial clusters is sorted position p: the box of that primitive, id ~p, count 1
//   distance  of the clusters at positions a < b: the half area of the union box, the lower position's box grown by the higher's
//   nearest   position i of m chooses, among the positions j != i within `radius` of it, the j with the least (distance, bitlen(i ^ j), j):
//             a total order of the unordered pairs, so the least pair of a round always choose each other and every round merges at least
//             one pair.  bitlen is the radix tree's own affinity: a run of coincident boxes pairs up as (2k, 2k + 1), not into a chain.
//   merge     positions i < j that chose each other become node done + rank (rank: merging pairs at lower positions), which takes
//             position i; position j goes; everything else stays, in position order
// until one cluster is left: node n - 2, the root.  Nodes are RebuildNode records with first = 0 (the host's compact_ploc_tree assigns it).
//
// Plain C++ shared by ploc.hip and the host twin (tests/twin_ploc), compiled with floating-point contraction off, in the manner of
// drebuild.h: the device and g++ agree byte for byte.
#pragma once
#include "drebuild.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace ljd {

constexpr int kPlocRadiusDefault = 8, kPlocRadiusMax = 32;
constexpr int kPlocTail = 1024;         // at most this many clusters: the rest of the rounds run in one workgroup (k_ploc_tail)
constexpr int kPlocMaxRounds = 256;     // rounds of whole-grid launches before the host gives up

LJ_HD int ploc_bitlen(uint32_t x) { return x ? 32 - __builtin_clz(x) : 0; }

// a, b: the boxes at the lower and the higher position.  An overflowing or undefined product (boxes 1e19 wide) counts as +inf, so that
// the order stays total.
LJ_HD float ploc_distance(const RefitBox &a, const RefitBox &b, RefitBox &u) {
    u = a; refit_grow(u, b);
    float e[3];
    for (int k = 0; k < 3; k++) e[k] = u.hi[k] - u.lo[k];
    const float d = (e[0] * e[1] + e[1] * e[2]) + e[2] * e[0];
    return d <= 3.402823466e38f ? d : INFINITY;
}

// The position that position i of m chooses; box_at(j): the box at position j, for every j within `radius` of i.  m >= 2.
template <class BoxAt> LJ_HD int ploc_nearest(const BoxAt &box_at, int m, int i, int radius) {
    const int j0 = i - radius < 0 ? 0 : i - radius, j1 = i + radius > m - 1 ? m - 1 : i + radius;
    const RefitBox mine = box_at(i);
    int best = -1, best_len = 0;
    float best_d = 0.0f;
    for (int j = j0; j <= j1; j++) {
        if (j == i) continue;
        RefitBox u;
        const RefitBox other = box_at(j);
        const float d = j < i ? ploc_distance(other, mine, u) : ploc_distance(mine, other, u);
        const int len = ploc_bitlen((uint32_t)i ^ (uint32_t)j);
        if (best < 0 || d < best_d || (d == best_d && len < best_len)) { best = j; best_d = d; best_len = len; }   // (j ascends: the lower j on a full tie)
    }
    return best;
}

// What position i does in a round, from the choices nn[]: 1 it merges with nn[i] above it (and writes the node), 2 it merges with
// nn[i] below it (and goes), 0 it stays as it is
LJ_HD int ploc_role(const int32_t *nn, int i) {
    const int j = nn[i];
    if (nn[j] != i) return 0;
    return j > i ? 1 : 2;
}

// The node of the pair at positions i < j
LJ_HD void ploc_merge(const RefitBox &box_i, const RefitBox &box_j, int id_i, int id_j, int count_i, int count_j, RebuildNode &nd) {
    (void)ploc_distance(box_i, box_j, nd.box);
    nd.left = id_i; nd.right = id_j; nd.first = 0; nd.count = count_i + count_j;
}

} // namespace ljd

#if defined(__clang__)
#pragma clang fp contract(fast)
#endif
