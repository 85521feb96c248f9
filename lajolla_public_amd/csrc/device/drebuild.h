// The build rule of lj_scene_rebuild_bvh: a linear BVH over the padded primitive boxes as they stand on the device.
//   box       the builder's padded box of a primitive (drefit.h refit_prim_box)
//   centroid  c = 0.5 ((double)lo + (double)hi), per axis; its bounds cmin, cmax over all primitives
//   code      per axis q = clamp((int64)floor((c - cmin) / (cmax - cmin) 2^B), 0, 2^B - 1), 0 on an axis of zero extent; B = 21; the three q
//             interleaved (x highest) into a 63-bit Morton code
//   order     a stable sort of (code, primitive) with the input in primitive order: equal codes keep primitive order
//   hierarchy Karras' binary radix tree ("Maximizing Parallelism in the Construction of BVHs, Octrees, and k-d Trees", HPG 2012) over the
//             sorted codes with delta(i, j) = clz(code_i ^ code_j), or 64 + clz(i ^ j) where the codes are equal — the index tie-break
//             splits a run of coincident primitives in the middle, not into a chain.  A node whose range holds at most four
//             primitives is a leaf; nothing below it is used.
//   boxes     bottom up: a leaf's box grows over its primitives in sorted order, an inner node's is its left child's box grown by the right's
//
// Plain C++ shared by rebuild.hip (one lane per primitive or node) and the host twin (tests/twin_rebuild), compiled with floating-point
// contraction off, in the manner of drefit.h: the device and g++ agree byte for byte.
#pragma once
#include "drefit.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace ljd {

constexpr int kRebuildBits = 21;       // per axis
constexpr int kRebuildLeafMax = 4;     // primitives per leaf: what a DNode8 slot addresses

// One node of the radix tree, as the kernels leave it: node i of n - 1 covers the sorted positions [first, first + count); a child
// >= 0 is a node, < 0 is the single sorted position ~child.  (The layout of LjBinaryNode, which holds the compacted tree.)
struct RebuildNode { RefitBox box; int32_t left, right, first, count; };
static_assert(sizeof(RebuildNode) == 40, "RebuildNode must be 40 bytes");

LJ_HD double rebuild_centroid(const RefitBox &b, int k) { return 0.5 * ((double)b.lo[k] + (double)b.hi[k]); }

// A double as an unsigned key of the same order (the device reduces the centroid bounds with integer atomics), and back
LJ_HD uint64_t rebuild_key(double d) { union { double d; uint64_t u; } c; c.d = d; return (c.u >> 63) ? ~c.u : (c.u | 0x8000000000000000ull); }
LJ_HD double rebuild_unkey(uint64_t k) { union { double d; uint64_t u; } c; c.u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k; return c.d; }

LJ_HD uint64_t rebuild_spread(uint64_t q) {   // bit i of a 21-bit q to bit 3 i
    q &= 0x1fffffull;
    q = (q | (q << 32)) & 0x001f00000000ffffull;
    q = (q | (q << 16)) & 0x001f0000ff0000ffull;
    q = (q | (q << 8)) & 0x100f00f00f00f00full;
    q = (q | (q << 4)) & 0x10c30c30c30c30c3ull;
    q = (q | (q << 2)) & 0x1249249249249249ull;
    return q;
}
LJ_HD uint64_t rebuild_quantise(double c, double cmin, double cmax) {
    const double extent = cmax - cmin;
    if (!(extent > 0.0)) return 0;
    const double t = floor((c - cmin) / extent * (double)(1 << kRebuildBits));
    const double top = (double)((1 << kRebuildBits) - 1);
    return (uint64_t)(long long)(t < 0.0 ? 0.0 : (t > top ? top : t));
}
LJ_HD uint64_t rebuild_code(const RefitBox &b, const double cmin[3], const double cmax[3]) {
    uint64_t code = 0;
    for (int k = 0; k < 3; k++) code = (code << 1) | rebuild_spread(rebuild_quantise(rebuild_centroid(b, k), cmin[k], cmax[k]));
    return code;   // (the shift of one axis against the next interleaves them: x ends at bits 3 i + 2)
}

// delta(i, j) over n sorted codes: the length of the common prefix, -1 for a j outside them
LJ_HD int rebuild_delta(const uint64_t *codes, long long n, long long i, long long j) {
    if (j < 0 || j >= n) return -1;
    const uint64_t x = codes[i] ^ codes[j];
    if (x) return __builtin_clzll(x);
    return 64 + __builtin_clz((uint32_t)i ^ (uint32_t)j);
}

// Node i of the n - 1 nodes over n >= 2 sorted codes: its range and its two children (node 0 is the root)
LJ_HD void rebuild_node(const uint64_t *codes, int n, int i, RebuildNode &nd) {
    const int d = rebuild_delta(codes, n, i, i + 1) - rebuild_delta(codes, n, i, i - 1) < 0 ? -1 : 1;
    const int dmin = rebuild_delta(codes, n, i, i - d);
    long long lmax = 2;
    while (rebuild_delta(codes, n, i, i + lmax * d) > dmin) lmax *= 2;
    long long l = 0;
    for (long long t = lmax / 2; t >= 1; t /= 2)
        if (rebuild_delta(codes, n, i, i + (l + t) * d) > dmin) l += t;
    const long long j = i + l * d;
    const int dnode = rebuild_delta(codes, n, i, j);
    long long s = 0, t = l;
    do {
        t = (t + 1) / 2;
        if (rebuild_delta(codes, n, i, i + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    const int split = (int)(i + s * d + (d < 0 ? -1 : 0));
    const int first = (int)(d > 0 ? i : j), last = (int)(d > 0 ? j : i);
    nd.first = first; nd.count = last - first + 1;
    nd.left = split == first ? ~split : split;
    nd.right = split + 1 == last ? ~(split + 1) : split + 1;
}

// The box of a leaf: its primitives' boxes in sorted order.  boxes: per primitive; order: sorted position -> primitive
LJ_HD void rebuild_leaf_box(const RefitBox *boxes, const int32_t *order, int first, int count, RefitBox &b) {
    refit_empty(b);
    for (int k = 0; k < count; k++) refit_grow(b, boxes[order[first + k]]);
}
// The box of child c of a node whose children's boxes are written
LJ_HD void rebuild_child_box(const RebuildNode *nodes, const RefitBox *boxes, const int32_t *order, int c, RefitBox &b) {
    if (c < 0) b = boxes[order[~c]]; else b = nodes[c].box;
}
// The box of a node from its left child's box and its right child's (a leaf: from its primitives, whatever the arguments hold)
LJ_HD void rebuild_node_box(RebuildNode &nd, const RefitBox *boxes, const int32_t *order, const RefitBox &left, const RefitBox &right) {
    if (nd.count <= kRebuildLeafMax) { rebuild_leaf_box(boxes, order, nd.first, nd.count, nd.box); return; }
    RefitBox b = left;
    refit_grow(b, right);
    nd.box = b;
}

} // namespace ljd

#if defined(__clang__)
#pragma clang fp contract(fast)
#endif
