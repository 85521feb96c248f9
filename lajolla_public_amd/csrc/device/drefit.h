// Refit of the acceleration structures after the vertices of an uploaded scene moved (lj_scene_update_geometry): the
// boxes of the BVH4 (DNode4), of the BVH8 with quantised planes (DNode8) and of a tiny scene's flat leaf table (DScanLeaf) are recomputed
// from the leaf-ordered primitives, bottom up; topology (children, slots, leaf ranges, leaf order) is read and never written.
//
// Plain C++ shared by refit.hip (one lane per node, one launch per tree level) and the host twin (tests/twin_refit), compiled with
// floating-point contraction off and with minima / maxima written as comparisons, so that the device and g++ agree bit for bit — the
// sign of a zero plane included.  The padded primitive box is the builder's (flatten.cpp calls the same functions): one definition.
#pragma once
#include "dtypes.h"
#include "dscan.h"
#include <math.h>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace ljd {

struct RefitBox { float lo[3], hi[3]; };   // an exact float box; empty: lo = +inf, hi = -inf

LJ_HD float refit_min(float a, float b) { return b < a ? b : a; }   // (std::min / std::max: the first argument on a tie, so -0 and +0 do
LJ_HD float refit_max(float a, float b) { return a < b ? b : a; }   //  not depend on which machine's fminf took them)
LJ_HD void refit_empty(RefitBox &b) { for (int k = 0; k < 3; k++) { b.lo[k] = INFINITY; b.hi[k] = -INFINITY; } }
LJ_HD void refit_grow(RefitBox &b, const RefitBox &o) { for (int k = 0; k < 3; k++) { b.lo[k] = refit_min(b.lo[k], o.lo[k]); b.hi[k] = refit_max(b.hi[k], o.hi[k]); } }

// The extent [l, h] of a primitive along axis k as the reference hands it to Embree: the float vertices' (triangle_mesh.inl:11-14), or
// sphere_bounds_func (sphere.inl:1-10): double arithmetic stored into float bounds.
LJ_HD void prim_extent(const DPrim &p, const DSphere &s, int k, float &l, float &h) {
    if (p.kind == 1) { l = (float)(s.center[k] - s.radius); h = (float)(s.center[k] + s.radius); }
    else { l = refit_min(p.v0[k], refit_min(p.v1[k], p.v2[k])); h = refit_max(p.v0[k], refit_max(p.v1[k], p.v2[k])); }
}
// The builder's padding of [l, h]: a box test may accept a box the exact ray misses, never the reverse.
LJ_HD void prim_pad(float l, float h, float &lo, float &hi) {
    const float pad = 1e-5f * (fabsf(l) + fabsf(h)) + 1e-7f * (h - l) + 1e-30f;
    lo = l - pad; hi = h + pad;
}
LJ_HD void refit_prim_box(const DPrim &p, const DSphere *spheres, RefitBox &b) {
    const DSphere &s = spheres[p.kind == 1 ? p.sphere_slot : 0];
    for (int k = 0; k < 3; k++) { float l, h; prim_extent(p, s, k, l, h); prim_pad(l, h, b.lo[k], b.hi[k]); }
}
// A leaf's box: the union of the padded boxes of its primitives [first, first + count).  (A leaf that a spatial split had clipped gets
// the whole boxes of its primitives: larger than the builder's, and correct.)
LJ_HD void refit_leaf_box(const DPrim *leaf_prims, const DSphere *spheres, int first, int count, RefitBox &b) {
    refit_empty(b);
    for (int i = 0; i < count; i++) { RefitBox pb; refit_prim_box(leaf_prims[first + i], spheres, pb); refit_grow(b, pb); }
}

// ---- BVH4: the six planes of every filled slot of node i, from the leaf's primitives or from box4[child] (written by the launch of the
// level below); box4[i] = the union.  Empty slots (lo = +inf, hi = -inf), child[] and pad[] are not touched.
LJ_HD void refit_node4(DNode4 *nodes, RefitBox *box4, const DPrim *leaf_prims, const DSphere *spheres, int i) {
    DNode4 &nd = nodes[i];
    RefitBox u; refit_empty(u);
    for (int k = 0; k < 4; k++) {
        if (!(nd.lox[k] <= nd.hix[k])) continue;
        RefitBox b;
        const int c = nd.child[k];
        if (c < 0) refit_leaf_box(leaf_prims, spheres, (~c) >> 3, ((~c) & 7) + 1, b); else b = box4[c];
        nd.lox[k] = b.lo[0]; nd.loy[k] = b.lo[1]; nd.loz[k] = b.lo[2];
        nd.hix[k] = b.hi[0]; nd.hiy[k] = b.hi[1]; nd.hiz[k] = b.hi[2];
        refit_grow(u, b);
    }
    box4[i] = u;
}

// ---- BVH8.  Grid step exponent of one axis: the smallest e >= -126 with 255 * 2^e >= extent (the builder's grid_exponent, bvh.cpp), by
// exponent arithmetic: extent = m 2^k with 1 <= m < 2 and 255 = (255 / 128) 2^7, so e = k - 7, one more when m > 255 / 128.
// A result above 127 is outside the node format: the host refuses such a scene before anything is written.
LJ_HD int refit_grid_exponent(double extent) {
    if (!(extent > 0.0)) return -126;
    union { double d; uint64_t u; } c; c.d = extent;
    const int be = (int)((c.u >> 52) & 0x7ffu);
    if (be == 0) return -126;   // (a denormal double: far below 255 * 2^-126)
    const uint64_t mant = c.u & 0xfffffffffffffull;
    const int e = be - 1023 - 7 + (mant > 0xfe00000000000ull ? 1 : 0);
    return e < -126 ? -126 : e;
}
LJ_HD double refit_pow2(int e) { union { double d; uint64_t u; } c; c.u = (uint64_t)(e + 1023) << 52; return c.d; }   // e in -1022 .. 1023

// Node i of a BVH8 stored `stride` bytes apart: grid origin = the lower corner of the children's union, one power-of-two step per axis,
// every filled slot's planes quantised in double exactly as the builder does (bvh.cpp): lower planes down, upper planes up, then the
// exact containment walk (q * step is exact in double).  imask, meta, child_base, prim_base and the slot assignment are not touched.
LJ_HD void refit_node8(unsigned char *nodes8, int stride, RefitBox *box8, const DPrim *leaf_prims, const DSphere *spheres, int i) {
    DNode8 &nd = *reinterpret_cast<DNode8 *>(nodes8 + (size_t)i * (size_t)stride);
    RefitBox cb[8], u; refit_empty(u);
    uint32_t used = 0u, rank = 0u;
    for (int s = 0; s < 8; s++) {
        if (nd.imask & (1u << s)) { cb[s] = box8[nd.child_base + rank]; rank++; }
        else if (nd.meta[s] & 0x80u) refit_leaf_box(leaf_prims, spheres, (int)(nd.prim_base + (nd.meta[s] & 31u)), (int)((nd.meta[s] >> 5) & 3u) + 1, cb[s]);
        else continue;
        used |= 1u << s;
        refit_grow(u, cb[s]);
    }
    box8[i] = u;
    if (!used) return;   // (the one node of an empty scene)
    uint8_t *qlo[3] = {nd.qlo_x, nd.qlo_y, nd.qlo_z}, *qhi[3] = {nd.qhi_x, nd.qhi_y, nd.qhi_z};
    for (int a = 0; a < 3; a++) {
        nd.p[a] = u.lo[a];
        const int e = refit_grid_exponent((double)u.hi[a] - (double)u.lo[a]);
        nd.e[a] = (uint8_t)(e + 127);
        const double step = refit_pow2(e), p = (double)u.lo[a];
        for (int s = 0; s < 8; s++) {
            if (!(used & (1u << s))) continue;
            const double clo = (double)cb[s].lo[a], chi = (double)cb[s].hi[a];
            double dlo = floor((clo - p) / step), dhi = ceil((chi - p) / step);
            dlo = dlo < 0.0 ? 0.0 : (dlo > 255.0 ? 255.0 : dlo); dhi = dhi < 0.0 ? 0.0 : (dhi > 255.0 ? 255.0 : dhi);
            int lo = (int)dlo, hi = (int)dhi;
            while (lo > 0 && p + lo * step > clo) lo--;
            while (hi < 255 && p + hi * step < chi) hi++;
            qlo[a][s] = (uint8_t)lo; qhi[a][s] = (uint8_t)hi;
        }
    }
}

// ---- leaf table of a tiny scene: record i (one of the n_scan_used leaves; the padding records are not touched) from its primitives
LJ_HD void refit_scan_leaf(DScanLeaf *leaves, const DPrim *leaf_prims, const DSphere *spheres, int i) {
    DScanLeaf &L = leaves[i];
    RefitBox b; refit_leaf_box(leaf_prims, spheres, L.first, L.count, b);
    scan_leaf_from_box(b.lo, b.hi, L.c, L.h);
}

} // namespace ljd

#if defined(__clang__)
#pragma clang fp contract(fast)
#endif
