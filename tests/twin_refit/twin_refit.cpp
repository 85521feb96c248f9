// TEST INFRASTRUCTURE — host twin of lj_scene_update_geometry: the product's flatten.cpp / bvh.cpp (flatten_update, commit_update, the level
// tables) and the refit arithmetic of device/drefit.h, compiled with g++ and run level by level as refit.hip launches it; plus traversal of
// the refitted BVH4, BVH8 and leaf table with the traversal code of device/dtrace.h.  Built only by the test suite, never loaded by the
// product, and not a fallback.
#include "../../lajolla_public_amd/csrc/device/dtrace.h"
#include "../../lajolla_public_amd/csrc/device/drefit.h"
#include "../../lajolla_public_amd/csrc/host/flatten.h"
#include <cstdio>
#include <cstring>
#include <vector>

using namespace ljd;

namespace {

struct Twin { lj::FlatScene flat; };

struct HostMem {   // (tests/twin/twin.cpp)
    const DScene &sc;
    int stack[192];
    uint32_t stack8[2 * 64];
    explicit HostMem(const DScene &s) : sc(s) {}
    DNode4 node(int i) const { return sc.nodes[i]; }
    DPrim prim(int i) const { return sc.leaf_prims[i]; }
    const DSphere &sphere(int s) const { return sc.spheres[s]; }
    void push(int sp, int v) { stack[sp] = v; }
    int pop(int sp) const { return stack[sp]; }
    const uint32_t *node8(int i) const { return reinterpret_cast<const uint32_t *>(&sc.nodes8[i]); }
    void push8(int sp, uint32_t base, uint32_t bits) { stack8[2 * sp] = base; stack8[2 * sp + 1] = bits; }
    void pop8(int sp, uint32_t &base, uint32_t &bits) const { base = stack8[2 * sp]; bits = stack8[2 * sp + 1]; }
};

// the flat leaf scan of a tiny scene: every used record's box against the ray (dscan.h scan_box, with the host's reciprocals), the
// primitives of the boxes entered through the primitive tests of dtrace.h
template <bool ANY_HIT>
bool scan_traverse(HostMem &mem, const RayF &ray, HitRec &best) {
    const DScene &sc = mem.sc;
    best.t = ray.tfar; best.u = 0.0f; best.v = 0.0f; best.gprim = -1;
    ScanRay r;
    r.ix = 1.0f / scan_clamp_dir(ray.dx); r.iy = 1.0f / scan_clamp_dir(ray.dy); r.iz = 1.0f / scan_clamp_dir(ray.dz);
    r.ox = ray.ox * r.ix; r.oy = ray.oy * r.iy; r.oz = ray.oz * r.iz;
    for (int i = 0; i < sc.n_scan_used; i++) {
        const DScanLeaf &L = sc.scan_leaves[i];
        const float b[6] = {L.c[0], L.c[1], L.c[2], L.h[0], L.h[1], L.h[2]};
        const float d = ANY_HIT ? scan_box<true>(b, r, fmaxf(ray.tnear, 0.0f), ray.tfar) : scan_box<false>(b, r, fmaxf(ray.tnear, 0.0f), INFINITY);
        if (!(d < 0.0f)) continue;
        for (int k = 0; k < L.count; k++)
            if (leaf_prim_test<ANY_HIT>(mem, ray, mem.prim(L.first + k), best)) return true;
    }
    return best.gprim >= 0;
}

// the refit as refit.hip runs it: the leaf table, then each tree level by level, deepest first
void refit_host(lj::FlatScene &F) {
    const DPrim *lp = F.leaf_prims.data(); const DSphere *sp = F.spheres.data();
    for (int i = 0; i < F.n_scan_used && !F.scan_leaves.empty(); i++) refit_scan_leaf(F.scan_leaves.data(), lp, sp, i);
    std::vector<RefitBox> box4(F.nodes.size()), box8(F.nodes8.size());
    for (size_t l = F.level4_first.size() - 1; l-- > 0;)
        for (int32_t i = F.level4_first[l]; i < F.level4_first[l + 1]; i++) refit_node4(F.nodes.data(), box4.data(), lp, sp, F.levels4[i]);
    for (size_t l = F.level8_first.size() - 1; l-- > 0;)
        for (int32_t i = F.level8_first[l]; i < F.level8_first[l + 1]; i++) refit_node8((unsigned char *)F.nodes8.data(), (int)sizeof(DNode8), box8.data(), lp, sp, F.levels8[i]);
}

template <class T> int64_t copy_out(const std::vector<T> &v, void *out, int64_t cap) {
    const int64_t n = (int64_t)(v.size() * sizeof(T));
    if (out && cap >= n && n > 0) memcpy(out, v.data(), (size_t)n);
    return n;
}

} // namespace

extern "C" {

void *refit_create(const LjSceneDesc *d, char *err, int err_len) {
    try {
        Twin *t = new Twin();
        t->flat = lj::flatten_scene(*d);
        return t;
    } catch (const std::exception &e) {
        if (err && err_len > 0) { strncpy(err, e.what(), err_len - 1); err[err_len - 1] = 0; }
        return nullptr;
    }
}
void refit_free(void *t) { delete (Twin *)t; }

// lj_scene_update_geometry on the host: 0, or the LJ_ERR_* code of a refused update (the twin is then exactly as it was)
int refit_update(void *tv, const LjSceneDesc *d, char *err, int err_len) {
    Twin *t = (Twin *)tv;
    try {
        lj::FlatScene U = lj::flatten_update(t->flat, *d);
        lj::commit_update(t->flat, std::move(U));
        refit_host(t->flat);
        return 0;
    } catch (const lj::LjError &e) {
        if (err && err_len > 0) { strncpy(err, e.what(), err_len - 1); err[err_len - 1] = 0; }
        return e.code;
    }
}

// which: 0 DNode4, 1 DNode8, 2 DScanLeaf (lj_scene_read_bvh); 3 prims, 4 spheres, 5 light_tris, 6 light_tri_cdf, 7 lights, 8 light_cdf,
// 9 leaf_prims, 10 leaf_order (int32), 11 levels4, 12 level4_first, 13 levels8, 14 level8_first.  Returns the size in bytes.
int64_t refit_read(void *tv, int which, void *out, int64_t cap) {
    const lj::FlatScene &F = ((Twin *)tv)->flat;
    switch (which) {
        case 0: return copy_out(F.nodes, out, cap);
        case 1: return copy_out(F.nodes8, out, cap);
        case 2: return copy_out(F.scan_leaves, out, cap);
        case 3: return copy_out(F.prims, out, cap);
        case 4: return copy_out(F.spheres, out, cap);
        case 5: return copy_out(F.light_tris, out, cap);
        case 6: return copy_out(F.light_tri_cdf, out, cap);
        case 7: return copy_out(F.lights, out, cap);
        case 8: return copy_out(F.light_cdf, out, cap);
        case 9: return copy_out(F.leaf_prims, out, cap);
        case 10: return copy_out(F.leaf_order, out, cap);
        case 11: return copy_out(F.levels4, out, cap);
        case 12: return copy_out(F.level4_first, out, cap);
        case 13: return copy_out(F.levels8, out, cap);
        case 14: return copy_out(F.level8_first, out, cap);
    }
    return -1;
}
// bounds_center[3], bounds_radius, shadow_epsilon, n_scan_used
void refit_bounds(void *tv, double *out) {
    const lj::FlatScene &F = ((Twin *)tv)->flat;
    for (int k = 0; k < 3; k++) out[k] = F.bounds_center[k];
    out[3] = F.bounds_radius; out[4] = F.shadow_epsilon; out[5] = (double)(F.scan_leaves.empty() ? 0 : F.n_scan_used);
}

// closest hits (hits != null) or any-hit (occ != null) through tree 0 (BVH4), 1 (BVH8) or 2 (the leaf table of a tiny scene)
int refit_trace(void *tv, int tree, int64_t n, const LjRay *rays, LjHit *hits, uint8_t *occ) {
    Twin *t = (Twin *)tv;
    const DScene sc = t->flat.host_view();
    if (tree == 2 && sc.n_scan_used == 0) return -1;
    HostMem mem(sc);
    for (int64_t i = 0; i < n; i++) {
        RayF r; r.ox = rays[i].org[0]; r.oy = rays[i].org[1]; r.oz = rays[i].org[2]; r.dx = rays[i].dir[0]; r.dy = rays[i].dir[1]; r.dz = rays[i].dir[2];
        r.tnear = rays[i].tnear; r.tfar = rays[i].tfar;
        HitRec h;
        if (hits) {
            const bool hit = tree == 0 ? traverse<false>(mem, r, h) : tree == 1 ? traverse8<false>(mem, r, h) : scan_traverse<false>(mem, r, h);
            LjHit o{0, 0, 0, -1, -1};
            if (hit) { const DPrimShade &ps = sc.prims[h.gprim]; o = LjHit{h.t, h.u, h.v, ps.shape_id, ps.prim_id}; }
            hits[i] = o;
        } else {
            occ[i] = (tree == 0 ? traverse<true>(mem, r, h) : tree == 1 ? traverse8<true>(mem, r, h) : scan_traverse<true>(mem, r, h)) ? 1 : 0;
        }
    }
    return 0;
}

// the padded box of every leaf-ordered primitive (drefit.h refit_prim_box): float[n][6], lo then hi
void refit_prim_boxes(void *tv, float *out) {
    const lj::FlatScene &F = ((Twin *)tv)->flat;
    for (size_t i = 0; i < F.leaf_prims.size(); i++) { RefitBox b; refit_prim_box(F.leaf_prims[i], F.spheres.data(), b); memcpy(out + 6 * i, &b, sizeof(b)); }
}

// the exponent routine of drefit.h and the builder's grid_exponent (bvh.cpp) on the same extents
void refit_grid_exponents(int64_t n, const double *extent, int32_t *device_style, int32_t *builder) {
    for (int64_t i = 0; i < n; i++) { device_style[i] = refit_grid_exponent(extent[i]); builder[i] = lj::grid_exponent(extent[i]); }
}

} // extern "C"
