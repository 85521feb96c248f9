// First-hit guide buffers (lj_render_features): the per-sample rule and the order of the per-pixel sums, for the device kernel
// (features.hip: k_features, k_resolve_variance) and for the host twin (tests/twin_features) — they share every line but the traversal.
//
// A sample's features come from the camera sample every path kernel starts from (camera_sample, dshade.h): the closest hit of that ray,
// passed through surfaces without a material (medium boundaries) the way dvol.h continues at an interface.
//
// Tracer provides:  bool closest(f3 org, f3 dir, float tnear, float tfar, float &t, float &u, float &v, int &gprim);   (as in dvol.h)
#pragma once
#include "dshade.h"

namespace ljd {

constexpr int kFeatureMaxCrossings = 16;   // segments of one sample: a sample whose 16th segment still ends on a medium boundary is a miss

struct FeatureSample { f3 a, n; float d, hit; };   // albedo, shading normal (world space, as build_vertex leaves it), distance to the camera, 1 on a hit; all 0 on a miss

// the camera sample of sample_id: the ray every path kernel starts that sample with (origin = the camera's, tnear = 0: camera.cpp:46)
template <bool VIEWS>
LJ_HD void feature_begin(const DScene &sc, const DPass &pass, uint32_t sample_id, f3 &cam_org, f3 &dir) {
    uint64_t rng;
    camera_sample<VIEWS>(sc, pass, sample_id, dir, rng);
    if constexpr (VIEWS) {   // (the sample's view from its id, as start_path finds it)
        const uint32_t view = view_decode(pass, pass.pixel_list[fast_div(sample_id, pass.by_spp)]).view;
        cam_org = with_view_camera(pass, view, [&](const DCamera &cam) { return ld3(cam.org); });
    } else cam_org = ld3(sc.cam.org);
}
// The end of a segment (org, dir) that hit gprim at (t, u, v).  A surface with a material: fills `o`, returns false.  A medium boundary: true,
// and (org, tnear) are the next segment's — on from the hit point, as dvol.h continues at an index-matched interface.
LJ_HD bool feature_vertex(const DScene &sc, f3 cam_org, f3 &org, f3 dir, float &tnear, float t, float u, float v, int gprim, FeatureSample &o) {
    // the vertex of this segment alone: after a crossing the texture footprint is that of the last segment
    const DVertex vx = build_vertex(sc, org, dir, t, u, v, gprim, sc.init_spread);
    if (vx.material_id < 0) { org = vx.position; tnear = sc.eps; return true; }
    const DMaterial &m = sc.materials[vx.material_id];
    // slot 0 is the material's get_texture() slot (aux_value); DisneyClearcoat's is a Real (clearcoat_gloss): white
    o.a = m.kind == 6 ? mk3(1, 1, 1) : eval_texture<FeatAll>(sc, m.tex[0], true, vx.u, vx.v, vx.uv_screen_size);
    o.n = vx.frame.n;
    o.d = length(vx.position - cam_org);
    o.hit = 1.0f;
    return false;
}
LJ_HD FeatureSample feature_miss() { FeatureSample o; o.a = mk3(0, 0, 0); o.n = mk3(0, 0, 0); o.d = 0.0f; o.hit = 0.0f; return o; }

template <bool VIEWS, class Tracer>
LJ_HD void feature_sample(const DScene &sc, const DPass &pass, uint32_t sample_id, Tracer &tr, FeatureSample &o) {
    f3 cam_org, dir;
    feature_begin<VIEWS>(sc, pass, sample_id, cam_org, dir);
    o = feature_miss();
    f3 org = cam_org;
    float tnear = 0.0f;
    for (int segment = 0; segment < kFeatureMaxCrossings; segment++) {
        float t, u, v; int gprim;
        if (!tr.closest(org, dir, tnear, INFINITY, t, u, v, gprim)) return;
        if (!feature_vertex(sc, cam_org, org, dir, tnear, t, u, v, gprim, o)) return;
    }
}

// ---- the order of the per-pixel sums.  It depends on spp alone.
// A pixel's samples are summed by a group of G lanes, G the smallest power of two >= min(spp, 64): lane l of the group adds samples
// l, l + G, l + 2G, ... in increasing order, then an xor butterfly over offsets G/2 ... 1 combines the G partial sums.  A wave holds 64 / G
// pixels, so that small sample counts keep its lanes busy; for spp >= 33 the group is the wave and the order is k_resolve's.
LJ_HD uint32_t feature_group_size(uint32_t spp) {
    const uint32_t m = spp < 64u ? spp : 64u;
    uint32_t g = 1u;
    while (g < m) g <<= 1;
    return g;
}
// lane l's partial sum of x(s) over its samples
template <class X>
LJ_HD float feature_lane_sum(uint32_t l, uint32_t G, uint32_t spp, X &&x) {
    float a = 0.0f;
    for (uint32_t s = l; s < spp; s += G) a += x(s);
    return a;
}
// ... of the squared deviations from `mean` (one fma per sample, on the device and on the host alike)
template <class X>
LJ_HD float feature_lane_sqdev(uint32_t l, uint32_t G, uint32_t spp, float mean, X &&x) {
    float a = 0.0f;
    for (uint32_t s = l; s < spp; s += G) { const float d = x(s) - mean; a = fmaf(d, d, a); }
    return a;
}
// the butterfly over a group's partial sums, as plain arithmetic (the kernels run it with __shfl_xor: every lane ends with this value)
LJ_HD float feature_butterfly(float *p, uint32_t G) {
    for (uint32_t o = G >> 1; o > 0u; o >>= 1) {
        for (uint32_t l = 0; l < G; l++) if ((l & o) == 0u) { const float s = p[l] + p[l ^ o]; p[l] = s; p[l ^ o] = s; }
    }
    return p[0];
}
// from the sums to the buffers' values
LJ_HD float feature_inv_spp(uint32_t spp) { return div_ieee(1.0f, (float)spp); }
LJ_HD float feature_depth(float sum_d, float sum_hit) { return sum_hit > 0.0f ? div_ieee(sum_d, sum_hit) : 0.0f; }
// the squared standard error of the mean from the sum of squared deviations; 0 for a single sample
LJ_HD float feature_variance(float sum_sqdev, uint32_t spp) { return spp > 1u ? div_ieee(sum_sqdev, (float)spp * (float)(spp - 1u)) : 0.0f; }

} // namespace ljd
