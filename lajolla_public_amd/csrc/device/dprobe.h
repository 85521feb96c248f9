// Paths along given rays (lj_radiance_rays) and from surface points (lj_irradiance), DESIGN.md §3.11: the source of first vertices of a
// pass whose DPass::ray_kind is set.  Shared by the device kernels — the refill loop of k_shade (kernels.hip), vol_path_begin_sample
// (dvol.h), k_probe_rays (queries.hip) — and by the host twin (tests/twin_rays).
//
// THE RULE.  Entry e of the table, sample s of spp: the pcg32 stream e * spp + s of the pass's seed, whose first two draws u0, u1 are
// taken before anything else — the two a camera sample spends on its jitter — so that everything after the first vertex draws what the
// same stream draws after a camera sample.
//   RAY_SOURCE_RAYS    the entry is (org, dir), used as given; u0 and u1 are discarded.
//   RAY_SOURCE_PROBES  the entry is (position, normal): dir = to_world(make_frame(normal), sample_cos_hemisphere(u0, u1)), what the
//                      Lambertian's sample_bsdf composes (dshade.h), and org = position + eps * normal, one float multiply and one float
//                      add per component (contraction is off in this header, as in ddenoise.h and dadaptive.h, so that the device and g++
//                      round the origin alike; the direction goes through dmath.h / dshade.h, whose sin and cos differ between the
//                      two: the twin holds it to 2e-5, the device reproduces its own rays bit for bit).
// The path then is what path_tracing() / vol_path_tracing() make of a camera ray with that origin and direction.
#pragma once
#include "dshade.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace ljd {

struct RayStart { f3 org, dir; };

LJ_HD RayStart probe_ray(f3 position, f3 normal, float eps, float u0, float u1) {
    RayStart r;
    r.dir = to_world(make_frame(normal), sample_cos_hemisphere(u0, u1));
    r.org = mk3(position.x + eps * normal.x, position.y + eps * normal.y, position.z + eps * normal.z);
    return r;
}

// the first segment of sample `sample_id` of a rays / probes pass, and its stream after the two leading draws
LJ_HD RayStart ray_source_sample(const DScene &sc, const DPass &pass, uint32_t sample_id, uint64_t &rng, uint64_t &inc) {
    const uint32_t p = fast_div(sample_id, pass.by_spp), s = sample_id - p * pass.spp;
    const uint32_t e = pass.pixel_list[p];
    const uint64_t stream = (uint64_t)e * pass.spp + s;
    inc = pcg32_inc(stream);
    uint64_t st = pcg32_init(stream, pass.seed);
    const float u0 = pcg32_real(st, inc);
    const float u1 = pcg32_real(st, inc);
    const float *t = pass.ray.table + 6ull * e;
    RayStart r;
    if (pass.ray_kind == RAY_SOURCE_PROBES) r = probe_ray(ld3(t), ld3(t + 3), sc.eps, u0, u1);
    else { r.org = ld3(t); r.dir = ld3(t + 3); }
    rng = st;
    return r;
}

// generate_path (dshade.h) for such a pass: the path record of a camera sample with the ray's origin, direction and spread
LJ_HD void generate_ray_path(const DScene &sc, const DPass &pass, uint32_t sample_id, PathState &ps) {
    uint64_t rng, inc;
    const RayStart r = ray_source_sample(sc, pass, sample_id, rng, inc);
    start_path<false>(sc, pass, sample_id, r.dir, rng, ps);
    ps.org = r.org;
    ps.spread = pass.ray.spread;
}

} // namespace ljd

#if defined(__clang__)
#pragma clang fp contract(fast)
#endif
