// TEST INFRASTRUCTURE — host build of the ray source of the device headers (device/dprobe.h: lj_radiance_rays, lj_irradiance,
// lj_probe_ray_queries) with g++, as tests/twin builds the camera path.
//
// A table of rays or probes is traced the way the library traces it — the checks of host/rays_call.h, one identity list over the table,
// generate_ray_path / vol_path_begin_sample with DPass::ray_kind set, then the path and volpath bodies the camera twin drives, and the
// two per-entry reductions in the order of k_resolve and k_resolve_variance — so that the rule (streams, the two leading draws, the
// probe's ray, what a refused call leaves) is checked on the CPU, sample by sample, against the camera twin.
// Built only by the test suite; the product never loads it.
#include "../../lajolla_public_amd/csrc/device/dshade.h"
#include "../../lajolla_public_amd/csrc/device/dvol.h"
#include "../../lajolla_public_amd/csrc/device/dprobe.h"
#include "../../lajolla_public_amd/csrc/device/dfeature.h"
#include "../../lajolla_public_amd/csrc/device/dtrace.h"
#include "../../lajolla_public_amd/csrc/host/flatten.h"
#include "../../lajolla_public_amd/csrc/host/rays_call.h"
#include <cstring>
#include <thread>
#include <vector>

using namespace ljd;

namespace {

struct HostMem {
    const DScene &sc;
    int stack[192];
    explicit HostMem(const DScene &s) : sc(s) {}
    DNode4 node(int i) const { return sc.nodes[i]; }
    DPrim prim(int i) const { return sc.leaf_prims[i]; }
    const DSphere &sphere(int s) const { return sc.spheres[s]; }
    void push(int sp, int v) { stack[sp] = v; }
    int pop(int sp) const { return stack[sp]; }
};

// what k_extend does for one queue slot (tests/twin/twin.cpp extend_one)
void extend_one(const DScene &sc, PathState &ps) {
    HostMem mem(sc);
    RayF ray; ray.ox = ps.org.x; ray.oy = ps.org.y; ray.oz = ps.org.z;
    int code = 0;
    if (ps.stfar > 0.0f) {
        ray.dx = ps.sdir.x; ray.dy = ps.sdir.y; ray.dz = ps.sdir.z; ray.tnear = sc.eps; ray.tfar = ps.stfar;
        HitRec h;
        if (!traverse<true>(mem, ray, h)) code |= HIT_VIS_BIT;
    }
    float t = 0, u = 0, v = 0;
    if (!(ps.flags & PF_NO_EXT)) {
        ray.dx = ps.dir.x; ray.dy = ps.dir.y; ray.dz = ps.dir.z;
        ray.tnear = ((ps.flags & 0xffffu) == 2u) ? 0.0f : sc.eps; ray.tfar = INFINITY;
        HitRec h;
        if (traverse<false>(mem, ray, h)) { code |= (h.gprim + 1); t = h.t; u = h.u; v = h.v; }
    }
    ps.ht = t; ps.hu = u; ps.hv = v; ps.hcode = code;
}

struct HostTracer {
    const DScene &sc;
    void tick(int) {}
    bool closest(f3 org, f3 dir, float tnear, float tfar, float &t, float &u, float &v, int &gprim) {
        HostMem mem(sc);
        RayF ray; ray.ox = org.x; ray.oy = org.y; ray.oz = org.z; ray.dx = dir.x; ray.dy = dir.y; ray.dz = dir.z; ray.tnear = tnear; ray.tfar = tfar;
        HitRec h;
        if (!traverse<false>(mem, ray, h)) return false;
        t = h.t; u = h.u; v = h.v; gprim = h.gprim;
        return true;
    }
};

struct TwinRays { lj::FlatScene flat; DScene view; };

int fail(const lj::LjError &e, char *err, int err_len) {
    if (err && err_len > 0) { strncpy(err, e.what(), err_len - 1); err[err_len - 1] = 0; }
    return e.code;
}

// the pass of a whole table (the twin has no pass boundaries: a sample's value does not depend on them)
DPass table_pass(const TwinRays *t, const std::vector<uint32_t> &list, const lj::RaysCall &call, const LjRenderArgs *a, const float *table, uint32_t kind) {
    DPass pass{};
    pass.pixel_list = list.data(); pass.n_pixels = (uint32_t)list.size(); set_pass_divisors(pass, (uint32_t)call.spp, (uint32_t)t->view.cam.width);
    pass.seed = (a && a->seed) ? a->seed : 0x853c49e6748fea9bULL;
    pass.ray.table = table; pass.ray_kind = kind; pass.ray.spread = call.spread; pass.ray.medium = call.medium;
    return pass;
}

} // namespace

extern "C" {

void *twin_rays_create(const LjSceneDesc *d, char *err, int err_len) {
    try {
        TwinRays *t = new TwinRays();
        t->flat = lj::flatten_scene(*d);
        t->view = t->flat.host_view();
        return t;
    } catch (const std::exception &e) {
        if (err && err_len > 0) { strncpy(err, e.what(), err_len - 1); err[err_len - 1] = 0; }
        return nullptr;
    }
}
void twin_rays_free(void *t) { delete (TwinRays *)t; }

// lj_radiance_rays (probes == 0) / lj_irradiance (probes != 0) on the host: the library's error code, its message in `err`
int twin_rays_trace(void *tv, int probes, const LjRenderArgs *a, const LjRaysArgs *ra, int64_t n, const float *table, const LjRadianceBuffers *out, int n_threads, char *err, int err_len) {
    TwinRays *t = (TwinRays *)tv;
    lj::RaysCall call;
    try {
        call = lj::check_rays_call(probes ? "lj_irradiance" : "lj_radiance_rays", t->flat.integrator, t->flat.spp, t->view.n_media, t->flat.cam_medium, t->view.init_spread, a, ra, n, table, out, true);
    } catch (const lj::LjError &e) { return fail(e, err, err_len); }
    if (n == 0) return LJ_OK;
    DScene sc = t->view;
    if (a && a->max_depth != INT32_MIN) sc.max_depth = a->max_depth;
    std::vector<uint32_t> list((size_t)n);
    for (int64_t i = 0; i < n; i++) list[(size_t)i] = (uint32_t)i;
    const uint32_t spp = (uint32_t)call.spp;
    std::vector<float> samples((size_t)n * spp * 3);
    DPass pass = table_pass(t, list, call, a, table, probes ? RAY_SOURCE_PROBES : RAY_SOURCE_RAYS);
    pass.sample_rgb = samples.data();
    const uint64_t total = (uint64_t)n * spp;
    if (n_threads <= 0) n_threads = (int)std::thread::hardware_concurrency();
    if (n_threads <= 0) n_threads = 1;
    const bool vol = t->flat.integrator == LJ_INTEGRATOR_VOLPATH;
    auto worker = [&](int tid) {
        ShadeCounters cnt{};
        for (uint64_t s = tid; s < total; s += n_threads) {
            f3 r;
            if (vol) {   // k_volpath: begin, then step until the path ends
                HostTracer tr{sc};
                VolPath P; r = mk3(0, 0, 0);
                if (vol_path_begin_sample<FeatAll, false, true>(sc, pass, tr, (uint32_t)s, P, r)) while (vol_path_step<FeatAll>(sc, tr, P, r)) {}
                if (!(std::isfinite(r.x) && std::isfinite(r.y) && std::isfinite(r.z))) r = mk3(0, 0, 0);   // (volpath_body)
            } else {   // the refill loop of k_shade, then extend / shade until the path ends
                PathState ps;
                generate_ray_path(sc, pass, (uint32_t)s, ps);
                for (int step = 0; step < 100000; step++) {
                    extend_one(sc, ps);
                    if (!shade_path<FeatAll, false>(sc, pass, ps, cnt)) break;
                }
                r = ps.rad;
            }
            samples[3 * s] = r.x; samples[3 * s + 1] = r.y; samples[3 * s + 2] = r.z;
        }
    };
    std::vector<std::thread> th;
    for (int i = 1; i < n_threads; i++) th.emplace_back(worker, i);
    worker(0);
    for (auto &x : th) x.join();
    if (out->samples) memcpy(out->samples, samples.data(), samples.size() * sizeof(float));
    // k_resolve and k_resolve_variance: one wave per entry, lane l sums samples l, l + 64, ..., then the butterfly
    const float inv = feature_inv_spp(spp), pi_f = 3.14159274f, pi2_f = pi_f * pi_f;
    for (int64_t i = 0; i < n; i++) {
        const float *src = samples.data() + (size_t)i * spp * 3;
        for (uint32_t c = 0; c < 3u; c++) {
            auto x = [&](uint32_t s) { return src[3 * s + c]; };
            float part[64];
            for (uint32_t l = 0; l < 64u; l++) part[l] = feature_lane_sum(l, 64u, spp, x);
            const float mean = feature_butterfly(part, 64u) * inv;
            for (uint32_t l = 0; l < 64u; l++) part[l] = feature_lane_sqdev(l, 64u, spp, mean, x);
            const float var = feature_variance(feature_butterfly(part, 64u), spp);
            if (out->radiance) out->radiance[3 * i + c] = probes ? pi_f * mean : mean;
            if (out->variance) out->variance[3 * i + c] = probes ? pi2_f * var : var;
        }
    }
    return LJ_OK;
}

// lj_probe_ray_queries on the host: rays_out[i * spp + s][6]
int twin_rays_probe_rays(void *tv, const LjRenderArgs *a, int64_t n, const float *probes, float *rays_out, char *err, int err_len) {
    TwinRays *t = (TwinRays *)tv;
    lj::RaysCall call;
    try {
        if (!rays_out) throw lj::LjError(LJ_ERR_INVALID_ARG, "lj_probe_ray_queries: null output");
        call = lj::check_rays_call("lj_probe_ray_queries", t->flat.integrator, t->flat.spp, t->view.n_media, t->flat.cam_medium, t->view.init_spread, a, nullptr, n, probes, nullptr, false);
    } catch (const lj::LjError &e) { return fail(e, err, err_len); }
    std::vector<uint32_t> list((size_t)n);
    for (int64_t i = 0; i < n; i++) list[(size_t)i] = (uint32_t)i;
    const DPass pass = table_pass(t, list, call, a, probes, RAY_SOURCE_PROBES);
    for (uint64_t s = 0; s < (uint64_t)n * (uint64_t)call.spp; s++) {
        uint64_t rng, inc;
        const RayStart r = ray_source_sample(t->view, pass, (uint32_t)s, rng, inc);
        float *o = rays_out + 6 * s;
        o[0] = r.org.x; o[1] = r.org.y; o[2] = r.org.z; o[3] = r.dir.x; o[4] = r.dir.y; o[5] = r.dir.z;
    }
    return LJ_OK;
}

void twin_rays_struct_sizes(int *out) { out[0] = (int)sizeof(LjRadianceRay); out[1] = (int)sizeof(LjProbe); out[2] = (int)sizeof(LjRaysArgs); out[3] = (int)sizeof(LjRadianceBuffers); }

} // extern "C"
