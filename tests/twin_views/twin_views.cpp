// TEST INFRASTRUCTURE — host build of the device headers' camera-batch path (DPass::views, the VIEWS instantiations of
// device/dshade.h and device/dvol.h) with g++, as tests/twin builds the single-camera path.
//
// A batch of cameras is rendered the way lj_render_views renders it — one pixel list over a frame of n_views x h rows, one
// camera table, the VIEWS builds of generate_path / shade_path / vol_path_begin_sample that the kernels call — so that the
// bookkeeping (the decode of a list entry, the view-local pcg32 stream, the per-view origin) is checked on the CPU, sample by
// sample, against the single-camera twin and the oracle.  Built only by the test suite; the product never loads it.
#include "../../lajolla_public_amd/csrc/device/dshade.h"
#include "../../lajolla_public_amd/csrc/device/dvol.h"
#include "../../lajolla_public_amd/csrc/device/dtrace.h"
#include "../../lajolla_public_amd/csrc/host/flatten.h"
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

struct TwinViews { lj::FlatScene flat; DScene view; };

} // namespace

extern "C" {

void *twin_views_create(const LjSceneDesc *d, char *err, int err_len) {
    try {
        TwinViews *t = new TwinViews();
        t->flat = lj::flatten_scene(*d);
        t->view = t->flat.host_view();
        return t;
    } catch (const std::exception &e) {
        if (err && err_len > 0) { strncpy(err, e.what(), err_len - 1); err[err_len - 1] = 0; }
        return nullptr;
    }
}
void twin_views_free(void *t) { delete (TwinViews *)t; }

// per-sample radiance of a batch over the full film: out[v][y][x][s][3].  Returns 0, or -1 for a camera the library would refuse.
int twin_views_render_samples(void *tv, int n_views, const LjCamera *views, int spp, int max_depth, int use_max_depth, uint64_t seed, int n_threads, float *out) {
    TwinViews *t = (TwinViews *)tv;
    DScene sc = t->view;
    if (use_max_depth) sc.max_depth = max_depth;
    const uint32_t w = (uint32_t)sc.cam.width, h = (uint32_t)sc.cam.height;
    std::vector<DCamera> table((size_t)n_views);
    try {
        for (int v = 0; v < n_views; v++) { lj::check_camera(views[v]); table[v] = lj::flatten_camera(views[v]); }
    } catch (const std::exception &) { return -1; }
    for (const DCamera &c : table) if ((uint32_t)c.width != w || (uint32_t)c.height != h) return -1;
    std::vector<uint32_t> pixels;
    for (uint32_t e = 0; e < (uint32_t)n_views * w * h; e++) pixels.push_back(e);
    DPass pass{}; pass.pixel_list = pixels.data(); pass.n_pixels = (uint32_t)pixels.size(); set_pass_divisors(pass, (uint32_t)spp, w);
    set_pass_views(pass, table.data(), w, h);
    pass.seed = seed ? seed : 0x853c49e6748fea9bULL; pass.sample_rgb = out;
    const uint64_t total = (uint64_t)pixels.size() * (uint64_t)spp;
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
                if (vol_path_begin_sample<FeatAll, true>(sc, pass, tr, (uint32_t)s, P, r)) while (vol_path_step<FeatAll>(sc, tr, P, r)) {}
                if (!(std::isfinite(r.x) && std::isfinite(r.y) && std::isfinite(r.z))) r = mk3(0, 0, 0);   // (volpath_body)
            } else {
                PathState ps;
                generate_path<true>(sc, pass, (uint32_t)s, ps);
                for (int step = 0; step < 100000; step++) {
                    extend_one(sc, ps);
                    if (!shade_path<FeatAll, true>(sc, pass, ps, cnt)) break;
                }
                r = ps.rad;
            }
            out[3 * s] = r.x; out[3 * s + 1] = r.y; out[3 * s + 2] = r.z;
        }
    };
    std::vector<std::thread> th;
    for (int i = 1; i < n_threads; i++) th.emplace_back(worker, i);
    worker(0);
    for (auto &x : th) x.join();
    return 0;
}

// view_decode against the machine's division for every list entry in [e0, e1) of a batch of w x h views: the number of disagreements
long long twin_views_decode_mismatches(uint32_t w, uint32_t h, uint64_t e0, uint64_t e1) {
    DPass pass{}; set_pass_divisors(pass, 1u, w); set_pass_views(pass, nullptr, w, h);
    long long bad = 0;
    for (uint64_t e64 = e0; e64 < e1; e64++) {
        const uint32_t e = (uint32_t)e64;
        const ViewPixel vp = view_decode(pass, e);
        const uint32_t v = e / (w * h), pixel = e % (w * h);
        if (vp.view != v || vp.pixel != pixel || vp.x != (int)(pixel % w) || vp.y != (int)(pixel / w)) bad++;
    }
    return bad;
}

} // extern "C"
