// TEST INFRASTRUCTURE — host build of the per-tile schedule (device/dtile.h, LJ_RNG_TILE) with g++, the companion of tests/twin/twin.cpp.
//
// The same tile_step that k_tile runs, driven here over a host closest-hit tracer, in bounded "launches" of `budget` path steps per
// tile exactly as the device driver cuts them.  Lets the CPU suite hold the schedule against the oracle's rng_mode = 1 before any GPU
// time is spent.  Built only by the test suite (lajolla_public_amd/build.py build_twin_tile), never loaded by the product.
#include "../../lajolla_public_amd/csrc/device/dtile.h"
#include "../../lajolla_public_amd/csrc/device/dtrace.h"
#include "../../lajolla_public_amd/csrc/host/flatten.h"
#include <algorithm>
#include <atomic>
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

// the Tracer interface of dvol.h / dtile.h: one closest-hit query over the BVH4
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

struct TwinTile { lj::FlatScene flat; DScene view; };

template <bool VOL>
void walk(const DScene &sc, const DTileJob &job, int budget, int n_threads, unsigned long long *stats) {
    std::vector<TileCursor<VOL>> cur(job.n_tiles);
    for (uint32_t i = 0; i < job.n_tiles; i++) tile_cursor_init(cur[i], job.tiles[i], job.seed);
    // launches of `budget` steps per tile until no tile has work left (the device driver's loop); the tiles of a launch are independent
    for (;;) {
        std::atomic<uint32_t> next{0}, alive{0};
        auto worker = [&]() {
            HostTracer tr{sc};
            for (uint32_t i; (i = next.fetch_add(1)) < job.n_tiles;) {
                bool more = true;
                for (int n = 0; (budget <= 0 || n < budget) && more; n++) more = tile_step<FeatAll, VOL>(sc, tr, job, job.tiles[i], cur[i]);
                if (more) alive++;
            }
        };
        std::vector<std::thread> th;
        for (int t = 1; t < n_threads; t++) th.emplace_back(worker);
        worker();
        for (auto &t : th) t.join();
        if (alive == 0) break;
    }
    for (auto &c : cur) { stats[0] += c.samples; stats[1] += c.bounces; stats[2] += c.rays_closest; stats[3] += c.rays_shadow; stats[4] += c.steps; }
}

} // namespace

extern "C" {

void *twin_tile_create(const LjSceneDesc *d, char *err, int err_len) {
    try {
        TwinTile *t = new TwinTile();
        t->flat = lj::flatten_scene(*d);
        t->view = t->flat.host_view();
        return t;
    } catch (const std::exception &e) {
        if (err && err_len > 0) { strncpy(err, e.what(), err_len - 1); err[err_len - 1] = 0; }
        return nullptr;
    }
}
void twin_tile_free(void *t) { delete (TwinTile *)t; }

// LJ_RNG_TILE render of the share (rank, world) over the crop window (all 0: the full frame).  rgb (w x h x 3, may be null): radiance / spp
// of the window's pixels; samples (crop_w x crop_h x spp x 3, may be null): per-sample radiance.  budget <= 0: no cut.
// stats[5]: samples traced, bounce iterations, closest rays, shadow rays, path steps.
int twin_tile_render(void *tv, int spp, int max_depth, int use_max_depth, uint64_t seed, int x0, int y0, int x1, int y1, int rank, int world,
                     int budget, int n_threads, float *rgb, float *samples, unsigned long long *stats) {
    TwinTile *t = (TwinTile *)tv;
    DScene sc = t->view;
    if (use_max_depth) sc.max_depth = max_depth;
    if (t->flat.integrator < LJ_INTEGRATOR_PATH) return -4;
    const int w = sc.cam.width, h = sc.cam.height, T = kTileSize, ntx = (w + T - 1) / T, nty = (h + T - 1) / T;
    if (!(x1 > x0 && y1 > y0)) { x0 = 0; y0 = 0; x1 = w; y1 = h; }
    if (world <= 0) world = 1;
    std::vector<uint32_t> tiles;
    for (int tt = 0; tt < ntx * nty; tt++) {
        if (tt % world != rank) continue;
        const int tx0 = (tt % ntx) * T, ty0 = (tt / ntx) * T;
        if (tx0 < x1 && tx0 + T > x0 && ty0 < y1 && ty0 + T > y0) tiles.push_back((uint32_t)tt);
    }
    DTileJob job{};
    job.tiles = tiles.data(); job.n_tiles = (uint32_t)tiles.size(); job.ntx = (uint32_t)ntx; job.spp = (uint32_t)spp;
    job.cx0 = x0; job.cy0 = y0; job.cx1 = x1; job.cy1 = y1;
    job.seed = seed ? seed : 0x853c49e6748fea9bULL; job.rgb = rgb; job.samples = samples;
    if (n_threads <= 0) n_threads = (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()));   // (a thread pool per launch: keep it small)
    for (int k = 0; k < 5; k++) stats[k] = 0;
    if (t->flat.integrator == LJ_INTEGRATOR_VOLPATH) walk<true>(sc, job, budget, n_threads, stats);
    else walk<false>(sc, job, budget, n_threads, stats);
    return 0;
}

} // extern "C"
