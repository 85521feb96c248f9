// The reference's own random-number schedule (LJ_RNG_TILE): one pcg32 stream per 16x16 tile, init_pcg32(ty * ntx + tx, seed), consumed
// in order — pixel by pixel, row-major inside the tile, sample by sample (path_render render.cpp:80-96, vol_path_render :125-141).
// The stream position of a sample depends on how many draws every earlier sample of its tile made, so a tile is one sequential walk;
// the only parallelism is across tiles.  A walk is cut into path steps: a TileCursor holds where it is (stream state, sample, the
// pixel's running sum, the path in flight) and tile_step advances it by one step, so a kernel can stop anywhere and a later launch
// resumes bit for bit.  Compiled for gfx950 (tile.hip: k_tile, DevTracer) and by g++ for the CPU-side tests (tests/twin_tile).
//
// Tracer provides:  bool closest(f3 org, f3 dir, float tnear, float tfar, float &t, float &u, float &v, int &gprim);  void tick(int slot);
#pragma once
#include <type_traits>
#include "dvol.h"

namespace ljd {

constexpr int kTileSize = 16;   // render.cpp:75

// (DTileJob, the job of a launch: dtypes.h)

// Where the walk of one tile stands.  VOL: vol_path_render's estimators (dvol.h), else path_tracing (dshade.h).
template <bool VOL>
struct TileCursor {
    uint64_t rng;          // the tile's stream between samples (while a sample is in flight it lives in `path`)
    uint32_t k;            // the sample in flight or next: pixel-in-tile * spp + sample
    uint32_t live;         // 1: `path` holds a started sample
    f3 sum;                // the current pixel's sum of finished samples (float, in sample order)
    uint32_t _pad;
    unsigned long long samples, bounces, rays_closest, rays_shadow, steps;   // statistics (LjStats)
    typename std::conditional<VOL, VolPath, PathState>::type path;
};

template <bool VOL>
LJ_HD void tile_cursor_init(TileCursor<VOL> &c, uint32_t tile, uint64_t seed) {
    c.rng = pcg32_init(tile, seed); c.k = 0; c.live = 0; c.sum = mk3(0, 0, 0); c._pad = 0;
    c.samples = c.bounces = c.rays_closest = c.rays_shadow = c.steps = 0;
}

// the ray casts k_extend / k_mega make for a queue slot, through a closest-hit tracer: the pending shadow ray (visible = no hit in
// [eps, stfar]), then the extension ray (tnear 0 for camera rays, camera.cpp:46)
template <class Tracer>
LJ_HD void tile_trace(const DScene &sc, Tracer &tr, PathState &ps, unsigned long long &closest, unsigned long long &shadow) {
    int code = 0;
    float t = 0.0f, u = 0.0f, v = 0.0f; int g = -1;
    if (ps.stfar > 0.0f) {
        if (!tr.closest(ps.org, ps.sdir, sc.eps, ps.stfar, t, u, v, g)) code |= HIT_VIS_BIT;
        shadow++;
    }
    t = u = v = 0.0f;
    if (!(ps.flags & PF_NO_EXT)) {
        const float tnear = ((ps.flags & 0xffffu) == 2u) ? 0.0f : sc.eps;
        float ht, hu, hv; int hg;
        if (tr.closest(ps.org, ps.dir, tnear, INFINITY, ht, hu, hv, hg)) { code |= hg + 1; t = ht; u = hu; v = hv; }
        closest++;
    }
    ps.ht = t; ps.hu = u; ps.hv = v; ps.hcode = code;
}

// Camera sample of the per-tile schedule: generate_path (dshade.h) with the jitter drawn from the tile's stream.
LJ_HD void tile_generate(const DScene &sc, int x, int y, uint64_t inc, uint64_t rng, uint32_t k, PathState &ps) {
    const float jy = pcg32_real(rng, inc);   // (y first: SURVEY §0.3)
    const float jx = pcg32_real(rng, inc);
    ps.org = ld3(sc.cam.org);
    ps.dir = camera_primary_dir(sc.cam, x, y, jx, jy);
    ps.sdir = mk3(0, 0, 0); ps.stfar = 0.0f;
    ps.W = mk3(1, 1, 1); ps.rr = 1.0f; ps.p2 = -1.0f;
    ps.rad = mk3(0, 0, 0); ps.nee = mk3(0, 0, 0);
    ps.sample = k; ps.rng = rng;
    ps.eta_scale = 1.0f; ps.spread = sc.init_spread;
    ps.flags = 2u;
}

// Advances the tile's walk by one path step: path_tracing — start the sample if none is in flight, trace its rays, shade
// (shade_path_body with the deferred Russian roulette draw); vol_path_tracing — vol_path_begin or one vol_path_step.  A finished
// sample goes into the pixel's sum (a non-finite volumetric one is left out, render.cpp:138-141), and into job.samples if the pixel is
// inside the crop; the pixel's last sample writes radiance / spp to job.rgb.  Returns false once every sample of the tile is done.
template <class Ft, bool VOL, class Tracer>
LJ_HD bool tile_step(const DScene &sc, Tracer &tr, const DTileJob &job, uint32_t tile, TileCursor<VOL> &c) {
    const uint32_t ty = tile / job.ntx, tx = tile - ty * job.ntx;
    const int x0 = (int)tx * kTileSize, y0 = (int)ty * kTileSize;
    const int tw = (sc.cam.width - x0 < kTileSize) ? sc.cam.width - x0 : kTileSize;
    const int th = (sc.cam.height - y0 < kTileSize) ? sc.cam.height - y0 : kTileSize;
    const uint32_t total = (uint32_t)(tw * th) * job.spp;
    if (c.k >= total) return false;
    const uint64_t inc = pcg32_inc(tile);
    const uint32_t p = c.k / job.spp, s = c.k - p * job.spp;
    const int x = x0 + (int)(p % (uint32_t)tw), y = y0 + (int)(p / (uint32_t)tw);
    bool finished = false;
    f3 rad = mk3(0, 0, 0);
    c.steps++;
    if constexpr (!VOL) {
        PathState &ps = c.path;
        if (!c.live) { tile_generate(sc, x, y, inc, c.rng, c.k, ps); c.live = 1; }
        tile_trace(sc, tr, ps, c.rays_closest, c.rays_shadow);
        ShadeCounters cnt{};
        if (!shade_path_body<Ft, true>(sc, inc, ps, cnt)) { finished = true; rad = ps.rad; c.rng = ps.rng; }
        c.bounces += cnt.bounces;
    } else {
        VolPath &P = c.path;
        if (!c.live) {
            VolRng r; r.state = c.rng; r.inc = inc;
            if (vol_path_begin<Ft>(sc, tr, x, y, r, P, rad)) c.live = 1;
            else finished = true;   // versions 1 and 2: one-shot estimators
        } else if (!vol_path_step<Ft>(sc, tr, P, rad)) finished = true;
        if (finished) { c.rng = P.rng.state; c.bounces += c.live ? P.bounce_iterations : 0u; }
        if (!(isfinite(rad.x) && isfinite(rad.y) && isfinite(rad.z))) rad = mk3(0, 0, 0);
    }
    if (!finished) return true;
    c.live = 0;
    c.samples++;
    c.sum = c.sum + rad;
    const bool inside = x >= job.cx0 && x < job.cx1 && y >= job.cy0 && y < job.cy1;
    if (inside && job.samples) {
        float *o = job.samples + 3ull * (((uint64_t)(y - job.cy0) * (uint64_t)(job.cx1 - job.cx0) + (uint64_t)(x - job.cx0)) * job.spp + s);
        o[0] = rad.x; o[1] = rad.y; o[2] = rad.z;
    }
    if (s + 1 == job.spp) {
        if (inside && job.rgb) {
            const float n = (float)job.spp;
            float *o = job.rgb + 3ull * ((uint64_t)y * (uint64_t)sc.cam.width + (uint64_t)x);
            o[0] = c.sum.x / n; o[1] = c.sum.y / n; o[2] = c.sum.z / n;
        }
        c.sum = mk3(0, 0, 0);
    }
    c.k++;
    return c.k < total;
}

} // namespace ljd
