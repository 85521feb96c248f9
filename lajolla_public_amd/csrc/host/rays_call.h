// The checks of lj_radiance_rays / lj_irradiance / lj_probe_ray_queries (include/lajolla_hip.h) and the values they resolve: plain host code,
// shared by the entry points (device/api_device.hip) and by the host twin of those calls (tests/twin_rays), so that a refusal is tested
// where no GPU is.  Everything here runs before the first device write.
#pragma once
#include "host_scene.h"
#include <cmath>
#include <cstdint>
#include <string>

namespace lj {

struct RaysCall { int spp; int medium; float spread; };   // samples per entry, the medium the paths start in, the spread they start with

// `table`: n entries of six floats (org, dir / position, normal); `out`: the call's buffers (null with want_out false: lj_probe_ray_queries)
inline RaysCall check_rays_call(const std::string &me, int integrator, int scene_spp, int n_media, int cam_medium, float init_spread,
                                const LjRenderArgs *a, const LjRaysArgs *ra, int64_t n, const float *table, const LjRadianceBuffers *out, bool want_out) {
    if (!table) throw LjError(LJ_ERR_INVALID_ARG, me + ": null table");
    if (want_out && !out) throw LjError(LJ_ERR_INVALID_ARG, me + ": null buffers");
    if (want_out && !out->radiance && !out->variance && !out->samples) throw LjError(LJ_ERR_INVALID_ARG, me + ": no buffer asked for");
    if (integrator < LJ_INTEGRATOR_PATH) throw LjError(LJ_ERR_UNSUPPORTED, me + ": the auxiliary integrators trace no paths (path and volpath only)");
    if (a && a->rng_mode == LJ_RNG_TILE) throw LjError(LJ_ERR_UNSUPPORTED, me + ": rng_mode must be LJ_RNG_SAMPLE (a table of rays has no tiles)");
    if (a && a->rng_mode != LJ_RNG_SAMPLE) throw LjError(LJ_ERR_UNSUPPORTED, me + ": rng_mode must be LJ_RNG_SAMPLE");
    if (n < 0 || n > ((int64_t)1 << 31)) throw LjError(LJ_ERR_INVALID_ARG, me + ": n must be in [0, 2^31]");
    RaysCall c{};
    c.spp = (a && a->spp > 0) ? a->spp : scene_spp;
    if (c.spp <= 0) throw LjError(LJ_ERR_INVALID_ARG, me + ": samples per ray must be positive");
    if (c.spp > (1 << 20)) throw LjError(LJ_ERR_INVALID_ARG, me + ": at most 2^20 samples per ray");
    if (a && (a->rank != 0 || (a->world_size != 0 && a->world_size != 1))) throw LjError(LJ_ERR_INVALID_ARG, me + ": a table of rays is not shared among ranks (rank 0 of 1)");
    if (a && (a->crop_x0 != 0 || a->crop_y0 != 0 || a->crop_x1 != 0 || a->crop_y1 != 0)) throw LjError(LJ_ERR_INVALID_ARG, me + ": a table of rays has no crop window");
    c.medium = cam_medium; c.spread = init_spread;
    if (ra) {
        if (ra->flags & ~(uint32_t)(LJ_RAYS_HAS_MEDIUM | LJ_RAYS_HAS_SPREAD)) throw LjError(LJ_ERR_INVALID_ARG, me + ": unknown flag");
        if ((ra->flags & LJ_RAYS_HAS_MEDIUM) && ra->medium_id != LJ_RAYS_CAMERA_MEDIUM) {
            if (ra->medium_id < -1 || ra->medium_id >= n_media) throw LjError(LJ_ERR_INVALID_ARG, me + ": medium_id must be in [-1, n_media)");
            c.medium = ra->medium_id;
        }
        if (ra->flags & LJ_RAYS_HAS_SPREAD) {
            if (!std::isfinite(ra->ray_spread)) throw LjError(LJ_ERR_INVALID_ARG, me + ": ray_spread is not finite");
            if (ra->ray_spread >= 0.0f) c.spread = ra->ray_spread;
        }
    }
    for (int64_t i = 0; i < n; i++) {
        const float *t = table + 6 * i;
        bool finite = true;
        for (int k = 0; k < 6; k++) finite = finite && std::isfinite(t[k]);
        if (!finite) throw LjError(LJ_ERR_INVALID_ARG, me + ": entry " + std::to_string(i) + " is not finite");
        const double len = std::sqrt((double)t[3] * t[3] + (double)t[4] * t[4] + (double)t[5] * t[5]);
        if (!(std::fabs(len - 1.0) <= 1e-4)) throw LjError(LJ_ERR_INVALID_ARG, me + ": entry " + std::to_string(i) + " has no unit direction (length " + std::to_string(len) + ")");
    }
    return c;
}

} // namespace lj
