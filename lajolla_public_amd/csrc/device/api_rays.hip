// C-ABI entry points over a table of rays or probes in place of a camera: lj_radiance_rays and lj_irradiance
// (radiance_rays) and lj_probe_ray_queries, all three on the plan that rays_plan makes of the table.
#include "api_calls.h"
#include "../host/rays_call.h"

// every check (host/rays_call.h), then the plan of the table: identity list, the ray source, the table on the device
static RenderPlan rays_plan(lj_scene *scene, const LjRenderArgs *args, const LjRaysArgs *ra, int64_t n, const float *table, uint32_t kind,
                            const LjRadianceBuffers *out, bool want_out, const std::string &me) {
    if (!scene) throw LjError(LJ_ERR_INVALID_ARG, me + ": null scene");
    const lj::FlatScene &F = scene->flat;
    const lj::RaysCall call = lj::check_rays_call(me, F.integrator, F.spp, scene->dscene.n_media, F.cam_medium, scene->dscene.init_spread, args, ra, n, table, out, want_out);
    RenderPlan plan = make_rays_plan(scene, args, n);
    plan.ray_kind = kind; plan.ray_spread = call.spread; plan.ray_medium = call.medium;
    // ---- nothing was written up to here
    if (n == 0) return plan;
    lj_context *ctx = scene->ctx;
    set_device(ctx);
    ensure(ctx->ray_table, (size_t)n * 24);
    HIP_CHECK(hipMemcpyAsync(ctx->ray_table.p, table, (size_t)n * 24, hipMemcpyHostToDevice, ctx->stream));
    plan.rays_dev = (const float *)ctx->ray_table.p;
    return plan;
}

static void radiance_rays(lj_scene *scene, const LjRenderArgs *args, const LjRaysArgs *ra, int64_t n, const float *table, uint32_t kind, const LjRadianceBuffers *out, const std::string &me) {
    RenderPlan plan = rays_plan(scene, args, ra, n, table, kind, out, true, me);
    if (n == 0) { scene->stats = LjStats{}; scene->feature_stats = LjFeatureStats{}; scene->adaptive_stats = LjAdaptiveStats{}; return; }
    lj_context *ctx = scene->ctx;
    hipStream_t s = ctx->stream;
    // radiance and variance of the entries on the device, written by the resolve launches of every pass with the entry standing in for the pixel
    ensure(ctx->ray_out, (size_t)n * 24);
    float *rad_dev = out->radiance ? (float *)ctx->ray_out.p : nullptr, *var_dev = out->variance ? (float *)ctx->ray_out.p + (size_t)n * 3 : nullptr;
    if (var_dev) { plan.feat.variance = var_dev; plan.feat.want = ljd::FEAT_VARIANCE; }
    run_render(scene, plan, rad_dev, out->samples, s, timing_requested(args));
    if (rad_dev) HIP_CHECK(hipMemcpyAsync(out->radiance, rad_dev, (size_t)n * 12, hipMemcpyDeviceToHost, s));
    if (var_dev) HIP_CHECK(hipMemcpyAsync(out->variance, var_dev, (size_t)n * 12, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (kind == ljd::RAY_SOURCE_PROBES) {   // E = pi * mean of L over cosine-distributed directions: one float multiply per value
        const float pi_f = 3.14159274f, pi2_f = pi_f * pi_f;
        if (out->radiance) for (int64_t i = 0; i < n * 3; i++) out->radiance[i] = pi_f * out->radiance[i];
        if (out->variance) for (int64_t i = 0; i < n * 3; i++) out->variance[i] = pi2_f * out->variance[i];
    }
}

extern "C" {

int lj_radiance_rays(lj_scene *scene, const LjRenderArgs *args, const LjRaysArgs *rays_args, int64_t n, const LjRadianceRay *rays_host, const LjRadianceBuffers *out_host) {
    return lj::guard([&]() { radiance_rays(scene, args, rays_args, n, (const float *)rays_host, ljd::RAY_SOURCE_RAYS, out_host, "lj_radiance_rays"); });
}

int lj_irradiance(lj_scene *scene, const LjRenderArgs *args, const LjRaysArgs *rays_args, int64_t n, const LjProbe *probes_host, const LjRadianceBuffers *out_host) {
    return lj::guard([&]() { radiance_rays(scene, args, rays_args, n, (const float *)probes_host, ljd::RAY_SOURCE_PROBES, out_host, "lj_irradiance"); });
}

int lj_probe_ray_queries(lj_scene *scene, const LjRenderArgs *args, int64_t n, const LjProbe *probes_host, LjRadianceRay *rays_out_host) {
    return lj::guard([&]() {
        if (!rays_out_host) throw LjError(LJ_ERR_INVALID_ARG, "lj_probe_ray_queries: null output");
        const RenderPlan plan = rays_plan(scene, args, nullptr, n, (const float *)probes_host, ljd::RAY_SOURCE_PROBES, nullptr, false, "lj_probe_ray_queries");
        if (n > 0) run_probe_rays(scene, plan, (float *)rays_out_host, scene->ctx->stream);
    });
}

} // extern "C"
