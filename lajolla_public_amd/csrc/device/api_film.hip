// C-ABI entry points for the film products of a render beyond its image: lj_render_features / _device with lj_get_feature_stats
// (render_features), and lj_render_adaptive / _device with lj_get_adaptive_stats and lj_adaptive_select_query (render_adaptive, the round
// driver on top of run_render, and the selection it shares with the query).
#include "api_calls.h"

// lj_render_features / _device: every check, then the render of api_device.hip with up to five more frames beside the image.
// `out`: host pointers (on_device false) or device pointers.
static void render_features(lj_scene *scene, const LjRenderArgs *args, int32_t n_views, const LjCamera *views, const LjFeatureBuffers *out, bool on_device, hipStream_t caller, const std::string &me) {
    if (!scene || !out) throw LjError(LJ_ERR_INVALID_ARG, me + ": null argument");
    float *const dst[6] = {out->rgb, out->albedo, out->normal, out->depth, out->alpha, out->variance};
    if (std::none_of(dst, dst + 6, [](float *p) { return p != nullptr; })) throw LjError(LJ_ERR_INVALID_ARG, me + ": no buffer asked for");
    if (n_views < 0) throw LjError(LJ_ERR_INVALID_ARG, me + ": n_views must not be negative");
    if ((n_views > 0) != (views != nullptr)) throw LjError(LJ_ERR_INVALID_ARG, me + ": n_views and views must both be given or both be left out");
    if (scene->flat.integrator < LJ_INTEGRATOR_PATH) throw LjError(LJ_ERR_UNSUPPORTED, me + ": the auxiliary integrators have no guide buffers (path and volpath only)");
    if (args && args->rng_mode == LJ_RNG_TILE) throw LjError(LJ_ERR_UNSUPPORTED, me + ": rng_mode must be LJ_RNG_SAMPLE (the per-tile schedule keeps no per-sample values)");
    const std::vector<ljd::DCamera> table = view_table(scene, n_views, views, me);   // (empty without views)
    const RenderPlan plan = n_views > 0 ? make_views_plan(scene, args, n_views) : make_plan(scene, args);
    // ---- nothing was written up to here
    render_frames(scene, plan, table, dst, on_device, caller, timing_requested(args));
}

// ---- lj_render_adaptive: a round driver on top of run_render

static ljd::AdaptiveCall adaptive_call(const LjAdaptiveArgs *args, const std::string &me) {
    const LjAdaptiveArgs a = args ? *args : LjAdaptiveArgs{};
    ljd::AdaptiveCall call{};
    static const char *const why[] = {"", "min_spp must be at least 2", "max_spp is below min_spp", "at most 2^20 samples per pixel", "at most 64 rounds", "target_error is negative or not finite"};
    const int rc = ljd::adaptive_resolve(a.min_spp, a.max_spp, a.round_spp, a.max_rounds, a.target_error, call);
    if (rc != 0) throw LjError(LJ_ERR_INVALID_ARG, me + ": " + why[rc]);
    return call;
}

// the workspace of a selection over a list of n_list entries
static void ensure_adaptive_select(lj_context *ctx, uint64_t n_list) {
    const size_t tiles = ljd::adaptive_tiles(n_list);
    ensure(ctx->ad_sel, std::max<size_t>(n_list, 1) * 4);
    ensure(ctx->ad_flags, std::max<size_t>(n_list, 1));
    ensure(ctx->ad_scan, (2 * tiles + 16) * 4);   // counts, offsets, then the total
}
// The select, scan and scatter launches over the list in ad_list; the next list goes to ad_sel, its length to the last word of ad_scan.
static uint32_t *adaptive_select(lj_context *ctx, const ljd::AdaptiveCall &call, int w, int h, uint64_t n_list, hipStream_t s) {
    const size_t tiles = ljd::adaptive_tiles(n_list);
    uint32_t *counts = (uint32_t *)ctx->ad_scan.p, *offsets = counts + tiles, *total = offsets + tiles;
    ljd::launch_adaptive_select(call, w, h, (const uint32_t *)ctx->ad_n.p, (const float *)ctx->ad_mean.p, (const float *)ctx->ad_m2.p, (const uint32_t *)ctx->ad_list.p, n_list,
                                (uint8_t *)ctx->ad_flags.p, counts, offsets, total, (uint32_t *)ctx->ad_sel.p, ctx->n_cus, adaptive_max_grid(), s);
    return total;
}

static void add_stats(LjStats &sum, const LjStats &st) {
    sum.samples += st.samples; sum.bounce_iterations += st.bounce_iterations; sum.rays_closest += st.rays_closest; sum.rays_shadow += st.rays_shadow;
    sum.wavefront_steps += st.wavefront_steps; sum.queue_bytes += st.queue_bytes; sum.render_ms += st.render_ms;
    sum.extend_ms += st.extend_ms; sum.shade_ms += st.shade_ms; sum.generate_ms += st.generate_ms; sum.resolve_ms += st.resolve_ms;
    sum.extend_launches += st.extend_launches; sum.shade_launches += st.shade_launches; sum.extend_bytes += st.extend_bytes; sum.shade_bytes += st.shade_bytes;
    sum.mega_ms += st.mega_ms; sum.mega_launches += st.mega_launches; sum.mega_bytes += st.mega_bytes; sum.path_steps += st.path_steps;
}

// Every check first; then per round: run_render of the round's list into the round frames, the merge, the selection, and one read of the
// next list's length (a wait) followed by the copy of that list into the host vector the next plan carries.
static void render_adaptive(lj_scene *scene, const LjRenderArgs *args, const LjAdaptiveArgs *aargs, const LjAdaptiveBuffers *out, bool on_device, hipStream_t caller, const std::string &me) {
    if (!scene || !out) throw LjError(LJ_ERR_INVALID_ARG, me + ": null argument");
    void *const dst[7] = {out->rgb, out->variance, out->samples, out->albedo, out->normal, out->depth, out->alpha};
    if (std::none_of(dst, dst + 7, [](void *p) { return p != nullptr; })) throw LjError(LJ_ERR_INVALID_ARG, me + ": no buffer asked for");
    if (scene->flat.integrator < LJ_INTEGRATOR_PATH) throw LjError(LJ_ERR_UNSUPPORTED, me + ": the auxiliary integrators have one deterministic value per pixel (path and volpath only)");
    if (args && args->rng_mode == LJ_RNG_TILE) throw LjError(LJ_ERR_UNSUPPORTED, me + ": rng_mode must be LJ_RNG_SAMPLE (the per-tile schedule keeps no per-sample values)");
    const ljd::AdaptiveCall call = adaptive_call(aargs, me);
    LjRenderArgs ra{};
    if (args) ra = *args; else ra.max_depth = INT32_MIN;
    ra.spp = (int32_t)call.min_spp;   // (the caller's spp is ignored)
    RenderPlan plan = make_plan(scene, &ra);
    // ---- nothing was written up to here
    lj_context *ctx = scene->ctx;
    hipStream_t s = enter_from_caller(ctx, caller, /* a given stream only, as render_frames: */ caller != nullptr);
    const int w = scene->flat.cam.width, h = scene->flat.cam.height;
    const size_t n_pix = (size_t)w * (size_t)h;
    const size_t chan[7] = {3, 3, 1, 3, 3, 1, 1};
    void *frame[7] = {};
    if (on_device) for (int k = 0; k < 7; k++) frame[k] = dst[k];
    else { stage_frames(dst, chan, 0, 3, n_pix, ctx->ad_out, frame); stage_frames(dst, chan, 3, 7, n_pix, ctx->feature_frames, frame); }
    ensure(ctx->ad_n, n_pix * 4); ensure(ctx->ad_mean, n_pix * 12); ensure(ctx->ad_m2, n_pix * 12);
    ensure(ctx->ad_rgb, n_pix * 12); ensure(ctx->ad_var, n_pix * 12);
    const uint64_t n_list0 = plan.pixels->size();
    ensure(ctx->ad_list, std::max<size_t>(n_list0, 1) * 4);
    ensure_adaptive_select(ctx, n_list0);
    HIP_CHECK(hipMemsetAsync(ctx->ad_n.p, 0, n_pix * 4, s)); HIP_CHECK(hipMemsetAsync(ctx->ad_mean.p, 0, n_pix * 12, s)); HIP_CHECK(hipMemsetAsync(ctx->ad_m2.p, 0, n_pix * 12, s));
    for (int k = 3; k < 7; k++) if (frame[k]) HIP_CHECK(hipMemsetAsync(frame[k], 0, n_pix * chan[k] * 4, s));
    if (n_list0) HIP_CHECK(hipMemcpyAsync(ctx->ad_list.p, plan.pixels->data(), n_list0 * 4, hipMemcpyHostToDevice, s));
    uint32_t *n_state = (uint32_t *)ctx->ad_n.p; float *mean = (float *)ctx->ad_mean.p, *m2 = (float *)ctx->ad_m2.p;
    float *round_rgb = (float *)ctx->ad_rgb.p, *round_var = (float *)ctx->ad_var.p;
    const uint64_t seed0 = plan.seed;
    const int max_grid = adaptive_max_grid();
    LjStats sum{};
    LjAdaptiveStats as{};
    unsigned int *h_total = (unsigned int *)ctx->stats_host + 12;   // (pinned; beyond the five statistics a k_mega pass reads back)
    RenderPlan round_plan = plan;
    for (uint32_t r = 0; r < call.max_rounds && !round_plan.pixels->empty(); r++) {
        const uint64_t n_round = round_plan.pixels->size();
        round_plan.feat = RenderPlan::Features{};
        round_plan.feat.variance = round_var; round_plan.feat.want = ljd::FEAT_VARIANCE;
        if (r == 0) {   // the guide buffers come from round 0 alone
            round_plan.feat.albedo = (float *)frame[3]; round_plan.feat.normal = (float *)frame[4]; round_plan.feat.depth = (float *)frame[5]; round_plan.feat.alpha = (float *)frame[6];
            round_plan.feat.want |= (frame[3] ? ljd::FEAT_ALBEDO : 0u) | (frame[4] ? ljd::FEAT_NORMAL : 0u) | (frame[5] ? ljd::FEAT_DEPTH : 0u) | (frame[6] ? ljd::FEAT_ALPHA : 0u);
        }
        run_render(scene, round_plan, round_rgb, nullptr, s, timing_requested(args));
        add_stats(sum, scene->stats);
        as.round_pixels[r] = n_round; as.rounds = r + 1; as.samples += n_round * (uint64_t)round_plan.spp;
        const bool last = r + 1 == call.max_rounds;
        HIP_CHECK(hipEventRecord(ctx->ev_a0, s));
        ljd::launch_adaptive_merge((const uint32_t *)(r == 0 ? ctx->ad_list.p : ctx->ad_sel.p), n_round, (uint32_t)round_plan.spp, r == 0, round_rgb, round_var, n_state, mean, m2, ctx->n_cus, max_grid, s);
        HIP_CHECK(hipEventRecord(ctx->ev_a1, s));
        uint32_t *total = last ? nullptr : adaptive_select(ctx, call, w, h, n_list0, s);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipEventRecord(ctx->ev_a2, s));
        if (total) HIP_CHECK(hipMemcpyAsync(h_total, total, 4, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));   // the round's one wait
        as.merge_ms += elapsed_ms(ctx->ev_a0, ctx->ev_a1); as.select_ms += elapsed_ms(ctx->ev_a1, ctx->ev_a2);
        if (last) break;
        if (*h_total > n_list0) throw LjError(LJ_ERR_INTERNAL, me + ": the selection returned more pixels than it was given");
        auto next = std::make_shared<std::vector<uint32_t>>((size_t)*h_total);
        if (!next->empty()) HIP_CHECK(hipMemcpy(next->data(), ctx->ad_sel.p, next->size() * 4, hipMemcpyDeviceToHost));
        // the next round's plan: the call's, with the selected list (key 0: run_render uploads it, and no later plan takes it for its own)
        round_plan.pixels = next; round_plan.pixels_key = 0;
        round_plan.spp = (int)call.round_spp;
        round_plan.seed = ljd::adaptive_seed(seed0, r + 1);
    }
    ljd::launch_adaptive_output(n_pix, n_state, mean, m2, (float *)frame[0], (float *)frame[1], (uint32_t *)frame[2], ctx->n_cus, max_grid, s);
    HIP_CHECK(hipGetLastError());
    if (!on_device) fetch_frames(dst, frame, chan, 0, 7, n_pix, s);
    leave_to_caller(ctx, caller, caller != nullptr);
    scene->stats = sum; scene->feature_stats = LjFeatureStats{}; scene->adaptive_stats = as;
}

extern "C" {

int lj_render_features(lj_scene *scene, const LjRenderArgs *args, int32_t n_views, const LjCamera *views, const LjFeatureBuffers *out_host) {
    return lj::guard([&]() { render_features(scene, args, n_views, views, out_host, false, nullptr, "lj_render_features"); });
}

int lj_render_features_device(lj_scene *scene, const LjRenderArgs *args, int32_t n_views, const LjCamera *views, const LjFeatureBuffers *out_device, void *hip_stream) {
    return lj::guard([&]() { render_features(scene, args, n_views, views, out_device, true, (hipStream_t)hip_stream, "lj_render_features_device"); });
}

int lj_get_feature_stats(const lj_scene *scene, LjFeatureStats *out) { return get_stats(scene, &lj_scene::feature_stats, out, "lj_get_feature_stats"); }

int lj_render_adaptive(lj_scene *scene, const LjRenderArgs *args, const LjAdaptiveArgs *adaptive, const LjAdaptiveBuffers *out_host) {
    return lj::guard([&]() { render_adaptive(scene, args, adaptive, out_host, false, nullptr, "lj_render_adaptive"); });
}

int lj_render_adaptive_device(lj_scene *scene, const LjRenderArgs *args, const LjAdaptiveArgs *adaptive, const LjAdaptiveBuffers *out_device, void *hip_stream) {
    return lj::guard([&]() { render_adaptive(scene, args, adaptive, out_device, true, (hipStream_t)hip_stream, "lj_render_adaptive_device"); });
}

int lj_get_adaptive_stats(const lj_scene *scene, LjAdaptiveStats *out) { return get_stats(scene, &lj_scene::adaptive_stats, out, "lj_get_adaptive_stats"); }

int lj_adaptive_select_query(lj_context *ctx, int32_t width, int32_t height, const uint32_t *n, const float *mean, const float *m2, const LjAdaptiveArgs *adaptive,
                             const uint32_t *pixel_list, int64_t n_list, uint32_t *selected_out, int64_t *n_selected) {
    return lj::guard([&]() {
        const std::string me("lj_adaptive_select_query");
        if (!ctx || !n || !mean || !m2 || !n_selected) throw LjError(LJ_ERR_INVALID_ARG, me + ": null argument");
        if (width <= 0 || height <= 0) throw LjError(LJ_ERR_INVALID_ARG, me + ": width and height must be positive");
        const uint64_t limit = 1ull << 31, n_pix = (uint64_t)width * (uint64_t)height;
        if (n_pix > limit) throw LjError(LJ_ERR_INVALID_ARG, me + ": more than 2^31 pixels");
        if (n_list < 0 || (uint64_t)n_list > limit) throw LjError(LJ_ERR_INVALID_ARG, me + ": n_list must be in [0, 2^31]");
        if (n_list > 0 && (!pixel_list || !selected_out)) throw LjError(LJ_ERR_INVALID_ARG, me + ": null list");
        for (int64_t i = 0; i < n_list; i++) if (pixel_list[i] >= n_pix) throw LjError(LJ_ERR_INVALID_ARG, me + ": a listed pixel lies outside the film");
        const ljd::AdaptiveCall call = adaptive_call(adaptive, me);
        // ---- nothing was written up to here
        *n_selected = 0;
        if (n_list == 0) return;
        set_device(ctx);
        hipStream_t s = ctx->stream;
        ensure(ctx->ad_n, n_pix * 4); ensure(ctx->ad_mean, n_pix * 12); ensure(ctx->ad_m2, n_pix * 12);
        ensure(ctx->ad_list, (size_t)n_list * 4);
        ensure_adaptive_select(ctx, (uint64_t)n_list);
        HIP_CHECK(hipMemcpyAsync(ctx->ad_n.p, n, n_pix * 4, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(ctx->ad_mean.p, mean, n_pix * 12, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(ctx->ad_m2.p, m2, n_pix * 12, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(ctx->ad_list.p, pixel_list, (size_t)n_list * 4, hipMemcpyHostToDevice, s));
        uint32_t *total = adaptive_select(ctx, call, width, height, (uint64_t)n_list, s);
        HIP_CHECK(hipGetLastError());
        unsigned int got = 0;
        HIP_CHECK(hipMemcpyAsync(&got, total, 4, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if ((int64_t)got > n_list) throw LjError(LJ_ERR_INTERNAL, me + ": the selection returned more pixels than it was given");
        if (got) HIP_CHECK(hipMemcpy(selected_out, ctx->ad_sel.p, (size_t)got * 4, hipMemcpyDeviceToHost));
        *n_selected = (int64_t)got;
    });
}

} // extern "C"
