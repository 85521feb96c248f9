// The render path behind the entry points of the api_*.hip files (api_device.hip: the plain renders; api_film.hip: features and adaptive
// rounds; api_rays.hip: tables of rays and probes): render plans (which pixels, how many samples, which cameras or rays) and run_render,
// which hands a plan to one of five drivers — render_aux, render_tiles, render_volpath, render_mega, render_wavefront — one per kernel plan.
// The drivers share the pass loop (pass_at), the end of a pass (finish_pass), the render timer (close_timer) and the workspace of the context.
//
// What every change here keeps (the kernels cannot tell one host from another, so this is all there is to keep):
//   - the order of the stream operations on every stream: kernel launches, hipMemsetAsync, hipMemcpyAsync, event records,
//     hipStreamWaitEvent and synchronisations.  The lane stagger of the wavefront driver — ev_fork, the single ev_join reused lane to
//     lane, the step-0 shade launches — is the case to watch: its overlap was measured and depends on the order of enqueue;
//   - launch shapes: grid, workgroup, LDS bytes and every kernel argument come from the same expressions;
//   - LjStats: every field is filled by the same rule in every driver, the fields a driver leaves zero included, and wavefront_steps
//     counts lane 0 only in the wavefront driver;
//   - error texts and codes;
//   - the workspace grows exactly when it has to: a render that fits the buffers the context holds allocates nothing;
//   - a render without a features request (RenderPlan::feat.want == 0: every entry point but lj_render_features*) enqueues nothing of
//     finish_pass's features hook, records none of its events and touches no buffer for it.
#include "api_internal.h"

namespace {

ljd::DQueue carve_queue(void *base, uint32_t cap) {
    // one allocation, eight arrays of 16-byte records; hipMalloc returns 256-byte aligned memory and cap is a
    // multiple of 64, so every array starts on a 1 KiB boundary (one full wave instruction)
    ljd::DQueue q{};
    ljd::Rec4 *p = (ljd::Rec4 *)base;
    auto take = [&]() { ljd::Rec4 *r = p; p += cap; return r; };
    q.ro = take(); q.rd = take(); q.rs = take(); q.rh = take(); q.rw = take(); q.rl = take(); q.rn = take(); q.rg = take();
    return q;
}
// the records from slot `o` on (a lane's part of the queue)
ljd::DQueue queue_at(ljd::DQueue q, size_t o) {
    for (ljd::Rec4 **r : {&q.ro, &q.rd, &q.rs, &q.rh, &q.rw, &q.rl, &q.rn, &q.rg}) *r += o;
    return q;
}

// a set of queue records for `cap` slots (a multiple of 64, as every capacity is)
void ensure_queue(DevBuf &mem, uint32_t &capacity, uint32_t cap) {
    if (capacity >= cap) return;
    mem.alloc((size_t)cap * kQueueSlotBytes);
    capacity = cap;
}

// the plan's pixel list on the device; the copy is skipped when the context still holds this very list
void upload_pixel_list(lj_context *ctx, const RenderPlan &plan, hipStream_t stream) {
    const size_t n = plan.pixels->size();
    if (ctx->pixel_list.bytes < n * 4) { ctx->pixel_list.alloc(n * 4); ctx->pixel_list_key = 0; }
    if (ctx->pixel_list_key == plan.pixels_key && plan.pixels_key != 0) return;
    HIP_CHECK(hipMemcpyAsync(ctx->pixel_list.p, plan.pixels->data(), n * 4, hipMemcpyHostToDevice, stream));
    ctx->pixel_list_key = plan.pixels_key;
}

// ---- passes: a render walks the pixel list in runs of pix_per_pass pixels, every sample of a pixel in the same pass

ljd::DPass make_pass(const lj_scene *sc, const RenderPlan &plan, uint64_t p0, uint64_t np) {   // pixels [p0, p0 + np) of the list
    ljd::DPass pass{};
    pass.pixel_list = (const uint32_t *)sc->ctx->pixel_list.p + p0; pass.n_pixels = (uint32_t)np; ljd::set_pass_divisors(pass, (uint32_t)plan.spp, (uint32_t)sc->flat.cam.width);
    pass.seed = plan.seed; pass.sample_rgb = (float *)sc->ctx->sample_rgb.p;
    if (plan.n_views > 0) ljd::set_pass_views(pass, plan.views_dev, (uint32_t)sc->flat.cam.width, (uint32_t)sc->flat.cam.height);
    if (plan.ray_kind != ljd::RAY_SOURCE_NONE) {   // (never with views: the ray source shares by_height's bytes, dtypes.h)
        pass.ray.table = plan.rays_dev; pass.ray_kind = plan.ray_kind; pass.ray.spread = plan.ray_spread; pass.ray.medium = plan.ray_medium;
    }
    return pass;
}

struct Pass { uint64_t p0, np, total; ljd::DPass d; };   // the pixels [p0, p0 + np) of the list, their `total` samples, the kernels' view of them

Pass pass_at(const lj_scene *sc, const RenderPlan &plan, uint64_t p0, uint64_t pix_per_pass) {
    const uint64_t np = std::min<uint64_t>(pix_per_pass, plan.pixels->size() - p0);
    return Pass{p0, np, np * (uint64_t)plan.spp, make_pass(sc, plan, p0, np)};
}

// list entries per pass: the per-sample radiance buffer stays <= ~1.5 GiB and sample ids stay in 32 bits
// (LJ_TUNE_PASS_SAMPLES, a developer knob: small passes, so that a test can put a pass boundary anywhere — inside a view of a batch, say — at a small size)
uint64_t pixels_per_pass(const RenderPlan &plan) {
    const uint64_t max_samples_pass = (uint64_t)std::min(1 << 27, std::max(64, env_int("LJ_TUNE_PASS_SAMPLES", 1 << 27)));
    return std::min<uint64_t>(std::max<uint64_t>(1, max_samples_pass / (uint64_t)plan.spp), plan.pixels->size());
}

// room for the per-sample radiance of the largest pass
void ensure_sample_rgb(lj_context *ctx, const RenderPlan &plan, uint64_t pix_per_pass) { ensure(ctx->sample_rgb, pix_per_pass * (uint64_t)plan.spp * 12); }

// The end of a pass on the render stream: its samples resolved into the frame and copied to the host at the pass's place in the list.
// stats_dev (k_mega): five 64-bit statistics, read into ctx->stats_host by the same wait.  Without either host copy nothing waits.
// A features request (plan.feat.want, lj_render_features) adds, after the resolve and while sample_rgb still holds the pass: the variance
// of the pass's samples and the guide buffers of its pixels, between events of their own; then it waits for them, so that the events can
// serve the next pass.  Without a request nothing here is enqueued that was not before.
void finish_pass(lj_scene *sc, const RenderPlan &plan, const Pass &P, float *rgb_dev, float *samples_host, const void *stats_dev, hipStream_t stream) {
    lj_context *ctx = sc->ctx;
    if (rgb_dev) ljd::launch_resolve(P.d, (uint32_t)P.np, rgb_dev, stream);
    if (plan.feat.want) {
        const RenderPlan::Features &f = plan.feat;
        LjFeatureStats &fs = sc->feature_stats;
        HIP_CHECK(hipEventRecord(ctx->ev_f0, stream));
        if (f.want & ljd::FEAT_VARIANCE) ljd::launch_resolve_variance(P.d, (uint32_t)P.np, f.variance, stream);
        HIP_CHECK(hipEventRecord(ctx->ev_f1, stream));
        if (f.want & ljd::FEAT_FIRST_HIT) {
            const int grid = ljd::features_grid(P.np, (uint32_t)plan.spp, ctx->n_cus);
            // (run_render made room for the largest pass before the driver carved its own stacks from the buffer: it must not move now)
            if (sc->ecfg.spill_levels > 0 && ctx->spill.bytes < (size_t)sc->ecfg.spill_levels * (size_t)grid * 256 * sizeof(int))
                throw LjError(LJ_ERR_INTERNAL, "the overflow stacks do not hold a features launch");
            ljd::launch_features(sc->dscene, P.d, (uint32_t)P.np, f.want, f.albedo, f.normal, f.depth, f.alpha, sc->ecfg, sc->ecfg.spill_levels > 0 ? (int *)ctx->spill.p : nullptr, grid, stream);
            fs.feature_rays += P.total; fs.feature_launches++;
        }
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipEventRecord(ctx->ev_f2, stream));
        HIP_CHECK(hipEventSynchronize(ctx->ev_f2));
        fs.variance_ms += elapsed_ms(ctx->ev_f0, ctx->ev_f1); fs.features_ms += elapsed_ms(ctx->ev_f1, ctx->ev_f2);
    }
    if (stats_dev) HIP_CHECK(hipMemcpyAsync(ctx->stats_host, stats_dev, 5 * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    if (samples_host) HIP_CHECK(hipMemcpyAsync(samples_host + P.p0 * (uint64_t)plan.spp * 3, ctx->sample_rgb.p, P.total * 12, hipMemcpyDeviceToHost, stream));
    if (stats_dev || samples_host) HIP_CHECK(hipStreamSynchronize(stream));
}

// ---- auxiliary buffers: one primary ray per pixel, no queue

void render_aux(lj_scene *sc, const RenderPlan &plan, float *rgb_dev, float *samples_host, hipStream_t stream) {
    lj_context *ctx = sc->ctx;
    LjStats &st = sc->stats;
    const uint64_t n_pix = plan.pixels->size();
    if (samples_host) throw LjError(LJ_ERR_UNSUPPORTED, "the auxiliary integrators have one deterministic value per pixel, no per-sample values");
    upload_pixel_list(ctx, plan, stream);
    HIP_CHECK(hipEventRecord(ctx->ev_begin, stream));
    const int grid = (int)std::min<uint64_t>((n_pix + 255) / 256, (uint64_t)ctx->n_cus * 4);
    ljd::launch_aux(sc->dscene, make_pass(sc, plan, 0, n_pix), (uint32_t)n_pix, sc->flat.integrator, rgb_dev, sc->ecfg,
                    ensure_spill(ctx, sc->ecfg.spill_levels, (uint32_t)grid), grid, stream);
    HIP_CHECK(hipGetLastError());
    st.render_ms = close_timer(ctx, stream); st.samples = n_pix; st.rays_closest = n_pix;
}

// The per-tile schedule (LJ_RNG_TILE, dtile.h / tile.hip) for path and volpath: every tile of the share that touches the crop window is
// walked whole — its stream is consumed for the pixels outside the window too — and only the window's pixels are written (rgb_dev:
// radiance / spp; samples_host: per-sample radiance in lj_render_samples layout).  Bounded launches: each advances every unfinished tile
// by at most LJ_TUNE_TILE_STEPS path steps; the cursors stay in HBM between launches.  LjStats.samples counts every sample traced,
// those outside the window included.
void render_tiles(lj_scene *sc, const ljd::DScene &ds, const RenderPlan &plan, float *rgb_dev, float *samples_host, hipStream_t stream) {
    lj_context *ctx = sc->ctx;
    LjStats &st = sc->stats;
    const bool vol = sc->flat.integrator == LJ_INTEGRATOR_VOLPATH;
    const int w = sc->flat.cam.width, h = sc->flat.cam.height, T = 16;   // render.cpp:75
    const int ntx = (w + T - 1) / T, nty = (h + T - 1) / T;
    std::vector<uint32_t> tiles;
    for (int t = 0; t < ntx * nty; t++) {
        if (t % plan.world != plan.rank) continue;
        const int x0 = (t % ntx) * T, y0 = (t / ntx) * T;
        if (x0 < plan.cx1 && x0 + T > plan.cx0 && y0 < plan.cy1 && y0 + T > plan.cy0) tiles.push_back((uint32_t)t);
    }
    if (tiles.empty()) return;
    const uint32_t n_tiles = (uint32_t)tiles.size();
    // tiles per wave (1..64): 1 spreads the tiles over the SIMDs one by one, 64 packs them into full waves
    const uint32_t lanes = (uint32_t)std::min(64, std::max(1, env_int("LJ_TUNE_TILE_LANES", 1)));
    const uint32_t budget = (uint32_t)std::max(1, env_int("LJ_TUNE_TILE_STEPS", 512));   // path steps per tile and launch
    const size_t cur_bytes = ljd::tile_cursor_bytes(vol) * n_tiles;
    ensure(ctx->tile_cursors, cur_bytes);
    ensure(ctx->tile_list, (size_t)n_tiles * 4 + 64);
    const uint64_t n_samples_out = samples_host ? (uint64_t)(plan.cx1 - plan.cx0) * (uint64_t)(plan.cy1 - plan.cy0) * (uint64_t)plan.spp : 0;
    if (samples_host) ensure(ctx->tile_samples, n_samples_out * 12);
    uint32_t *tile_ids = (uint32_t *)ctx->tile_list.p, *alive = tile_ids + ((n_tiles + 15u) & ~15u);   // (the alive counter after the list)
    HIP_CHECK(hipMemcpyAsync(tile_ids, tiles.data(), (size_t)n_tiles * 4, hipMemcpyHostToDevice, stream));
    ljd::DTileJob job{};
    job.tiles = tile_ids; job.n_tiles = n_tiles; job.ntx = (uint32_t)ntx; job.spp = (uint32_t)plan.spp;
    job.cx0 = plan.cx0; job.cy0 = plan.cy0; job.cx1 = plan.cx1; job.cy1 = plan.cy1;
    job.seed = plan.seed; job.rgb = rgb_dev; job.samples = samples_host ? (float *)ctx->tile_samples.p : nullptr;
    int *spill = ensure_spill(ctx, sc->ecfg.spill_levels, (uint32_t)ljd::tile_grid(n_tiles, lanes));
    HIP_CHECK(hipEventRecord(ctx->ev_begin, stream));
    ljd::launch_tile_init(vol, ctx->tile_cursors.p, tile_ids, n_tiles, plan.seed, stream);
    HIP_CHECK(hipGetLastError());
    unsigned int *h_alive = (unsigned int *)ctx->stats_host;
    uint64_t launches = 0;
    for (;;) {
        HIP_CHECK(hipMemsetAsync(alive, 0, 4, stream));
        ljd::launch_tile(vol, ds, job, ctx->tile_cursors.p, lanes, budget, alive, sc->ecfg, spill, stream);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(h_alive, alive, 4, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        launches++;
        if (*h_alive == 0) break;
        if (launches >= (1u << 24)) throw LjError(LJ_ERR_INTERNAL, "tile walk did not finish");
    }
    st.render_ms = close_timer(ctx, stream);
    std::vector<unsigned char> cur_host(cur_bytes);
    HIP_CHECK(hipMemcpy(cur_host.data(), ctx->tile_cursors.p, cur_bytes, hipMemcpyDeviceToHost));
    if (samples_host) HIP_CHECK(hipMemcpy(samples_host, ctx->tile_samples.p, n_samples_out * 12, hipMemcpyDeviceToHost));
    unsigned long long c[5];
    ljd::tile_cursor_stats(vol, cur_host.data(), n_tiles, c);
    st.samples = c[0]; st.bounce_iterations = c[1]; st.rays_closest = c[2]; st.rays_shadow = c[3]; st.path_steps = c[4];
    st.wavefront_steps = launches;
}

// ---- volumetric path tracer: one lane per sample, whole path (dvol.h)

void render_volpath(lj_scene *sc, const ljd::DScene &ds, const RenderPlan &plan, uint64_t pix_per_pass, float *rgb_dev, float *samples_host, hipStream_t stream) {
    lj_context *ctx = sc->ctx;
    LjStats &st = sc->stats;
    ensure_sample_rgb(ctx, plan, pix_per_pass);
    if (!ctx->chunk_counter.p) ctx->chunk_counter.alloc(128 * kMaxLanes);
    upload_pixel_list(ctx, plan, stream);
    HIP_CHECK(hipMemsetAsync(ctx->chunk_counter.p, 0, 256, stream));
    HIP_CHECK(hipEventRecord(ctx->ev_begin, stream));
    for (uint64_t p0 = 0; p0 < plan.pixels->size(); p0 += pix_per_pass) {
        const Pass P = pass_at(sc, plan, p0, pix_per_pass);
        // persistent grid (k_volpath regenerates paths): as many workgroups as stay resident, fewer for a small pass
        const int grid = (int)std::max<uint64_t>(1, std::min<uint64_t>((P.total + 255) / 256, (uint64_t)ctx->n_cus * (uint64_t)ljd::volpath_blocks_per_cu(ds)));
        HIP_CHECK(hipMemsetAsync((char *)ctx->chunk_counter.p + 8, 0, 4, stream));   // the launch's sample counter
        ljd::launch_volpath(ds, P.d, (uint32_t)P.total, (uint32_t *)ctx->chunk_counter.p, sc->ecfg, sc->scfg.variant,
                            /* plain: */ (sc->feat_kinds & ~7u) == 0u && !sc->feat_textured && !sc->feat_envmap && !sc->feat_sphere_lights,
                            ensure_spill(ctx, sc->ecfg.spill_levels, (uint32_t)grid), grid, stream);
        HIP_CHECK(hipGetLastError());
        st.samples += P.total; st.wavefront_steps++;
        finish_pass(sc, plan, P, rgb_dev, samples_host, nullptr, stream);
    }
    st.render_ms = close_timer(ctx, stream);
    unsigned long long nb = 0;
    HIP_CHECK(hipMemcpy(&nb, ctx->chunk_counter.p, 8, hipMemcpyDeviceToHost));
    st.bounce_iterations = nb;
    if (env_set("LJ_VOLPATH_STATS")) {   // developer build only (-DLJ_VOLPATH_STATS=1): events and lane-events per part of the tracer
        unsigned long long h[32];
        HIP_CHECK(hipMemcpy(h, ctx->chunk_counter.p, sizeof(h), hipMemcpyDeviceToHost));
        const char *names[8] = {"node iterations", "leaf steps", "closest calls", "tracking (bounce ray)", "tracking (shadow segment)", "shadow segments", "path steps", "-"};
        for (int k = 0; k < 7; k++) fprintf(stderr, "[volpath stats] %-26s wave events %12llu  lanes active %5.1f %%  per sample %.2f\n", names[k], h[2 + 2 * k], h[2 + 2 * k] ? 100.0 * h[3 + 2 * k] / (64.0 * h[2 + 2 * k]) : 0.0, (double)h[3 + 2 * k] / (double)st.samples);
    }
}

// ---- tiny scenes (flat leaf table, shading tables in LDS): the fused persistent kernel, one launch per pass (mega.hip)

void render_mega(lj_scene *sc, const ljd::DScene &ds, const RenderPlan &plan, uint64_t pix_per_pass, float *rgb_dev, float *samples_host, hipStream_t stream, bool timing) {
    lj_context *ctx = sc->ctx;
    LjStats &st = sc->stats;
    ensure_sample_rgb(ctx, plan, pix_per_pass);
    // the launch's counter and statistics (an LJ_MEGA_ROUND_STATS build: and its tallies of the test rounds, dconfig.h)
    constexpr size_t state_bytes = LJ_MEGA_ROUND_STATS ? 256 : 64;
    static_assert(8 + (5 + ljd::kMegaRoundStats) * sizeof(unsigned long long) <= 256, "the tallies follow the five statistics");
    unsigned long long rounds[ljd::kMegaRoundStats] = {};
    if (!ctx->mega_state.p) ctx->mega_state.alloc(state_bytes);
    upload_pixel_list(ctx, plan, stream);
    HIP_CHECK(hipEventRecord(ctx->ev_begin, stream));
    const int per_cu = std::max(1, env_int("LJ_TUNE_MEGA_BLOCKS_PER_CU", ljd::mega_blocks_per_cu(sc->dscene, sc->scfg)));
    // camera samples a wave takes off the counter at a time: a multiple of 64 so that a wave's lanes share pixels, chosen so that
    // every wave draws ~16 times and the grid ends together — between 192 (below that the counter traffic shows) and 768:
    // the full bench frame 13.28 ms at 1024 per draw, 13.06 at 768; a 1/8 share of it (one rank of eight: tools/shard_time.py)
    // 2.50 ms at 1024, 2.00 at 192 (ideal 1.65)
    const bool grab_fixed = env_set("LJ_TUNE_MEGA_GRAB");
    const uint32_t grab_min = 192, grab_max = grab_fixed ? (uint32_t)std::max(64, env_int("LJ_TUNE_MEGA_GRAB", 768)) & ~63u : 768u;
    const uint64_t draws = (uint64_t)std::max(1, env_int("LJ_TUNE_MEGA_DRAWS", 16));
    const uint32_t item_cap_tune = mega_item_cap_tune();
    unsigned long long hstats[5] = {};
    for (uint64_t p0 = 0; p0 < plan.pixels->size(); p0 += pix_per_pass) {
        const Pass P = pass_at(sc, plan, p0, pix_per_pass);
        HIP_CHECK(hipMemsetAsync(ctx->mega_state.p, 0, state_bytes, stream));
        uint32_t grab = grab_max;
        if (!grab_fixed) {
            const uint64_t waves = (uint64_t)ctx->n_cus * per_cu * 4, per_draw = P.total / (waves * draws);
            grab = (uint32_t)std::min<uint64_t>(grab_max, std::max<uint64_t>(grab_min, per_draw & ~(uint64_t)63));
        }
        // persistent grid: as many workgroups as stay resident, but no more waves than there are `grab`-sized pieces of work
        const uint64_t pieces = (P.total + grab - 1) / grab;
        const int grid = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)ctx->n_cus * per_cu, (pieces + 3) / 4));
        unsigned long long *stats_dev = (unsigned long long *)((char *)ctx->mega_state.p + 8);
        if (timing) HIP_CHECK(hipEventRecord(ctx->ev_k0, stream));
        ljd::launch_mega(ds, P.d, sc->scfg, sc->flat.n_spheres > 0, (uint32_t)P.total, grab, item_cap_tune, (uint32_t *)ctx->mega_state.p, stats_dev, grid, stream);
        HIP_CHECK(hipGetLastError());
        if (timing) {
            HIP_CHECK(hipEventRecord(ctx->ev_k1, stream)); HIP_CHECK(hipEventSynchronize(ctx->ev_k1));
            st.mega_ms += elapsed_ms(ctx->ev_k0, ctx->ev_k1);
        }
        st.mega_launches++; st.wavefront_steps++;
        finish_pass(sc, plan, P, rgb_dev, samples_host, stats_dev, stream);   // (always waits: the launch's statistics)
        const unsigned long long *h = ctx->stats_host;
        if (h[3] != P.total)
            throw LjError(LJ_ERR_INTERNAL, "mega launch ended with " + std::to_string(h[3]) + " of " + std::to_string(P.total) + " samples finished");
        for (int k = 0; k < 5; k++) hstats[k] += h[k];
        st.samples += P.total;
#if LJ_MEGA_ROUND_STATS
        unsigned long long r[ljd::kMegaRoundStats];
        HIP_CHECK(hipMemcpy(r, stats_dev + 5, sizeof(r), hipMemcpyDeviceToHost));
        for (int k = 0; k < ljd::kMegaRoundStats; k++) rounds[k] += r[k];
#endif
    }
    st.render_ms = close_timer(ctx, stream);
    if (LJ_MEGA_ROUND_STATS && rounds[0]) {   // developer build only: the test rounds of the leaf scan, over the render
        unsigned long long half = 0;
        for (int k = 0; k < 4; k++) half += rounds[3 + k];
        fprintf(stderr, "[mega round stats] passes %llu  items per pass %.1f  test rounds per pass %.3f  last round at most half full (<= 32 items) %.1f %% of passes\n",
                rounds[0], (double)rounds[1] / (double)rounds[0], (double)rounds[2] / (double)rounds[0], 100.0 * (double)half / (double)rounds[0]);
        for (int k = 0; k < 8; k++) fprintf(stderr, "[mega round stats] last round of %2d .. %2d items: %12llu passes  %5.1f %%\n", 8 * k + 1, 8 * k + 8, rounds[3 + k], 100.0 * (double)rounds[3 + k] / (double)rounds[0]);
    }
    st.bounce_iterations = hstats[0]; st.rays_closest = hstats[1]; st.rays_shadow = hstats[2]; st.path_steps = hstats[4];
    // algorithmic HBM bytes of a mega launch: the finished radiance of every sample (12 B) and its pixel's list entry — the path state
    // never leaves the registers
    st.mega_bytes = st.samples * 12ull + plan.pixels->size() * 4ull;
    st.queue_bytes = st.mega_bytes;
}

// ---- the wavefront plan: extend / shade steps over a queue of paths, in up to four lanes

// queue geometry: n_blocks workgroups x seg slots; workgroup b owns slots [b*seg, (b+1)*seg)
struct WaveGeometry {
    uint32_t pool, n_lanes, n_blocks, lane_blocks, seg, n_slots, lane_slots;
    uint32_t ext_grid, lane_chunks, spill_grid;
    bool use_tail, sort_segments;
    uint64_t tail_num, tail_den;   // fuse once fewer than tail_num / tail_den of the slots hold a path
};

// instrumented: kernels timed one by one, or the extend kernel's utilisation counters asked for
WaveGeometry wavefront_geometry(const lj_scene *sc, const RenderPlan &plan, uint64_t pass_samples_max, bool instrumented) {
    WaveGeometry g{};
    g.pool = (uint32_t)std::min<uint64_t>(plan.pool, std::max<uint64_t>(pass_samples_max, 256));
    const uint32_t blocks_per_cu = (uint32_t)std::max(1, env_int("LJ_TUNE_BLOCKS_PER_CU", 8));
    // Lanes: the pool, its workgroup segments and the pass's samples are split into four parts that advance
    // independently on four streams.  The extend kernel is bound by VALU issue and moves few bytes, the shade kernel
    // streams the queue and leaves the VALUs mostly idle; with four staggered lanes the GPU always has some of each to
    // run side by side (two lanes: +13 % time on cbox; six or eight: worse again — more streams than hardware queues).
    // (One lane when kernels are timed individually or for tiny renders, two for small ones, or on request.)
    g.n_lanes = (instrumented || g.pool < (1u << 20)) ? 1u : (g.pool < (1u << 22) ? 2u : 4u);
    // the Disney / all-features shade kernels (164 VGPRs, three waves per SIMD) leave an extend kernel no registers to run beside
    // them: lanes would only time-slice the GPU (disney_bsdf 256 spp: 104 ms with one lane, 116 with two; a 64-spp render, which fits
    // the pool at once, is the other way round by 7 %)
    if (sc->scfg.variant >= 4) g.n_lanes = 1;   // (FeatDisney, FeatAll)
    // a tree beyond the LDS image (nodes fetched through L2): one lane.  Its extend launches fill every CU (five workgroups of 30 KiB
    // LDS and 92 VGPRs each), so the lanes' kernels queue up behind one another instead of running side by side (tools/lanes_sweep.sh,
    // sponza 256 spp: 202.5 ms with one lane, 208.8 with four)
    const bool large_tree = sc->dscene.n_nodes > sc->ecfg.lds_nodes;
    if (large_tree) g.n_lanes = 1;
    g.n_lanes = (uint32_t)std::min((int)kMaxLanes, std::max(1, env_int("LJ_TUNE_LANES", (int)g.n_lanes)));
    g.n_blocks = std::min<uint32_t>(kMaxBlocks, std::max<uint32_t>(g.n_lanes, std::min<uint32_t>((uint32_t)sc->ctx->n_cus * blocks_per_cu, g.pool / 256)));
    g.n_blocks = (g.n_blocks / g.n_lanes) * g.n_lanes;
    g.lane_blocks = g.n_blocks / g.n_lanes;
    g.seg = ((g.pool + g.n_blocks - 1) / g.n_blocks + 255u) & ~255u;
    g.n_slots = g.n_blocks * g.seg; g.lane_slots = g.lane_blocks * g.seg;
    // feature sets that sort a segment as a whole shade from one set of queue records into another (kernels.hip shade_sorted_segment)
    g.sort_segments = ljd::shade_sorts_segments(sc->scfg);
    // extend: persistent workgroups that draw 256-slot chunks of the queue.  One lane: more workgroups than fit at once, so
    // the hardware keeps every CU as full as registers and LDS allow; several lanes: few enough that the other lanes'
    // shade workgroups find registers beside them (8 extend waves per CU and lane).
    const uint32_t ext_per_cu = (uint32_t)std::max(1, env_int("LJ_TUNE_EXTEND_BLOCKS_PER_CU", g.n_lanes == 1 ? 8 : (g.n_lanes == 2 ? 4 : 2)));
    g.lane_chunks = g.lane_slots / 256u;
    g.ext_grid = std::max<uint32_t>(1, std::min<uint32_t>((uint32_t)sc->ctx->n_cus * ext_per_cu, (g.lane_chunks + 3) / 4));
    // (the fused tail launches one workgroup per segment, so its overflow stacks are sized for the shade grid)
    // (not for a large tree: the tail's lane-by-lane traversal — one workgroup per segment, leaves tested unpooled — is slower there than
    // the extend / shade launches it replaces: tools/tail_sweep.sh, sponza 64 spp 60.4 -> 56.2 ms, disney_bsdf 256 spp 98.7 -> 97.2 without it)
    g.use_tail = !instrumented && !large_tree && ljd::tail_smem(sc->ecfg, sc->scfg) > 0 && env_int("LJ_TUNE_TAIL", 1) != 0;
    g.tail_num = (uint64_t)std::max(1, env_int("LJ_TUNE_TAIL_FRAC", 1));   // (LJ_TUNE_TAIL_FRAC=n: n / 16)
    g.tail_den = env_set("LJ_TUNE_TAIL_FRAC") ? 16 : 4;
    g.spill_grid = std::max<uint32_t>(g.ext_grid, g.use_tail ? g.lane_blocks : 0u);
    return g;
}

// one lane's part of the workspace and its state on the host
struct Lane {
    hipStream_t stream; ljd::DQueue q, q2; uint32_t *sort_perm; uint8_t *sort_keys; ljd::DBlockState *dblocks; ljd::DBlockState *hblocks;
    uint32_t *work; uint32_t *lists[2]; uint32_t parity; int *spill; bool done, pending; int batch;
};

// grows the context's workspace to the geometry and carves the lanes from it (lane 0 runs on the render stream)
void setup_lanes(lj_scene *sc, const WaveGeometry &g, hipStream_t stream, Lane *lanes) {
    lj_context *ctx = sc->ctx;
    const uint32_t cap = (g.n_slots + 63u) & ~63u;
    ensure_queue(ctx->queue_mem, ctx->queue_capacity, cap);
    if (g.sort_segments) {
        ensure_queue(ctx->queue_mem2, ctx->queue2_capacity, cap);
        ensure(ctx->sort_perm, (size_t)cap * 4);
        ensure(ctx->sort_keys, (size_t)cap);
    }
    int *spill_base = ensure_spill(ctx, sc->ecfg.spill_levels, g.spill_grid * g.n_lanes);
    // per lane: work[0] = the extend kernel's draw counter, work[1 + parity] = number of listed chunks; two chunk lists, used
    // alternately, so that a shade launch can append to one while nothing reads it
    if (!ctx->chunk_counter.p) ctx->chunk_counter.alloc(128 * kMaxLanes);
    ensure(ctx->chunk_list, (size_t)g.lane_chunks * 8 * g.n_lanes);
    const ljd::DQueue q_all = carve_queue(ctx->queue_mem.p, ctx->queue_capacity);
    const ljd::DQueue q2_all = g.sort_segments ? carve_queue(ctx->queue_mem2.p, ctx->queue2_capacity) : q_all;
    for (uint32_t l = 0; l < g.n_lanes; l++) {
        Lane &L = lanes[l];
        L.stream = l == 0 ? stream : ctx->lane_streams[l - 1];
        const size_t o = (size_t)l * g.lane_slots;
        L.q = queue_at(q_all, o); L.q2 = queue_at(q2_all, o);
        L.sort_perm = g.sort_segments ? (uint32_t *)ctx->sort_perm.p + o : nullptr; L.sort_keys = g.sort_segments ? (uint8_t *)ctx->sort_keys.p + o : nullptr;
        L.dblocks = (ljd::DBlockState *)ctx->blocks.p + (size_t)l * g.lane_blocks; L.hblocks = ctx->blocks_host + (size_t)l * g.lane_blocks;
        L.work = (uint32_t *)ctx->chunk_counter.p + 32 * l;
        L.lists[0] = (uint32_t *)ctx->chunk_list.p + (size_t)l * 2 * g.lane_chunks; L.lists[1] = L.lists[0] + g.lane_chunks;
        L.spill = spill_base ? spill_base + (size_t)l * sc->ecfg.spill_levels * g.spill_grid * 256 : nullptr;
    }
}

// one shade launch of a lane at its current parity; afterwards L.q is the record set the paths are in
void shade_step(const lj_scene *sc, const ljd::DScene &ds, const WaveGeometry &g, const ljd::DPass &pass, Lane &L) {
    ljd::launch_shade(ds, pass, L.q, L.q2, L.sort_perm, L.sort_keys, L.dblocks, g.lane_blocks, g.seg, sc->scfg, L.work, L.lists[L.parity], L.parity, g.ext_grid * 4u, L.stream);
    if (g.sort_segments) std::swap(L.q, L.q2);
}

// the pass's inputs on the device, then every lane's step 0
void start_pass(lj_scene *sc, const ljd::DScene &ds, const WaveGeometry &g, const Pass &P, Lane *lanes, hipStream_t stream) {
    lj_context *ctx = sc->ctx;
    // contiguous sample ranges per workgroup, multiples of 64 so that a wave's first samples share a pixel
    const uint64_t per = ((P.total + g.n_blocks - 1) / g.n_blocks + 63) & ~(uint64_t)63;
    for (uint32_t b = 0; b < g.n_blocks; b++) {
        ljd::DBlockState bs{};
        bs.next_sample = (uint32_t)std::min<uint64_t>(P.total, (uint64_t)b * per); bs.end_sample = (uint32_t)std::min<uint64_t>(P.total, (uint64_t)(b + 1) * per);
        ctx->blocks_host[b] = bs;
    }
    HIP_CHECK(hipMemcpyAsync(ctx->blocks.p, ctx->blocks_host, sizeof(ljd::DBlockState) * g.n_blocks, hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipMemsetAsync(ctx->chunk_counter.p, 0, 128 * kMaxLanes, stream));
    if (g.n_lanes > 1) {  // the second lane starts once the pass's inputs are in place
        HIP_CHECK(hipEventRecord(ctx->ev_fork, stream));
        for (uint32_t l = 1; l < g.n_lanes; l++) HIP_CHECK(hipStreamWaitEvent(ctx->lane_streams[l - 1], ctx->ev_fork, 0));
    }
    // step 0 is a shade over empty segments: it only generates camera rays
    for (uint32_t l = 0; l < g.n_lanes; l++) {
        Lane &L = lanes[l];
        L.parity = 0; L.done = false; L.pending = false; L.batch = 8;  // steps per host round trip; all per-step state lives on the device
        // stagger: lane l starts when lane l-1 has generated its camera rays, so its shade launches fall on the other
        // lane's extend launches (the two lanes have equal work per step, so the phase offset persists)
        if (l > 0) HIP_CHECK(hipStreamWaitEvent(L.stream, ctx->ev_join, 0));
        shade_step(sc, ds, g, P.d, L);
        if (l + 1 < g.n_lanes) HIP_CHECK(hipEventRecord(ctx->ev_join, L.stream));
    }
}

// Round-robin over the lanes until every path of the pass has ended: look at a lane's block states only when its previous batch has
// drained, and give it its next batch at once, so the other lane's kernels keep the GPU busy during this lane's host round trip.
void run_lanes(lj_scene *sc, const ljd::DScene &ds, const WaveGeometry &g, const Pass &P, Lane *lanes, bool timing, unsigned long long *xstats) {
    lj_context *ctx = sc->ctx;
    LjStats &st = sc->stats;
    for (int guard = 0; guard < (1 << 21); guard++) {
        bool any = false;
        for (uint32_t l = 0; l < g.n_lanes; l++) {
            Lane &L = lanes[l];
            if (L.done) continue;
            bool fuse = false;
            if (L.pending) {
                HIP_CHECK(hipStreamSynchronize(L.stream));
                L.pending = false;
                uint64_t alive = 0;
                for (uint32_t b = 0; b < g.lane_blocks; b++) alive += L.hblocks[b].count;
                L.done = alive == 0;
                // the long tail (a few deep paths left): launches are nearly empty, so look less often
                L.batch = alive * 64ull < (uint64_t)g.lane_slots ? 16 : 8;
                if (L.done) continue;
                // ... or not at all: once every camera sample has been started and the segments are mostly empty, the
                // rest of the lane's paths finish inside one fused launch (k_tail)
                uint64_t to_start = 0;
                for (uint32_t b = 0; b < g.lane_blocks; b++) to_start += L.hblocks[b].end_sample - L.hblocks[b].next_sample;
                fuse = g.use_tail && to_start == 0 && alive * g.tail_den < (uint64_t)g.lane_slots * g.tail_num;
            }
            any = true;
            if (fuse) ljd::launch_tail(ds, P.d, L.q, L.dblocks, g.lane_blocks, g.seg, sc->ecfg, sc->scfg, L.spill, L.stream);
            else for (int b = 0; b < L.batch; b++) {
                if (timing) HIP_CHECK(hipEventRecord(ctx->ev_k0, L.stream));
                ljd::launch_extend(ds, L.q, L.dblocks, g.ext_grid, g.seg, L.work, L.lists[L.parity], L.parity, sc->ecfg, L.spill, xstats, L.stream);
                if (timing) HIP_CHECK(hipEventRecord(ctx->ev_k1, L.stream));
                L.parity ^= 1u;
                shade_step(sc, ds, g, P.d, L);
                if (timing) {
                    HIP_CHECK(hipEventRecord(ctx->ev_end, L.stream));
                    HIP_CHECK(hipEventSynchronize(ctx->ev_end));
                    st.extend_ms += elapsed_ms(ctx->ev_k0, ctx->ev_k1); st.shade_ms += elapsed_ms(ctx->ev_k1, ctx->ev_end);
                }
                st.extend_launches++; st.shade_launches++;
                if (l == 0) st.wavefront_steps++;
            }
            HIP_CHECK(hipGetLastError());
            HIP_CHECK(hipMemcpyAsync(L.hblocks, L.dblocks, sizeof(ljd::DBlockState) * g.lane_blocks, hipMemcpyDeviceToHost, L.stream));
            L.pending = true;
        }
        if (!any) break;
    }
}

// the finished pass in LjStats, from the block states the lanes left on the host
void account_pass(lj_scene *sc, const WaveGeometry &g, const Pass &P) {
    LjStats &st = sc->stats;
    uint64_t samples_done = 0, path_steps = 0, shadow_rays = 0;
    for (uint32_t b = 0; b < g.n_blocks; b++) {
        const ljd::DBlockState &bs = sc->ctx->blocks_host[b];
        samples_done += bs.samples_done; path_steps += bs.path_steps; shadow_rays += bs.rays_shadow;
        st.bounce_iterations += bs.bounce_iterations; st.rays_closest += bs.rays_closest; st.rays_shadow += bs.rays_shadow;
    }
    if (samples_done != P.total)
        throw LjError(LJ_ERR_INTERNAL, "wavefront loop ended with " + std::to_string(samples_done) + " of " + std::to_string(P.total) + " samples finished");
    st.samples += P.total;
    // algorithmic queue traffic per live path-step: extend reads ro, rd (32 B), rs (16 B) when a shadow ray
    // is pending, and writes rh (16 B); shade reads 7 records (112 B) and writes 7 (112 B), plus 12 B per finished sample
    st.path_steps += path_steps;
    st.extend_bytes += path_steps * 48ull + shadow_rays * 16ull;
    st.shade_bytes += path_steps * 224ull + P.total * 12ull;
}

void render_wavefront(lj_scene *sc, const ljd::DScene &ds, const RenderPlan &plan, uint64_t pix_per_pass, float *rgb_dev, float *samples_host, hipStream_t stream, bool timing) {
    lj_context *ctx = sc->ctx;
    // developer instrumentation of the extend kernel (utilisation counters printed to stderr); off unless asked for
    unsigned long long *xstats = nullptr;
    DevBuf xstats_buf;
    if (env_set("LJ_EXTEND_STATS")) { xstats_buf.alloc(64); HIP_CHECK(hipMemsetAsync(xstats_buf.p, 0, 64, stream)); xstats = (unsigned long long *)xstats_buf.p; }
    const WaveGeometry g = wavefront_geometry(sc, plan, pix_per_pass * (uint64_t)plan.spp, timing || xstats);
    Lane lanes[kMaxLanes];
    setup_lanes(sc, g, stream, lanes);
    ensure_sample_rgb(ctx, plan, pix_per_pass);
    upload_pixel_list(ctx, plan, stream);
    HIP_CHECK(hipEventRecord(ctx->ev_begin, stream));
    for (uint64_t p0 = 0; p0 < plan.pixels->size(); p0 += pix_per_pass) {
        const Pass P = pass_at(sc, plan, p0, pix_per_pass);
        start_pass(sc, ds, g, P, lanes, stream);
        run_lanes(sc, ds, g, P, lanes, timing, xstats);
        account_pass(sc, g, P);
        // (both lanes were synchronised with the host above, so the caller's stream may read what the second lane wrote)
        finish_pass(sc, plan, P, rgb_dev, samples_host, nullptr, stream);
    }
    sc->stats.render_ms = close_timer(ctx, stream);
    if (xstats) {
        unsigned long long h[8];
        HIP_CHECK(hipMemcpy(h, xstats, 64, hipMemcpyDeviceToHost));
        fprintf(stderr, "[extend stats] rays %llu | outer iters %llu busy lanes %.1f%% | node steps %llu (%.2f/ray) lane use %.1f%% | prim rounds %llu (%.2f tests/ray) lane use %.1f%% | refills %llu\n",
                h[7], h[0], 100.0 * h[1] / (64.0 * h[0]), h[2], (double)h[3] / h[7], 100.0 * h[3] / (64.0 * h[2]), h[4], (double)h[5] / h[7], 100.0 * h[5] / (64.0 * h[4]), h[6]);
    }
    sc->stats.queue_bytes = sc->stats.extend_bytes + sc->stats.shade_bytes;
}

} // namespace

// overflow stack storage for a launch of `grid` workgroups over a scene whose BVH needs `levels` levels beyond LDS
int *ensure_spill(lj_context *ctx, int levels, uint32_t grid) {
    if (levels <= 0) return nullptr;
    ensure(ctx->spill, (size_t)levels * grid * 256 * sizeof(int));
    return (int *)ctx->spill.p;
}

// what a plan takes from the arguments whatever it renders: samples, seed, depth, pool
static void plan_basics(const lj_scene *sc, const LjRenderArgs *a, RenderPlan &p) {
    p.spp = (a && a->spp > 0) ? a->spp : sc->flat.spp;
    if (p.spp <= 0) throw LjError(LJ_ERR_INVALID_ARG, "samples per pixel must be positive");
    p.seed = (a && a->seed) ? a->seed : 0x853c49e6748fea9bULL;
    p.max_depth = (a && a->max_depth != INT32_MIN) ? a->max_depth : sc->flat.max_depth;
    // 128 M paths in flight = 16 GiB of queue records (of the 288 GB a MI355X has; allocated only as far as a pass has samples): long
    // per-wave slices keep the extend kernel's lanes refilled and every launch's drain phase is amortised over more paths
    // (tools/pool_big.sh, sponza 1024 spp: 2^25 828 ms, 2^26 811, 2^27 794, 2^28 793; disney_bsdf 256 spp: 97.3 / 93.4 / 91.8 / 91.5)
    p.pool = (a && a->pool_paths) ? a->pool_paths : (1u << 27);
    p.pool = std::max<uint32_t>(p.pool, 4096);
}

RenderPlan make_plan(lj_scene *sc, const LjRenderArgs *a) {
    RenderPlan p;
    const int w = sc->flat.cam.width, h = sc->flat.cam.height;
    plan_basics(sc, a, p);
    p.rng_mode = a ? a->rng_mode : LJ_RNG_SAMPLE;
    if (p.rng_mode != LJ_RNG_SAMPLE && p.rng_mode != LJ_RNG_TILE) throw LjError(LJ_ERR_UNSUPPORTED, "rng_mode must be LJ_RNG_SAMPLE or LJ_RNG_TILE");
    int rank = a ? a->rank : 0, world = (a && a->world_size > 0) ? a->world_size : 1;
    if (rank < 0 || rank >= world) throw LjError(LJ_ERR_INVALID_ARG, "rank must be in [0, world_size)");
    bool crop = a && a->crop_x1 > a->crop_x0 && a->crop_y1 > a->crop_y0;
    int cx0 = crop ? a->crop_x0 : 0, cy0 = crop ? a->crop_y0 : 0, cx1 = crop ? a->crop_x1 : w, cy1 = crop ? a->crop_y1 : h;
    if (cx0 < 0 || cy0 < 0 || cx1 > w || cy1 > h) throw LjError(LJ_ERR_INVALID_ARG, "crop window outside the film");
    const int tile = 16, ntx = (w + tile - 1) / tile, nty = (h + tile - 1) / tile;  // render.cpp:75-77
    p.rank = rank; p.world = world; p.cx0 = cx0; p.cy0 = cy0; p.cx1 = cx1; p.cy1 = cy1;
    // the pixel list depends on the share only (rank, world, crop): a render loop asks for the same one every frame
    const uint64_t key_parts[9] = {(uint64_t)rank, (uint64_t)world, (uint64_t)crop, (uint64_t)cx0, (uint64_t)cy0, (uint64_t)cx1, (uint64_t)cy1, (uint64_t)w, (uint64_t)h};
    uint64_t key = 1469598103934665603ull;
    for (uint64_t v : key_parts) { key ^= v + 0x9e3779b97f4a7c15ull; key *= 1099511628211ull; }
    key ^= (uint64_t)(uintptr_t)sc; key |= 1ull;
    if (sc->plan_pixels && sc->plan_pixels_key == key) { p.pixels = sc->plan_pixels; p.pixels_key = key; return p; }
    auto pixels = std::make_shared<std::vector<uint32_t>>();
    if (crop) {  // crop windows are enumerated row-major (lj_render_samples layout)
        for (int y = cy0; y < cy1; y++) for (int x = cx0; x < cx1; x++) {
            int t = (y / tile) * ntx + (x / tile);
            if (t % world == rank) pixels->push_back((uint32_t)(y * w + x));
        }
    } else {
        for (int t = 0; t < ntx * nty; t++) {
            if (t % world != rank) continue;
            int tx = t % ntx, ty = t / ntx;
            int x0 = tx * tile, x1 = std::min(x0 + tile, w), y0 = ty * tile, y1 = std::min(y0 + tile, h);
            for (int y = y0; y < y1; y++) for (int x = x0; x < x1; x++) pixels->push_back((uint32_t)(y * w + x));
        }
    }
    p.pixels = pixels; p.pixels_key = key;
    sc->plan_pixels = pixels; sc->plan_pixels_key = key;
    return p;
}

// The plan of a batch of n_views cameras: the single-view plan of the same args (share and crop apply to every view) with its pixel list
// repeated per view, offset by the view's first pixel in the n_views * h rows tall frame.
RenderPlan make_views_plan(lj_scene *sc, const LjRenderArgs *a, int n_views) {
    RenderPlan p = make_plan(sc, a);
    if (p.rng_mode != LJ_RNG_SAMPLE) throw LjError(LJ_ERR_UNSUPPORTED, "lj_render_views: rng_mode must be LJ_RNG_SAMPLE (no per-tile schedule for a batch of cameras)");
    const uint64_t view_pixels = (uint64_t)sc->flat.cam.width * (uint64_t)sc->flat.cam.height;
    uint64_t key = (p.pixels_key ^ (0x9e3779b97f4a7c15ull + (uint64_t)n_views)) * 1099511628211ull; key |= 1ull;
    p.n_views = n_views;
    if (sc->views_pixels && sc->views_pixels_key == key) { p.pixels = sc->views_pixels; p.pixels_key = key; return p; }
    auto all = std::make_shared<std::vector<uint32_t>>();
    all->reserve(p.pixels->size() * (size_t)n_views);
    for (int v = 0; v < n_views; v++) {
        const uint32_t first = (uint32_t)((uint64_t)v * view_pixels);   // (n_views * w * h <= 2^31: checked by the caller)
        for (uint32_t e : *p.pixels) all->push_back(first + e);
    }
    p.pixels = all; p.pixels_key = key;
    sc->views_pixels = all; sc->views_pixels_key = key;
    return p;
}

// The plan of a table of n rays or probes (lj_radiance_rays / lj_irradiance, dprobe.h): the identity list — entry i is ray i, so that a sample's
// stream is i * spp + s — no tiles, no share, no crop, no views.  The caller (who has checked the arguments) sets the table and the ray source.
RenderPlan make_rays_plan(lj_scene *sc, const LjRenderArgs *a, int64_t n) {
    RenderPlan p;
    plan_basics(sc, a, p);
    p.rng_mode = LJ_RNG_SAMPLE;
    p.rank = 0; p.world = 1; p.cx0 = 0; p.cy0 = 0; p.cx1 = sc->flat.cam.width; p.cy1 = sc->flat.cam.height;
    uint64_t key = (0x7261797300000000ull ^ (uint64_t)n) * 1099511628211ull; key ^= (uint64_t)(uintptr_t)sc; key |= 1ull;
    if (sc->rays_pixels && sc->rays_pixels_key == key) { p.pixels = sc->rays_pixels; p.pixels_key = key; return p; }
    auto list = std::make_shared<std::vector<uint32_t>>((size_t)n);
    for (int64_t i = 0; i < n; i++) (*list)[(size_t)i] = (uint32_t)i;
    p.pixels = list; p.pixels_key = key;
    sc->rays_pixels = list; sc->rays_pixels_key = key;
    return p;
}

// Renders plan.pixels; if rgb_dev != null writes radiance/spp there (other pixels untouched), if samples_host != null
// the per-sample radiance of every pass is copied to host memory in pixel-list order.  One driver per kernel plan, picked in this order.
void run_render(lj_scene *sc, const RenderPlan &plan, float *rgb_dev, float *samples_host, hipStream_t stream, bool timing) {
    set_device(sc->ctx);
    sc->stats = LjStats{};
    sc->feature_stats = LjFeatureStats{};
    sc->adaptive_stats = LjAdaptiveStats{};
    if (plan.pixels->empty()) return;
    if (sc->flat.integrator < LJ_INTEGRATOR_PATH) return render_aux(sc, plan, rgb_dev, samples_host, stream);
    ljd::DScene ds = sc->dscene;   // the scene as the plan's kernels see it
    ds.max_depth = plan.max_depth;
    if (plan.rng_mode == LJ_RNG_TILE) return render_tiles(sc, ds, plan, rgb_dev, samples_host, stream);   // (the auxiliary integrators draw nothing: as above)
    const uint64_t pix_per_pass = pixels_per_pass(plan);
    // a features request: room in the overflow stacks for the guide-buffer launch of the largest pass, before a driver takes its part of them
    if (plan.feat.want & ljd::FEAT_FIRST_HIT) ensure_spill(sc->ctx, sc->ecfg.spill_levels, (uint32_t)ljd::features_grid(pix_per_pass, (uint32_t)plan.spp, sc->ctx->n_cus));
    if (sc->flat.integrator == LJ_INTEGRATOR_VOLPATH) return render_volpath(sc, ds, plan, pix_per_pass, rgb_dev, samples_host, stream);
    // (a table of rays never runs k_mega: its first vertices are made in the refill loop of k_shade and in k_volpath alone)
    if (plan.ray_kind == ljd::RAY_SOURCE_NONE && ljd::mega_smem(sc->dscene, sc->scfg) > 0 && mega_enabled()) return render_mega(sc, ds, plan, pix_per_pass, rgb_dev, samples_host, stream, timing);
    render_wavefront(sc, ds, plan, pix_per_pass, rgb_dev, samples_host, stream, timing);
}

// lj_probe_ray_queries: the passes of run_render over a probes plan, each answered by k_probe_rays instead of a path kernel — the same list,
// the same pass arithmetic, the same DPass, so that a sample's ray here is the ray its path starts with there.
void run_probe_rays(lj_scene *sc, const RenderPlan &plan, float *rays_host, hipStream_t stream) {
    set_device(sc->ctx);
    if (plan.pixels->empty()) return;
    lj_context *ctx = sc->ctx;
    const uint64_t pix_per_pass = pixels_per_pass(plan);
    ensure(ctx->ray_out, pix_per_pass * (uint64_t)plan.spp * 24);
    upload_pixel_list(ctx, plan, stream);
    for (uint64_t p0 = 0; p0 < plan.pixels->size(); p0 += pix_per_pass) {
        const Pass P = pass_at(sc, plan, p0, pix_per_pass);
        ljd::launch_probe_rays(sc->dscene, P.d, (uint32_t)P.total, (float *)ctx->ray_out.p, ctx->n_cus, stream);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(rays_host + P.p0 * (uint64_t)plan.spp * 6, ctx->ray_out.p, P.total * 24, hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
    }
}
