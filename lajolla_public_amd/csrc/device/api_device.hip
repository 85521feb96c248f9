// C-ABI entry points that own the GPU: context, scene upload, the wavefront render loop, batched ray queries.
// One context = one HIP device + one stream; one process per GPU (the multi-GPU layer above this is
// torch.distributed over RCCL, see bench.py).  Every HIP call is checked; failures surface as LJ_ERR_DEVICE with
// the HIP error string — there is no CPU fallback behind any of these functions.
#include "api_internal.h"
#include <chrono>
#include <mutex>
#include <set>

namespace {

void set_device(lj_context *ctx) { HIP_CHECK(hipSetDevice(ctx->device)); }

ljd::DQueue carve_queue(void *base, uint32_t cap) {
    // one allocation, eight arrays of 16-byte records; hipMalloc returns 256-byte aligned memory and cap is a
    // multiple of 64, so every array starts on a 1 KiB boundary (one full wave instruction)
    ljd::DQueue q{};
    ljd::Rec4 *p = (ljd::Rec4 *)base;
    auto take = [&]() { ljd::Rec4 *r = p; p += cap; return r; };
    q.ro = take(); q.rd = take(); q.rs = take(); q.rh = take(); q.rw = take(); q.rl = take(); q.rn = take(); q.rg = take();
    return q;
}
size_t queue_bytes(uint32_t cap) { return (size_t)cap * kQueueSlotBytes; }

void ensure_queues(lj_context *ctx, uint32_t cap) {
    if (ctx->queue_capacity >= cap) return;
    cap = (cap + 63u) & ~63u;
    ctx->queue_mem.alloc(queue_bytes(cap));
    ctx->queue_capacity = cap;
}

// overflow stack storage for a launch of `grid` workgroups over a scene whose BVH needs `levels` levels beyond LDS
int *ensure_spill(lj_context *ctx, int levels, uint32_t grid) {
    if (levels <= 0) return nullptr;
    const size_t need = (size_t)levels * grid * 256 * sizeof(int);
    if (ctx->spill.bytes < need) ctx->spill.alloc(need);
    return (int *)ctx->spill.p;
}

struct RenderPlan {
    int spp; uint32_t pool; uint64_t seed;
    std::shared_ptr<const std::vector<uint32_t>> pixels;  // rendered pixels in tile order (cached per scene: same share -> same list)
    uint64_t pixels_key = 0;                               // identifies the list on the device (lj_context::pixel_list_key)
    int max_depth;
    int rng_mode;                                          // LJ_RNG_SAMPLE / LJ_RNG_TILE
    int rank, world, cx0, cy0, cx1, cy1;                   // the share and the crop window (the full frame when there is none)
    // a batch of cameras (lj_render_views): `pixels` lists e = v*w*h + y*w + x — the single-view list, in its order, once per view — and
    // views_dev is the batch's camera table on the device (0 / null: the scene's one camera)
    int n_views = 0; const ljd::DCamera *views_dev = nullptr;
};

RenderPlan make_plan(const lj_scene *sc, const LjRenderArgs *a) {
    RenderPlan p;
    const int w = sc->flat.cam.width, h = sc->flat.cam.height;
    p.spp = (a && a->spp > 0) ? a->spp : sc->flat.spp;
    if (p.spp <= 0) throw LjError(LJ_ERR_INVALID_ARG, "samples per pixel must be positive");
    p.seed = (a && a->seed) ? a->seed : 0x853c49e6748fea9bULL;
    p.max_depth = (a && a->max_depth != INT32_MIN) ? a->max_depth : sc->flat.max_depth;
    // 128 M paths in flight = 16 GiB of queue records (of the 288 GB a MI355X has; allocated only as far as a pass has samples): long
    // per-wave slices keep the extend kernel's lanes refilled and every launch's drain phase is amortised over more paths
    // (tools/pool_big.sh, sponza 1024 spp: 2^25 828 ms, 2^26 811, 2^27 794, 2^28 793; disney_bsdf 256 spp: 97.3 / 93.4 / 91.8 / 91.5)
    p.pool = (a && a->pool_paths) ? a->pool_paths : (1u << 27);
    p.pool = std::max<uint32_t>(p.pool, 4096);
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
    lj_scene *msc = const_cast<lj_scene *>(sc);
    if (msc->plan_pixels && msc->plan_pixels_key == key) { p.pixels = msc->plan_pixels; p.pixels_key = key; return p; }
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
    msc->plan_pixels = pixels; msc->plan_pixels_key = key;
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

// the plan's pixel list on the device; the copy is skipped when the context still holds this very list
void upload_pixel_list(lj_context *ctx, const RenderPlan &plan, hipStream_t stream) {
    const size_t n = plan.pixels->size();
    if (ctx->pixel_list.bytes < n * 4) { ctx->pixel_list.alloc(n * 4); ctx->pixel_list_key = 0; }
    if (ctx->pixel_list_key == plan.pixels_key && plan.pixels_key != 0) return;
    HIP_CHECK(hipMemcpyAsync(ctx->pixel_list.p, plan.pixels->data(), n * 4, hipMemcpyHostToDevice, stream));
    ctx->pixel_list_key = plan.pixels_key;
}

// The per-tile schedule (LJ_RNG_TILE, dtile.h / tile.hip) for path and volpath: every tile of the share that touches the crop window is
// walked whole — its stream is consumed for the pixels outside the window too — and only the window's pixels are written (rgb_dev:
// radiance / spp; samples_host: per-sample radiance in lj_render_samples layout).  Bounded launches: each advances every unfinished tile
// by at most LJ_TUNE_TILE_STEPS path steps; the cursors stay in HBM between launches.  LjStats.samples counts every sample traced,
// those outside the window included.
void run_tiles(lj_scene *sc, const RenderPlan &plan, const ljd::DScene &ds, float *rgb_dev, float *samples_host, hipStream_t stream) {
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
    uint32_t lanes = 1;
    if (const char *e = getenv("LJ_TUNE_TILE_LANES")) lanes = (uint32_t)std::min(64, std::max(1, atoi(e)));
    uint32_t budget = 512;   // path steps per tile and launch
    if (const char *e = getenv("LJ_TUNE_TILE_STEPS")) budget = (uint32_t)std::max(1, atoi(e));
    const size_t cur_bytes = ljd::tile_cursor_bytes(vol) * n_tiles;
    if (ctx->tile_cursors.bytes < cur_bytes) ctx->tile_cursors.alloc(cur_bytes);
    if (ctx->tile_list.bytes < (size_t)n_tiles * 4 + 64) ctx->tile_list.alloc((size_t)n_tiles * 4 + 64);
    const uint64_t n_samples_out = samples_host ? (uint64_t)(plan.cx1 - plan.cx0) * (uint64_t)(plan.cy1 - plan.cy0) * (uint64_t)plan.spp : 0;
    if (samples_host && ctx->tile_samples.bytes < n_samples_out * 12) ctx->tile_samples.alloc(n_samples_out * 12);
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
    HIP_CHECK(hipEventRecord(ctx->ev_end, stream));
    HIP_CHECK(hipEventSynchronize(ctx->ev_end));
    float ms = 0; HIP_CHECK(hipEventElapsedTime(&ms, ctx->ev_begin, ctx->ev_end));
    std::vector<unsigned char> cur_host(cur_bytes);
    HIP_CHECK(hipMemcpy(cur_host.data(), ctx->tile_cursors.p, cur_bytes, hipMemcpyDeviceToHost));
    if (samples_host) HIP_CHECK(hipMemcpy(samples_host, ctx->tile_samples.p, n_samples_out * 12, hipMemcpyDeviceToHost));
    unsigned long long c[5];
    ljd::tile_cursor_stats(vol, cur_host.data(), n_tiles, c);
    st.render_ms = ms; st.samples = c[0]; st.bounce_iterations = c[1]; st.rays_closest = c[2]; st.rays_shadow = c[3]; st.path_steps = c[4];
    st.wavefront_steps = launches;
}

// Renders plan.pixels; if rgb_dev != null writes radiance/spp there (other pixels untouched), if samples_host != null
// the per-sample radiance of every pass is copied to host memory in pixel-list order.
void run_render(lj_scene *sc, const RenderPlan &plan, float *rgb_dev, float *samples_host, hipStream_t stream, bool timing) {
    lj_context *ctx = sc->ctx;
    set_device(ctx);
    ljd::DScene ds = sc->dscene;
    ds.max_depth = plan.max_depth;
    const uint64_t n_pix = plan.pixels->size();
    LjStats &st = sc->stats; st = LjStats{};
    if (n_pix == 0) return;
    auto make_pass = [&](uint64_t p0, uint64_t np) {   // pixels [p0, p0 + np) of the list
        ljd::DPass pass{};
        pass.pixel_list = (const uint32_t *)ctx->pixel_list.p + p0; pass.n_pixels = (uint32_t)np; ljd::set_pass_divisors(pass, (uint32_t)plan.spp, (uint32_t)sc->flat.cam.width);
        pass.seed = plan.seed; pass.sample_rgb = (float *)ctx->sample_rgb.p;
        if (plan.n_views > 0) ljd::set_pass_views(pass, plan.views_dev, (uint32_t)sc->flat.cam.width, (uint32_t)sc->flat.cam.height);
        return pass;
    };
    if (sc->flat.integrator < LJ_INTEGRATOR_PATH) {   // auxiliary buffers: one primary ray per pixel, no queue
        if (samples_host) throw LjError(LJ_ERR_UNSUPPORTED, "the auxiliary integrators have one deterministic value per pixel, no per-sample values");
        upload_pixel_list(ctx, plan, stream);
        HIP_CHECK(hipEventRecord(ctx->ev_begin, stream));
        const int grid = (int)std::min<uint64_t>((n_pix + 255) / 256, (uint64_t)ctx->n_cus * 4);
        ljd::launch_aux(sc->dscene, make_pass(0, n_pix), (uint32_t)n_pix, sc->flat.integrator, rgb_dev, sc->ecfg,
                        ensure_spill(ctx, sc->ecfg.spill_levels, (uint32_t)grid), grid, stream);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipEventRecord(ctx->ev_end, stream));
        HIP_CHECK(hipEventSynchronize(ctx->ev_end));
        float ms = 0; HIP_CHECK(hipEventElapsedTime(&ms, ctx->ev_begin, ctx->ev_end));
        st.render_ms = ms; st.samples = n_pix; st.rays_closest = n_pix;
        return;
    }
    if (plan.rng_mode == LJ_RNG_TILE) { run_tiles(sc, plan, ds, rgb_dev, samples_host, stream); return; }   // (the auxiliary integrators draw nothing: as above)
    // pass size: keep the per-sample radiance buffer <= ~1.5 GiB and sample ids in 32 bits
    uint64_t max_samples_pass = (uint64_t)1 << 27;
    // (developer knob: small passes, so that a test can put a pass boundary anywhere — inside a view of a batch, say — at a small size)
    if (const char *e = getenv("LJ_TUNE_PASS_SAMPLES")) max_samples_pass = std::min<uint64_t>(max_samples_pass, (uint64_t)std::max(64ll, atoll(e)));
    uint64_t pix_per_pass = std::max<uint64_t>(1, max_samples_pass / (uint64_t)plan.spp);
    pix_per_pass = std::min<uint64_t>(pix_per_pass, n_pix);
    if (sc->flat.integrator == LJ_INTEGRATOR_VOLPATH) {   // volumetric path tracer: one lane per sample, whole path (dvol.h)
        const uint64_t pass_samples_max = pix_per_pass * (uint64_t)plan.spp;
        if (ctx->sample_rgb.bytes < pass_samples_max * 12) ctx->sample_rgb.alloc(pass_samples_max * 12);
        if (!ctx->chunk_counter.p) ctx->chunk_counter.alloc(128 * kMaxLanes);
        upload_pixel_list(ctx, plan, stream);
        HIP_CHECK(hipMemsetAsync(ctx->chunk_counter.p, 0, 256, stream));
        HIP_CHECK(hipEventRecord(ctx->ev_begin, stream));
        for (uint64_t p0 = 0; p0 < n_pix; p0 += pix_per_pass) {
            const uint64_t np = std::min<uint64_t>(pix_per_pass, n_pix - p0);
            const uint64_t total = np * (uint64_t)plan.spp;
            const ljd::DPass pass = make_pass(p0, np);
            // persistent grid (k_volpath regenerates paths): as many workgroups as stay resident, fewer for a small pass
            const int grid = (int)std::max<uint64_t>(1, std::min<uint64_t>((total + 255) / 256, (uint64_t)ctx->n_cus * (uint64_t)ljd::volpath_blocks_per_cu(ds)));
            HIP_CHECK(hipMemsetAsync((char *)ctx->chunk_counter.p + 8, 0, 4, stream));   // the launch's sample counter
            ljd::launch_volpath(ds, pass, (uint32_t)total, (uint32_t *)ctx->chunk_counter.p, sc->ecfg, sc->scfg.variant,
                                /* plain: */ (sc->feat_kinds & ~7u) == 0u && !sc->feat_textured && !sc->feat_envmap && !sc->feat_sphere_lights,
                                ensure_spill(ctx, sc->ecfg.spill_levels, (uint32_t)grid), grid, stream);
            HIP_CHECK(hipGetLastError());
            st.samples += total; st.wavefront_steps++;
            if (rgb_dev) ljd::launch_resolve(pass, (uint32_t)np, rgb_dev, stream);
            if (samples_host) {
                HIP_CHECK(hipMemcpyAsync(samples_host + p0 * (uint64_t)plan.spp * 3, ctx->sample_rgb.p, total * 12, hipMemcpyDeviceToHost, stream));
                HIP_CHECK(hipStreamSynchronize(stream));
            }
        }
        HIP_CHECK(hipEventRecord(ctx->ev_end, stream));
        HIP_CHECK(hipEventSynchronize(ctx->ev_end));
        float ms = 0; HIP_CHECK(hipEventElapsedTime(&ms, ctx->ev_begin, ctx->ev_end));
        unsigned long long nb = 0;
        HIP_CHECK(hipMemcpy(&nb, ctx->chunk_counter.p, 8, hipMemcpyDeviceToHost));
        st.render_ms = ms; st.bounce_iterations = nb;
        if (getenv("LJ_VOLPATH_STATS")) {   // developer build only (-DLJ_VOLPATH_STATS=1): events and lane-events per part of the tracer
            unsigned long long h[32];
            HIP_CHECK(hipMemcpy(h, ctx->chunk_counter.p, sizeof(h), hipMemcpyDeviceToHost));
            const char *names[8] = {"node iterations", "leaf steps", "closest calls", "tracking (bounce ray)", "tracking (shadow segment)", "shadow segments", "path steps", "-"};
            for (int k = 0; k < 7; k++) fprintf(stderr, "[volpath stats] %-26s wave events %12llu  lanes active %5.1f %%  per sample %.2f\n", names[k], h[2 + 2 * k], h[2 + 2 * k] ? 100.0 * h[3 + 2 * k] / (64.0 * h[2 + 2 * k]) : 0.0, (double)h[3 + 2 * k] / (double)st.samples);
        }
        return;
    }
    // ---- tiny scenes (flat leaf table, shading tables in LDS): the fused persistent kernel, one launch per pass (mega.hip)
    const size_t mega_lds = ljd::mega_smem(sc->dscene, sc->scfg);
    const bool mega_off = getenv("LJ_TUNE_MEGA") && atoi(getenv("LJ_TUNE_MEGA")) == 0;
    if (mega_lds > 0 && !mega_off) {
        const uint64_t pass_samples_max = pix_per_pass * (uint64_t)plan.spp;
        if (ctx->sample_rgb.bytes < pass_samples_max * 12) ctx->sample_rgb.alloc(pass_samples_max * 12);
        if (!ctx->mega_state.p) ctx->mega_state.alloc(64);
        upload_pixel_list(ctx, plan, stream);
        HIP_CHECK(hipEventRecord(ctx->ev_begin, stream));
        int per_cu = ljd::mega_blocks_per_cu(sc->dscene, sc->scfg);
        if (const char *e = getenv("LJ_TUNE_MEGA_BLOCKS_PER_CU")) per_cu = std::max(1, atoi(e));
        // camera samples a wave takes off the counter at a time: a multiple of 64 so that a wave's lanes share pixels, chosen so that
        // every wave draws ~16 times and the grid ends together — between 192 (below that the counter traffic shows) and 768:
        // the full bench frame 13.28 ms at 1024 per draw, 13.06 at 768; a 1/8 share of it (one rank of eight: tools/shard_time.py)
        // 2.50 ms at 1024, 2.00 at 192 (ideal 1.65)
        uint32_t grab_max = 768, grab_min = 192;
        bool grab_fixed = false;
        if (const char *e = getenv("LJ_TUNE_MEGA_GRAB")) { grab_max = (uint32_t)std::max(64, atoi(e)) & ~63u; grab_fixed = true; }
        double mega_ms = 0;
        unsigned long long hstats[5] = {};
        for (uint64_t p0 = 0; p0 < n_pix; p0 += pix_per_pass) {
            const uint64_t np = std::min<uint64_t>(pix_per_pass, n_pix - p0);
            const uint64_t total = np * (uint64_t)plan.spp;
            const ljd::DPass pass = make_pass(p0, np);
            HIP_CHECK(hipMemsetAsync(ctx->mega_state.p, 0, 64, stream));
            uint32_t grab = grab_max;
            if (!grab_fixed) {
                uint64_t draws = 16;
                if (const char *e = getenv("LJ_TUNE_MEGA_DRAWS")) draws = (uint64_t)std::max(1, atoi(e));
                const uint64_t waves = (uint64_t)ctx->n_cus * per_cu * 4, per_draw = total / (waves * draws);
                grab = (uint32_t)std::min<uint64_t>(grab_max, std::max<uint64_t>(grab_min, per_draw & ~(uint64_t)63));
            }
            // persistent grid: as many workgroups as stay resident, but no more waves than there are `grab`-sized pieces of work
            const uint64_t pieces = (total + grab - 1) / grab;
            const int grid = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)ctx->n_cus * per_cu, (pieces + 3) / 4));
            if (timing) HIP_CHECK(hipEventRecord(ctx->ev_k0, stream));
            ljd::launch_mega(ds, pass, sc->scfg, sc->flat.n_spheres > 0, (uint32_t)total, grab, (uint32_t *)ctx->mega_state.p,
                             (unsigned long long *)((char *)ctx->mega_state.p + 8), grid, stream);
            HIP_CHECK(hipGetLastError());
            if (timing) {
                HIP_CHECK(hipEventRecord(ctx->ev_k1, stream)); HIP_CHECK(hipEventSynchronize(ctx->ev_k1));
                float a = 0; HIP_CHECK(hipEventElapsedTime(&a, ctx->ev_k0, ctx->ev_k1)); mega_ms += a;
            }
            st.mega_launches++; st.wavefront_steps++;
            if (rgb_dev) ljd::launch_resolve(pass, (uint32_t)np, rgb_dev, stream);
            unsigned long long *h = ctx->stats_host;
            HIP_CHECK(hipMemcpyAsync(h, (char *)ctx->mega_state.p + 8, 5 * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
            if (samples_host) HIP_CHECK(hipMemcpyAsync(samples_host + p0 * (uint64_t)plan.spp * 3, ctx->sample_rgb.p, total * 12, hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipStreamSynchronize(stream));
            if (h[3] != total)
                throw LjError(LJ_ERR_INTERNAL, "mega launch ended with " + std::to_string(h[3]) + " of " + std::to_string(total) + " samples finished");
            for (int k = 0; k < 5; k++) hstats[k] += h[k];
            st.samples += total;
        }
        HIP_CHECK(hipEventRecord(ctx->ev_end, stream));
        HIP_CHECK(hipEventSynchronize(ctx->ev_end));
        float ms = 0; HIP_CHECK(hipEventElapsedTime(&ms, ctx->ev_begin, ctx->ev_end));
        st.render_ms = ms; st.mega_ms = mega_ms;
        st.bounce_iterations = hstats[0]; st.rays_closest = hstats[1]; st.rays_shadow = hstats[2]; st.path_steps = hstats[4];
        // algorithmic HBM bytes of a mega launch: the finished radiance of every sample (12 B) and its pixel's list entry — the path state
        // never leaves the registers
        st.mega_bytes = st.samples * 12ull + n_pix * 4ull;
        st.queue_bytes = st.mega_bytes;
        return;
    }
    // queue geometry: n_blocks workgroups x seg slots; workgroup b owns slots [b*seg, (b+1)*seg)
    const uint64_t pass_samples_max = pix_per_pass * (uint64_t)plan.spp;
    uint32_t pool = (uint32_t)std::min<uint64_t>(plan.pool, std::max<uint64_t>(pass_samples_max, 256));
    uint32_t blocks_per_cu = 8;
    if (const char *e = getenv("LJ_TUNE_BLOCKS_PER_CU")) blocks_per_cu = (uint32_t)std::max(1, atoi(e));
    // Lanes: the pool, its workgroup segments and the pass's samples are split into four parts that advance
    // independently on four streams.  The extend kernel is bound by VALU issue and moves few bytes, the shade kernel
    // streams the queue and leaves the VALUs mostly idle; with four staggered lanes the GPU always has some of each to
    // run side by side (two lanes: +13 % time on cbox; six or eight: worse again — more streams than hardware queues).
    // (One lane when kernels are timed individually or for tiny renders, two for small ones, or on request.)
    // developer instrumentation of the extend kernel (utilisation counters printed to stderr); off unless asked for
    unsigned long long *xstats = nullptr;
    DevBuf xstats_buf;
    if (getenv("LJ_EXTEND_STATS")) { xstats_buf.alloc(64); HIP_CHECK(hipMemsetAsync(xstats_buf.p, 0, 64, stream)); xstats = (unsigned long long *)xstats_buf.p; }
    uint32_t n_lanes = (timing || xstats || pool < (1u << 20)) ? 1u : (pool < (1u << 22) ? 2u : 4u);
    // the Disney / all-features shade kernels (164 VGPRs, three waves per SIMD) leave an extend kernel no registers to run beside
    // them: lanes would only time-slice the GPU (disney_bsdf 256 spp: 104 ms with one lane, 116 with two; a 64-spp render, which fits
    // the pool at once, is the other way round by 7 %)
    if (sc->scfg.variant >= 4) n_lanes = 1;   // (FeatDisney, FeatAll)
    // a tree beyond the LDS image (nodes fetched through L2): one lane.  Its extend launches fill every CU (five workgroups of 30 KiB
    // LDS and 92 VGPRs each), so the lanes' kernels queue up behind one another instead of running side by side (tools/lanes_sweep.sh,
    // sponza 256 spp: 202.5 ms with one lane, 208.8 with four)
    const bool large_tree = ds.n_nodes > sc->ecfg.lds_nodes;
    if (large_tree) n_lanes = 1;
    if (const char *e = getenv("LJ_TUNE_LANES")) n_lanes = (uint32_t)std::min((int)kMaxLanes, std::max(1, atoi(e)));
    uint32_t n_blocks = std::min<uint32_t>(kMaxBlocks, std::max<uint32_t>(n_lanes, std::min<uint32_t>((uint32_t)ctx->n_cus * blocks_per_cu, pool / 256)));
    n_blocks = (n_blocks / n_lanes) * n_lanes;
    const uint32_t lane_blocks = n_blocks / n_lanes;
    uint32_t seg = ((pool + n_blocks - 1) / n_blocks + 255u) & ~255u;
    const uint32_t n_slots = n_blocks * seg, lane_slots = lane_blocks * seg;
    ensure_queues(ctx, n_slots);
    // feature sets that sort a segment as a whole shade from one set of queue records into another (kernels.hip shade_sorted_segment)
    const bool sort_segments = ljd::shade_sorts_segments(sc->scfg);
    if (sort_segments) {
        const uint32_t cap = (n_slots + 63u) & ~63u;
        if (ctx->queue2_capacity < cap) { ctx->queue_mem2.alloc(queue_bytes(cap)); ctx->queue2_capacity = cap; }
        if (ctx->sort_perm.bytes < (size_t)cap * 4) ctx->sort_perm.alloc((size_t)cap * 4);
        if (ctx->sort_keys.bytes < (size_t)cap) ctx->sort_keys.alloc((size_t)cap);
    }
    // extend: persistent workgroups that draw 256-slot chunks of the queue.  One lane: more workgroups than fit at once, so
    // the hardware keeps every CU as full as registers and LDS allow; several lanes: few enough that the other lanes'
    // shade workgroups find registers beside them (8 extend waves per CU and lane).
    uint32_t ext_per_cu = n_lanes == 1 ? 8 : (n_lanes == 2 ? 4 : 2);
    if (const char *e = getenv("LJ_TUNE_EXTEND_BLOCKS_PER_CU")) ext_per_cu = (uint32_t)std::max(1, atoi(e));
    const uint32_t lane_chunks = lane_slots / 256u;
    const uint32_t ext_grid = std::max<uint32_t>(1, std::min<uint32_t>((uint32_t)ctx->n_cus * ext_per_cu, (lane_chunks + 3) / 4));
    // (the fused tail launches one workgroup per segment, so its overflow stacks are sized for the shade grid)
    // (not for a large tree: the tail's lane-by-lane traversal — one workgroup per segment, leaves tested unpooled — is slower there than
    // the extend / shade launches it replaces: tools/tail_sweep.sh, sponza 64 spp 60.4 -> 56.2 ms, disney_bsdf 256 spp 98.7 -> 97.2 without it)
    bool use_tail = !timing && !xstats && !large_tree && ljd::tail_smem(sc->ecfg, sc->scfg) > 0;
    if (const char *e = getenv("LJ_TUNE_TAIL")) use_tail = use_tail && atoi(e) != 0;
    uint64_t tail_num = 1, tail_den = 4;   // fuse once fewer than tail_num / tail_den of the slots hold a path
    if (const char *e = getenv("LJ_TUNE_TAIL_FRAC")) { tail_num = (uint64_t)std::max(1, atoi(e)); tail_den = 16; }
    const uint32_t spill_grid = std::max<uint32_t>(ext_grid, use_tail ? lane_blocks : 0u);
    int *spill_base = ensure_spill(ctx, sc->ecfg.spill_levels, spill_grid * n_lanes);
    // per lane: work[0] = the extend kernel's draw counter, work[1 + parity] = number of listed chunks; two chunk lists, used
    // alternately, so that a shade launch can append to one while nothing reads it
    if (!ctx->chunk_counter.p) ctx->chunk_counter.alloc(128 * kMaxLanes);
    if (ctx->chunk_list.bytes < (size_t)lane_chunks * 8 * n_lanes) ctx->chunk_list.alloc((size_t)lane_chunks * 8 * n_lanes);
    const ljd::DQueue q_all = carve_queue(ctx->queue_mem.p, ctx->queue_capacity);
    const ljd::DQueue q2_all = sort_segments ? carve_queue(ctx->queue_mem2.p, ctx->queue2_capacity) : q_all;
    struct Lane {
        hipStream_t stream; ljd::DQueue q, q2; uint32_t *sort_perm; uint8_t *sort_keys; ljd::DBlockState *dblocks; ljd::DBlockState *hblocks;
        uint32_t *work; uint32_t *lists[2]; uint32_t parity; int *spill; int *spill_tail; bool done; int batch;
    } lanes[kMaxLanes];
    for (uint32_t l = 0; l < n_lanes; l++) {
        Lane &L = lanes[l];
        L.stream = l == 0 ? stream : ctx->lane_streams[l - 1];
        const size_t o = (size_t)l * lane_slots;
        L.q = q_all; L.q.ro += o; L.q.rd += o; L.q.rs += o; L.q.rh += o; L.q.rw += o; L.q.rl += o; L.q.rn += o; L.q.rg += o;
        L.q2 = q2_all; L.q2.ro += o; L.q2.rd += o; L.q2.rs += o; L.q2.rh += o; L.q2.rw += o; L.q2.rl += o; L.q2.rn += o; L.q2.rg += o;
        L.sort_perm = sort_segments ? (uint32_t *)ctx->sort_perm.p + o : nullptr; L.sort_keys = sort_segments ? (uint8_t *)ctx->sort_keys.p + o : nullptr;
        L.dblocks = (ljd::DBlockState *)ctx->blocks.p + (size_t)l * lane_blocks; L.hblocks = ctx->blocks_host + (size_t)l * lane_blocks;
        L.work = (uint32_t *)ctx->chunk_counter.p + 32 * l;
        L.lists[0] = (uint32_t *)ctx->chunk_list.p + (size_t)l * 2 * lane_chunks; L.lists[1] = L.lists[0] + lane_chunks;
        L.spill = spill_base ? spill_base + (size_t)l * sc->ecfg.spill_levels * spill_grid * 256 : nullptr;
        L.spill_tail = L.spill;
    }
    if (ctx->sample_rgb.bytes < pass_samples_max * 12) ctx->sample_rgb.alloc(pass_samples_max * 12);
    upload_pixel_list(ctx, plan, stream);
    HIP_CHECK(hipEventRecord(ctx->ev_begin, stream));
    double extend_ms = 0, shade_ms = 0;
    for (uint64_t p0 = 0; p0 < n_pix; p0 += pix_per_pass) {
        const uint64_t np = std::min<uint64_t>(pix_per_pass, n_pix - p0);
        const uint64_t total = np * (uint64_t)plan.spp;
        const ljd::DPass pass = make_pass(p0, np);
        // contiguous sample ranges per workgroup, multiples of 64 so that a wave's first samples share a pixel
        {
            uint64_t per = ((total + n_blocks - 1) / n_blocks + 63) & ~(uint64_t)63;
            for (uint32_t b = 0; b < n_blocks; b++) {
                ljd::DBlockState bs{};
                uint64_t lo = std::min<uint64_t>(total, (uint64_t)b * per), hi = std::min<uint64_t>(total, (uint64_t)(b + 1) * per);
                bs.next_sample = (uint32_t)lo; bs.end_sample = (uint32_t)hi;
                ctx->blocks_host[b] = bs;
            }
            HIP_CHECK(hipMemcpyAsync(ctx->blocks.p, ctx->blocks_host, sizeof(ljd::DBlockState) * n_blocks, hipMemcpyHostToDevice, stream));
        }
        HIP_CHECK(hipMemsetAsync(ctx->chunk_counter.p, 0, 128 * kMaxLanes, stream));
        if (n_lanes > 1) {  // the second lane starts once the pass's inputs are in place
            HIP_CHECK(hipEventRecord(ctx->ev_fork, stream));
            for (uint32_t l = 1; l < n_lanes; l++) HIP_CHECK(hipStreamWaitEvent(ctx->lane_streams[l - 1], ctx->ev_fork, 0));
        }
        // step 0 is a shade over empty segments: it only generates camera rays
        for (uint32_t l = 0; l < n_lanes; l++) {
            Lane &L = lanes[l];
            L.parity = 0; L.done = false; L.batch = 8;  // steps per host round trip; all per-step state lives on the device
            // stagger: lane l starts when lane l-1 has generated its camera rays, so its shade launches fall on the other
            // lane's extend launches (the two lanes have equal work per step, so the phase offset persists)
            if (l > 0) HIP_CHECK(hipStreamWaitEvent(L.stream, ctx->ev_join, 0));
            ljd::launch_shade(ds, pass, L.q, L.q2, L.sort_perm, L.sort_keys, L.dblocks, lane_blocks, seg, sc->scfg, L.work, L.lists[0], 0, ext_grid * 4u, L.stream);
            if (sort_segments) std::swap(L.q, L.q2);   // (L.q: the set the paths are in now)
            if (l + 1 < n_lanes) HIP_CHECK(hipEventRecord(ctx->ev_join, L.stream));
        }
        // Round-robin over the lanes: look at a lane's block states only when its previous batch has drained, and give it
        // its next batch at once, so the other lane's kernels keep the GPU busy during this lane's host round trip.
        bool pending[kMaxLanes] = {};
        for (int guard = 0; guard < (1 << 21); guard++) {
            bool any = false;
            for (uint32_t l = 0; l < n_lanes; l++) {
                Lane &L = lanes[l];
                if (L.done) continue;
                if (pending[l]) {
                    HIP_CHECK(hipStreamSynchronize(L.stream));
                    pending[l] = false;
                    uint64_t alive = 0;
                    for (uint32_t b = 0; b < lane_blocks; b++) alive += L.hblocks[b].count;
                    L.done = alive == 0;
                    // the long tail (a few deep paths left): launches are nearly empty, so look less often
                    L.batch = alive * 64ull < (uint64_t)lane_slots ? 16 : 8;
                    if (L.done) continue;
                    // ... or not at all: once every camera sample has been started and the segments are mostly empty, the
                    // rest of the lane's paths finish inside one fused launch (k_tail)
                    uint64_t to_start = 0;
                    for (uint32_t b = 0; b < lane_blocks; b++) to_start += L.hblocks[b].end_sample - L.hblocks[b].next_sample;
                    if (use_tail && to_start == 0 && alive * tail_den < (uint64_t)lane_slots * tail_num) {
                        ljd::launch_tail(ds, pass, L.q, L.dblocks, lane_blocks, seg, sc->ecfg, sc->scfg, L.spill_tail, L.stream);
                        HIP_CHECK(hipGetLastError());
                        HIP_CHECK(hipMemcpyAsync(L.hblocks, L.dblocks, sizeof(ljd::DBlockState) * lane_blocks, hipMemcpyDeviceToHost, L.stream));
                        pending[l] = true; any = true;
                        continue;
                    }
                }
                any = true;
                for (int b = 0; b < L.batch; b++) {
                    if (timing) HIP_CHECK(hipEventRecord(ctx->ev_k0, L.stream));
                    ljd::launch_extend(ds, L.q, L.dblocks, ext_grid, seg, L.work, L.lists[L.parity], L.parity, sc->ecfg, L.spill, xstats, L.stream);
                    if (timing) HIP_CHECK(hipEventRecord(ctx->ev_k1, L.stream));
                    L.parity ^= 1u;
                    ljd::launch_shade(ds, pass, L.q, L.q2, L.sort_perm, L.sort_keys, L.dblocks, lane_blocks, seg, sc->scfg, L.work, L.lists[L.parity], L.parity, ext_grid * 4u, L.stream);
                    if (sort_segments) std::swap(L.q, L.q2);
                    if (timing) {
                        HIP_CHECK(hipEventRecord(ctx->ev_end, L.stream));
                        HIP_CHECK(hipEventSynchronize(ctx->ev_end));
                        float a = 0, c = 0;
                        HIP_CHECK(hipEventElapsedTime(&a, ctx->ev_k0, ctx->ev_k1)); HIP_CHECK(hipEventElapsedTime(&c, ctx->ev_k1, ctx->ev_end));
                        extend_ms += a; shade_ms += c;
                    }
                    st.extend_launches++; st.shade_launches++;
                    if (l == 0) st.wavefront_steps++;
                }
                HIP_CHECK(hipGetLastError());
                HIP_CHECK(hipMemcpyAsync(L.hblocks, L.dblocks, sizeof(ljd::DBlockState) * lane_blocks, hipMemcpyDeviceToHost, L.stream));
                pending[l] = true;
            }
            if (!any) break;
        }
        uint64_t samples_done = 0, path_steps = 0, shadow_rays = 0;
        for (uint32_t b = 0; b < n_blocks; b++) {
            const ljd::DBlockState &bs = ctx->blocks_host[b];
            samples_done += bs.samples_done; path_steps += bs.path_steps; shadow_rays += bs.rays_shadow;
            st.bounce_iterations += bs.bounce_iterations; st.rays_closest += bs.rays_closest; st.rays_shadow += bs.rays_shadow;
        }
        if (samples_done != total)
            throw LjError(LJ_ERR_INTERNAL, "wavefront loop ended with " + std::to_string(samples_done) + " of " + std::to_string(total) + " samples finished");
        st.samples += total;
        // algorithmic queue traffic per live path-step: extend reads ro, rd (32 B), rs (16 B) when a shadow ray
        // is pending, and writes rh (16 B); shade reads 7 records (112 B) and writes 7 (112 B), plus 12 B per finished sample
        st.path_steps += path_steps;
        st.extend_bytes += path_steps * 48ull + shadow_rays * 16ull;
        st.shade_bytes += path_steps * 224ull + total * 12ull;
        // (both lanes were synchronised with the host above, so the caller's stream may read what the second lane wrote)
        if (rgb_dev) ljd::launch_resolve(pass, (uint32_t)np, rgb_dev, stream);
        if (samples_host) {
            HIP_CHECK(hipMemcpyAsync(samples_host + p0 * (uint64_t)plan.spp * 3, ctx->sample_rgb.p, total * 12, hipMemcpyDeviceToHost, stream));
            HIP_CHECK(hipStreamSynchronize(stream));
        }
    }
    HIP_CHECK(hipEventRecord(ctx->ev_end, stream));
    HIP_CHECK(hipEventSynchronize(ctx->ev_end));
    float ms = 0; HIP_CHECK(hipEventElapsedTime(&ms, ctx->ev_begin, ctx->ev_end));
    st.render_ms = ms; st.extend_ms = extend_ms; st.shade_ms = shade_ms;
    if (xstats) {
        unsigned long long h[8];
        HIP_CHECK(hipMemcpy(h, xstats, 64, hipMemcpyDeviceToHost));
        fprintf(stderr, "[extend stats] rays %llu | outer iters %llu busy lanes %.1f%% | node steps %llu (%.2f/ray) lane use %.1f%% | prim rounds %llu (%.2f tests/ray) lane use %.1f%% | refills %llu\n",
                h[7], h[0], 100.0 * h[1] / (64.0 * h[0]), h[2], (double)h[3] / h[7], 100.0 * h[3] / (64.0 * h[2]), h[4], (double)h[5] / h[7], 100.0 * h[5] / (64.0 * h[4]), h[6]);
    }
    st.queue_bytes = st.extend_bytes + st.shade_bytes;
}

// The uploaded scenes of this process: lj_scene_update_geometry and lj_scene_read_bvh look a handle up before they touch it, so that a
// destroyed one is an error and not a use after free.
std::mutex g_live_mutex;
std::set<const lj_scene *> g_live_scenes;
bool scene_is_live(const lj_scene *sc) { std::lock_guard<std::mutex> lock(g_live_mutex); return sc && g_live_scenes.count(sc) != 0; }

} // namespace

extern "C" {

int lj_context_create(int device_id, lj_context **out) {
    return lj::guard([&]() {
        if (!out) throw LjError(LJ_ERR_INVALID_ARG, "lj_context_create: null out");
        *out = nullptr;
        int n = 0;
        hipError_t e = hipGetDeviceCount(&n);
        if (e != hipSuccess || n == 0) throw LjError(LJ_ERR_DEVICE, std::string("no HIP device available (") + hipGetErrorString(e) + "); this library has no CPU path");
        if (device_id < 0 || device_id >= n) throw LjError(LJ_ERR_INVALID_ARG, "device id out of range");
        auto ctx = std::make_unique<lj_context>();
        ctx->device = device_id;
        HIP_CHECK(hipSetDevice(device_id));
        hipDeviceProp_t prop; HIP_CHECK(hipGetDeviceProperties(&prop, device_id));
        if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
            throw LjError(LJ_ERR_DEVICE, std::string("device is ") + prop.gcnArchName + "; this build contains gfx950 code objects only");
        ctx->n_cus = prop.multiProcessorCount;
        HIP_CHECK(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
        for (auto &ls : ctx->lane_streams) HIP_CHECK(hipStreamCreateWithFlags(&ls, hipStreamNonBlocking));
        HIP_CHECK(hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming)); HIP_CHECK(hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming));
        HIP_CHECK(hipEventCreateWithFlags(&ctx->ev_caller, hipEventDisableTiming));
        ctx->blocks.alloc(sizeof(ljd::DBlockState) * kMaxBlocks);
        HIP_CHECK(hipHostMalloc((void **)&ctx->blocks_host, sizeof(ljd::DBlockState) * kMaxBlocks, hipHostMallocDefault));
        HIP_CHECK(hipHostMalloc((void **)&ctx->stats_host, 64, hipHostMallocDefault));
        HIP_CHECK(hipEventCreate(&ctx->ev_begin)); HIP_CHECK(hipEventCreate(&ctx->ev_end));
        HIP_CHECK(hipEventCreate(&ctx->ev_k0)); HIP_CHECK(hipEventCreate(&ctx->ev_k1));
        *out = ctx.release();
    });
}

void lj_context_destroy(lj_context *ctx) {
    if (!ctx) return;
    if (ctx->live_scenes > 0) { ctx->doomed = true; return; }   // released by the last lj_scene_destroy
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) { (void)hipStreamSynchronize(ctx->stream); (void)hipStreamDestroy(ctx->stream); }
    for (auto &ls : ctx->lane_streams) if (ls) { (void)hipStreamSynchronize(ls); (void)hipStreamDestroy(ls); }
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
    if (ctx->ev_caller) (void)hipEventDestroy(ctx->ev_caller);
    if (ctx->blocks_host) (void)hipHostFree(ctx->blocks_host);
    if (ctx->stats_host) (void)hipHostFree(ctx->stats_host);
    for (hipEvent_t e : {ctx->ev_begin, ctx->ev_end, ctx->ev_k0, ctx->ev_k1}) if (e) (void)hipEventDestroy(e);
    delete ctx;
}

int lj_scene_upload(lj_context *ctx, const LjSceneDesc *desc, lj_scene **out) {
    return lj::guard([&]() {
        if (!ctx || !desc || !out) throw LjError(LJ_ERR_INVALID_ARG, "lj_scene_upload: null argument");
        *out = nullptr;
        set_device(ctx);
        auto sc = std::make_unique<lj_scene>();
        sc->ctx = ctx;
        sc->flat = lj::flatten_scene(*desc);
        lj::FlatScene &F = sc->flat;
        hipStream_t s = ctx->stream;
        upload(sc->nodes, F.nodes, s);
        // BVH8 nodes: 80 bytes each; LJ_TUNE_NODE8_STRIDE=128 lays them out one per 128-byte cache line (a node then never straddles two lines)
        int node8_stride = (int)sizeof(ljd::DNode8);
        if (const char *e = getenv("LJ_TUNE_NODE8_STRIDE")) node8_stride = atoi(e) >= 128 ? 128 : 80;
        std::vector<unsigned char> nodes8_padded;
        if (node8_stride == (int)sizeof(ljd::DNode8)) upload(sc->nodes8, F.nodes8, s);
        else {
            nodes8_padded.assign(F.nodes8.size() * (size_t)node8_stride, 0);
            for (size_t i = 0; i < F.nodes8.size(); i++) memcpy(&nodes8_padded[i * (size_t)node8_stride], &F.nodes8[i], sizeof(ljd::DNode8));
            upload(sc->nodes8, nodes8_padded, s);
        }
        upload(sc->leaf_prims, F.leaf_prims, s); upload(sc->prims, F.prims, s); upload(sc->spheres, F.spheres, s);
        upload(sc->materials, F.materials, s); upload(sc->lights, F.lights, s); upload(sc->light_cdf, F.light_cdf, s);
        upload(sc->light_tris, F.light_tris, s); upload(sc->light_tri_cdf, F.light_tri_cdf, s);
        upload(sc->images3, F.images3, s); upload(sc->images1, F.images1, s); upload(sc->texels, F.texels, s); upload(sc->env_tables, F.env_tables, s);
        upload(sc->media, F.media, s); upload(sc->volume_data, F.volume_data, s); upload(sc->shape_media, F.shape_media, s);
        upload(sc->scan_leaves, F.scan_leaves, s);
        HIP_CHECK(hipStreamSynchronize(s));
        ljd::DScene d = F.host_view();
        d.nodes = (const ljd::DNode4 *)sc->nodes.p; d.nodes8 = (const ljd::DNode8 *)sc->nodes8.p; d.node8_stride = node8_stride; d.leaf_prims = (const ljd::DPrim *)sc->leaf_prims.p; d.prims = (const ljd::DPrimShade *)sc->prims.p;
        d.spheres = (const ljd::DSphere *)sc->spheres.p; d.materials = (const ljd::DMaterial *)sc->materials.p; d.lights = (const ljd::DLight *)sc->lights.p;
        d.light_cdf = (const float *)sc->light_cdf.p; d.light_tris = (const ljd::DLightTri *)sc->light_tris.p; d.light_tri_cdf = (const float *)sc->light_tri_cdf.p;
        d.images3 = (const ljd::DImage *)sc->images3.p; d.images1 = (const ljd::DImage *)sc->images1.p; d.texels = (const float *)sc->texels.p; d.env_tables = (const float *)sc->env_tables.p; d.env_marg = d.env_tables + F.env_marg_first;
        d.media = (const ljd::DMedium *)sc->media.p; d.volume_data = (const float *)sc->volume_data.p; d.shape_media = (const int32_t *)sc->shape_media.p;
        d.scan_leaves = F.scan_leaves.empty() ? nullptr : (const ljd::DScanLeaf *)sc->scan_leaves.p;
        sc->dscene = d;
        {   int64_t g = 0;
            for (int si = 0; si < desc->n_shapes; si++) { sc->shape_first_gprim.push_back(g); g += desc->shapes[si].kind == LJ_SHAPE_SPHERE ? 1 : desc->shapes[si].n_triangles; }
            sc->shape_first_gprim.push_back(g);
        }
        if (F.bvh_depth > ljd::max_stack_depth())
            throw LjError(LJ_ERR_INTERNAL, "BVH depth " + std::to_string(F.bvh_depth) + " exceeds the traversal stack");
        sc->ecfg = ljd::extend_config((int)F.nodes.size(), (int)F.leaf_prims.size(), F.bvh_depth, (int)F.n_spheres, (int)F.nodes8.size(), F.bvh8_depth, /* open scene: */ F.envmap_light_id >= 0);
        if (const char *e = getenv("LJ_TUNE_REFILL")) sc->ecfg.refill_min = (uint32_t)atoi(e);
        if (const char *e = getenv("LJ_TUNE_MINDESC")) sc->ecfg.min_descending = (uint32_t)atoi(e);
        sc->scfg = ljd::shade_config(F.prims.size(), F.materials.size(), F.lights.size(), F.light_tris.size(), F.light_tri_cdf.size(), F.images3.size(), F.images1.size(), (size_t)F.env_marg_count);
        {   // which Material / Texture / Light alternatives the scene holds decides the shade kernel instantiation
            uint32_t kinds = 0; bool textured = false, sphere_lights = false;
            for (const auto &m : F.materials) { kinds |= 1u << m.kind; for (int t = 0; t < 12; t++) textured = textured || m.tex[t].kind != 0; }
            for (const auto &l : F.lights) sphere_lights = sphere_lights || (l.kind == 0 && l.is_sphere);
            sc->feat_kinds = kinds; sc->feat_textured = textured; sc->feat_envmap = F.envmap_light_id >= 0; sc->feat_sphere_lights = sphere_lights;
            sc->scfg.variant = ljd::shade_variant(kinds, textured, F.envmap_light_id >= 0, sphere_lights);
            if (const char *e = getenv("LJ_TUNE_SHADE_VARIANT")) sc->scfg.variant = std::max(sc->scfg.variant, atoi(e));
            if (sc->scfg.smem == 0) sc->scfg.variant = ljd::kShadeVariantAll;   // tables too large to stage: one instantiation serves that case
        }
        ctx->live_scenes++;
        *out = sc.release();
        { std::lock_guard<std::mutex> lock(g_live_mutex); g_live_scenes.insert(*out); }
    });
}

void lj_scene_destroy(lj_scene *scene) {
    if (!scene) return;
    lj_context *ctx = scene->ctx;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    { std::lock_guard<std::mutex> lock(g_live_mutex); g_live_scenes.erase(scene); }
    delete scene;
    if (--ctx->live_scenes == 0 && ctx->doomed) lj_context_destroy(ctx);
}

int lj_render_device(lj_scene *scene, const LjRenderArgs *args, float *rgb_device, void *hip_stream) {
    return lj::guard([&]() {
        if (!scene || !rgb_device) throw LjError(LJ_ERR_INVALID_ARG, "lj_render_device: null argument");
        lj_context *ctx = scene->ctx;
        set_device(ctx);
        // The render always runs on the context's own streams — its lanes were created together and sit on distinct hardware
        // queues; a caller's stream created later may share a queue with one of them, which serialises two lanes (measured:
        // 26 -> 32 ms per cbox render) — and is ordered against the caller's stream by events on both sides.
        hipStream_t caller = (hipStream_t)hip_stream, s = ctx->stream;
        if (caller) { HIP_CHECK(hipEventRecord(ctx->ev_caller, caller)); HIP_CHECK(hipStreamWaitEvent(s, ctx->ev_caller, 0)); }
        RenderPlan plan = make_plan(scene, args);
        const size_t fb = (size_t)scene->flat.cam.width * scene->flat.cam.height * 3 * sizeof(float);
        HIP_CHECK(hipMemsetAsync(rgb_device, 0, fb, s));
        run_render(scene, plan, rgb_device, nullptr, s, args && (args->flags & 1u));
        if (caller) { HIP_CHECK(hipEventRecord(ctx->ev_caller, s)); HIP_CHECK(hipStreamWaitEvent(caller, ctx->ev_caller, 0)); }
    });
}

int lj_render(lj_scene *scene, const LjRenderArgs *args, float *rgb_host) {
    return lj::guard([&]() {
        if (!scene || !rgb_host) throw LjError(LJ_ERR_INVALID_ARG, "lj_render: null argument");
        lj_context *ctx = scene->ctx;
        set_device(ctx);
        const size_t fb = (size_t)scene->flat.cam.width * scene->flat.cam.height * 3 * sizeof(float);
        if (ctx->frame.bytes < fb) ctx->frame.alloc(fb);
        RenderPlan plan = make_plan(scene, args);
        HIP_CHECK(hipMemsetAsync(ctx->frame.p, 0, fb, ctx->stream));
        run_render(scene, plan, (float *)ctx->frame.p, nullptr, ctx->stream, args && (args->flags & 1u));
        HIP_CHECK(hipMemcpyAsync(rgb_host, ctx->frame.p, fb, hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
    });
}

int lj_scene_set_camera(lj_scene *scene, const LjCamera *camera) {
    return lj::guard([&]() {
        if (!scene || !camera) throw LjError(LJ_ERR_INVALID_ARG, "lj_scene_set_camera: null argument");
        lj::check_camera(*camera);
        lj::FlatScene &F = scene->flat;
        if (camera->medium_id < -1 || camera->medium_id >= (int)F.media.size()) throw LjError(LJ_ERR_INVALID_ARG, "camera references a missing medium");
        const bool resized = camera->width != F.cam.width || camera->height != F.cam.height;
        F.cam = lj::flatten_camera(*camera); F.cam_medium = camera->medium_id;
        // what a DScene holds of the camera, from the code that fills it at upload
        const ljd::DScene h = F.host_view();
        scene->dscene.cam = h.cam; scene->dscene.init_spread = h.init_spread; scene->dscene.cam_medium = h.cam_medium;
        if (resized) { scene->plan_pixels.reset(); scene->plan_pixels_key = 0; scene->views_pixels.reset(); scene->views_pixels_key = 0; }   // lists of the old film
    });
}

int lj_scene_update_geometry(lj_scene *scene, const LjSceneDesc *desc) {
    return lj::guard([&]() {
        if (!scene || !desc) throw LjError(LJ_ERR_INVALID_ARG, "lj_scene_update_geometry: null argument");
        if (!scene_is_live(scene)) throw LjError(LJ_ERR_INVALID_ARG, "lj_scene_update_geometry: not an uploaded scene (destroyed?)");
        const auto t0 = std::chrono::steady_clock::now();
        lj::FlatScene &F = scene->flat;
        // ---- host: every check, and everything lj_scene_upload derives from positions.  Nothing of the scene is touched before this returns.
        lj::FlatScene U = lj::flatten_update(F, *desc);
        auto same = [](size_t a, size_t b) { if (a != b) throw LjError(LJ_ERR_INTERNAL, "lj_scene_update_geometry: a re-derived table changed its size"); };
        same(U.leaf_prims.size(), F.leaf_prims.size()); same(U.prims.size(), F.prims.size()); same(U.spheres.size(), F.spheres.size()); same(U.lights.size(), F.lights.size());
        same(U.light_cdf.size(), F.light_cdf.size()); same(U.light_tris.size(), F.light_tris.size()); same(U.light_tri_cdf.size(), F.light_tri_cdf.size());
        const double host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        lj_context *ctx = scene->ctx;
        set_device(ctx);
        hipStream_t s = ctx->stream;
        const size_t bb = ljd::refit_box_bytes();
        if (!scene->refit_box4.p) {
            scene->refit_box4.alloc(std::max<size_t>(F.nodes.size(), 1) * bb); scene->refit_box8.alloc(std::max<size_t>(F.nodes8.size(), 1) * bb);
            upload(scene->refit_levels4, F.levels4, s); upload(scene->refit_levels8, F.levels8, s);
        }
        // ---- device, in stream order: the tables, then the boxes of the three structures from the new leaf-ordered primitives
        HIP_CHECK(hipEventRecord(ctx->ev_begin, s));
        auto put = [&](DevBuf &b, const auto &v) { HIP_CHECK(hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(v[0]), hipMemcpyHostToDevice, s)); };
        put(scene->leaf_prims, U.leaf_prims); put(scene->prims, U.prims); put(scene->spheres, U.spheres); put(scene->light_tris, U.light_tris);
        put(scene->light_tri_cdf, U.light_tri_cdf); put(scene->lights, U.lights); put(scene->light_cdf, U.light_cdf);
        const ljd::DPrim *lp = (const ljd::DPrim *)scene->leaf_prims.p; const ljd::DSphere *sp = (const ljd::DSphere *)scene->spheres.p;
        if (!F.scan_leaves.empty()) ljd::launch_refit_scan((ljd::DScanLeaf *)scene->scan_leaves.p, lp, sp, F.n_scan_used, s);
        for (size_t l = F.level4_first.size() - 1; l-- > 0;)
            ljd::launch_refit4((ljd::DNode4 *)scene->nodes.p, scene->refit_box4.p, lp, sp, (const int32_t *)scene->refit_levels4.p + F.level4_first[l], F.level4_first[l + 1] - F.level4_first[l], s);
        const int stride8 = scene->dscene.node8_stride;
        for (size_t l = F.level8_first.size() - 1; l-- > 0;)
            ljd::launch_refit8(scene->nodes8.p, stride8, scene->refit_box8.p, lp, sp, (const int32_t *)scene->refit_levels8.p + F.level8_first[l], F.level8_first[l + 1] - F.level8_first[l], s);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipEventRecord(ctx->ev_end, s));
        // the host copy of the nodes follows the device's (lj_scene_info and the tests read it)
        HIP_CHECK(hipMemcpyAsync(F.nodes.data(), scene->nodes.p, F.nodes.size() * sizeof(ljd::DNode4), hipMemcpyDeviceToHost, s));
        if (stride8 == (int)sizeof(ljd::DNode8)) HIP_CHECK(hipMemcpyAsync(F.nodes8.data(), scene->nodes8.p, F.nodes8.size() * sizeof(ljd::DNode8), hipMemcpyDeviceToHost, s));
        else HIP_CHECK(hipMemcpy2DAsync(F.nodes8.data(), sizeof(ljd::DNode8), scene->nodes8.p, (size_t)stride8, sizeof(ljd::DNode8), F.nodes8.size(), hipMemcpyDeviceToHost, s));
        if (!F.scan_leaves.empty()) HIP_CHECK(hipMemcpyAsync(F.scan_leaves.data(), scene->scan_leaves.p, F.scan_leaves.size() * sizeof(ljd::DScanLeaf), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        float ms = 0; HIP_CHECK(hipEventElapsedTime(&ms, ctx->ev_begin, ctx->ev_end));
        lj::commit_update(F, std::move(U));
        scene->dscene.eps = (float)F.shadow_epsilon;
        // LjStats of an update: render_ms = device time (copies of the tables and the refit launches), generate_ms = host time of the re-derivation
        scene->stats = LjStats{}; scene->stats.render_ms = ms; scene->stats.generate_ms = host_ms;
    });
}

int lj_scene_read_bvh(const lj_scene *scene, int32_t which, void *out_host, int64_t capacity_bytes, int64_t *bytes) {
    return lj::guard([&]() {
        if (!scene || !bytes) throw LjError(LJ_ERR_INVALID_ARG, "lj_scene_read_bvh: null argument");
        if (!scene_is_live(scene)) throw LjError(LJ_ERR_INVALID_ARG, "lj_scene_read_bvh: not an uploaded scene (destroyed?)");
        if (which < 0 || which > 2) throw LjError(LJ_ERR_INVALID_ARG, "lj_scene_read_bvh: which must be 0 (DNode4), 1 (DNode8) or 2 (DScanLeaf)");
        const lj::FlatScene &F = scene->flat;
        const size_t n = which == 0 ? F.nodes.size() : which == 1 ? F.nodes8.size() : F.scan_leaves.size();
        const size_t rec = which == 0 ? sizeof(ljd::DNode4) : which == 1 ? sizeof(ljd::DNode8) : sizeof(ljd::DScanLeaf);
        *bytes = (int64_t)(n * rec);
        if (!out_host) return;   // (a size query)
        if (capacity_bytes < *bytes) throw LjError(LJ_ERR_INVALID_ARG, "lj_scene_read_bvh: buffer too small");
        if (n == 0) return;
        lj_context *ctx = scene->ctx;
        set_device(ctx);
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        const void *src = which == 0 ? scene->nodes.p : which == 1 ? scene->nodes8.p : scene->scan_leaves.p;
        const size_t pitch = which == 1 ? (size_t)scene->dscene.node8_stride : rec;
        if (pitch == rec) HIP_CHECK(hipMemcpy(out_host, src, n * rec, hipMemcpyDeviceToHost));
        else HIP_CHECK(hipMemcpy2D(out_host, rec, src, pitch, rec, n, hipMemcpyDeviceToHost));
    });
}

static void render_views(lj_scene *scene, const LjRenderArgs *args, int32_t n_views, const LjCamera *views, float *rgb_host, float *rgb_device, hipStream_t caller, const char *who) {
    if (!scene || !views || (!rgb_host && !rgb_device)) throw LjError(LJ_ERR_INVALID_ARG, std::string(who) + ": null argument");
    if (n_views <= 0) throw LjError(LJ_ERR_INVALID_ARG, std::string(who) + ": n_views must be positive");
    const lj::FlatScene &F = scene->flat;
    const uint64_t view_pixels = (uint64_t)F.cam.width * (uint64_t)F.cam.height;
    if ((uint64_t)n_views * view_pixels > (1ull << 31)) throw LjError(LJ_ERR_INVALID_ARG, std::string(who) + ": more than 2^31 pixels in the batch");
    std::vector<ljd::DCamera> table((size_t)n_views);
    for (int v = 0; v < n_views; v++) {
        lj::check_camera(views[v]);
        table[v] = lj::flatten_camera(views[v]);
        if (table[v].width != F.cam.width || table[v].height != F.cam.height || table[v].filter_kind != F.cam.filter_kind || table[v].filter_param != F.cam.filter_param ||
            views[v].medium_id != F.cam_medium)
            throw LjError(LJ_ERR_INVALID_ARG, std::string(who) + ": view " + std::to_string(v) + " differs from the scene camera in film size, filter or medium");
    }
    lj_context *ctx = scene->ctx;
    set_device(ctx);
    RenderPlan plan = make_views_plan(scene, args, n_views);
    hipStream_t s = ctx->stream;
    if (caller) { HIP_CHECK(hipEventRecord(ctx->ev_caller, caller)); HIP_CHECK(hipStreamWaitEvent(s, ctx->ev_caller, 0)); }   // (as lj_render_device)
    const size_t table_bytes = table.size() * sizeof(ljd::DCamera);
    if (ctx->view_table.bytes < table_bytes) ctx->view_table.alloc(table_bytes);
    HIP_CHECK(hipMemcpyAsync(ctx->view_table.p, table.data(), table_bytes, hipMemcpyHostToDevice, s));
    plan.views_dev = (const ljd::DCamera *)ctx->view_table.p;
    const size_t fb = (size_t)n_views * view_pixels * 3 * sizeof(float);
    float *frame = rgb_device;
    if (!frame) { if (ctx->frame.bytes < fb) ctx->frame.alloc(fb); frame = (float *)ctx->frame.p; }
    HIP_CHECK(hipMemsetAsync(frame, 0, fb, s));
    run_render(scene, plan, frame, nullptr, s, args && (args->flags & 1u));
    if (rgb_host) { HIP_CHECK(hipMemcpyAsync(rgb_host, frame, fb, hipMemcpyDeviceToHost, s)); HIP_CHECK(hipStreamSynchronize(s)); }
    if (caller) { HIP_CHECK(hipEventRecord(ctx->ev_caller, s)); HIP_CHECK(hipStreamWaitEvent(caller, ctx->ev_caller, 0)); }
}

int lj_render_views(lj_scene *scene, const LjRenderArgs *args, int32_t n_views, const LjCamera *views, float *rgb_host) {
    return lj::guard([&]() { render_views(scene, args, n_views, views, rgb_host, nullptr, nullptr, "lj_render_views"); });
}

int lj_render_views_device(lj_scene *scene, const LjRenderArgs *args, int32_t n_views, const LjCamera *views, float *rgb_device, void *hip_stream) {
    return lj::guard([&]() { render_views(scene, args, n_views, views, nullptr, rgb_device, (hipStream_t)hip_stream, "lj_render_views_device"); });
}

int lj_render_samples(lj_scene *scene, const LjRenderArgs *args, float *radiance_host) {
    return lj::guard([&]() {
        if (!scene || !radiance_host || !args) throw LjError(LJ_ERR_INVALID_ARG, "lj_render_samples: null argument");
        if (!(args->crop_x1 > args->crop_x0 && args->crop_y1 > args->crop_y0)) throw LjError(LJ_ERR_INVALID_ARG, "lj_render_samples needs a crop window");
        if (args->world_size > 1) throw LjError(LJ_ERR_INVALID_ARG, "lj_render_samples is single-rank");
        set_device(scene->ctx);
        RenderPlan plan = make_plan(scene, args);
        run_render(scene, plan, nullptr, radiance_host, scene->ctx->stream, false);
    });
}

static int trace_batch(lj_scene *scene, int64_t n, const LjRay *rays_host, LjHit *hits_host, uint8_t *occ_host) {
    return lj::guard([&]() {
        if (!scene || !rays_host || n < 0) throw LjError(LJ_ERR_INVALID_ARG, "trace: bad argument");
        if (n == 0) return;
        lj_context *ctx = scene->ctx;
        set_device(ctx);
        DevBuf rays, out;
        rays.alloc((size_t)n * sizeof(LjRay));
        out.alloc((size_t)n * (hits_host ? sizeof(LjHit) : 1));
        HIP_CHECK(hipMemcpyAsync(rays.p, rays_host, (size_t)n * sizeof(LjRay), hipMemcpyHostToDevice, ctx->stream));
        int grid = (int)std::min<int64_t>((n + 255) / 256, ctx->n_cus * 4);
        // a tiny scene is traced by the leaf scan of mega.hip in a render, so that is what answers here too (LJ_TUNE_MEGA=0: the BVH
        // traversal of k_extend, as for every other scene)
        const bool scan = scene->dscene.n_scan_leaves > 0 && !(getenv("LJ_TUNE_MEGA") && atoi(getenv("LJ_TUNE_MEGA")) == 0);
        HIP_CHECK(hipEventRecord(ctx->ev_begin, ctx->stream));
        if (scan) ljd::launch_trace_rays_scan(scene->dscene, rays.p, n, hits_host ? out.p : nullptr, hits_host ? nullptr : (unsigned char *)out.p, grid, ctx->stream);
        else ljd::launch_trace_rays(scene->dscene, rays.p, n, hits_host ? out.p : nullptr, hits_host ? nullptr : (unsigned char *)out.p, scene->ecfg, ensure_spill(ctx, scene->ecfg.spill_levels, (uint32_t)grid), grid, ctx->stream);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipEventRecord(ctx->ev_end, ctx->stream));
        if (hits_host) HIP_CHECK(hipMemcpyAsync(hits_host, out.p, (size_t)n * sizeof(LjHit), hipMemcpyDeviceToHost, ctx->stream));
        else HIP_CHECK(hipMemcpyAsync(occ_host, out.p, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        float ms = 0; HIP_CHECK(hipEventElapsedTime(&ms, ctx->ev_begin, ctx->ev_end));
        scene->stats = LjStats{}; scene->stats.render_ms = ms; scene->stats.rays_closest = hits_host ? (uint64_t)n : 0; scene->stats.rays_shadow = hits_host ? 0 : (uint64_t)n;   // (the query kernel's device time)
        if (scan) scene->stats.mega_launches = 1; else scene->stats.extend_launches = 1;   // which route answered: the leaf scan of mega.hip or the BVH traversal
    });
}
int lj_intersect(lj_scene *scene, int64_t n, const LjRay *rays_host, LjHit *hits_host) {
    if (!hits_host) { lj::set_last_error("lj_intersect: null output"); return LJ_ERR_INVALID_ARG; }
    return trace_batch(scene, n, rays_host, hits_host, nullptr);
}
int lj_occluded(lj_scene *scene, int64_t n, const LjRay *rays_host, uint8_t *occluded_host) {
    if (!occluded_host) { lj::set_last_error("lj_occluded: null output"); return LJ_ERR_INVALID_ARG; }
    return trace_batch(scene, n, rays_host, nullptr, occluded_host);
}

int lj_get_stats(const lj_scene *scene, LjStats *out) {
    if (!scene || !out) { lj::set_last_error("lj_get_stats: null argument"); return LJ_ERR_INVALID_ARG; }
    *out = scene->stats;
    return LJ_OK;
}

int lj_scene_info(const lj_scene *scene, LjSceneInfo *out) {
    if (!scene || !out) { lj::set_last_error("lj_scene_info: null argument"); return LJ_ERR_INVALID_ARG; }
    const lj::FlatScene &F = scene->flat;
    LjSceneInfo i{};
    i.width = F.cam.width; i.height = F.cam.height; i.spp = F.spp; i.max_depth = F.max_depth; i.rr_depth = F.rr_depth; i.integrator = F.integrator;
    i.n_triangles = F.n_triangles; i.n_spheres = F.n_spheres; i.n_bvh_nodes = (int64_t)F.nodes.size();
    i.bounds_radius = F.bounds_radius; for (int k = 0; k < 3; k++) i.bounds_center[k] = F.bounds_center[k];
    i.shadow_epsilon = F.shadow_epsilon;
    *out = i;
    return LJ_OK;
}

} // extern "C"
