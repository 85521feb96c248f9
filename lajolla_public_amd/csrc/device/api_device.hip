// C-ABI entry points that own the GPU, the base family: context and scene lifetime, lj_scene_upload with install_trees, lj_scene_set_camera,
// lj_scene_info, lj_get_stats, lj_scene_read_bvh, the plain render entry points (lj_render, _device, _samples, _views*) over render_frames,
// and the batched ray queries (trace_batch).  The other families live beside this file: api_geometry.hip, api_film.hip, api_denoise.hip and
// api_rays.hip; what they all render with (render plans, run_render and its five drivers) lives in render.hip.
// One context = one HIP device + one stream; one process per GPU (the multi-GPU layer above this is
// torch.distributed over RCCL, see bench.py).  Every HIP call is checked; failures surface as LJ_ERR_DEVICE with
// the HIP error string — there is no CPU fallback behind any of these functions.
#include "api_calls.h"
#include <mutex>
#include <set>

// The uploaded scenes of this process: lj_scene_update_geometry, the rebuilds and lj_scene_read_bvh look a handle up before they touch it, so
// that a destroyed one is an error and not a use after free.
static std::mutex g_live_mutex;
static std::set<const lj_scene *> g_live_scenes;
bool scene_is_live(const lj_scene *sc) { std::lock_guard<std::mutex> lock(g_live_mutex); return sc && g_live_scenes.count(sc) != 0; }

// One render of a plan, all its views, into up to six frames: the image and the five of a features request (dst[1..5]: albedo, normal, depth,
// alpha, variance; all null in the plain entry points, whose render is then exactly the plan's).  on_device: dst are the caller's device
// frames; else host buffers, filled through the context's workspace, from which only those asked for are copied back.
// `views`: the camera table of a batch, uploaded for this render (empty: the scene's own camera).
// The render always runs on the context's own streams — its lanes were created together and sit on distinct hardware
// queues; a caller's stream created later may share a queue with one of them, which serialises two lanes (measured:
// 26 -> 32 ms per cbox render) — and is ordered against the caller's stream by events on both sides.
// The render entry points order against a stream that was given and not against the null stream: a host variant passes none and waits
// for the context's stream itself before it returns (what a device variant handed the null stream is left with: DESIGN.md §3.12).
void render_frames(lj_scene *scene, RenderPlan plan, const std::vector<ljd::DCamera> &views, float *const dst[6], bool on_device, hipStream_t caller, bool timing) {
    lj_context *ctx = scene->ctx;
    hipStream_t s = enter_from_caller(ctx, caller, caller != nullptr);
    upload_view_table(ctx, views, plan, s);
    const size_t n_pix = (size_t)std::max(plan.n_views, 1) * scene->flat.cam.width * scene->flat.cam.height;
    const size_t chan[6] = {3, 3, 3, 1, 1, 3};
    float *frame[6] = {};
    if (on_device) for (int k = 0; k < 6; k++) frame[k] = dst[k];
    else { stage_frames(dst, chan, 0, 1, n_pix, ctx->frame, frame); stage_frames(dst, chan, 1, 6, n_pix, ctx->feature_frames, frame); }
    for (int k = 0; k < 6; k++) if (frame[k]) HIP_CHECK(hipMemsetAsync(frame[k], 0, n_pix * chan[k] * sizeof(float), s));
    plan.feat.albedo = frame[1]; plan.feat.normal = frame[2]; plan.feat.depth = frame[3]; plan.feat.alpha = frame[4]; plan.feat.variance = frame[5];
    plan.feat.want = (frame[1] ? ljd::FEAT_ALBEDO : 0u) | (frame[2] ? ljd::FEAT_NORMAL : 0u) | (frame[3] ? ljd::FEAT_DEPTH : 0u) | (frame[4] ? ljd::FEAT_ALPHA : 0u) | (frame[5] ? ljd::FEAT_VARIANCE : 0u);
    run_render(scene, plan, frame[0], nullptr, s, timing);
    if (!on_device) fetch_frames(dst, frame, chan, 0, 6, n_pix, s);
    leave_to_caller(ctx, caller, caller != nullptr);
}
// the image alone, into the caller's device memory or a host buffer
static void render_frame(lj_scene *scene, const RenderPlan &plan, const std::vector<ljd::DCamera> &views, float *rgb_host, float *rgb_device, hipStream_t caller, bool timing) {
    float *const dst[6] = {rgb_device ? rgb_device : rgb_host};
    render_frames(scene, plan, views, dst, rgb_device != nullptr, caller, timing);
}

// The trees of scene->flat onto the device, for lj_scene_upload and lj_scene_rebuild_bvh alike: the nodes of both trees (LJ_TUNE_NODE8_STRIDE
// read here) and the leaf-ordered primitives, what the DScene holds of them, the depth check, and the extend kernels' launch plan with its
// two overrides.  scene->dscene holds everything else already.  Returns with the copies done.
void install_trees(lj_scene *sc, hipStream_t s) {
    lj::FlatScene &F = sc->flat;
    if (F.bvh_depth > ljd::max_stack_depth())
        throw LjError(LJ_ERR_INTERNAL, "BVH depth " + std::to_string(F.bvh_depth) + " exceeds the traversal stack");
    upload(sc->nodes, F.nodes, s);
    // BVH8 nodes: 80 bytes each; LJ_TUNE_NODE8_STRIDE=128 lays them out one per 128-byte cache line (a node then never straddles two lines)
    const int node8_stride = env_int("LJ_TUNE_NODE8_STRIDE", 0) >= 128 ? 128 : (int)sizeof(ljd::DNode8);
    std::vector<unsigned char> nodes8_padded;
    if (node8_stride == (int)sizeof(ljd::DNode8)) upload(sc->nodes8, F.nodes8, s);
    else {
        nodes8_padded.assign(F.nodes8.size() * (size_t)node8_stride, 0);
        for (size_t i = 0; i < F.nodes8.size(); i++) memcpy(&nodes8_padded[i * (size_t)node8_stride], &F.nodes8[i], sizeof(ljd::DNode8));
        upload(sc->nodes8, nodes8_padded, s);
    }
    upload(sc->leaf_prims, F.leaf_prims, s);
    HIP_CHECK(hipStreamSynchronize(s));
    ljd::DScene &d = sc->dscene;
    d.nodes = (const ljd::DNode4 *)sc->nodes.p; d.n_nodes = (int32_t)F.nodes.size();
    d.nodes8 = (const ljd::DNode8 *)sc->nodes8.p; d.n_nodes8 = (int32_t)F.nodes8.size(); d.node8_stride = node8_stride;
    d.leaf_prims = (const ljd::DPrim *)sc->leaf_prims.p; d.n_prims = (int32_t)F.leaf_prims.size();
    sc->ecfg = ljd::extend_config((int)F.nodes.size(), (int)F.leaf_prims.size(), F.bvh_depth, (int)F.n_spheres, (int)F.nodes8.size(), F.bvh8_depth, /* open scene: */ F.envmap_light_id >= 0);
    sc->ecfg.refill_min = (uint32_t)env_int("LJ_TUNE_REFILL", (int)sc->ecfg.refill_min);
    sc->ecfg.min_descending = (uint32_t)env_int("LJ_TUNE_MINDESC", (int)sc->ecfg.min_descending);
}

// the camera table of a batch, every view checked against the scene's camera
std::vector<ljd::DCamera> view_table(const lj_scene *scene, int32_t n_views, const LjCamera *views, const std::string &me) {
    const lj::FlatScene &F = scene->flat;
    const uint64_t view_pixels = (uint64_t)F.cam.width * (uint64_t)F.cam.height;
    if ((uint64_t)n_views * view_pixels > (1ull << 31)) throw LjError(LJ_ERR_INVALID_ARG, me + ": more than 2^31 pixels in the batch");
    std::vector<ljd::DCamera> table((size_t)n_views);
    for (int v = 0; v < n_views; v++) {
        lj::check_camera(views[v]);
        table[v] = lj::flatten_camera(views[v]);
        if (table[v].width != F.cam.width || table[v].height != F.cam.height || table[v].filter_kind != F.cam.filter_kind || table[v].filter_param != F.cam.filter_param ||
            views[v].medium_id != F.cam_medium)
            throw LjError(LJ_ERR_INVALID_ARG, me + ": view " + std::to_string(v) + " differs from the scene camera in film size, filter or medium");
    }
    return table;
}

static void render_views(lj_scene *scene, const LjRenderArgs *args, int32_t n_views, const LjCamera *views, float *rgb_host, float *rgb_device, hipStream_t caller, const std::string &me) {
    if (!scene || !views || (!rgb_host && !rgb_device)) throw LjError(LJ_ERR_INVALID_ARG, me + ": null argument");
    if (n_views <= 0) throw LjError(LJ_ERR_INVALID_ARG, me + ": n_views must be positive");
    const std::vector<ljd::DCamera> table = view_table(scene, n_views, views, me);
    render_frame(scene, make_views_plan(scene, args, n_views), table, rgb_host, rgb_device, caller, timing_requested(args));
}

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
        for (auto ev : kTimingEvents) HIP_CHECK(hipEventCreate(&(ctx.get()->*ev)));
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
    for (auto ev : kTimingEvents) if (ctx->*ev) (void)hipEventDestroy(ctx->*ev);
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
        upload(sc->prims, F.prims, s); upload(sc->spheres, F.spheres, s);
        upload(sc->materials, F.materials, s); upload(sc->lights, F.lights, s); upload(sc->light_cdf, F.light_cdf, s);
        upload(sc->light_tris, F.light_tris, s); upload(sc->light_tri_cdf, F.light_tri_cdf, s);
        upload(sc->images3, F.images3, s); upload(sc->images1, F.images1, s); upload(sc->texels, F.texels, s); upload(sc->env_tables, F.env_tables, s);
        upload(sc->media, F.media, s); upload(sc->volume_data, F.volume_data, s); upload(sc->shape_media, F.shape_media, s);
        upload(sc->scan_leaves, F.scan_leaves, s);
        HIP_CHECK(hipStreamSynchronize(s));
        ljd::DScene d = F.host_view();
        d.prims = (const ljd::DPrimShade *)sc->prims.p;
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
        install_trees(sc.get(), s);
        sc->scfg = ljd::shade_config(F.prims.size(), F.materials.size(), F.lights.size(), F.light_tris.size(), F.light_tri_cdf.size(), F.images3.size(), F.images1.size(), (size_t)F.env_marg_count);
        {   // which Material / Texture / Light alternatives the scene holds decides the shade kernel instantiation
            uint32_t kinds = 0; bool textured = false, sphere_lights = false;
            for (const auto &m : F.materials) { kinds |= 1u << m.kind; for (int t = 0; t < 12; t++) textured = textured || m.tex[t].kind != 0; }
            for (const auto &l : F.lights) sphere_lights = sphere_lights || (l.kind == 0 && l.is_sphere);
            sc->feat_kinds = kinds; sc->feat_textured = textured; sc->feat_envmap = F.envmap_light_id >= 0; sc->feat_sphere_lights = sphere_lights;
            // (LJ_TUNE_SHADE_VARIANT: a larger feature set than the scene needs, taken only if it covers the scene)
            sc->scfg.variant = ljd::shade_variant(kinds, textured, F.envmap_light_id >= 0, sphere_lights, env_int("LJ_TUNE_SHADE_VARIANT", -1));
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
        render_frame(scene, make_plan(scene, args), {}, nullptr, rgb_device, (hipStream_t)hip_stream, timing_requested(args));
    });
}

int lj_render(lj_scene *scene, const LjRenderArgs *args, float *rgb_host) {
    return lj::guard([&]() {
        if (!scene || !rgb_host) throw LjError(LJ_ERR_INVALID_ARG, "lj_render: null argument");
        render_frame(scene, make_plan(scene, args), {}, rgb_host, nullptr, nullptr, timing_requested(args));
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
        run_render(scene, make_plan(scene, args), nullptr, radiance_host, scene->ctx->stream, false);
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
        const bool scan = scene->dscene.n_scan_leaves > 0 && mega_enabled();
        HIP_CHECK(hipEventRecord(ctx->ev_begin, ctx->stream));
        if (scan) ljd::launch_trace_rays_scan(scene->dscene, rays.p, n, hits_host ? out.p : nullptr, hits_host ? nullptr : (unsigned char *)out.p, mega_item_cap_tune(), grid, ctx->stream);
        else ljd::launch_trace_rays(scene->dscene, rays.p, n, hits_host ? out.p : nullptr, hits_host ? nullptr : (unsigned char *)out.p, scene->ecfg, ensure_spill(ctx, scene->ecfg.spill_levels, (uint32_t)grid), grid, ctx->stream);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipEventRecord(ctx->ev_end, ctx->stream));
        if (hits_host) HIP_CHECK(hipMemcpyAsync(hits_host, out.p, (size_t)n * sizeof(LjHit), hipMemcpyDeviceToHost, ctx->stream));
        else HIP_CHECK(hipMemcpyAsync(occ_host, out.p, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        const float ms = elapsed_ms(ctx->ev_begin, ctx->ev_end);
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

int lj_get_stats(const lj_scene *scene, LjStats *out) { return get_stats(scene, &lj_scene::stats, out, "lj_get_stats"); }

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
