// C-ABI entry points that own the GPU: context and scene lifetime, scene upload, camera and geometry updates, BVH read-back, batched ray
// queries, and the thin render entry points — what they render with (render plans, run_render and its five drivers) lives in render.hip.
// One context = one HIP device + one stream; one process per GPU (the multi-GPU layer above this is
// torch.distributed over RCCL, see bench.py).  Every HIP call is checked; failures surface as LJ_ERR_DEVICE with
// the HIP error string — there is no CPU fallback behind any of these functions.
#include "api_internal.h"
#include "../host/rays_call.h"
#include "dploc.h"
#include <chrono>
#include <mutex>
#include <set>

namespace {

// The uploaded scenes of this process: lj_scene_update_geometry and lj_scene_read_bvh look a handle up before they touch it, so that a
// destroyed one is an error and not a use after free.
std::mutex g_live_mutex;
std::set<const lj_scene *> g_live_scenes;
bool scene_is_live(const lj_scene *sc) { std::lock_guard<std::mutex> lock(g_live_mutex); return sc && g_live_scenes.count(sc) != 0; }

// One frame of a plan, all its views, into the caller's device memory or — for a host result — through the context's frame buffer.
// `views`: the camera table of a batch, uploaded for this render (null: the scene's own camera).
// The render always runs on the context's own streams — its lanes were created together and sit on distinct hardware
// queues; a caller's stream created later may share a queue with one of them, which serialises two lanes (measured:
// 26 -> 32 ms per cbox render) — and is ordered against the caller's stream by events on both sides.
void render_frame(lj_scene *scene, RenderPlan plan, const std::vector<ljd::DCamera> *views, float *rgb_host, float *rgb_device, hipStream_t caller, bool timing) {
    lj_context *ctx = scene->ctx;
    set_device(ctx);
    hipStream_t s = ctx->stream;
    if (caller) { HIP_CHECK(hipEventRecord(ctx->ev_caller, caller)); HIP_CHECK(hipStreamWaitEvent(s, ctx->ev_caller, 0)); }
    if (views) {
        const size_t table_bytes = views->size() * sizeof(ljd::DCamera);
        ensure(ctx->view_table, table_bytes);
        HIP_CHECK(hipMemcpyAsync(ctx->view_table.p, views->data(), table_bytes, hipMemcpyHostToDevice, s));
        plan.views_dev = (const ljd::DCamera *)ctx->view_table.p;
    }
    const size_t fb = (size_t)std::max(plan.n_views, 1) * scene->flat.cam.width * scene->flat.cam.height * 3 * sizeof(float);
    float *frame = rgb_device;
    if (!frame) { ensure(ctx->frame, fb); frame = (float *)ctx->frame.p; }
    HIP_CHECK(hipMemsetAsync(frame, 0, fb, s));
    run_render(scene, plan, frame, nullptr, s, timing);
    if (rgb_host) { HIP_CHECK(hipMemcpyAsync(rgb_host, frame, fb, hipMemcpyDeviceToHost, s)); HIP_CHECK(hipStreamSynchronize(s)); }
    if (caller) { HIP_CHECK(hipEventRecord(ctx->ev_caller, s)); HIP_CHECK(hipStreamWaitEvent(caller, ctx->ev_caller, 0)); }
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

// The refit launches over the scene's level tables (the leaf table first, then each tree from its deepest level up), and the copy of the
// refitted nodes into the host's (lj_scene_info and the tests read it); the caller waits for the stream.
void refit_launches(lj_scene *scene, hipStream_t s) {
    const lj::FlatScene &F = scene->flat;
    const ljd::DPrim *lp = (const ljd::DPrim *)scene->leaf_prims.p; const ljd::DSphere *sp = (const ljd::DSphere *)scene->spheres.p;
    if (!F.scan_leaves.empty()) ljd::launch_refit_scan((ljd::DScanLeaf *)scene->scan_leaves.p, lp, sp, F.n_scan_used, s);
    for (size_t l = F.level4_first.size() - 1; l-- > 0;)
        ljd::launch_refit4((ljd::DNode4 *)scene->nodes.p, scene->refit_box4.p, lp, sp, (const int32_t *)scene->refit_levels4.p + F.level4_first[l], F.level4_first[l + 1] - F.level4_first[l], s);
    const int stride8 = scene->dscene.node8_stride;
    for (size_t l = F.level8_first.size() - 1; l-- > 0;)
        ljd::launch_refit8(scene->nodes8.p, stride8, scene->refit_box8.p, lp, sp, (const int32_t *)scene->refit_levels8.p + F.level8_first[l], F.level8_first[l + 1] - F.level8_first[l], s);
    HIP_CHECK(hipGetLastError());
}
void read_back_nodes(lj_scene *scene, hipStream_t s) {
    lj::FlatScene &F = scene->flat;
    const int stride8 = scene->dscene.node8_stride;
    HIP_CHECK(hipMemcpyAsync(F.nodes.data(), scene->nodes.p, F.nodes.size() * sizeof(ljd::DNode4), hipMemcpyDeviceToHost, s));
    if (stride8 == (int)sizeof(ljd::DNode8)) HIP_CHECK(hipMemcpyAsync(F.nodes8.data(), scene->nodes8.p, F.nodes8.size() * sizeof(ljd::DNode8), hipMemcpyDeviceToHost, s));
    else HIP_CHECK(hipMemcpy2DAsync(F.nodes8.data(), sizeof(ljd::DNode8), scene->nodes8.p, (size_t)stride8, sizeof(ljd::DNode8), F.nodes8.size(), hipMemcpyDeviceToHost, s));
    if (!F.scan_leaves.empty()) HIP_CHECK(hipMemcpyAsync(F.scan_leaves.data(), scene->scan_leaves.p, F.scan_leaves.size() * sizeof(ljd::DScanLeaf), hipMemcpyDeviceToHost, s));
}
// the per-node box scratch and the level tables of a refit, for the trees as they stand
void alloc_refit_tables(lj_scene *scene, hipStream_t s) {
    const lj::FlatScene &F = scene->flat;
    const size_t bb = ljd::refit_box_bytes();
    scene->refit_box4.alloc(std::max<size_t>(F.nodes.size(), 1) * bb); scene->refit_box8.alloc(std::max<size_t>(F.nodes8.size(), 1) * bb);
    upload(scene->refit_levels4, F.levels4, s); upload(scene->refit_levels8, F.levels8, s);
}

static_assert(sizeof(LjBinaryNode) == sizeof(lj::BinaryNode) && sizeof(LjBinaryNode) == 40, "LjBinaryNode must be 40 bytes");

// The builder of a rebuild call: LjRebuildArgs checked and resolved (null or zeroed: the linear BVH)
struct Builder { int32_t kind = LJ_BUILD_LBVH, radius = 0; };
Builder resolve_builder(const LjRebuildArgs *args, const std::string &me) {
    Builder b;
    if (!args) return b;
    if (args->builder != LJ_BUILD_LBVH && args->builder != LJ_BUILD_PLOC) throw LjError(LJ_ERR_INVALID_ARG, me + ": unknown builder " + std::to_string(args->builder));
    b.kind = args->builder;
    if (b.kind == LJ_BUILD_PLOC) {
        if (args->radius > ljd::kPlocRadiusMax) throw LjError(LJ_ERR_INVALID_ARG, me + ": radius " + std::to_string(args->radius) + " is above " + std::to_string(ljd::kPlocRadiusMax));
        b.radius = args->radius <= 0 ? ljd::kPlocRadiusDefault : args->radius;
    }
    return b;
}
// LJ_TUNE_PLOC_TAIL=m: the single-workgroup launch takes over at m clusters or fewer (clamped to [1, 1024]; 1: every round is a round of
// whole-grid launches) — the tests compare the two paths with it.  The tree does not depend on it.
inline int ploc_tail() { return env_int("LJ_TUNE_PLOC_TAIL", ljd::kPlocTail); }

// The workspace of a build over n boxes: rebuild.hip's, and behind it ploc.hip's where that builder runs
struct BuildWork { ljd::RebuildWork w; ljd::PlocWork p; };
BuildWork build_workspace(lj_context *ctx, const Builder &b, int n, hipStream_t s) {
    const size_t first = ljd::rebuild_carve(nullptr, n, s).bytes;
    ensure(ctx->rebuild_ws, first + (b.kind == LJ_BUILD_PLOC ? ljd::ploc_carve(nullptr, n).bytes : 0));
    return BuildWork{ljd::rebuild_carve(ctx->rebuild_ws.p, n, s), b.kind == LJ_BUILD_PLOC ? ljd::ploc_carve((char *)ctx->rebuild_ws.p + first, n) : ljd::PlocWork{}};
}

// The device's binary tree over the n boxes in w.boxes — the linear BVH, or the clustering of dploc.h: order and the compacted binary tree on
// the host.  Waits for the stream.
std::vector<lj::BinaryNode> build_binary_tree(lj_context *ctx, const BuildWork &bw, const Builder &b, int n, hipStream_t s, std::vector<int> &order, LjBuildStats &bs) {
    const ljd::RebuildWork &w = bw.w;
    bs = LjBuildStats{}; bs.builder = b.kind; bs.radius = b.radius;
    if (b.kind == LJ_BUILD_PLOC) {
        const auto t0 = std::chrono::steady_clock::now();
        const ljd::PlocRun run = ljd::launch_ploc(w, bw.p, n, b.radius, ploc_tail(), (uint32_t *)ctx->stats_host, s);
        if (!run.finished) throw LjError(LJ_ERR_UNSUPPORTED, std::to_string(ljd::kPlocMaxRounds) + " rounds of clustering left more than " + std::to_string(ljd::kPlocTail) + " clusters: use the linear builder (LJ_BUILD_LBVH) for this scene");
        bs.rounds = run.rounds; bs.tail_rounds = run.tail_rounds;
        bs.cluster_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    } else ljd::launch_rebuild(w, n, s);
    HIP_CHECK(hipGetLastError());
    std::vector<float> boxes((size_t)n * 6);
    std::vector<int32_t> order32((size_t)n);
    std::vector<unsigned char> raw((size_t)std::max(n - 1, 0) * ljd::rebuild_node_bytes());
    HIP_CHECK(hipMemcpyAsync(boxes.data(), w.boxes, boxes.size() * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(order32.data(), w.order, order32.size() * 4, hipMemcpyDeviceToHost, s));
    if (!raw.empty()) HIP_CHECK(hipMemcpyAsync(raw.data(), w.nodes, raw.size(), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    for (int32_t g : order32) if (g < 0 || g >= n) throw LjError(LJ_ERR_INTERNAL, "the device's sort returned an index outside the primitives");
    if (b.kind == LJ_BUILD_PLOC) {
        std::vector<int32_t> walked;
        std::vector<lj::BinaryNode> tree = lj::compact_ploc_tree(raw.data(), boxes.data(), order32.data(), n, walked);
        order.assign(walked.begin(), walked.end());
        return tree;
    }
    order.assign(order32.begin(), order32.end());
    return lj::compact_radix_tree(raw.data(), boxes.data(), order32.data(), n);
}

// lj_scene_rebuild_bvh and lj_scene_rebuild_bvh_ex
void rebuild_scene(lj_scene *scene, const LjRebuildArgs *args, const std::string &me) {
    if (!scene) throw LjError(LJ_ERR_INVALID_ARG, me + ": null scene");
    if (!scene_is_live(scene)) throw LjError(LJ_ERR_INVALID_ARG, me + ": not an uploaded scene (destroyed?)");
    const Builder builder = resolve_builder(args, me);
    lj::FlatScene &F = scene->flat;
    auto tree_stats = [&](uint64_t rebuilt) {
        LjRebuildStats r{};
        r.rebuilt = rebuilt; r.n_prims = F.prims.size(); r.n_nodes4 = F.nodes.size(); r.n_nodes8 = F.nodes8.size(); r.depth4 = F.bvh_depth; r.depth8 = F.bvh8_depth;
        for (const ljd::DNode4 &nd : F.nodes) for (int k = 0; k < 4; k++) if (nd.lox[k] <= nd.hix[k] && nd.child[k] < 0) r.n_leaves++;
        return r;
    };
    const size_t n_prims = F.prims.size();
    if (!F.scan_leaves.empty() || n_prims == 0 || F.leaf_prims.empty()) {   // a leaf-scan scene or an empty one: nothing to rebuild
        scene->rebuild_stats = tree_stats(0); scene->build_stats = LjBuildStats{}; scene->stats = LjStats{};
        return;
    }
    if ((long long)n_prims * 8 >= (1ll << 30)) throw LjError(LJ_ERR_UNSUPPORTED, me + ": too many primitives for the 30-bit leaf code");
    const int n = (int)n_prims;
    lj_context *ctx = scene->ctx;
    set_device(ctx);
    hipStream_t s = ctx->stream;
    // ---- device: the binary tree, into the context's workspace (the scene is only read)
    const BuildWork bw = build_workspace(ctx, builder, n, s);
    const auto t0 = std::chrono::steady_clock::now();
    ljd::launch_rebuild_prim_boxes((const ljd::DPrim *)scene->leaf_prims.p, (int)F.leaf_prims.size(), (const ljd::DSphere *)scene->spheres.p, bw.w, n, s);
    std::vector<int> order;
    LjBuildStats bs;
    std::vector<lj::BinaryNode> tree;
    try { tree = build_binary_tree(ctx, bw, builder, n, s, order, bs); }
    catch (const LjError &e) { throw LjError(e.code, me + ": " + e.what()); }
    const auto t1 = std::chrono::steady_clock::now();
    // ---- host: the wide trees, the leaf order and the level tables; every refusal comes from here
    lj::FlatScene R;
    try { R = lj::rebuild_trees(F, tree, order, ljd::max_stack_depth()); }
    catch (const LjError &e) { throw LjError(e.code, me + ": " + e.what()); }
    // ---- nothing of the scene was written up to here
    lj::commit_rebuild(F, std::move(R));
    const auto t2 = std::chrono::steady_clock::now();
    HIP_CHECK(hipEventRecord(ctx->ev_begin, s));
    install_trees(scene, s);
    alloc_refit_tables(scene, s);
    refit_launches(scene, s);
    HIP_CHECK(hipEventRecord(ctx->ev_end, s));
    read_back_nodes(scene, s);
    HIP_CHECK(hipStreamSynchronize(s));
    auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    LjRebuildStats r = tree_stats(1);
    r.build_ms = ms(t0, t1); r.emit_ms = ms(t1, t2); r.refit_ms = elapsed_ms(ctx->ev_begin, ctx->ev_end);
    scene->rebuild_stats = r; scene->build_stats = bs;
    // LjStats of a rebuild: render_ms = device time (the build with its readback, the upload of the trees and the refit), generate_ms = host time
    scene->stats = LjStats{}; scene->stats.render_ms = (float)(r.build_ms + r.refit_ms); scene->stats.generate_ms = (float)r.emit_ms;
}

// lj_bvh_build_query and lj_bvh_build_query_ex
void build_query(lj_context *ctx, const LjRebuildArgs *args, int64_t n, const float *boxes, int32_t *order_out, LjBinaryNode *nodes_out, int64_t capacity, int64_t *n_nodes, const std::string &me) {
    if (!ctx || !n_nodes) throw LjError(LJ_ERR_INVALID_ARG, me + ": null argument");
    const Builder builder = resolve_builder(args, me);
    if (n < 0 || n * 8 >= (1ll << 30)) throw LjError(LJ_ERR_INVALID_ARG, me + ": n must be in [0, 2^27)");
    if (n > 0 && (!boxes || !order_out)) throw LjError(LJ_ERR_INVALID_ARG, me + ": null array");
    for (int64_t i = 0; i < n; i++) for (int k = 0; k < 3; k++) {
        const float lo = boxes[6 * i + k], hi = boxes[6 * i + 3 + k];
        if (!(lo <= hi) || !(std::fabs(lo) <= 3.402823466e38f) || !(std::fabs(hi) <= 3.402823466e38f)) throw LjError(LJ_ERR_INVALID_ARG, me + ": box " + std::to_string(i) + " is empty or not finite");
    }
    // ---- nothing was written up to here
    *n_nodes = 0;
    if (n == 0) return;
    set_device(ctx);
    hipStream_t s = ctx->stream;
    const BuildWork bw = build_workspace(ctx, builder, (int)n, s);
    HIP_CHECK(hipMemcpyAsync(bw.w.boxes, boxes, (size_t)n * 24, hipMemcpyHostToDevice, s));
    std::vector<int> order;
    LjBuildStats bs;
    std::vector<lj::BinaryNode> tree;
    try { tree = build_binary_tree(ctx, bw, builder, (int)n, s, order, bs); }
    catch (const LjError &e) { throw LjError(e.code, me + ": " + e.what()); }
    *n_nodes = (int64_t)tree.size();
    if (nodes_out && capacity < *n_nodes) throw LjError(LJ_ERR_INVALID_ARG, me + ": buffer too small");
    for (int64_t i = 0; i < n; i++) order_out[i] = order[(size_t)i];
    if (nodes_out) memcpy(nodes_out, tree.data(), tree.size() * sizeof(LjBinaryNode));
}

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
        HIP_CHECK(hipEventCreate(&ctx->ev_f0)); HIP_CHECK(hipEventCreate(&ctx->ev_f1)); HIP_CHECK(hipEventCreate(&ctx->ev_f2));
        HIP_CHECK(hipEventCreate(&ctx->ev_d0)); HIP_CHECK(hipEventCreate(&ctx->ev_d1));
        HIP_CHECK(hipEventCreate(&ctx->ev_a0)); HIP_CHECK(hipEventCreate(&ctx->ev_a1)); HIP_CHECK(hipEventCreate(&ctx->ev_a2));
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
    for (hipEvent_t e : {ctx->ev_begin, ctx->ev_end, ctx->ev_k0, ctx->ev_k1, ctx->ev_f0, ctx->ev_f1, ctx->ev_f2, ctx->ev_d0, ctx->ev_d1, ctx->ev_a0, ctx->ev_a1, ctx->ev_a2}) if (e) (void)hipEventDestroy(e);
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
            sc->scfg.variant = ljd::shade_variant(kinds, textured, F.envmap_light_id >= 0, sphere_lights);
            sc->scfg.variant = std::max(sc->scfg.variant, env_int("LJ_TUNE_SHADE_VARIANT", sc->scfg.variant));
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
        render_frame(scene, make_plan(scene, args), nullptr, nullptr, rgb_device, (hipStream_t)hip_stream, timing_requested(args));
    });
}

int lj_render(lj_scene *scene, const LjRenderArgs *args, float *rgb_host) {
    return lj::guard([&]() {
        if (!scene || !rgb_host) throw LjError(LJ_ERR_INVALID_ARG, "lj_render: null argument");
        render_frame(scene, make_plan(scene, args), nullptr, rgb_host, nullptr, nullptr, timing_requested(args));
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
        if (!scene->refit_box4.p) alloc_refit_tables(scene, s);
        // ---- device, in stream order: the tables, then the boxes of the three structures from the new leaf-ordered primitives
        HIP_CHECK(hipEventRecord(ctx->ev_begin, s));
        auto put = [&](DevBuf &b, const auto &v) { HIP_CHECK(hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(v[0]), hipMemcpyHostToDevice, s)); };
        put(scene->leaf_prims, U.leaf_prims); put(scene->prims, U.prims); put(scene->spheres, U.spheres); put(scene->light_tris, U.light_tris);
        put(scene->light_tri_cdf, U.light_tri_cdf); put(scene->lights, U.lights); put(scene->light_cdf, U.light_cdf);
        refit_launches(scene, s);
        HIP_CHECK(hipEventRecord(ctx->ev_end, s));
        // the host copy of the nodes follows the device's (lj_scene_info and the tests read it)
        read_back_nodes(scene, s);
        HIP_CHECK(hipStreamSynchronize(s));
        const float ms = elapsed_ms(ctx->ev_begin, ctx->ev_end);
        lj::commit_update(F, std::move(U));
        scene->dscene.eps = (float)F.shadow_epsilon;
        // LjStats of an update: render_ms = device time (copies of the tables and the refit launches), generate_ms = host time of the re-derivation
        scene->stats = LjStats{}; scene->stats.render_ms = ms; scene->stats.generate_ms = host_ms;
    });
}

int lj_scene_rebuild_bvh(lj_scene *scene) {
    return lj::guard([&]() { rebuild_scene(scene, nullptr, "lj_scene_rebuild_bvh"); });
}

int lj_scene_rebuild_bvh_ex(lj_scene *scene, const LjRebuildArgs *args) {
    return lj::guard([&]() { rebuild_scene(scene, args, "lj_scene_rebuild_bvh_ex"); });
}

int lj_get_build_stats(const lj_scene *scene, LjBuildStats *out) {
    if (!scene || !out) { lj::set_last_error("lj_get_build_stats: null argument"); return LJ_ERR_INVALID_ARG; }
    *out = scene->build_stats;
    return LJ_OK;
}

int lj_get_rebuild_stats(const lj_scene *scene, LjRebuildStats *out) {
    if (!scene || !out) { lj::set_last_error("lj_get_rebuild_stats: null argument"); return LJ_ERR_INVALID_ARG; }
    *out = scene->rebuild_stats;
    return LJ_OK;
}

int lj_bvh_build_query(lj_context *ctx, int64_t n, const float *boxes, int32_t *order_out, LjBinaryNode *nodes_out, int64_t capacity, int64_t *n_nodes) {
    return lj::guard([&]() { build_query(ctx, nullptr, n, boxes, order_out, nodes_out, capacity, n_nodes, "lj_bvh_build_query"); });
}

int lj_bvh_build_query_ex(lj_context *ctx, const LjRebuildArgs *args, int64_t n, const float *boxes, int32_t *order_out, LjBinaryNode *nodes_out, int64_t capacity, int64_t *n_nodes) {
    return lj::guard([&]() { build_query(ctx, args, n, boxes, order_out, nodes_out, capacity, n_nodes, "lj_bvh_build_query_ex"); });
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

// the camera table of a batch, every view checked against the scene's camera
static std::vector<ljd::DCamera> view_table(const lj_scene *scene, int32_t n_views, const LjCamera *views, const char *who) {
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
    return table;
}

static void render_views(lj_scene *scene, const LjRenderArgs *args, int32_t n_views, const LjCamera *views, float *rgb_host, float *rgb_device, hipStream_t caller, const char *who) {
    if (!scene || !views || (!rgb_host && !rgb_device)) throw LjError(LJ_ERR_INVALID_ARG, std::string(who) + ": null argument");
    if (n_views <= 0) throw LjError(LJ_ERR_INVALID_ARG, std::string(who) + ": n_views must be positive");
    const std::vector<ljd::DCamera> table = view_table(scene, n_views, views, who);
    render_frame(scene, make_views_plan(scene, args, n_views), &table, rgb_host, rgb_device, caller, timing_requested(args));
}

// lj_render_features / _device: every check first, then render_frame's steps with up to five more frames beside the image.
// `out`: host pointers (on_device false: the frames live in the context's workspace and only those asked for are copied back) or device pointers.
static void render_features(lj_scene *scene, const LjRenderArgs *args, int32_t n_views, const LjCamera *views, const LjFeatureBuffers *out, bool on_device, hipStream_t caller, const char *who) {
    if (!scene || !out) throw LjError(LJ_ERR_INVALID_ARG, std::string(who) + ": null argument");
    float *const dst[6] = {out->rgb, out->albedo, out->normal, out->depth, out->alpha, out->variance};
    if (std::none_of(dst, dst + 6, [](float *p) { return p != nullptr; })) throw LjError(LJ_ERR_INVALID_ARG, std::string(who) + ": no buffer asked for");
    if (n_views < 0) throw LjError(LJ_ERR_INVALID_ARG, std::string(who) + ": n_views must not be negative");
    if ((n_views > 0) != (views != nullptr)) throw LjError(LJ_ERR_INVALID_ARG, std::string(who) + ": n_views and views must both be given or both be left out");
    if (scene->flat.integrator < LJ_INTEGRATOR_PATH) throw LjError(LJ_ERR_UNSUPPORTED, std::string(who) + ": the auxiliary integrators have no guide buffers (path and volpath only)");
    if (args && args->rng_mode == LJ_RNG_TILE) throw LjError(LJ_ERR_UNSUPPORTED, std::string(who) + ": rng_mode must be LJ_RNG_SAMPLE (the per-tile schedule keeps no per-sample values)");
    std::vector<ljd::DCamera> table;
    if (n_views > 0) table = view_table(scene, n_views, views, who);
    RenderPlan plan = n_views > 0 ? make_views_plan(scene, args, n_views) : make_plan(scene, args);
    // ---- nothing was written up to here
    lj_context *ctx = scene->ctx;
    set_device(ctx);
    hipStream_t s = ctx->stream;
    if (caller) { HIP_CHECK(hipEventRecord(ctx->ev_caller, caller)); HIP_CHECK(hipStreamWaitEvent(s, ctx->ev_caller, 0)); }
    if (n_views > 0) {
        const size_t table_bytes = table.size() * sizeof(ljd::DCamera);
        ensure(ctx->view_table, table_bytes);
        HIP_CHECK(hipMemcpyAsync(ctx->view_table.p, table.data(), table_bytes, hipMemcpyHostToDevice, s));
        plan.views_dev = (const ljd::DCamera *)ctx->view_table.p;
    }
    const size_t n_pix = (size_t)std::max(n_views, 1) * scene->flat.cam.width * scene->flat.cam.height;
    const size_t chan[6] = {3, 3, 3, 1, 1, 3};
    float *frame[6] = {};
    if (on_device) for (int k = 0; k < 6; k++) frame[k] = dst[k];
    else {
        if (dst[0]) { ensure(ctx->frame, n_pix * 3 * sizeof(float)); frame[0] = (float *)ctx->frame.p; }
        size_t need = 0;
        for (int k = 1; k < 6; k++) if (dst[k]) need += n_pix * chan[k];
        ensure(ctx->feature_frames, need * sizeof(float));
        float *at = (float *)ctx->feature_frames.p;
        for (int k = 1; k < 6; k++) if (dst[k]) { frame[k] = at; at += n_pix * chan[k]; }
    }
    for (int k = 0; k < 6; k++) if (frame[k]) HIP_CHECK(hipMemsetAsync(frame[k], 0, n_pix * chan[k] * sizeof(float), s));
    plan.feat.albedo = frame[1]; plan.feat.normal = frame[2]; plan.feat.depth = frame[3]; plan.feat.alpha = frame[4]; plan.feat.variance = frame[5];
    plan.feat.want = (frame[1] ? ljd::FEAT_ALBEDO : 0u) | (frame[2] ? ljd::FEAT_NORMAL : 0u) | (frame[3] ? ljd::FEAT_DEPTH : 0u) | (frame[4] ? ljd::FEAT_ALPHA : 0u) | (frame[5] ? ljd::FEAT_VARIANCE : 0u);
    run_render(scene, plan, frame[0], nullptr, s, timing_requested(args));
    if (!on_device) {
        for (int k = 0; k < 6; k++) if (dst[k]) HIP_CHECK(hipMemcpyAsync(dst[k], frame[k], n_pix * chan[k] * sizeof(float), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
    }
    if (caller) { HIP_CHECK(hipEventRecord(ctx->ev_caller, s)); HIP_CHECK(hipStreamWaitEvent(caller, ctx->ev_caller, 0)); }
}

int lj_render_views(lj_scene *scene, const LjRenderArgs *args, int32_t n_views, const LjCamera *views, float *rgb_host) {
    return lj::guard([&]() { render_views(scene, args, n_views, views, rgb_host, nullptr, nullptr, "lj_render_views"); });
}

int lj_render_views_device(lj_scene *scene, const LjRenderArgs *args, int32_t n_views, const LjCamera *views, float *rgb_device, void *hip_stream) {
    return lj::guard([&]() { render_views(scene, args, n_views, views, nullptr, rgb_device, (hipStream_t)hip_stream, "lj_render_views_device"); });
}

int lj_render_features(lj_scene *scene, const LjRenderArgs *args, int32_t n_views, const LjCamera *views, const LjFeatureBuffers *out_host) {
    return lj::guard([&]() { render_features(scene, args, n_views, views, out_host, false, nullptr, "lj_render_features"); });
}

int lj_render_features_device(lj_scene *scene, const LjRenderArgs *args, int32_t n_views, const LjCamera *views, const LjFeatureBuffers *out_device, void *hip_stream) {
    return lj::guard([&]() { render_features(scene, args, n_views, views, out_device, true, (hipStream_t)hip_stream, "lj_render_features_device"); });
}

int lj_get_feature_stats(const lj_scene *scene, LjFeatureStats *out) {
    if (!scene || !out) { lj::set_last_error("lj_get_feature_stats: null argument"); return LJ_ERR_INVALID_ARG; }
    *out = scene->feature_stats;
    return LJ_OK;
}

// lj_denoise / _device: every check first, then pack, one k_atrous launch per iteration, unpack — on the context's stream, ordered against
// the caller's as render_frame orders a render.  The host variant stages its buffers in the context's workspace.
static void denoise(lj_context *ctx, int32_t n, int32_t w, int32_t h, const LjFeatureBuffers *in, const LjDenoiseArgs *args, float *rgb_out, float *variance_out,
                    bool on_device, hipStream_t caller, const char *who) {
    const std::string me(who);
    if (!ctx || !in || !in->rgb || !rgb_out) throw LjError(LJ_ERR_INVALID_ARG, me + ": null argument");
    if (n <= 0 || w <= 0 || h <= 0) throw LjError(LJ_ERR_INVALID_ARG, me + ": n, width and height must be positive");
    const uint64_t limit = 1ull << 31, image = (uint64_t)w * (uint64_t)h;
    if (image > limit || image * (uint64_t)n > limit) throw LjError(LJ_ERR_INVALID_ARG, me + ": more than 2^31 pixels");
    const LjDenoiseArgs a = args ? *args : LjDenoiseArgs{};
    if (a.iterations > ljd::denoise_max_iterations()) throw LjError(LJ_ERR_INVALID_ARG, me + ": at most 8 iterations");
    for (float sg : {a.sigma_color, a.sigma_normal, a.sigma_depth, a.sigma_albedo})
        if (!(sg >= 0.0f) || !(sg <= 3.402823466e38f)) throw LjError(LJ_ERR_INVALID_ARG, me + ": a sigma is negative or not finite");
    if (a.flags & ~(uint32_t)LJ_DENOISE_DEMODULATE) throw LjError(LJ_ERR_INVALID_ARG, me + ": unknown flag");
    if ((a.flags & LJ_DENOISE_DEMODULATE) && !in->albedo) throw LjError(LJ_ERR_INVALID_ARG, me + ": LJ_DENOISE_DEMODULATE needs the albedo buffer");
    if (variance_out && !in->variance) throw LjError(LJ_ERR_INVALID_ARG, me + ": variance_out needs the variance buffer");
    const uint32_t has = ljd::denoise_has(in->variance, in->albedo, in->normal, in->depth, (a.flags & LJ_DENOISE_DEMODULATE) != 0);
    const ljd::DenoiseCall call{has, a.iterations, {a.sigma_color, a.sigma_normal, a.sigma_depth, a.sigma_albedo}};
    const int iterations = ljd::denoise_iterations(call);
    // ---- nothing was written up to here
    set_device(ctx);
    hipStream_t s = ctx->stream;
    // the device variant returns without waiting, so it is ordered against the caller's stream on both sides even when that is the null
    // stream (the context's stream does not synchronise with it by itself)
    if (on_device) { HIP_CHECK(hipEventRecord(ctx->ev_caller, caller)); HIP_CHECK(hipStreamWaitEvent(s, ctx->ev_caller, 0)); }
    const uint64_t total = image * (uint64_t)n;
    const float *src[5] = {in->rgb, in->variance, in->albedo, in->normal, in->depth};
    const size_t chan[5] = {3, 3, 3, 3, 1};
    float *out_rgb = rgb_out, *out_var = variance_out;
    if (!on_device) {
        size_t need = 0;
        for (int k = 0; k < 5; k++) if (src[k]) need += total * chan[k];
        ensure(ctx->dn_in, need * sizeof(float));
        ensure(ctx->dn_out, total * 6 * sizeof(float));
        float *at = (float *)ctx->dn_in.p;
        for (int k = 0; k < 5; k++) if (src[k]) {
            HIP_CHECK(hipMemcpyAsync(at, src[k], total * chan[k] * sizeof(float), hipMemcpyHostToDevice, s));
            src[k] = at; at += total * chan[k];
        }
        out_rgb = (float *)ctx->dn_out.p; out_var = variance_out ? out_rgb + total * 3 : nullptr;
    }
    ensure(ctx->dn_guide, total * ljd::denoise_record_bytes());
    for (DevBuf &b : ctx->dn_dyn) ensure(b, total * ljd::denoise_record_bytes());
    const int lds_iterations = denoise_lds_iterations();
    HIP_CHECK(hipEventRecord(ctx->ev_d0, s));
    ljd::launch_denoise_pack(has, total, src[0], src[1], src[2], src[3], src[4], ctx->dn_guide.p, ctx->dn_dyn[0].p, s);
    for (int i = 0; i < iterations; i++)
        ljd::launch_atrous(call, n, w, h, i, i < lds_iterations, ctx->dn_guide.p, ctx->dn_dyn[i & 1].p, ctx->dn_dyn[(i + 1) & 1].p, s);
    ljd::launch_denoise_unpack(has, total, ctx->dn_guide.p, ctx->dn_dyn[iterations & 1].p, out_rgb, out_var, s);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(ctx->ev_d1, s));
    ctx->denoise_stats = LjDenoiseStats{}; ctx->denoise_stats.launches = (uint64_t)iterations + 2; ctx->denoise_stats.pixels = total;
    ctx->denoise_time_pending = true;
    if (!on_device) {
        HIP_CHECK(hipMemcpyAsync(rgb_out, out_rgb, total * 3 * sizeof(float), hipMemcpyDeviceToHost, s));
        if (variance_out) HIP_CHECK(hipMemcpyAsync(variance_out, out_var, total * 3 * sizeof(float), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
    }
    if (on_device) { HIP_CHECK(hipEventRecord(ctx->ev_caller, s)); HIP_CHECK(hipStreamWaitEvent(caller, ctx->ev_caller, 0)); }
}

int lj_denoise(lj_context *ctx, int32_t n, int32_t width, int32_t height, const LjFeatureBuffers *in_host, const LjDenoiseArgs *args, float *rgb_out_host, float *variance_out_host) {
    return lj::guard([&]() { denoise(ctx, n, width, height, in_host, args, rgb_out_host, variance_out_host, false, nullptr, "lj_denoise"); });
}

int lj_denoise_device(lj_context *ctx, int32_t n, int32_t width, int32_t height, const LjFeatureBuffers *in_device, const LjDenoiseArgs *args, float *rgb_out_device, float *variance_out_device,
                      void *hip_stream) {
    return lj::guard([&]() { denoise(ctx, n, width, height, in_device, args, rgb_out_device, variance_out_device, true, (hipStream_t)hip_stream, "lj_denoise_device"); });
}

int lj_get_denoise_stats(const lj_context *ctx_in, LjDenoiseStats *out) {
    return lj::guard([&]() {
        if (!ctx_in || !out) throw LjError(LJ_ERR_INVALID_ARG, "lj_get_denoise_stats: null argument");
        lj_context *ctx = const_cast<lj_context *>(ctx_in);
        if (ctx->denoise_time_pending) {   // the last call's launches may still run (the device variant does not wait): their time is read here, once
            set_device(ctx);
            HIP_CHECK(hipEventSynchronize(ctx->ev_d1));
            ctx->denoise_stats.denoise_ms = elapsed_ms(ctx->ev_d0, ctx->ev_d1);
            ctx->denoise_time_pending = false;
        }
        *out = ctx->denoise_stats;
    });
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
static void render_adaptive(lj_scene *scene, const LjRenderArgs *args, const LjAdaptiveArgs *aargs, const LjAdaptiveBuffers *out, bool on_device, hipStream_t caller, const char *who) {
    const std::string me(who);
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
    set_device(ctx);
    hipStream_t s = ctx->stream;
    if (caller) { HIP_CHECK(hipEventRecord(ctx->ev_caller, caller)); HIP_CHECK(hipStreamWaitEvent(s, ctx->ev_caller, 0)); }
    const int w = scene->flat.cam.width, h = scene->flat.cam.height;
    const size_t n_pix = (size_t)w * (size_t)h;
    const size_t chan[7] = {3, 3, 1, 3, 3, 1, 1};
    void *frame[7] = {};
    if (on_device) for (int k = 0; k < 7; k++) frame[k] = dst[k];
    else {
        size_t need = 0, guides = 0;
        for (int k = 0; k < 3; k++) if (dst[k]) need += n_pix * chan[k];
        for (int k = 3; k < 7; k++) if (dst[k]) guides += n_pix * chan[k];
        ensure(ctx->ad_out, need * 4);
        ensure(ctx->feature_frames, guides * 4);
        float *at = (float *)ctx->ad_out.p, *gat = (float *)ctx->feature_frames.p;
        for (int k = 0; k < 3; k++) if (dst[k]) { frame[k] = at; at += n_pix * chan[k]; }
        for (int k = 3; k < 7; k++) if (dst[k]) { frame[k] = gat; gat += n_pix * chan[k]; }
    }
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
    if (!on_device) {
        for (int k = 0; k < 7; k++) if (dst[k]) HIP_CHECK(hipMemcpyAsync(dst[k], frame[k], n_pix * chan[k] * 4, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
    }
    if (caller) { HIP_CHECK(hipEventRecord(ctx->ev_caller, s)); HIP_CHECK(hipStreamWaitEvent(caller, ctx->ev_caller, 0)); }
    scene->stats = sum; scene->feature_stats = LjFeatureStats{}; scene->adaptive_stats = as;
}

int lj_render_adaptive(lj_scene *scene, const LjRenderArgs *args, const LjAdaptiveArgs *adaptive, const LjAdaptiveBuffers *out_host) {
    return lj::guard([&]() { render_adaptive(scene, args, adaptive, out_host, false, nullptr, "lj_render_adaptive"); });
}

int lj_render_adaptive_device(lj_scene *scene, const LjRenderArgs *args, const LjAdaptiveArgs *adaptive, const LjAdaptiveBuffers *out_device, void *hip_stream) {
    return lj::guard([&]() { render_adaptive(scene, args, adaptive, out_device, true, (hipStream_t)hip_stream, "lj_render_adaptive_device"); });
}

int lj_get_adaptive_stats(const lj_scene *scene, LjAdaptiveStats *out) {
    if (!scene || !out) { lj::set_last_error("lj_get_adaptive_stats: null argument"); return LJ_ERR_INVALID_ARG; }
    *out = scene->adaptive_stats;
    return LJ_OK;
}

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

// ---- lj_radiance_rays / lj_irradiance / lj_probe_ray_queries: run_render over a table of rays or probes

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

static void radiance_rays(lj_scene *scene, const LjRenderArgs *args, const LjRaysArgs *ra, int64_t n, const float *table, uint32_t kind, const LjRadianceBuffers *out, const char *who) {
    RenderPlan plan = rays_plan(scene, args, ra, n, table, kind, out, true, who);
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
