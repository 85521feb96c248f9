// C-ABI entry points that move or rebuild an uploaded scene's geometry: lj_scene_update_geometry with the refit helpers (alloc_refit_tables,
// refit_launches, read_back_nodes), the two BVH builders behind lj_scene_rebuild_bvh / _ex (resolve_builder, build_workspace,
// build_binary_tree, rebuild_scene), lj_bvh_build_query / _ex (build_query), and lj_get_rebuild_stats / lj_get_build_stats.
#include "api_calls.h"
#include "dploc.h"
#include <chrono>

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

namespace {

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
    const std::vector<lj::BinaryNode> tree = relabelled(me, [&] { return build_binary_tree(ctx, bw, builder, n, s, order, bs); });
    const auto t1 = std::chrono::steady_clock::now();
    // ---- host: the wide trees, the leaf order and the level tables; every refusal comes from here
    lj::FlatScene R = relabelled(me, [&] { return lj::rebuild_trees(F, tree, order, ljd::max_stack_depth()); });
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
    const std::vector<lj::BinaryNode> tree = relabelled(me, [&] { return build_binary_tree(ctx, bw, builder, (int)n, s, order, bs); });
    *n_nodes = (int64_t)tree.size();
    if (nodes_out && capacity < *n_nodes) throw LjError(LJ_ERR_INVALID_ARG, me + ": buffer too small");
    for (int64_t i = 0; i < n; i++) order_out[i] = order[(size_t)i];
    if (nodes_out) memcpy(nodes_out, tree.data(), tree.size() * sizeof(LjBinaryNode));
}

} // namespace

extern "C" {

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

int lj_get_build_stats(const lj_scene *scene, LjBuildStats *out) { return get_stats(scene, &lj_scene::build_stats, out, "lj_get_build_stats"); }

int lj_get_rebuild_stats(const lj_scene *scene, LjRebuildStats *out) { return get_stats(scene, &lj_scene::rebuild_stats, out, "lj_get_rebuild_stats"); }

int lj_bvh_build_query(lj_context *ctx, int64_t n, const float *boxes, int32_t *order_out, LjBinaryNode *nodes_out, int64_t capacity, int64_t *n_nodes) {
    return lj::guard([&]() { build_query(ctx, nullptr, n, boxes, order_out, nodes_out, capacity, n_nodes, "lj_bvh_build_query"); });
}

int lj_bvh_build_query_ex(lj_context *ctx, const LjRebuildArgs *args, int64_t n, const float *boxes, int32_t *order_out, LjBinaryNode *nodes_out, int64_t capacity, int64_t *n_nodes) {
    return lj::guard([&]() { build_query(ctx, args, n, boxes, order_out, nodes_out, capacity, n_nodes, "lj_bvh_build_query_ex"); });
}

} // extern "C"
