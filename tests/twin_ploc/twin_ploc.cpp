// TEST INFRASTRUCTURE — host twin of lj_scene_rebuild_bvh_ex with LJ_BUILD_PLOC: the clustering of device/dploc.h run round by round over
// the order of the rebuild twin (whole rounds only: the device's single-workgroup tail must give the same bytes), then the product's
// compact_ploc_tree, rebuild_trees and the refit.  The twin of lj_scene_rebuild_bvh (tests/twin_rebuild) is compiled into this library
// whole, as that one holds the twin of the geometry update: a PLOC rebuild works on a scene that update created and moved, and is traced
// and read through the same entry points.  Built only by the test suite, never loaded by the product, and not a fallback.
#include "../twin_rebuild/twin_rebuild.cpp"
#include "../../lajolla_public_amd/csrc/device/dploc.h"

namespace {

// The clustering over n boxes: the Morton order and the n - 1 raw nodes as the kernels leave them; returns the rounds it took
int ploc_host(int n, const RefitBox *boxes, int radius, std::vector<int32_t> &order, std::vector<RebuildNode> &nodes) {
    std::vector<RebuildNode> radix;
    lbvh_host(n, boxes, order, radix);   // (for its order: the codes and the stable sort)
    nodes.assign((size_t)std::max(n - 1, 0), RebuildNode{});
    if (n < 2) return 0;
    std::vector<RefitBox> box((size_t)n), next_box;
    std::vector<int32_t> id((size_t)n), count((size_t)n, 1), next_id, next_count, nn;
    for (int p = 0; p < n; p++) { box[p] = boxes[order[p]]; id[p] = ~p; }
    int done = 0, rounds = 0;
    for (int m = n; m > 1; m = (int)box.size(), rounds++) {
        nn.resize((size_t)m);
        const RefitBox *at = box.data();
        for (int i = 0; i < m; i++) nn[i] = ploc_nearest([at](int j) { return at[j]; }, m, i, radius);
        next_box.clear(); next_id.clear(); next_count.clear();
        for (int i = 0; i < m; i++) {
            const int role = ploc_role(nn.data(), i);
            if (role == 2) continue;
            if (role == 1) {
                const int j = nn[i];
                RebuildNode &nd = nodes[(size_t)done];
                ploc_merge(box[i], box[j], id[i], id[j], count[i], count[j], nd);
                next_box.push_back(nd.box); next_id.push_back(done); next_count.push_back(nd.count);
                done++;
            } else { next_box.push_back(box[i]); next_id.push_back(id[i]); next_count.push_back(count[i]); }
        }
        if ((int)next_box.size() >= m) throw lj::LjError(LJ_ERR_INTERNAL, "a round of the clustering merged nothing");
        box.swap(next_box); id.swap(next_id); count.swap(next_count);
    }
    return rounds;
}

int resolve_radius(int radius) { return radius <= 0 ? kPlocRadiusDefault : radius; }

} // namespace

extern "C" {

// lj_bvh_build_query_ex(LJ_BUILD_PLOC) on the host: order[n], nodes (40-byte LjBinaryNode records, capacity `cap`); returns the number of
// nodes, -1 when cap is too small; rounds[0]: the rounds of clustering
int64_t ploc_build(int64_t n, const float *boxes, int radius, int32_t *order_out, void *nodes_out, int64_t cap, int32_t *rounds) {
    std::vector<int32_t> order, walked; std::vector<RebuildNode> raw;
    const int r = ploc_host((int)n, (const RefitBox *)boxes, resolve_radius(radius), order, raw);
    if (rounds) *rounds = r;
    const std::vector<lj::BinaryNode> tree = lj::compact_ploc_tree(raw.data(), boxes, order.data(), n, walked);
    if ((int64_t)tree.size() > cap) return -1;
    if (n > 0) memcpy(order_out, walked.data(), (size_t)n * 4);
    if (!tree.empty()) memcpy(nodes_out, tree.data(), tree.size() * sizeof(lj::BinaryNode));
    return (int64_t)tree.size();
}

// lj_scene_rebuild_bvh_ex(LJ_BUILD_PLOC) on the host, on a twin of refit_create: as rebuild_rebuild
int ploc_rebuild(void *tv, int radius, int max_depth4, int32_t *rebuilt, char *err, int err_len) {
    Twin *t = (Twin *)tv;
    lj::FlatScene &F = t->flat;
    *rebuilt = 0;
    try {
        const int n = (int)F.prims.size();
        if (!F.scan_leaves.empty() || n == 0 || F.leaf_prims.empty()) return 0;
        std::vector<RefitBox> boxes((size_t)n);
        for (const DPrim &p : F.leaf_prims) refit_prim_box(p, F.spheres.data(), boxes[p.gprim]);
        std::vector<int32_t> order32, walked; std::vector<RebuildNode> raw;
        ploc_host(n, boxes.data(), resolve_radius(radius), order32, raw);
        const std::vector<lj::BinaryNode> tree = lj::compact_ploc_tree(raw.data(), (const float *)boxes.data(), order32.data(), n, walked);
        lj::FlatScene R = lj::rebuild_trees(F, tree, std::vector<int>(walked.begin(), walked.end()), max_depth4);
        lj::commit_rebuild(F, std::move(R));
        refit_host(F);
        *rebuilt = 1;
        return 0;
    } catch (const lj::LjError &e) { return fail(e, err, err_len); }
}

// The padded primitive boxes of a twin's scene by global primitive, what either builder starts from: out[n][2][3]; returns n
int64_t ploc_scene_boxes(void *tv, float *out) {
    const lj::FlatScene &F = ((Twin *)tv)->flat;
    if (out) for (const DPrim &p : F.leaf_prims) refit_prim_box(p, F.spheres.data(), ((RefitBox *)out)[p.gprim]);
    return (int64_t)F.prims.size();
}

// emit_wide on the PLOC tree of n boxes.  The outputs start as sentinels; returns emit_wide's code (0: accepted) and in out[0..3] the sizes
// of nodes, nodes8 and leaf_order and depth4 as the call left them.
int ploc_emit(int64_t n, const float *boxes, int radius, int max_depth4, int64_t *out, char *err, int err_len) {
    std::vector<int32_t> order, walked; std::vector<RebuildNode> raw;
    ploc_host((int)n, (const RefitBox *)boxes, resolve_radius(radius), order, raw);
    const std::vector<lj::BinaryNode> tree = lj::compact_ploc_tree(raw.data(), boxes, order.data(), n, walked);
    std::vector<ljd::DNode4> nodes(3); std::vector<ljd::DNode8> nodes8(5); std::vector<int> leaf_order(7, -9);
    int depth4 = -7, depth8 = -7, rc = 0;
    try { lj::emit_wide(tree, std::vector<int>(walked.begin(), walked.end()), 0, max_depth4, nodes, nodes8, leaf_order, depth4, depth8); }
    catch (const lj::LjError &e) { rc = fail(e, err, err_len); }
    out[0] = (int64_t)nodes.size(); out[1] = (int64_t)nodes8.size(); out[2] = (int64_t)leaf_order.size(); out[3] = depth4;
    return rc;
}

// compact_ploc_tree on raw records from the caller (the refusals of a malformed tree): its code, 0 when accepted
int ploc_compact(int64_t n, const void *raw, const float *boxes, const int32_t *order, char *err, int err_len) {
    std::vector<int32_t> walked;
    try { lj::compact_ploc_tree(raw, boxes, order, n, walked); }
    catch (const lj::LjError &e) { return fail(e, err, err_len); }
    return 0;
}

} // extern "C"
