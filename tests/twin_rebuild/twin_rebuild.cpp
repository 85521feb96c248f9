// TEST INFRASTRUCTURE — host twin of lj_scene_rebuild_bvh: the build rule of device/drebuild.h run primitive by primitive and node by node
// as rebuild.hip launches it (with std::stable_sort for the order), then the product's compact_radix_tree, rebuild_trees (emit_wide, the
// level tables) and the refit of device/drefit.h.  The twin of the geometry update (tests/twin_refit) is compiled into this library whole:
// a rebuild works on a scene that update created and moved, and is traced and read through the same entry points.  Built only by the test
// suite, never loaded by the product, and not a fallback.
#include "../twin_refit/twin_refit.cpp"
#include "../../lajolla_public_amd/csrc/device/drebuild.h"
#include <algorithm>

namespace {

// The linear BVH over n boxes: order and the raw nodes of the radix tree, as the kernels leave them
void lbvh_host(int n, const RefitBox *boxes, std::vector<int32_t> &order, std::vector<RebuildNode> &nodes) {
    order.resize((size_t)n); nodes.assign((size_t)std::max(n - 1, 0), RebuildNode{});
    if (n <= 0) return;
    double cmin[3], cmax[3];
    for (int k = 0; k < 3; k++) { cmin[k] = INFINITY; cmax[k] = -INFINITY; }
    for (int i = 0; i < n; i++) for (int k = 0; k < 3; k++) { const double c = rebuild_centroid(boxes[i], k); if (c < cmin[k]) cmin[k] = c; if (c > cmax[k]) cmax[k] = c; }
    std::vector<uint64_t> codes((size_t)n), sorted((size_t)n);
    for (int i = 0; i < n; i++) { codes[i] = rebuild_code(boxes[i], cmin, cmax); order[i] = i; }
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return codes[a] < codes[b]; });
    for (int i = 0; i < n; i++) sorted[i] = codes[order[i]];
    if (n < 2) return;
    std::vector<int32_t> parent(2 * (size_t)n, -1);
    for (int i = 0; i < n - 1; i++) {
        RebuildNode &nd = nodes[i];
        rebuild_node(sorted.data(), n, i, nd);
        parent[nd.left < 0 ? n - 1 + ~nd.left : nd.left] = i;
        parent[nd.right < 0 ? n - 1 + ~nd.right : nd.right] = i;
    }
    // the fit, one walk per sorted primitive behind the arrival counters, in position order (the device's lanes run in any order: the
    // second arriver computes a node from both children in left-right order whichever child it came from)
    std::vector<uint32_t> arrived((size_t)n - 1, 0);
    for (int pos = 0; pos < n; pos++) {
        int p = parent[n - 1 + pos];
        while (p >= 0) {
            if (arrived[p]++ == 0) break;
            RefitBox l, r;
            rebuild_child_box(nodes.data(), boxes, order.data(), nodes[p].left, l);
            rebuild_child_box(nodes.data(), boxes, order.data(), nodes[p].right, r);
            rebuild_node_box(nodes[p], boxes, order.data(), l, r);
            p = parent[p];
        }
    }
}

int fail(const lj::LjError &e, char *err, int err_len) {
    if (err && err_len > 0) { strncpy(err, e.what(), err_len - 1); err[err_len - 1] = 0; }
    return e.code;
}

} // namespace

extern "C" {

// lj_bvh_build_query on the host: order[n], nodes (40-byte LjBinaryNode records, capacity `cap`); returns the number of nodes, -1 when cap is too small
int64_t rebuild_build(int64_t n, const float *boxes, int32_t *order_out, void *nodes_out, int64_t cap) {
    std::vector<int32_t> order; std::vector<RebuildNode> raw;
    lbvh_host((int)n, (const RefitBox *)boxes, order, raw);
    const std::vector<lj::BinaryNode> tree = lj::compact_radix_tree(raw.data(), boxes, order.data(), n);
    if ((int64_t)tree.size() > cap) return -1;
    if (n > 0) memcpy(order_out, order.data(), (size_t)n * 4);
    if (!tree.empty()) memcpy(nodes_out, tree.data(), tree.size() * sizeof(lj::BinaryNode));
    return (int64_t)tree.size();
}

// lj_scene_rebuild_bvh on the host, on a twin of refit_create: 0 (rebuilt[0] = 1, or 0 for the no-op of a leaf-scan or empty scene), or the
// LJ_ERR_* code of a refused rebuild (the twin is then exactly as it was).  max_depth4: the traversal stack's levels.
int rebuild_rebuild(void *tv, int max_depth4, int32_t *rebuilt, char *err, int err_len) {
    Twin *t = (Twin *)tv;
    lj::FlatScene &F = t->flat;
    *rebuilt = 0;
    try {
        const int n = (int)F.prims.size();
        if (!F.scan_leaves.empty() || n == 0 || F.leaf_prims.empty()) return 0;
        std::vector<RefitBox> boxes((size_t)n);
        for (const DPrim &p : F.leaf_prims) refit_prim_box(p, F.spheres.data(), boxes[p.gprim]);
        std::vector<int32_t> order32; std::vector<RebuildNode> raw;
        lbvh_host(n, boxes.data(), order32, raw);
        const std::vector<lj::BinaryNode> tree = lj::compact_radix_tree(raw.data(), (const float *)boxes.data(), order32.data(), n);
        lj::FlatScene R = lj::rebuild_trees(F, tree, std::vector<int>(order32.begin(), order32.end()), max_depth4);
        lj::commit_rebuild(F, std::move(R));
        refit_host(F);
        *rebuilt = 1;
        return 0;
    } catch (const lj::LjError &e) { return fail(e, err, err_len); }
}

// bvh_depth, bvh8_depth, leaves of the BVH4, global primitives
void rebuild_info(void *tv, int64_t *out) {
    const lj::FlatScene &F = ((Twin *)tv)->flat;
    out[0] = F.bvh_depth; out[1] = F.bvh8_depth; out[2] = 0; out[3] = (int64_t)F.prims.size();
    for (const DNode4 &nd : F.nodes) for (int k = 0; k < 4; k++) if (nd.lox[k] <= nd.hix[k] && nd.child[k] < 0) out[2]++;
}

// emit_wide on a hand-made chain: `links` inner nodes, each with a one-primitive leaf on the left and the rest of the chain on the right, over
// links + 1 unit boxes in a row.  The outputs start as sentinels; returns emit_wide's code (0: accepted) and in out[0..3] the sizes of nodes,
// nodes8 and leaf_order and depth4 as the call left them.
int rebuild_emit_chain(int links, int max_depth4, int64_t *out, char *err, int err_len) {
    const int n = links + 1;
    std::vector<lj::BinaryNode> tree((size_t)(2 * links + 1));
    std::vector<int> order((size_t)n);
    for (int i = 0; i < n; i++) order[i] = i;
    auto box = [](lj::BinaryNode &b, float x0, float x1) { b.lo[0] = x0; b.hi[0] = x1; b.lo[1] = b.lo[2] = 0.0f; b.hi[1] = b.hi[2] = 1.0f; };
    for (int i = 0; i < links; i++) {   // inner node i at 2 i, its leaf at 2 i + 1, the last leaf at 2 links
        lj::BinaryNode &in = tree[2 * (size_t)i], &lf = tree[2 * (size_t)i + 1];
        box(in, (float)i, (float)n); in.left = 2 * i + 1; in.right = 2 * i + 2; in.first = 0; in.count = 0;
        box(lf, (float)i, (float)i + 1.0f); lf.left = lf.right = -1; lf.first = i; lf.count = 1;
    }
    lj::BinaryNode &last = tree[2 * (size_t)links];
    box(last, (float)links, (float)n); last.left = last.right = -1; last.first = links; last.count = 1;
    std::vector<ljd::DNode4> nodes(3); std::vector<ljd::DNode8> nodes8(5); std::vector<int> leaf_order(7, -9);
    int depth4 = -7, depth8 = -7, rc = 0;
    try { lj::emit_wide(tree, order, 0, max_depth4, nodes, nodes8, leaf_order, depth4, depth8); }
    catch (const lj::LjError &e) { rc = fail(e, err, err_len); }
    out[0] = (int64_t)nodes.size(); out[1] = (int64_t)nodes8.size(); out[2] = (int64_t)leaf_order.size(); out[3] = depth4;
    return rc;
}

} // extern "C"
