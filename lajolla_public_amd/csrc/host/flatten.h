// LjSceneDesc -> flat, pointer-free arrays in the device layouts of device/dtypes.h.
// This is the host half of the reference's Scene::Scene (scene.cpp:3-53): bounds sphere, per-mesh area tables,
// envmap table, light table — plus the BVH that replaces rtcCommitScene.  Pure C++ (no HIP), so the CPU test
// suite can check the flattened tables against the golden vectors without a GPU.
#pragma once
#include "../device/dtypes.h"
#include "host_scene.h"
#include <vector>

namespace lj {

struct FlatScene {
    ljd::DCamera cam{};
    std::vector<ljd::DNode4> nodes;
    std::vector<ljd::DNode8> nodes8;   // the same tree eight wide with quantised boxes (trees beyond the extend kernel's LDS image)
    std::vector<ljd::DPrim> leaf_prims;
    std::vector<ljd::DPrimShade> prims;
    std::vector<ljd::DSphere> spheres;
    std::vector<ljd::DMaterial> materials;
    std::vector<ljd::DLight> lights;
    std::vector<float> light_cdf;
    std::vector<ljd::DLightTri> light_tris;
    std::vector<float> light_tri_cdf;
    std::vector<ljd::DImage> images3, images1;
    std::vector<float> texels;
    std::vector<float> env_tables;
    int env_marg_first = 0, env_marg_count = 0;   // the environment map's marginal tables inside env_tables (dtypes.h DScene::env_marg)
    std::vector<ljd::DMedium> media;
    std::vector<float> volume_data;
    std::vector<int32_t> shape_media;
    int n_scan_used = 0;                       // leaves among scan_leaves (the rest pads the table to a multiple of four)
    std::vector<ljd::DScanLeaf> scan_leaves;   // tiny scenes only (else empty): the flat leaf table of device/dscan.h
    int cam_medium = -1, max_null_collisions = 1000, vol_path_version = 0;
    int envmap_light_id = -1, max_depth = -1, rr_depth = 5, spp = 4, integrator = LJ_INTEGRATOR_PATH;
    int bvh_depth = 0, bvh8_depth = 0;
    int64_t n_triangles = 0, n_spheres = 0;
    double bounds_radius = 0, bounds_center[3] = {0, 0, 0}, shadow_epsilon = 0;
    // double-precision tables kept for inspection by tests (scene.cpp:47-52)
    std::vector<double> light_pmf_d, light_cdf_d, light_power_d;
    // ---- what lj_scene_update_geometry needs of the upload (flatten_update below)
    std::vector<int32_t> leaf_order;           // leaf_prims[i] is global primitive leaf_order[i] (the builder's leaf order)
    // level tables of the two trees: the wide nodes grouped by depth (found by walking the stored nodes from the root), root level first;
    // level l is levels[level_first[l] .. level_first[l + 1])
    std::vector<int32_t> levels4, level4_first, levels8, level8_first;
    std::vector<LjShape> shapes_sig;           // the uploaded shapes and (kind, shape_id) of the lights: what an update may not change
    std::vector<int32_t> lights_sig;
    int64_t n_vertices_sig = 0, n_index_triangles_sig = 0;
    uint64_t topology_hash = 0;                // of the index and uv arrays
    std::vector<double> env_total;             // per light: the environment map's table total (its power follows bounds_radius), else 0
    // a DScene whose pointers refer to the vectors above (host memory)
    ljd::DScene host_view() const;
};

// One camera, as flatten_scene treats the scene's: check_camera throws LjError(LJ_ERR_INVALID_ARG) for a matrix or filter parameter that is
// not finite and for a bad film size; flatten_camera is the conversion that fills FlatScene::cam (lj_scene_set_camera and the camera
// table of lj_render_views go through the same two).
void check_camera(const LjCamera &c);
ljd::DCamera flatten_camera(const LjCamera &c);

// Throws LjError(LJ_ERR_UNSUPPORTED) for variant alternatives the device path does not implement.
FlatScene flatten_scene(const LjSceneDesc &d);

// lj_scene_update_geometry, host part.  `prev` is the flattened upload of a description of which `d` may differ in positions, normals and
// each sphere's position / radius only.  Verifies that (counts; per shape kind, ranges, has_normals / has_uvs, material, light and medium
// ids; per light kind and shape_id; the index and uv arrays by their hash; finite numbers; a scene extent inside the BVH8 grid's exponent
// range) and throws LjError(LJ_ERR_INVALID_ARG) otherwise; then re-derives, with the code flatten_scene runs, everything that depends on
// positions: prims, spheres, leaf_prims (in prev's leaf order), light_tris, light_tri_cdf, lights, light_cdf, the double tables, bounds and
// shadow_epsilon.  Reads the shapes, positions, normals, uvs, indices and lights of `d`; ignores camera, options, materials, images, media.
// The result holds those fields only; nothing of `prev` is changed.  commit_update moves them into the scene (the boxes of the trees are
// the caller's to refit: device/drefit.h).
FlatScene flatten_update(const FlatScene &prev, const LjSceneDesc &d);
void commit_update(FlatScene &scene, FlatScene &&update);

// bvh.cpp: grid step exponent of one BVH8 axis, the smallest e >= -126 with 255 * 2^e >= extent; throws beyond 127
int grid_exponent(double extent);

// bvh.cpp — binned-SAH tree with spatial splits (SBVH) over padded float boxes, collapsed to a BVH4; fills nodes (breadth-first)
// and leaf order.
// depth_out = number of inner (wide) levels; a traversal needs at most 3 * depth_out stack entries.
// `tri`: the primitive is the triangle v[0..2] (float vertices as the device tests them) — what a spatial split clips; else
// only its box is known (spheres).  leaf_order lists the primitives of the leaves one leaf after the other; with spatial
// splits a primitive that straddles a split plane is referenced by a leaf on either side, so the list may be longer than `prims`.
struct BuildPrim { float lo[3], hi[3]; float v[3][3]; int tri; };
// nodes8 / depth8_out: the same binary tree collapsed eight wide (DNode8); a traversal of it holds at most depth8_out node groups.
void build_bvh(const std::vector<BuildPrim> &prims, int max_leaf, int max_depth,
               std::vector<ljd::DNode4> &nodes, std::vector<ljd::DNode8> &nodes8, std::vector<int> &leaf_order, int &depth_out, int &depth8_out);

// bvh.cpp — the second half of build_bvh on a binary tree from anywhere (lj_scene_rebuild_bvh hands it the device's linear BVH).
// One node of such a tree (the layout of LjBinaryNode): an inner node has left / right >= 0, a leaf has both < 0 and the primitives
// order[first .. first + count).
struct BinaryNode { float lo[3], hi[3]; int32_t left, right, first, count; };
// Everything from the split of leaves beyond four primitives down: the collapse, BVH8 slots and quantisation, BVH4, both depths.
// max_depth4 > 0: throws LjError(LJ_ERR_UNSUPPORTED) for a BVH4 deeper than that; throws it too at the 24-bit node and 30-bit leaf
// index limits.  The outputs are written after the last check: a refused call leaves them as they were.
void emit_wide(const std::vector<BinaryNode> &tree, const std::vector<int> &order, int root, int max_depth4,
               std::vector<ljd::DNode4> &nodes, std::vector<ljd::DNode8> &nodes8, std::vector<int> &leaf_order, int &depth_out, int &depth8_out);
// The reachable part of the device's radix tree (device/drebuild.h: raw[0] is the root of the n - 1 nodes over n >= 2 sorted primitives,
// a node of at most four primitives is a leaf; n == 1: one leaf), compacted breadth-first from the root (root = 0).
// raw: n - 1 records of 40 bytes (ljd::RebuildNode); boxes: float[6] per primitive; order: sorted position -> primitive.
std::vector<BinaryNode> compact_radix_tree(const void *raw, const float *boxes, const int32_t *order, int64_t n);
// The same of the device's cluster tree (device/dploc.h: raw[n - 2] is the root of the n - 1 nodes, which carry no ranges and may be n
// deep): an iterative left-first depth-first walk from the root gives order_out[p], the primitive at depth-first position p; a node of at
// most four primitives becomes a leaf over its positions with its own box, a single primitive a leaf with the primitive's box (an inner node carries the
// range of positions below it too); nodes are numbered breadth-first from node 0, so everything downstream of compact_radix_tree runs unchanged on (the result, order_out).  Every child
// index is range-checked, every count must be the sum of its children's, and every node and position must be reached once: otherwise
// LJ_ERR_INTERNAL.
std::vector<BinaryNode> compact_ploc_tree(const void *raw, const float *boxes, const int32_t *order, int64_t n, std::vector<int32_t> &order_out);

// lj_scene_rebuild_bvh, host part: from the compacted binary tree over the scene's global primitives (tree leaves index `order`, which
// holds global primitive ids, each once), the trees, leaf order, leaf-ordered primitives (from prev's), level tables and depths of the
// rebuilt scene — those fields only, nothing of `prev` is changed.  Throws what emit_wide throws.  commit_rebuild moves them into the scene.
FlatScene rebuild_trees(const FlatScene &prev, const std::vector<BinaryNode> &tree, const std::vector<int> &order, int max_depth4);
void commit_rebuild(FlatScene &scene, FlatScene &&rebuilt);

} // namespace lj
