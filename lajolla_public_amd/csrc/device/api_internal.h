// Internals shared by the translation units that own the GPU.  The entry points, one file per family: api_device.hip (context and scene
// lifetime, upload, camera, BVH read-back, the plain renders, batched ray queries), api_geometry.hip (geometry update, refit, the two BVH
// builders, the build query), api_film.hip (lj_render_features*, lj_render_adaptive*), api_denoise.hip (lj_denoise*) and api_rays.hip
// (tables of rays and probes).  Behind them render.hip (render plans, run_render and its five drivers) and queries.hip (the batched
// per-object queries); the kernel files include this header for their launchers' declarations.
// In order: the launchers of every kernel file; the HIP error boundary, device buffers and developer switches; the context and scene
// objects behind the opaque handles of include/lajolla_hip.h; and what render.hip, api_device.hip and api_geometry.hip offer the
// other files.  The call sequences that the entry points share are in api_calls.h.
#pragma once
#include <hip/hip_runtime.h>
#include "../host/api_common.h"
#include "../host/flatten.h"
#include "dtypes.h"
#include "dconfig.h"
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace ljd {
// kernels.hip (shade_*, launch_shade / _tail / _resolve) and extend.hip (extend_config, max_stack_depth, launch_extend / _aux / _trace_rays)
ShadeConfig shade_config(size_t n_prims, size_t n_materials, size_t n_lights, size_t n_light_tris, size_t n_light_tri_cdf, size_t n_images3, size_t n_images1, size_t n_env_marg);
int shade_variant(uint32_t kinds, bool textured, bool envmap, bool sphere_lights, int preferred = -1);
ExtendConfig extend_config(int n_nodes, int n_prims, int bvh_depth, int n_spheres, int n_nodes8, int bvh8_depth, bool open_scene);
int max_stack_depth();
void launch_extend(const DScene &sc, const DQueue &q, const DBlockState *blocks, uint32_t grid, uint32_t seg, uint32_t *work, const uint32_t *chunk_list, uint32_t parity, const ExtendConfig &cfg, int *spill, unsigned long long *stats, hipStream_t s);
bool shade_sorts_segments(const ShadeConfig &cfg);
void launch_shade(const DScene &sc, const DPass &pass, const DQueue &q, const DQueue &qo, uint32_t *sort_perm, uint8_t *sort_keys, DBlockState *blocks, uint32_t n_blocks, uint32_t seg, const ShadeConfig &cfg, uint32_t *work, uint32_t *chunk_list, uint32_t parity, uint32_t extend_waves, hipStream_t s);
void launch_resolve(const DPass &pass, uint32_t n_pixels, float *rgb, hipStream_t s);
size_t tail_smem(const ExtendConfig &ecfg, const ShadeConfig &scfg);
void launch_tail(const DScene &sc, const DPass &pass, const DQueue &q, DBlockState *blocks, uint32_t n_blocks, uint32_t seg, const ExtendConfig &ecfg, const ShadeConfig &scfg, int *spill, hipStream_t s);
void launch_aux(const DScene &sc, const DPass &pass, uint32_t n_pixels, int integrator, float *rgb, const ExtendConfig &cfg, int *spill, int grid, hipStream_t s);
void launch_volpath(const DScene &sc, const DPass &pass, uint32_t n_samples, uint32_t *counters, const ExtendConfig &cfg, int shade_variant, bool plain, int *spill, int grid, hipStream_t s);
int volpath_blocks_per_cu(const DScene &sc);
void launch_trace_rays(const DScene &sc, const void *rays, long long n, void *hits, unsigned char *occ, const ExtendConfig &cfg, int *spill, int grid, hipStream_t s);
// queries.hip: the first segments (six floats: org, dir) of the n_samples samples of a pass over a table of probes (lj_probe_ray_queries)
void launch_probe_rays(const DScene &sc, const DPass &pass, uint32_t n_samples, float *rays_out, int n_cus, hipStream_t s);
// features.hip: the guide buffers and the variance of a pass (lj_render_features; `want`: the FEAT_* bits of dtypes.h)
int features_grid(uint64_t n_pixels, uint32_t spp, int n_cus);
void launch_features(const DScene &sc, const DPass &pass, uint32_t n_pixels, uint32_t want, float *albedo, float *normal, float *depth, float *alpha, const ExtendConfig &cfg, int *spill, int grid, hipStream_t s);
void launch_resolve_variance(const DPass &pass, uint32_t n_pixels, float *variance, hipStream_t s);
// denoise.hip: the a-trous filter of lj_denoise over `total` = n * w * h pixels; guide / dyn: one denoise_record_bytes() record per pixel.
// (ddenoise.h, the rule, is not included here: it switches floating-point contraction off for the rest of a translation unit.)
struct DenoiseCall { uint32_t has; int32_t iterations; float sigma[4]; };   // has: denoise_has(); iterations and sigma (colour, normal, depth, albedo) as LjDenoiseArgs gives them
uint32_t denoise_has(bool variance, bool albedo, bool normal, bool depth, bool demodulate);
int denoise_max_iterations();
int denoise_iterations(const DenoiseCall &c);   // with the default filled in
size_t denoise_record_bytes();
void launch_denoise_pack(uint32_t has, uint64_t total, const float *rgb, const float *variance, const float *albedo, const float *normal, const float *depth, void *guide, void *dyn, hipStream_t s);
void launch_atrous(const DenoiseCall &c, int n, int w, int h, int iteration, bool lds, const void *guide, const void *dyn_in, void *dyn_out, hipStream_t s);
void launch_denoise_unpack(uint32_t has, uint64_t total, const void *guide, const void *dyn, float *rgb_out, float *variance_out, hipStream_t s);
// adaptive.hip: the kernels of lj_render_adaptive between the renders of its rounds (dadaptive.h, the rule, is not included here either).
// State of a w x h film: n (one word per pixel), mean and m2 (three floats per pixel).  max_grid > 0 caps a launch's workgroups (LJ_TUNE_ADAPTIVE_GRID).
struct AdaptiveCall { uint32_t min_spp, max_spp, round_spp, max_rounds; float target_error; };   // LjAdaptiveArgs with the defaults filled in
int adaptive_resolve(int32_t min_spp, int32_t max_spp, int32_t round_spp, int32_t max_rounds, float target_error, AdaptiveCall &out);   // 0, or what is wrong (dadaptive.h adaptive_params)
uint64_t adaptive_seed(uint64_t seed0, uint32_t round);
int adaptive_max_rounds();
uint32_t adaptive_tiles(uint64_t n_list);   // 256-entry tiles of a list: the words of `counts` and of `offsets`
void launch_adaptive_merge(const uint32_t *list, uint64_t n_list, uint32_t k, bool init, const float *rgb, const float *variance, uint32_t *n, float *mean, float *m2, int n_cus, int max_grid, hipStream_t s);
void launch_adaptive_select(const AdaptiveCall &c, int w, int h, const uint32_t *n, const float *mean, const float *m2, const uint32_t *list, uint64_t n_list,
                            uint8_t *flags, uint32_t *counts, uint32_t *offsets, uint32_t *total, uint32_t *selected, int n_cus, int max_grid, hipStream_t s);
void launch_adaptive_output(uint64_t n_pixels, const uint32_t *n, const float *mean, const float *m2, float *rgb, float *variance, uint32_t *samples, int n_cus, int max_grid, hipStream_t s);
// mega.hip
size_t mega_smem(const DScene &sc, const ShadeConfig &scfg);
int mega_blocks_per_cu(const DScene &sc, const ShadeConfig &scfg);
void launch_mega(const DScene &sc, const DPass &pass, const ShadeConfig &scfg, bool spheres, uint32_t n_samples, uint32_t grab, uint32_t item_cap_tune, uint32_t *sample_counter, unsigned long long *stats, int grid, hipStream_t s);
void launch_trace_rays_scan(const DScene &sc, const void *rays, long long n, void *hits, unsigned char *occ, uint32_t item_cap_tune, int grid, hipStream_t s);
// tile.hip: the per-tile schedule (LJ_RNG_TILE)
size_t tile_cursor_bytes(bool vol);
void launch_tile_init(bool vol, void *cursors, const uint32_t *tiles, uint32_t n_tiles, uint64_t seed, hipStream_t s);
int tile_grid(uint32_t n_tiles, uint32_t lanes);
void launch_tile(bool vol, const DScene &sc, const DTileJob &job, void *cursors, uint32_t lanes, uint32_t budget, uint32_t *alive, const ExtendConfig &cfg, int *spill, hipStream_t s);
void tile_cursor_stats(bool vol, const void *cursors_host, uint32_t n, unsigned long long out[5]);
// refit.hip: the refit of lj_scene_update_geometry (drefit.h); `list`: node indices of one tree level, box4 / box8: one refit_box_bytes() record per node
size_t refit_box_bytes();
void launch_refit4(DNode4 *nodes, void *box4, const DPrim *leaf_prims, const DSphere *spheres, const int32_t *list, int n, hipStream_t s);
void launch_refit8(void *nodes8, int stride, void *box8, const DPrim *leaf_prims, const DSphere *spheres, const int32_t *list, int n, hipStream_t s);
void launch_refit_scan(DScanLeaf *leaves, const DPrim *leaf_prims, const DSphere *spheres, int n, hipStream_t s);
// rebuild.hip: the linear BVH of lj_scene_rebuild_bvh (drebuild.h) over n primitives.  The pieces of one workspace: boxes (six floats per
// primitive), order (sorted position -> primitive) and nodes (n - 1 records of rebuild_node_bytes(), boxes included) are what the host
// reads back; the rest is scratch.  rebuild_carve(null, n, s).bytes is the size to allocate.
struct RebuildWork { void *boxes, *bounds, *codes, *codes_sorted; int32_t *vals, *order; void *nodes; int32_t *parent; void *arrived, *sort_temp; size_t sort_temp_bytes, bytes; };
RebuildWork rebuild_carve(void *workspace, int n, hipStream_t s);
size_t rebuild_node_bytes();
void launch_rebuild_prim_boxes(const DPrim *leaf_prims, int n_leaf_prims, const DSphere *spheres, const RebuildWork &w, int n, hipStream_t s);
void launch_rebuild_order(const RebuildWork &w, int n, hipStream_t s);   // the first half of launch_rebuild: w.order and the sorted codes
void launch_rebuild(const RebuildWork &w, int n, hipStream_t s);
// ploc.hip: the clustering of lj_scene_rebuild_bvh_ex (dploc.h) over the order that launch_rebuild_order leaves; its nodes go to w.nodes, its
// own scratch is a PlocWork carved behind the RebuildWork in the same workspace.  ploc_carve(null, n).bytes is the size to add.
struct PlocWork { void *box[2]; int32_t *id[2], *count[2], *nn; uint8_t *flags; void *counts, *offsets; uint32_t *total; size_t bytes; };
struct PlocRun { uint64_t rounds, tail_rounds; bool finished; };
PlocWork ploc_carve(void *workspace, int n);
PlocRun launch_ploc(const RebuildWork &w, const PlocWork &p, int n, int radius, int tail, uint32_t *host_word, hipStream_t s);
}

using lj::LjError;

#define HIP_CHECK(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) \
    throw LjError(LJ_ERR_DEVICE, std::string(#expr) + " failed: " + hipGetErrorString(_e)); } while (0)

struct DevBuf {
    void *p = nullptr; size_t bytes = 0;
    void alloc(size_t n) { release(); if (n) { HIP_CHECK(hipMalloc(&p, n)); bytes = n; } }
    void release() { if (p) { (void)hipFree(p); p = nullptr; bytes = 0; } }
    ~DevBuf() { release(); }
    DevBuf() = default; DevBuf(const DevBuf &) = delete; DevBuf &operator=(const DevBuf &) = delete;
};

// grow-only workspace: a buffer that already holds `bytes` is left alone
inline void ensure(DevBuf &b, size_t bytes) { if (b.bytes < bytes) b.alloc(bytes); }

// A developer switch: the integer the environment gives `name`, or `dflt` when it is unset.  Read at every call — tests and tools flip
// LJ_TUNE_* between two renders of one process — and clamped where it is used.
inline bool env_set(const char *name) { return getenv(name) != nullptr; }
inline int env_int(const char *name, int dflt) {
    const char *e = getenv(name);
    return e ? atoi(e) : dflt;
}
// LJ_TUNE_MEGA=0: no scene takes the leaf-scan route of mega.hip — a render runs the wavefront kernels, a ray query k_extend's traversal
inline bool mega_enabled() { return env_int("LJ_TUNE_MEGA", 1) != 0; }
// LJ_TUNE_MEGA_ITEM_CAP=n: the leaf scan pools at most n candidates per wave and pass (clamped to [1, the build's pool] by the launchers; 0: unset).
// Read per render and per query: the tests reach several passes per wave-step with it at sizes where the pool would never fill.
inline uint32_t mega_item_cap_tune() { return (uint32_t)std::max(0, env_int("LJ_TUNE_MEGA_ITEM_CAP", 0)); }

// LJ_TUNE_DENOISE_LDS=k: the first k iterations of lj_denoise (steps 1, 2, .. 1 << (k - 1)) filter from a haloed tile in LDS, the others
// gather from global memory; 0: all direct.  Clamped to [0, 3] (step 4: a 64 KiB tile); the default is the measured choice of DESIGN.md §3.8.
static constexpr int kDenoiseLdsDefault = 2, kDenoiseLdsMax = 3;
// LJ_TUNE_ADAPTIVE_GRID=n: at most n workgroups per launch of adaptive.hip (0: the CU-count cap alone) — the tests reach several tiles per
// workgroup with it at small films.  The lists do not depend on it.
inline int adaptive_max_grid() { return std::max(0, env_int("LJ_TUNE_ADAPTIVE_GRID", 0)); }
inline int denoise_lds_iterations() { return std::min(std::max(env_int("LJ_TUNE_DENOISE_LDS", kDenoiseLdsDefault), 0), kDenoiseLdsMax); }

template <typename T> inline void upload(DevBuf &b, const std::vector<T> &v, hipStream_t s) {
    b.alloc(((std::max<size_t>(v.size(), 1) * sizeof(T)) + 31) & ~(size_t)15);
    if (!v.empty()) HIP_CHECK(hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s));
}

static constexpr size_t kQueueSlotBytes = 128;  // eight 16-byte records per path
static constexpr uint32_t kMaxBlocks = 8192;

static constexpr uint32_t kMaxLanes = 8;   // render lanes (streams) a context can run side by side
struct lj_context {
    int device = 0;
    // lifetime: a context outlives its scenes whatever order the caller destroys them in — lj_context_destroy on a context that still
    // has scenes only marks it, and the last lj_scene_destroy releases it
    int live_scenes = 0; bool doomed = false;
    hipStream_t stream = nullptr;
    hipStream_t lane_streams[kMaxLanes - 1] = {};   // further lanes of a render (run_render)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_caller = nullptr;
    int n_cus = 256;
    // workspace, grown on demand and reused across renders
    DevBuf queue_mem; uint32_t queue_capacity = 0;
    DevBuf queue_mem2, sort_perm, sort_keys; uint32_t queue2_capacity = 0;   // segment-sorted shading: the second record set, slot permutation, keys
    DevBuf chunk_counter, chunk_list;  // the extend kernel's work counters and the two lists of live queue chunks
    DevBuf spill;  // overflow levels of the traversal stacks: spill_levels x (grid * 256) ints
    DevBuf blocks, sample_rgb, pixel_list, frame;
    uint64_t pixel_list_key = 0;   // which pixel list `pixel_list` holds (RenderPlan::pixels_key), 0: none
    DevBuf tile_cursors, tile_list, tile_samples;   // the per-tile schedule: one cursor per tile (dtile.h), the tile ids, per-sample radiance
    DevBuf view_table;   // the camera table of a batch (lj_render_views): one DCamera per view, uploaded per call
    DevBuf ray_table, ray_out;   // lj_radiance_rays / lj_irradiance: the table of rays or probes, uploaded per call, and the radiance and variance of its entries
    DevBuf mega_state;   // k_mega: [0] the grid-wide camera-sample counter (uint32), [8..] five 64-bit statistics
    ljd::DBlockState *blocks_host = nullptr;  // pinned, kMaxBlocks entries
    unsigned long long *stats_host = nullptr; // pinned, 8 entries: where a launch's statistics are read back (one wait per pass, no staged copy)
    hipEvent_t ev_begin = nullptr, ev_end = nullptr, ev_k0 = nullptr, ev_k1 = nullptr;
    // lj_render_features: the host variant's five buffers, and the events around a pass's variance and feature launches (recorded in a features call only)
    DevBuf feature_frames;
    hipEvent_t ev_f0 = nullptr, ev_f1 = nullptr, ev_f2 = nullptr;
    // lj_denoise: the packed records (guide; the two dynamic buffers an iteration ping-pongs between), the host variant's inputs and outputs on
    // the device, events of its own around a call's launches, and the last call's statistics (the time is read when they are asked for)
    DevBuf dn_guide, dn_dyn[2], dn_in, dn_out;
    hipEvent_t ev_d0 = nullptr, ev_d1 = nullptr;
    LjDenoiseStats denoise_stats{}; bool denoise_time_pending = false;
    // lj_render_adaptive: the state of the film (n, mean, m2), a round's rgb and variance frames, the call's list and the selected one, the
    // selection's flags and tile counts / offsets / total, the host variant's three outputs, and events around a round's merge and selection
    DevBuf ad_n, ad_mean, ad_m2, ad_rgb, ad_var, ad_list, ad_sel, ad_flags, ad_scan, ad_out;
    hipEvent_t ev_a0 = nullptr, ev_a1 = nullptr, ev_a2 = nullptr;
    DevBuf rebuild_ws;   // lj_scene_rebuild_bvh / lj_bvh_build_query: the workspace of rebuild.hip
};
// the context's timing events (hipEventCreate: they time), which lj_context_create and lj_context_destroy both walk
static constexpr hipEvent_t lj_context::*kTimingEvents[] = {&lj_context::ev_begin, &lj_context::ev_end, &lj_context::ev_k0, &lj_context::ev_k1, &lj_context::ev_f0, &lj_context::ev_f1,
    &lj_context::ev_f2, &lj_context::ev_d0, &lj_context::ev_d1, &lj_context::ev_a0, &lj_context::ev_a1, &lj_context::ev_a2};

struct lj_scene {
    lj_context *ctx = nullptr;
    lj::FlatScene flat;  // host copy (tables for lj_scene_info; arrays already uploaded)
    DevBuf nodes, nodes8, leaf_prims, prims, spheres, materials, lights, light_cdf, light_tris, light_tri_cdf, images3, images1, texels, env_tables;
    DevBuf media, volume_data, shape_media, scan_leaves;
    DevBuf refit_box4, refit_box8, refit_levels4, refit_levels8;   // lj_scene_update_geometry: per-node boxes and the level tables (allocated by the first update)
    ljd::DScene dscene{};
    ljd::ExtendConfig ecfg{};
    ljd::ShadeConfig scfg{};
    uint32_t feat_kinds = 0; bool feat_textured = false, feat_envmap = false, feat_sphere_lights = false;   // what the scene holds (picks scfg.variant)
    std::shared_ptr<const std::vector<uint32_t>> plan_pixels; uint64_t plan_pixels_key = 0;   // the last render plan's pixel list (make_plan)
    std::shared_ptr<const std::vector<uint32_t>> views_pixels; uint64_t views_pixels_key = 0;   // ... and the last batch plan's (make_views_plan)
    std::shared_ptr<const std::vector<uint32_t>> rays_pixels; uint64_t rays_pixels_key = 0;     // ... and the last table's identity list (make_rays_plan)
    std::vector<int64_t> shape_first_gprim;   // global primitive id of each shape's first primitive (shape order, then triangle order)
    LjStats stats{};
    LjFeatureStats feature_stats{};   // of the last lj_render_features* call; zeros after any other render
    LjAdaptiveStats adaptive_stats{};   // of the last lj_render_adaptive* call; zeros after any other render
    LjRebuildStats rebuild_stats{};   // of the last lj_scene_rebuild_bvh
    LjBuildStats build_stats{};       // of the last lj_scene_rebuild_bvh or lj_scene_rebuild_bvh_ex: which builder ran, and its rounds
};

inline void set_device(lj_context *ctx) { HIP_CHECK(hipSetDevice(ctx->device)); }

inline float elapsed_ms(hipEvent_t from, hipEvent_t to) { float ms = 0; HIP_CHECK(hipEventElapsedTime(&ms, from, to)); return ms; }
// closes the timed region that a record of ev_begin opened on `s`: device milliseconds, after a wait for the region's end
inline float close_timer(lj_context *ctx, hipStream_t s) {
    HIP_CHECK(hipEventRecord(ctx->ev_end, s));
    HIP_CHECK(hipEventSynchronize(ctx->ev_end));
    return elapsed_ms(ctx->ev_begin, ctx->ev_end);
}

// ---- render.hip
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
    // a table of rays or probes (lj_radiance_rays / lj_irradiance): `pixels` is the identity list over the table's entries, rays_dev the table
    // on the device (six floats per entry), ray_kind the RAY_SOURCE_* of dtypes.h (none: cameras), ray_spread / ray_medium what the paths start with
    const float *rays_dev = nullptr; uint32_t ray_kind = 0; float ray_spread = 0.0f; int ray_medium = -1;
    // a features request (lj_render_features): device frames of the plan's size, written at the plan's pixels after every pass's resolve;
    // want: the FEAT_* bits (dtypes.h) of the frames that are asked for, 0: none — the render is then exactly lj_render's
    struct Features { uint32_t want = 0; float *albedo = nullptr, *normal = nullptr, *depth = nullptr, *alpha = nullptr, *variance = nullptr; } feat;
};
inline bool timing_requested(const LjRenderArgs *a) { return a && (a->flags & 1u); }   // (LjRenderArgs::flags bit 0: time every kernel)
RenderPlan make_plan(lj_scene *sc, const LjRenderArgs *a);
RenderPlan make_views_plan(lj_scene *sc, const LjRenderArgs *a, int n_views);
RenderPlan make_rays_plan(lj_scene *sc, const LjRenderArgs *a, int64_t n);
void run_render(lj_scene *sc, const RenderPlan &plan, float *rgb_dev, float *samples_host, hipStream_t stream, bool timing);
void run_probe_rays(lj_scene *sc, const RenderPlan &plan, float *rays_host, hipStream_t stream);   // the first segments of a probes plan, pass by pass: rays_host[list position * spp + s][6]
int *ensure_spill(lj_context *ctx, int levels, uint32_t grid);

// ---- api_device.hip and api_geometry.hip (`me`, in every entry-point file: the extern "C" function's name, which its error messages begin with)
bool scene_is_live(const lj_scene *sc);   // an uploaded scene of this process that was not destroyed
void install_trees(lj_scene *sc, hipStream_t s);
void render_frames(lj_scene *scene, RenderPlan plan, const std::vector<ljd::DCamera> &views, float *const dst[6], bool on_device, hipStream_t caller, bool timing);
std::vector<ljd::DCamera> view_table(const lj_scene *scene, int32_t n_views, const LjCamera *views, const std::string &me);
void alloc_refit_tables(lj_scene *scene, hipStream_t s);
void refit_launches(lj_scene *scene, hipStream_t s);
void read_back_nodes(lj_scene *scene, hipStream_t s);
