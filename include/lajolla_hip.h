/* lajolla_hip.h — C ABI of liblajolla_hip.so: the MI355X (gfx950) drop-in for lajolla's
 * per-pixel-sample hot path.
 *
 * The reference has no FFI layer.  Its de-facto boundary is
 *     Image3 render(const Scene &scene)                      (src/render.h:9, src/render.cpp:155-170)
 * fed by
 *     Scene parse_scene(const fs::path&, const RTCDevice&)   (src/parse_scene.h:9)
 * and, one level down, the two Embree-backed queries
 *     intersect(scene, ray, ray_diff) / occluded(scene, ray) (src/intersection.h:40-47).
 * Each entry point below names the reference interface it replaces.  Everything that crosses this
 * line is a plain pointer, size or POD struct: no C++ types, no torch types, no exceptions.
 *
 * Variant model.  The reference's std::variant alternatives (Shape shape.h:53, Material
 * material.h:102-110, Light light.h:34, Texture texture.h:108, Filter filter.h:45) become tagged PODs
 * with the same alternative order and the same field names, so a maintainer can fill an LjSceneDesc
 * from a reference `Scene` field by field.
 *
 * Numeric convention.  Host-side scene data is double (the reference's Real, lajolla.h:23); the
 * device narrows to float exactly where the reference narrows for Embree (intersection.cpp:15-24,
 * triangle_mesh.inl:11-14) and shades in float (tolerance stated in DESIGN.md).
 */
#ifndef LAJOLLA_HIP_H
#define LAJOLLA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- error codes (flexception.h:8-24 throws; we return) */
enum {
    LJ_OK = 0,
    LJ_ERR_INVALID_ARG = -1,
    LJ_ERR_PARSE = -2,       /* Error("...") sites of parse_scene.cpp / parse_obj.cpp / load_serialized.cpp */
    LJ_ERR_IO = -3,
    LJ_ERR_UNSUPPORTED = -4, /* a variant alternative / integrator the device path does not implement yet: loud, never a CPU fallback */
    LJ_ERR_DEVICE = -5,      /* HIP runtime error or no gfx950 device */
    LJ_ERR_INTERNAL = -6
};
/* Message for the last failing call on this thread ("" if none). */
const char *lj_last_error(void);
const char *lj_version(void);

/* ---------------------------------------------------------------- variant tags (alternative order == reference order) */
enum { LJ_FILTER_BOX = 0, LJ_FILTER_TENT = 1, LJ_FILTER_GAUSSIAN = 2 };                 /* filter.h:45 */
enum { LJ_SHAPE_SPHERE = 0, LJ_SHAPE_TRIMESH = 1 };                                      /* shape.h:53 */
enum { LJ_TEX_CONSTANT = 0, LJ_TEX_IMAGE = 1, LJ_TEX_CHECKERBOARD = 2 };                 /* texture.h:108 */
enum { LJ_LIGHT_AREA = 0, LJ_LIGHT_ENVMAP = 1 };                                         /* light.h:34 */
enum {                                                                                   /* material.h:102-110 */
    LJ_MAT_LAMBERTIAN = 0, LJ_MAT_ROUGHPLASTIC = 1, LJ_MAT_ROUGHDIELECTRIC = 2,
    LJ_MAT_DISNEYDIFFUSE = 3, LJ_MAT_DISNEYMETAL = 4, LJ_MAT_DISNEYGLASS = 5,
    LJ_MAT_DISNEYCLEARCOAT = 6, LJ_MAT_DISNEYSHEEN = 7, LJ_MAT_DISNEYBSDF = 8
};
enum {                                                                                   /* scene.h:14-22 */
    LJ_INTEGRATOR_DEPTH = 0, LJ_INTEGRATOR_SHADING_NORMAL = 1, LJ_INTEGRATOR_MEAN_CURVATURE = 2,
    LJ_INTEGRATOR_RAY_DIFFERENTIAL = 3, LJ_INTEGRATOR_MIPMAP_LEVEL = 4, LJ_INTEGRATOR_PATH = 5,
    LJ_INTEGRATOR_VOLPATH = 6
};

/* Texture<T> (texture.h:76-92).  A Texture<Real> uses value[0]/color1[0] only. */
typedef struct LjTexture {
    int32_t kind;        /* LJ_TEX_* */
    int32_t texture_id;  /* ImageTexture::texture_id: index into LjSceneDesc.images (3-channel) or images1 (1-channel) */
    double value[3];     /* ConstantTexture::value, or CheckerboardTexture::color0 */
    double color1[3];    /* CheckerboardTexture::color1 */
    double uscale, vscale, uoffset, voffset;
} LjTexture;

/* Material (material.h:12-98).  Texture slots, in the reference's field order:
 *   LAMBERTIAN       0 reflectance
 *   ROUGHPLASTIC     0 diffuse_reflectance  1 specular_reflectance   2 roughness        (+eta)
 *   ROUGHDIELECTRIC  0 specular_reflectance 1 specular_transmittance 2 roughness        (+eta)
 *   DISNEYDIFFUSE    0 base_color 1 roughness 2 subsurface
 *   DISNEYMETAL      0 base_color 1 roughness 2 anisotropic
 *   DISNEYGLASS      0 base_color 1 roughness 2 anisotropic                              (+eta)
 *   DISNEYCLEARCOAT  0 clearcoat_gloss
 *   DISNEYSHEEN      0 base_color 1 sheen_tint
 *   DISNEYBSDF       0 base_color 1 specular_transmission 2 metallic 3 subsurface 4 specular 5 roughness
 *                    6 specular_tint 7 anisotropic 8 sheen 9 sheen_tint 10 clearcoat 11 clearcoat_gloss (+eta) */
#define LJ_MAX_TEX_SLOTS 12
typedef struct LjMaterial {
    int32_t kind;  /* LJ_MAT_* */
    int32_t n_tex;
    double eta;    /* internal IOR / external IOR where the alternative has one */
    LjTexture tex[LJ_MAX_TEX_SLOTS];
} LjMaterial;

/* Shape = variant<Sphere, TriangleMesh> (shape.h:26-53).  Mesh arrays live in the scene-wide pools below;
 * indices are mesh-local like the reference's. */
typedef struct LjShape {
    int32_t kind;  /* LJ_SHAPE_* */
    int32_t material_id, area_light_id, interior_medium_id, exterior_medium_id;  /* ShapeBase, -1 = none */
    int32_t has_normals, has_uvs;   /* TriangleMesh::normals.size()>0 / uvs.size()>0 */
    int32_t _pad;
    int64_t first_vertex, n_vertices;     /* into positions / normals / uvs */
    int64_t first_triangle, n_triangles;  /* into indices */
    double position[3];  /* Sphere::position */
    double radius;       /* Sphere::radius */
} LjShape;

/* Light = variant<DiffuseAreaLight, Envmap> (light.h:15-34). */
typedef struct LjLight {
    int32_t kind;      /* LJ_LIGHT_* */
    int32_t shape_id;  /* DiffuseAreaLight::shape_id */
    double intensity[3];
    LjTexture values;  /* Envmap::values */
    double to_world[16], to_local[16];  /* row-major Matrix4x4 (matrix.h) */
    double scale;
} LjLight;

/* Level 0 of a TexturePool image (texture.h:13-19), as the decoders return it (float, image.cpp:44,96):
 * row-major, y=0 at the top, `channels` interleaved.  Mip chains (mipmap.h:25-48) are rebuilt by the consumer. */
typedef struct LjImage {
    int32_t width, height, channels, _pad;
    const float *data;
} LjImage;

/* Camera (camera.h:10-24) + RenderOptions (scene.h:24-31). */
typedef struct LjCamera {
    double cam_to_world[16], world_to_cam[16], sample_to_cam[16], cam_to_sample[16];
    int32_t width, height;
    int32_t filter_kind;  /* LJ_FILTER_* */
    int32_t medium_id;
    double filter_param;  /* Box::width / Tent::width / Gaussian::stddev */
} LjCamera;

/* VolumeSpectrum (volume.h:13-30): a constant, or a grid of RGB values interpolated trilinearly inside [p_min, p_max]. */
typedef enum LjVolumeKind { LJ_VOLUME_CONSTANT = 0, LJ_VOLUME_GRID = 1 } LjVolumeKind;
typedef struct LjVolume {
    int32_t kind;               /* LJ_VOLUME_* */
    int32_t resolution[3];      /* grid: x, y, z */
    double value[3];            /* constant (the medium's scale already applied, volume.h:105-107) */
    double p_min[3], p_max[3], max_data[3];
    double scale;               /* GridVolume::scale (set_scale, volume.h:109-111) */
    const float *data;          /* grid: 3 floats per voxel, x fastest; the file's float32 values (volume.cpp:62-98) */
} LjVolume;

/* Medium (medium.h:10-21) with its PhaseFunction (phase_function.h:10-17). */
typedef enum LjMediumKind { LJ_MEDIUM_HOMOGENEOUS = 0, LJ_MEDIUM_HETEROGENEOUS = 1 } LjMediumKind;
typedef enum LjPhaseKind { LJ_PHASE_ISOTROPIC = 0, LJ_PHASE_HG = 1 } LjPhaseKind;
typedef struct LjMedium {
    int32_t kind;               /* LJ_MEDIUM_* */
    int32_t phase_kind;         /* LJ_PHASE_* */
    double g;                   /* HenyeyGreenstein::g */
    double sigma_a[3], sigma_s[3];   /* homogeneous */
    LjVolume albedo, density;        /* heterogeneous */
} LjMedium;

typedef struct LjRenderOptions {
    int32_t integrator;  /* LJ_INTEGRATOR_* */
    int32_t samples_per_pixel, max_depth, rr_depth, vol_path_version, max_null_collisions;
} LjRenderOptions;

/* The flat mirror of the reference `Scene` *inputs* (scene.h:42-53 constructor arguments).  Derived tables —
 * bounds sphere, per-mesh triangle_sampler, envmap sampling_dist, light_dist (scene.cpp:30-52) — are NOT part of
 * the description: lj_scene_upload builds them, as Scene::Scene does. */
typedef struct LjSceneDesc {
    LjCamera camera;
    LjRenderOptions options;
    int32_t n_shapes, n_materials, n_lights, n_images3, n_images1, envmap_light_id;
    const LjShape *shapes;
    const LjMaterial *materials;
    const LjLight *lights;
    const LjImage *images3;  /* TexturePool::image3s level 0 */
    const LjImage *images1;  /* TexturePool::image1s level 0 */
    int64_t n_vertices, n_triangles;
    const double *positions;  /* 3 per vertex */
    const double *normals;    /* 3 per vertex; garbage where !has_normals */
    const double *uvs;        /* 2 per vertex; garbage where !has_uvs */
    const int32_t *indices;   /* 3 per triangle, mesh-local */
    const char *output_filename;
    int32_t n_media, _pad_media;
    const LjMedium *media;    /* Scene::media (scene.h:66); referenced by LjCamera::medium_id and LjShape::*_medium_id */
} LjSceneDesc;

/* ---------------------------------------------------------------- front end (host only)
 * Replaces parse_scene(path, embree_device) (parse_scene.cpp:1134-1149) up to, not including, Scene::Scene.
 * Same Mitsuba-0.x XML dialect, same std::stof number semantics, same material/shape/light/texture order. */
typedef struct lj_host_scene lj_host_scene;
int lj_parse_scene(const char *xml_path, lj_host_scene **out);
const LjSceneDesc *lj_host_scene_desc(const lj_host_scene *hs);
void lj_host_scene_free(lj_host_scene *hs);

/* ---------------------------------------------------------------- device side */
typedef struct lj_context lj_context;  /* one HIP device + stream + workspace; main.cpp:30 rtcNewDevice analogue */
typedef struct lj_scene lj_scene;      /* device-resident Scene: flattened BVH + tables; scene.cpp:3-53 analogue */

int lj_context_create(int device_id, lj_context **out);
/* Lifetime: scenes keep their context alive.  Destroying a context (or a device group, below) that still has scenes only marks it; the
 * last lj_scene_destroy (lj_group_scene_destroy) releases it — any destruction order is safe, every handle is destroyed exactly once.
 * Not thread-safe: the count of a context's live scenes is a plain field, so lj_scene_upload, lj_scene_destroy and lj_context_destroy on
 * handles of ONE context must be serialised by the caller (as must every other call on one context: it has one stream and one workspace). */
void lj_context_destroy(lj_context *ctx);

/* Replaces Scene::Scene (scene.cpp:3-53): builds the BVH (instead of rtcCommitScene), the bounds sphere,
 * sampling tables and the light table, and uploads everything.  The description may be freed afterwards. */
int lj_scene_upload(lj_context *ctx, const LjSceneDesc *desc, lj_scene **out);
void lj_scene_destroy(lj_scene *scene);

enum {
    LJ_RNG_SAMPLE = 0, /* one pcg32 stream per (pixel, sample): stream = (y*w + x)*spp + s */
    LJ_RNG_TILE = 1    /* the reference's render() schedule (render.cpp:80-96, 125-141): one pcg32 stream per 16x16 tile,
                          stream = ty*ntx + tx (ntx = ceil(w / 16)), initialised with `seed`; each tile consumes its stream pixel by
                          pixel, row-major inside the tile, and sample by sample, every draw of a sample before the next sample's.
                          The only parallelism is across tiles: a fidelity mode, not a fast one.  A crop window renders
                          every tile it touches whole and writes only its own pixels, so they are bit-identical to the same pixels of a
                          full-frame render; LjStats.samples then counts the samples traced outside the window too.  The auxiliary
                          integrators draw nothing: their output is the same in both modes. */
};

typedef struct LjRenderArgs {
    int32_t spp;         /* <=0: RenderOptions::samples_per_pixel */
    int32_t max_depth;   /* INT32_MIN: RenderOptions::max_depth */
    int32_t rng_mode;    /* LJ_RNG_SAMPLE or LJ_RNG_TILE; any other value: LJ_ERR_UNSUPPORTED */
    int32_t rank, world_size; /* render only the 16x16 tiles t = ty*ntx+tx with t % world_size == rank (render.cpp:75-88);
                                 other pixels are written as 0 so a sum over ranks is the full image */
    int32_t crop_x0, crop_y0, crop_x1, crop_y1; /* all 0: full frame; else only pixels in [x0,x1)x[y0,y1) */
    uint32_t pool_paths; /* paths in flight (128 bytes of queue records each, allocated as far as a pass has samples); 0: default = 128 M */
    uint32_t flags;
    uint64_t seed;       /* 0: 0x853c49e6748fea9b (pcg.h:33) */
} LjRenderArgs;

/* Replaces `Image3 render(const Scene&)` (render.h:9; path_render render.cpp:71-101): fills rgb[h][w][3]
 * (row-major, y=0 top, image.h:28-34) with radiance / spp.  Blocking.  `rgb_host` is caller-owned. */
int lj_render(lj_scene *scene, const LjRenderArgs *args, float *rgb_host);
/* Same, but into caller-owned DEVICE memory, ordered on `hip_stream` (a hipStream_t; NULL: no ordering requested): the render
 * starts after everything `hip_stream` holds at the call and `hip_stream` waits for the finished frame before anything enqueued
 * on it later.  (The kernels themselves run on the context's own streams.)  Returns once the render has completed.  This is the
 * hand-off used for the RCCL framebuffer reduce. */
int lj_render_device(lj_scene *scene, const LjRenderArgs *args, float *rgb_device, void *hip_stream);

/* ---- cameras of an uploaded scene
 * Everything lj_scene_upload spends time on (the BVH, the light, environment-map and texture tables) is independent of the camera;
 * these calls move the camera of a scene that is already on the device.
 *
 * lj_camera_look_at: Camera::Camera (camera.cpp:7-21) behind look_at (transform.cpp), exactly as the XML front end builds the camera of a
 * <lookat> sensor: host only.  fov: degrees, the value Camera::Camera takes (the "x" axis fov, i.e. after parse_sensor's fovAxis
 * conversion).  medium_id = -1. */
int lj_camera_look_at(const double origin[3], const double target[3], const double up[3], double fov,
                      int32_t width, int32_t height, int32_t filter_kind, double filter_param, LjCamera *out);

/* Replace the camera of an uploaded scene.  Everything lj_scene_upload derives from the camera is re-derived by the same code; nothing
 * else is rebuilt.  Film size and filter may change.  Later lj_render* / lj_*_queries calls see the new camera. */
int lj_scene_set_camera(lj_scene *scene, const LjCamera *camera);

/* ---- moving geometry of an uploaded scene
 * The uploaded scene with its vertices moved: re-derives everything lj_scene_upload derives from positions, normals and sphere
 * position / radius — by the same code — and refits the boxes of the BVH4, the BVH8 and the tiny-scene leaf table on the device.
 * The trees' topology, leaf order, mip pyramids, environment-map tables, materials, media, camera and kernel plan are kept.
 *
 * desc is the description that was uploaded, in which only `positions`, `normals` and each sphere's `position` / `radius` may differ.
 * The call reads again what the geometry and light sections of the upload read — shapes, positions, normals, uvs, indices and lights —
 * and IGNORES camera, options, materials, images and media.  Checked, LJ_ERR_INVALID_ARG otherwise: n_shapes, n_vertices, n_triangles,
 * n_lights; per shape kind, vertex and triangle range, has_normals / has_uvs, material, light and medium ids; per light kind and
 * shape_id; the index and uv arrays (by a 64-bit hash kept at upload); finite positions, normals, sphere centres and radii; a scene
 * extent inside the BVH8 grid's exponent range.  Every check runs on the host before the first device write: a refused call leaves the
 * scene exactly as it was.
 *
 * Closest hits are the minimum of (t, global primitive id) over everything a ray tests, so they do not depend on the tree: hits and
 * per-sample radiance after an update are bit-identical to those of a fresh lj_scene_upload of the same description.  What a refit costs
 * is tree quality (a tree built for the old positions; leaves that spatial splits had clipped get their primitives' whole boxes), i.e.
 * render time — never a hit.
 *
 * Blocking, ordered on the context's stream: later lj_render*, lj_render_views*, lj_intersect / lj_occluded and lj_*_queries calls see the
 * new geometry, lj_scene_info the new bounds and shadow_epsilon.  lj_get_stats after the call: render_ms = the update's device time,
 * generate_ms = the host time of the re-derivation.  Device groups: apply the update to each lj_group_scene_member. */
int lj_scene_update_geometry(lj_scene *scene, const LjSceneDesc *desc);

/* ---- rebuilding the trees of a moved scene
 * Rebuilds the BVH4 and the BVH8 of an uploaded scene for the geometry that is on the device now, after any number of
 * lj_scene_update_geometry calls: a linear BVH (Morton order of the padded primitive boxes, Karras' radix tree, leaves of at most four
 * primitives) built on the device, collapsed into the two wide trees by the code lj_scene_upload runs, then refitted by the kernels of
 * lj_scene_update_geometry — so the stored boxes are by definition the refit of the new topology, and a later update with unchanged
 * positions changes no byte.
 * Kept: primitive records, light tables, materials, media, camera, mip pyramids, shade configuration.  Replaced: both trees, the
 * leaf-ordered primitives and the leaf order (now a permutation of the primitives: a linear BVH has no split references), the refit
 * level tables, both depths.  Recomputed: the extend kernels' launch plan, by the function lj_scene_upload calls — it reads LJ_TUNE_*
 * again, as at upload (LJ_TUNE_BVH8, LJ_TUNE_NODE8_STRIDE, LJ_TUNE_REFILL, LJ_TUNE_MINDESC: keep them set across both calls).
 * lj_scene_info, lj_scene_read_bvh and a later lj_scene_update_geometry see the new trees.  Hits and per-sample radiance do not depend on
 * the tree (see above): after a rebuild they are bit-identical to a fresh lj_scene_upload of the same description.
 *
 * A scene with a leaf table (at most 32 leaves and 256 primitives: every ray tests every leaf box, there is no tree to degrade, and the
 * underfilled leaves of a linear BVH would push the scene out of that plan) and an empty scene are left untouched: the call returns
 * LJ_OK with LjRebuildStats::rebuilt = 0.
 *
 * LJ_ERR_INVALID_ARG: a null scene or one that is not live.  LJ_ERR_UNSUPPORTED: the emitted BVH4 is deeper than the traversal stack
 * (40 levels), or the 24-bit node / 30-bit leaf index limits are hit.  Every check runs before the first write to the scene: a refused
 * call leaves it as it was.
 * Blocking, ordered on the context's stream.  lj_get_stats after the call: render_ms = device time, generate_ms = host time, every
 * other field 0.
 *
 * Refit, rebuild or re-upload (measured, DESIGN.md sections 3.10 and 3.12: 60 K - 66 K triangles, 16 spp, one MI355X): an update costs
 * 4 - 5 ms, update plus rebuild 12 - 15 ms with either builder of lj_scene_rebuild_bvh_ex, a re-upload 340 - 790 ms; a frame on the refitted
 * tree takes 1.4 - 5.7 times the freshly built tree's time, on the linear builder's tree 1.15 - 1.56 times, on LJ_BUILD_PLOC's 1.11 - 1.43
 * times (5 - 8 % below the linear builder's on sponza, 0 - 4 % on disney_bsdf).  So: refit alone for a scene with a leaf table (nothing else
 * happens anyway) and for a pose that is rendered for less than the rebuild's 8 - 10 ms; rebuild after the update whenever more than that is
 * rendered per pose — it paid for itself within one 16-spp frame in every case measured, at amplitude 0 too, because it also sheds what the
 * first refit lost (the clipping of the upload's split leaves) — and with LJ_BUILD_PLOC where triangle sizes are mixed, as it costs no more;
 * re-upload only for a pose that is rendered for seconds, where the last 11 - 43 % are still worth half a second of host time. */
int lj_scene_rebuild_bvh(lj_scene *scene);
/* Of the scene's last lj_scene_rebuild_bvh (zeros before the first): rebuilt 1 or 0 (the no-op above); primitives, leaves, nodes and
 * depths of the trees as they stand; build_ms = the device's linear BVH (boxes, codes, sort, hierarchy, fit) and its readback,
 * emit_ms = the host's collapse into the wide trees and level tables, refit_ms = upload of the trees and the refit launches. */
typedef struct LjRebuildStats { uint64_t rebuilt, n_prims, n_leaves, n_nodes4, n_nodes8; int32_t depth4, depth8;
                                double build_ms, emit_ms, refit_ms; } LjRebuildStats;
int lj_get_rebuild_stats(const lj_scene *scene, LjRebuildStats *out);
/* Test hook, a pure function on a context: the device's linear BVH over n boxes (float[n][2][3]: lo, hi; finite, lo <= hi, else
 * LJ_ERR_INVALID_ARG).  order_out[n]: sorted position -> box.  nodes_out: the reachable nodes, breadth-first from the root (node 0); an
 * inner node has left / right >= 0, a leaf has both -1 and holds order_out[first .. first + count), count <= 4.  *n_nodes = their number
 * (0 for n = 0); nodes_out may be null to ask for it, else capacity (in nodes) must hold them. */
typedef struct LjBinaryNode { float lo[3], hi[3]; int32_t left, right, first, count; } LjBinaryNode;   /* 40 bytes */
int lj_bvh_build_query(lj_context *ctx, int64_t n, const float *boxes, int32_t *order_out, LjBinaryNode *nodes_out, int64_t capacity, int64_t *n_nodes);

/* ---- the same with a choice of builder
 * LJ_BUILD_LBVH is lj_scene_rebuild_bvh itself, byte for byte.  LJ_BUILD_PLOC replaces the radix tree by parallel locally-ordered
 * clustering (Meister & Bittner, TVCG 2018) over the same Morton order: in rounds, every cluster merges with the neighbour within `radius`
 * positions that gives the smallest union box, until one is left; a cluster of at most four primitives becomes a leaf.  It looks at the boxes
 * it joins, which the linear BVH never does, so its trees are cheaper to traverse where triangle sizes are mixed; it takes 50 - 70 rounds where
 * the radix tree takes one launch, and was no slower per rebuild where measured (its trees have fewer leaves to emit).  radius: PLOC only; <= 0: 8; at most 32.  args NULL or zeroed: lj_scene_rebuild_bvh.
 * Everything lj_scene_rebuild_bvh documents holds: the no-op for a scene with a leaf table and an empty one, every check before the first
 * write, blocking, LjStats and LjRebuildStats (build_ms covers the clustering), LJ_TUNE_* read again.  Further refusals:
 * LJ_ERR_INVALID_ARG for an unknown builder or a radius above 32; LJ_ERR_UNSUPPORTED when 256 rounds of clustering leave more than 1024
 * clusters (the measured scenes take 19 - 25 to get there; boxes nested inside each other along the whole Morton curve would not) — use the
 * linear builder for such a scene; nothing is written. */
enum { LJ_BUILD_LBVH = 0, LJ_BUILD_PLOC = 1 };
typedef struct LjRebuildArgs { int32_t builder; int32_t radius; } LjRebuildArgs;
int lj_scene_rebuild_bvh_ex(lj_scene *scene, const LjRebuildArgs *args);
/* lj_bvh_build_query with the builder of args.  With LJ_BUILD_PLOC, order_out is the primitives in the depth-first order of the
 * cluster tree (a leaf still holds order_out[first .. first + count)). */
int lj_bvh_build_query_ex(lj_context *ctx, const LjRebuildArgs *args, int64_t n, const float *boxes, int32_t *order_out,
                          LjBinaryNode *nodes_out, int64_t capacity, int64_t *n_nodes);
/* Of the scene's last rebuild by either call (zeros before the first, and after the no-op): the builder and radius that ran (radius 0 for
 * LJ_BUILD_LBVH), the rounds of clustering in all, how many of them ran in the single-workgroup tail launch, and the host time of the builder's
 * launches from the centroid bounds to the last round, which build_ms includes. */
typedef struct LjBuildStats { int32_t builder, radius; uint64_t rounds, tail_rounds; double cluster_ms; } LjBuildStats;
int lj_get_build_stats(const lj_scene *scene, LjBuildStats *out);

/* Readback of an acceleration structure as it stands on the device, for tests: which = 0 the BVH4 (128-byte DNode4 records), 1 the BVH8
 * (80-byte DNode8 records, packed whatever their stride on the device), 2 a tiny scene's leaf table (32-byte DScanLeaf records; none for
 * other scenes).  *bytes = the size of the structure; out_host may be null to ask for it, else capacity_bytes must hold it. */
int lj_scene_read_bvh(const lj_scene *scene, int32_t which, void *out_host, int64_t capacity_bytes, int64_t *bytes);

/* n_views renders of the scene in one pass: rgb[n_views][h][w][3].  Every view must have the scene camera's width, height, filter_kind,
 * filter_param and medium_id (else LJ_ERR_INVALID_ARG); cam_to_world and sample_to_cam are per view.  View v is bit-identical to
 * lj_render of the same scene uploaded with views[v] and the same args: the batch is rendered as one frame of n_views * h rows whose
 * pcg32 streams are those of the pixel inside its view, (y*w + x)*spp + s.
 * args: spp, max_depth, seed, pool_paths and flags as for lj_render; rank / world_size and the crop window apply to every view (pixels
 * outside the share or window are 0, so the sum over ranks of a batch is the full batch); rng_mode must be LJ_RNG_SAMPLE (LJ_RNG_TILE:
 * LJ_ERR_UNSUPPORTED).  All integrators.  LJ_ERR_INVALID_ARG: n_views <= 0, NULL pointers, a matrix that is not finite,
 * n_views * w * h > 2^31.  lj_get_stats afterwards reports the sums over all views.  (Device groups have no batched call.) */
int lj_render_views(lj_scene *scene, const LjRenderArgs *args, int32_t n_views, const LjCamera *views, float *rgb_host);
/* Same, into caller-owned DEVICE memory; ordering on `hip_stream` as lj_render_device. */
int lj_render_views_device(lj_scene *scene, const LjRenderArgs *args, int32_t n_views, const LjCamera *views,
                           float *rgb_device, void *hip_stream);

/* ---- guide buffers beside the image
 * What lj_render / lj_render_views render for the same arguments, and from the same camera samples up to five more buffers: the first-hit
 * albedo, shading normal, depth and coverage, and the variance of the image.  One upload, one BVH; anti-aliased like the image.
 * LJ_RNG_SAMPLE and the path / volpath integrators only.
 *
 * Sample s of pixel p uses the camera sample of every path kernel: pcg32 stream (pixel * spp + s) — the pixel inside its view for a batch —
 * of the call's seed, first draw jy, second draw jx, the ray from the camera's origin with tnear = 0.
 *   First surface: the closest hit of that ray.  A hit on a shape without a material (a medium boundary) is passed through: the ray goes
 *   on from the float hit position in the same direction with tnear = LjSceneInfo.shadow_epsilon and tfar = inf.  A sample traces at most 16
 *   such segments; one whose 16th still ends on a boundary is a miss.  The vertex of the final hit is the one lj_vertex_queries computes for
 *   its segment (ray_spread = the camera's), so after a crossing the texture footprint comes from the last segment only.
 *   Per sample, on a hit: a = the material's slot-0 texture as a Spectrum at the vertex uv and footprint ((1,1,1) for disneyclearcoat, whose
 *   slot 0 is a Real); n = the vertex's shading normal (world space, not flipped, not renormalised); d = |position - camera origin|; hit = 1.
 *   On a miss all four are 0.
 *   Per pixel: albedo = sum a / spp, normal = sum n / spp, alpha = sum hit / spp, depth = sum d / sum hit (0 without a hit), rgb as lj_render,
 *   variance[c] = sum_s (x_sc - rgb[c])^2 / (spp (spp - 1)) over the per-sample radiance x (what lj_render_samples returns) — the squared
 *   standard error of rgb, computed in two passes; 0 when spp == 1.
 *   All sums are float sums in a fixed order that depends on spp alone: results are bit-identical from call to call, for any
 *   crop, share, pass size, pool size, and between a view of a batch and the single-camera call.
 *
 * rgb is bit-identical to lj_render / lj_render_views of the same arguments, and lj_get_stats afterwards is what that call would have
 * left, except that render_ms also covers the extra launches.  Pixels outside the rank's share or the crop window are 0 in every buffer,
 * so the ranks' buffers add up to the full ones.  Nothing is launched for a buffer that is not asked for.
 * LJ_ERR_UNSUPPORTED: rng_mode LJ_RNG_TILE; a scene with one of the five auxiliary integrators.  LJ_ERR_INVALID_ARG: a NULL LjFeatureBuffers
 * or one with all six pointers NULL; n_views < 0; n_views > 0 without views, or views with n_views == 0; everything lj_render_views checks
 * of the views.  A refused call writes nothing.  (Device groups have no features call: render on each lj_group_scene_member.) */
typedef struct LjFeatureBuffers {      /* any pointer may be NULL: not wanted */
    float *rgb;       /* [n][h][w][3] */
    float *albedo;    /* [n][h][w][3] */
    float *normal;    /* [n][h][w][3] */
    float *depth;     /* [n][h][w]    */
    float *alpha;     /* [n][h][w]    */
    float *variance;  /* [n][h][w][3] */
} LjFeatureBuffers;
/* n_views == 0 and views == NULL: the scene's own camera (n = 1); else as lj_render_views.  Blocking; host pointers. */
int lj_render_features(lj_scene *scene, const LjRenderArgs *args, int32_t n_views, const LjCamera *views, const LjFeatureBuffers *out_host);
/* Same, into caller-owned DEVICE memory; ordering on `hip_stream` as lj_render_device. */
int lj_render_features_device(lj_scene *scene, const LjRenderArgs *args, int32_t n_views, const LjCamera *views,
                              const LjFeatureBuffers *out_device, void *hip_stream);
/* Of the last lj_render_features* call on the scene (zeros after any other render): device time of the guide-buffer and of the variance
 * launches, camera samples the guide-buffer kernel traced (segments after a crossing are not counted) and its launches (one per pass). */
typedef struct LjFeatureStats { double features_ms, variance_ms; uint64_t feature_rays, feature_launches; } LjFeatureStats;
int lj_get_feature_stats(const lj_scene *scene, LjFeatureStats *out);

/* ---- Denoising: an edge-stopping a-trous filter over the buffers of lj_render_features.  A pure image operation on a context: no
 * scene, no BVH, no render plan.  The rule — taps, weights, order of the float sums — is spelled out in csrc/device/ddenoise.h (shared by
 * the kernels and a host twin, which agree bit for bit) and in DESIGN.md 3.8.  In short: `iterations` passes with step 1, 2, 4, ..., each a
 * 5 x 5 B3-spline stencil whose weights are multiplied by max(0, 1 - x)^2 stopping terms on the normal, relative depth, albedo and — scaled
 * by the 3 x 3-prefiltered variance — the colour difference of centre and tap; the variance is filtered with the squared weights.
 * in: n images of height x width, laid out as LjFeatureBuffers says.  rgb is required; variance, albedo, normal and depth are optional
 * (NULL: that stopping term is left out); alpha is not read.  INPUTS MUST BE FINITE: the library does not scan them.
 * LJ_DENOISE_DEMODULATE (needs albedo): the filter runs on rgb / (albedo + 1e-3) and multiplies the result back.
 * rgb_out: [n][h][w][3], may be in->rgb (every input is read before anything is written); variance_out (may be NULL; needs in->variance):
 * the filtered variance.  Results are bit-identical from call to call, for the host and the device variant and for any LJ_TUNE_* setting.
 * LJ_ERR_INVALID_ARG: NULL ctx, in, in->rgb or rgb_out; n, width or height <= 0; n * width * height > 2^31; iterations > 8; a sigma that is
 * negative or not finite; LJ_DENOISE_DEMODULATE without in->albedo; variance_out without in->variance.  A refused call writes nothing. */
enum { LJ_DENOISE_DEMODULATE = 1 };
typedef struct LjDenoiseArgs {         /* every field: <= 0 (flags: 0) for the default */
    int32_t iterations;                /* default 5, at most 8 */
    uint32_t flags;                    /* LJ_DENOISE_* */
    float sigma_color, sigma_normal, sigma_depth, sigma_albedo;   /* defaults 4, 0.5, 0.1, 0.25 */
} LjDenoiseArgs;
/* Blocking; host pointers.  args NULL: the defaults. */
int lj_denoise(lj_context *ctx, int32_t n, int32_t width, int32_t height, const LjFeatureBuffers *in_host,
               const LjDenoiseArgs *args, float *rgb_out_host, float *variance_out_host);
/* Same on caller-owned DEVICE memory of the context's device; ordering on `hip_stream` as lj_render_device — the buffers that
 * lj_render_features_device filled on that stream can be passed straight on. */
int lj_denoise_device(lj_context *ctx, int32_t n, int32_t width, int32_t height, const LjFeatureBuffers *in_device,
                      const LjDenoiseArgs *args, float *rgb_out_device, float *variance_out_device, void *hip_stream);
/* Of the last lj_denoise* call on the context (it waits for that call's launches): their device time, their number (iterations + 2:
 * pack, one per iteration, unpack) and n * width * height.  A scene's LjStats is not touched by a denoise call. */
typedef struct LjDenoiseStats { double denoise_ms; uint64_t launches, pixels; } LjDenoiseStats;
int lj_get_denoise_stats(const lj_context *ctx, LjDenoiseStats *out);

/* ---- Adaptive sampling: samples where the error is.  The render runs in rounds: round 0 gives every pixel of the call's share min_spp
 * samples; after each round the pixels whose relative error — the largest variance of the mean in their 3 x 3 neighbourhood over their squared
 * brightness — still exceeds target_error^2, and that have room below max_spp, get round_spp more.  The rule — state, merge, error, selection,
 * seeds, order of the float operations — is spelled out in csrc/device/dadaptive.h (shared by the kernels and a host twin, which agree bit
 * for bit) and in DESIGN.md 3.9.  Round r renders its list with seed_r = seed + r * 0x9e3779b97f4a7c15 (0 becomes 1) and streams
 * pixel * k_r + s, so it yields at each listed pixel what lj_render_features(spp = k_r, seed = seed_r) yields there.
 * Outputs: rgb = the mean over all of a pixel's samples, variance = its squared standard error (0 below two samples), samples = how many it
 * got; albedo, normal, depth, alpha: the guide buffers of round 0, bit-identical to lj_render_features at spp = min_spp — lj_denoise takes
 * an adaptive result as it is.  Pixels outside the rank's share or the crop window are 0 in every buffer.
 * args: max_depth, seed, rank / world_size, the crop window, pool_paths and flags as for lj_render; spp is ignored.
 * Results are bit-identical from call to call, for any pass size, pool size and kernel plan, and between the host and the device variant.
 * NOT promised past round 0: invariance under crop or share (the neighbourhood at a share's border differs from the full frame's).
 * One camera, one device: no camera batches and no device groups (render on each lj_group_scene_member).
 * LJ_ERR_UNSUPPORTED: rng_mode LJ_RNG_TILE; a scene with one of the five auxiliary integrators.  LJ_ERR_INVALID_ARG: a NULL
 * LjAdaptiveBuffers or one with all seven pointers NULL; min_spp == 1; max_spp < min_spp; an spp above 2^20; max_rounds > 64; a target_error
 * that is negative or not finite.  A refused call writes nothing. */
typedef struct LjAdaptiveArgs {        /* every field: <= 0 for the default; NULL args: all defaults */
    int32_t min_spp;                   /* samples of round 0; default 16, must not be 1 */
    int32_t max_spp;                   /* no pixel gets more; default 16 * min_spp, at least min_spp, at most 2^20 */
    int32_t round_spp;                 /* samples of a later round; default min_spp */
    int32_t max_rounds;                /* renders of a call, round 0 included; default 16, at most 64 */
    float target_error;                /* relative standard error to reach; default 0.05; finite, not negative */
} LjAdaptiveArgs;
typedef struct LjAdaptiveBuffers {     /* any pointer may be NULL: not wanted */
    float *rgb;         /* [h][w][3] */
    float *variance;    /* [h][w][3] */
    uint32_t *samples;  /* [h][w]    */
    float *albedo;      /* [h][w][3] */
    float *normal;      /* [h][w][3] */
    float *depth;       /* [h][w]    */
    float *alpha;       /* [h][w]    */
} LjAdaptiveBuffers;
/* Blocking; host pointers. */
int lj_render_adaptive(lj_scene *scene, const LjRenderArgs *args, const LjAdaptiveArgs *adaptive, const LjAdaptiveBuffers *out_host);
/* Same, into caller-owned DEVICE memory; ordering on `hip_stream` as lj_render_device.  (The call waits once per round, for the length of
 * the next list.) */
int lj_render_adaptive_device(lj_scene *scene, const LjRenderArgs *args, const LjAdaptiveArgs *adaptive, const LjAdaptiveBuffers *out_device,
                              void *hip_stream);
/* Of the last lj_render_adaptive* call on the scene (zeros after any other render): the renders it ran (round 0 included), the samples it
 * traced, the length of each round's list, and the device time of the selection and of the merge launches over all rounds.
 * lj_get_stats after an adaptive call returns the field-wise sums over the rounds' renders. */
typedef struct LjAdaptiveStats { uint64_t rounds, samples; uint64_t round_pixels[64]; double select_ms, merge_ms; } LjAdaptiveStats;
int lj_get_adaptive_stats(const lj_scene *scene, LjAdaptiveStats *out);
/* Test hook: the selection of one round on caller-supplied state of a width x height film — n[h][w], mean[h][w][3], m2[h][w][3] as
 * dadaptive.h defines them — over pixel_list[n_list] (film pixel indices y * width + x, each at most once), by the very select, scan and
 * scatter launches a render's rounds run.  selected_out: room for n_list entries; *n_selected: how many were written.  A pure image
 * operation on a context, like lj_denoise.  Host pointers; blocking.  LJ_ERR_INVALID_ARG: NULL pointers, width or height <= 0, more than
 * 2^31 pixels, n_list < 0 or above 2^31, a listed pixel outside the film, arguments lj_render_adaptive refuses. */
int lj_adaptive_select_query(lj_context *ctx, int32_t width, int32_t height, const uint32_t *n, const float *mean, const float *m2,
                             const LjAdaptiveArgs *adaptive, const uint32_t *pixel_list, int64_t n_list, uint32_t *selected_out, int64_t *n_selected);

/* ---- Radiance along given rays, irradiance at surface points: the integrator of lj_render started from a table of rays instead of a camera
 * (lightmap texels, irradiance probes, a reflection gather, a validation ray through a medium).  DESIGN.md 3.11, csrc/device/dprobe.h.
 *
 * lj_radiance_rays.  Ray i, sample s of spp is one path whose first segment is (org_i, dir_i), traced exactly as the integrator traces a
 * camera ray: tnear = 0 and tfar = inf for the path integrator and for volpath versions 1 and 2, tnear = LjSceneInfo.shadow_epsilon for the
 * full volpath (its camera rays start there as well).  Origins are used as given: callers who start on a surface offset them themselves,
 * by LjSceneInfo.shadow_epsilon along the normal as lj_irradiance does.  Directions must be unit vectors.
 *   The path draws from pcg32 stream i * spp + s of args->seed, and THE FIRST TWO DRAWS OF THE STREAM ARE TAKEN AND DISCARDED: they are the
 *   two a camera sample spends on its jitter (jy, jx).  From there the path is what path_tracing() / vol_path_tracing() make of a camera ray:
 *   emission seen directly at the first hit is included; max_depth, rr_depth and the scene's volpath version apply as for lj_render.
 *   Consequence: let ray p * k + s be camera sample (pixel p, sample s) of a k-spp render — origin the camera's, direction that of
 *   lj_primary_ray_queries with the sample's jitter — and trace the table with spp = 1, the same seed and max_depth: the result is bit for
 *   bit what lj_render_samples returns for that sample, whichever kernel plan rendered it.
 *   path:    ray_spread seeds the RayDifferential spread of the first segment (texture footprints); medium_id is not used.
 *   volpath: the path starts in medium_id with spread 0, as its camera samples do; ray_spread is not used.
 *   radiance[i] is the float sum of ray i's spp samples in the order lj_render's resolve sums a pixel's, times 1 / spp; variance[i] the
 *   squared standard error of that mean by the two-pass formula of lj_render_features (0 when spp == 1); samples the raw per-sample values.
 *   Results are bit-identical from call to call and for any pool_paths / pass size, and prefix-stable: ray i's outputs depend only on
 *   (rays[i], i, spp, seed, max_depth), so the first m rays of a call give what a call with only those m gives.
 *   A tiny scene, whose renders run the fused persistent kernel, takes the wavefront kernels for these calls (same per-sample values).
 *   What a ray costs against a pixel sample (one MI355X, device time, the camera's own 16 samples per pixel fed back as rays):
 *   cbox 512 x 512: 1202 Msamples/s against lj_render's 3474 (2.9 times the time: the wavefront plan against the fused kernel);
 *   disney_bsdf 683 x 512: 526 against 549 (1.04 times).  The blocking call adds the upload, the host-side check and the read-back of the table:
 *   ~30 ns of wall time per ray.  lj_get_stats afterwards is what a render of n * spp samples leaves.
 * args: spp (<= 0: the scene's samples per pixel), max_depth, seed, pool_paths and flags as for lj_render.
 * LjRaysArgs: NULL, or a zero-initialised struct, means all defaults — a field is read only when its LJ_RAYS_HAS_* bit is set in `flags`, so
 * that zeroed memory never means "medium 0".
 * LJ_ERR_UNSUPPORTED: rng_mode LJ_RNG_TILE; a scene with one of the five auxiliary integrators.
 * LJ_ERR_INVALID_ARG: NULL scene / table / buffers, or buffers with all three pointers NULL; n < 0 or n > 2^31 (a list entry is 32 bits wide,
 *   as for a batch of cameras); spp > 2^20 (n * spp itself is not bounded: a call runs in passes of at most 2^27 samples, whose sample ids
 *   are 32 bits wide, and streams are 64 bits wide); rank / world_size other than 0 / 0-or-1, or a non-zero crop; an unknown flag; a
 *   medium_id that is neither LJ_RAYS_CAMERA_MEDIUM nor in [-1, n_media); a ray_spread that is not finite; a ray that is not finite, or
 *   whose | |dir| - 1 | exceeds 1e-4 (a float-normalised direction is off by ~1e-7).  The message names the first offending index.
 * Every check runs on the host before the first device write: a refused call writes nothing.  n == 0 returns LJ_OK and launches nothing.
 * All three calls block, take host pointers and are ordered on the context's stream.
 *
 * lj_irradiance.  Probe i, sample s, stream i * spp + s; here the two leading draws are USED: u0 is the first, u1 the second.
 *   dir = to_world(make_frame(normal), sample_cos_hemisphere(u0, u1)) — the device functions the Lambertian's sample_bsdf calls, composed
 *   the way it composes them, so a probe's ray is what a Lambertian surface at that point would have sampled — and
 *   org = position + shadow_epsilon * normal in float.  Everything after that is the rule above with that ray.
 *   radiance[i] = pi_f * mean_i and variance[i] = pi_f * pi_f * var_i (pi_f = 3.14159274f), one float multiply each: the cosine-weighted
 *   estimator of E = integral of L cos(theta) over the hemisphere.  samples are the raw L values.  Normals are validated like directions.
 * lj_probe_ray_queries (a test hook) returns exactly the (org, dir) the kernel builds, rays_out[i * spp + s]: fed to lj_radiance_rays at
 *   spp = 1 with the same seed they reproduce lj_irradiance's samples bit for bit. */
typedef struct LjRadianceRay { float org[3]; float dir[3]; } LjRadianceRay;          /* 24 bytes */
typedef struct LjProbe       { float position[3]; float normal[3]; } LjProbe;        /* 24 bytes */
#define LJ_RAYS_CAMERA_MEDIUM INT32_MIN
enum { LJ_RAYS_HAS_MEDIUM = 1, LJ_RAYS_HAS_SPREAD = 2 };
typedef struct LjRaysArgs {            /* NULL or all zero: all defaults */
    int32_t medium_id;                 /* read with LJ_RAYS_HAS_MEDIUM only.  volpath: the medium the origins lie in, -1: none;
                                          LJ_RAYS_CAMERA_MEDIUM, and the default: the scene camera's */
    float   ray_spread;                /* read with LJ_RAYS_HAS_SPREAD only.  path: spread of the first segment; < 0, and the default: the
                                          scene camera's, 0.25 / max(width, height) */
    uint32_t flags;                    /* LJ_RAYS_HAS_* */
} LjRaysArgs;
typedef struct LjRadianceBuffers {     /* any pointer may be NULL: not wanted; all three NULL: LJ_ERR_INVALID_ARG */
    float *radiance;   /* [n][3]       mean over the spp samples (lj_irradiance: the irradiance) */
    float *variance;   /* [n][3]       squared standard error of that mean; 0 when spp == 1 */
    float *samples;    /* [n][spp][3]  per-sample radiance, the layout of lj_render_samples with the ray index for the pixel */
} LjRadianceBuffers;
int lj_radiance_rays(lj_scene *scene, const LjRenderArgs *args, const LjRaysArgs *rays_args, int64_t n, const LjRadianceRay *rays_host,
                     const LjRadianceBuffers *out_host);
int lj_irradiance(lj_scene *scene, const LjRenderArgs *args, const LjRaysArgs *rays_args, int64_t n, const LjProbe *probes_host,
                  const LjRadianceBuffers *out_host);
int lj_probe_ray_queries(lj_scene *scene, const LjRenderArgs *args, int64_t n, const LjProbe *probes_host, LjRadianceRay *rays_out_host);

/* Per-sample radiance for the crop window: out[((y-y0)*(x1-x0) + (x-x0))*spp + s][3] — one path_tracing()
 * value (path_tracing.h:7-325) per entry, for path-by-path parity tests. */
int lj_render_samples(lj_scene *scene, const LjRenderArgs *args, float *radiance_host);

/* Batched replacements for intersect()/occluded() (intersection.cpp:7-85) on the flattened BVH, for parity tests
 * of the traversal alone.  Rays are float as Embree sees them (intersection.cpp:15-24). */
typedef struct LjRay { float org[3]; float tnear; float dir[3]; float tfar; } LjRay;
typedef struct LjHit { float t, u, v; int32_t shape_id, prim_id; } LjHit;  /* shape_id == -1: miss */
int lj_intersect(lj_scene *scene, int64_t n, const LjRay *rays_host, LjHit *hits_host);
int lj_occluded(lj_scene *scene, int64_t n, const LjRay *rays_host, uint8_t *occluded_host);

/* ---------------------------------------------------------------- per-object queries on the device, batched
 * The reference's free functions on Material / Light / Shape / Camera / Filter / pcg32, evaluated by the SAME float device
 * code the shade kernels run (device/dshade.h), one query per lane: what lets a test hold the HIP code value for value
 * against vectors produced by the reference's own functions (tests/golden) and re-run the reference's unit tests
 * (src/tests/materials.cpp, filter.cpp, frame.cpp, mipmap.cpp) on the GPU.  Host pointers in, host pointers out; blocking.
 *
 * `variant`: which compiled feature set of the device code answers — -1: the one lj_scene_upload chose for
 * this scene; 0..lj_shade_variant_count()-1: that one, LJ_ERR_INVALID_ARG if it does not cover what the scene holds. */
int lj_shade_variant_count(void);
int lj_scene_shade_variant(const lj_scene *scene);

/* The PathVertex fields a BSDF reads (intersection.h:15-35). */
typedef struct LjVertex {
    float position[3], geometry_normal[3];
    float frame_x[3], frame_y[3], frame_n[3];   /* shading_frame (frame.h:24-41) */
    float uv_screen_size, mean_curvature;
    double uv[2];                                /* double: tiled texture coordinates */
    int32_t material_id, light_id;               /* light_id: get_area_light_id(shape), -1 if not an emitter */
    int32_t shape_id, primitive_id;
} LjVertex;

/* eval(material, dir_in, dir_out, vertex, pool) (material.h:126), pdf_sample_bsdf (material.h:161) and
 * sample_bsdf(material, dir_in, vertex, pool, rnd_uv, rnd_w) (material.h:147), TransportDirection::TO_LIGHT. */
typedef struct LjBsdfQuery { LjVertex vertex; float dir_in[3], dir_out[3], rnd_uv[2], rnd_w; int32_t _pad; } LjBsdfQuery;
typedef struct LjBsdfResult { float eval[3], pdf; float sample_dir[3], sample_eta, sample_roughness; int32_t sample_valid; } LjBsdfResult;
int lj_bsdf_queries(lj_scene *scene, int variant, int64_t n, const LjBsdfQuery *queries_host, LjBsdfResult *results_host);

/* sample_point_on_light(light, ref, rnd_uv, rnd_w, scene), pdf_point_on_light of that point and
 * emission(light, view_dir, footprint, point, scene) (light.h:46-67); light_pmf(scene, id) (scene.cpp:77) beside them. */
typedef struct LjLightQuery { int32_t light_id; float ref[3], rnd_uv[2], rnd_w, view_dir[3]; } LjLightQuery;
typedef struct LjLightResult { float position[3], normal[3], pdf, emission[3], pmf; int32_t _pad; double position_d[3]; } LjLightResult;
int lj_light_queries(lj_scene *scene, int variant, int64_t n, const LjLightQuery *queries_host, LjLightResult *results_host);
/* sample_light(scene, u) (scene.cpp:73) */
int lj_sample_light_queries(lj_scene *scene, int64_t n, const float *u_host, int32_t *light_id_host);

/* compute_shading_info + the PathVertex assembly of intersect() (intersection.cpp:38-62, shape.h:92) for a hit record
 * (shape_id, primitive_id, t, u, v) of the ray (org, dir) whose differential has radius 0 and the given spread
 * (ray.h:27-42); `emission`: emission(vertex, -dir, scene) (path_tracing.h:58-61) when the shape is an emitter, else 0. */
typedef struct LjHitQuery { float org[3], dir[3], t, u, v, ray_spread; int32_t shape_id, primitive_id; } LjHitQuery;
typedef struct LjHitResult { LjVertex vertex; float emission[3]; int32_t _pad; } LjHitResult;
int lj_vertex_queries(lj_scene *scene, int variant, int64_t n, const LjHitQuery *queries_host, LjHitResult *results_host);

/* sample_primary(camera, screen_pos) (camera.cpp:23-47) for pixel (x, y) and the sub-pixel jitter (jx, jy). */
typedef struct LjPrimaryQuery { int32_t x, y; float jx, jy; } LjPrimaryQuery;
typedef struct LjPrimaryResult { float org[3], dir[3]; } LjPrimaryResult;
int lj_primary_ray_queries(lj_scene *scene, int64_t n, const LjPrimaryQuery *queries_host, LjPrimaryResult *results_host);

/* sample(filter, rnd) (filter.h:47, filters/{box,tent,gaussian}.inl); no scene needed. */
typedef struct LjFilterQuery { int32_t kind; float param, rnd[2]; } LjFilterQuery;
int lj_filter_queries(lj_context *ctx, int64_t n, const LjFilterQuery *queries_host, float *offsets_host /* 2 per query */);

/* init_pcg32(stream, seed) then `count` draws (pcg.h:22-68): u32_host[i*count + k] = next_pcg32, real_host = the device's
 * [0,1) float from the same word (NULL: not wanted).  seed 0: 0x853c49e6748fea9b. */
int lj_pcg32_queries(lj_context *ctx, int64_t n, const uint64_t *stream_ids_host, uint64_t seed, int32_t count, uint32_t *u32_host, float *real_host);

/* eval(texture, uv, footprint, pool) (texture.h:123-154, mipmap.h:52-89) of a caller-described texture against the scene's
 * TexturePool; spectrum != 0: Texture<Spectrum> (3 values), else Texture<Real> (value in out[0..2] replicated). */
typedef struct LjTextureQuery { LjTexture texture; double uv[2]; float footprint; int32_t spectrum; } LjTextureQuery;
int lj_texture_queries(lj_scene *scene, int64_t n, const LjTextureQuery *queries_host, float *rgb_host /* 3 per query */);

/* to_local(frame, v) / to_world(frame, v) / Frame(n) (frame.h:11-56) */
typedef struct LjFrameQuery { float n[3], v[3]; } LjFrameQuery;
typedef struct LjFrameResult { float x[3], y[3], to_local[3], to_world[3]; } LjFrameResult;
int lj_frame_queries(lj_context *ctx, int64_t n, const LjFrameQuery *queries_host, LjFrameResult *results_host);

/* eval(phase_function, dir_in, dir_out) — which is also pdf_sample_phase — and sample_phase_function(phase_function, dir_in, rnd)
 * (phase_function.h:18-30, isotropic.inl and henyeygreenstein.inl) of the device code the volumetric path tracer runs
 * (device/dvol.h phase_eval / phase_sample); no scene needed.  phase_kind: LJ_PHASE_*; g: HenyeyGreenstein::g (ignored when isotropic). */
typedef struct LjPhaseQuery { int32_t phase_kind; float g, dir_in[3], dir_out[3], rnd[2]; } LjPhaseQuery;
typedef struct LjPhaseResult { float eval, sample[3]; } LjPhaseResult;
int lj_phase_queries(lj_context *ctx, int64_t n, const LjPhaseQuery *queries_host, LjPhaseResult *results_host);

/* get_sigma_s(medium, p) and get_sigma_a(medium, p) at the point p, and get_majorant(medium, ray) for the ray (org, dir, tfar)
 * (medium.h:25-27, media/heterogeneous.inl; the grid volume's trilinear lookup and box test, volume.h:39-81, 118-144) of medium `medium_id` of the
 * scene, by device/dvol.h get_sigmas / get_majorant.  LJ_ERR_INVALID_ARG: a medium_id outside the scene's media. */
typedef struct LjMediumQuery { int32_t medium_id; float p[3], org[3], dir[3], tfar; } LjMediumQuery;
typedef struct LjMediumResult { float sigma_s[3], sigma_a[3], majorant[3]; } LjMediumResult;
int lj_medium_queries(lj_scene *scene, int64_t n, const LjMediumQuery *queries_host, LjMediumResult *results_host);

/* Counters of the last lj_render* call — or of the last lj_intersect, lj_occluded, lj_scene_update_geometry or lj_scene_rebuild_bvh, which
 * overwrite them too:
 * a ray query leaves render_ms = the query kernel's device time, rays_closest or rays_shadow = n, and mega_launches = 1 or
 * extend_launches = 1 for the route that answered (a tiny scene's leaf scan, or the BVH traversal); an update leaves render_ms and
 * generate_ms (see lj_scene_update_geometry), and so does a rebuild (see lj_scene_rebuild_bvh).  Every other field is then 0.  Read the counters of a render before the next such call. */
typedef struct LjStats {
    uint64_t samples;          /* camera samples traced (LJ_RNG_TILE: those of every tile walked, outside a crop window too) */
    uint64_t bounce_iterations;/* sum over samples of executed iterations of the loop at path_tracing.h:66 (K) */
    uint64_t rays_closest, rays_shadow;
    uint64_t wavefront_steps;  /* host-side iterations of the extend/shade cycle */
    uint64_t queue_bytes;      /* algorithmic queue bytes moved */
    double render_ms;          /* device time of the timed region (HIP events on the render stream) */
    double extend_ms, shade_ms, generate_ms, resolve_ms; /* per-kernel sums, HIP events */
    uint64_t extend_launches, shade_launches;
    uint64_t extend_bytes, shade_bytes; /* algorithmic bytes of each kernel, summed over launches */
    /* tiny scenes run as one fused persistent launch per pass (k_mega) instead of extend / shade steps */
    double mega_ms; uint64_t mega_launches, mega_bytes, path_steps;
} LjStats;
int lj_get_stats(const lj_scene *scene, LjStats *out);

/* Scene facts the host needs (scene.h:58-81). */
typedef struct LjSceneInfo {
    int32_t width, height, spp, max_depth, rr_depth, integrator;
    int64_t n_triangles, n_spheres, n_bvh_nodes;
    double bounds_radius, bounds_center[3], shadow_epsilon;
} LjSceneInfo;
int lj_scene_info(const lj_scene *scene, LjSceneInfo *out);

/* ---------------------------------------------------------------- device groups: one process, N devices
 * The reference's data-parallel axis is its tile loop (render.cpp:75-98 on parallel.cpp:183-237: independent 16x16 tiles, disjoint
 * pixel writes).  A group shards that loop over devices from one host process: tile t = ty*ntx + tx goes to device t mod N, every
 * device renders its tiles at full spp into a zeroed full frame, one ncclReduce(sum, root 0) of the float frames over xGMI, one
 * copy to the host.  Each pixel has one non-zero contributor, so the image is bit-identical to a one-device render.
 * (The process-per-GPU route — LjRenderArgs.rank / world_size + the caller's own collective — stays available: bench.py.)
 *
 * device_ids: n_devices HIP device ids (NULL: 0..n-1).  Ids may repeat ("logical ranks" on one GPU: same sharding, frames summed by
 * a device kernel, since RCCL refuses duplicate devices).  RCCL (librccl.so) is bound at run time, only for >= 2 distinct devices. */
typedef struct lj_device_group lj_device_group;
typedef struct lj_group_scene lj_group_scene;
int lj_group_create(int n_devices, const int *device_ids, lj_device_group **out);
void lj_group_destroy(lj_device_group *group);
int lj_group_size(const lj_device_group *group);
lj_context *lj_group_context(lj_device_group *group, int i);     /* borrowed: device i's context */
int lj_group_uses_rccl(const lj_device_group *group);             /* 1: the frames are reduced by ncclReduce, 0: by a device-side sum */
/* Scene::Scene (scene.cpp:3-53) on every device of the group; the description may be freed afterwards. */
int lj_group_scene_upload(lj_device_group *group, const LjSceneDesc *desc, lj_group_scene **out);
void lj_group_scene_destroy(lj_group_scene *scene);
lj_scene *lj_group_scene_member(lj_group_scene *scene, int i);   /* borrowed: the scene on device i */
/* Replaces `Image3 render(const Scene&)` (render.h:9) across the group.  args->rank / world_size must be 0 (the group shards). */
int lj_group_render(lj_group_scene *scene, const LjRenderArgs *args, float *rgb_host);
int lj_group_get_stats(const lj_group_scene *scene, LjStats *out);   /* sums over the shares; render_ms is the slowest share's */

/* imwrite() (image.h:46, image.cpp:135-173), host only: writes a width x height RGB float image (row-major, y = 0 at the
 * top) by extension — ".pfm": "PF", "<w> <h>", "-1", then the rows top to bottom as little-endian float (the
 * reference's layout, image.cpp:141-149); ".exr": scan-line OpenEXR, HALF channels B, G, R (what the reference asks
 * tinyexr for with "write as fp16", image.cpp:161).  The reference ignores other extensions; here they are
 * LJ_ERR_UNSUPPORTED. */
int lj_image_write(const char *filename, int32_t width, int32_t height, const float *rgb);
/* imread3() / imread1() (image.h:41-45, image.cpp:28-133), host only: decodes a texture file the way the reference's loaders do (JPEG, PNG,
 * TGA, BMP, PSD, GIF, PIC and Radiance HDR with stb_image's conventions incl. its (float) pow(v / 255, 2.2) for 8-bit data; OpenEXR; PFM) into `channels`
 * (1 or 3) floats per pixel, row-major, y = 0 at the top.  *data is owned by the library: release it with lj_image_free. */
int lj_image_read(const char *filename, int32_t channels, int32_t *width, int32_t *height, float **data);
void lj_image_free(float *data);

#ifdef __cplusplus
}
#endif
#endif
