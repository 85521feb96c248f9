// gfx950 kernels that trace rays through the flattened BVH4: the extend kernel of the wavefront integrator, the batched ray queries and the
// auxiliary buffers, with the launch plan they share (extend_config).  Written for wave64 / 256-thread workgroups / 160 KB LDS per CU.
//
//   k_extend    persistent   : closest hit of the extension ray + any hit of the pending shadow ray over the
//                              flattened BVH4: extend_loop (dextend.h) over Walk4 (dtrav.h).  Top of the tree, leaf primitives
//                              of small scenes and the per-lane traversal stacks live in LDS.  (intersection.cpp:7-85)
//                              Trees beyond the LDS image may be walked as a BVH8 instead: k_extend8, extend8.hip.
//   k_trace_rays             : batched intersect()/occluded() for the parity tests
//   k_aux                    : the five auxiliary buffers (render.cpp:12-69)
#include <hip/hip_runtime.h>
#include <cstdlib>
#include "dstage.h"
#include "dtrace.h"
#include "dconfig.h"
#include "dtrav.h"
#include "dextend.h"

namespace ljd {

// ---------------------------------------------------------------- extend (the driver lives in dextend.h, the traversal steps in dtrav.h)
#ifndef LJ_EXT_RESIDENT_OCC
#define LJ_EXT_RESIDENT_OCC 4
#endif
#ifndef LJ_EXT_GENERAL_OCC
#define LJ_EXT_GENERAL_OCC 4
#endif
template <bool STATS, bool RESIDENT, bool SPHERES>
__global__ void __launch_bounds__(kBlock, (RESIDENT && !SPHERES && !STATS) ? LJ_EXT_RESIDENT_OCC : (STATS ? 4 : LJ_EXT_GENERAL_OCC)) k_extend(DScene sc, DQueue q, const DBlockState *blocks, uint32_t seg, uint32_t *work, const uint32_t *chunk_list, uint32_t parity, int stack, int lds_nodes, int lds_prims, int *spill, uint32_t refill_min, uint32_t min_descending, unsigned long long *stats, uint32_t pool_at) {
    const TreeView tv = stage_tree(sc, stack, lds_nodes, lds_prims, spill, gridDim.x * kBlock, blockIdx.x * kBlock + threadIdx.x);
    const LeafPool lp = leaf_pool_at(pool_at);
    extend_loop<STATS, Walk4<RESIDENT, SPHERES>>(tv, lp, sc, q, blocks, seg, work, chunk_list, parity, refill_min, min_descending, stats);
}

// ---------------------------------------------------------------- batched ray queries for the parity tests
// Closest hit (or any hit) of every lane's ray, the whole wave together, with k_extend's two phases — inner nodes lane by lane, leaves
// pooled.  L: set up by trav_begin (lanes without a ray: L.cur = kDone).  Ends with trav_finish.
__device__ __forceinline__ void trace_wave(const TreeView &tv, const LeafPool &lp, LaneTrav &L, const bool any_hit) {
    for (;;) {
        for (;;) {
            if (L.cur < 0 && L.held == 0) trav_hold<false>(tv, L);
            const bool descending = L.cur >= 0 && L.cur != kDone;
            if (__ballot(descending) == 0ull) break;
            if (descending) trav_node_step<false>(tv, L);
        }
        const bool at_leaf = L.cur < 0 || L.held != 0;
        if (__ballot(at_leaf) == 0ull) break;
        uint32_t n_pairs;
        (void)trav_leaf_pool<false, true>(tv, lp, L, at_leaf, any_hit, n_pairs);
    }
    trav_finish(L);
}

// (wave-complete iterations over the rays, traced by trace_wave: the parity tests of intersect() / occluded() hold the pooled leaf phase
// to the oracle, bit for bit)
__global__ void __launch_bounds__(kBlock) k_trace_rays(DScene sc, const RayIO *rays, long long n, HitIO *hits, unsigned char *occ, int stack, int lds_nodes, int lds_prims, int *spill, uint32_t pool_at) {
    const TreeView tv = stage_tree(sc, stack, lds_nodes, lds_prims, spill, gridDim.x * kBlock, blockIdx.x * kBlock + threadIdx.x);
    LeafPool lp{};
    lp = leaf_pool_at(pool_at);
    for (long long i0 = (long long)blockIdx.x * kBlock; i0 < n; i0 += (long long)gridDim.x * kBlock) {
        const long long i = i0 + threadIdx.x;
        const bool act = i < n;
        LaneTrav L;
        query_begin<Walk4<false, true>>(L, rays, i, act);
        trace_wave(tv, lp, L, occ != nullptr);
        if (!act) continue;
        if (occ) occ[i] = L.best.gprim >= 0 ? 1 : 0;
        else { HitIO o; query_hit(sc, L.best, o); hits[i] = o; }
    }
}

// ---------------------------------------------------------------- auxiliary buffers (render.cpp:12-69)
// One thread per listed pixel: primary ray through the pixel centre, closest hit, aux_value().
// (pass: the pixel list, and for a batch of cameras — VIEWS — the table the list's entries are decoded with; no sample buffer, nothing is drawn)
template <bool VIEWS>
__global__ void __launch_bounds__(kBlock) k_aux(DScene sc, DPass pass, uint32_t n_pixels, int integrator, float *rgb, int stack, int lds_nodes, int lds_prims, int *spill) {
    const TreeView tv = stage_tree(sc, stack, lds_nodes, lds_prims, spill, gridDim.x * kBlock, blockIdx.x * kBlock + threadIdx.x);
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n_pixels; i += gridDim.x * kBlock) {
        const uint32_t pixel = pass.pixel_list[i];
        f3 org, dir;
        if constexpr (VIEWS) {
            const ViewPixel vp = view_decode(pass, pixel);
            with_view_camera(pass, vp.view, [&](const DCamera &cam) { org = ld3(cam.org); dir = camera_primary_dir(cam, vp.x, vp.y, 0.5f, 0.5f); return 0; });
        } else {
            const int x = (int)(pixel % (uint32_t)sc.cam.width), y = (int)(pixel / (uint32_t)sc.cam.width);
            org = ld3(sc.cam.org); dir = camera_primary_dir(sc.cam, x, y, 0.5f, 0.5f);
        }
        LaneTrav L;
        L.ray.ox = org.x; L.ray.oy = org.y; L.ray.oz = org.z; L.ray.dx = dir.x; L.ray.dy = dir.y; L.ray.dz = dir.z;
        trav_begin(L, 0.0f, INFINITY);   // camera.cpp:46: tnear 0
        trace_lane(tv, L, false);
        trav_finish(L);
        const f3 c = aux_value(sc, integrator, org, dir, L.best.t, L.best.u, L.best.v, L.best.gprim);
        rgb[3ull * pixel] = c.x; rgb[3ull * pixel + 1] = c.y; rgb[3ull * pixel + 2] = c.z;
    }
}

// ---------------------------------------------------------------- launch plan and launchers (called from api_device.hip, render.hip)
// A traversal of a BVH4 with `depth` inner levels holds at most 3 * depth entries.  The first `stack` levels of every
// lane's stack live in LDS (1 KiB per level and workgroup); deeper levels — rare — go to a global overflow buffer.
// LDS per 256-thread workgroup = stack * 1 KiB + staged nodes * 112 B + staged prims * 48 B; four workgroups share a
// CU's 160 KiB, so the budget per workgroup is 40 KiB.
ExtendConfig extend_config(int n_nodes, int n_prims, int bvh_depth, int n_spheres, int n_nodes8, int bvh8_depth, bool open_scene) {
    ExtendConfig c{};
    c.spheres = n_spheres > 0 ? 1 : 0;
    const int need = 3 * (bvh_depth < 1 ? 1 : bvh_depth);
    // LDS image: small scenes (which may become fully resident) get 16 stack levels and up to 32 KiB; for the others 12
    // levels + 20 KiB (the top ~70 nodes): with the 10 KiB of leaf pools a workgroup then takes 30 KiB and five fit a CU (the kernel
    // needs 92 VGPRs: five waves per SIMD).  tools/lds_sweep.sh, 64 spp: disney_bsdf 28.5 ms at 20-22 KiB against 29.8 at 24 (four
    // workgroups), sponza flat (63.5 / 63.8); 14 KiB: +2 %; 64 KiB: +30 % — it crowds out the other workgroups of the CU
    int cap = n_prims <= 256 ? 16 : 12, kib = n_prims <= 256 ? 32 : 20;
    if (const char *e = getenv("LJ_TUNE_EXT_STACK")) cap = atoi(e);
    if (const char *e = getenv("LJ_TUNE_EXT_LDS_KB")) kib = atoi(e);
    c.stack = need < cap ? need : cap;
    c.spill_levels = need - c.stack;
    const int budget = kib * 1024 - 256 - c.stack * kBlock * 4;
    const int small = n_prims <= 256;                                     // primitives only when the whole scene fits (<= 12 KiB)
    c.lds_prims = small ? n_prims : 0;
    int max_nodes = (budget - c.lds_prims * 48) / 112;
    if (max_nodes < 0) max_nodes = 0;
    c.lds_nodes = n_nodes < max_nodes ? n_nodes : max_nodes;
    // whole tree, all primitives and every stack level (+1: the branch-free pushes store one slot ahead) in LDS
    c.resident = (c.lds_nodes == n_nodes && c.lds_prims == n_prims && c.spill_levels == 0 && c.stack + 1 <= 16) ? 1 : 0;
    if (c.resident) c.stack += 1;
    c.smem = (size_t)c.stack * kBlock * 4 + (size_t)c.lds_nodes * 112 + (size_t)c.lds_prims * 48;
    // tuned on MI355X (tools/pool_probe.sh): when the tree is LDS-resident a node step is cheap and waiting for the last
    // descending lane costs little; with nodes in L2 the (pooled) leaf phase starts once fewer than 40 lanes still descend
    // (sponza / disney_bsdf at 64 spp: 16: 65.2 / 30.6 ms, 24: 64.2 / 30.0, 32: 63.2 / 29.7, 40: 63.3 / 30.3, 48: 67.8 / 31.9; with held
    // leaves — a lane that reaches a leaf keeps descending until its second one — 24: 62.6 / 27.8, 32: 61.7 / 27.5, 40: 60.9 / 27.4)
    c.refill_min = 8; c.min_descending = (n_nodes <= c.lds_nodes) ? 1 : 40;
    // A tree beyond the LDS image can be traversed as a BVH8 instead (k_extend8, extend8.hip): 8-byte group entries, at most one push per
    // step, 80-byte nodes.  Measured on MI355X (tools/bvh8_ab.sh, tools/ab1024.sh, profiles/r03_bvh8_ab.txt): 26 % fewer node steps per ray
    // and a third fewer vector-memory instructions, but 26 % more VALU instructions (eight quantised children cost ~200 per step), and with
    // five waves per SIMD the extend kernel is bound by instruction issue, not by the gather path.  Which tree wins depends on what the rays
    // do.  In a closed scene every ray ends on a surface and the BVH4's distance-sorted descent culls most of what lies behind it: sponza
    // 1024 spp 784 ms (BVH4) against 815.  In an open scene under an environment map most rays leave the scene — a ray that hits nothing
    // visits everything along its way whatever the order, so the BVH8's fewer steps are all gain: disney_bsdf 256 spp 82.5 ms against 85.3,
    // matpreview 64 spp 61.0 against 65.3, disney_metal 25.3 against 26.4.  So: BVH8 for trees beyond the LDS image of scenes lit by an
    // environment map, BVH4 otherwise; LJ_TUNE_BVH8=0 / 1 overrides.
    // A ray's stack is rarely more than four groups deep (sponza: 1 push in 600 lands on level 4, 1 in 10^5 on level 6), so six levels
    // live in LDS and the rest of the tree's depth goes to the global overflow buffer; with the first 96 nodes (three full levels and part
    // of the fourth) and the pools a workgroup takes 29.5 KiB: five per CU.  `spill_levels` counts 4-byte units per lane (ensure_spill):
    // two per group level.
    const bool can_wide = !c.resident && n_nodes > c.lds_nodes && n_nodes8 > 0;
    c.wide = (can_wide && open_scene) ? 1 : 0;
    if (const char *e = getenv("LJ_TUNE_BVH8")) c.wide = (atoi(e) != 0 && can_wide) ? 1 : 0;
    if (c.wide) {
        int cap8 = 6, nodes8 = 96;
        if (const char *e = getenv("LJ_TUNE_EXT8_STACK")) cap8 = atoi(e);
        if (const char *e = getenv("LJ_TUNE_EXT8_NODES")) nodes8 = atoi(e);
        const int need8 = bvh8_depth < 1 ? 1 : bvh8_depth;
        c.stack8 = need8 < cap8 ? need8 : cap8;
        if (c.stack8 < 1) c.stack8 = 1;
        c.lds_nodes8 = n_nodes8 < nodes8 ? n_nodes8 : nodes8;
        c.smem8 = (size_t)c.stack8 * kBlock * 8 + (size_t)c.lds_nodes8 * 80;
        const int spill8 = 2 * (need8 - c.stack8 > 0 ? need8 - c.stack8 : 0);
        if (spill8 > c.spill_levels) c.spill_levels = spill8;   // (k_aux / k_volpath still walk the BVH4 with the 4-byte levels)
    }
    return c;
}
int max_stack_depth() { return 40; }  // inner levels; the builder's own cap is 38

// LDS of an extend launch: the traversal image, then the leaf pools of its four waves
size_t extend_smem(const ExtendConfig &cfg) { return ((cfg.smem + 15) & ~(size_t)15) + (kBlock / 64) * kWavePoolBytes; }
void launch_extend(const DScene &sc, const DQueue &q, const DBlockState *blocks, uint32_t grid, uint32_t seg, uint32_t *work, const uint32_t *chunk_list, uint32_t parity, const ExtendConfig &cfg, int *spill, unsigned long long *stats, hipStream_t s) {
    if (cfg.wide) { launch_extend8(sc, q, blocks, grid, seg, work, chunk_list, parity, cfg, spill, stats, s); return; }
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), extend_smem(cfg), s, sc, q, blocks, seg, work, chunk_list, parity, cfg.stack, cfg.lds_nodes, cfg.lds_prims, spill, cfg.refill_min, cfg.min_descending, stats,
                           (uint32_t)((cfg.smem + 15) & ~(size_t)15));
    };
    const int variant = (stats ? 4 : 0) | (cfg.resident ? 2 : 0) | (cfg.spheres ? 1 : 0);
    switch (variant) {
        case 0: launch(k_extend<false, false, false>); break;
        case 1: launch(k_extend<false, false, true>); break;
        case 2: launch(k_extend<false, true, false>); break;
        case 3: launch(k_extend<false, true, true>); break;
        case 4: launch(k_extend<true, false, false>); break;
        case 5: launch(k_extend<true, false, true>); break;
        case 6: launch(k_extend<true, true, false>); break;
        default: launch(k_extend<true, true, true>); break;
    }
}
void launch_aux(const DScene &sc, const DPass &pass, uint32_t n_pixels, int integrator, float *rgb, const ExtendConfig &cfg, int *spill, int grid, hipStream_t s) {
    if (n_pixels) hipLaunchKernelGGL(pass.views ? k_aux<true> : k_aux<false>, dim3(grid), dim3(kBlock), cfg.smem, s, sc, pass, n_pixels, integrator, rgb, cfg.stack, cfg.lds_nodes, cfg.lds_prims, spill);
}
void launch_trace_rays(const DScene &sc, const void *rays, long long n, void *hits, unsigned char *occ, const ExtendConfig &cfg, int *spill, int grid, hipStream_t s) {
    if (cfg.wide) { launch_trace_rays8(sc, rays, n, hits, occ, cfg, spill, grid, s); return; }
    hipLaunchKernelGGL(k_trace_rays, dim3(grid), dim3(kBlock), extend_smem(cfg), s, sc, (const RayIO *)rays, n, (HitIO *)hits, occ, cfg.stack, cfg.lds_nodes, cfg.lds_prims, spill, (uint32_t)((cfg.smem + 15) & ~(size_t)15));
}

} // namespace ljd
