// The per-lane tracer of the kernels that walk a whole path in one lane (volpath.hip: k_volpath; tile.hip: k_tile): closest hits lane by
// lane through the BVH4 traversal steps of dtrav.h, in the Tracer interface dvol.h / dtile.h expect.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include "dtrav.h"

namespace ljd {

// ---------------------------------------------------------------- the tracer's ray casts: lane by lane through the BVH4
// LJ_VOLPATH_STATS (a developer build, tools/dev/volpath_stats.sh): wave-level counts of how often each part of the volumetric tracer
// runs and how many lanes are active in it — slots: 0 traversal node iterations, 1 leaf steps, 2 closest() calls, 3 / 4 tracking iterations
// of the bounce loop / of shadow segments, 5 shadow segments, 6 vol_path_step calls.  64-bit words 2 + 2 s and 3 + 2 s of `counters`: wave-level events, lane-events.
#ifndef LJ_VOLPATH_STATS
#define LJ_VOLPATH_STATS 0
#endif
// SPHERES: 0 the scene holds no sphere; 1 spheres are tested where the traversal meets their leaves; 2 (a scene with a single sphere)
// the traversal passes over them — a sphere's leaf-ordered record has three zero vertices, which the triangle test rejects — and every
// ray tests every sphere afterwards.  Why: inlined into the lane-by-lane leaf step, the reference's double-precision sphere callback holds
// ~50 VGPRs at the tracer's register peak (65 - 112 spilled registers instead of 8 - 63); after the traversal its registers are free.
// The closest hit is the minimum of (t, primitive id) over everything tested, so where a test happens cannot change it.
template <int SPHERES>
struct DevTracer {
    const TreeView &tv;
    const DSphere *spheres; int n_spheres;
#if LJ_VOLPATH_STATS
    uint32_t ev[8], ln[8];   // ln: events this lane was active in; ev: events this lane was the first active lane of (their sum over a wave = the wave's events)
    __device__ __forceinline__ void tick(int s) {
        const unsigned long long b = __ballot(true);
        ln[s]++;
        if (__builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u)) == 0u) ev[s]++;
    }
#else
    __device__ __forceinline__ void tick(int) {}
#endif
    __device__ __forceinline__ bool closest(f3 org, f3 dir, float tnear, float tfar, float &t, float &u, float &v, int &gprim) {
        LaneTrav L;
        L.ray.ox = org.x; L.ray.oy = org.y; L.ray.oz = org.z; L.ray.dx = dir.x; L.ray.dy = dir.y; L.ray.dz = dir.z;
        trav_begin(L, tnear, tfar);
        tick(2);
        trace_lane<SPHERES == 1>(tv, L, false, [&](int s) { tick(s); });
        trav_finish(L);
        t = L.best.t; u = L.best.u; v = L.best.v; gprim = L.best.gprim;
        if (SPHERES == 2) {
            RayF ray; ray.ox = org.x; ray.oy = org.y; ray.oz = org.z; ray.dx = dir.x; ray.dy = dir.y; ray.dz = dir.z; ray.tnear = tnear; ray.tfar = tfar;
            for (int s = 0; s < n_spheres; s++) {
                double td;
                if (sphere_test(ray, spheres[s], td)) {
                    const float tf = (float)td; const int g = spheres[s].gprim;
                    if (tf < t || (tf == t && (gprim < 0 || g < gprim))) { t = tf; u = 0.0f; v = 0.0f; gprim = g; }   // the rule of trav_leaf_step on (t, gprim)
                }
            }
        }
        return gprim >= 0;
    }
};

} // namespace ljd
