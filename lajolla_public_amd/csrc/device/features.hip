// gfx950 kernels of lj_render_features: the first-hit guide buffers of a pass (albedo, shading normal, depth, coverage) and the variance of
// its per-sample radiance.  Both run after the pass's k_resolve, on the render stream (render.hip finish_pass).
//
//   k_features          group/pixel : feature_sample (dfeature.h) of every camera sample of the pass, summed per pixel in the fixed order of
//                                     dfeature.h.  Closest hits lane by lane through the BVH4 (the tracer of dtracer.h, k_aux's LDS plan).
//                                     A bounded grid-stride loop: no atomics, no counters, nothing per sample goes to HBM.
//   k_resolve_variance  wave/pixel  : k_resolve's sum again (the mean, bit for bit), then the squared deviations of pass.sample_rgb from it.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "dtrav.h"
#include "dtracer.h"
#include "dfeature.h"

namespace ljd {

// every lane of a group of G ends with the group's sum (feature_butterfly: a + b == b + a, so both lanes of a pair hold the same bits)
__device__ __forceinline__ float group_butterfly(float x, uint32_t G) {
    for (uint32_t o = G >> 1; o > 0u; o >>= 1) x += __shfl_xor(x, (int)o, 64);
    return x;
}

// n_items: wave-sized pieces of the pass, 64 / G consecutive pixels each (G = feature_group_size(pass.spp)).  Only the buffers in `want` are written.
template <bool VIEWS>
__global__ void __launch_bounds__(kBlock) k_features(DScene sc, DPass pass, uint32_t n_pixels, uint32_t G, uint32_t n_items, uint32_t want, float *albedo, float *normal, float *depth, float *alpha,
                                                     int stack, int lds_nodes, int lds_prims, int *spill) {
    const TreeView tv = stage_tree(sc, stack, lds_nodes, lds_prims, spill, gridDim.x * kBlock, blockIdx.x * kBlock + threadIdx.x);
    DevTracer<1> tr{tv, sc.spheres, sc.n_spheres};
    const uint32_t lane = threadIdx.x & 63u, l = lane & (G - 1u), sub = lane >> __builtin_ctz(G), per_wave = 64u >> __builtin_ctz(G);
    const uint32_t n_waves = gridDim.x * (kBlock / 64u);
    for (uint32_t item = (blockIdx.x * kBlock + threadIdx.x) >> 6; item < n_items; item += n_waves) {   // (wave-uniform: the whole wave shuffles below)
        const uint32_t p = item * per_wave + sub;
        const bool act = p < n_pixels;
        f3 a = mk3(0, 0, 0), n = mk3(0, 0, 0);
        float d = 0.0f, hit = 0.0f;
        if (act) for (uint32_t s = l; s < pass.spp; s += G) {   // feature_lane_sum of each value
            FeatureSample f;
            feature_sample<VIEWS>(sc, pass, p * pass.spp + s, tr, f);
            a = a + f.a; n = n + f.n; d += f.d; hit += f.hit;
        }
        const float inv = feature_inv_spp(pass.spp);
        const bool writer = act && l == 0u;
        const uint32_t pixel = writer ? pass.pixel_list[p] : 0u;
        if (want & FEAT_ALBEDO) {
            a.x = group_butterfly(a.x, G); a.y = group_butterfly(a.y, G); a.z = group_butterfly(a.z, G);
            if (writer) { albedo[3ull * pixel] = a.x * inv; albedo[3ull * pixel + 1] = a.y * inv; albedo[3ull * pixel + 2] = a.z * inv; }
        }
        if (want & FEAT_NORMAL) {
            n.x = group_butterfly(n.x, G); n.y = group_butterfly(n.y, G); n.z = group_butterfly(n.z, G);
            if (writer) { normal[3ull * pixel] = n.x * inv; normal[3ull * pixel + 1] = n.y * inv; normal[3ull * pixel + 2] = n.z * inv; }
        }
        if (want & (FEAT_DEPTH | FEAT_ALPHA)) {
            hit = group_butterfly(hit, G);
            if (want & FEAT_DEPTH) { d = group_butterfly(d, G); if (writer) depth[pixel] = feature_depth(d, hit); }
            if ((want & FEAT_ALPHA) && writer) alpha[pixel] = hit * inv;
        }
    }
}

// One wave per pixel of the pass, k_resolve's order: the mean first, then the deviations from it.
__global__ void __launch_bounds__(kBlock) k_resolve_variance(DPass pass, uint32_t n_pixels, float *variance) {
    const uint32_t wave = (blockIdx.x * kBlock + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (wave >= n_pixels) return;
    const float *src = pass.sample_rgb + 3ull * (uint64_t)wave * pass.spp;
    const float inv = feature_inv_spp(pass.spp);
    float out[3];
    for (uint32_t c = 0; c < 3u; c++) {
        auto x = [&](uint32_t s) { return src[3 * s + c]; };
        const float mean = group_butterfly(feature_lane_sum(lane, 64u, pass.spp, x), 64u) * inv;
        out[c] = feature_variance(group_butterfly(feature_lane_sqdev(lane, 64u, pass.spp, mean, x), 64u), pass.spp);
    }
    if (lane == 0) {
        const uint32_t pixel = pass.pixel_list[wave];
        variance[3ull * pixel] = out[0]; variance[3ull * pixel + 1] = out[1]; variance[3ull * pixel + 2] = out[2];
    }
}

// ---------------------------------------------------------------- launchers (called from render.hip)
// workgroups of a k_features launch over n_pixels pixels: one wave per 64 / G pixels, capped by the CU count as render_aux caps k_aux
int features_grid(uint64_t n_pixels, uint32_t spp, int n_cus) {
    const uint64_t per_wave = 64u / feature_group_size(spp), items = (n_pixels + per_wave - 1) / per_wave;
    const uint64_t grid = std::min<uint64_t>((items + 3) / 4, (uint64_t)n_cus * 4);
    return (int)(grid < 1 ? 1 : grid);
}
void launch_features(const DScene &sc, const DPass &pass, uint32_t n_pixels, uint32_t want, float *albedo, float *normal, float *depth, float *alpha, const ExtendConfig &cfg, int *spill, int grid, hipStream_t s) {
    if (!n_pixels || !(want & FEAT_FIRST_HIT)) return;
    const uint32_t G = feature_group_size(pass.spp), per_wave = 64u / G, n_items = (n_pixels + per_wave - 1) / per_wave;
    hipLaunchKernelGGL(pass.views ? k_features<true> : k_features<false>, dim3(grid), dim3(kBlock), cfg.smem, s, sc, pass, n_pixels, G, n_items, want, albedo, normal, depth, alpha,
                       cfg.stack, cfg.lds_nodes, cfg.lds_prims, spill);
}
void launch_resolve_variance(const DPass &pass, uint32_t n_pixels, float *variance, hipStream_t s) {
    const uint32_t waves_per_block = kBlock / 64;
    const uint32_t grid = (n_pixels + waves_per_block - 1) / waves_per_block;
    if (grid) hipLaunchKernelGGL(k_resolve_variance, dim3(grid), dim3(kBlock), 0, s, pass, n_pixels, variance);
}

} // namespace ljd
