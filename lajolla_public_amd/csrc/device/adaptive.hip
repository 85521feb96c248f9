// gfx950 kernels of lj_render_adaptive: the rule of dadaptive.h between the renders of a call's rounds.
//
//   k_adaptive_merge    lane/entry : folds a round's rgb and variance frames into the state (n, mean, m2) at each pixel of the round's list
//                                    (round 0: initialises it).  A list names a pixel once, so every state record has one writer.
//   k_adaptive_select   lane/entry : over the call's list in tiles of 256 entries: the 3 x 3 error of the entry's pixel, a flag byte per entry,
//                                    and the tile's count — per wave the population of the 64-bit ballot, summed over the four waves in LDS.
//   k_adaptive_scan     one group  : exclusive prefix sum of the tile counts (a wave scan, the wave sums through LDS, a carry from chunk to
//                                    chunk of 256 tiles), and the total.
//   k_adaptive_scatter  lane/entry : list[offset(tile) + waves before + rank in the wave] = entry, the rank from the ballot and mbcnt.
//   k_adaptive_output   lane/pixel : rgb, variance and samples of the whole film from the state.
// No atomics anywhere: where an entry lands in the next list is a function of the flags alone, so the list keeps the order of the call's
// list whatever the grid.  Grids are bounded grid-stride loops, capped by the CU count as features_grid caps k_features.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "dstage.h"
#include "dadaptive.h"

namespace ljd {

static_assert(kBlock == 256, "a tile is four waves of 64 entries");
constexpr uint32_t kAdaptiveWaves = kBlock / 64u;

__device__ __forceinline__ uint32_t ballot_rank(unsigned long long b) { return __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u)); }

__global__ void __launch_bounds__(kBlock) k_adaptive_merge(const uint32_t *list, uint64_t n_list, uint32_t k, int init, const float *rgb, const float *variance, uint32_t *n, float *mean, float *m2) {
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n_list; i += (uint64_t)gridDim.x * kBlock)
        adaptive_merge_entry(list, i, k, init != 0, rgb, variance, n, mean, m2);
}

// tile t: entries [256 t, 256 t + 256) of the list; flags: one byte per entry, counts: one word per tile
__global__ void __launch_bounds__(kBlock) k_adaptive_select(AdaptiveParams P, int w, int h, const uint32_t *n, const float *mean, const float *m2, const uint32_t *list, uint64_t n_list,
                                                            uint32_t n_tiles, uint8_t *flags, uint32_t *counts) {
    __shared__ uint32_t wave_count[kAdaptiveWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {   // (workgroup-uniform: every lane reaches the barriers)
        const uint64_t i = (uint64_t)t * kBlock + threadIdx.x;
        const bool sel = i < n_list && adaptive_selected(P, list[i], w, h, n, mean, m2);
        if (i < n_list) flags[i] = sel ? 1u : 0u;
        const unsigned long long b = __ballot(sel);
        if (lane == 0u) wave_count[wave] = (uint32_t)__popcll(b);
        __syncthreads();
        if (threadIdx.x == 0u) counts[t] = (wave_count[0] + wave_count[1]) + (wave_count[2] + wave_count[3]);
        __syncthreads();   // the next tile's writers wait for this reader
    }
}

// one workgroup: offsets[t] = counts[0] + .. + counts[t - 1], total[0] = the sum of all
__global__ void __launch_bounds__(kBlock) k_adaptive_scan(const uint32_t *counts, uint32_t n_tiles, uint32_t *offsets, uint32_t *total) {
    __shared__ uint32_t wave_sum[kAdaptiveWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t carry = 0u;
    for (uint32_t base = 0u; base < n_tiles; base += kBlock) {
        const uint32_t t = base + threadIdx.x;
        const uint32_t c = t < n_tiles ? counts[t] : 0u;
        uint32_t incl = c;   // inclusive scan over the wave
        for (uint32_t o = 1u; o < 64u; o <<= 1) { const uint32_t up = (uint32_t)__shfl_up((int)incl, o, 64); if (lane >= o) incl += up; }
        if (lane == 63u) wave_sum[wave] = incl;
        __syncthreads();
        uint32_t before = carry;
        for (uint32_t v = 0u; v < wave; v++) before += wave_sum[v];
        if (t < n_tiles) offsets[t] = before + (incl - c);
        carry += (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
        __syncthreads();
    }
    if (threadIdx.x == 0u) total[0] = carry;
}

__global__ void __launch_bounds__(kBlock) k_adaptive_scatter(const uint32_t *list, uint64_t n_list, uint32_t n_tiles, const uint8_t *flags, const uint32_t *offsets, uint32_t *selected) {
    __shared__ uint32_t wave_count[kAdaptiveWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uint64_t i = (uint64_t)t * kBlock + threadIdx.x;
        const bool sel = i < n_list && flags[i] != 0u;
        const unsigned long long b = __ballot(sel);
        if (lane == 0u) wave_count[wave] = (uint32_t)__popcll(b);
        __syncthreads();
        uint32_t at = offsets[t];
        for (uint32_t v = 0u; v < wave; v++) at += wave_count[v];
        // (at + rank < the total of the scan <= n_list: `selected` holds n_list entries)
        if (sel) selected[at + ballot_rank(b)] = list[i];
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kBlock) k_adaptive_output(uint64_t n_pixels, const uint32_t *n, const float *mean, const float *m2, float *rgb, float *variance, uint32_t *samples) {
    for (uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x; p < n_pixels; p += (uint64_t)gridDim.x * kBlock)
        adaptive_output(p, n, mean, m2, rgb, variance, samples);
}

// ---------------------------------------------------------------- launchers (called from api_device.hip)
// what api_internal.h declares of a call (it does not include dadaptive.h)
struct AdaptiveCall { uint32_t min_spp, max_spp, round_spp, max_rounds; float target_error; };
static AdaptiveParams params_of(const AdaptiveCall &c) { AdaptiveParams P; P.min_spp = c.min_spp; P.max_spp = c.max_spp; P.round_spp = c.round_spp; P.max_rounds = c.max_rounds; P.target_error = c.target_error; return P; }

int adaptive_resolve(int32_t min_spp, int32_t max_spp, int32_t round_spp, int32_t max_rounds, float target_error, AdaptiveCall &out) {
    AdaptiveParams P{};
    const int rc = adaptive_params(min_spp, max_spp, round_spp, max_rounds, target_error, P);
    if (rc == 0) { out.min_spp = P.min_spp; out.max_spp = P.max_spp; out.round_spp = P.round_spp; out.max_rounds = P.max_rounds; out.target_error = P.target_error; }
    return rc;
}
uint64_t adaptive_seed(uint64_t seed0, uint32_t round) { return adaptive_round_seed(seed0, round); }
int adaptive_max_rounds() { return kAdaptiveMaxRounds; }
uint32_t adaptive_tiles(uint64_t n_list) { return (uint32_t)((n_list + kBlock - 1) / kBlock); }

// workgroups of a launch over `items` workgroup-sized pieces: at most four per CU (features_grid's cap), or max_grid when that is smaller
static uint32_t bounded_grid(uint64_t items, int n_cus, int max_grid) {
    uint64_t cap = (uint64_t)n_cus * 4;
    if (max_grid > 0) cap = std::min<uint64_t>(cap, (uint64_t)max_grid);
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(items, cap));
}

void launch_adaptive_merge(const uint32_t *list, uint64_t n_list, uint32_t k, bool init, const float *rgb, const float *variance, uint32_t *n, float *mean, float *m2, int n_cus, int max_grid, hipStream_t s) {
    if (!n_list) return;
    hipLaunchKernelGGL(k_adaptive_merge, dim3(bounded_grid(adaptive_tiles(n_list), n_cus, max_grid)), dim3(kBlock), 0, s, list, n_list, k, init ? 1 : 0, rgb, variance, n, mean, m2);
}
// The three launches of a selection over list[0, n_list): `selected` (n_list entries) gets the next list, total[0] its length.
// flags: n_list bytes; counts, offsets: adaptive_tiles(n_list) words each.
void launch_adaptive_select(const AdaptiveCall &c, int w, int h, const uint32_t *n, const float *mean, const float *m2, const uint32_t *list, uint64_t n_list,
                            uint8_t *flags, uint32_t *counts, uint32_t *offsets, uint32_t *total, uint32_t *selected, int n_cus, int max_grid, hipStream_t s) {
    if (!n_list) return;
    const uint32_t n_tiles = adaptive_tiles(n_list), grid = bounded_grid(n_tiles, n_cus, max_grid);
    hipLaunchKernelGGL(k_adaptive_select, dim3(grid), dim3(kBlock), 0, s, params_of(c), w, h, n, mean, m2, list, n_list, n_tiles, flags, counts);
    hipLaunchKernelGGL(k_adaptive_scan, dim3(1), dim3(kBlock), 0, s, counts, n_tiles, offsets, total);
    hipLaunchKernelGGL(k_adaptive_scatter, dim3(grid), dim3(kBlock), 0, s, list, n_list, n_tiles, flags, offsets, selected);
}
void launch_adaptive_output(uint64_t n_pixels, const uint32_t *n, const float *mean, const float *m2, float *rgb, float *variance, uint32_t *samples, int n_cus, int max_grid, hipStream_t s) {
    if (!n_pixels) return;
    hipLaunchKernelGGL(k_adaptive_output, dim3(bounded_grid((n_pixels + kBlock - 1) / kBlock, n_cus, max_grid)), dim3(kBlock), 0, s, n_pixels, n, mean, m2, rgb, variance, samples);
}

} // namespace ljd
