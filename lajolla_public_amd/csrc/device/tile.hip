// gfx950 per-tile schedule (LJ_RNG_TILE, dtile.h): one lane walks one 16x16 tile's pcg32 stream, sample after sample, with the per-lane
// tracer of k_volpath (dtracer.h).  A fidelity mode, not a fast one: the walk of a tile is sequential, so the only parallelism is the
// tile count (1 024 on a 512 x 512 frame).  Launches are bounded: each advances every tile by at most `budget` path steps and leaves its
// cursor in HBM, and the host relaunches until no tile has work left, so no launch holds a shared GPU for long and where
// the walks are cut cannot change a bit.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <algorithm>
#include "dtrav.h"
#include "dtracer.h"
#include "dtile.h"

namespace ljd {

// `lanes` tiles per wave (1..64): lane l < lanes of wave w walks tile w * lanes + l; the other lanes only help stage the LDS image.
// alive[0] += the tiles this launch left unfinished.
template <bool VOL, int SPHERES>
__global__ void __launch_bounds__(kBlock) k_tile(DScene sc, DTileJob job, TileCursor<VOL> *cursors, uint32_t lanes, uint32_t budget, uint32_t *alive,
                                                 int stack, int lds_nodes, int lds_prims, int *spill) {
    const TreeView tv = stage_tree(sc, stack, lds_nodes, lds_prims, spill, gridDim.x * kBlock, blockIdx.x * kBlock + threadIdx.x);
    DevTracer<SPHERES> tr{tv, sc.spheres, sc.n_spheres};
#if LJ_VOLPATH_STATS
    for (int k = 0; k < 8; k++) { tr.ev[k] = 0; tr.ln[k] = 0; }
#endif
    const uint32_t wave = (blockIdx.x * kBlock + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (lane >= lanes) return;
    const uint32_t i = wave * lanes + lane;
    if (i >= job.n_tiles) return;
    const uint32_t tile = job.tiles[i];
    TileCursor<VOL> c = cursors[i];
    bool more = true;
    for (uint32_t n = 0; n < budget && more; n++) more = tile_step<FeatAll, VOL>(sc, tr, job, tile, c);
    cursors[i] = c;
    if (more) atomicAdd(alive, 1u);
}

template <bool VOL>
__global__ void __launch_bounds__(kBlock) k_tile_init(TileCursor<VOL> *cursors, const uint32_t *tiles, uint32_t n_tiles, uint64_t seed) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_tiles) return;
    TileCursor<VOL> c;
    tile_cursor_init(c, tiles[i], seed);
    cursors[i] = c;
}

size_t tile_cursor_bytes(bool vol) { return vol ? sizeof(TileCursor<true>) : sizeof(TileCursor<false>); }

void launch_tile_init(bool vol, void *cursors, const uint32_t *tiles, uint32_t n_tiles, uint64_t seed, hipStream_t s) {
    const dim3 grid((n_tiles + kBlock - 1) / kBlock);
    if (vol) hipLaunchKernelGGL(k_tile_init<true>, grid, dim3(kBlock), 0, s, (TileCursor<true> *)cursors, tiles, n_tiles, seed);
    else hipLaunchKernelGGL(k_tile_init<false>, grid, dim3(kBlock), 0, s, (TileCursor<false> *)cursors, tiles, n_tiles, seed);
}

int tile_grid(uint32_t n_tiles, uint32_t lanes) {
    const uint32_t waves = (n_tiles + lanes - 1) / lanes;
    return (int)std::max<uint32_t>(1, (waves + kBlock / 64 - 1) / (kBlock / 64));
}

void launch_tile(bool vol, const DScene &sc, const DTileJob &job, void *cursors, uint32_t lanes, uint32_t budget, uint32_t *alive, const ExtendConfig &cfg,
                 int *spill, hipStream_t s) {
    const int grid = tile_grid(job.n_tiles, lanes);
    // spheres as k_volpath takes them: none / a single one after the traversal / several inside it (DevTracer)
    const int sph = cfg.spheres == 0 ? 0 : (sc.n_spheres == 1 ? 2 : 1);
    auto go = [&](auto kernel, auto *cur) {
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), cfg.smem, s, sc, job, cur, lanes, budget, alive, cfg.stack, cfg.lds_nodes, cfg.lds_prims, spill);
    };
    if (vol) {
        TileCursor<true> *c = (TileCursor<true> *)cursors;
        if (sph == 0) go(k_tile<true, 0>, c); else if (sph == 2) go(k_tile<true, 2>, c); else go(k_tile<true, 1>, c);
    } else {
        TileCursor<false> *c = (TileCursor<false> *)cursors;
        if (sph == 0) go(k_tile<false, 0>, c); else if (sph == 2) go(k_tile<false, 2>, c); else go(k_tile<false, 1>, c);
    }
}

// the statistics of finished cursors (read back by the host): samples, bounce iterations, closest rays, shadow rays, path steps
void tile_cursor_stats(bool vol, const void *cursors_host, uint32_t n, unsigned long long out[5]) {
    for (int k = 0; k < 5; k++) out[k] = 0;
    auto add = [&](const auto *c) {
        for (uint32_t i = 0; i < n; i++) { out[0] += c[i].samples; out[1] += c[i].bounces; out[2] += c[i].rays_closest; out[3] += c[i].rays_shadow; out[4] += c[i].steps; }
    };
    if (vol) add((const TileCursor<true> *)cursors_host); else add((const TileCursor<false> *)cursors_host);
}

} // namespace ljd
