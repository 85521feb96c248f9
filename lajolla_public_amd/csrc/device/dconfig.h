// Launch plans decided at scene upload (extend.hip, kernels.hip, mega.hip) and carried by the scene object (api_internal.h).
#pragma once
#include <stddef.h>
#include <stdint.h>

// LJ_MEGA_ROUND_STATS (a developer build, tools/dev/mega_round_stats.sh): per pass of k_mega's test loop, how many items it held, how many
// rounds it ran and how full the last of them was — what splitting a short last round by primitive (dmegapool.h) can save.  Three atomics per
// pass: never on in a build that is timed.  The tallies follow the launch's five statistics (mega.hip: kMegaRoundStats of them); render_mega
// (render.hip) prints them.
#ifndef LJ_MEGA_ROUND_STATS
#define LJ_MEGA_ROUND_STATS 0
#endif

namespace ljd {

constexpr int kMegaRoundStats = 11;   // [0] passes, [1] items, [2] test rounds, [3 + k] passes whose last round held 8 k + 1 .. 8 k + 8 items

// feature-set instantiations of the shading code (dshade.h lists them, smallest first)
constexpr int kNumShadeVariants = 6;
constexpr int kShadeVariantAll = kNumShadeVariants - 1;

// LDS image of the extend kernel: stack levels, staged nodes / primitives, which instantiation
struct ExtendConfig {
    int stack; int spill_levels; int lds_nodes; int lds_prims; int resident; int spheres; size_t smem; uint32_t refill_min, min_descending;
    // trees beyond the LDS image: the BVH8 kernels (k_extend8); group-stack levels in LDS, staged nodes, bytes of that image
    int wide; int stack8; int lds_nodes8; size_t smem8;
};
// LDS staging plan of the shade kernel (sizes rounded up to 16 bytes) and the feature-set instantiation (dshade.h)
struct ShadeConfig { uint32_t prims_bytes, materials_bytes, lights_bytes, light_cdf_bytes, light_tris_bytes, light_tri_cdf_bytes, stage_prims, images3_bytes, images1_bytes, env_marg_bytes; int variant; size_t smem; };

} // namespace ljd
