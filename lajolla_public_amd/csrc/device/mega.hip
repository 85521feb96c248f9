// k_mega — the path tracer of a TINY scene (at most 32 BVH leaves / 256 primitives: cbox, veach_mi, the single-object test
// scenes) as ONE persistent launch: every lane carries one path in registers from its camera ray to its end and then takes
// the next camera sample off a grid-wide counter (path regeneration), so a wave stays full until the frame runs out of
// samples.  No path queue exists for such a scene: nothing but the finished per-sample radiance ever goes to HBM.
//
// Why a different plan for tiny scenes.  The wavefront kernels (kernels.hip) cut the bounce loop at its ray casts because a
// BVH traversal of unknown length and a shading step of unknown kind do not share a wave well.  A scene whose whole tree is
// a handful of leaves has neither problem: the closest hit is found by testing EVERY leaf box against the ray — a
// straight-line scan with the boxes in scalar registers, no stack, no node fetch, no lane idle (dscan below) — and the few
// (ray, leaf) candidates that survive are pooled per wave in LDS and tested by whichever lane is free, 64 at a time, with
// the closest hit merged by an LDS atomic min on (t, primitive id): the same total order the BVH traversal minimises, so
// hit records are bit-identical to k_extend's.  With the trace that regular, fusing it with shade_path (dshade.h — the very
// function k_shade runs) costs no occupancy and removes the queue round trip (290 B per path-step) altogether.
//
// The per-sample values are those of the wavefront kernels bit for bit: same shade_path, same primitive tests, same order
// of the radiance additions (path_tracing.h:207 before the next vertex's emission); a sample's value depends on its pcg32
// stream only, never on the lane, wave or launch that computed it.
#include "dstage.h"
#include "dtrace.h"
#include "dconfig.h"
#include "dregen.h"
#include "dscan.h"
#include "dmegapool.h"

namespace ljd {

#define LJ_CONST __attribute__((address_space(4)))   // constant address space: uniform loads become s_load (scalar cache)

// (ray, leaf) candidates pooled per wave and pass: a pass lists the wave's first `cap` candidates in lane order (dmegapool.h: the whole cap is
// used, a lane's candidates may be split between passes), the rest waits for the next pass.  LJ_TUNE_MEGA_ITEM_CAP lowers it per render / query.  512,
// except in the k_mega build that carries a camera-sample stash (below; cbox: a wave-step pools ~150, 2.3 per lane): 304 there, so that
// its workgroup needs 31 984 B of LDS — the most that still lets five of them share a CU (kLdsPerCU in kLdsGranule steps: 32 000 B each).
constexpr uint32_t kItemCap = 512, kItemCapTight = 304;
constexpr uint32_t kWaveStashBytes = kRegenSlots * (8 + 12);   // a wave's generated camera samples: pcg32 states | directions (x[], y[], z[])
// a wave's scratch: rays | keys | [stash] | occluded flags | items
constexpr uint32_t wave_scan_bytes(uint32_t item_cap, bool stash) { return 64 * 48 + 64 * 8 + (stash ? kWaveStashBytes : 0u) + 64 + item_cap * 2; }
static_assert(wave_scan_bytes(kItemCap, false) % 16 == 0 && wave_scan_bytes(kItemCapTight, true) % 16 == 0, "the next wave's rays are 16-byte records");
// LDS of a gfx950 CU and the unit it is handed out in: the LLVM AMDGPU backend allocates LDS on subtargets with 160 KiB of it in granules of
// 320 dwords (getLdsDwGranularity, AMDGPUBaseInfo.cpp; 128 dwords on the 64 KiB parts) and reports occupancy accordingly
constexpr size_t kLdsPerCU = 160 * 1024, kLdsGranule = 320 * 4;

struct ScanCtx {
    const LJ_CONST float *boxes;        // DScanLeaf records (8 dwords each), wave-uniform reads
    int n_used;                         // leaves in the table
    const LJ_LDS int *leaf_tab;         // (first, count) per leaf
    const LJ_LDS v4f *lprims; int prim_stride;   // leaf-ordered primitives, transposed: v4f k of primitive i at [k * stride + i]
    const DSphere *spheres;
    // this wave's scratch
    LJ_LDS v4f *rays;                   // [lane * 3 + {0: org | tfar_shadow, 1: dir_ext | tnear_ext, 2: dir_shadow | tnear_shadow}]; tfar_ext = inf
    LJ_LDS unsigned long long *keys;    // closest hit of lane's extension ray: float bits of t << 32 | gprim << 16 | leaf-order index
    LJ_LDS uint8_t *occl;               // != 0: lane's shadow ray is blocked
    LJ_LDS uint16_t *items; uint32_t item_cap;
    uint32_t split_m;                   // the largest leaf `count`, rounded up to a power of two (DScene::scan_split_m): lanes per item of a split round
#if LJ_MEGA_ROUND_STATS
    unsigned long long *round_stats;    // developer build (dconfig.h): kMegaRoundStats tallies; null in the ray queries
#endif
    LJ_LDS uint64_t *st_rng;            // stash of camera samples (k_mega builds with STASH only): slot i holds sample st_base + i — its pcg32 state after the jitter draws
    LJ_LDS float *st_dir;               // and its primary direction at [i], [64 + i], [128 + i]
};

__device__ __forceinline__ uint32_t lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

// Inclusive prefix sum over the 64 lanes of a wave (all of them active), no ballot and no LDS: six DPP adds — within each row of 16 lanes by
// row_shr 1, 2, 4, 8 (lanes the shift runs out of add 0), then lane 15 of row 0 / 2 into row 1 / 3 (row_bcast:15, row_mask 0xa) and lane 31
// into rows 2 and 3 (row_bcast:31, row_mask 0xc).  Lane 63 holds the wave's total.
__device__ __forceinline__ uint32_t wave_prefix_incl(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);
    return v;
}

// Leaf-box scan: one bit of a ray's mask per leaf box its segment [tnear, tfar] overlaps.  Slab arithmetic on the table's centre /
// half-extent records (dscan.h: scan_box with its error argument, the 1e-18 clamp of tiny direction components; exit widened by 4 ulp;
// the boxes carry the builder's 1e-5 padding), 14 vector instructions per box for an extension ray and 15 for a shadow ray.  The
// reciprocals are v_rcp_f32 as in the BVH node step.
__device__ __forceinline__ ScanRay scan_ray(f3 org, f3 dir) {
    ScanRay r;
    r.ix = __builtin_amdgcn_rcpf(scan_clamp_dir(dir.x)); r.iy = __builtin_amdgcn_rcpf(scan_clamp_dir(dir.y));
    r.iz = __builtin_amdgcn_rcpf(scan_clamp_dir(dir.z));
    r.ox = org.x * r.ix; r.oy = org.y * r.iy; r.oz = org.z * r.iz;
    return r;
}
__device__ __forceinline__ uint32_t shift_in_sign(uint32_t mask, float d) { return __builtin_amdgcn_alignbit(mask, f2u(d), 31u); }   // (mask << 1) | sign(d)

// Both rays of a path (E: some lane has an extension ray, S: some lane has a shadow ray — wave-uniform, decided outside the loop) against
// every leaf box in ONE pass over the table: the boxes (centre | half-extent) are fetched (scalar loads, four boxes ahead) once, and the two
// independent slab chains interleave.  Bit (n_used - 1 - k) of a ray's mask = its segment overlaps leaf box k (the bits are shifted in from below).
template <bool E, bool S>
__device__ __forceinline__ void scan_leaf_boxes(const ScanCtx &sx, const ScanRay &re, float tnear_e, const ScanRay &rs, float tnear_s, float tfar_s, uint32_t &me, uint32_t &ms) {
    const int n = sx.n_used;
    int k = 0;
    for (; k + 4 <= n; k += 4) {
        float b[4][6];
#pragma unroll
        for (int c = 0; c < 4; c++)
#pragma unroll
            for (int j = 0; j < 6; j++) b[c][j] = sx.boxes[(k + c) * 8 + j];
#pragma unroll
        for (int c = 0; c < 4; c++) {
            if (E) me = shift_in_sign(me, scan_box<false>(b[c], re, tnear_e, INFINITY));
            if (S) ms = shift_in_sign(ms, scan_box<true>(b[c], rs, tnear_s, tfar_s));
        }
    }
    for (; k < n; k++) {
        float b[6];
#pragma unroll
        for (int j = 0; j < 6; j++) b[j] = sx.boxes[k * 8 + j];
        if (E) me = shift_in_sign(me, scan_box<false>(b, re, tnear_e, INFINITY));
        if (S) ms = shift_in_sign(ms, scan_box<true>(b, rs, tnear_s, tfar_s));
    }
}
__device__ __forceinline__ void scan_leaf_boxes2(const ScanCtx &sx, f3 org, f3 dir_e, float tnear_e, f3 dir_s, float tnear_s, float tfar_s, bool any_e, bool any_s,
                                                 uint32_t &me, uint32_t &ms) {
    const ScanRay re = scan_ray(org, dir_e), rs = scan_ray(org, dir_s);
    tnear_e = fmaxf(tnear_e, 0.0f); tnear_s = fmaxf(tnear_s, 0.0f);
    me = 0u; ms = 0u;
    if (any_e && any_s) scan_leaf_boxes<true, true>(sx, re, tnear_e, rs, tnear_s, tfar_s, me, ms);
    else if (any_e) scan_leaf_boxes<true, false>(sx, re, tnear_e, rs, tnear_s, tfar_s, me, ms);
    else if (any_s) scan_leaf_boxes<false, true>(sx, re, tnear_e, rs, tnear_s, tfar_s, me, ms);
}

// Closest hit of every lane's extension ray (has_e) and occlusion of its shadow ray (has_s), wave-synchronous: all 64 lanes
// call it together.  Results: gprim (-1: miss), t, u, v exactly as k_extend reports them; occluded.
// LANE_MAJOR: how the candidates are listed (mega_pool_lane_major below); SPLIT: a short last test round of a pass runs one primitive per
// lane (mega_round_split below) — neither order can change a result: the closest hit is a minimum over a total order and occlusion an OR.
template <bool SPHERES, bool LANE_MAJOR, bool SPLIT>
__device__ __forceinline__ void scan_trace(const ScanCtx &sx, bool has_e, bool has_s, f3 org, f3 dir_e, float tnear_e, f3 dir_s, float tnear_s, float tfar_s,
                                           float &ht, float &hu, float &hv, int &gprim_out, bool &occluded) {
    // No floating-point contraction in here: u = U * (1 / S) must reach the shading code as the rounded product k_extend stores in
    // the hit record, not as a multiply the compiler may fuse into the consumer's `1 - u - v` (a 1-ulp difference in 1e-4 of the samples).
#pragma clang fp contract(off)
    const uint32_t lane = lane_id();
    uint32_t me = 0, ms = 0;
    scan_leaf_boxes2(sx, org, dir_e, tnear_e, dir_s, tnear_s, tfar_s, __ballot(has_e) != 0ull, __ballot(has_s) != 0ull, me, ms);
    me = has_e ? me : 0u; ms = has_s ? ms : 0u;
    v4f r0, r1, r2;
    r0.x = org.x; r0.y = org.y; r0.z = org.z; r0.w = tfar_s;
    r1.x = dir_e.x; r1.y = dir_e.y; r1.z = dir_e.z; r1.w = tnear_e;
    r2.x = dir_s.x; r2.y = dir_s.y; r2.z = dir_s.z; r2.w = tnear_s;
    sx.rays[lane * 3] = r0; sx.rays[lane * 3 + 1] = r1; sx.rays[lane * 3 + 2] = r2;
    sx.keys[lane] = ~0ull; sx.occl[lane] = 0;
    for (;;) {
        uint32_t n_items = 0, total = 0;
        if constexpr (LANE_MAJOR) {
            // ---- pool the candidates of all lanes, lane-major: one prefix sum over the lanes' counts, then every lane lists its own (shadow ray
            // first) from the index the sum gives it — as many as the pool still holds there (pool_share: no index reaches items[item_cap])
            const uint32_t c_s = (uint32_t)__builtin_popcount(ms), c = c_s + (uint32_t)__builtin_popcount(me), incl = wave_prefix_incl(c);
            total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            if (total == 0u) break;
            uint32_t n_s, n_e, idx = incl - c;
            pool_share(c_s, c - c_s, idx, sx.item_cap, n_s, n_e);
            for (const uint32_t end = idx + n_s; idx != end; idx++) sx.items[idx] = (uint16_t)pool_item(lane, pool_pop(ms));
            for (const uint32_t end = idx + n_e; idx != end; idx++) sx.items[idx] = (uint16_t)pool_item(lane, kPoolExtBit + pool_pop(me));
            n_items = pool_pass_items(total, sx.item_cap);
        } else {
            // ---- pool them in rounds: round j takes every lane's j-th candidate (shadow ray first); a pass stops taking rounds above
            // item_cap - 64 (item_cap >= 64 here: clamp_item_cap).  A test round then holds candidates of one rank: rays that run together
            // meet the same leaf there, its primitives are read by broadcast and a sphere leaf's lanes do not wait for a triangle leaf's
            for (;;) {
                const bool has = (ms | me) != 0u;
                const unsigned long long b = __ballot(has);
                if (b == 0ull || n_items + 64u > sx.item_cap) break;
                if (has) {
                    uint32_t bit;
                    if (ms) bit = pool_pop(ms); else bit = kPoolExtBit + pool_pop(me);
                    const uint32_t idx = n_items + __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
                    sx.items[idx] = (uint16_t)pool_item(lane, bit);
                }
                n_items += (uint32_t)__popcll(b);
            }
            if (n_items == 0u) break;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier();
#if LJ_MEGA_ROUND_STATS
        if (lane == 0u && sx.round_stats) {
            atomicAdd(&sx.round_stats[0], 1ull); atomicAdd(&sx.round_stats[1], (unsigned long long)n_items); atomicAdd(&sx.round_stats[2], (unsigned long long)((n_items + 63u) / 64u));
            atomicAdd(&sx.round_stats[3u + ((n_items - 1u) & 63u) / 8u], 1ull);
        }
#endif
        // ---- test them, 64 at a time, whichever lane is free (lane-major: consecutive items mostly share a ray, its reads are LDS broadcasts).
        // A lane walks the primitives of its item's leaf — except in a short last round (SPLIT; shift != 0, wave-uniform), where W = 1 << shift
        // lanes share an item and each tests every W-th primitive of its leaf (dmegapool.h): on cbox (two triangles in all leaves but one, ~150
        // items in a pass) the third round holds about 22 items and costs one triangle test instead of two
        for (uint32_t r = 0; r < n_items; r += 64u) {
            const uint32_t shift = SPLIT ? pool_round_shift(n_items - r, sx.split_m) : 0u;   // (more than 64 items left: not the last round, never split)
            const uint32_t slot = pool_round_item(r, lane, shift);
            if (slot < n_items) {
                const uint32_t it = sx.items[slot];
                const uint32_t src = pool_item_lane(it), leaf = pool_item_leaf(it, (uint32_t)sx.n_used), kind = 1u - pool_item_ext(it);
                const v4f o4 = sx.rays[src * 3], d4 = sx.rays[src * 3 + 1 + kind];
                RayF ray;
                ray.ox = o4.x; ray.oy = o4.y; ray.oz = o4.z; ray.dx = d4.x; ray.dy = d4.y; ray.dz = d4.z;
                ray.tnear = d4.w; ray.tfar = kind ? o4.w : INFINITY;
                const int first = sx.leaf_tab[2 * leaf], cnt = sx.leaf_tab[2 * leaf + 1], step = 1 << shift;
                for (int p = (int)pool_round_prim(lane, shift); p < cnt; p += step) {
                    const int pi = first + p, S = sx.prim_stride;
                    const v4f p0 = sx.lprims[pi], p1 = sx.lprims[S + pi], p2 = sx.lprims[2 * S + pi];
                    const int gprim = __float_as_int(p0.w);
                    bool hit; float t;
                    if (!SPHERES || __float_as_int(p1.w) == 0) {
                        const float v0[3] = {p0.x, p0.y, p0.z}, v1[3] = {p1.x, p1.y, p1.z}, v2[3] = {p2.x, p2.y, p2.z};
                        float U, V, Ssum;
                        hit = tri_test_raw(ray, ray.tfar, v0, v1, v2, t, U, V, Ssum);
                    } else {
                        double td = 0.0;
                        hit = sphere_test(ray, sx.spheres[__float_as_int(p2.w)], td);
                        t = (float)td;
                    }
                    if (hit) {
                        if (kind) sx.occl[src] = 1;
                        else (void)__hip_atomic_fetch_min(&sx.keys[src], ((unsigned long long)f2u(t) << 32) | (unsigned long long)(((uint32_t)gprim << 16) | (uint32_t)pi), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                    }
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier();
        if constexpr (LANE_MAJOR) { if (pool_last_pass(total, sx.item_cap)) break; }   // (the next prefix sum would come to 0)
        else if (__ballot((ms | me) != 0u) == 0ull) break;
    }
    // ---- every lane picks up its own results; the winner's barycentrics are recomputed (one test per ray instead of carrying
    // U, V, S through the pool)
    const unsigned long long key = sx.keys[lane];
    const uint32_t low = (uint32_t)key;
    occluded = sx.occl[lane] != 0u;
    gprim_out = -1; ht = 0.0f; hu = 0.0f; hv = 0.0f;
    if (has_e && low != 0xffffffffu) {
        const int pi = (int)(low & 0xffffu), S = sx.prim_stride;
        gprim_out = (int)(low >> 16);
        ht = u2f((uint32_t)(key >> 32));
        const v4f p0 = sx.lprims[pi], p1 = sx.lprims[S + pi], p2 = sx.lprims[2 * S + pi];
        if (!SPHERES || __float_as_int(p1.w) == 0) {
            RayF ray;
            ray.ox = org.x; ray.oy = org.y; ray.oz = org.z; ray.dx = dir_e.x; ray.dy = dir_e.y; ray.dz = dir_e.z; ray.tnear = tnear_e; ray.tfar = INFINITY;
            const float v0[3] = {p0.x, p0.y, p0.z}, v1[3] = {p1.x, p1.y, p1.z}, v2[3] = {p2.x, p2.y, p2.z};
            float t, U, V, Ssum;
            (void)tri_test_raw(ray, INFINITY, v0, v1, v2, t, U, V, Ssum);
            const float rS = div_ieee(1.0f, Ssum);   // (trav_finish of k_extend)
            hu = U * rS; hv = V * rS;
        }
    }
}

// a + b of two values that are each already rounded: the wavefront kernels add the next-event contribution after it has been through
// the queue, so the product that formed it must not be fused into this addition
__device__ __forceinline__ f3 add_rounded(f3 a, f3 b) {
#pragma clang fp contract(off)
    return mk3(a.x + b.x, a.y + b.y, a.z + b.z);
}

// The wavefront kernels hand a path from one step to the next through the queue, so every value shade_path receives is a rounded
// float the compiler knows nothing about.  Here the same values stay in registers across the loop; without this fence the optimiser
// may fuse the multiply that produced one of them into an addition that consumes it in the next step (a 1-ulp difference in one
// sample of 10^4).  An empty asm per field makes each an opaque register value: no instruction is emitted.
__device__ __forceinline__ void opaque(float &x) { asm volatile("" : "+v"(x)); }
__device__ __forceinline__ void opaque(f3 &v) { opaque(v.x); opaque(v.y); opaque(v.z); }
__device__ __forceinline__ void opaque_state(PathState &ps) {
    opaque(ps.org); opaque(ps.dir); opaque(ps.ht); opaque(ps.hu); opaque(ps.hv); opaque(ps.sdir); opaque(ps.stfar);
    opaque(ps.W); opaque(ps.rr); opaque(ps.p2); opaque(ps.rad); opaque(ps.nee); opaque(ps.eta_scale); opaque(ps.spread);
}

// A dead lane starts the path of stash slot `slot` (generated by whichever lane had that index; same values as generate_path on this lane)
// (a batch of cameras: the stash holds no origin — start_path finds the sample's view from its id and reads the origin from the table)
template <bool VIEWS>
__device__ __forceinline__ void stash_start(const DScene &sc, const DPass &pass, const ScanCtx &sx, uint32_t st_base, uint32_t slot, PathState &ps) {
    const f3 dir = mk3(sx.st_dir[slot], sx.st_dir[64 + slot], sx.st_dir[128 + slot]);
    start_path<VIEWS>(sc, pass, st_base + slot, dir, sx.st_rng[slot], ps);
}

// LDS image of the scan area at byte offset `at` (16-byte aligned): [leaf table][primitives, transposed][4 x wave scratch]
template <uint32_t ITEM_CAP, bool STASH>
__device__ __forceinline__ ScanCtx stage_scan(const DScene &sc, uint32_t at, uint32_t item_cap, unsigned long long *round_stats = nullptr) {
    ScanCtx sx;
    char *base = (char *)lj_smem + at;
    LJ_LDS int *lt = (LJ_LDS int *)base;
    for (int i = threadIdx.x; i < sc.n_scan_leaves; i += kBlock) { lt[2 * i] = sc.scan_leaves[i].first; lt[2 * i + 1] = sc.scan_leaves[i].count; }
    const uint32_t lt_bytes = ((uint32_t)sc.n_scan_leaves * 8u + 15u) & ~15u;
    LJ_LDS v4f *lp = (LJ_LDS v4f *)(base + lt_bytes);
    const v4f *src = reinterpret_cast<const v4f *>(sc.leaf_prims);
    for (int i = threadIdx.x; i < sc.n_prims * 3; i += kBlock) lp[(i % 3) * sc.n_prims + (i / 3)] = src[i];
    char *wave = base + lt_bytes + (uint32_t)sc.n_prims * 48u + (threadIdx.x >> 6) * wave_scan_bytes(ITEM_CAP, STASH);
    sx.boxes = (const LJ_CONST float *)(uintptr_t)sc.scan_leaves; sx.n_used = sc.n_scan_used;
    sx.leaf_tab = lt; sx.lprims = lp; sx.prim_stride = sc.n_prims; sx.spheres = sc.spheres;
    sx.rays = (LJ_LDS v4f *)wave; sx.keys = (LJ_LDS unsigned long long *)(wave + 64 * 48);
    sx.st_rng = (LJ_LDS uint64_t *)(wave + 64 * 48 + 64 * 8); sx.st_dir = (LJ_LDS float *)(wave + 64 * 48 + 64 * 8 + kRegenSlots * 8);
    const uint32_t after = 64 * 48 + 64 * 8 + (STASH ? kWaveStashBytes : 0u);   // (without a stash st_rng / st_dir are never used)
    sx.occl = (LJ_LDS uint8_t *)(wave + after); sx.items = (LJ_LDS uint16_t *)(wave + after + 64);
    sx.item_cap = item_cap < ITEM_CAP ? item_cap : ITEM_CAP;   // (the launchers pass 1 .. ITEM_CAP: the pool is ITEM_CAP items whatever arrives)
    sx.split_m = (uint32_t)sc.scan_split_m;
#if LJ_MEGA_ROUND_STATS
    sx.round_stats = round_stats;
#endif
    return sx;
}
size_t scan_smem(int n_scan_leaves, int n_prims, uint32_t item_cap = kItemCap, bool stash = false) { return (((size_t)n_scan_leaves * 8 + 15) & ~(size_t)15) + (size_t)n_prims * 48 + 4 * (size_t)wave_scan_bytes(item_cap, stash); }

// waves per SIMD the kernel is built for.  The Lambert-only instantiation needs 113 VGPRs unconstrained; built for five waves (96
// VGPRs, 6 of them spilled to scratch) it is 7 % faster than for four — the kernel waits on LDS round trips and dependent issue,
// which a fifth wave hides (measured on MI355X, cbox 256 spp: 3 waves 17.8 ms, 4: 16.1, 5: 14.9, 6: 15.7 with 43 spills).  The
// feature sets with textures, microfacet lobes or sphere lights need ~150 VGPRs and spill 25-70 registers already at four: three.
#ifndef LJ_MEGA_OCC
#define LJ_MEGA_OCC 5
#endif
template <class Ft> struct MegaOccupancy { static constexpr int waves = 3; };
template <> struct MegaOccupancy<FeatLambert> { static constexpr int waves = LJ_MEGA_OCC; };
#ifndef LJ_MEGA_OCC_PLASTIC
#define LJ_MEGA_OCC_PLASTIC 4
#endif
template <> struct MegaOccupancy<FeatPlastic> { static constexpr int waves = LJ_MEGA_OCC_PLASTIC; };
// Which builds generate camera samples 64 at a time into a per-wave stash (k_mega below).  It pays where paths are short: on cbox (4.02
// steps per path, 29 % of lane slots idle) it takes 4.3 % off a render; on veach_mi (Plastic: 85 % of the lanes live anyway) it cost 0.9 %
// (profiles/mega_stash_ab.txt).  So: the five-wave Lambert build only; every other build regenerates lane by lane, as before.
#ifndef LJ_MEGA_STASH
#define LJ_MEGA_STASH 1
#endif
template <class Ft> constexpr bool mega_stash() { return LJ_MEGA_STASH && MegaOccupancy<Ft>::waves >= 5; }
#ifndef LJ_MEGA_ITEM_CAP_TIGHT   // (developer A/B: the small pool without the stash)
#define LJ_MEGA_ITEM_CAP_TIGHT 0
#endif
template <class Ft> constexpr uint32_t mega_item_cap() { return (mega_stash<Ft>() || (LJ_MEGA_ITEM_CAP_TIGHT && MegaOccupancy<Ft>::waves >= 5)) ? kItemCapTight : kItemCap; }

// Which builds list the scan's candidates lane-major off one wave prefix sum (scan_trace, dmegapool.h) instead of in rounds.  It takes 57 vector
// and 113 scalar instructions off a cbox wave-step (-3.1 % of a render); on veach_mi (spheres, Plastic build, 26 leaves, coherent rays) a render
// was 5 % SLOWER with it — a lane-major test round mixes leaves, so sphere and triangle leaves share rounds (profiles/mega_pool_ab.txt).
// So: the triangle-only five-wave Lambert build, and the ray queries; every other build pools in rounds, as before.
template <class Ft, bool SPHERES> constexpr bool mega_pool_lane_major() { return !SPHERES && MegaOccupancy<Ft>::waves >= 5; }

// Which builds split a short last test round of a pass by primitive (scan_trace, dmegapool.h).  On cbox the last round of a pass holds at most 32
// items in 54.9 % of the passes; split, a pass issues 58 vector instructions fewer and 42 scalar ones more, and a render is 1.0 % faster (11.059 ->
// 10.945 ms).  veach_mi pools in rounds, which fills its rounds (15.5 % of its last rounds hold at most 32 items): split, it was 0.8 % SLOWER
// (profiles/mega_round_ab.txt).  So: the builds that pool lane-major, and the ray queries; every other build keeps the loop it had.
// LJ_MEGA_ROUND_SPLIT (developer A/B): 0 nowhere, 1 as said, 2 every build.
#ifndef LJ_MEGA_ROUND_SPLIT
#define LJ_MEGA_ROUND_SPLIT 1
#endif
template <class Ft, bool SPHERES> constexpr bool mega_round_split() { return LJ_MEGA_ROUND_SPLIT >= 2 || (LJ_MEGA_ROUND_SPLIT == 1 && mega_pool_lane_major<Ft, SPHERES>()); }
constexpr bool kQueryRoundSplit = LJ_MEGA_ROUND_SPLIT >= 1;

// stats: [0] bounce iterations, [1] closest-hit rays, [2] shadow rays, [3] samples finished, [4] path steps (shade_path calls)
// (VIEWS: the pass is a batch of cameras, dshade.h; same occupancy, same LDS — the stash has no per-view entry)
template <class Ft, bool SPHERES, bool VIEWS>
__global__ void __launch_bounds__(kBlock, MegaOccupancy<Ft>::waves) k_mega(DScene sc, DPass pass, ShadeStage stg, uint32_t scan_at, uint32_t n_samples, uint32_t grab,
                                                              uint32_t item_cap, uint32_t *sample_counter, unsigned long long *stats) {
    stage_shade_tables<2>(sc, stg, 0u);
    constexpr bool STASH = mega_stash<Ft>();
    const ScanCtx sx = stage_scan<mega_item_cap<Ft>(), STASH>(sc, scan_at, item_cap, stats + 5);   // (the tallies of an LJ_MEGA_ROUND_STATS build)
    __syncthreads();
    const uint32_t lane = lane_id();
    ShadeCounters cnt; cnt.bounces = cnt.closest = cnt.shadow = cnt.done = 0;
    uint32_t steps = 0;
    bool live = false;
    RegenState rg; regen_init(rg);   // wave-uniform: the wave's open range of camera samples and its stash (dregen.h)
    PathState ps;
    ps.flags = 0u; ps.stfar = 0.0f; ps.sample = 0u;
    for (;;) {
        // ---- the step of a path that is under way: hit accounting, next-event estimation, BSDF sampling (path_tracing.h:58-322)
        opaque_state(ps);
        if (live) {
            steps++;
            if (!shade_path<Ft, VIEWS>(sc, pass, ps, cnt)) {
                float *o = pass.sample_rgb + 3ull * ps.sample;
                o[0] = ps.rad.x; o[1] = ps.rad.y; o[2] = ps.rad.z;
                cnt.done++; live = false;
            }
        }
        // ---- lanes without a path take the next camera samples (path_tracing.h:10-14)
        const unsigned long long dead = __ballot(!live);
        if constexpr (STASH) {
            // first what the wave's stash still holds; when that runs out the wave generates its next 64 samples with all lanes at once (a
            // quarter of the lanes end per step: generated lane by lane, the block would be issued every step three quarters empty) and the
            // lanes still waiting are served from the new fill
            uint32_t n_dead = (uint32_t)__popcll(dead);
            if (n_dead != 0u) {
                uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(dead >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)dead, 0u));
                uint32_t first;
                uint32_t take = regen_take(rg, n_dead, first);
                if (!live && rank < take) { stash_start<VIEWS>(sc, pass, sx, rg.st_base, first + rank, ps); live = true; }
                n_dead -= take; rank -= take;   // (rank of a lane that is still dead among those still dead)
                if (n_dead != 0u) {
                    if (regen_needs_grab(rg)) {
                        uint32_t b = 0;
                        if (lane == 0u) b = atomicAdd(sample_counter, grab);
                        regen_grabbed(rg, (uint32_t)__builtin_amdgcn_readfirstlane((int)b), n_samples, grab);
                    }
                    const uint32_t n_gen = regen_refill(rg);
                    if (n_gen != 0u) {
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier();   // the reads above come first
                        if (lane < n_gen) {
                            f3 dir; uint64_t rng;
                            camera_sample<VIEWS>(sc, pass, rg.st_base + lane, dir, rng);
                            sx.st_rng[lane] = rng; sx.st_dir[lane] = dir.x; sx.st_dir[64 + lane] = dir.y; sx.st_dir[128 + lane] = dir.z;
                        }
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier();
                        take = regen_take(rg, n_dead, first);
                        if (!live && rank < take) { stash_start<VIEWS>(sc, pass, sx, rg.st_base, first + rank, ps); live = true; }
                    }
                }
            }
            // No lane is live here only if the wave may end.  Every lane was dead and asked for a sample, so regen_take drained the stash; lanes
            // were left over, so the wave went to the counter unless its range was still open, and refilled unless the range was empty — and a
            // refill of n >= 1 slots makes a lane live.  So: stash empty, range empty, counter exhausted, which is regen_done(rg); the host
            // model (tests/twin_regen) asserts the implication on every iteration.  Written as this plain test the loop also keeps the
            // shape the register allocator handles well (6 VGPRs spilled in the Lambert build, as without the stash).
            if (__ballot(live) == 0ull) break;
        } else {
            if (dead != 0ull && !rg.exhausted) {   // lane by lane, straight off the wave's open range
                if (rg.w_next == rg.w_end) {
                    uint32_t b = 0;
                    if (lane == 0u) b = atomicAdd(sample_counter, grab);
                    regen_grabbed(rg, (uint32_t)__builtin_amdgcn_readfirstlane((int)b), n_samples, grab);
                }
                if (!rg.exhausted) {
                    const uint32_t left = rg.w_end - rg.w_next, n_dead = (uint32_t)__popcll(dead);
                    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(dead >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)dead, 0u));
                    if (!live && rank < left) { generate_path<VIEWS>(sc, pass, rg.w_next + rank, ps); live = true; }
                    rg.w_next += n_dead < left ? n_dead : left;
                }
            }
            if (__ballot(live) == 0ull) { if (rg.exhausted) break; else continue; }
        }
        // ---- both rays of the vertex: the pending shadow ray [eps, (1 - eps) d] and the extension ray [eps, inf) (camera rays from 0)
        opaque_state(ps);
        const bool has_e = live && !(ps.flags & PF_NO_EXT), has_s = live && ps.stfar > 0.0f;
        float ht, hu, hv; int gprim; bool occluded;
        scan_trace<SPHERES, mega_pool_lane_major<Ft, SPHERES>(), mega_round_split<Ft, SPHERES>()>(sx, has_e, has_s, ps.org, ps.dir, (ps.flags & 0xffffu) == 2u ? 0.0f : sc.eps, ps.sdir, sc.eps, ps.stfar, ht, hu, hv, gprim, occluded);
        if (live) {
            if (has_s && !occluded) ps.rad = add_rounded(ps.rad, ps.nee);   // path_tracing.h:207 (k_shade adds it at the top of the next step)
            ps.ht = ht; ps.hu = hu; ps.hv = hv; ps.hcode = gprim + 1;
            if (ps.flags & PF_NO_EXT) {   // sample_bsdf failed (path_tracing.h:220-223): nothing left but the contribution just added
                float *o = pass.sample_rgb + 3ull * ps.sample;
                o[0] = ps.rad.x; o[1] = ps.rad.y; o[2] = ps.rad.z;
                cnt.done++; live = false;
            }
        }
    }
    const uint32_t b = wave_sum(cnt.bounces), cl = wave_sum(cnt.closest), sh = wave_sum(cnt.shadow), dn = wave_sum(cnt.done), sp = wave_sum(steps);
    if (lane == 0u) {
        atomicAdd(&stats[0], (unsigned long long)b); atomicAdd(&stats[1], (unsigned long long)cl); atomicAdd(&stats[2], (unsigned long long)sh);
        atomicAdd(&stats[3], (unsigned long long)dn); atomicAdd(&stats[4], (unsigned long long)sp);
    }
}

// batched intersect() / occluded() through the scan (the parity tests hold it bit for bit to the oracle like the BVH traversal)
struct RayIO { float org[3]; float tnear; float dir[3]; float tfar; };
struct HitIO { float t, u, v; int32_t shape_id, prim_id; };
__global__ void __launch_bounds__(kBlock) k_trace_rays_scan(DScene sc, const RayIO *rays, long long n, HitIO *hits, unsigned char *occ, uint32_t item_cap) {
    const ScanCtx sx = stage_scan<kItemCap, false>(sc, 0u, item_cap);
    __syncthreads();
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i0 = (long long)blockIdx.x * kBlock; i0 < n; i0 += stride) {   // wave-complete iterations
        const long long i = i0 + threadIdx.x;
        const bool act = i < n;
        f3 org = mk3(0, 0, 0), dir = mk3(0, 0, 1); float tn = 0.0f, tf = 0.0f;
        if (act) { org = ld3(rays[i].org); dir = ld3(rays[i].dir); tn = rays[i].tnear; tf = rays[i].tfar; }
        float ht, hu, hv; int gprim; bool occluded;
        if (occ) {   // any hit in (tnear, tfar]: the shadow-ray slot
            scan_trace<true, true, kQueryRoundSplit>(sx, false, act, org, dir, 0.0f, dir, tn, tf, ht, hu, hv, gprim, occluded);
            if (act) occ[i] = occluded ? 1 : 0;
        } else {
            // closest hit in (tnear, tfar]: the extension-ray slot has tfar = inf, so the far end is applied to the result
            scan_trace<true, true, kQueryRoundSplit>(sx, act, false, org, dir, tn, dir, 0.0f, 0.0f, ht, hu, hv, gprim, occluded);
            if (act) {
                HitIO o; o.t = 0; o.u = 0; o.v = 0; o.shape_id = -1; o.prim_id = -1;
                if (gprim >= 0 && ht <= tf) { const DPrimShade &ps = sc.prims[gprim]; o.t = ht; o.u = hu; o.v = hv; o.shape_id = ps.shape_id; o.prim_id = ps.prim_id; }
                hits[i] = o;
            }
        }
    }
}

// ---------------------------------------------------------------- launchers

// LDS a k_mega workgroup needs (0: the scene cannot run as a mega launch)
size_t mega_smem(const DScene &sc, const ShadeConfig &scfg) {
    if (sc.n_scan_leaves <= 0 || !scfg.stage_prims || scfg.smem == 0) return 0;
    uint32_t item_cap = kItemCap; bool stash = false;
    with_shade_variant(scfg.variant, [&](auto ft) { item_cap = mega_item_cap<decltype(ft)>(); stash = mega_stash<decltype(ft)>(); });
    const size_t at = (scfg.smem + 15) & ~(size_t)15, total = at + scan_smem(sc.n_scan_leaves, sc.n_prims, item_cap, stash);
    return total <= 64 * 1024 ? total : 0;
}

// workgroups per CU a mega launch keeps resident (the grid is persistent: n_cus * this): what the registers allow, and no more than
// fit the CU's 160 KiB of LDS
int mega_blocks_per_cu(const DScene &sc, const ShadeConfig &scfg) {
    int waves = 3;
    with_shade_variant(scfg.variant, [&](auto ft) { waves = MegaOccupancy<decltype(ft)>::waves; });
    const size_t smem = (mega_smem(sc, scfg) + kLdsGranule - 1) / kLdsGranule * kLdsGranule;
    const int by_lds = smem ? (int)(kLdsPerCU / smem) : waves;
    return waves < by_lds ? waves : by_lds;
}

// the pool's size for one launch: `tune` items (LJ_TUNE_MEGA_ITEM_CAP; 0: unset) within [1, what the build's LDS holds] — [64, that] where
// the candidates are pooled in rounds of up to 64
static uint32_t clamp_item_cap(uint32_t tune, uint32_t build_cap, bool lane_major) {
    const uint32_t lo = lane_major ? 1u : 64u;
    return tune == 0u || tune > build_cap ? build_cap : (tune < lo ? lo : tune);
}

void launch_mega(const DScene &sc, const DPass &pass, const ShadeConfig &scfg, bool spheres, uint32_t n_samples, uint32_t grab, uint32_t item_cap_tune,
                 uint32_t *sample_counter, unsigned long long *stats, int grid, hipStream_t s) {
    const ShadeStage st = make_shade_stage(scfg);
    const uint32_t at = (uint32_t)((scfg.smem + 15) & ~(size_t)15);
    const size_t smem = mega_smem(sc, scfg);
    with_shade_variant(scfg.variant, [&](auto ft) {
        using Ft = decltype(ft);
        const uint32_t item_cap = clamp_item_cap(item_cap_tune, mega_item_cap<Ft>(), spheres ? mega_pool_lane_major<Ft, true>() : mega_pool_lane_major<Ft, false>());
        auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), smem, s, sc, pass, st, at, n_samples, grab, item_cap, sample_counter, stats); };
        if (pass.views) { if (spheres) launch(k_mega<Ft, true, true>); else launch(k_mega<Ft, false, true>); }
        else if (spheres) launch(k_mega<Ft, true, false>);
        else launch(k_mega<Ft, false, false>);
    });
}

void launch_trace_rays_scan(const DScene &sc, const void *rays, long long n, void *hits, unsigned char *occ, uint32_t item_cap_tune, int grid, hipStream_t s) {
    hipLaunchKernelGGL(k_trace_rays_scan, dim3(grid), dim3(kBlock), scan_smem(sc.n_scan_leaves, sc.n_prims), s, sc, (const RayIO *)rays, n, (HitIO *)hits, occ,
                       clamp_item_cap(item_cap_tune, kItemCap, true));
}

} // namespace ljd
