// gfx950 kernels of the wavefront integrator: everything but the ray casts (k_extend: extend.hip, k_extend8: extend8.hip).
// Written for wave64 / 256-thread workgroups / 160 KB LDS per CU.
//
//   k_shade     block/segment: hit accounting, NEE, BSDF sampling, Russian roulette (path_tracing.h:58-322).  Each
//                              workgroup owns one segment of the queue: survivors are compacted to the front of the
//                              segment in order (wave ballots + a 4-entry LDS scan), then the workgroup's next camera
//                              samples (path_tracing.h:10-14) are appended behind them and its live chunks listed.
//                              Instantiated per scene feature set (ShadeFeat).
//   k_tail      block/segment: the end of a render, fused: trace (lane by lane, dtrav.h) + shade + compact in a loop inside one launch
//   k_resolve   wave/pixel   : fixed-order sum of the per-sample radiance -> radiance / spp (render.cpp:94)
// (k_aux and k_trace_rays: extend.hip; k_volpath, the volumetric path tracer: volpath.hip)
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <algorithm>
#include "dstage.h"
#include "dtrace.h"
#include "dconfig.h"
#include "dtrav.h"
#include "dprobe.h"

namespace ljd {

// ---------------------------------------------------------------- queue <-> registers (16-byte records)
__device__ __forceinline__ void q_load_for_shade(const DQueue &q, uint32_t i, PathState &ps) {
    const Rec4 ro = q.ro[i], rd = q.rd[i], rh = q.rh[i], rw = q.rw[i], rl = q.rl[i], rn = q.rn[i], rg = q.rg[i];
    ps.org = mk3(ro.x, ro.y, ro.z); ps.dir = mk3(rd.x, rd.y, rd.z); ps.flags = f2u(rd.w);
    ps.ht = rh.x; ps.hu = rh.y; ps.hv = rh.z; ps.hcode = (int32_t)f2u(rh.w);
    ps.W = mk3(rw.x, rw.y, rw.z); ps.rr = rw.w;
    ps.rad = mk3(rl.x, rl.y, rl.z); ps.eta_scale = rl.w;
    ps.nee = mk3(rn.x, rn.y, rn.z); ps.spread = rn.w;
    ps.sample = f2u(rg.x); ps.rng = (uint64_t)f2u(rg.y) | ((uint64_t)f2u(rg.z) << 32); ps.p2 = rg.w;
    ps.sdir = mk3(0, 0, 0); ps.stfar = 0.0f;
}
__device__ __forceinline__ void q_store(const DQueue &q, uint32_t i, const PathState &ps) {
    q.ro[i] = mk4(ps.org.x, ps.org.y, ps.org.z, ps.stfar);
    q.rd[i] = mk4(ps.dir.x, ps.dir.y, ps.dir.z, u2f(ps.flags));
    q.rs[i] = mk4(ps.sdir.x, ps.sdir.y, ps.sdir.z, 0.0f);
    q.rw[i] = mk4(ps.W.x, ps.W.y, ps.W.z, ps.rr);
    q.rl[i] = mk4(ps.rad.x, ps.rad.y, ps.rad.z, ps.eta_scale);
    q.rn[i] = mk4(ps.nee.x, ps.nee.y, ps.nee.z, ps.spread);
    q.rg[i] = mk4(u2f(ps.sample), u2f((uint32_t)ps.rng), u2f((uint32_t)(ps.rng >> 32)), ps.p2);
}

// ---------------------------------------------------------------- shade + compaction
struct ShadeSortBuf { uint32_t *perm; uint8_t *keys; uint32_t octant_bin; };   // (perm == nullptr: chunks are compacted in place)
// Where a chunk's survivors go inside the output range [out, out + total): in thread order, or — `octant_bin` — grouped by the direction
// octant of their new extension ray (a counting sort over eight keys by wave ballots), so that the 64 rays a wave of the extend kernel picks
// up start out in the same octant.  Returns the survivor's offset and the chunk's total (identical in every thread).  Call from all threads.
__device__ __forceinline__ uint32_t survivor_offset(bool alive, const PathState &ps, bool octant_bin, uint32_t (*s_cnt)[kBlock / 64], uint32_t &total) {
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    if (!octant_bin) {
        const unsigned long long mask = __ballot(alive);
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
        if (lane == 0u) s_cnt[0][wave] = (uint32_t)__popcll(mask);
        __syncthreads();
        uint32_t before = 0; total = 0;
        for (uint32_t w = 0; w < kBlock / 64; w++) { const uint32_t n = s_cnt[0][w]; before += (w < wave) ? n : 0u; total += n; }
        return before + rank;   // (the caller alternates between two count tables, so the next chunk's counts do not race these reads)
    }
    const uint32_t oct = (ps.dir.x < 0.0f ? 1u : 0u) | (ps.dir.y < 0.0f ? 2u : 0u) | (ps.dir.z < 0.0f ? 4u : 0u);
    uint32_t rank = 0;
#pragma unroll
    for (uint32_t k = 0; k < 8u; k++) {
        const unsigned long long m = __ballot(alive && oct == k);
        if (alive && oct == k) rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        if (lane == 0u) s_cnt[k][wave] = (uint32_t)__popcll(m);
    }
    __syncthreads();
    uint32_t before = 0; total = 0;
    for (uint32_t k = 0; k < 8u; k++) for (uint32_t w = 0; w < kBlock / 64; w++) {
        const uint32_t n = s_cnt[k][w];
        before += (k < oct || (k == oct && w < wave)) ? n : 0u; total += n;
    }
    return before + rank;
}

// What a path will do in this shade step, as far as its queue records tell — the key its chunk is sorted by before shading (below):
// 0 nothing (no extension ray was traced: only the pending next-event estimate is added), 1 its ray left the scene (environment map),
// 2 it only accounts for the hit (Russian roulette ended it), 3 + k full shading on Material alternative k (material.h:102-110).
constexpr int kShadeKeys = 12;
template <class Ft>
__device__ __forceinline__ int shade_key(const DScene &sc, const DQueue &q, uint32_t slot) {
    const uint32_t flags = f2u(q.rd[slot].w);
    if (flags & PF_NO_EXT) return 0;
    const int gprim = (int)(f2u(q.rh[slot].w) & 0x3fffffffu) - 1;
    if (gprim < 0) return 1;
    if (flags & PF_DYING) return 2;
    return 3 + sc.materials[sc.prims[gprim].material_id].kind;
}
// Scenes with several Material alternatives or an environment map: the lanes of a wave would each take another branch of shade_path
// (disney_bsdf.xml: 42 % of lanes active per instruction).  Such a feature set sorts every 256-path chunk by shade_key first.
template <class Ft> struct ShadeSorted { static constexpr bool value = Ft::envmap || (Ft::kinds & (Ft::kinds - 1u)) != 0u; };

// Shade the `count` live paths at the front of one segment chunk by chunk; survivors are compacted to the front, in
// order (stable).  Returns the number of survivors (identical in every thread).  s_wcnt: 2 x (kBlock / 64) words of LDS.
// Sorted feature sets: within a chunk, thread t takes the t-th path in (key, slot) order — a counting sort by wave ballots, one LDS
// table of counts and one of slots — so that a wave's lanes run the same branch of shade_path; the survivors are then compacted in that
// order.  A path's value does not depend on where it sits in the queue (its radiance goes to sample_rgb[sample]), so images are unchanged.
template <class Ft, bool VIEWS>
__device__ __forceinline__ uint32_t shade_compact_segment(const DScene &sc, const DPass &pass, const DQueue &q, uint32_t base, uint32_t count, ShadeCounters &cnt, uint32_t (*s_oct)[kBlock / 64], bool octant_bin = false) {
    constexpr bool SORT = ShadeSorted<Ft>::value;
    __shared__ uint16_t s_perm[SORT ? kBlock : 1];
    __shared__ uint16_t s_kcnt[SORT ? kShadeKeys : 1][kBlock / 64];
    const uint32_t wave = threadIdx.x >> 6;
    uint32_t out = 0;  // survivors written so far (identical in every thread)
    for (uint32_t c0 = 0, it = 0; c0 < count; c0 += kBlock, it++) {
        uint32_t j = c0 + threadIdx.x;
        if (SORT) {
            const int key = j < count ? shade_key<Ft>(sc, q, base + j) : kShadeKeys;   // (slots beyond the live front sort last)
            uint32_t rank_in_key = 0;
#pragma unroll
            for (int k = 0; k < kShadeKeys; k++) {
                if (k >= 3 && !Ft::kind(k - 3)) continue;
                if (k == 1 && !Ft::envmap) { /* misses still exist without an environment map: they end the path */ }
                const unsigned long long m = __ballot(key == k);
                if (key == k) rank_in_key = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                if ((threadIdx.x & 63) == 0) s_kcnt[k][wave] = (uint16_t)__popcll(m);
            }
            __syncthreads();
            if (key < kShadeKeys) {
                uint32_t pos = rank_in_key;
#pragma unroll
                for (int k = 0; k < kShadeKeys; k++) {
                    if (k >= 3 && !Ft::kind(k - 3)) continue;
                    for (uint32_t w = 0; w < kBlock / 64; w++) { const uint32_t n = s_kcnt[k][w]; pos += (k < key || (k == key && w < wave)) ? n : 0u; }
                }
                s_perm[pos] = (uint16_t)threadIdx.x;
            }
            __syncthreads();
            const uint32_t live = count - c0 < kBlock ? count - c0 : kBlock;
            j = threadIdx.x < live ? c0 + s_perm[threadIdx.x] : count;
        }
        bool alive = false;
        PathState ps;
        if (j < count) {
            q_load_for_shade(q, base + j, ps);
            alive = shade_path<Ft, VIEWS>(sc, pass, ps, cnt);
            if (!alive) {
                float *o = pass.sample_rgb + 3ull * ps.sample;
                o[0] = ps.rad.x; o[1] = ps.rad.y; o[2] = ps.rad.z;
                cnt.done++;
            }
        }
        // every record of this chunk has been read (and consumed) once the threads meet in survivor_offset, so writing into
        // [out, out + survivors) — which never reaches past the end of this chunk — cannot overtake a read
        uint32_t total;
        const uint32_t off = survivor_offset(alive, ps, octant_bin, s_oct + (it & 1u) * 8u, total);
        if (alive) q_store(q, base + out + off, ps);
        out += total;
    }
    return out;
}

// The same with the WHOLE live front of the segment sorted by shade_key, not each 256-path chunk of it (k_shade, scenes with several
// Material alternatives or an environment map).  Why: a chunk costs what its slowest wave costs — with the chunk's paths sorted that
// is still the wave that got the heaviest class (disney_bsdf.xml: the Disney BSDF on 15 % of the paths), while the other three wait
// at the chunk's barrier; sorted over the whole segment, most chunks hold ONE class and cost what that class costs.  Three passes over
// the front: (1) keys (one byte per path, kept in `sb.keys`) and their histogram, (2) a stable scatter of the slot numbers into
// `sb.perm` (key-major), (3) shading in that order — reading the queue records of slot perm[t] from `q` and writing the survivors,
// compacted, to `qo`: a SECOND set of queue records, because a path read from anywhere in the segment may not be overwritten by an
// earlier survivor.  The extend launch that follows works on `qo`; the two sets swap roles every step.
template <class Ft, bool VIEWS>
__device__ __forceinline__ uint32_t shade_sorted_segment(const DScene &sc, const DPass &pass, const DQueue &q, const DQueue &qo, const ShadeSortBuf &sb, uint32_t base, uint32_t count,
                                                         ShadeCounters &cnt, uint32_t (*s_oct)[kBlock / 64]) {
    __shared__ uint32_t s_start[kShadeKeys];
    __shared__ uint16_t s_kc[kShadeKeys][kBlock / 64];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    if (threadIdx.x < kShadeKeys) s_start[threadIdx.x] = 0u;
    __syncthreads();
    // ---- (1) keys and histogram
    for (uint32_t c0 = 0; c0 < count; c0 += kBlock) {
        const uint32_t j = c0 + threadIdx.x;
        const int key = j < count ? shade_key<Ft>(sc, q, base + j) : kShadeKeys;
        if (j < count) sb.keys[base + j] = (uint8_t)key;
#pragma unroll
        for (int k = 0; k < kShadeKeys; k++) {
            if (k >= 3 && !Ft::kind(k - 3)) continue;
            const unsigned long long m = __ballot(key == k);
            if (lane == 0u && m != 0ull) atomicAdd(&s_start[k], (uint32_t)__popcll(m));
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) { uint32_t run = 0; for (int k = 0; k < kShadeKeys; k++) { const uint32_t c = s_start[k]; s_start[k] = run; run += c; } }
    __syncthreads();
    // ---- (2) slot numbers in (key, slot) order
    for (uint32_t c0 = 0; c0 < count; c0 += kBlock) {
        const uint32_t j = c0 + threadIdx.x;
        const int key = j < count ? (int)sb.keys[base + j] : kShadeKeys;
        uint32_t rank_in_key = 0;
#pragma unroll
        for (int k = 0; k < kShadeKeys; k++) {
            if (k >= 3 && !Ft::kind(k - 3)) continue;
            const unsigned long long m = __ballot(key == k);
            if (key == k) rank_in_key = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            if (lane == 0u) s_kc[k][wave] = (uint16_t)__popcll(m);
        }
        __syncthreads();
        if (key < kShadeKeys) {
            uint32_t pos = s_start[key] + rank_in_key;
            for (uint32_t w = 0; w < wave; w++) pos += s_kc[key][w];
            sb.perm[base + pos] = j;
        }
        __syncthreads();
        if (threadIdx.x < kShadeKeys) {
            const int k = (int)threadIdx.x;
            if (k < 3 || Ft::kind(k - 3)) { uint32_t n = 0; for (uint32_t w = 0; w < kBlock / 64; w++) n += s_kc[k][w]; s_start[k] += n; }
        }
        __syncthreads();
    }
    // ---- (3) shade in that order; survivors compacted into the other record set
    uint32_t out = 0;
    for (uint32_t c0 = 0, it = 0; c0 < count; c0 += kBlock, it++) {
        const uint32_t t = c0 + threadIdx.x;
        bool alive = false;
        PathState ps;
        if (t < count) {
            const uint32_t j = sb.perm[base + t];
            q_load_for_shade(q, base + j, ps);
            alive = shade_path<Ft, VIEWS>(sc, pass, ps, cnt);
            if (!alive) {
                float *o = pass.sample_rgb + 3ull * ps.sample;
                o[0] = ps.rad.x; o[1] = ps.rad.y; o[2] = ps.rad.z;
                cnt.done++;
            }
        }
        uint32_t total;
        const uint32_t off = survivor_offset(alive, ps, sb.octant_bin != 0u, s_oct + (it & 1u) * 8u, total);
        if (alive) q_store(qo, base + out + off, ps);
        out += total;
    }
    return out;
}

// (the feature sets the shade kernel is compiled for — FeatLambert ... FeatAll — are listed in dshade.h)
#ifndef LJ_LAMBERT_OCC
#define LJ_LAMBERT_OCC 4
#endif
#ifndef LJ_SHADE_OCC
#define LJ_SHADE_OCC 3   // the feature sets beyond Lambert-only need 140 - 165 VGPRs: at 4 waves they spill (matpreview -3 % at 3)
#endif
#ifndef LJ_SHADE_OCC_LARGE
#define LJ_SHADE_OCC_LARGE 4   // ... but the two that run alone on the GPU beside a large tree's extend launches (one lane) gain from the fourth wave:
#endif                         // sponza 256 spp 200.0 -> 196.8 ms (shade alone -6.5 %), disney_bsdf 256 spp 91.6 -> 89.9 (tools/variant_ab.sh)
template <class Ft> struct ShadeOccupancy { static constexpr int waves = LJ_SHADE_OCC; };
template <> struct ShadeOccupancy<FeatLambert> { static constexpr int waves = LJ_LAMBERT_OCC; };
template <> struct ShadeOccupancy<FeatLambertTex> { static constexpr int waves = LJ_SHADE_OCC_LARGE; };
template <> struct ShadeOccupancy<FeatDisney> { static constexpr int waves = LJ_SHADE_OCC_LARGE; };

// RAYS: the pass is a table of rays or probes (DPass::ray_kind, dprobe.h): the refill loop starts paths from the table's entries instead of
// camera samples.  A compile-time switch like VIEWS, and for its reason: tested at run time it moved the spilled registers of every
// single-camera instantiation.  The RAYS instantiations are compiled in a translation unit of their own, shade_rays.hip.
template <class Ft, int STAGE, bool VIEWS, bool RAYS = false>
__global__ void __launch_bounds__(kBlock, ShadeOccupancy<Ft>::waves) k_shade(DScene sc, DPass pass, DQueue q, DQueue qo, ShadeSortBuf sb, DBlockState *blocks, uint32_t seg, ShadeStage stg, uint32_t *work, uint32_t *chunk_list, uint32_t parity, uint32_t extend_waves) {
    __shared__ uint32_t s_list_base;
    if (blockIdx.x == 0 && threadIdx.x == 0) work[0] = extend_waves;   // the extend launch that follows draws list entries beyond its own waves from it
    __shared__ uint32_t s_wcnt[16][kBlock / 64];   // two tables of (octant x wave) survivor counts, used alternately
    __shared__ unsigned long long s_cnt[5];
    stage_shade_tables<STAGE>(sc, stg, 0u);
    DBlockState &bs = blocks[blockIdx.x];
    const uint32_t count = bs.count, next_sample = bs.next_sample, end_sample = bs.end_sample;
    if (threadIdx.x < 5) s_cnt[threadIdx.x] = 0ull;
    __syncthreads();
    ShadeCounters cnt; cnt.bounces = cnt.closest = cnt.shadow = cnt.done = 0;
    const uint32_t base = blockIdx.x * seg;
    // ---- shade the live front of the segment chunk by chunk; survivors are compacted to the front, in order
    // (qo: the record set the survivors go to — `q` itself unless the segment is sorted as a whole, shade_sorted_segment)
    uint32_t out;
    if (ShadeSorted<Ft>::value && sb.perm != nullptr) out = shade_sorted_segment<Ft, VIEWS>(sc, pass, q, qo, sb, base, count, cnt, s_wcnt);
    else out = shade_compact_segment<Ft, VIEWS>(sc, pass, q, base, count, cnt, s_wcnt, sb.octant_bin != 0u);
    // ---- refill the rest of the segment with the workgroup's next camera samples (path_tracing.h:10-14)
    const uint32_t left = end_sample - next_sample, room = seg - out;
    const uint32_t n_new = left < room ? left : room;
    for (uint32_t g = threadIdx.x; g < n_new; g += kBlock) {
        PathState ps;
        if constexpr (RAYS) generate_ray_path(sc, pass, next_sample + g, ps);
        else generate_path<VIEWS>(sc, pass, next_sample + g, ps);
        q_store(qo, base + out + g, ps);
    }
    const uint32_t b = wave_sum(cnt.bounces), cl = wave_sum(cnt.closest), sh = wave_sum(cnt.shadow), dn = wave_sum(cnt.done);
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&s_cnt[0], (unsigned long long)b); atomicAdd(&s_cnt[1], (unsigned long long)cl); atomicAdd(&s_cnt[2], (unsigned long long)sh);
        atomicAdd(&s_cnt[3], (unsigned long long)dn);
    }
    __syncthreads();
    // list this segment's live chunks for the extend launch (one atomic per workgroup)
    const uint32_t live_chunks = (out + n_new + kChunk - 1) / kChunk;
    if (threadIdx.x == 0) s_list_base = live_chunks ? atomicAdd(&work[1 + parity], live_chunks) : 0u;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < live_chunks; i += kBlock) chunk_list[s_list_base + i] = blockIdx.x * (seg / kChunk) + i;
    if (threadIdx.x == 0) {
        bs.next_sample = next_sample + n_new;
        bs.count = out + n_new;
        bs.bounce_iterations += s_cnt[0]; bs.rays_closest += s_cnt[1]; bs.rays_shadow += s_cnt[2]; bs.samples_done += s_cnt[3]; bs.path_steps += count;
    }
}

// ---------------------------------------------------------------- the tail of a render, fused
// When no camera sample is left to start and only the long-lived paths remain, a launch pair per bounce is mostly launch
// overhead (~10 us each, tens of bounces).  A workgroup's segment is independent of every other one, so the rest of the
// render runs inside ONE launch: each workgroup alternates "trace my live paths" and "shade + compact my segment" until
// its segment is empty.  Per-sample values are the same as with separate launches, bit for bit.
template <class Ft, bool VIEWS>
__global__ void __launch_bounds__(kBlock, 2) k_tail(DScene sc, DPass pass, DQueue q, DBlockState *blocks, uint32_t seg, ShadeStage stg, uint32_t shade_lds_at,
                                                    int stack, int lds_nodes, int lds_prims, int *spill) {
    __shared__ uint32_t s_wcnt[16][kBlock / 64];   // two tables of (octant x wave) survivor counts, used alternately
    const TreeView tv = stage_tree(sc, stack, lds_nodes, lds_prims, spill, gridDim.x * kBlock, blockIdx.x * kBlock + threadIdx.x);
    DScene ssc = sc;                       // the shading view of the scene: tables in LDS
    stage_shade_tables<-1>(ssc, stg, shade_lds_at);
    __syncthreads();
    DBlockState &bs = blocks[blockIdx.x];
    uint32_t count = bs.count;
    const uint32_t base = blockIdx.x * seg;
    ShadeCounters cnt; cnt.bounces = cnt.closest = cnt.shadow = cnt.done = 0;
    unsigned long long path_steps = 0;
    for (int guard = 0; guard < (1 << 16) && count > 0; guard++) {
        // ---- extend: one lane per path, shadow ray (any hit) then extension ray (closest hit)
        for (uint32_t i = threadIdx.x; i < count; i += kBlock) {
            const uint32_t path = base + i;
            const Rec4 ro = q.ro[path], rd = q.rd[path];
            const uint32_t flags = f2u(rd.w);
            LaneTrav L;
            L.ray.ox = ro.x; L.ray.oy = ro.y; L.ray.oz = ro.z;
            uint32_t vis = 0;
            if (ro.w > 0.0f) {
                const Rec4 rs = q.rs[path];
                L.ray.dx = rs.x; L.ray.dy = rs.y; L.ray.dz = rs.z;
                trav_begin(L, sc.eps, ro.w);
                trace_lane(tv, L, true);
                vis = (L.best.gprim < 0) ? (uint32_t)HIT_VIS_BIT : 0u;
            }
            if (!(flags & PF_NO_EXT)) {
                L.ray.dx = rd.x; L.ray.dy = rd.y; L.ray.dz = rd.z;
                trav_begin(L, ((flags & 0xffffu) == 2u) ? 0.0f : sc.eps, INFINITY);
                trace_lane(tv, L, false);
                trav_finish(L);
                const bool hit = L.best.gprim >= 0;
                q.rh[path] = mk4(hit ? L.best.t : 0.0f, L.best.u, L.best.v, u2f(vis | (uint32_t)(L.best.gprim + 1)));
            } else q.rh[path] = mk4(0.0f, 0.0f, 0.0f, u2f(vis));
        }
        __syncthreads();   // (workgroup-scope release/acquire of the records just written)
        // ---- shade + compact
        path_steps += count;
        count = shade_compact_segment<Ft, VIEWS>(ssc, pass, q, base, count, cnt, s_wcnt);
        __syncthreads();
    }
    __shared__ unsigned long long s_cnt[4];
    if (threadIdx.x < 4) s_cnt[threadIdx.x] = 0ull;
    __syncthreads();
    const uint32_t b = wave_sum(cnt.bounces), cl = wave_sum(cnt.closest), sh = wave_sum(cnt.shadow), dn = wave_sum(cnt.done);
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&s_cnt[0], (unsigned long long)b); atomicAdd(&s_cnt[1], (unsigned long long)cl); atomicAdd(&s_cnt[2], (unsigned long long)sh);
        atomicAdd(&s_cnt[3], (unsigned long long)dn);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        bs.count = count;
        bs.bounce_iterations += s_cnt[0]; bs.rays_closest += s_cnt[1]; bs.rays_shadow += s_cnt[2]; bs.samples_done += s_cnt[3]; bs.path_steps += path_steps;
    }
}

// shade_rays.hip: launch_shade for a pass over a table of rays or probes — the RAYS instantiations of k_shade
void launch_shade_rays(const DScene &sc, const DPass &pass, const DQueue &q, const DQueue &qo, uint32_t *sort_perm, uint8_t *sort_keys, DBlockState *blocks, uint32_t n_blocks, uint32_t seg, const ShadeConfig &cfg, uint32_t *work, uint32_t *chunk_list, uint32_t parity, uint32_t extend_waves, hipStream_t s);

// launch_shade's choice of instantiation for one kind of pass: feature set and staging from the scene's ShadeConfig
template <bool VIEWS, bool RAYS>
static void launch_shade_kind(const DScene &sc, const DPass &pass, const DQueue &q, const DQueue &qo, uint32_t *sort_perm, uint8_t *sort_keys, DBlockState *blocks, uint32_t n_blocks, uint32_t seg, const ShadeConfig &cfg, uint32_t *work, uint32_t *chunk_list, uint32_t parity, uint32_t extend_waves, hipStream_t s) {
    ShadeSortBuf sb; sb.perm = sort_perm; sb.keys = sort_keys;
    sb.octant_bin = (getenv("LJ_TUNE_OCTANT_BIN") && atoi(getenv("LJ_TUNE_OCTANT_BIN")) != 0) ? 1u : 0u;
    const ShadeStage st = make_shade_stage(cfg);
    auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(n_blocks), dim3(kBlock), cfg.smem, s, sc, pass, q, qo, sb, blocks, seg, st, work, chunk_list, parity, extend_waves); };
    // (a scene whose tables are not staged at all runs the all-features instantiation: lj_scene_upload picks it)
    const int stage = cfg.smem == 0 ? 0 : (cfg.stage_prims ? 2 : 1);
    if (stage == 0) { launch(k_shade<FeatAll, 0, VIEWS, RAYS>); return; }
    with_shade_variant(cfg.variant, [&](auto ft) {
        using Ft = decltype(ft);
        if (stage == 2) launch(k_shade<Ft, 2, VIEWS, RAYS>); else launch(k_shade<Ft, 1, VIEWS, RAYS>);
    });
}

#ifdef LJ_SHADE_RAYS_UNIT   // shade_rays.hip: the templates above, and this launcher alone
void launch_shade_rays(const DScene &sc, const DPass &pass, const DQueue &q, const DQueue &qo, uint32_t *sort_perm, uint8_t *sort_keys, DBlockState *blocks, uint32_t n_blocks, uint32_t seg, const ShadeConfig &cfg, uint32_t *work, uint32_t *chunk_list, uint32_t parity, uint32_t extend_waves, hipStream_t s) {
    launch_shade_kind<false, true>(sc, pass, q, qo, sort_perm, sort_keys, blocks, n_blocks, seg, cfg, work, chunk_list, parity, extend_waves, s);
}
#else
// ---------------------------------------------------------------- resolve: radiance / spp, deterministic
// One wave per pixel; lanes stride over the pixel's samples, then a fixed xor-butterfly combines the 64 partials.
__global__ void __launch_bounds__(kBlock) k_resolve(DPass pass, uint32_t n_pixels, float *rgb) {
    const uint32_t wave = (blockIdx.x * kBlock + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (wave >= n_pixels) return;
    const float *src = pass.sample_rgb + 3ull * (uint64_t)wave * pass.spp;
    float r = 0.0f, g = 0.0f, b = 0.0f;
    for (uint32_t s = lane; s < pass.spp; s += 64) { r += src[3 * s]; g += src[3 * s + 1]; b += src[3 * s + 2]; }
    for (int o = 32; o > 0; o >>= 1) { r += __shfl_xor(r, o, 64); g += __shfl_xor(g, o, 64); b += __shfl_xor(b, o, 64); }
    if (lane == 0) {
        const uint32_t pixel = pass.pixel_list[wave];
        const float inv = div_ieee(1.0f, (float)pass.spp);
        rgb[3ull * pixel] = r * inv; rgb[3ull * pixel + 1] = g * inv; rgb[3ull * pixel + 2] = b * inv;
    }
}

// ---------------------------------------------------------------- launchers (called from render.hip)
// LDS staging plan of the shade kernel; sizes are rounded up to 16 bytes (the device buffers are padded accordingly).
ShadeConfig shade_config(size_t n_prims, size_t n_materials, size_t n_lights, size_t n_light_tris, size_t n_light_tri_cdf, size_t n_images3, size_t n_images1, size_t n_env_marg) {
    auto r16 = [](size_t b) { return (uint32_t)((b + 15) & ~(size_t)15); };
    ShadeConfig c{};
    c.variant = kShadeVariantAll;
    c.materials_bytes = r16(n_materials * sizeof(DMaterial)); c.lights_bytes = r16(n_lights * sizeof(DLight));
    c.light_cdf_bytes = r16((n_lights + 1) * 4); c.light_tris_bytes = r16(n_light_tris * sizeof(DLightTri)); c.light_tri_cdf_bytes = r16(n_light_tri_cdf * 4);
    size_t small = (size_t)c.materials_bytes + c.lights_bytes + c.light_cdf_bytes + c.light_tris_bytes + c.light_tri_cdf_bytes;
    if (small > 24 * 1024) {  // too many materials / emissive triangles: leave everything in global memory
        c = ShadeConfig{}; c.variant = kShadeVariantAll; c.smem = 0; return c;
    }
    c.prims_bytes = r16(n_prims * sizeof(DPrimShade));
    c.stage_prims = (small + c.prims_bytes <= 32 * 1024) ? 1u : 0u;
    if (!c.stage_prims) c.prims_bytes = 0;
    c.smem = small + c.prims_bytes;
    // beside those, while they stay small: the image descriptors (the first, dependent, load of every texture lookup) and the
    // environment map's marginal cdf / pdf / guide (its first search then never leaves the CU)
    const uint32_t img3 = r16(n_images3 * sizeof(DImage)), img1 = r16(n_images1 * sizeof(DImage)), marg = r16(n_env_marg * 4);
    if (!(getenv("LJ_TUNE_STAGE_IMAGES") && atoi(getenv("LJ_TUNE_STAGE_IMAGES")) == 0)) {
        if (img3 + img1 <= 8 * 1024) { c.images3_bytes = img3; c.images1_bytes = img1; c.smem += img3 + img1; }
        if (n_env_marg > 0 && marg <= 8 * 1024) { c.env_marg_bytes = marg; c.smem += marg; }
    }
    return c;
}

// shade_variant() returns the first (smallest) feature set that covers a scene — or `preferred`, where that is one and covers the scene too.
// (The sets are not ordered by what they hold: FeatDisney, 4, has no roughplastic.  A path on a Material alternative its kernel lacks gets
// no slot in the kernel's sort, so a set that does not cover the scene must never run.)
int shade_variant(uint32_t kinds, bool textured, bool envmap, bool sphere_lights, int preferred) {
    if (preferred >= 0 && preferred < kNumShadeVariants && variant_covers(preferred, kinds, textured, envmap, sphere_lights)) return preferred;
    for (int v = 0; v < kNumShadeVariants; v++) if (variant_covers(v, kinds, textured, envmap, sphere_lights)) return v;
    return kNumShadeVariants - 1;
}

bool shade_sorts_segments(const ShadeConfig &cfg) {   // feature sets whose k_shade sorts a segment as a whole (they need the second record set + sort buffers)
    if (const char *e = getenv("LJ_TUNE_SHADE_SORT")) { if (atoi(e) < 2) return false; }
    bool sorted = false;
    if (cfg.smem == 0) return ShadeSorted<FeatAll>::value;
    with_shade_variant(cfg.variant, [&](auto ft) { sorted = ShadeSorted<decltype(ft)>::value; });
    return sorted;
}
void launch_shade(const DScene &sc, const DPass &pass, const DQueue &q, const DQueue &qo, uint32_t *sort_perm, uint8_t *sort_keys, DBlockState *blocks, uint32_t n_blocks, uint32_t seg, const ShadeConfig &cfg, uint32_t *work, uint32_t *chunk_list, uint32_t parity, uint32_t extend_waves, hipStream_t s) {
    // (a table of rays, DPass::ray_kind, runs the RAYS instantiations of shade_rays.hip; a batch of cameras, DPass::views, the VIEWS ones: dshade.h)
    if (pass.ray_kind != RAY_SOURCE_NONE) launch_shade_rays(sc, pass, q, qo, sort_perm, sort_keys, blocks, n_blocks, seg, cfg, work, chunk_list, parity, extend_waves, s);
    else if (pass.views) launch_shade_kind<true, false>(sc, pass, q, qo, sort_perm, sort_keys, blocks, n_blocks, seg, cfg, work, chunk_list, parity, extend_waves, s);
    else launch_shade_kind<false, false>(sc, pass, q, qo, sort_perm, sort_keys, blocks, n_blocks, seg, cfg, work, chunk_list, parity, extend_waves, s);
}
// LDS the fused tail needs: the extend image followed by the shade tables; 0 when that does not fit one workgroup's share
size_t tail_smem(const ExtendConfig &ecfg, const ShadeConfig &scfg) {
    const size_t at = (ecfg.smem + 15) & ~(size_t)15, total = at + scfg.smem;
    return total <= 64 * 1024 ? total : 0;
}
void launch_tail(const DScene &sc, const DPass &pass, const DQueue &q, DBlockState *blocks, uint32_t n_blocks, uint32_t seg, const ExtendConfig &ecfg, const ShadeConfig &scfg, int *spill, hipStream_t s) {
    const ShadeStage st = make_shade_stage(scfg);
    const uint32_t at = (uint32_t)((ecfg.smem + 15) & ~(size_t)15);
    const size_t smem = tail_smem(ecfg, scfg);
    auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(n_blocks), dim3(kBlock), smem, s, sc, pass, q, blocks, seg, st, at, ecfg.stack, ecfg.lds_nodes, ecfg.lds_prims, spill); };
    with_shade_variant(scfg.variant, [&](auto ft) { if (pass.views) launch(k_tail<decltype(ft), true>); else launch(k_tail<decltype(ft), false>); });
}
void launch_resolve(const DPass &pass, uint32_t n_pixels, float *rgb, hipStream_t s) {
    const uint32_t waves_per_block = kBlock / 64;
    const uint32_t grid = (n_pixels + waves_per_block - 1) / waves_per_block;
    if (grid) hipLaunchKernelGGL(k_resolve, dim3(grid), dim3(kBlock), 0, s, pass, n_pixels, rgb);
}
#endif   // LJ_SHADE_RAYS_UNIT

} // namespace ljd
