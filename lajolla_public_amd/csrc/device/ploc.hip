// Kernels of lj_scene_rebuild_bvh_ex with LJ_BUILD_PLOC: the clustering of device/dploc.h over the sorted primitives that
// the first half of rebuild.hip leaves.  A round over m clusters is four launches:
//   k_ploc_nearest  lane/cluster : the position each cluster chooses, from a workgroup's 256 + 2 radius boxes staged in LDS
//   k_ploc_flag     lane/cluster : what each position does (dploc.h ploc_role), and per tile of 256 how many stay and how many pairs merge
//   k_ploc_scan     one group    : exclusive prefix sums of both tile counts, and the totals (the next m, the nodes written)
//   k_ploc_scatter  lane/cluster : the nodes of the merging pairs and the next round's clusters, into the other half of a ping-pong
// and the host reads the next m.  Where a cluster lands and which node a pair writes are functions of the flags alone (ballot ranks, no
// atomics), so the result does not depend on the grid.  Once m <= kPlocTail, k_ploc_tail runs the remaining rounds in one workgroup with the
// clusters in LDS and barriers between a round's steps; its loop is bounded by m - 1 rounds, each of which merges at least one pair.
// No kernel spins, no lane waits for another workgroup, and no fences are needed: a merged box is computed where it is merged.
#include "api_internal.h"
#include "dploc.h"

namespace ljd {

namespace {

constexpr int kPlocBlock = 256, kPlocWaves = kPlocBlock / 64;
constexpr int kPlocTile = kPlocBlock + 2 * kPlocRadiusMax;   // boxes a workgroup stages
constexpr int kPlocTailWaves = kPlocTail / 64;
static_assert(kPlocTail == 1024, "k_ploc_tail is one workgroup of 1024 lanes, one per cluster");

struct PlocClusters { RefitBox *box; int32_t *id, *count; };

// Six planes of `stride` floats each, position `base` first: conflict-free whichever plane a wave reads
struct PlaneBoxes {
    const float *planes; int stride, base;
    __device__ RefitBox operator()(int j) const {
        RefitBox b;
        for (int k = 0; k < 3; k++) { b.lo[k] = planes[k * stride + (j - base)]; b.hi[k] = planes[(3 + k) * stride + (j - base)]; }
        return b;
    }
};
__device__ __forceinline__ void put_box(float *planes, int stride, int at, const RefitBox &b) {
    for (int k = 0; k < 3; k++) { planes[k * stride + at] = b.lo[k]; planes[(3 + k) * stride + at] = b.hi[k]; }
}

__device__ __forceinline__ uint32_t ballot_rank(unsigned long long b) { return __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u)); }

__global__ void __launch_bounds__(kPlocBlock) k_ploc_init(const RefitBox *boxes, const int32_t *order, int n, PlocClusters out) {
    for (int p = (int)(blockIdx.x * blockDim.x + threadIdx.x); p < n; p += (int)(gridDim.x * blockDim.x)) {
        const int g = order[p];
        if (g < 0 || g >= n) continue;   // (the host checks the order it reads back and refuses the build)
        out.box[p] = boxes[g]; out.id[p] = ~p; out.count[p] = 1;
    }
}

// tile t: positions [256 t, 256 t + 256) of the m >= 2 clusters
__global__ void __launch_bounds__(kPlocBlock) k_ploc_nearest(const RefitBox *box, int m, int radius, int n_tiles, int32_t *nn) {
    __shared__ float planes[6 * kPlocTile];
    for (int t = (int)blockIdx.x; t < n_tiles; t += (int)gridDim.x) {   // (workgroup-uniform: every lane reaches the barriers)
        const int base = t * kPlocBlock - radius;
        for (int k = (int)threadIdx.x; k < kPlocBlock + 2 * radius; k += kPlocBlock) {
            const int j = base + k;
            if (j >= 0 && j < m) put_box(planes, kPlocTile, k, box[j]);
        }
        __syncthreads();
        const int i = t * kPlocBlock + (int)threadIdx.x;
        if (i < m) nn[i] = ploc_nearest(PlaneBoxes{planes, kPlocTile, base}, m, i, radius);
        __syncthreads();   // the next tile's writers wait for these readers
    }
}

// flags[i]: ploc_role of position i; counts[t]: x the positions of tile t that stay (roles 0 and 1), y its merging pairs (role 1)
__global__ void __launch_bounds__(kPlocBlock) k_ploc_flag(const int32_t *nn, int m, int n_tiles, uint8_t *flags, uint2 *counts) {
    __shared__ uint32_t wave_kept[kPlocWaves], wave_pairs[kPlocWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (int t = (int)blockIdx.x; t < n_tiles; t += (int)gridDim.x) {
        const int i = t * kPlocBlock + (int)threadIdx.x;
        const int role = i < m ? ploc_role(nn, i) : 2;
        if (i < m) flags[i] = (uint8_t)role;
        const unsigned long long kept = __ballot(role != 2), pairs = __ballot(role == 1);
        if (lane == 0u) { wave_kept[wave] = (uint32_t)__popcll(kept); wave_pairs[wave] = (uint32_t)__popcll(pairs); }
        __syncthreads();
        if (threadIdx.x == 0u) counts[t] = make_uint2((wave_kept[0] + wave_kept[1]) + (wave_kept[2] + wave_kept[3]), (wave_pairs[0] + wave_pairs[1]) + (wave_pairs[2] + wave_pairs[3]));
        __syncthreads();
    }
}

// one workgroup: offsets[t] = counts[0] + .. + counts[t - 1] in both components; total[0] = the clusters left, total[1] = the pairs merged
__global__ void __launch_bounds__(kPlocBlock) k_ploc_scan(const uint2 *counts, int n_tiles, uint2 *offsets, uint32_t *total) {
    __shared__ uint2 wave_sum[kPlocWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint2 carry = make_uint2(0u, 0u);
    for (int base = 0; base < n_tiles; base += kPlocBlock) {
        const int t = base + (int)threadIdx.x;
        const uint2 c = t < n_tiles ? counts[t] : make_uint2(0u, 0u);
        uint2 incl = c;   // inclusive scan over the wave
        for (uint32_t o = 1u; o < 64u; o <<= 1) {
            const uint32_t ux = (uint32_t)__shfl_up((int)incl.x, o, 64), uy = (uint32_t)__shfl_up((int)incl.y, o, 64);
            if (lane >= o) { incl.x += ux; incl.y += uy; }
        }
        if (lane == 63u) wave_sum[wave] = incl;
        __syncthreads();
        uint2 before = carry;
        for (uint32_t v = 0u; v < wave; v++) { before.x += wave_sum[v].x; before.y += wave_sum[v].y; }
        if (t < n_tiles) offsets[t] = make_uint2(before.x + (incl.x - c.x), before.y + (incl.y - c.y));
        for (int v = 0; v < kPlocWaves; v++) { carry.x += wave_sum[v].x; carry.y += wave_sum[v].y; }
        __syncthreads();
    }
    if (threadIdx.x == 0u) { total[0] = carry.x; total[1] = carry.y; }
}

// `done` nodes are written; next: the clusters of the next round (total[0] of them)
__global__ void __launch_bounds__(kPlocBlock) k_ploc_scatter(PlocClusters cur, int m, int n_tiles, const int32_t *nn, const uint8_t *flags, const uint2 *offsets, int done,
                                                           RebuildNode *nodes, PlocClusters next) {
    __shared__ uint32_t wave_kept[kPlocWaves], wave_pairs[kPlocWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (int t = (int)blockIdx.x; t < n_tiles; t += (int)gridDim.x) {
        const int i = t * kPlocBlock + (int)threadIdx.x;
        const int role = i < m ? (int)flags[i] : 2;
        const unsigned long long kept = __ballot(role != 2), pairs = __ballot(role == 1);
        if (lane == 0u) { wave_kept[wave] = (uint32_t)__popcll(kept); wave_pairs[wave] = (uint32_t)__popcll(pairs); }
        __syncthreads();
        const uint2 off = offsets[t];
        uint32_t to = off.x + ballot_rank(kept), pair = off.y + ballot_rank(pairs);
        for (uint32_t v = 0u; v < wave; v++) { to += wave_kept[v]; pair += wave_pairs[v]; }
        if (role == 1) {
            const int j = nn[i];
            RebuildNode nd;
            ploc_merge(cur.box[i], cur.box[j], cur.id[i], cur.id[j], cur.count[i], cur.count[j], nd);
            const int at = done + (int)pair;
            nodes[at] = nd;
            next.box[to] = nd.box; next.id[to] = at; next.count[to] = nd.count;
        } else if (role == 0) {
            next.box[to] = cur.box[i]; next.id[to] = cur.id[i]; next.count[to] = cur.count[i];
        }
        __syncthreads();
    }
}

// The rounds from m <= kPlocTail clusters down to one, lane = position.  total[0]: the clusters left (1), [1]: the nodes written in all, [2]: rounds
__global__ void __launch_bounds__(kPlocTail) k_ploc_tail(PlocClusters cur, int m0, int radius, int done0, RebuildNode *nodes, uint32_t *total) {
    __shared__ float planes[6 * kPlocTail];
    __shared__ int32_t ids[kPlocTail], counts[kPlocTail], nn[kPlocTail];
    __shared__ uint32_t wave_kept[kPlocTailWaves], wave_pairs[kPlocTailWaves];
    const int tid = (int)threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (tid < m0) { put_box(planes, kPlocTail, tid, cur.box[tid]); ids[tid] = cur.id[tid]; counts[tid] = cur.count[tid]; }
    __syncthreads();
    const PlaneBoxes box_at{planes, kPlocTail, 0};
    int m = m0, done = done0, rounds = 0;   // (the same in every lane: the barriers below are reached by all)
    for (; rounds < m0 - 1 && m > 1; rounds++) {
        if (tid < m) nn[tid] = ploc_nearest(box_at, m, tid, radius);
        __syncthreads();
        const int role = tid < m ? ploc_role(nn, tid) : 2;
        RebuildNode nd{};
        if (role == 1) { const int j = nn[tid]; ploc_merge(box_at(tid), box_at(j), ids[tid], ids[j], counts[tid], counts[j], nd); }
        else if (role == 0) { nd.box = box_at(tid); nd.left = ids[tid]; nd.count = counts[tid]; }
        const unsigned long long kept = __ballot(role != 2), pairs = __ballot(role == 1);
        if (lane == 0u) { wave_kept[wave] = (uint32_t)__popcll(kept); wave_pairs[wave] = (uint32_t)__popcll(pairs); }
        __syncthreads();   // every lane has read the round's clusters
        uint32_t to = ballot_rank(kept), pair = ballot_rank(pairs), all_kept = 0u, all_pairs = 0u;
        for (uint32_t v = 0u; v < (uint32_t)kPlocTailWaves; v++) {
            if (v < wave) { to += wave_kept[v]; pair += wave_pairs[v]; }
            all_kept += wave_kept[v]; all_pairs += wave_pairs[v];
        }
        if (role == 1) {
            const int at = done + (int)pair;
            nodes[at] = nd;
            put_box(planes, kPlocTail, (int)to, nd.box); ids[to] = at; counts[to] = nd.count;
        } else if (role == 0) {
            put_box(planes, kPlocTail, (int)to, nd.box); ids[to] = nd.left; counts[to] = nd.count;
        }
        m = (int)all_kept; done += (int)all_pairs;
        __syncthreads();
    }
    if (tid == 0) { total[0] = (uint32_t)m; total[1] = (uint32_t)done; total[2] = (uint32_t)rounds; }
}

int ploc_grid(int n) { return std::max(1, std::min((n + kPlocBlock - 1) / kPlocBlock, 2048)); }

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

} // namespace

PlocWork ploc_carve(void *ws, int n) {
    PlocWork w{};
    const size_t m = (size_t)std::max(n, 1), tiles = (m + kPlocBlock - 1) / kPlocBlock;
    size_t at = 0;
    auto take = [&](size_t bytes) { void *p = ws ? (char *)ws + at : nullptr; at += align256(bytes); return p; };
    for (int h = 0; h < 2; h++) { w.box[h] = take(m * sizeof(RefitBox)); w.id[h] = (int32_t *)take(m * 4); w.count[h] = (int32_t *)take(m * 4); }
    w.nn = (int32_t *)take(m * 4);
    w.flags = (uint8_t *)take(m);
    w.counts = take(tiles * 8); w.offsets = take(tiles * 8);
    w.total = (uint32_t *)take(4 * 4);
    w.bytes = at;
    return w;
}

// From w.boxes[0 .. n): w.order and, for n >= 2, the n - 1 nodes of the clustering in w.nodes (node n - 2 is the root).  Waits for the stream
// once per round; host_word: four pinned words.  finished = false: kPlocMaxRounds rounds left more than `tail` clusters.
PlocRun launch_ploc(const RebuildWork &w, const PlocWork &p, int n, int radius, int tail, uint32_t *host_word, hipStream_t s) {
    PlocRun run{};
    run.finished = true;
    if (n <= 0) return run;
    launch_rebuild_order(w, n, s);
    if (n < 2) return run;
    radius = std::min(std::max(radius, 1), kPlocRadiusMax);
    tail = std::min(std::max(tail, 1), kPlocTail);
    RebuildNode *nodes = (RebuildNode *)w.nodes;
    PlocClusters half[2];
    for (int h = 0; h < 2; h++) half[h] = PlocClusters{(RefitBox *)p.box[h], p.id[h], p.count[h]};
    hipLaunchKernelGGL(k_ploc_init, dim3(ploc_grid(n)), dim3(kPlocBlock), 0, s, (const RefitBox *)w.boxes, (const int32_t *)w.order, n, half[0]);
    int m = n, done = 0, cur = 0;
    while (m > tail) {
        if (run.rounds == (uint64_t)kPlocMaxRounds) { run.finished = false; HIP_CHECK(hipStreamSynchronize(s)); return run; }
        const int tiles = (m + kPlocBlock - 1) / kPlocBlock, grid = ploc_grid(m);
        hipLaunchKernelGGL(k_ploc_nearest, dim3(grid), dim3(kPlocBlock), 0, s, (const RefitBox *)half[cur].box, m, radius, tiles, p.nn);
        hipLaunchKernelGGL(k_ploc_flag, dim3(grid), dim3(kPlocBlock), 0, s, (const int32_t *)p.nn, m, tiles, p.flags, (uint2 *)p.counts);
        hipLaunchKernelGGL(k_ploc_scan, dim3(1), dim3(kPlocBlock), 0, s, (const uint2 *)p.counts, tiles, (uint2 *)p.offsets, p.total);
        hipLaunchKernelGGL(k_ploc_scatter, dim3(grid), dim3(kPlocBlock), 0, s, half[cur], m, tiles, (const int32_t *)p.nn, (const uint8_t *)p.flags, (const uint2 *)p.offsets, done, nodes, half[cur ^ 1]);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(host_word, p.total, 4, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        const int left = (int)host_word[0];
        if (left < 1 || left >= m) throw LjError(LJ_ERR_INTERNAL, "the clustering's round merged nothing");
        done += m - left; m = left; cur ^= 1; run.rounds++;
    }
    if (m > 1) {
        hipLaunchKernelGGL(k_ploc_tail, dim3(1), dim3(kPlocTail), 0, s, half[cur], m, radius, done, nodes, p.total);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(host_word, p.total, 3 * 4, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (host_word[0] != 1u || host_word[1] != (uint32_t)(n - 1)) throw LjError(LJ_ERR_INTERNAL, "the clustering's last rounds did not end in one root");
        run.tail_rounds = host_word[2]; run.rounds += host_word[2];
    }
    return run;
}

} // namespace ljd
