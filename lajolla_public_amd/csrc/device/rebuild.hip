// Kernels of lj_scene_rebuild_bvh: a linear BVH built on the device from the primitives as they stand there.  Box scatter,
// centroid bounds and Morton codes are bounded grid-stride passes with one lane per primitive; the order is rocprim's radix sort of
// (code, primitive) pairs (least significant digit first, so equal codes keep their input order); the hierarchy is one lane per node; the
// boxes are fitted by one lane per sorted primitive that walks up the tree behind a per-node arrival counter: the first lane to arrive at a
// node stops, the second computes the node from both children in left-right order and goes on.  No lane waits for another, no loop spins,
// every walk is bounded by the tree's depth.  The arithmetic is device/drebuild.h, which the host twin runs too.
#include "api_internal.h"
#include "drebuild.h"
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>

namespace ljd {

namespace {

constexpr int kRebuildBlock = 256;

__global__ void __launch_bounds__(kRebuildBlock) k_rebuild_prim_boxes(const DPrim *leaf_prims, int n_leaf_prims, const DSphere *spheres, RefitBox *boxes, int n) {
    for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < n_leaf_prims; i += (int)(gridDim.x * blockDim.x)) {
        const DPrim p = leaf_prims[i];
        if (p.gprim < 0 || p.gprim >= n) continue;
        RefitBox b; refit_prim_box(p, spheres, b);
        boxes[p.gprim] = b;   // (the references a spatial split duplicated write the same value)
    }
}

// bounds[0..2]: keys of the centroid minima, [3..5]: of the maxima (rebuild_key); preset to ~0 and 0
__global__ void __launch_bounds__(kRebuildBlock) k_rebuild_bounds(const RefitBox *boxes, int n, unsigned long long *bounds) {
    unsigned long long lo[3] = {~0ull, ~0ull, ~0ull}, hi[3] = {0ull, 0ull, 0ull};
    for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < n; i += (int)(gridDim.x * blockDim.x)) {
        const RefitBox b = boxes[i];
        for (int k = 0; k < 3; k++) {
            const unsigned long long key = rebuild_key(rebuild_centroid(b, k));
            lo[k] = key < lo[k] ? key : lo[k]; hi[k] = key > hi[k] ? key : hi[k];
        }
    }
    for (int k = 0; k < 3; k++) {
        for (int m = 32; m >= 1; m >>= 1) {
            const unsigned long long a = __shfl_xor(lo[k], m, 64), c = __shfl_xor(hi[k], m, 64);
            lo[k] = a < lo[k] ? a : lo[k]; hi[k] = c > hi[k] ? c : hi[k];
        }
        if ((threadIdx.x & 63u) == 0u) { atomicMin(&bounds[k], lo[k]); atomicMax(&bounds[3 + k], hi[k]); }
    }
}

__global__ void __launch_bounds__(kRebuildBlock) k_rebuild_codes(const RefitBox *boxes, int n, const unsigned long long *bounds, uint64_t *codes, int32_t *vals) {
    double cmin[3], cmax[3];
    for (int k = 0; k < 3; k++) { cmin[k] = rebuild_unkey(bounds[k]); cmax[k] = rebuild_unkey(bounds[3 + k]); }
    for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < n; i += (int)(gridDim.x * blockDim.x)) {
        codes[i] = rebuild_code(boxes[i], cmin, cmax);
        vals[i] = i;
    }
}

// parent[c]: of node c; parent[n - 1 + pos]: of the single sorted position pos; -1: the root
__global__ void __launch_bounds__(kRebuildBlock) k_rebuild_hierarchy(const uint64_t *codes, int n, RebuildNode *nodes, int32_t *parent) {
    for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < n - 1; i += (int)(gridDim.x * blockDim.x)) {
        RebuildNode nd;
        rebuild_node(codes, n, i, nd);
        nodes[i].left = nd.left; nodes[i].right = nd.right; nodes[i].first = nd.first; nodes[i].count = nd.count;
        parent[nd.left < 0 ? n - 1 + ~nd.left : nd.left] = i;
        parent[nd.right < 0 ? n - 1 + ~nd.right : nd.right] = i;
        if (i == 0) parent[0] = -1;
    }
}

// arrived[]: zero before the launch.  A lane publishes the box it wrote with an agent-scope fence before it counts itself in at the parent;
// the lane that finds the other child already counted fences again before it reads that child's box.
__global__ void __launch_bounds__(kRebuildBlock) k_rebuild_fit(RebuildNode *nodes, const RefitBox *boxes, const int32_t *order, const int32_t *parent, unsigned int *arrived, int n) {
    for (int pos = (int)(blockIdx.x * blockDim.x + threadIdx.x); pos < n; pos += (int)(gridDim.x * blockDim.x)) {
        int child = ~pos, p = parent[n - 1 + pos];
        RefitBox mine = boxes[order[pos]];
        for (int level = 0; p >= 0 && level < 128; level++) {   // (a radix tree over 96-bit keys is at most 96 deep)
            __threadfence();
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (atomicAdd(&arrived[p], 1u) == 0u) break;
            __threadfence();
            RebuildNode nd;
            nd.left = nodes[p].left; nd.right = nodes[p].right; nd.first = nodes[p].first; nd.count = nodes[p].count;
            const bool from_left = nd.left == child;
            RefitBox other;
            rebuild_child_box(nodes, boxes, order, from_left ? nd.right : nd.left, other);
            rebuild_node_box(nd, boxes, order, from_left ? mine : other, from_left ? other : mine);
            nodes[p].box = nd.box;
            mine = nd.box; child = p; p = parent[p];
        }
    }
}

int rebuild_grid(int n) { return std::max(1, std::min((n + kRebuildBlock - 1) / kRebuildBlock, 2048)); }

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

size_t sort_temp_bytes(int n, hipStream_t s) {
    size_t bytes = 0;
    if (n > 0 && rocprim::radix_sort_pairs(nullptr, bytes, (uint64_t *)nullptr, (uint64_t *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr, (unsigned int)n, 0, 63, s) != hipSuccess)
        throw LjError(LJ_ERR_DEVICE, "rocprim::radix_sort_pairs: size query failed");
    return bytes;
}

} // namespace

RebuildWork rebuild_carve(void *ws, int n, hipStream_t s) {
    RebuildWork w{};
    const size_t m = (size_t)std::max(n, 1);
    size_t at = 0;
    auto take = [&](size_t bytes) { void *p = ws ? (char *)ws + at : nullptr; at += align256(bytes); return p; };
    w.boxes = take(m * sizeof(RefitBox));
    w.bounds = take(6 * 8);
    w.codes = take(m * 8); w.codes_sorted = take(m * 8);
    w.vals = (int32_t *)take(m * 4); w.order = (int32_t *)take(m * 4);
    w.nodes = take(m * sizeof(RebuildNode));
    w.parent = (int32_t *)take(2 * m * 4);
    w.arrived = take(m * 4);
    w.sort_temp_bytes = sort_temp_bytes(n, s);
    w.sort_temp = take(w.sort_temp_bytes);
    w.bytes = at;
    return w;
}
size_t rebuild_node_bytes() { return sizeof(RebuildNode); }

void launch_rebuild_prim_boxes(const DPrim *leaf_prims, int n_leaf_prims, const DSphere *spheres, const RebuildWork &w, int n, hipStream_t s) {
    if (n_leaf_prims <= 0) return;
    hipLaunchKernelGGL(k_rebuild_prim_boxes, dim3(rebuild_grid(n_leaf_prims)), dim3(kRebuildBlock), 0, s, leaf_prims, n_leaf_prims, spheres, (RefitBox *)w.boxes, n);
}

// From w.boxes[0 .. n): the sorted codes in w.codes_sorted and w.order (sorted position -> primitive); ploc.hip starts from these too
void launch_rebuild_order(const RebuildWork &w, int n, hipStream_t s) {
    if (n <= 0) return;
    const RefitBox *boxes = (const RefitBox *)w.boxes;
    unsigned long long *bounds = (unsigned long long *)w.bounds;
    HIP_CHECK(hipMemsetAsync(bounds, 0xff, 3 * 8, s));
    HIP_CHECK(hipMemsetAsync(bounds + 3, 0, 3 * 8, s));
    hipLaunchKernelGGL(k_rebuild_bounds, dim3(rebuild_grid(n)), dim3(kRebuildBlock), 0, s, boxes, n, bounds);
    hipLaunchKernelGGL(k_rebuild_codes, dim3(rebuild_grid(n)), dim3(kRebuildBlock), 0, s, boxes, n, bounds, (uint64_t *)w.codes, w.vals);
    size_t temp = w.sort_temp_bytes;
    HIP_CHECK(rocprim::radix_sort_pairs(w.sort_temp, temp, (uint64_t *)w.codes, (uint64_t *)w.codes_sorted, w.vals, w.order, (unsigned int)n, 0, 63, s));
}

// From w.boxes[0 .. n): w.order and, for n >= 2, the n - 1 nodes of the radix tree with their boxes
void launch_rebuild(const RebuildWork &w, int n, hipStream_t s) {
    if (n <= 0) return;
    launch_rebuild_order(w, n, s);
    if (n < 2) return;
    const RefitBox *boxes = (const RefitBox *)w.boxes;
    HIP_CHECK(hipMemsetAsync(w.arrived, 0, (size_t)(n - 1) * 4, s));
    hipLaunchKernelGGL(k_rebuild_hierarchy, dim3(rebuild_grid(n - 1)), dim3(kRebuildBlock), 0, s, (const uint64_t *)w.codes_sorted, n, (RebuildNode *)w.nodes, w.parent);
    hipLaunchKernelGGL(k_rebuild_fit, dim3(rebuild_grid(n)), dim3(kRebuildBlock), 0, s, (RebuildNode *)w.nodes, boxes, w.order, w.parent, (unsigned int *)w.arrived, n);
}

} // namespace ljd
