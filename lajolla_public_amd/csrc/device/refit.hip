// Refit kernels of lj_scene_update_geometry: the boxes of the BVH4, the BVH8 and a tiny scene's leaf table recomputed on the
// device from the re-uploaded leaf-ordered primitives.  One lane per node (or leaf record), one launch per tree level, deepest level first:
// a node reads the boxes its children's launch wrote.  Every launch is a bounded grid-stride pass over a host-built list of node indices —
// no atomics, no cross-lane operations, no persistent loop.  The arithmetic is device/drefit.h, which the host twin runs too.
#include "api_internal.h"
#include "drefit.h"

namespace ljd {

namespace {

constexpr int kRefitBlock = 256;

__global__ void __launch_bounds__(kRefitBlock) k_refit4(DNode4 *nodes, RefitBox *box4, const DPrim *leaf_prims, const DSphere *spheres, const int32_t *list, int n) {
    for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < n; i += (int)(gridDim.x * blockDim.x))
        refit_node4(nodes, box4, leaf_prims, spheres, list[i]);
}

__global__ void __launch_bounds__(kRefitBlock) k_refit8(unsigned char *nodes8, int stride, RefitBox *box8, const DPrim *leaf_prims, const DSphere *spheres, const int32_t *list, int n) {
    for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < n; i += (int)(gridDim.x * blockDim.x))
        refit_node8(nodes8, stride, box8, leaf_prims, spheres, list[i]);
}

__global__ void __launch_bounds__(kRefitBlock) k_refit_scan(DScanLeaf *leaves, const DPrim *leaf_prims, const DSphere *spheres, int n) {
    for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < n; i += (int)(gridDim.x * blockDim.x))
        refit_scan_leaf(leaves, leaf_prims, spheres, i);
}

int refit_grid(int n) { return std::max(1, std::min((n + kRefitBlock - 1) / kRefitBlock, 4096)); }

} // namespace

void launch_refit4(DNode4 *nodes, void *box4, const DPrim *leaf_prims, const DSphere *spheres, const int32_t *list, int n, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_refit4, dim3(refit_grid(n)), dim3(kRefitBlock), 0, s, nodes, (RefitBox *)box4, leaf_prims, spheres, list, n);
}
void launch_refit8(void *nodes8, int stride, void *box8, const DPrim *leaf_prims, const DSphere *spheres, const int32_t *list, int n, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_refit8, dim3(refit_grid(n)), dim3(kRefitBlock), 0, s, (unsigned char *)nodes8, stride, (RefitBox *)box8, leaf_prims, spheres, list, n);
}
void launch_refit_scan(DScanLeaf *leaves, const DPrim *leaf_prims, const DSphere *spheres, int n, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_refit_scan, dim3(refit_grid(n)), dim3(kRefitBlock), 0, s, leaves, leaf_prims, spheres, n);
}
size_t refit_box_bytes() { return sizeof(RefitBox); }

} // namespace ljd
