// gfx950 kernels of lj_denoise: the edge-stopping a-trous filter of ddenoise.h over n images of h x w.
//
//   k_denoise_pack    lane/pixel : the caller's buffers, demodulated, into two 32-byte records per pixel (DnGuide: normal, depth, albedo;
//                                  DnDyn: c, v) — a tap is then two or four 16-byte loads, not fourteen strided ones.
//   k_atrous<LDS>     lane/pixel : one iteration, a workgroup per 16 x 16 tile, DnDyn ping-ponged between two buffers.
//                                  LDS: the tile and a halo of 2 s, staged once as four planes of 16-byte quads, filtered from there.
//                                  Direct: every tap from global memory (the tap set of a tile is L2-resident).
//                                  Both call denoise_atrous with a source of their own: the same arithmetic in the same order.
//   k_denoise_unpack  lane/pixel : remodulates and writes rgb_out and, when asked for, variance_out.
// No atomics, no counters; grids are bounded by the pixel count (bounded grid-stride loops).
#include <hip/hip_runtime.h>
#include <algorithm>
#include "dstage.h"
#include "ddenoise.h"

namespace ljd {

static_assert(kBlock == kDenoiseTile * kDenoiseTile, "one lane per pixel of a tile");
static_assert(sizeof(DnGuide) == 32 && sizeof(DnDyn) == 32, "two 16-byte quads per record");

constexpr uint32_t kDenoiseMaxGrid = 1u << 20;

__global__ void __launch_bounds__(kBlock) k_denoise_pack(uint32_t has, uint64_t total, const float *rgb, const float *variance, const float *albedo, const float *normal, const float *depth,
                                                         DnGuide *guide, DnDyn *dyn) {
    for (uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (uint64_t)gridDim.x * kBlock) {
        DnGuide g; DnDyn d;
        denoise_pack(has, e, rgb, variance, albedo, normal, depth, g, d);
        guide[e] = g; dyn[e] = d;
    }
}

__global__ void __launch_bounds__(kBlock) k_denoise_unpack(uint32_t has, uint64_t total, const DnGuide *guide, const DnDyn *dyn, float *rgb_out, float *variance_out) {
    for (uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (uint64_t)gridDim.x * kBlock) {
        float c[3], v[3];
        denoise_unpack(has, guide[e], dyn[e], c, v);
        rgb_out[3 * e] = c[0]; rgb_out[3 * e + 1] = c[1]; rgb_out[3 * e + 2] = c[2];
        if (variance_out) { variance_out[3 * e] = v[0]; variance_out[3 * e + 1] = v[1]; variance_out[3 * e + 2] = v[2]; }
    }
}

// A haloed tile in LDS: four planes (guide q0, q1; dyn q0, q1) of side * side quads, so that the lanes of a row read consecutive 16-byte
// slots.  Cells outside the image are never written and never read: denoise_atrous asks for in-image pixels only.
struct DenoiseTileSrc {
    const DnQuad *lds; int x0, y0, side;   // (x0, y0): the image pixel of cell (0, 0)
    __device__ __forceinline__ int cell(int x, int y) const { return (y - y0) * side + (x - x0); }
    __device__ __forceinline__ void load(int x, int y, DnGuide &g, DnDyn &d) const {
        const int c = cell(x, y), plane = side * side;
        g.q0 = lds[c]; g.q1 = lds[plane + c]; d.q0 = lds[2 * plane + c]; d.q1 = lds[3 * plane + c];
    }
    __device__ __forceinline__ DnDyn dyn(int x, int y) const {
        const int c = cell(x, y), plane = side * side;
        DnDyn d; d.q0 = lds[2 * plane + c]; d.q1 = lds[3 * plane + c];
        return d;
    }
};

// n_tiles = n * tiles_y * tiles_x tiles, walked by a bounded grid-stride loop (tile index: image-major, then rows of tiles)
template <bool LDS>
__global__ void __launch_bounds__(kBlock) k_atrous(DenoiseParams P, int w, int h, int s, uint32_t tiles_x, uint32_t tiles_y, uint64_t n_tiles, const DnGuide *guide, const DnDyn *dyn_in, DnDyn *dyn_out) {
    extern __shared__ DnQuad lds[];
    const int lx = (int)(threadIdx.x & (kDenoiseTile - 1)), ly = (int)(threadIdx.x / kDenoiseTile);
    const uint64_t per_image = (uint64_t)tiles_x * tiles_y, image_pixels = (uint64_t)w * (uint64_t)h;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t img = tile / per_image;
        const uint32_t t = (uint32_t)(tile - img * per_image);
        const int ox = (int)(t % tiles_x) * kDenoiseTile, oy = (int)(t / tiles_x) * kDenoiseTile;
        const DnGuide *ig = guide + img * image_pixels;
        const DnDyn *id = dyn_in + img * image_pixels;
        const int x = ox + lx, y = oy + ly;
        const bool inside = x < w && y < h;
        DnDyn o;
        if constexpr (LDS) {
            const int halo = 2 * s, side = kDenoiseTile + 2 * halo, plane = side * side;
            __syncthreads();   // the previous tile's readers are done
            for (int c = (int)threadIdx.x; c < plane; c += kBlock) {
                const int qx = ox - halo + c % side, qy = oy - halo + c / side;
                if (qx < 0 || qy < 0 || qx >= w || qy >= h) continue;
                const size_t i = (size_t)qy * (size_t)w + (size_t)qx;
                const DnGuide g = ig[i]; const DnDyn d = id[i];
                lds[c] = g.q0; lds[plane + c] = g.q1; lds[2 * plane + c] = d.q0; lds[3 * plane + c] = d.q1;
            }
            __syncthreads();
            const DenoiseTileSrc src{lds, ox - halo, oy - halo, side};
            if (inside) o = denoise_atrous(P, src, x, y, w, h, s);
        } else {
            const DenoisePlain src{ig, id, w};
            if (inside) o = denoise_atrous(P, src, x, y, w, h, s);
        }
        if (inside) dyn_out[img * image_pixels + (uint64_t)y * (uint64_t)w + (uint64_t)x] = o;
    }
}

// ---------------------------------------------------------------- launchers (called from api_device.hip)
// LDS bytes of the haloed tile of iteration i (step 1 << i): 4 planes x (16 + 4 s)^2 quads
size_t denoise_tile_bytes(int iteration) {
    const size_t side = (size_t)kDenoiseTile + 4u * ((size_t)1 << iteration);
    return 4 * side * side * sizeof(DnQuad);
}
static uint32_t pixel_grid(uint64_t total) { return (uint32_t)std::min<uint64_t>((total + kBlock - 1) / kBlock, kDenoiseMaxGrid); }

void launch_denoise_pack(uint32_t has, uint64_t total, const float *rgb, const float *variance, const float *albedo, const float *normal, const float *depth, void *guide, void *dyn, hipStream_t s) {
    hipLaunchKernelGGL(k_denoise_pack, dim3(pixel_grid(total)), dim3(kBlock), 0, s, has, total, rgb, variance, albedo, normal, depth, (DnGuide *)guide, (DnDyn *)dyn);
}
void launch_denoise_unpack(uint32_t has, uint64_t total, const void *guide, const void *dyn, float *rgb_out, float *variance_out, hipStream_t s) {
    hipLaunchKernelGGL(k_denoise_unpack, dim3(pixel_grid(total)), dim3(kBlock), 0, s, has, total, (const DnGuide *)guide, (const DnDyn *)dyn, rgb_out, variance_out);
}
// what api_internal.h declares of a call (it does not include ddenoise.h)
struct DenoiseCall { uint32_t has; int32_t iterations; float sigma[4]; };
uint32_t denoise_has(bool variance, bool albedo, bool normal, bool depth, bool demodulate) {
    return (variance ? DN_VARIANCE : 0u) | (albedo ? DN_ALBEDO : 0u) | (normal ? DN_NORMAL : 0u) | (depth ? DN_DEPTH : 0u) | (demodulate ? DN_DEMODULATE : 0u);
}
int denoise_max_iterations() { return kDenoiseMaxIterations; }
static DenoiseParams params_of(const DenoiseCall &c) { return denoise_params(c.has, c.iterations, c.sigma[0], c.sigma[1], c.sigma[2], c.sigma[3]); }
int denoise_iterations(const DenoiseCall &c) { return params_of(c).iterations; }
size_t denoise_record_bytes() { return sizeof(DnDyn); }

void launch_atrous(const DenoiseCall &c, int n, int w, int h, int iteration, bool lds, const void *guide, const void *dyn_in, void *dyn_out, hipStream_t s) {
    const DenoiseParams P = params_of(c);
    const uint32_t tiles_x = ((uint32_t)w + kDenoiseTile - 1) / kDenoiseTile, tiles_y = ((uint32_t)h + kDenoiseTile - 1) / kDenoiseTile;
    const uint64_t n_tiles = (uint64_t)n * tiles_x * tiles_y;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(n_tiles, kDenoiseMaxGrid);
    const int step = 1 << iteration;
    if (lds) hipLaunchKernelGGL(k_atrous<true>, dim3(grid), dim3(kBlock), denoise_tile_bytes(iteration), s, P, w, h, step, tiles_x, tiles_y, n_tiles, (const DnGuide *)guide, (const DnDyn *)dyn_in, (DnDyn *)dyn_out);
    else hipLaunchKernelGGL(k_atrous<false>, dim3(grid), dim3(kBlock), 0, s, P, w, h, step, tiles_x, tiles_y, n_tiles, (const DnGuide *)guide, (const DnDyn *)dyn_in, (DnDyn *)dyn_out);
}

} // namespace ljd
