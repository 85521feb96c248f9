// TEST INFRASTRUCTURE — host build of the filter of lj_denoise (device/ddenoise.h) with g++: a plain loop over the functions the kernels
// call — pack, one denoise_atrous per pixel and iteration from plain memory, unpack.  It depends on no scene source.  Built only by the
// test suite; the product never loads it.
#include "../../lajolla_public_amd/csrc/device/ddenoise.h"
#include <vector>

using namespace ljd;

// the arguments of lj_denoise, buffers as LjFeatureBuffers lays them out (null: absent); returns 0, or -1 for a call lj_denoise refuses
extern "C" int twin_denoise(int n, int w, int h, const float *rgb, const float *variance, const float *albedo, const float *normal, const float *depth,
                            int iterations, unsigned flags, float sigma_c, float sigma_n, float sigma_d, float sigma_a, float *rgb_out, float *variance_out) {
    if (n <= 0 || w <= 0 || h <= 0 || !rgb || !rgb_out || iterations > kDenoiseMaxIterations) return -1;
    if ((flags & 1u) && !albedo) return -1;
    if (variance_out && !variance) return -1;
    const uint32_t has = (variance ? DN_VARIANCE : 0u) | (albedo ? DN_ALBEDO : 0u) | (normal ? DN_NORMAL : 0u) | (depth ? DN_DEPTH : 0u) | ((flags & 1u) ? DN_DEMODULATE : 0u);
    const DenoiseParams P = denoise_params(has, iterations, sigma_c, sigma_n, sigma_d, sigma_a);
    const size_t image = (size_t)w * (size_t)h, total = image * (size_t)n;
    std::vector<DnGuide> guide(total);
    std::vector<DnDyn> dyn[2] = {std::vector<DnDyn>(total), std::vector<DnDyn>(total)};
    for (size_t e = 0; e < total; e++) denoise_pack(has, e, rgb, variance, albedo, normal, depth, guide[e], dyn[0][e]);
    for (int i = 0; i < P.iterations; i++) {
        const std::vector<DnDyn> &src = dyn[i & 1];
        std::vector<DnDyn> &dst = dyn[(i + 1) & 1];
        for (int img = 0; img < n; img++) {
            const DenoisePlain plain{guide.data() + img * image, src.data() + img * image, w};
            for (int y = 0; y < h; y++)
                for (int x = 0; x < w; x++) dst[img * image + (size_t)y * w + x] = denoise_atrous(P, plain, x, y, w, h, 1 << i);
        }
    }
    const std::vector<DnDyn> &last = dyn[P.iterations & 1];
    for (size_t e = 0; e < total; e++) {
        float c[3], v[3];
        denoise_unpack(has, guide[e], last[e], c, v);
        for (int k = 0; k < 3; k++) { rgb_out[3 * e + k] = c[k]; if (variance_out) variance_out[3 * e + k] = v[k]; }
    }
    return 0;
}
