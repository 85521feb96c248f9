// TEST INFRASTRUCTURE — host build of the rule of lj_render_adaptive (device/dadaptive.h) with g++: plain loops over the functions the
// kernels call — the merge of a round over its list, the error of every pixel, select + compact over a list, the outputs.  It depends on
// no scene source.  Built only by the test suite; the product never loads it.
#include "../../lajolla_public_amd/csrc/device/dadaptive.h"

using namespace ljd;

// k_adaptive_merge: a round's frames (film-sized rgb and variance) folded into the state at list[0, n_list); init: round 0
extern "C" void twin_adaptive_merge(const uint32_t *list, int64_t n_list, uint32_t k, int init, const float *rgb, const float *variance, uint32_t *n, float *mean, float *m2) {
    for (int64_t i = 0; i < n_list; i++) adaptive_merge_entry(list, (uint64_t)i, k, init != 0, rgb, variance, n, mean, m2);
}

// e2 of every pixel with n > 0 of a w x h film (0 elsewhere)
extern "C" void twin_adaptive_error(int w, int h, const uint32_t *n, const float *mean, const float *m2, float *e2) {
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const size_t p = (size_t)y * (size_t)w + (size_t)x;
            e2[p] = n[p] ? adaptive_error(x, y, w, h, n, mean, m2) : 0.0f;
        }
}

// select + compact over list[0, n_list): returns the number of entries written to `selected`, or -1 for arguments lj_render_adaptive refuses
extern "C" int64_t twin_adaptive_select(int w, int h, const uint32_t *n, const float *mean, const float *m2, int min_spp, int max_spp, int round_spp, int max_rounds, float target_error,
                                        const uint32_t *list, int64_t n_list, uint32_t *selected) {
    AdaptiveParams P;
    if (adaptive_params(min_spp, max_spp, round_spp, max_rounds, target_error, P) != 0) return -1;
    int64_t out = 0;
    for (int64_t i = 0; i < n_list; i++) if (adaptive_selected(P, list[i], w, h, n, mean, m2)) selected[out++] = list[i];
    return out;
}

// the arguments with the defaults filled in: {min_spp, max_spp, round_spp, max_rounds}; returns adaptive_params' code
extern "C" int twin_adaptive_params(int min_spp, int max_spp, int round_spp, int max_rounds, float target_error, uint32_t out[4], float *target_out) {
    AdaptiveParams P{};
    const int rc = adaptive_params(min_spp, max_spp, round_spp, max_rounds, target_error, P);
    out[0] = P.min_spp; out[1] = P.max_spp; out[2] = P.round_spp; out[3] = P.max_rounds; *target_out = P.target_error;
    return rc;
}

extern "C" uint64_t twin_adaptive_seed(uint64_t seed0, uint32_t round) { return adaptive_round_seed(seed0, round); }

// k_adaptive_output over n_pixels pixels (a null buffer is not wanted)
extern "C" void twin_adaptive_output(int64_t n_pixels, const uint32_t *n, const float *mean, const float *m2, float *rgb, float *variance, uint32_t *samples) {
    for (int64_t p = 0; p < n_pixels; p++) adaptive_output((uint64_t)p, n, mean, m2, rgb, variance, samples);
}
