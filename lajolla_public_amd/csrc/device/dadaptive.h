// Variance-driven sampling in rounds (lj_render_adaptive): the rule, for the device kernels (adaptive.hip: k_adaptive_merge,
// k_adaptive_select and its scan and scatter, k_adaptive_output) and for the host twin (tests/twin_adaptive) — they share every line but the
// compaction, which the kernels do with ballots and prefix sums and the twin with a loop: the same list either way.
//
// Plain C++ with floating-point contraction off, built from + - * / and comparisons and integer operations only (the division of this
// build is correctly rounded, see build.py), float32 in the order written here, so that the device and g++ agree bit for bit.
//
// THE RULE.  State per pixel of the film: n (uint32, samples so far), mean[3], m2[3] (float; m2: the sum of squared deviations from the mean).
// All zero for a pixel outside the call's share or crop window.  pairs(k) = float(k (k - 1)), the product taken in 64-bit integers.
//   Round 0 renders the call's whole pixel list (make_plan's, in its order) with k_0 = min_spp samples and seed_0 = the call's resolved seed:
//     mean = rgb_0,  m2 = variance_0 * pairs(k_0),  n = k_0          rgb_0, variance_0: what lj_render_features writes for that spp and seed
//   Round r >= 1 renders the selected list with k_r = round_spp samples and seed_r = seed_0 + r * 0x9e3779b97f4a7c15 (wrapping; 0 becomes 1,
//   since 0 asks make_plan for the default seed).  The pcg32 streams stay pixel * k_r + s of seed_r, so round r yields at pixel p, bit for
//   bit, what lj_render_features(spp = k_r, seed = seed_r) yields there.
//   Merge of a round's (b = rgb_r, v = variance_r, k) into (n, mean, m2), per channel, in this order:
//     n' = n + k;   d = b - mean;   f = float(k) / float(n');   mean' = mean + d * f;   m2_b = v * pairs(k);
//     m2' = (m2 + m2_b) + (d * d) * (float(n) * f)
//   Error of a pixel with n > 0:
//     V = ((m2[0] + m2[1]) + m2[2]) / pairs(n), 0 when n < 2;      S = ((mean[0] + mean[1]) + mean[2]) * (1/3)   (the float 1.0f / 3.0f)
//     g = the maximum of V over the pixel and its in-film 3 x 3 neighbours that have n > 0 (a low-sample pixel that happened to see no
//         variance must not escape refinement while its neighbours are noisy);      e2 = g / (S * S + 1e-4f)
//   A pixel is selected for the next round iff n > 0, e2 > target_error * target_error (the float product) and n + round_spp <= max_spp.
//   The selected list keeps the relative order of the call's list (tile-major, as make_plan enumerates it).  Rounds end when the list is
//   empty or max_rounds renders have run.
//   Outputs: rgb = mean;  variance[c] = m2[c] / pairs(n), 0 where n < 2;  samples = n.
// Defaults (<= 0): min_spp 16, max_spp 16 * min_spp, round_spp min_spp, max_rounds 16, target_error 0.05.
//
// Results are bit-identical from call to call, for any pass size, pool size and kernel plan: the compaction is ordered (no atomics) and a
// merge touches each listed pixel exactly once.  NOT promised past round 0: invariance under crop or share — a pixel at the border of a
// share has other neighbours with n > 0 than the same pixel of the full frame, so it may be selected in one and not in the other.
#pragma once
#include "dtypes.h"
#include <stddef.h>
#include <stdint.h>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace ljd {

constexpr int kAdaptiveMaxRounds = 64;
constexpr uint32_t kAdaptiveMaxSpp = 1u << 20;
constexpr uint64_t kAdaptiveSeedStep = 0x9e3779b97f4a7c15ull;

struct AdaptiveParams { uint32_t min_spp, max_spp, round_spp, max_rounds; float target_error; };

// The arguments of a call with the defaults filled in.  0: fine; else what lj_render_adaptive refuses — 1: min_spp == 1, 2: max_spp < min_spp,
// 3: an spp above 2^20, 4: more than 64 rounds, 5: a target_error that is negative or not finite.
LJ_HD int adaptive_params(int32_t min_spp, int32_t max_spp, int32_t round_spp, int32_t max_rounds, float target_error, AdaptiveParams &P) {
    if (min_spp == 1) return 1;
    if (!(target_error >= 0.0f) || !(target_error <= 3.402823466e38f)) return 5;
    if (max_rounds > kAdaptiveMaxRounds) return 4;
    if (min_spp > (int32_t)kAdaptiveMaxSpp || max_spp > (int32_t)kAdaptiveMaxSpp || round_spp > (int32_t)kAdaptiveMaxSpp) return 3;
    P.min_spp = min_spp > 0 ? (uint32_t)min_spp : 16u;
    const uint32_t dflt_max = 16u * P.min_spp < kAdaptiveMaxSpp ? 16u * P.min_spp : kAdaptiveMaxSpp;
    P.max_spp = max_spp > 0 ? (uint32_t)max_spp : dflt_max;
    if (P.max_spp < P.min_spp) return 2;
    P.round_spp = round_spp > 0 ? (uint32_t)round_spp : P.min_spp;
    P.max_rounds = max_rounds > 0 ? (uint32_t)max_rounds : 16u;
    P.target_error = target_error > 0.0f ? target_error : 0.05f;
    return 0;
}

// the seed of round r (never 0)
LJ_HD uint64_t adaptive_round_seed(uint64_t seed0, uint32_t r) {
    const uint64_t s = seed0 + (uint64_t)r * kAdaptiveSeedStep;
    return s ? s : 1ull;
}

LJ_HD float adaptive_pairs(uint32_t k) { return (float)((uint64_t)k * (uint64_t)(k - 1u)); }   // (k >= 1)

// round 0 at one pixel
LJ_HD void adaptive_init(uint32_t &n, float mean[3], float m2[3], const float b[3], const float v[3], uint32_t k) {
    const float pairs = adaptive_pairs(k);
    for (int c = 0; c < 3; c++) { mean[c] = b[c]; m2[c] = v[c] * pairs; }
    n = k;
}
// a later round at one pixel
LJ_HD void adaptive_merge(uint32_t &n, float mean[3], float m2[3], const float b[3], const float v[3], uint32_t k) {
    const uint32_t n1 = n + k;
    const float f = (float)k / (float)n1;
    const float pairs = adaptive_pairs(k), nf = (float)n * f;
    for (int c = 0; c < 3; c++) {
        const float d = b[c] - mean[c];
        mean[c] = mean[c] + d * f;
        const float m2b = v[c] * pairs;
        m2[c] = (m2[c] + m2b) + (d * d) * nf;
    }
    n = n1;
}
// the merge of a round at entry i of its list: the round's frames are read, and the state written, at the listed pixel alone
LJ_HD void adaptive_merge_entry(const uint32_t *list, uint64_t i, uint32_t k, bool init, const float *rgb, const float *variance, uint32_t *n, float *mean, float *m2) {
    const uint64_t p = list[i];
    float b[3], v[3], mn[3], q[3];
    for (int c = 0; c < 3; c++) { b[c] = rgb[3 * p + c]; v[c] = variance[3 * p + c]; mn[c] = mean[3 * p + c]; q[c] = m2[3 * p + c]; }
    uint32_t cnt = n[p];
    if (init) adaptive_init(cnt, mn, q, b, v, k); else adaptive_merge(cnt, mn, q, b, v, k);
    for (int c = 0; c < 3; c++) { mean[3 * p + c] = mn[c]; m2[3 * p + c] = q[c]; }
    n[p] = cnt;
}

LJ_HD float adaptive_v(uint32_t n, const float *m2) { return n < 2u ? 0.0f : ((m2[0] + m2[1]) + m2[2]) / adaptive_pairs(n); }

// e2 of pixel (x, y) of a w x h film (n > 0 there)
LJ_HD float adaptive_error(int x, int y, int w, int h, const uint32_t *n, const float *mean, const float *m2) {
    const uint64_t p = (uint64_t)y * (uint64_t)w + (uint64_t)x;
    float g = adaptive_v(n[p], m2 + 3 * p);
    for (int dy = -1; dy <= 1; dy++) {
        const int qy = y + dy;
        if (qy < 0 || qy >= h) continue;
        for (int dx = -1; dx <= 1; dx++) {
            const int qx = x + dx;
            if (qx < 0 || qx >= w || (dx == 0 && dy == 0)) continue;
            const uint64_t q = (uint64_t)qy * (uint64_t)w + (uint64_t)qx;
            const uint32_t nq = n[q];
            if (nq == 0u) continue;
            const float v = adaptive_v(nq, m2 + 3 * q);
            if (v > g) g = v;
        }
    }
    const float S = ((mean[3 * p] + mean[3 * p + 1]) + mean[3 * p + 2]) * (1.0f / 3.0f);
    return g / (S * S + 1e-4f);
}

// is film pixel p selected for the next round?
LJ_HD bool adaptive_selected(const AdaptiveParams &P, uint32_t p, int w, int h, const uint32_t *n, const float *mean, const float *m2) {
    const uint32_t np = n[p];
    if (np == 0u || (uint64_t)np + (uint64_t)P.round_spp > (uint64_t)P.max_spp) return false;
    const int y = (int)(p / (uint32_t)w), x = (int)(p - (uint32_t)y * (uint32_t)w);
    return adaptive_error(x, y, w, h, n, mean, m2) > P.target_error * P.target_error;
}

// the outputs of film pixel p (a null buffer is not wanted)
LJ_HD void adaptive_output(uint64_t p, const uint32_t *n, const float *mean, const float *m2, float *rgb, float *variance, uint32_t *samples) {
    const uint32_t np = n[p];
    if (rgb) for (int c = 0; c < 3; c++) rgb[3 * p + c] = mean[3 * p + c];
    if (variance) for (int c = 0; c < 3; c++) variance[3 * p + c] = np < 2u ? 0.0f : m2[3 * p + c] / adaptive_pairs(np);
    if (samples) samples[p] = np;
}

} // namespace ljd
