// Edge-stopping a-trous filter over the guide buffers (lj_denoise): the rule, for the device kernels (denoise.hip:
// k_denoise_pack, k_atrous, k_denoise_unpack) and for the host twin (tests/twin_denoise) — they share every line but the memory a tap
// is read from.
//
// Plain C++ with floating-point contraction off, built from + - * / and comparisons only (no exp, pow, sqrt; minima and maxima written
// as comparisons; the division of this build is correctly rounded, see build.py), so that the device and g++ agree bit for bit.
//
// THE RULE.  Inputs per image, all float and row-major as LjFeatureBuffers: rgb[3] (required); variance[3], albedo[3], normal[3] and
// depth (optional); alpha is not read.  A batch is n images of h x w; a tap never leaves its own image.  INPUTS MUST BE FINITE: the
// library does not scan them, and a NaN or an infinity spreads over the reach of the filter.
//   Working signal: c = rgb, v = variance (0 when there is none).  With LJ_DENOISE_DEMODULATE (needs albedo), per channel:
//     e = albedo + 1e-3f,  c = rgb / e,  v = variance / (e * e);  after the last iteration c is multiplied by e and v by e * e.
//   Iteration i = 0 .. iterations - 1 has step s = 1 << i.  The taps of pixel p are q = p + s * (dx, dy), dy outer and dx inner, both
//   from -2 to 2 in increasing order; taps outside the image are skipped.  k = hk[dx + 2] * hk[dy + 2], hk = {1/16, 1/4, 3/8, 1/4, 1/16}.
//   w = k * f(xn) * f(xd) * f(xa) * f(xc), multiplied from left to right, f(x) = max(0, 1 - x)^2; a term whose buffer is absent is left out:
//     xn = |n_p - n_q|^2 / sigma_n^2           |a - b|^2 = (dx*dx + dy*dy) + dz*dz of the float differences
//     xd = (d_p - d_q)^2 / (sigma_d^2 * m^2)   m = max(d_p, d_q); xd = 0 when m == 0 (two misses).  With sigma_d < 1 a hit beside a miss has w = 0
//     xa = |a_p - a_q|^2 / sigma_a^2
//     xc = |c_p - c_q|^2 / (sigma_c^2 * g_p + 1e-12f)     only with a variance buffer
//   g_p: the 3 x 3 binomial average of (v.x + v.y) + v.z over p and its eight direct neighbours (offset 1 at every step) in the current
//   iteration's input: weights 1/4, 1/8, 1/16, summed dy outer, dx inner, and divided by the sum of the in-image weights (SVGF's prefilter).
//   Output of an iteration, float sums in tap order:  c'_p = sum w c_q / sum w,   v'_p = sum (w * w) v_q / ((sum w) * (sum w)).
//   The centre tap has w = 9/64, so sum w > 0.  The average is evaluated about the centre, c'_p = c_p + (sum w (c_q - c_p)) / sum w: the
//   same number in exact arithmetic, and a constant image comes back bit for bit (the plain quotient of two 25-term float sums was measured
//   at up to 5 ulp off a constant after one iteration: its two sums round differently).
// Defaults: iterations 5, sigma_c 4, sigma_n 0.5, sigma_d 0.1, sigma_a 0.25 (not retuned since they were set: a retune goes
// here with the measurement of tools/denoise_cost.py beside it).
#pragma once
#include "dtypes.h"
#include <stddef.h>
#include <stdint.h>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace ljd {

enum : uint32_t { DN_VARIANCE = 1u, DN_ALBEDO = 2u, DN_NORMAL = 4u, DN_DEPTH = 8u, DN_DEMODULATE = 16u };
constexpr int kDenoiseMaxIterations = 8;
constexpr int kDenoiseTile = 16;   // the kernels' tile: 16 x 16 pixels per workgroup

struct alignas(16) DnQuad { float x, y, z, w; };
// the two 32-byte records of a pixel, each two 16-byte quads: what never changes, and what an iteration reads and the next one writes
struct DnGuide { DnQuad q0, q1; };   // q0 = normal.xyz, depth;  q1 = albedo.xyz, pad
struct DnDyn { DnQuad q0, q1; };     // q0 = c.xyz, v.x;  q1 = v.y, v.z, pad, pad

struct DenoiseParams { uint32_t has; int32_t iterations; float sc2, sn2, sd2, sa2; };   // has: DN_* bits; the squared sigmas

// the arguments of a call with the defaults filled in (<= 0: the default); `has`: which buffers the caller gave, and the demodulate flag
LJ_HD DenoiseParams denoise_params(uint32_t has, int32_t iterations, float sigma_c, float sigma_n, float sigma_d, float sigma_a) {
    DenoiseParams P;
    P.has = has;
    P.iterations = iterations > 0 ? iterations : 5;
    const float sc = sigma_c > 0.0f ? sigma_c : 4.0f, sn = sigma_n > 0.0f ? sigma_n : 0.5f, sd = sigma_d > 0.0f ? sigma_d : 0.1f, sa = sigma_a > 0.0f ? sigma_a : 0.25f;
    P.sc2 = sc * sc; P.sn2 = sn * sn; P.sd2 = sd * sd; P.sa2 = sa * sa;
    return P;
}

LJ_HD float denoise_hk(int i) { return i == 2 ? 0.375f : ((i == 1 || i == 3) ? 0.25f : 0.0625f); }   // {1/16, 1/4, 3/8, 1/4, 1/16}
LJ_HD float denoise_stop(float x) { float t = 1.0f - x; t = t < 0.0f ? 0.0f : t; return t * t; }   // f(x) = max(0, 1 - x)^2
LJ_HD float denoise_dist2(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return (dx * dx + dy * dy) + dz * dz;
}

// ---- pack: the records of pixel e from the caller's buffers (absent buffers: null; their fields are 0)
LJ_HD void denoise_pack(uint32_t has, uint64_t e, const float *rgb, const float *variance, const float *albedo, const float *normal, const float *depth, DnGuide &g, DnDyn &d) {
    g.q0.x = g.q0.y = g.q0.z = g.q0.w = 0.0f; g.q1.x = g.q1.y = g.q1.z = g.q1.w = 0.0f;
    if (has & DN_NORMAL) { g.q0.x = normal[3 * e]; g.q0.y = normal[3 * e + 1]; g.q0.z = normal[3 * e + 2]; }
    if (has & DN_DEPTH) g.q0.w = depth[e];
    if (has & DN_ALBEDO) { g.q1.x = albedo[3 * e]; g.q1.y = albedo[3 * e + 1]; g.q1.z = albedo[3 * e + 2]; }
    float c[3], v[3];
    for (int k = 0; k < 3; k++) { c[k] = rgb[3 * e + k]; v[k] = (has & DN_VARIANCE) ? variance[3 * e + k] : 0.0f; }
    if (has & DN_DEMODULATE) {
        const float a[3] = {g.q1.x, g.q1.y, g.q1.z};
        for (int k = 0; k < 3; k++) { const float den = a[k] + 1e-3f; c[k] = c[k] / den; v[k] = v[k] / (den * den); }
    }
    d.q0.x = c[0]; d.q0.y = c[1]; d.q0.z = c[2]; d.q0.w = v[0];
    d.q1.x = v[1]; d.q1.y = v[2]; d.q1.z = 0.0f; d.q1.w = 0.0f;
}
// ---- unpack: the outputs of a pixel from its records after the last iteration
LJ_HD void denoise_unpack(uint32_t has, const DnGuide &g, const DnDyn &d, float rgb[3], float variance[3]) {
    rgb[0] = d.q0.x; rgb[1] = d.q0.y; rgb[2] = d.q0.z;
    variance[0] = d.q0.w; variance[1] = d.q1.x; variance[2] = d.q1.y;
    if (has & DN_DEMODULATE) {
        const float a[3] = {g.q1.x, g.q1.y, g.q1.z};
        for (int k = 0; k < 3; k++) { const float den = a[k] + 1e-3f; rgb[k] = rgb[k] * den; variance[k] = variance[k] * (den * den); }
    }
}

// Src provides, for a pixel (x, y) INSIDE the image:   void load(int x, int y, DnGuide &g, DnDyn &d) const;   DnDyn dyn(int x, int y) const;

// g_p: the 3 x 3 binomial average of the summed variance around (x, y), renormalised by the in-image weights
template <class Src>
LJ_HD float denoise_prefilter(const Src &src, int x, int y, int w, int h) {
    float sum = 0.0f, wsum = 0.0f;
    for (int dy = -1; dy <= 1; dy++) {
        const int qy = y + dy;
        if (qy < 0 || qy >= h) continue;
        for (int dx = -1; dx <= 1; dx++) {
            const int qx = x + dx;
            if (qx < 0 || qx >= w) continue;
            const float k = (dx == 0 ? 0.5f : 0.25f) * (dy == 0 ? 0.5f : 0.25f);
            const DnDyn d = src.dyn(qx, qy);
            sum += k * ((d.q0.w + d.q1.x) + d.q1.y);
            wsum += k;
        }
    }
    return sum / wsum;
}

// one iteration at one pixel: step s, image w x h
template <class Src>
LJ_HD DnDyn denoise_atrous(const DenoiseParams &P, const Src &src, int x, int y, int w, int h, int s) {
    DnGuide gp; DnDyn dp;
    src.load(x, y, gp, dp);
    float cden = 0.0f;
    if (P.has & DN_VARIANCE) cden = P.sc2 * denoise_prefilter(src, x, y, w, h) + 1e-12f;
    float sw = 0.0f, sc[3] = {0.0f, 0.0f, 0.0f}, sv[3] = {0.0f, 0.0f, 0.0f};
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + s * dy;
        if (qy < 0 || qy >= h) continue;
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + s * dx;
            if (qx < 0 || qx >= w) continue;
            DnGuide gq; DnDyn dq;
            src.load(qx, qy, gq, dq);
            float wt = denoise_hk(dx + 2) * denoise_hk(dy + 2);
            if (P.has & DN_NORMAL) wt = wt * denoise_stop(denoise_dist2(gp.q0.x, gp.q0.y, gp.q0.z, gq.q0.x, gq.q0.y, gq.q0.z) / P.sn2);
            if (P.has & DN_DEPTH) {
                const float m = gp.q0.w < gq.q0.w ? gq.q0.w : gp.q0.w, dd = gp.q0.w - gq.q0.w;
                const float xd = m == 0.0f ? 0.0f : (dd * dd) / (P.sd2 * (m * m));
                wt = wt * denoise_stop(xd);
            }
            if (P.has & DN_ALBEDO) wt = wt * denoise_stop(denoise_dist2(gp.q1.x, gp.q1.y, gp.q1.z, gq.q1.x, gq.q1.y, gq.q1.z) / P.sa2);
            if (P.has & DN_VARIANCE) wt = wt * denoise_stop(denoise_dist2(dp.q0.x, dp.q0.y, dp.q0.z, dq.q0.x, dq.q0.y, dq.q0.z) / cden);
            const float w2 = wt * wt;
            sw += wt;
            sc[0] += wt * (dq.q0.x - dp.q0.x); sc[1] += wt * (dq.q0.y - dp.q0.y); sc[2] += wt * (dq.q0.z - dp.q0.z);
            sv[0] += w2 * dq.q0.w; sv[1] += w2 * dq.q1.x; sv[2] += w2 * dq.q1.y;
        }
    }
    const float sw2 = sw * sw;
    DnDyn o;
    o.q0.x = dp.q0.x + sc[0] / sw; o.q0.y = dp.q0.y + sc[1] / sw; o.q0.z = dp.q0.z + sc[2] / sw; o.q0.w = sv[0] / sw2;
    o.q1.x = sv[1] / sw2; o.q1.y = sv[2] / sw2; o.q1.z = 0.0f; o.q1.w = 0.0f;
    return o;
}

// the records of one image in plain memory: what the direct route of k_atrous and the host twin read
struct DenoisePlain {
    const DnGuide *guide; const DnDyn *dynamic; int w;
    LJ_HD void load(int x, int y, DnGuide &g, DnDyn &d) const { const size_t i = (size_t)y * (size_t)w + (size_t)x; g = guide[i]; d = dynamic[i]; }
    LJ_HD DnDyn dyn(int x, int y) const { return dynamic[(size_t)y * (size_t)w + (size_t)x]; }
};

} // namespace ljd
