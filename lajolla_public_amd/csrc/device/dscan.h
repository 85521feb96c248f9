// Leaf-box arithmetic of a tiny scene's flat leaf scan (mega.hip) and the host-side conversion that fills its table (flatten.cpp).
//
// Everything here is plain float arithmetic that g++ compiles as well as hipcc: the kernel's reciprocal (v_rcp_f32) and the shift of the
// result's sign into a candidate mask (v_alignbit) stay in mega.hip, so that the host twin (tests/twin_scan) checks the very expressions
// the kernel runs, with reciprocals of its own choosing.
#pragma once
#include "dtypes.h"
#include <math.h>

namespace ljd {

// A ray as the scan sees it: per axis i = 1 / d (d moved away from zero to 1e-18, see below) and o * i, each rounded once.
struct ScanRay { float ix, iy, iz, ox, oy, oz; };

// A direction component closer to zero than 1e-18 is moved there: the slab then spans |t| < 1e18 * (distance to the plane) instead of
// producing inf - inf.  The traced ray then drifts 1e-18 t off the true one: it can only mis-decide a slab whose plane lies that close to
// the ray, and the table's boxes are grown beyond that (kScanDrift below, on top of the builder's padding).
LJ_HD float scan_clamp_dir(float d) { const float tiny = 1e-18f; return fabsf(d) < tiny ? copysignf(tiny, d) : d; }

// One box (b = centre c[3] | half-extent h[3]) against one ray; FAR: the segment has a far end (shadow rays; extension rays run to
// infinity).  Per axis
//     m = fma(c, i, -o i)      near = fma(-h, |i|, m)      far = fma(h, |i|, m)
// c and h are wave-uniform (scalar registers), negation and |.| are source modifiers: three instructions per axis and no ordering of a
// plane pair by the lane's direction sign — h |i| is never negative, so near <= far whatever the sign of i.  Returns te - 1.0000005 tx in
// one rounding: NEGATIVE (sign bit set) when the segment overlaps the box.  The scan shifts that sign bit into the ray's candidate mask
// with one v_alignbit — no compare, no select.  (Against `te <= round(tx * 1.0000005)` the decision can differ only for |te - tx c| below
// one rounding, i.e. for boxes the exact ray touches in a single point behind its own 4-ulp allowance; which boxes are entered never
// changes a hit — the closest hit is the (t, primitive) minimum over every box that holds it — it only has to stay conservative.)
// `tnear` must be a canonical number (the callers pass max(tnear, 0)), so that the maximum below compiles without a quieting copy.
//
// Error, with u = 2^-24 and T(p) = (p - o) i the exact distance to plane p for the kernel's own i.  The BVH node step computes a plane as
// fl(p i - fl(o i)): off T(p) by at most u (|o i| + |T(p)|).  Here near = fl(fl(c i - fl(o i)) - h |i|) is off T(c - h) by at most
// u (|o i| + |T(c)| + |T(c - h)|): ONE more rounding, that of m, worth u |T(c)| <= u (|T(c - h)| + h |i|), i.e. u (|c - h - o| + h) in
// space.  (m is common to near and far, which therefore never cross: far - near >= 2 h |i| (1 - u) - u |m|.)  The builder's padding does NOT
// cover that: it is 1e-5 (|lo| + |hi|) of the PRIMITIVE whose box defines a face, while h is the half-extent of the whole leaf, the union
// of up to eight such boxes — a small primitive near coordinate zero in a leaf with a large one has a pad far below u h.  The table record
// absorbs it instead: scan_leaf_from_box grows h by kScanGrow (|c| + h) = 64 u (|c| + h) beyond the builder's box, which outweighs the
// rounding of m for every origin within 63 (|c| + h) of the face (u (|p - o| + h) <= 64 u (|c| + h)): there the test is at least as
// conservative on the builder's box as the plane form.  For origins further out — more than 60 times the box's own coordinates away — m
// costs one relative rounding of the distance more than the plane form, beside the two it has and the 4 ulp the exit is widened by.
// The growth is a third of the builder's own pad for a single primitive's box and costs no instruction.
template <bool FAR>
LJ_HD float scan_box(const float (&b)[6], const ScanRay &r, float tnear, float tfar) {
    const float mx = __builtin_fmaf(b[0], r.ix, -r.ox), my = __builtin_fmaf(b[1], r.iy, -r.oy), mz = __builtin_fmaf(b[2], r.iz, -r.oz);
    const float ax = fabsf(r.ix), ay = fabsf(r.iy), az = fabsf(r.iz);
    const float nx = __builtin_fmaf(-b[3], ax, mx), ny = __builtin_fmaf(-b[4], ay, my), nz = __builtin_fmaf(-b[5], az, mz);
    const float fx = __builtin_fmaf(b[3], ax, mx), fy = __builtin_fmaf(b[4], ay, my), fz = __builtin_fmaf(b[5], az, mz);
    const float te = fmaxf(fmaxf(fmaxf(nx, ny), nz), tnear);
    float tx = fminf(fminf(fx, fy), fz);
    if (FAR) tx = fminf(tx, tfar);
    return __builtin_fmaf(tx, -1.0000005f, te);
}

// The table's record of the box [lo, hi] (the builder's padded float box): flatten.cpp on the host, and the refit of an updated scene
// (drefit.h) on the device — contraction off, so that the two agree bit for bit.  c = the float nearest the midpoint, h = the smallest
// float >= max(hi - c, c - lo) + kScanGrow (|c| + that) + kScanDrift, taken in double: [c - h, c + h] contains [lo, hi] with room for the
// rounding of m (above) and for the 1e-18 clamp: a direction component of zero is traced as 1e-18, which drifts 1e-18 t off the true ray;
// kScanDrift covers segments up to 1e6 long where the builder's pad does not (a flat box at coordinate zero is padded by 1e-30 only).
// (A difference of two floats is exact in double unless their exponents lie more than 29 apart; scan_sub_up then returns the next double
// above, found from the rounding error.)
constexpr double kScanGrow = 64.0 / 16777216.0, kScanDrift = 1e-12;
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
LJ_HD double scan_sub_up(double a, double b) {
    const double s = a - b, a1 = s + b, b1 = a1 - s, err = (a - a1) + (b1 - b);   // (TwoSum of a and -b: a - b = s + err exactly)
    return err > 0.0 ? nextafter(s, (double)INFINITY) : s;
}
LJ_HD void scan_leaf_from_box(const float lo[3], const float hi[3], float c[3], float h[3]) {
    for (int k = 0; k < 3; k++) {
        const double l = lo[k], u = hi[k];
        c[k] = (float)(0.5 * (l + u));
        const double need = fmax(scan_sub_up(u, (double)c[k]), scan_sub_up((double)c[k], l));
        const double grown = need + kScanGrow * (fabs((double)c[k]) + need) + kScanDrift;
        float hk = (float)grown;
        if ((double)hk < grown) hk = nextafterf(hk, INFINITY);
        h[k] = hk;
    }
}
#if defined(__clang__)
#pragma clang fp contract(fast)
#endif

} // namespace ljd
