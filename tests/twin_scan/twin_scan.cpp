// TEST INFRASTRUCTURE — host build of the leaf scan's box arithmetic (device/dscan.h) with g++: the table conversion flatten.cpp runs
// (padded lo / hi -> centre / half-extent) and scan_box exactly as k_mega evaluates it, except for the two device-only pieces: the
// reciprocal (v_rcp_f32 there; here the correctly rounded quotient moved by a caller-chosen number of ulps) and the shift of the sign
// into the candidate mask (here: the sign itself).
// Built only by the test suite (lajolla_public_amd/build.py build_twin_scan), never loaded by the product.
#include "../../lajolla_public_amd/csrc/device/dscan.h"
#include <cstdint>

using namespace ljd;

namespace {

float rcp_moved(float d, int ulps) {
    float i = 1.0f / d;
    for (; ulps > 0; ulps--) i = nextafterf(i, INFINITY);
    for (; ulps < 0; ulps++) i = nextafterf(i, -INFINITY);
    return i;
}

}  // namespace

extern "C" {

// lo, hi, c, h: n x 3 floats
void twin_scan_convert(int64_t n, const float *lo, const float *hi, float *c, float *h) {
    for (int64_t k = 0; k < n; k++) scan_leaf_from_box(lo + 3 * k, hi + 3 * k, c + 3 * k, h + 3 * k);
}

// Case k: box record c[3k..], h[3k..] against the segment org + t dir, t in [tnear, tfar] (far != 0), or [tnear, inf) (far == 0: tfar is
// not read, as for an extension ray), the reciprocal of axis a moved by rcp_ulps[a] ulps.  accept[k] = 1: the scan would enter the box.
void twin_scan_box(int64_t n, const float *c, const float *h, const float *org, const float *dir, const float *tnear, const float *tfar,
                   int far, const int *rcp_ulps, uint8_t *accept) {
    for (int64_t k = 0; k < n; k++) {
        const float b[6] = {c[3 * k], c[3 * k + 1], c[3 * k + 2], h[3 * k], h[3 * k + 1], h[3 * k + 2]};
        ScanRay r;   // (scan_ray of mega.hip)
        r.ix = rcp_moved(scan_clamp_dir(dir[3 * k]), rcp_ulps[0]); r.iy = rcp_moved(scan_clamp_dir(dir[3 * k + 1]), rcp_ulps[1]);
        r.iz = rcp_moved(scan_clamp_dir(dir[3 * k + 2]), rcp_ulps[2]);
        r.ox = org[3 * k] * r.ix; r.oy = org[3 * k + 1] * r.iy; r.oz = org[3 * k + 2] * r.iz;
        const float tn = fmaxf(tnear[k], 0.0f);
        const float d = far ? scan_box<true>(b, r, tn, tfar[k]) : scan_box<false>(b, r, tn, INFINITY);
        accept[k] = signbit(d) ? 1 : 0;
    }
}

}
