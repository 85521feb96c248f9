"""The leaf scan's box test (device/dscan.h: centre / half-extent records, three fused multiply-adds per axis) built for the host
(tests/twin_scan) and checked for the one property the scan needs: it is CONSERVATIVE.  Whenever the exact segment meets the builder's
UNPADDED primitive box, the float test on the table record of the leaf that holds it accepts — for the correctly rounded reciprocal and for its neighbours one ulp
either side (the device's v_rcp_f32 is a 1-ulp reciprocal), on every axis together and on the axes in opposite directions.

The exact decision is taken in double on the float inputs, closed intervals (a direction component of exactly zero: the origin must lie
within the slab); its rounding is 1e-9 of the float test's own, and a flat box or an origin on a face gives exact ties either way.

A leaf is the union of up to eight primitive boxes, each padded on its own (1e-5 of ITS coordinates): half the cases build the record from
the primitive's padded box joined with a second padded box up to 10^6 times its size, a fifth of those with the primitive within 1e-9 .. 1e-3
of coordinate zero, and put origins inside the leaf within 1e-9 .. 1e-6 of its size of a face the small primitive defines, heading out
through it — where the rounding of the box centre's distance is largest against the primitive's own pad.  Some flat boxes lie at coordinate
exactly zero, where the builder's pad is 1e-30."""
import ctypes as C

import numpy as np
import pytest

from lajolla_public_amd import build

N = 500_000   # cases per segment kind (bounded / unbounded): 10^6 in all, each run with five reciprocal variants

_lib = None


def _twin():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build.build_twin_scan(verbose=False))
        _lib.twin_scan_convert.argtypes = [C.c_int64] + [C.c_void_p] * 4
        _lib.twin_scan_box.argtypes = [C.c_int64] + [C.c_void_p] * 6 + [C.c_int, C.c_void_p, C.c_void_p]
    return _lib


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _pad(lo, hi):
    """The builder's box padding (host/bvh.cpp, Box::pad), in float like there."""
    p = np.float32(1e-5) * (np.abs(lo) + np.abs(hi)) + np.float32(1e-7) * (hi - lo) + np.float32(1e-30)
    return _f32(lo - p), _f32(hi + p)


def _convert(lo, hi):
    c, h = np.zeros_like(lo), np.zeros_like(lo)
    _twin().twin_scan_convert(len(lo), lo.ctypes.data, hi.ctypes.data, c.ctypes.data, h.ctypes.data)
    return c, h


def _cases(seed, far):
    """Boxes of every kind the table can hold and segments aimed where a slab test can go wrong."""
    rng = np.random.default_rng(seed)
    n = N
    # ---- boxes: coordinates of magnitude 1e-3 .. 1e4, extents from a thousandth of that up to it; 40 % flat on one or two axes
    scale = 10.0 ** rng.uniform(-3, 4, (n, 1))
    ctr = scale * rng.uniform(0.1, 1.0, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))
    ext = scale * 10.0 ** rng.uniform(-3, 0, (n, 3)) * rng.random((n, 3))
    flat = rng.random(n) < 0.4
    n_flat = rng.integers(1, 3, n)
    order = np.argsort(rng.random((n, 3)), axis=1)   # a random permutation of the axes per case
    for j in range(2):
        m = flat & (n_flat > j)
        ext[m, order[m, j]] = 0.0
    # a twentieth of the boxes: flat at coordinate exactly zero on one axis
    at_zero = rng.random(n) < 0.05
    az_axis = rng.integers(0, 3, n)
    rows = np.flatnonzero(at_zero)
    ctr[rows, az_axis[rows]] = 0.0
    ext[rows, az_axis[rows]] = 0.0
    # half the boxes share their leaf with a second, much larger box (below); a fifth of those lie within 1e-9 .. 1e-3 of coordinate zero
    multi = rng.random(n) < 0.5
    tiny = multi & (rng.random(n) < 0.2)
    shrink = 10.0 ** rng.uniform(-9, -3, (n, 1)) / scale
    ctr = np.where(tiny[:, None], ctr * shrink, ctr)
    ext = np.where(tiny[:, None], ext * shrink, ext)
    lo, hi = _f32(ctr - ext), _f32(ctr + ext)
    hi = np.maximum(lo, hi)
    # the leaf's record input: the primitive's padded box, for `multi` joined with the padded box of a neighbour that extends away from it
    # on every axis (so the primitive defines one face per axis), 1 .. 10^6 times its size
    rec_lo, rec_hi = _pad(lo, hi)
    big = np.maximum(np.maximum((hi - lo).max(axis=1, keepdims=True), np.abs(lo).max(axis=1, keepdims=True)).astype(np.float64), 1e-9)
    big = big * 10.0 ** rng.uniform(0, 6, (n, 1))
    side = rng.choice([-1.0, 1.0], (n, 3))
    gap, length = big * rng.random((n, 3)) * 0.1, big * rng.uniform(0.1, 1.0, (n, 3))
    q_lo = np.where(side > 0, lo + gap, hi - gap - length)
    q_hi = np.where(side > 0, lo + gap + length, hi - gap)
    q_lo, q_hi = _pad(_f32(q_lo), _f32(np.maximum(q_lo, q_hi)))
    rec_lo = np.where(multi[:, None], np.minimum(rec_lo, q_lo), rec_lo)
    rec_hi = np.where(multi[:, None], np.maximum(rec_hi, q_hi), rec_hi)
    size = np.maximum((hi - lo).max(axis=1, keepdims=True).astype(np.float64), 1e-3 * scale)
    lo64, hi64 = lo.astype(np.float64), hi.astype(np.float64)
    # ---- origins: a) around the box, b) inside it, c) exactly on a face, the other coordinates in or near the box
    kind = rng.integers(0, 3, n)
    inside = lo64 + (hi64 - lo64) * rng.random((n, 3))
    near = 0.5 * (lo64 + hi64) + size * rng.uniform(-3, 3, (n, 3))
    org = np.where((kind == 1)[:, None], inside, near)
    on_face = kind == 2
    face_axis = rng.integers(0, 3, n)
    face_side = rng.random(n) < 0.5
    mixed = np.where(rng.random((n, 3)) < 0.7, inside, near)
    org[on_face] = mixed[on_face]
    org = _f32(org)
    rows = np.flatnonzero(on_face)
    org[rows, face_axis[rows]] = np.where(face_side[rows], lo[rows, face_axis[rows]], hi[rows, face_axis[rows]])
    # d) multi-primitive leaves, half of them: inside the leaf, 1e-9 .. 1e-6 of its size from the face the small primitive defines on one
    # axis (the other coordinates within the primitive), heading out through that face
    leaf_size = (rec_hi - rec_lo).max(axis=1).astype(np.float64)
    graze = multi & (rng.random(n) < 0.5)
    g_axis = rng.integers(0, 3, n)
    rows = np.flatnonzero(graze)
    g_low = side[rows, g_axis[rows]] > 0                      # the primitive defines the leaf's LOWER face on this axis
    inward = leaf_size[rows] * 10.0 ** rng.uniform(-9, -6, len(rows))
    org[rows] = _f32(inside[rows])
    org[rows, g_axis[rows]] = _f32(np.where(g_low, rec_lo[rows, g_axis[rows]] + inward, rec_hi[rows, g_axis[rows]] - inward))
    # ---- directions: towards a point in or just around the box, or anywhere; then some components exactly zero or +-1e-30
    target = 0.5 * (lo64 + hi64) + (0.5 * (hi64 - lo64) + 0.3 * size * (rng.random((n, 1)) < 0.5)) * rng.uniform(-1.3, 1.3, (n, 3))
    d = np.where((rng.random(n) < 0.7)[:, None], target - org, rng.normal(size=(n, 3)))
    d[np.abs(d).sum(axis=1) == 0] = 1.0
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    # (the largest component stays as it is: the renderer's directions are unit vectors, and the 1e-18 clamp of tiny components
    # presupposes that some component is not tiny — a direction of (0, 0, 1e-30) is not a ray the scan is built for)
    special = rng.random((n, 3))
    special[np.arange(n), np.abs(d).argmax(axis=1)] = 1.0
    d = np.where(special < 0.12, 0.0, d)
    d = np.where((special >= 0.12) & (special < 0.2), 1e-30 * np.sign(d + 1e-300), d)
    d = np.where(rng.random((n, 3)) < 0.03, np.sign(d), d)                      # components of exactly +-1
    rows = np.flatnonzero(graze)
    d[rows, g_axis[rows]] = np.where(g_low, -1.0, 1.0) * np.maximum(np.abs(d[rows, g_axis[rows]]), 1e-3 * rng.random(len(rows)) + 1e-6)
    d = _f32(d)
    # ---- tnear 0 or epsilon; tfar finite around the distance to the box, or infinite
    dist = np.linalg.norm(0.5 * (lo64 + hi64) - org, axis=1)
    tnear = _f32(np.where(rng.random(n) < 0.5, 0.0, 1e-5 * scale[:, 0]))
    tfar = _f32(np.where(rng.random(n) < 0.25, np.inf, (dist + 0.1 * size[:, 0]) * rng.uniform(0, 2, n) + tnear))   # (never a segment of no length)
    if not far:
        tfar = np.full(n, np.inf, np.float32)
    tnear[graze & (rng.random(n) < 0.8)] = 0.0
    return lo, hi, rec_lo, rec_hi, org, d, tnear, tfar, multi, graze


def _exact_meets(lo, hi, org, d, tnear, tfar):
    lo, hi, org, d = (a.astype(np.float64) for a in (lo, hi, org, d))
    zero = d == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        t1, t2 = (lo - org) / d, (hi - org) / d
    tn = np.where(zero, -np.inf, np.minimum(t1, t2))
    tf = np.where(zero, np.inf, np.maximum(t1, t2))
    ok = np.where(zero, (lo <= org) & (org <= hi), True).all(axis=1)
    te = np.maximum(tn.max(axis=1), tnear.astype(np.float64))
    tx = np.minimum(tf.min(axis=1), tfar.astype(np.float64))
    return ok & (te <= tx)


@pytest.fixture(scope="module", params=[0, 1], ids=["unbounded", "bounded"])
def cases(request):
    far = request.param
    lo, hi, plo, phi, org, d, tnear, tfar, multi, graze = _cases(20 + far, far)
    plo, phi = _f32(plo), _f32(phi)
    c, h = _convert(plo, phi)
    return dict(far=far, multi=multi, graze=graze, lo=lo, hi=hi, plo=plo, phi=phi, c=c, h=h, org=org, d=d, tnear=tnear, tfar=tfar,
                meets=_exact_meets(lo, hi, org, d, tnear, tfar))


def test_table_record_contains_the_leaf_box_grown_as_documented_and_no_further(cases):
    plo, phi, c, h = (cases[k].astype(np.float64) for k in ("plo", "phi", "c", "h"))
    assert (c - h <= plo).all() and (c + h >= phi).all()          # (sums of two floats this close in magnitude are exact in double)
    assert (np.abs(c - 0.5 * (plo + phi)) <= 0.5 * np.spacing(np.abs(cases["c"])).astype(np.float64)).all()
    # h = the smallest float >= need + 64 * 2^-24 * (|c| + need) + 1e-12 (dscan.h: the rounding of the centre's distance, the clamp's drift)
    need = np.maximum(phi - c, c - plo)
    grown = need + 2.0 ** -18 * (np.abs(c) + need) + 1e-12
    assert (h >= grown * (1 - 1e-15)).all()
    assert (np.nextafter(cases["h"], np.float32(-np.inf)).astype(np.float64) < grown * (1 + 1e-15)).all(), "grown further than documented"


def test_cases_exercise_both_outcomes(cases):
    share = cases["meets"].mean()
    print(f"exact test says 'meets' in {share:.3f} of the cases")
    assert 0.1 < share < 0.9
    flat = ((cases["hi"] - cases["lo"]) == 0).any(axis=1)
    # each kind of case takes part with both outcomes
    for name, m in (("flat boxes", flat), ("zero direction components", (cases["d"] == 0).any(axis=1)),
                    ("1e-30 direction components", (np.abs(cases["d"]) == np.float32(1e-30)).any(axis=1)),
                    ("origins on a face", ((cases["org"] == cases["lo"]) | (cases["org"] == cases["hi"])).any(axis=1)),
                    ("origins inside", ((cases["org"] >= cases["lo"]) & (cases["org"] <= cases["hi"])).all(axis=1)),
                    ("leaves of two primitives", cases["multi"]), ("origins just inside a face the small primitive defines", cases["graze"]),
                    ("flat boxes at coordinate zero", ((cases["lo"] == 0) & (cases["hi"] == 0)).any(axis=1))):
        assert m.sum() > 10000 and 0.02 < cases["meets"][m].mean() <= 1.0, name
        assert cases["meets"][m].sum() > 5000, name


@pytest.mark.parametrize("ulps", [(0, 0, 0), (1, 1, 1), (-1, -1, -1), (1, -1, 1), (-1, 1, -1)])
def test_scan_enters_every_box_the_exact_segment_meets(cases, ulps):
    n = len(cases["lo"])
    accept = np.zeros(n, np.uint8)
    u = np.asarray(ulps, np.int32)
    _twin().twin_scan_box(n, cases["c"].ctypes.data, cases["h"].ctypes.data, cases["org"].ctypes.data, cases["d"].ctypes.data,
                          cases["tnear"].ctypes.data, cases["tfar"].ctypes.data, cases["far"], u.ctypes.data, accept.ctypes.data)
    missed = np.flatnonzero(cases["meets"] & (accept == 0))
    k = missed[:1]
    assert len(missed) == 0, (f"{len(missed)} boxes the segment meets are not entered; first: lo {cases['lo'][k]} hi {cases['hi'][k]} "
                              f"org {cases['org'][k]} dir {cases['d'][k]} tnear {cases['tnear'][k]} tfar {cases['tfar'][k]}")
    # ... and the test still rejects: it is a filter, not a constant
    assert (accept[~cases["meets"]] == 0).mean() > 0.5
