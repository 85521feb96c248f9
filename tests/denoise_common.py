"""Shared pieces of the denoising tests (lj_denoise): the host twin of device/ddenoise.h (tests/twin_denoise), a float64 numpy model of the
rule written from the header's text, and seeded synthetic inputs — piecewise-planar "scenes" (regions with their own normal, albedo and depth
ramp, and a miss region of depth 0), a smooth colour field, and per-pixel noise drawn with the stated variance."""
import ctypes as C

import numpy as np

from lajolla_public_amd import build

OPTIONAL = ("variance", "albedo", "normal", "depth")
CHANNELS = {"rgb": 3, "variance": 3, "albedo": 3, "normal": 3, "depth": 1}
DEFAULTS = dict(sigma_color=4.0, sigma_normal=0.5, sigma_depth=0.1, sigma_albedo=0.25)
SIZES = [(1, 1, 1), (1, 5, 7), (1, 29, 37), (2, 16, 20)]   # (n, h, w): 1x1, 7x5, 37x29 (partial tiles), a batch of two 20x16

_lib = None


def twin_lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build.build_twin_denoise(verbose=False))
        _lib.twin_denoise.restype = C.c_int
        _lib.twin_denoise.argtypes = [C.c_int] * 3 + [C.c_void_p] * 5 + [C.c_int, C.c_uint] + [C.c_float] * 4 + [C.c_void_p] * 2
    return _lib


def twin_denoise(inputs, iterations=0, demodulate=False, in_place=False, **sigmas):
    """The host twin on a dict of (n, h, w, c) / (n, h, w) float32 arrays: (rgb_out, variance_out or None)."""
    rgb = np.ascontiguousarray(inputs["rgb"], np.float32)
    n, h, w = rgb.shape[:3]
    arrays = {k: np.ascontiguousarray(inputs[k], np.float32) for k in OPTIONAL if inputs.get(k) is not None}
    out = rgb.copy() if in_place else np.full(rgb.shape, 7.0, np.float32)
    var = np.full(rgb.shape, 7.0, np.float32) if "variance" in arrays else None
    src = out if in_place else rgb
    rc = twin_lib().twin_denoise(n, w, h, src.ctypes.data, *[arrays[k].ctypes.data if k in arrays else None for k in OPTIONAL], int(iterations), 1 if demodulate else 0,
                                 *[float(sigmas.get(k, 0.0)) for k in DEFAULTS], out.ctypes.data, var.ctypes.data if var is not None else None)
    assert rc == 0
    return out, var


def same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------ the float64 model (from the text of ddenoise.h)
def _shifted(a, oy, ox):
    """(view of a at q = p + (oy, ox), slices of p) for the p whose q is inside the image; a: (n, h, w, ...)"""
    h, w = a.shape[1:3]
    y0, y1, x0, x1 = max(0, -oy), min(h, h - oy), max(0, -ox), min(w, w - ox)
    if y0 >= y1 or x0 >= x1:
        return None, None
    return a[:, y0 + oy:y1 + oy, x0 + ox:x1 + ox], (slice(None), slice(y0, y1), slice(x0, x1))


def _stop(x):
    return np.maximum(0.0, 1.0 - x) ** 2


def model_denoise(inputs, iterations=0, demodulate=False, **sigmas):
    """float64: (rgb_out, variance_out or None)."""
    f64 = lambda k: None if inputs.get(k) is None else np.asarray(inputs[k], np.float32).astype(np.float64)
    rgb, var, alb, nrm, dep = (f64(k) for k in ("rgb",) + OPTIONAL)
    sg = {k: float(np.float32(sigmas.get(k) or DEFAULTS[k])) for k in DEFAULTS}
    iterations = iterations if iterations > 0 else 5
    eps, tiny = float(np.float32(1e-3)), float(np.float32(1e-12))
    c, v = rgb.copy(), (var.copy() if var is not None else np.zeros_like(rgb))
    if demodulate:
        e = alb + eps
        c, v = c / e, v / (e * e)
    hk = [1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16]
    for i in range(iterations):
        s = 1 << i
        if var is not None:   # g_p: the renormalised 3 x 3 binomial average of the summed variance
            vs = v.sum(-1)
            gs, gw = np.zeros_like(vs), np.zeros_like(vs)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    q, p = _shifted(vs, dy, dx)
                    if q is None:
                        continue
                    k = (0.5 if dx == 0 else 0.25) * (0.5 if dy == 0 else 0.25)
                    gs[p] += k * q
                    gw[p] += k
            cden = sg["sigma_color"] ** 2 * (gs / gw) + tiny
        sw, sc, sv = np.zeros(c.shape[:3]), np.zeros_like(c), np.zeros_like(v)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                cq, p = _shifted(c, s * dy, s * dx)
                if cq is None:
                    continue
                wt = np.full(cq.shape[:3], hk[dx + 2] * hk[dy + 2])
                if nrm is not None:
                    wt = wt * _stop(((nrm[p] - _shifted(nrm, s * dy, s * dx)[0]) ** 2).sum(-1) / sg["sigma_normal"] ** 2)
                if dep is not None:
                    dp, dq = dep[p], _shifted(dep, s * dy, s * dx)[0]
                    m = np.maximum(dp, dq)
                    wt = wt * _stop(np.where(m == 0, 0.0, (dp - dq) ** 2 / (sg["sigma_depth"] ** 2 * np.where(m == 0, 1.0, m) ** 2)))
                if alb is not None:
                    wt = wt * _stop(((alb[p] - _shifted(alb, s * dy, s * dx)[0]) ** 2).sum(-1) / sg["sigma_albedo"] ** 2)
                if var is not None:
                    wt = wt * _stop(((c[p] - cq) ** 2).sum(-1) / cden[p])
                sw[p] += wt
                sc[p] += wt[..., None] * cq
                sv[p] += (wt * wt)[..., None] * _shifted(v, s * dy, s * dx)[0]
        c, v = sc / sw[..., None], sv / (sw * sw)[..., None]
    if demodulate:
        c, v = c * e, v * (e * e)
    return c, (v if var is not None else None)


def rel_err(got, ref):
    """largest relative error, floor 1e-6 on the denominator"""
    return float((np.abs(got.astype(np.float64) - ref) / np.maximum(np.abs(ref), 1e-6)).max())


# ------------------------------------------------------------------ synthetic inputs
def make_inputs(n, h, w, seed=0):
    """All five buffers, (n, h, w, c) float32: three planar regions and a miss region per image, a smooth field, noise of the stated variance."""
    rng = np.random.default_rng(1000 * seed + 17 * n + 31 * h + w)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    out = {k: np.zeros((n, h, w) + ((3,) if CHANNELS[k] == 3 else ()), np.float32) for k in CHANNELS}
    for i in range(n):
        region = np.zeros((h, w), np.int32)
        region[x > 0.4 * w + 0.15 * y + i] = 1
        region[(y > 0.6 * h) & (x > 0.55 * w)] = 2
        region[(y < 0.25 * h) & (x > 0.75 * w)] = 3   # the miss region
        normals = np.array([[0.0, 0.0, 1.0], [0.8, 0.0, 0.6], [0.0, 1.0, 0.0]])
        albedos = rng.uniform(0.15, 0.9, (3, 3))
        nrm, alb, dep = np.zeros((h, w, 3)), np.zeros((h, w, 3)), np.zeros((h, w))
        for r in range(3):
            sel = region == r
            nrm[sel], alb[sel] = normals[r], albedos[r]
            dep[sel] = (2.0 + 1.5 * r + 0.01 * (1 + r) * x + 0.007 * y)[sel]
        field = 0.6 + 0.3 * np.sin(x / 7.0 + i) * np.cos(y / 5.0) + 0.002 * x
        clean = np.where((region == 3)[..., None], 0.05, alb * field[..., None])
        sd = 0.04 + 0.12 * clean
        out["rgb"][i] = clean + sd * rng.standard_normal((h, w, 3))
        out["variance"][i], out["albedo"][i], out["normal"][i], out["depth"][i] = sd * sd, alb, nrm, dep
    return out


def subset(inputs, *drop):
    return {k: v for k, v in inputs.items() if k not in drop}


def image_of(inputs, i):
    return {k: v[i:i + 1] for k, v in inputs.items()}


# which buffers a case leaves out, and whether it demodulates: all with and without the flag, each optional buffer left out, none at all
CASES = [((), True), ((), False), (("variance",), True), (("albedo",), False), (("normal",), True), (("depth",), False), (OPTIONAL, False)]
