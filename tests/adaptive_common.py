"""Shared pieces of the adaptive-sampling tests (lj_render_adaptive): the host twin of device/dadaptive.h (tests/twin_adaptive), a float64
numpy model of the rule written from the header's text, make_plan's tile order, and seeded synthetic state."""
import ctypes as C

import numpy as np

from lajolla_public_amd import build

SEED_STEP = 0x9e3779b97f4a7c15
DEFAULT_SEED = 0x853c49e6748fea9b
ARGS = ("min_spp", "max_spp", "round_spp", "max_rounds", "target_error")

_lib = None


def twin_lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build.build_twin_adaptive(verbose=False))
        _lib.twin_adaptive_merge.restype = None
        _lib.twin_adaptive_merge.argtypes = [C.c_void_p, C.c_int64, C.c_uint32, C.c_int] + [C.c_void_p] * 5
        _lib.twin_adaptive_error.restype = None
        _lib.twin_adaptive_error.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 4
        _lib.twin_adaptive_select.restype = C.c_int64
        _lib.twin_adaptive_select.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_float, C.c_void_p, C.c_int64, C.c_void_p]
        _lib.twin_adaptive_params.restype = C.c_int
        _lib.twin_adaptive_params.argtypes = [C.c_int] * 4 + [C.c_float, C.c_void_p, C.c_void_p]
        _lib.twin_adaptive_seed.restype = C.c_uint64
        _lib.twin_adaptive_seed.argtypes = [C.c_uint64, C.c_uint32]
        _lib.twin_adaptive_output.restype = None
        _lib.twin_adaptive_output.argtypes = [C.c_int64] + [C.c_void_p] * 6
    return _lib


def same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


class State:
    """(n, mean, m2) of an h x w film, zeroed"""

    def __init__(self, h, w):
        self.h, self.w = h, w
        self.n, self.mean, self.m2 = np.zeros((h, w), np.uint32), np.zeros((h, w, 3), np.float32), np.zeros((h, w, 3), np.float32)


def twin_merge(state, lst, k, init, rgb, variance):
    lst, rgb, variance = np.ascontiguousarray(lst, np.uint32), np.ascontiguousarray(rgb, np.float32), np.ascontiguousarray(variance, np.float32)
    assert rgb.shape == state.mean.shape and variance.shape == state.mean.shape
    twin_lib().twin_adaptive_merge(lst.ctypes.data, lst.size, int(k), 1 if init else 0, rgb.ctypes.data, variance.ctypes.data, state.n.ctypes.data, state.mean.ctypes.data, state.m2.ctypes.data)


def twin_error(state):
    e2 = np.zeros((state.h, state.w), np.float32)
    twin_lib().twin_adaptive_error(state.w, state.h, state.n.ctypes.data, state.mean.ctypes.data, state.m2.ctypes.data, e2.ctypes.data)
    return e2


def twin_select(state, lst=None, min_spp=0, max_spp=0, round_spp=0, max_rounds=0, target_error=0.0):
    lst = np.arange(state.h * state.w, dtype=np.uint32) if lst is None else np.ascontiguousarray(lst, np.uint32)
    out = np.empty(max(lst.size, 1), np.uint32)
    got = twin_lib().twin_adaptive_select(state.w, state.h, state.n.ctypes.data, state.mean.ctypes.data, state.m2.ctypes.data, int(min_spp), int(max_spp), int(round_spp), int(max_rounds),
                                          float(target_error), lst.ctypes.data, lst.size, out.ctypes.data)
    assert got >= 0, "the twin refuses these arguments"
    return out[:got].copy()


def twin_params(min_spp=0, max_spp=0, round_spp=0, max_rounds=0, target_error=0.0):
    """(code, {the arguments with the defaults filled in})"""
    out, t = (C.c_uint32 * 4)(), C.c_float()
    rc = twin_lib().twin_adaptive_params(int(min_spp), int(max_spp), int(round_spp), int(max_rounds), float(target_error), out, C.byref(t))
    return rc, dict(min_spp=out[0], max_spp=out[1], round_spp=out[2], max_rounds=out[3], target_error=t.value)


def twin_seed(seed0, r):
    return int(twin_lib().twin_adaptive_seed(int(seed0), int(r)))


def twin_output(state):
    rgb, var, samples = np.empty_like(state.mean), np.empty_like(state.mean), np.empty_like(state.n)
    twin_lib().twin_adaptive_output(state.h * state.w, state.n.ctypes.data, state.mean.ctypes.data, state.m2.ctypes.data, rgb.ctypes.data, var.ctypes.data, samples.ctypes.data)
    return rgb, var, samples


def tile_order(w, h, rank=0, world=1, tile=16):
    """make_plan's list of a full frame: 16 x 16 tiles row-major, t % world == rank, row-major inside a tile"""
    ntx, nty = (w + tile - 1) // tile, (h + tile - 1) // tile
    out = []
    for t in range(ntx * nty):
        if t % world != rank:
            continue
        x0, y0 = (t % ntx) * tile, (t // ntx) * tile
        for y in range(y0, min(y0 + tile, h)):
            out.extend(range(y * w + x0, y * w + min(x0 + tile, w)))
    return np.array(out, np.uint32)


# ------------------------------------------------------------------ the float64 model (from the text of dadaptive.h)
def pairs(n):
    n = np.asarray(n, np.float64)
    return n * (n - 1.0)


def model_e2(state):
    """float64 e2 of every pixel (nan where n == 0)"""
    n = state.n.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        V = np.where(state.n >= 2, state.m2.astype(np.float64).sum(axis=-1) / pairs(n), 0.0)
    V = np.where(state.n > 0, V, -np.inf)   # a pixel without samples never is the maximum
    h, w = state.n.shape
    padded = np.full((h + 2, w + 2), -np.inf)
    padded[1:-1, 1:-1] = V
    g = np.max([padded[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy in (-1, 0, 1) for dx in (-1, 0, 1)], axis=0)
    S = state.mean.astype(np.float64).sum(axis=-1) / 3.0
    return np.where(state.n > 0, g / (S * S + np.float64(np.float32(1e-4))), np.nan)


def model_select(state, lst, max_spp, round_spp, target_error):
    """(the model's list, the pixels with n > 0 whose e2 lies within 1e-5 relative of target_error^2)"""
    t2 = np.float64(np.float32(target_error)) ** 2
    e2 = model_e2(state).reshape(-1)
    n = state.n.reshape(-1).astype(np.int64)
    ok = (n > 0) & (n + round_spp <= max_spp)
    with np.errstate(invalid="ignore"):
        sel = ok & (e2 > t2)
        band = (n > 0) & (np.abs(e2 - t2) <= 1e-5 * t2)
    lst = np.asarray(lst, np.uint32)
    return lst[sel[lst]], np.flatnonzero(band)


def rel_err(got, ref):
    """largest relative error, floor 1e-6 on the denominator (the convention of the denoising tests)"""
    return float((np.abs(got.astype(np.float64) - ref) / np.maximum(np.abs(ref), 1e-6)).max())


# ------------------------------------------------------------------ synthetic state
def make_state(h, w, seed=0, counts=(0, 4, 8, 28, 30, 32), level=1.0):
    """A film whose pixels hold one of `counts` samples (0: outside the share), a smooth brightness with a dark corner, and a variance of
    the mean that is `level` x the squared brightness x a factor: 10^-1.5 .. 1 at one pixel in twenty, 10^-6 .. 10^-3 elsewhere — so
    that a target near sqrt(level) x 0.1 selects the neighbourhoods of the noisy pixels and nothing else."""
    rng = np.random.default_rng(seed)
    st = State(h, w)
    st.n[...] = rng.choice(np.array(counts, np.uint32), size=(h, w))
    y, x = np.mgrid[0:h, 0:w]
    bright = 0.02 + 0.9 * (x + 1.0) / w * (y + 1.0) / h
    colour = 0.5 + rng.random((h, w, 3))
    st.mean[...] = (bright[..., None] * colour).astype(np.float32)
    S2 = (st.mean.astype(np.float64).sum(axis=-1) / 3.0) ** 2
    noisy = rng.random((h, w)) < 0.05   # (sparse: a noisy pixel selects its whole neighbourhood)
    V = level * (S2 + 1e-4) * 10.0 ** np.where(noisy, rng.uniform(-1.5, 0.0, size=(h, w)), rng.uniform(-6.0, -3.0, size=(h, w)))
    share = rng.dirichlet(np.ones(3), size=(h, w))
    st.m2[...] = (V[..., None] * share * pairs(np.maximum(st.n, 2))[..., None]).astype(np.float32)
    st.mean[st.n == 0] = 0
    st.m2[st.n == 0] = 0
    return st
