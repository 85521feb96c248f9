"""Shared pieces of the guide-buffer tests (lj_render_features): the host twin of device/dfeature.h (tests/twin_features), and the rule of
include/lajolla_hip.h composed from the per-object queries — pcg32, primary ray, intersect (iterated through medium boundaries), vertex,
texture — on either executor of tests/helpers.py (the host twin of the device headers, or the GPU)."""
import ctypes as C
import os

import numpy as np

import lajolla_public_amd as lj
from lajolla_public_amd import _abi, build
from helpers import SCENES

MAX_SEGMENTS = 16   # a sample traces at most 16 segments; one whose 16th still ends on a medium boundary is a miss
HETVOL = os.path.join(SCENES, "volpath_test", "hetvol.xml")
FEATURES = ("albedo", "normal", "depth", "alpha", "variance")

_lib = None


def twin_features_lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build.build_twin_features(verbose=False))
        _lib.twin_features_create.restype = C.c_void_p
        _lib.twin_features_create.argtypes = [C.POINTER(_abi.LjSceneDesc), C.c_char_p, C.c_int]
        _lib.twin_features_free.argtypes = [C.c_void_p]
        _lib.twin_features_group_size.restype = C.c_uint32
        _lib.twin_features_group_size.argtypes = [C.c_uint32]
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _cams(cameras):
    if not cameras:
        return 0, None
    arr = (_abi.LjCamera * len(cameras))()
    for i, c in enumerate(cameras):
        C.memmove(C.addressof(arr[i]), C.addressof(c), C.sizeof(_abi.LjCamera))
    return len(cameras), arr


class TwinFeatures:
    """Host build of feature_sample and the reduction order (tests/twin_features)."""

    def __init__(self, host_scene):
        self.hs = host_scene
        self.lib = twin_features_lib()
        err = C.create_string_buffer(512)
        self.h = C.c_void_p(self.lib.twin_features_create(host_scene.desc_ptr, err, 512))
        if not self.h:
            raise RuntimeError(err.value.decode())

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.twin_features_free(self.h)
            self.h = None

    def samples(self, crop, spp, cameras=None, seed=0):
        """Per-sample values over the crop window: dict of a (.., ch, cw, spp, 3), n, d (.., ch, cw, spp), hit, segments; a leading view axis for a camera list."""
        x0, y0, x1, y1 = crop
        n, cams = _cams(cameras)
        lead = ((n,) if n else ()) + (y1 - y0, x1 - x0, spp)
        out = dict(a=np.zeros(lead + (3,), np.float32), n=np.zeros(lead + (3,), np.float32), d=np.zeros(lead, np.float32), hit=np.zeros(lead, np.float32),
                   segments=np.zeros(lead, np.int32))
        rc = self.lib.twin_features_samples(self.h, C.c_int(n), cams, C.c_int(spp), C.c_uint64(seed), C.c_int(x0), C.c_int(y0), C.c_int(x1), C.c_int(y1),
                                            _p(out["a"]), _p(out["n"]), _p(out["d"]), _p(out["hit"]), _p(out["segments"]))
        assert rc == 0
        return out

    def buffers(self, crop, spp, cameras=None, seed=0):
        x0, y0, x1, y1 = crop
        n, cams = _cams(cameras)
        lead = ((n,) if n else ()) + (y1 - y0, x1 - x0)
        out = dict(albedo=np.zeros(lead + (3,), np.float32), normal=np.zeros(lead + (3,), np.float32), depth=np.zeros(lead, np.float32), alpha=np.zeros(lead, np.float32))
        rc = self.lib.twin_features_buffers(self.h, C.c_int(n), cams, C.c_int(spp), C.c_uint64(seed), C.c_int(x0), C.c_int(y0), C.c_int(x1), C.c_int(y1),
                                            _p(out["albedo"]), _p(out["normal"]), _p(out["depth"]), _p(out["alpha"]))
        assert rc == 0
        return out


def image_textured(hs):
    """disney_bsdf with its object's base colour (material 0, slot 0) read from the scene's one RGB image — the environment map's — so that
    slot 0 is an image texture with a mip pyramid; the plane keeps its checkerboard.  (The description is plain memory owned by the HostScene.)"""
    assert hs.desc.n_images3 >= 1 and _abi.MATERIAL_KINDS[hs.desc.materials[0].kind] == "disneybsdf"
    t = hs.desc.materials[0].tex[0]
    t.kind, t.texture_id, t.uscale, t.vscale, t.uoffset, t.voffset = _abi.LJ_TEX_IMAGE, 0, 3.0, 2.0, 0.25, 0.0
    return hs


def disney_scene():
    """disney_bsdf on the 47 x 41 film of tests/views_common.py, image-textured, from a raised camera: the object, the checkerboard plane and
    the sky (misses under the environment map) all lie inside the crop windows of the tests."""
    from helpers import scene_path
    from views_common import W, H, set_host_camera
    hs = image_textured(lj.parse_scene(scene_path("disney_bsdf")))
    c = hs.desc.camera
    return set_host_camera(hs, lj.look_at_camera((3.69558, -3.46243, 3.25463), (0.0, 0.0, 1.0), (0.0, 0.0, 1.0), 80.0, W, H, c.filter_kind, c.filter_param, c.medium_id))


def twin_reduce(x):
    """x: (n, spp) float32 -> (sum in the group order, mean and variance in the wave order), each (n,) float32."""
    x = np.ascontiguousarray(x, np.float32)
    n, spp = x.shape
    s, m, v = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    twin_features_lib().twin_features_reduce(_p(x), C.c_int64(n), C.c_uint32(spp), _p(s), _p(m), _p(v))
    return s, m, v


def twin_depth_alpha(d, hit):
    d, hit = np.ascontiguousarray(d, np.float32), np.ascontiguousarray(hit, np.float32)
    n, spp = d.shape
    depth, alpha = np.zeros(n, np.float32), np.zeros(n, np.float32)
    twin_features_lib().twin_features_depth_alpha(_p(d), _p(hit), C.c_int64(n), C.c_uint32(spp), _p(depth), _p(alpha))
    return depth, alpha


def group_size(spp):
    return int(twin_features_lib().twin_features_group_size(C.c_uint32(spp)))


# ------------------------------------------------------------------ the rule, composed from the per-object queries
def sample_jitter(ex, w, crop, spp, seed=0):
    """(x, y, jx, jy) of every camera sample of the window, (ch * cw * spp,) each: stream (y*w + x)*spp + s, first draw jy, second jx."""
    x0, y0, x1, y1 = crop
    ys, xs, ss = np.meshgrid(np.arange(y0, y1), np.arange(x0, x1), np.arange(spp), indexing="ij")
    streams = ((ys * w + xs) * spp + ss).astype(np.uint64).ravel()
    _, f = ex.pcg32(streams, 2, seed)
    return xs.ravel().astype(np.int32), ys.ravel().astype(np.int32), f[:, 1].copy(), f[:, 0].copy()


def slot0_albedo(ex, hs, material_ids, uv, footprint):
    """The materials' slot-0 texture as a Spectrum at (uv, footprint), through the executor's texture query; (1, 1, 1) for disneyclearcoat."""
    out = np.zeros((len(material_ids), 3), np.float32)
    tex_dtype = lj.TEXTURE_QUERY["texture"]
    for m in np.unique(material_ids):
        sel = np.nonzero(material_ids == m)[0]
        mat = hs.desc.materials[int(m)]
        if _abi.MATERIAL_KINDS[mat.kind] == "disneyclearcoat":
            out[sel] = 1.0
            continue
        q = np.zeros(len(sel), lj.TEXTURE_QUERY)
        q["texture"] = np.frombuffer(bytes(mat.tex[0]), dtype=tex_dtype)[0]
        q["uv"], q["footprint"], q["spectrum"] = uv[sel], footprint[sel], 1
        out[sel] = ex.texture(q)
    return out


def compose_samples(ex, intersect, hs, eps, crop, spp, seed=0):
    """The per-sample rule from the executor's queries.  intersect(rays) -> hits (lj.HIT_DTYPE).  Returns dict of a, n (N, 3), d, hit (N,),
    segments, material (N,), N = ch * cw * spp in window order; a, n, hit exactly as the queries return them, d in float32 arithmetic."""
    w, h = hs.width, hs.height
    x, y, jx, jy = sample_jitter(ex, w, crop, spp, seed)
    N = len(x)
    q = np.zeros(N, lj.PRIMARY_QUERY)
    q["x"], q["y"], q["jx"], q["jy"] = x, y, jx, jy
    pr = ex.primary(q)
    cam_org, org, dirs = pr["org"].copy(), pr["org"].copy(), pr["dir"].copy()
    tnear = np.zeros(N, np.float32)
    out = dict(a=np.zeros((N, 3), np.float32), n=np.zeros((N, 3), np.float32), d=np.zeros(N, np.float32), hit=np.zeros(N, np.float32), segments=np.zeros(N, np.int32),
               material=np.full(N, -1, np.int32))
    alive = np.ones(N, bool)
    spread = np.float32(0.25 / max(w, h))
    for _ in range(MAX_SEGMENTS):
        idx = np.nonzero(alive)[0]
        if len(idx) == 0:
            break
        out["segments"][idx] += 1
        hits = intersect(lj._rays_array(org[idx], dirs[idx], tnear[idx], np.inf))
        got = hits["shape_id"] >= 0
        alive[idx[~got]] = False
        idx, hits = idx[got], hits[got]
        if len(idx) == 0:
            break
        vq = np.zeros(len(idx), lj.HIT_QUERY)
        vq["org"], vq["dir"], vq["t"], vq["u"], vq["v"] = org[idx], dirs[idx], hits["t"], hits["u"], hits["v"]
        vq["ray_spread"], vq["shape_id"], vq["primitive_id"] = spread, hits["shape_id"], hits["prim_id"]
        vx = ex.vertex(vq)["vertex"]
        surf = vx["material_id"] >= 0
        s_idx, sv = idx[surf], vx[surf]
        out["a"][s_idx] = slot0_albedo(ex, hs, sv["material_id"], sv["uv"], sv["uv_screen_size"])
        out["n"][s_idx], out["material"][s_idx] = sv["frame_n"], sv["material_id"]
        dp = (sv["position"] - cam_org[s_idx]).astype(np.float32)
        out["d"][s_idx] = np.sqrt((dp[:, 0] * dp[:, 0] + dp[:, 1] * dp[:, 1] + dp[:, 2] * dp[:, 2]).astype(np.float32)).astype(np.float32)
        out["hit"][s_idx] = 1.0
        alive[s_idx] = False
        b_idx = idx[~surf]                      # a medium boundary: on from the hit position with tnear = the scene's epsilon
        org[b_idx] = vx[~surf]["position"]
        tnear[b_idx] = np.float32(eps)
    return out


def reduce64(s, shape, spp):
    """The buffers from per-sample values, summed in float64: dict of albedo, normal (.., 3), depth, alpha, and mean |x| per buffer for the bounds."""
    a, n = s["a"].astype(np.float64).reshape(shape + (spp, 3)), s["n"].astype(np.float64).reshape(shape + (spp, 3))
    d, hit = s["d"].astype(np.float64).reshape(shape + (spp,)), s["hit"].astype(np.float64).reshape(shape + (spp,))
    hits = hit.sum(-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        depth = np.where(hits > 0, d.sum(-1) / np.maximum(hits, 1), 0.0)
    return dict(albedo=a.mean(-2), normal=n.mean(-2), depth=depth, alpha=hits / spp, hits=hits,
                mag=dict(albedo=np.abs(a).mean(-2), normal=np.abs(n).mean(-2), depth=np.where(hits > 0, np.abs(d).sum(-1) / np.maximum(hits, 1), 0.0)))


def sum_bound(spp, mag):
    """What a float sum of spp terms in another order may differ by from the exact one: spp * 2^-23 * mean |x_i|."""
    return spp * 2.0 ** -23 * mag


def variance64(x):
    """x (.., spp, 3) per-sample radiance -> (variance of the mean in float64, its bound for the float two-pass computation)."""
    x = x.astype(np.float64)
    spp = x.shape[-2]
    if spp == 1:
        return np.zeros(x.shape[:-2] + (3,)), np.zeros(x.shape[:-2] + (3,))
    var = ((x - x.mean(-2, keepdims=True)) ** 2).sum(-2) / (spp * (spp - 1))
    return var, 8 * spp * 2.0 ** -23 * var + (spp * 2.0 ** -24 * np.abs(x).mean(-2)) ** 2
