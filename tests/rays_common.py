"""Shared pieces of the tests of lj_radiance_rays / lj_irradiance: the host twin of device/dprobe.h (tests/twin_rays), the scenes on the
47 x 41 film of tests/views_common.py, and the table of camera samples the main test feeds back as rays — the first 3 rows of the film at
4 spp, 564 rays: no multiple of 64, and across the 16-pixel tile edge."""
import ctypes as C
import math
import os

import numpy as np

import lajolla_public_amd as lj
from lajolla_public_amd import _abi, build
from helpers import SCENES, scene_path
from features_common import disney_scene, sample_jitter
from views_common import W, H, CBOX_VIEWS, cbox_cameras, derived_cameras, set_host_camera

ROWS, SPP = 3, 4
CROP = (0, 0, W, ROWS)
N_RAYS = W * ROWS * SPP
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rays")
LE = np.array([0.5, 1.0, 2.0], np.float32)
PI_F = np.float32(3.14159274)
SENTINEL = np.float32(-7.25)

_lib = None


def twin_rays_lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build.build_twin_rays(verbose=False))
        _lib.twin_rays_create.restype = C.c_void_p
        _lib.twin_rays_create.argtypes = [C.POINTER(_abi.LjSceneDesc), C.c_char_p, C.c_int]
        _lib.twin_rays_free.argtypes = [C.c_void_p]
        _lib.twin_rays_trace.argtypes = [C.c_void_p, C.c_int, C.POINTER(_abi.LjRenderArgs), C.POINTER(_abi.LjRaysArgs), C.c_int64, C.c_void_p,
                                         C.POINTER(_abi.LjRadianceBuffers), C.c_int, C.c_char_p, C.c_int]
        _lib.twin_rays_probe_rays.argtypes = [C.c_void_p, C.POINTER(_abi.LjRenderArgs), C.c_int64, C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
    return _lib


def table(a, b):
    """(n, 6) float32: LjRadianceRay (org, dir) or LjProbe (position, normal)."""
    return np.ascontiguousarray(np.concatenate([np.asarray(a, np.float32).reshape(-1, 3), np.asarray(b, np.float32).reshape(-1, 3)], axis=1))


def buffers(n, spp, fill=SENTINEL):
    """The three outputs, pre-filled, and the struct that points at them."""
    out = dict(radiance=np.full((n, 3), fill, np.float32), variance=np.full((n, 3), fill, np.float32), samples=np.full((n, spp, 3), fill, np.float32))
    b = _abi.LjRadianceBuffers()
    for k, a in out.items():
        setattr(b, k, a.ctypes.data)
    return out, b


class TwinRays:
    """Host build of lj_radiance_rays / lj_irradiance / lj_probe_ray_queries (tests/twin_rays): the same checks, the same generation code."""

    def __init__(self, host_scene):
        self.hs = host_scene
        self.lib = twin_rays_lib()
        err = C.create_string_buffer(512)
        self.h = C.c_void_p(self.lib.twin_rays_create(host_scene.desc_ptr, err, 512))
        if not self.h:
            raise RuntimeError(err.value.decode())

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.twin_rays_free(self.h)
            self.h = None

    def call(self, probes, args, rays_args, n, tab, bufs):
        """The raw call: (error code, message)."""
        err = C.create_string_buffer(512)
        rc = self.lib.twin_rays_trace(self.h, C.c_int(1 if probes else 0), C.byref(args) if args is not None else None, C.byref(rays_args) if rays_args is not None else None,
                                      C.c_int64(n), tab.ctypes.data_as(C.c_void_p) if tab is not None else None, C.byref(bufs) if bufs is not None else None, C.c_int(0), err, 512)
        return rc, err.value.decode()

    def trace(self, tab, spp, probes=False, medium_id=None, ray_spread=None, **kw):
        tab = np.ascontiguousarray(tab, np.float32).reshape(-1, 6)
        out, b = buffers(len(tab), spp)
        rc, msg = self.call(probes, lj.make_args(spp=spp, **kw), lj.make_rays_args(medium_id, ray_spread), len(tab), tab, b)
        assert rc == 0, msg
        return out

    def probe_rays(self, probes, spp, seed=0):
        probes = np.ascontiguousarray(probes, np.float32).reshape(-1, 6)
        out = np.zeros((len(probes), spp, 6), np.float32)
        err = C.create_string_buffer(512)
        args = lj.make_args(spp=spp, seed=seed)
        rc = self.lib.twin_rays_probe_rays(self.h, C.byref(args), C.c_int64(len(probes)), probes.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), err, 512)
        assert rc == 0, err.value.decode()
        return out


def vol_file(name):
    return os.path.join(SCENES, "volpath_test", name + ".xml")


def film_scene(name, view=0):
    """The scene on the 47 x 41 film; cbox: from CBOX_VIEWS[view] (3 lies inside the box)."""
    if name == "disney":
        assert view == 0
        return disney_scene()
    if name in ("furnace", "furnace_vol"):
        return lj.parse_scene(os.path.join(GOLDEN, name + ".xml"))
    hs = lj.parse_scene(scene_path(name) if name in ("cbox", "veach_mi") else vol_file(name))
    if name == "hetvol":
        # the parsed pose with 0.3 of its field of view: the smoke then reaches the first rows of the film, which the scene's own camera leaves black
        assert view == 0
        c = hs.desc.camera
        m = np.array(list(c.cam_to_world)).reshape(4, 4)
        fov = math.degrees(2.0 * math.atan(1.0 / (-2.0 * c.cam_to_sample[0])))
        return set_host_camera(hs, lj.look_at_camera(m[:3, 3], m[:3, 3] + m[:3, 2], m[:3, 1], 0.3 * fov, W, H, c.filter_kind, c.filter_param, c.medium_id))
    cams = cbox_cameras(hs) if name in ("cbox", "vol_cbox") else derived_cameras(hs, 1.0)
    return set_host_camera(hs, cams[view])


def camera_sample_rays(ex, hs, seed=0, crop=CROP, spp=SPP):
    """Ray p * spp + s = camera sample (pixel p of the window, sample s) of an spp-sample render with `seed`: (n, 6) float32, from the executor's
    pcg32 and primary-ray queries (helpers.TwinQueries / GpuQueries)."""
    x, y, jx, jy = sample_jitter(ex, hs.width, crop, spp, seed)
    q = np.zeros(len(x), lj.PRIMARY_QUERY)
    q["x"], q["y"], q["jx"], q["jy"] = x, y, jx, jy
    pr = ex.primary(q)
    return table(pr["org"], pr["dir"])


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def cbox_probes():
    """Probes on the floor and on a wall of the Cornell box (cbox units): positions on the surfaces, normals into the box."""
    pos, nrm = [], []
    for x in (100.0, 278.0, 450.0):
        for z in (100.0, 300.0, 500.0):
            pos.append((x, 0.0, z)); nrm.append((0.0, 1.0, 0.0))          # floor
    for y in (100.0, 300.0, 500.0):
        for z in (150.0, 400.0):
            pos.append((0.5, y, z)); nrm.append((1.0, 0.0, 0.0))          # the wall at x = 0, seen from inside
    return table(pos, nrm)


def error_calls(hs):
    """(label, expected code, probes, args, rays args, n, table, pass buffers?, text the message holds) for every declared refusal."""
    ok = table([(0, 0, 0)] * 4, [(0, 0, 1)] * 4)
    bad_dir, nan_org, inf_dir, zero_dir = ok.copy(), ok.copy(), ok.copy(), ok.copy()
    bad_dir[2, 3:] = (0, 0, 1.001); nan_org[1, 0] = np.nan; inf_dir[3, 4] = np.inf; zero_dir[0, 3:] = 0
    A, R = lj.make_args, lj.make_rays_args
    inv, uns = _abi.LJ_ERR_INVALID_ARG, _abi.LJ_ERR_UNSUPPORTED
    flags = _abi.LjRaysArgs(); flags.flags = 4
    nan_spread = R(ray_spread=float("nan"))
    calls = [("tile schedule", uns, False, A(spp=1, rng_mode=_abi.LJ_RNG_TILE), None, 4, ok, True, "rng_mode"),
             ("null table", inv, False, A(spp=1), None, 4, None, True, "null"),
             ("null buffers", inv, False, A(spp=1), None, 4, ok, False, "null"),
             ("negative n", inv, False, A(spp=1), None, -1, ok, True, "n must"),
             ("n beyond 2^31", inv, False, A(spp=1), None, (1 << 31) + 1, ok, True, "n must"),
             ("spp beyond 2^20", inv, False, A(spp=(1 << 20) + 1), None, 4, ok, True, "2^20"),
             ("rank", inv, False, A(spp=1, rank=1, world_size=2), None, 4, ok, True, "rank"),
             ("world", inv, False, A(spp=1, world_size=2), None, 4, ok, True, "rank"),
             ("crop", inv, False, A(spp=1, crop=(0, 0, 4, 4)), None, 4, ok, True, "crop"),
             ("medium too large", inv, False, A(spp=1), R(medium_id=hs.desc.n_media), 4, ok, True, "medium_id"),
             ("medium below -1", inv, False, A(spp=1), R(medium_id=-2), 4, ok, True, "medium_id"),
             ("unknown flag", inv, False, A(spp=1), flags, 4, ok, True, "flag"),
             ("spread not finite", inv, False, A(spp=1), nan_spread, 4, ok, True, "ray_spread"),
             ("direction not unit", inv, False, A(spp=1), None, 4, bad_dir, True, "entry 2"),
             ("origin not finite", inv, False, A(spp=1), None, 4, nan_org, True, "entry 1"),
             ("direction not finite", inv, False, A(spp=1), None, 4, inf_dir, True, "entry 3"),
             ("normal of length 0", inv, True, A(spp=1), None, 4, zero_dir, True, "entry 0"),
             ("normal not unit", inv, True, A(spp=1), None, 4, bad_dir, True, "entry 2")]
    return calls
