"""Shared inputs of the camera-batch tests (lj_render_views / lj_scene_set_camera): the 47 x 41 film — neither a multiple of 16 nor of 64, and
47 * 41 * spp is no multiple of 64 for odd spp, so waves straddle view boundaries — and four cameras per scene."""
import ctypes as C
import math
import os

import numpy as np

import lajolla_public_amd as lj
from lajolla_public_amd import _abi, build
from helpers import SCENES, scene_path

W, H = 47, 41
UP = (0.0, 1.0, 0.0)
# cbox units: the scene's own pose, two from outside the box, one from inside it
CBOX_VIEWS = [((278, 273, -800), (278, 273, -799), 39.3077),
              ((100, 400, -700), (278, 273, 280), 50.0),
              ((500, 150, -600), (278, 273, 280), 30.0),
              ((278, 273, 100), (200, 100, 400), 70.0)]


def scene_file(name):
    if name == "vol_cbox":
        return os.path.join(SCENES, "volpath_test", "vol_cbox.xml")
    return scene_path(name)


def cbox_cameras(hs, width=W, height=H):
    """V0..V3 with the scene's own filter and the parsed camera's medium."""
    c = hs.desc.camera
    return [lj.look_at_camera(o, t, UP, fov, width, height, c.filter_kind, c.filter_param, c.medium_id) for o, t, fov in CBOX_VIEWS]


def derived_cameras(hs, bounds_radius, width=W, height=H):
    """Other scenes: the parsed camera's pose and fov on the test film as V0, and three more with the origin moved by 10 % of the bounds
    radius and another fov."""
    c = hs.desc.camera
    m = np.array(list(c.cam_to_world)).reshape(4, 4)
    org, up, fwd = m[:3, 3], m[:3, 1], m[:3, 2]
    fov = math.degrees(2.0 * math.atan(1.0 / (-2.0 * c.cam_to_sample[0])))   # Camera::Camera: cam_to_sample(0, 0) = -cot(fov / 2) / 2
    r = 0.1 * bounds_radius
    out = []
    for d, f in (((0, 0, 0), fov), ((r, 0, 0), fov * 1.2), ((0, -r, 0), fov * 0.8), ((r, r, 0), fov * 1.1)):
        o = org + np.array(d, float)
        out.append(lj.look_at_camera(o, o + fwd, up, f, width, height, c.filter_kind, c.filter_param, c.medium_id))
    return out


def set_host_camera(hs, cam):
    """Overwrite the camera of a parsed scene (the description is plain memory owned by the HostScene)."""
    C.memmove(C.addressof(hs.desc.camera), C.addressof(cam), C.sizeof(_abi.LjCamera))
    return hs


def host_scene_with(name, cam):
    return set_host_camera(lj.parse_scene(scene_file(name)), cam)


def cameras_for(name, hs, bounds_radius=None, width=W, height=H):
    return cbox_cameras(hs, width, height) if name in ("cbox", "vol_cbox") else derived_cameras(hs, bounds_radius, width, height)


_twin_views = None


def twin_views_lib():
    global _twin_views
    if _twin_views is None:
        _twin_views = C.CDLL(build.build_twin_views(verbose=False))
        _twin_views.twin_views_create.restype = C.c_void_p
        _twin_views.twin_views_create.argtypes = [C.POINTER(_abi.LjSceneDesc), C.c_char_p, C.c_int]
        _twin_views.twin_views_free.argtypes = [C.c_void_p]
        _twin_views.twin_views_decode_mismatches.restype = C.c_longlong
        _twin_views.twin_views_decode_mismatches.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64]
    return _twin_views


class TwinViews:
    """Host build of the camera-batch path of the device headers (tests/twin_views)."""

    def __init__(self, host_scene):
        self.hs = host_scene
        self.lib = twin_views_lib()
        err = C.create_string_buffer(512)
        self.h = C.c_void_p(self.lib.twin_views_create(host_scene.desc_ptr, err, 512))
        if not self.h:
            raise RuntimeError(err.value.decode())

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.twin_views_free(self.h)
            self.h = None

    def render_samples(self, cameras, spp, max_depth=None, threads=0, seed=0):
        """(n, h, w, spp, 3) float32: per-sample radiance of every view over the full film."""
        cams = (_abi.LjCamera * len(cameras))()
        for i, c in enumerate(cameras):
            C.memmove(C.addressof(cams[i]), C.addressof(c), C.sizeof(_abi.LjCamera))
        out = np.zeros((len(cameras), self.hs.height, self.hs.width, spp, 3), np.float32)
        rc = self.lib.twin_views_render_samples(self.h, C.c_int(len(cameras)), cams, C.c_int(spp), C.c_int(0 if max_depth is None else max_depth),
                                                C.c_int(0 if max_depth is None else 1), C.c_uint64(seed), C.c_int(threads), out.ctypes.data_as(C.c_void_p))
        assert rc == 0
        return out
