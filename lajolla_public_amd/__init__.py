"""lajolla_public_amd — host-side mirror of lajolla's render interface over the MI355X (gfx950) hot path.

    hs    = parse_scene("scenes/cbox/cbox.xml")   # parse_scene(path, device)   src/parse_scene.h:9   (host, no GPU)
    ctx   = Context(device=0)                     # rtcNewDevice                src/main.cpp:30
    scene = Scene(ctx, hs)                        # Scene::Scene(...)           src/scene.cpp:3-53
    img   = render(scene)                         # Image3 render(const Scene&) src/render.h:9  -> (h, w, 3) float32

Everything goes through the C ABI of liblajolla_hip.so (include/lajolla_hip.h).  There is no CPU rendering path
in this package: if the library is missing, or no gfx950 device is present, the calls raise.
"""
import ctypes as C
import os
import sys

import numpy as np

from . import _abi
from ._abi import LjRenderArgs, LjSceneDesc, LjStats, LjSceneInfo, LjRay, LjHit, LjCamera, LjFeatureBuffers, LjFeatureStats
from ._abi import LJ_RNG_SAMPLE, LJ_RNG_TILE

_HERE = os.path.dirname(os.path.abspath(__file__))
# (LJ_VARIANT: a developer build of the same library with other compile flags, see build.py; unset in every shipped path)
LIB_PATH = os.path.join(_HERE, "liblajolla_hip" + ("_" + os.environ["LJ_VARIANT"] if os.environ.get("LJ_VARIANT") else "") + ".so")
_lib = None


class LajollaError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"[lj error {code}] {message}")
        self.code = code


def load_library():
    """dlopen liblajolla_hip.so and bind every symbol include/lajolla_hip.h declares.  No fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the HIP extension has not been built. Run `python -c 'import __graft_entry__ as g; "
            f"g.build()'` (or `python -m lajolla_public_amd.build`) from the repo root. There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, restype, argtypes in _abi.SYMBOLS:
        fn = getattr(lib, name)  # AttributeError here == the library does not export what the header declares
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


def _check(rc):
    if rc != _abi.LJ_OK:
        raise LajollaError(rc, load_library().lj_last_error().decode("utf-8", "replace"))


class HostScene:
    """Result of the XML front end: owns an LjSceneDesc (the constructor arguments of the reference's Scene)."""

    def __init__(self, handle):
        self._h = handle
        self.desc_ptr = load_library().lj_host_scene_desc(handle)
        self.desc = self.desc_ptr.contents

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.lj_host_scene_free(self._h)
            self._h = None

    # -- convenience views (copies) used by tests and tools
    @property
    def width(self):
        return self.desc.camera.width

    @property
    def height(self):
        return self.desc.camera.height

    @property
    def spp(self):
        return self.desc.options.samples_per_pixel

    def positions(self):
        n = self.desc.n_vertices
        return np.ctypeslib.as_array(self.desc.positions, shape=(n, 3)).copy() if n else np.zeros((0, 3))

    def normals(self):
        n = self.desc.n_vertices
        return np.ctypeslib.as_array(self.desc.normals, shape=(n, 3)).copy() if n else np.zeros((0, 3))

    def uvs(self):
        n = self.desc.n_vertices
        return np.ctypeslib.as_array(self.desc.uvs, shape=(n, 2)).copy() if n else np.zeros((0, 2))

    def positions_view(self):
        """The description's own position array, (n_vertices, 3) float64: writable and not a copy — what is written here is what
        Scene(ctx, hs) and Scene.update_geometry(hs) read.  Valid while this HostScene lives."""
        n = self.desc.n_vertices
        return np.ctypeslib.as_array(self.desc.positions, shape=(n, 3)) if n else np.zeros((0, 3))

    def normals_view(self):
        """The description's own normal array, as positions_view."""
        n = self.desc.n_vertices
        return np.ctypeslib.as_array(self.desc.normals, shape=(n, 3)) if n else np.zeros((0, 3))

    def indices(self):
        n = self.desc.n_triangles
        return np.ctypeslib.as_array(self.desc.indices, shape=(n, 3)).copy() if n else np.zeros((0, 3), np.int32)


def parse_scene(path):
    """Mitsuba-0.x XML -> HostScene.  Host only (no GPU needed).  Mirrors parse_scene() (parse_scene.cpp:1134-1149)."""
    lib = load_library()
    h = C.c_void_p()
    _check(lib.lj_parse_scene(os.fsencode(path), C.byref(h)))
    return HostScene(h)


def write_image(path, rgb):
    """imwrite() (image.cpp:135-173): `rgb` is (h, w, 3); .pfm in the reference's top-down layout, or .exr (HALF)."""
    a = np.ascontiguousarray(rgb, dtype=np.float32)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("write_image expects an (h, w, 3) array")
    _check(load_library().lj_image_write(os.fsencode(path), a.shape[1], a.shape[0], a.ctypes.data_as(C.c_void_p)))


def read_image(path, channels=3):
    """imread3 / imread1 (image.cpp:28-133): (h, w, channels) float32, y = 0 at the top."""
    lib = load_library()
    w, h, data = C.c_int32(), C.c_int32(), C.POINTER(C.c_float)()
    _check(lib.lj_image_read(os.fsencode(path), int(channels), C.byref(w), C.byref(h), C.byref(data)))
    try:
        return np.ctypeslib.as_array(data, shape=(h.value, w.value, int(channels))).copy()
    finally:
        lib.lj_image_free(data)


class Context:
    """One HIP device + stream + workspace."""

    def __init__(self, device=0):
        lib = load_library()
        self._h = C.c_void_p()
        self.device = int(device)
        self._scenes = 0        # live Scene objects on this context
        self._released = False  # __del__ has run while scenes were still alive: the last scene destroys the context
        _check(lib.lj_context_create(int(device), C.byref(self._h)))

    def _destroy(self):
        if getattr(self, "_h", None) and _lib is not None and not sys.is_finalizing():
            _lib.lj_context_destroy(self._h)
            self._h = None

    def __del__(self):
        # A scene keeps its context alive by reference, but when both die in one garbage-collected cycle (a failed test's
        # traceback holds them) Python may finalise the context first: it must then outlive the scenes at the C level.
        if getattr(self, "_scenes", 0) > 0:
            self._released = True
        else:
            self._destroy()


class Scene:
    """Device-resident scene: flattened BVH + sampling tables (the reference's Scene::Scene, scene.cpp:3-53)."""

    def __init__(self, ctx, host_scene_or_desc):
        lib = load_library()
        self._ctx = ctx  # keep the context alive
        self._h = C.c_void_p()
        desc_ptr = host_scene_or_desc.desc_ptr if isinstance(host_scene_or_desc, HostScene) else C.pointer(host_scene_or_desc)
        _check(lib.lj_scene_upload(ctx._h, desc_ptr, C.byref(self._h)))
        ctx._scenes += 1
        info = LjSceneInfo()
        _check(lib.lj_scene_info(self._h, C.byref(info)))
        self.info = info

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None and not sys.is_finalizing():
            _lib.lj_scene_destroy(self._h)
            self._h = None
            self._ctx._scenes -= 1
            if self._ctx._released and self._ctx._scenes == 0:
                self._ctx._destroy()

    def stats(self):
        st = LjStats()
        _check(load_library().lj_get_stats(self._h, C.byref(st)))
        return st

    def set_camera(self, cam):
        """Replace the scene's camera (an LjCamera, e.g. from look_at_camera) without rebuilding anything else; film size and
        filter may change.  Later renders and queries see the new camera."""
        lib = load_library()
        _check(lib.lj_scene_set_camera(self._h, C.byref(cam)))
        info = LjSceneInfo()
        _check(lib.lj_scene_info(self._h, C.byref(info)))
        self.info = info

    def update_geometry(self, host_scene_or_desc, rebuild=False):
        """The scene with its vertices moved: `host_scene_or_desc` is the uploaded description with other positions, normals or sphere
        positions / radii (HostScene.positions_view()); everything derived from them is re-derived and the BVHs are refitted on the device,
        nothing else is rebuilt (lj_scene_update_geometry).  Later renders and queries see the new geometry, bit-identical to a fresh
        Scene of the same description.  A refused update (LajollaError, LJ_ERR_INVALID_ARG) leaves the scene as it was.
        rebuild=True: rebuild_bvh() after the update; rebuild="lbvh" or "ploc": rebuild_bvh(builder=rebuild)."""
        lib = load_library()
        desc_ptr = host_scene_or_desc.desc_ptr if isinstance(host_scene_or_desc, HostScene) else C.pointer(host_scene_or_desc)
        if isinstance(rebuild, str):
            _builder_args(rebuild, None)   # (a misspelt builder is refused before the update)
        _check(lib.lj_scene_update_geometry(self._h, desc_ptr))
        if isinstance(rebuild, str):
            _check(lib.lj_scene_rebuild_bvh_ex(self._h, C.byref(_builder_args(rebuild, None))))
        elif rebuild:
            _check(lib.lj_scene_rebuild_bvh(self._h))
        info = LjSceneInfo()
        _check(lib.lj_scene_info(self._h, C.byref(info)))
        self.info = info

    def rebuild_bvh(self, builder="lbvh", radius=None):
        """Rebuild both trees on the device for the geometry as it stands there (lj_scene_rebuild_bvh_ex): builder="lbvh", a linear BVH in
        place of the refitted trees (lj_scene_rebuild_bvh itself), or "ploc", locally-ordered clustering with the given search radius (None:
        8; at most 32).  Hits and per-sample radiance do not change.  A leaf-scan scene (at most 32 leaves and 256 primitives) and an empty
        scene are left as they are (rebuild_stats(scene).rebuilt == 0).  LJ_TUNE_* are read again, as at upload."""
        lib = load_library()
        if builder == "lbvh" and radius is None:
            _check(lib.lj_scene_rebuild_bvh(self._h))
        else:
            _check(lib.lj_scene_rebuild_bvh_ex(self._h, C.byref(_builder_args(builder, radius))))
        info = LjSceneInfo()
        _check(lib.lj_scene_info(self._h, C.byref(info)))
        self.info = info


_BUILDERS = {"lbvh": _abi.LJ_BUILD_LBVH, "ploc": _abi.LJ_BUILD_PLOC}


def _builder_args(builder, radius):
    """LjRebuildArgs of a builder's name (or its LJ_BUILD_* number, handed on as it is) and a radius"""
    if isinstance(builder, str):
        if builder not in _BUILDERS:
            raise ValueError("builder must be one of %s, not %r" % (sorted(_BUILDERS), builder))
        builder = _BUILDERS[builder]
    return _abi.LjRebuildArgs(int(builder), 0 if radius is None else int(radius))


def read_bvh(scene, which):
    """An acceleration structure as it stands on the device, as a uint8 array: which = 0 the BVH4 (128-byte DNode4 records), 1 the BVH8
    (80-byte DNode8 records), 2 a tiny scene's leaf table (32-byte DScanLeaf records; empty for other scenes).  For tests."""
    lib = load_library()
    n = C.c_int64()
    _check(lib.lj_scene_read_bvh(scene._h, int(which), None, 0, C.byref(n)))
    out = np.zeros(n.value, np.uint8)
    if n.value:
        _check(lib.lj_scene_read_bvh(scene._h, int(which), out.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
    return out


def rebuild_stats(scene):
    """LjRebuildStats of the scene's last rebuild_bvh() (zeros before the first)."""
    st = _abi.LjRebuildStats()
    _check(load_library().lj_get_rebuild_stats(scene._h, C.byref(st)))
    return st


def build_stats(scene):
    """LjBuildStats of the scene's last rebuild_bvh(): the builder and radius that ran, its rounds of clustering (zeros before the first)."""
    st = _abi.LjBuildStats()
    _check(load_library().lj_get_build_stats(scene._h, C.byref(st)))
    return st


BINARY_NODE = np.dtype([("lo", np.float32, 3), ("hi", np.float32, 3), ("left", np.int32), ("right", np.int32), ("first", np.int32), ("count", np.int32)])


def bvh_build_query(ctx, boxes, builder="lbvh", radius=None):
    """The device's binary tree over boxes (n, 2, 3) float32 — lo, hi — (lj_bvh_build_query_ex, a test hook), by the linear builder or by
    "ploc" with its search radius: (order, nodes); order[i] is the box at position i of the leaves' order, nodes a BINARY_NODE array,
    breadth-first from the root."""
    boxes = np.ascontiguousarray(boxes, np.float32).reshape(-1, 2, 3)
    n = boxes.shape[0]
    order = np.zeros(n, np.int32)
    nodes = np.zeros(max(2 * n, 1), BINARY_NODE)
    got = C.c_int64()
    lib, ptr = load_library(), lambda a: a.ctypes.data_as(C.c_void_p)
    if builder == "lbvh" and radius is None:
        _check(lib.lj_bvh_build_query(ctx._h, n, ptr(boxes), ptr(order), ptr(nodes), nodes.size, C.byref(got)))
    else:
        _check(lib.lj_bvh_build_query_ex(ctx._h, C.byref(_builder_args(builder, radius)), n, ptr(boxes), ptr(order), ptr(nodes), nodes.size, C.byref(got)))
    return order, nodes[:got.value].copy()


def make_args(spp=0, max_depth=None, rank=0, world_size=1, crop=None, pool_paths=0, seed=0, flags=0, rng_mode=_abi.LJ_RNG_SAMPLE):
    """rng_mode: _abi.LJ_RNG_SAMPLE (one pcg32 stream per pixel sample, the default) or _abi.LJ_RNG_TILE (the reference's render()
    schedule: one stream per 16x16 tile, consumed in order — include/lajolla_hip.h)."""
    a = LjRenderArgs()
    a.spp = int(spp)
    a.max_depth = _abi.INT32_MIN if max_depth is None else int(max_depth)
    a.rng_mode = int(rng_mode)
    a.rank, a.world_size = int(rank), int(world_size)
    if crop is not None:
        a.crop_x0, a.crop_y0, a.crop_x1, a.crop_y1 = [int(v) for v in crop]
    a.pool_paths = int(pool_paths)
    a.flags = int(flags)
    a.seed = int(seed)
    return a


def render(scene, **kw):
    """Image3 render(const Scene&) (render.h:9): returns (h, w, 3) float32 radiance, y = 0 at the top."""
    args = make_args(**kw)
    out = np.empty((scene.info.height, scene.info.width, 3), np.float32)
    _check(load_library().lj_render(scene._h, C.byref(args), out.ctypes.data_as(C.c_void_p)))
    return out


def render_device(scene, device_ptr, stream=None, **kw):
    """Same, into caller-owned device memory (e.g. a torch tensor's data_ptr()) on a HIP stream; asynchronous."""
    args = make_args(**kw)
    _check(load_library().lj_render_device(scene._h, C.byref(args), C.c_void_p(int(device_ptr)), C.c_void_p(int(stream or 0))))


def look_at_camera(origin, target, up, fov, width, height, filter_kind=_abi.LJ_FILTER_BOX, filter_param=1.0, medium_id=-1):
    """The LjCamera the XML front end builds for a perspective sensor with a <lookat> transform: fov in degrees along x."""
    d3 = C.c_double * 3
    cam = LjCamera()
    _check(load_library().lj_camera_look_at(d3(*[float(v) for v in origin]), d3(*[float(v) for v in target]), d3(*[float(v) for v in up]),
                                            float(fov), int(width), int(height), int(filter_kind), float(filter_param), C.byref(cam)))
    cam.medium_id = int(medium_id)
    return cam


def _camera_array(cameras):
    arr = (LjCamera * len(cameras))()
    for i, c in enumerate(cameras):
        C.memmove(C.addressof(arr[i]), C.addressof(c), C.sizeof(LjCamera))
    return arr


def render_views(scene, cameras, **kw):
    """Many cameras of one uploaded scene in one pass: (n, h, w, 3) float32.  `cameras`: a sequence of LjCamera with the scene camera's film,
    filter and medium.  View v is bit-identical to render() of the scene uploaded with cameras[v] and the same arguments."""
    args = make_args(**kw)
    cams = _camera_array(cameras)
    out = np.empty((len(cameras), scene.info.height, scene.info.width, 3), np.float32)
    _check(load_library().lj_render_views(scene._h, C.byref(args), len(cameras), cams, out.ctypes.data_as(C.c_void_p)))
    return out


def render_views_device(scene, cameras, device_ptr, stream=None, **kw):
    """Same, into caller-owned device memory of n * h * w * 3 floats (e.g. a torch tensor's data_ptr()), ordered on a HIP stream as render_device."""
    args = make_args(**kw)
    cams = _camera_array(cameras)
    _check(load_library().lj_render_views_device(scene._h, C.byref(args), len(cameras), cams, C.c_void_p(int(device_ptr)), C.c_void_p(int(stream or 0))))


FEATURES = ("albedo", "normal", "depth", "alpha", "variance")


def _feature_names(features):
    names = [features] if isinstance(features, str) else list(features)
    for f in names:
        if f not in FEATURES:
            raise ValueError(f"unknown feature {f!r}: expected some of {FEATURES}")
    if len(set(names)) != len(names):
        raise ValueError("a feature is named twice")
    return names


def render_features(scene, cameras=None, features=FEATURES, **kw):
    """render() / render_views() and, from the same camera samples, the first-hit guide buffers and the variance of the image
    (lj_render_features): a dict of float32 arrays — "rgb" always, and each of `features` ("albedo", "normal", "depth", "alpha", "variance").
    (h, w, 3) arrays, (h, w) for depth and alpha; with a camera list (n, h, w, 3) and (n, h, w).  "rgb" is bit-identical to render()."""
    names = _feature_names(features)
    if cameras is not None and len(cameras) == 0:
        raise ValueError("render_features: an empty camera list (pass cameras=None for the scene's own camera)")
    args = make_args(**kw)
    lead = (scene.info.height, scene.info.width) if cameras is None else (len(cameras), scene.info.height, scene.info.width)
    out = {}
    bufs = LjFeatureBuffers()
    for name in ["rgb"] + names:
        c = _abi.FEATURE_CHANNELS[name]
        out[name] = np.empty(lead + ((c,) if c > 1 else ()), np.float32)
        setattr(bufs, name, out[name].ctypes.data)
    cams = _camera_array(cameras) if cameras is not None else None
    _check(load_library().lj_render_features(scene._h, C.byref(args), 0 if cameras is None else len(cameras), cams, C.byref(bufs)))
    return out


def render_features_device(scene, buffers, cameras=None, stream=None, **kw):
    """Same, into caller-owned device memory, ordered on a HIP stream as render_device: `buffers` maps "rgb" / "albedo" / "normal" / "depth" /
    "alpha" / "variance" to device pointers (e.g. a torch tensor's data_ptr()) of n * h * w * channels floats; a name left out is not computed."""
    bufs = LjFeatureBuffers()
    for name, ptr in buffers.items():
        if name not in _abi.FEATURE_CHANNELS:
            raise ValueError(f"unknown buffer {name!r}: expected some of {tuple(_abi.FEATURE_CHANNELS)}")
        setattr(bufs, name, int(ptr) if ptr else None)
    if cameras is not None and len(cameras) == 0:
        raise ValueError("render_features_device: an empty camera list (pass cameras=None for the scene's own camera)")
    args = make_args(**kw)
    cams = _camera_array(cameras) if cameras is not None else None
    _check(load_library().lj_render_features_device(scene._h, C.byref(args), 0 if cameras is None else len(cameras), cams, C.byref(bufs), C.c_void_p(int(stream or 0))))


def feature_stats(scene):
    """LjFeatureStats of the scene's last render_features* call (zeros after any other render)."""
    st = LjFeatureStats()
    _check(load_library().lj_get_feature_stats(scene._h, C.byref(st)))
    return st


DENOISE_SIGMAS = ("sigma_color", "sigma_normal", "sigma_depth", "sigma_albedo")
_default_ctx = None


def make_denoise_args(iterations=0, demodulate=False, **sigmas):
    """LjDenoiseArgs: iterations (<= 0: the default 5, at most 8), demodulate, and sigma_color / sigma_normal / sigma_depth / sigma_albedo (0: the default)."""
    for k in sigmas:
        if k not in DENOISE_SIGMAS:
            raise ValueError(f"unknown argument {k!r}: expected some of {DENOISE_SIGMAS}")
    if int(iterations) > 8:
        raise ValueError("denoise: at most 8 iterations")
    a = _abi.LjDenoiseArgs()
    a.iterations = max(int(iterations), 0)
    a.flags = _abi.LJ_DENOISE_DEMODULATE if demodulate else 0
    for k, v in sigmas.items():
        if not (np.isfinite(v) and v >= 0):
            raise ValueError(f"denoise: {k} must be finite and not negative")
        setattr(a, k, float(v))
    return a


def _denoise_buffers(buffers, demodulate):
    for name in buffers:
        if name not in _abi.FEATURE_CHANNELS:
            raise ValueError(f"unknown buffer {name!r}: expected some of {tuple(_abi.FEATURE_CHANNELS)}")
    if buffers.get("rgb") is None:
        raise ValueError("denoise: the buffers must hold \"rgb\"")
    if demodulate and buffers.get("albedo") is None:
        raise ValueError("denoise: demodulate=True needs the \"albedo\" buffer (pass demodulate=False to filter rgb itself)")


def denoise(buffers, ctx=None, iterations=0, demodulate=True, **sigmas):
    """The edge-stopping a-trous filter of lj_denoise over the dict render_features returns — one image, (h, w, 3), or a batch, (n, h, w, 3) —
    with whichever of "variance", "albedo", "normal" and "depth" it holds ("alpha" is not read): {"rgb": the filtered image, "variance": the
    filtered variance or None without a variance buffer}.  demodulate: filter rgb / (albedo + 1e-3) and multiply back (needs "albedo").
    sigma_color / sigma_normal / sigma_depth / sigma_albedo and iterations: 0 for the defaults (4, 0.5, 0.1, 0.25; 5).  Inputs must be finite.
    ctx: the Context to run on (None: one on device 0, created at the first such call and kept)."""
    global _default_ctx
    _denoise_buffers(buffers, demodulate)
    args = make_denoise_args(iterations, demodulate, **sigmas)
    rgb = np.ascontiguousarray(buffers["rgb"], np.float32)
    if rgb.ndim not in (3, 4) or rgb.shape[-1] != 3 or 0 in rgb.shape:
        raise ValueError("denoise: \"rgb\" must be (h, w, 3) or (n, h, w, 3) and not empty")
    lead = rgb.shape[:-1]
    n, (h, w) = (1 if rgb.ndim == 3 else lead[0]), lead[-2:]
    bufs, keep = LjFeatureBuffers(), [rgb]
    bufs.rgb = rgb.ctypes.data
    for name in ("variance", "albedo", "normal", "depth"):
        if buffers.get(name) is None:
            continue
        a = np.ascontiguousarray(buffers[name], np.float32)
        c = _abi.FEATURE_CHANNELS[name]
        if a.shape != lead + ((c,) if c > 1 else ()):
            raise ValueError(f"denoise: {name!r} has shape {a.shape}, which does not go with rgb's {rgb.shape}")
        keep.append(a)
        setattr(bufs, name, a.ctypes.data)
    if ctx is None:
        if _default_ctx is None:
            _default_ctx = Context(0)
        ctx = _default_ctx
    out = {"rgb": np.empty(rgb.shape, np.float32), "variance": np.empty(rgb.shape, np.float32) if bufs.variance else None}
    _check(load_library().lj_denoise(ctx._h, n, w, h, C.byref(bufs), C.byref(args), out["rgb"].ctypes.data_as(C.c_void_p),
                                     out["variance"].ctypes.data_as(C.c_void_p) if bufs.variance else None))
    return out


def denoise_device(ctx, buffers, n, width, height, rgb_out, variance_out=None, stream=None, iterations=0, demodulate=True, **sigmas):
    """Same on device memory of ctx's device, ordered on a HIP stream as render_device: `buffers` maps "rgb" and any of "variance", "albedo",
    "normal", "depth" to device pointers of n * height * width * channels floats (what render_features_device filled); rgb_out (may be
    buffers["rgb"]) and variance_out (optional; needs "variance") are device pointers of n * height * width * 3 floats.  Asynchronous."""
    _denoise_buffers(buffers, demodulate)
    if variance_out and not buffers.get("variance"):
        raise ValueError("denoise_device: variance_out needs the \"variance\" buffer")
    if not rgb_out:
        raise ValueError("denoise_device: no rgb_out")
    args = make_denoise_args(iterations, demodulate, **sigmas)
    bufs = LjFeatureBuffers()
    for name, ptr in buffers.items():
        setattr(bufs, name, int(ptr) if ptr else None)
    _check(load_library().lj_denoise_device(ctx._h, int(n), int(width), int(height), C.byref(bufs), C.byref(args), C.c_void_p(int(rgb_out)),
                                            C.c_void_p(int(variance_out)) if variance_out else None, C.c_void_p(int(stream or 0))))


def render_denoised(scene, cameras=None, iterations=0, demodulate=True, sigmas=None, **kw):
    """render_features_device and denoise_device back to back on the scene's device, no host copy in between: {"rgb", "variance"} as
    denoise() returns them, bit-identical to denoise(render_features(scene, cameras, **kw)).  Device memory comes from torch.
    sigmas: a dict of sigma_* values; **kw: the render's arguments (spp, seed, ...)."""
    import torch
    if cameras is not None and len(cameras) == 0:
        raise ValueError("render_denoised: an empty camera list (pass cameras=None for the scene's own camera)")
    make_denoise_args(iterations, demodulate, **(sigmas or {}))
    n = 1 if cameras is None else len(cameras)
    h, w = scene.info.height, scene.info.width
    with torch.cuda.device(scene._ctx.device):
        stream = torch.cuda.current_stream()
        names = ("rgb",) + FEATURES
        t = {k: torch.empty((n, h, w) + ((3,) if _abi.FEATURE_CHANNELS[k] == 3 else ()), device="cuda", dtype=torch.float32) for k in names}
        out_var = torch.empty((n, h, w, 3), device="cuda", dtype=torch.float32)
        render_features_device(scene, {k: t[k].data_ptr() for k in names}, cameras=cameras, stream=stream.cuda_stream, **kw)
        denoise_device(scene._ctx, {k: t[k].data_ptr() for k in names}, n, w, h, t["rgb"].data_ptr(), out_var.data_ptr(), stream=stream.cuda_stream,
                       iterations=iterations, demodulate=demodulate, **(sigmas or {}))
        rgb, var = t["rgb"].cpu().numpy(), out_var.cpu().numpy()
    return {"rgb": rgb if cameras is not None else rgb[0], "variance": var if cameras is not None else var[0]}


def denoise_stats(ctx):
    """LjDenoiseStats of the context's last denoise* call: device time of its launches (waits for them), their number, the pixel count."""
    st = _abi.LjDenoiseStats()
    _check(load_library().lj_get_denoise_stats(ctx._h, C.byref(st)))
    return st


ADAPTIVE_GUIDES = ("albedo", "normal", "depth", "alpha")


def make_adaptive_args(min_spp=0, max_spp=0, round_spp=0, target_error=0.0, max_rounds=0):
    """LjAdaptiveArgs: 0 (or less) for a default — min_spp 16, max_spp 16 * min_spp, round_spp min_spp, target_error 0.05, max_rounds 16."""
    a = _abi.LjAdaptiveArgs()
    a.min_spp, a.max_spp, a.round_spp, a.max_rounds = int(min_spp), int(max_spp), int(round_spp), int(max_rounds)
    a.target_error = float(target_error)
    return a


def render_adaptive(scene, min_spp=0, max_spp=0, round_spp=0, target_error=0.0, max_rounds=0, guides=False, **kw):
    """Variance-driven sampling in rounds (lj_render_adaptive): every pixel gets min_spp samples, then the pixels whose relative error still
    exceeds target_error get round_spp more per round, up to max_spp and max_rounds.  A dict: "rgb" (h, w, 3) float32, "variance" (h, w, 3)
    float32 — the squared standard error of rgb — and "samples" (h, w) uint32; with guides=True also "albedo", "normal", "depth" and "alpha"
    of round 0, so that the dict can go to denoise() as it is.  **kw: seed, max_depth, rank / world_size, crop, pool_paths, flags as for
    render(); spp is ignored."""
    args = make_args(**kw)
    aargs = make_adaptive_args(min_spp, max_spp, round_spp, target_error, max_rounds)
    lead = (scene.info.height, scene.info.width)
    out, bufs = {}, _abi.LjAdaptiveBuffers()
    for name in ("rgb", "variance", "samples") + (ADAPTIVE_GUIDES if guides else ()):
        c, dtype = _abi.ADAPTIVE_BUFFERS[name]
        out[name] = np.empty(lead + ((c,) if c > 1 else ()), dtype)
        setattr(bufs, name, out[name].ctypes.data)
    _check(load_library().lj_render_adaptive(scene._h, C.byref(args), C.byref(aargs), C.byref(bufs)))
    return out


def render_adaptive_device(scene, buffers, stream=None, min_spp=0, max_spp=0, round_spp=0, target_error=0.0, max_rounds=0, **kw):
    """Same, into caller-owned device memory, ordered on a HIP stream as render_device: `buffers` maps "rgb" / "variance" / "samples" (uint32) /
    "albedo" / "normal" / "depth" / "alpha" to device pointers of h * w * channels elements; a name left out is not written."""
    bufs = _abi.LjAdaptiveBuffers()
    for name, ptr in buffers.items():
        if name not in _abi.ADAPTIVE_BUFFERS:
            raise ValueError(f"unknown buffer {name!r}: expected some of {tuple(_abi.ADAPTIVE_BUFFERS)}")
        setattr(bufs, name, int(ptr) if ptr else None)
    args = make_args(**kw)
    aargs = make_adaptive_args(min_spp, max_spp, round_spp, target_error, max_rounds)
    _check(load_library().lj_render_adaptive_device(scene._h, C.byref(args), C.byref(aargs), C.byref(bufs), C.c_void_p(int(stream or 0))))


def adaptive_stats(scene):
    """LjAdaptiveStats of the scene's last render_adaptive* call (zeros after any other render)."""
    st = _abi.LjAdaptiveStats()
    _check(load_library().lj_get_adaptive_stats(scene._h, C.byref(st)))
    return st


def adaptive_select(ctx, n, mean, m2, pixel_list=None, **adaptive):
    """The selection of one round on given state (lj_adaptive_select_query, a test hook): n (h, w) uint32, mean and m2 (h, w, 3) float32,
    pixel_list: film pixel indices in the order to keep (None: row-major, the whole film).  Returns the selected list, uint32.
    **adaptive: min_spp, max_spp, round_spp, target_error, max_rounds."""
    n = np.ascontiguousarray(n, np.uint32)
    if n.ndim != 2:
        raise ValueError("adaptive_select: n must be (h, w)")
    h, w = n.shape
    mean, m2 = np.ascontiguousarray(mean, np.float32), np.ascontiguousarray(m2, np.float32)
    if mean.shape != (h, w, 3) or m2.shape != (h, w, 3):
        raise ValueError("adaptive_select: mean and m2 must be (h, w, 3)")
    lst = np.arange(h * w, dtype=np.uint32) if pixel_list is None else np.ascontiguousarray(pixel_list, np.uint32).reshape(-1)
    out, got = np.empty(max(lst.size, 1), np.uint32), C.c_int64()
    aargs = make_adaptive_args(**adaptive)
    _check(load_library().lj_adaptive_select_query(ctx._h, w, h, _vp(n), _vp(mean), _vp(m2), C.byref(aargs), _vp(lst), lst.size, _vp(out), C.byref(got)))
    return out[:got.value].copy()


def render_samples(scene, crop, **kw):
    """Per-sample radiance over a crop window: (crop_h, crop_w, spp, 3) float32 — one path_tracing() value each."""
    args = make_args(crop=crop, **kw)
    spp = args.spp if args.spp > 0 else scene.info.spp
    x0, y0, x1, y1 = crop
    out = np.empty((y1 - y0, x1 - x0, spp, 3), np.float32)
    _check(load_library().lj_render_samples(scene._h, C.byref(args), out.ctypes.data_as(C.c_void_p)))
    return out


def make_rays_args(medium_id=None, ray_spread=None):
    """LjRaysArgs, or None when both are left to their defaults (the scene camera's medium and spread)."""
    if medium_id is None and ray_spread is None:
        return None
    a = _abi.LjRaysArgs()
    if medium_id is not None:
        a.medium_id, a.flags = int(medium_id), a.flags | _abi.LJ_RAYS_HAS_MEDIUM
    if ray_spread is not None:
        a.ray_spread, a.flags = float(ray_spread), a.flags | _abi.LJ_RAYS_HAS_SPREAD
    return a


def _ray_table(a, b, what):
    a, b = np.asarray(a, np.float32).reshape(-1, 3), np.asarray(b, np.float32).reshape(-1, 3)
    if a.shape != b.shape:
        raise ValueError(f"{what}: the two arrays must hold as many vectors")
    return np.ascontiguousarray(np.concatenate([a, b], axis=1))   # (n, 6): LjRadianceRay / LjProbe


def _radiance_call(fn, scene, table, spp, variance, samples, medium_id, ray_spread, kw):
    args = make_args(spp=spp, **kw)
    k = args.spp if args.spp > 0 else scene.info.spp
    n = table.shape[0]
    out, bufs = {"radiance": np.empty((n, 3), np.float32)}, _abi.LjRadianceBuffers()
    if variance:
        out["variance"] = np.empty((n, 3), np.float32)
    if samples:
        out["samples"] = np.empty((n, max(k, 0), 3), np.float32)
    for name, a in out.items():
        setattr(bufs, name, a.ctypes.data)
    ra = make_rays_args(medium_id, ray_spread)
    _check(fn(scene._h, C.byref(args), C.byref(ra) if ra is not None else None, n, _vp(table), C.byref(bufs)))
    return out


def radiance_rays(scene, org, dir, spp=0, variance=False, samples=False, medium_id=None, ray_spread=None, **render_kw):
    """Path-traced radiance along given rays (lj_radiance_rays): org, dir (n, 3), dir of unit length.  A dict: "radiance" (n, 3) float32, the
    mean over spp samples per ray; with variance=True "variance" (n, 3), its squared standard error; with samples=True "samples" (n, spp, 3).
    Ray i, sample s draws from pcg32 stream i * spp + s (its first two draws are discarded, as a camera sample spends them on its jitter).
    medium_id (volpath): the medium the origins lie in, None: the camera's; ray_spread (path): spread of the first segment, None: the camera's.
    **render_kw: max_depth, seed, pool_paths, flags as for render()."""
    return _radiance_call(load_library().lj_radiance_rays, scene, _ray_table(org, dir, "radiance_rays"), spp, variance, samples, medium_id, ray_spread, render_kw)


def irradiance(scene, positions, normals, spp=0, variance=False, samples=False, medium_id=None, ray_spread=None, **render_kw):
    """Irradiance at surface points (lj_irradiance): positions, normals (n, 3), normals of unit length.  Per probe, spp cosine-distributed
    directions about the normal from the point offset by the scene's shadow epsilon; "radiance" is pi times the mean of the radiance along
    them, "variance" pi^2 times its squared standard error, "samples" the radiance values themselves.  Arguments as radiance_rays()."""
    return _radiance_call(load_library().lj_irradiance, scene, _ray_table(positions, normals, "irradiance"), spp, variance, samples, medium_id, ray_spread, render_kw)


def probe_rays(scene, positions, normals, spp, seed=0):
    """The rays irradiance() traces (lj_probe_ray_queries, a test hook): (org, dir), each (n, spp, 3) float32."""
    table = _ray_table(positions, normals, "probe_rays")
    args = make_args(spp=spp, seed=seed)
    k = args.spp if args.spp > 0 else scene.info.spp
    out = np.empty((table.shape[0], max(k, 0), 6), np.float32)
    _check(load_library().lj_probe_ray_queries(scene._h, C.byref(args), table.shape[0], _vp(table), _vp(out)))
    return out[..., :3].copy(), out[..., 3:].copy()


def _rays_array(org, dir, tnear, tfar):
    org = np.asarray(org, np.float32).reshape(-1, 3)
    n = org.shape[0]
    rays = np.zeros(n, dtype=np.dtype([("org", np.float32, 3), ("tnear", np.float32), ("dir", np.float32, 3), ("tfar", np.float32)]))
    rays["org"] = org
    rays["dir"] = np.asarray(dir, np.float32).reshape(-1, 3)
    rays["tnear"] = tnear
    rays["tfar"] = tfar
    return rays


HIT_DTYPE = np.dtype([("t", np.float32), ("u", np.float32), ("v", np.float32), ("shape_id", np.int32), ("prim_id", np.int32)])


def intersect(scene, org, dir, tnear=0.0, tfar=np.inf):
    """Batched intersect() (intersection.cpp:7-65, hit record only) on the device BVH."""
    rays = _rays_array(org, dir, tnear, tfar)
    hits = np.zeros(rays.shape[0], HIT_DTYPE)
    _check(load_library().lj_intersect(scene._h, rays.shape[0], rays.ctypes.data_as(C.c_void_p), hits.ctypes.data_as(C.c_void_p)))
    return hits


def occluded(scene, org, dir, tnear=0.0, tfar=np.inf):
    """Batched occluded() (intersection.cpp:67-85) on the device BVH."""
    rays = _rays_array(org, dir, tnear, tfar)
    occ = np.zeros(rays.shape[0], np.uint8)
    _check(load_library().lj_occluded(scene._h, rays.shape[0], rays.ctypes.data_as(C.c_void_p), occ.ctypes.data_as(C.c_void_p)))
    return occ.astype(bool)


# ------------------------------------------------------------------ per-object queries on the device (lajolla_hip.h)
# numpy structured arrays with the C structs' layouts in, the same out.  One query per GPU lane, answered by the device
# functions the shade kernels are built from; there is no host arithmetic behind any of these.
BSDF_QUERY, BSDF_RESULT = np.dtype(_abi.LjBsdfQuery), np.dtype(_abi.LjBsdfResult)
LIGHT_QUERY, LIGHT_RESULT = np.dtype(_abi.LjLightQuery), np.dtype(_abi.LjLightResult)
HIT_QUERY, HIT_RESULT = np.dtype(_abi.LjHitQuery), np.dtype(_abi.LjHitResult)
PRIMARY_QUERY, PRIMARY_RESULT = np.dtype(_abi.LjPrimaryQuery), np.dtype(_abi.LjPrimaryResult)
FILTER_QUERY = np.dtype(_abi.LjFilterQuery)
TEXTURE_QUERY = np.dtype(_abi.LjTextureQuery)
FRAME_QUERY, FRAME_RESULT = np.dtype(_abi.LjFrameQuery), np.dtype(_abi.LjFrameResult)
PHASE_QUERY, PHASE_RESULT = np.dtype(_abi.LjPhaseQuery), np.dtype(_abi.LjPhaseResult)
MEDIUM_QUERY, MEDIUM_RESULT = np.dtype(_abi.LjMediumQuery), np.dtype(_abi.LjMediumResult)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _q(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return a.reshape(-1)


def shade_variant_count():
    return load_library().lj_shade_variant_count()


def scene_shade_variant(scene):
    return load_library().lj_scene_shade_variant(scene._h)


def bsdf_queries(scene, queries, variant=-1):
    """eval / pdf_sample_bsdf / sample_bsdf (material.h:126,147,161) of the device BSDF code, per query."""
    q = _q(queries, BSDF_QUERY)
    r = np.zeros(q.shape[0], BSDF_RESULT)
    _check(load_library().lj_bsdf_queries(scene._h, int(variant), q.shape[0], _vp(q), _vp(r)))
    return r


def light_queries(scene, queries, variant=-1):
    """sample_point_on_light / pdf_point_on_light / emission (light.h:46-67) + light_pmf, per query."""
    q = _q(queries, LIGHT_QUERY)
    r = np.zeros(q.shape[0], LIGHT_RESULT)
    _check(load_library().lj_light_queries(scene._h, int(variant), q.shape[0], _vp(q), _vp(r)))
    return r


def sample_light_queries(scene, u):
    u = np.ascontiguousarray(u, np.float32).reshape(-1)
    ids = np.zeros(u.shape[0], np.int32)
    _check(load_library().lj_sample_light_queries(scene._h, u.shape[0], _vp(u), _vp(ids)))
    return ids


def vertex_queries(scene, queries, variant=-1):
    """compute_shading_info + PathVertex assembly (intersection.cpp:38-62) for given hit records."""
    q = _q(queries, HIT_QUERY)
    r = np.zeros(q.shape[0], HIT_RESULT)
    _check(load_library().lj_vertex_queries(scene._h, int(variant), q.shape[0], _vp(q), _vp(r)))
    return r


def primary_ray_queries(scene, queries):
    q = _q(queries, PRIMARY_QUERY)
    r = np.zeros(q.shape[0], PRIMARY_RESULT)
    _check(load_library().lj_primary_ray_queries(scene._h, q.shape[0], _vp(q), _vp(r)))
    return r


def filter_queries(ctx, queries):
    q = _q(queries, FILTER_QUERY)
    r = np.zeros((q.shape[0], 2), np.float32)
    _check(load_library().lj_filter_queries(ctx._h, q.shape[0], _vp(q), _vp(r)))
    return r


def pcg32_queries(ctx, stream_ids, count, seed=0, reals=True):
    s = np.ascontiguousarray(stream_ids, np.uint64).reshape(-1)
    u = np.zeros((s.shape[0], count), np.uint32)
    f = np.zeros((s.shape[0], count), np.float32) if reals else None
    _check(load_library().lj_pcg32_queries(ctx._h, s.shape[0], _vp(s), int(seed), int(count), _vp(u), _vp(f) if reals else None))
    return u, f


def texture_queries(scene, queries):
    q = _q(queries, TEXTURE_QUERY)
    r = np.zeros((q.shape[0], 3), np.float32)
    _check(load_library().lj_texture_queries(scene._h, q.shape[0], _vp(q), _vp(r)))
    return r


def frame_queries(ctx, queries):
    q = _q(queries, FRAME_QUERY)
    r = np.zeros(q.shape[0], FRAME_RESULT)
    _check(load_library().lj_frame_queries(ctx._h, q.shape[0], _vp(q), _vp(r)))
    return r


def phase_queries(ctx, queries):
    """eval (== pdf_sample_phase) and sample_phase_function of the device phase-function code (dvol.h), per query."""
    q = _q(queries, PHASE_QUERY)
    r = np.zeros(q.shape[0], PHASE_RESULT)
    _check(load_library().lj_phase_queries(ctx._h, q.shape[0], _vp(q), _vp(r)))
    return r


def medium_queries(scene, queries):
    """get_sigma_s / get_sigma_a at a point and get_majorant along a ray of the device medium code (dvol.h), per query."""
    q = _q(queries, MEDIUM_QUERY)
    r = np.zeros(q.shape[0], MEDIUM_RESULT)
    _check(load_library().lj_medium_queries(scene._h, q.shape[0], _vp(q), _vp(r)))
    return r


# ------------------------------------------------------------------ device groups: one process, N devices (lajolla_hip.h)
class DeviceGroup:
    """N devices driven from this process; RCCL communicator inside when they are distinct and N >= 2."""

    def __init__(self, device_ids):
        ids = (C.c_int * len(device_ids))(*[int(d) for d in device_ids])
        self._h = C.c_void_p()
        self._scenes = 0
        self._released = False
        _check(load_library().lj_group_create(len(device_ids), ids, C.byref(self._h)))
        self.size = load_library().lj_group_size(self._h)
        self.uses_rccl = bool(load_library().lj_group_uses_rccl(self._h))

    def _destroy(self):
        if getattr(self, "_h", None) and _lib is not None and not sys.is_finalizing():
            _lib.lj_group_destroy(self._h)
            self._h = None

    def __del__(self):
        if getattr(self, "_scenes", 0) > 0:
            self._released = True
        else:
            self._destroy()


class GroupScene:
    """The scene on every device of a group."""

    def __init__(self, group, host_scene_or_desc):
        self._group = group
        self._h = C.c_void_p()
        desc_ptr = host_scene_or_desc.desc_ptr if isinstance(host_scene_or_desc, HostScene) else C.pointer(host_scene_or_desc)
        _check(load_library().lj_group_scene_upload(group._h, desc_ptr, C.byref(self._h)))
        group._scenes += 1
        info = LjSceneInfo()
        _check(load_library().lj_scene_info(load_library().lj_group_scene_member(self._h, 0), C.byref(info)))
        self.info = info

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None and not sys.is_finalizing():
            _lib.lj_group_scene_destroy(self._h)
            self._h = None
            self._group._scenes -= 1
            if self._group._released and self._group._scenes == 0:
                self._group._destroy()

    def stats(self):
        st = LjStats()
        _check(load_library().lj_group_get_stats(self._h, C.byref(st)))
        return st


def render_group(group_scene, **kw):
    """render() across a device group: tiles sharded t % N, one sum-reduce onto device 0 -> (h, w, 3) float32."""
    args = make_args(**kw)
    out = np.empty((group_scene.info.height, group_scene.info.width, 3), np.float32)
    _check(load_library().lj_group_render(group_scene._h, C.byref(args), out.ctypes.data_as(C.c_void_p)))
    return out
