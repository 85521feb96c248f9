"""Shared by tests/test_refit_cpu.py and tests/test_gpu_refit.py: the scenes and motions of the geometry-update tests,
the host twin of lj_scene_update_geometry (tests/twin_refit), and numpy layouts of the three acceleration structures.  Not a test module."""
import ctypes as C
import os

import numpy as np

import lajolla_public_amd as lj
from lajolla_public_amd import _abi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# device/dtypes.h
NODE4 = np.dtype([("lo", np.float32, (3, 4)), ("hi", np.float32, (3, 4)), ("child", np.int32, 4), ("pad", np.int32, 4)])
NODE8 = np.dtype([("p", np.float32, 3), ("e", np.uint8, 3), ("imask", np.uint8), ("child_base", np.uint32), ("prim_base", np.uint32), ("meta", np.uint8, 8),
                  ("qlo", np.uint8, (3, 8)), ("qhi", np.uint8, (3, 8))])
SCAN_LEAF = np.dtype([("c", np.float32, 3), ("h", np.float32, 3), ("first", np.int32), ("count", np.int32)])
PRIM = np.dtype([("v0", np.float32, 3), ("gprim", np.int32), ("v1", np.float32, 3), ("kind", np.int32), ("v2", np.float32, 3), ("sphere_slot", np.int32)])
assert NODE4.itemsize == 128 and NODE8.itemsize == 80 and SCAN_LEAF.itemsize == 32 and PRIM.itemsize == 48
TABLES = {"prims": 3, "spheres": 4, "light_tris": 5, "light_tri_cdf": 6, "lights": 7, "light_cdf": 8, "leaf_prims": 9}

_lib = None


def refit_lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build.build_twin_refit(verbose=False))
        _lib.refit_create.restype = C.c_void_p
        _lib.refit_create.argtypes = [C.POINTER(_abi.LjSceneDesc), C.c_char_p, C.c_int]
        _lib.refit_free.argtypes = [C.c_void_p]
        _lib.refit_update.argtypes = [C.c_void_p, C.POINTER(_abi.LjSceneDesc), C.c_char_p, C.c_int]
        _lib.refit_read.restype = C.c_int64
        _lib.refit_read.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64]
        _lib.refit_bounds.argtypes = [C.c_void_p, C.c_void_p]
        _lib.refit_trace.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.refit_prim_boxes.argtypes = [C.c_void_p, C.c_void_p]
        _lib.refit_grid_exponents.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    return _lib


class RefitTwin:
    """flatten_scene of a description on the host, then lj_scene_update_geometry as the host twin runs it."""

    def __init__(self, hs):
        self.hs, self.lib = hs, refit_lib()
        err = C.create_string_buffer(512)
        self.h = C.c_void_p(self.lib.refit_create(hs.desc_ptr, err, 512))
        if not self.h:
            raise RuntimeError(err.value.decode())

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.refit_free(self.h)
            self.h = None

    def update(self, hs):
        """0, or the LJ_ERR_* code of a refused update; the message in self.error"""
        err = C.create_string_buffer(512)
        rc = self.lib.refit_update(self.h, hs.desc_ptr, err, 512)
        self.error = err.value.decode()
        return rc

    def read(self, which):
        n = self.lib.refit_read(self.h, which, None, 0)
        out = np.zeros(n, np.uint8)
        if n:
            self.lib.refit_read(self.h, which, out.ctypes.data_as(C.c_void_p), n)
        return out

    def structures(self):
        return [self.read(w) for w in (0, 1, 2)]

    def table(self, name):
        return self.read(TABLES[name])

    def leaf_order(self):
        return self.read(10).view(np.int32)

    def levels(self, tree):
        return self.read(11 if tree == 4 else 13).view(np.int32), self.read(12 if tree == 4 else 14).view(np.int32)

    def bounds(self):
        out = np.zeros(6)
        self.lib.refit_bounds(self.h, out.ctypes.data_as(C.c_void_p))
        return dict(center=out[:3].copy(), radius=out[3], shadow_epsilon=out[4], n_scan_used=int(out[5]))

    def prim_boxes(self):
        n = len(self.read(9)) // PRIM.itemsize
        out = np.zeros((n, 2, 3), np.float32)
        self.lib.refit_prim_boxes(self.h, out.ctypes.data_as(C.c_void_p))
        return out

    def intersect(self, tree, rays):
        hits = np.zeros(rays.shape[0], lj.HIT_DTYPE)
        assert self.lib.refit_trace(self.h, tree, rays.shape[0], rays.ctypes.data_as(C.c_void_p), hits.ctypes.data_as(C.c_void_p), None) == 0
        return hits

    def occluded(self, tree, rays):
        occ = np.zeros(rays.shape[0], np.uint8)
        assert self.lib.refit_trace(self.h, tree, rays.shape[0], rays.ctypes.data_as(C.c_void_p), None, occ.ctypes.data_as(C.c_void_p)) == 0
        return occ.astype(bool)


def grid_exponents(extents):
    e = np.ascontiguousarray(extents, np.float64)
    a, b = np.zeros(len(e), np.int32), np.zeros(len(e), np.int32)
    refit_lib().refit_grid_exponents(len(e), e.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p))
    return a, b


# ------------------------------------------------------------------ scenes
def synthetic_scene(tmp_path):
    """A bumpy, tilted 24x24 height field (1 152 triangles), a quad emitter (2 triangles) and one non-emissive sphere: more than 256
    primitives (spatial splits are on) and more wide nodes than the extend kernel's LDS image holds."""
    n = 25
    u, v = np.meshgrid(np.linspace(-1, 1, n), np.linspace(-1, 1, n), indexing="xy")
    h = 0.45 * np.sin(5.3 * u + 0.4) * np.cos(4.1 * v - 0.7) + 0.25 * np.sin(11.0 * u * v)
    # tilted out of the axes, so that the boxes of neighbouring triangles overlap
    p = np.stack([u + 0.35 * h, 0.8 * h + 0.3 * u - 0.2 * v, v - 0.3 * h], axis=-1).reshape(-1, 3)
    lines = ["v %.9g %.9g %.9g" % tuple(q) for q in p]
    for j in range(n - 1):
        for i in range(n - 1):
            a, b, c, d = j * n + i + 1, j * n + i + 2, (j + 1) * n + i + 2, (j + 1) * n + i + 1
            lines += ["f %d %d %d" % (a, c, b), "f %d %d %d" % (a, d, c)]   # (facing up, towards the emitter)
    (tmp_path / "field.obj").write_text("\n".join(lines) + "\n")
    (tmp_path / "quad.obj").write_text("v -0.6 1.6 -0.6\nv 0.6 1.6 -0.6\nv 0.6 1.6 0.6\nv -0.6 1.6 0.6\nf 1 2 3\nf 1 3 4\n")
    xml = tmp_path / "synthetic.xml"
    xml.write_text("""<scene version="0.6.0"><integrator type="path"><integer name="maxDepth" value="4"/></integrator>
      <sensor type="perspective"><float name="fov" value="45"/><transform name="toWorld"><lookat origin="0.4, 2.2, 3.4" target="0, 0, 0" up="0, 1, 0"/></transform>
        <sampler type="independent"><integer name="sampleCount" value="4"/></sampler>
        <film type="hdrfilm"><integer name="width" value="64"/><integer name="height" value="64"/></film></sensor>
      <shape type="obj"><string name="filename" value="field.obj"/><bsdf type="diffuse"><rgb name="reflectance" value="0.6, 0.5, 0.4"/></bsdf></shape>
      <shape type="obj"><string name="filename" value="quad.obj"/><bsdf type="diffuse"/><emitter type="area"><rgb name="radiance" value="9, 9, 8"/></emitter></shape>
      <shape type="sphere"><point name="center" x="0.3" y="0.75" z="0.2"/><float name="radius" value="0.3"/><bsdf type="diffuse"><rgb name="reflectance" value="0.3, 0.6, 0.3"/></bsdf></shape>
    </scene>""")
    return lj.parse_scene(str(xml))


def load_scene(name, tmp_path=None):
    from helpers import scene_path
    if name == "synthetic":
        return synthetic_scene(tmp_path)
    if name in ("volpath_test4", "vol_cbox"):
        return lj.parse_scene(os.path.join(ROOT, "scenes", "volpath_test", name + ".xml"))
    return lj.parse_scene(scene_path(name))


# ------------------------------------------------------------------ motions
def snapshot(hs):
    """The movable numbers of a description as loaded, and its bounds radius R (of the float scene bounds, as the upload computes it)."""
    d = hs.desc
    P, N = hs.positions(), hs.normals()
    spheres = {i: (np.array(d.shapes[i].position[:]), d.shapes[i].radius) for i in range(d.n_shapes) if d.shapes[i].kind == _abi.LJ_SHAPE_SPHERE}
    lo, hi = [], []
    for i in range(d.n_shapes):
        sh = d.shapes[i]
        if sh.kind == _abi.LJ_SHAPE_SPHERE:
            lo.append(spheres[i][0] - spheres[i][1]); hi.append(spheres[i][0] + spheres[i][1])
        elif sh.n_vertices:
            q = P[sh.first_vertex:sh.first_vertex + sh.n_vertices]
            lo.append(q.min(0)); hi.append(q.max(0))
    R = float(np.linalg.norm(np.max(hi, 0) - np.min(lo, 0)) / 2)
    centre = (np.max(hi, 0) + np.min(lo, 0)) / 2
    return dict(P=P, N=N, spheres=spheres, R=R, centre=centre)


def restore(hs, snap):
    if hs.desc.n_vertices:
        hs.positions_view()[:] = snap["P"]
        hs.normals_view()[:] = snap["N"]
    for i, (c, r) in snap["spheres"].items():
        for k in range(3):
            hs.desc.shapes[i].position[k] = c[k]
        hs.desc.shapes[i].radius = r


def _meshes(hs, emissive):
    d = hs.desc
    return [i for i in range(d.n_shapes) if d.shapes[i].kind != _abi.LJ_SHAPE_SPHERE and d.shapes[i].n_vertices > 0 and (d.shapes[i].area_light_id >= 0) == emissive]


def _rotation(axis, degrees):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    t = np.radians(degrees)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


MOTIONS = ("M0", "M1", "M2", "M3", "M4")


def apply_motion(hs, snap, motion, reset=True):
    """Write motion `motion` into the description through positions_view() / normals_view() and the sphere records.
    M0 identity; M1 one shape translated by three bounds radii and rotated by 40 degrees (the mesh with the fewest vertices, the last of them; its
    normals turn with it); M2 every vertex displaced by 0.1 R sin(k p); M3 the first sphere moved by R, its radius x 1.5 (identity for a scene without
    spheres); M4 the emitter mesh scaled x 2 about its centroid (a scene whose emitters are all spheres: the first emissive sphere's radius
    x 2).  reset=False applies the motion on top of what the description holds."""
    if reset:
        restore(hs, snap)
    d, R = hs.desc, snap["R"]
    P = hs.positions_view() if d.n_vertices else None
    if motion == "M0":
        return hs
    if motion == "M1":
        i = min(_meshes(hs, False) + _meshes(hs, True), key=lambda j: (d.shapes[j].n_vertices, -j))
        sh = d.shapes[i]
        sl = slice(sh.first_vertex, sh.first_vertex + sh.n_vertices)
        rot = _rotation((1.0, 2.0, 3.0), 40.0)
        c = P[sl].mean(0)
        P[sl] = (P[sl] - c) @ rot.T + c + 3.0 * R * np.array([0.6, 0.0, 0.8])
        if sh.has_normals:
            hs.normals_view()[sl] = hs.normals_view()[sl] @ rot.T
    elif motion == "M2":
        k = 9.0 / R
        P += 0.1 * R * np.sin(k * P[:, [1, 2, 0]] + np.array([0.3, 1.1, 2.0]))
    elif motion == "M3":
        ids = sorted(snap["spheres"])
        if ids:
            s = d.shapes[ids[0]]
            for k, v in enumerate((0.48, 0.6, 0.64)):
                s.position[k] += R * v
            s.radius *= 1.5
    elif motion == "M4":
        em = _meshes(hs, True)
        if em:
            sh = d.shapes[em[0]]
            sl = slice(sh.first_vertex, sh.first_vertex + sh.n_vertices)
            c = P[sl].mean(0)
            P[sl] = (P[sl] - c) * 2.0 + c
        else:
            i = [i for i in sorted(snap["spheres"]) if d.shapes[i].area_light_id >= 0][0]
            d.shapes[i].radius *= 2.0
    else:
        raise ValueError(motion)
    return hs


class _Placed:
    def __init__(self, centre, radius):
        self.t = dict(bounds_center=centre, bounds_radius=radius)

    def tables(self):
        return self.t


def mixed_rays(hs, snap, n, seed, oracle):
    """n random_rays: an eighth aimed into the bounds of the description as it stands (oracle: of the moved description), the rest into
    the bounds it was loaded with.  After a motion that carries a shape three radii away the new bounds are mostly empty space; the
    second population still meets the bulk of the scene — and the place the shape left, where a refit that did nothing would report it."""
    from helpers import random_rays
    a = random_rays(hs, n // 8, seed, oracle)
    b = random_rays(hs, n - n // 8, seed + 1000, _Placed(snap["centre"], snap["R"]))
    return np.concatenate([a, b])


def shadow_rays(hs, n, seed, oracle):
    """Shadow-style segments as tests/test_gpu_bvh8.py draws them: random_rays from shadow_epsilon to a random fraction of the bounds radius."""
    from helpers import random_rays
    tb = oracle.tables()
    rays = random_rays(hs, n, seed, oracle)
    rays["tnear"] = np.float32(tb["shadow_epsilon"])
    rays["tfar"] = (np.random.default_rng(seed + 1).random(n) * tb["bounds_radius"]).astype(np.float32)
    return rays
