"""Shared by tests/test_ploc_cpu.py and tests/test_gpu_ploc.py: the host twin of lj_scene_rebuild_bvh_ex with LJ_BUILD_PLOC (tests/twin_ploc,
which holds the twins of the linear rebuild and of the geometry update too), the box inputs of its build query, and the SAH cost of a
binary tree.  Not a test module."""
import ctypes as C

import numpy as np

import lajolla_public_amd as lj
from lajolla_public_amd import _abi, build
from rebuild_common import MAX_STACK_DEPTH, RebuildTwin, query_inputs

_lib = None


def ploc_lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build.build_twin_ploc(verbose=False))
        _lib.refit_create.restype = C.c_void_p
        _lib.refit_create.argtypes = [C.POINTER(_abi.LjSceneDesc), C.c_char_p, C.c_int]
        _lib.refit_free.argtypes = [C.c_void_p]
        _lib.refit_update.argtypes = [C.c_void_p, C.POINTER(_abi.LjSceneDesc), C.c_char_p, C.c_int]
        _lib.refit_read.restype = C.c_int64
        _lib.refit_read.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64]
        _lib.refit_bounds.argtypes = [C.c_void_p, C.c_void_p]
        _lib.refit_trace.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.refit_prim_boxes.argtypes = [C.c_void_p, C.c_void_p]
        _lib.rebuild_rebuild.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.c_char_p, C.c_int]
        _lib.rebuild_info.argtypes = [C.c_void_p, C.c_void_p]
        _lib.ploc_build.restype = C.c_int64
        _lib.ploc_build.argtypes = [C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int32)]
        _lib.ploc_rebuild.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_char_p, C.c_int]
        _lib.ploc_scene_boxes.restype = C.c_int64
        _lib.ploc_scene_boxes.argtypes = [C.c_void_p, C.c_void_p]
        _lib.ploc_emit.argtypes = [C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_char_p, C.c_int]
        _lib.ploc_compact.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
    return _lib


class PlocTwin(RebuildTwin):
    """The twin of the geometry update and of the linear rebuild, with lj_scene_rebuild_bvh_ex(LJ_BUILD_PLOC) as the host twin runs it."""

    def __init__(self, hs):
        self.hs, self.lib = hs, ploc_lib()
        err = C.create_string_buffer(512)
        self.h = C.c_void_p(self.lib.refit_create(hs.desc_ptr, err, 512))
        if not self.h:
            raise RuntimeError(err.value.decode())

    def rebuild(self, max_depth4=MAX_STACK_DEPTH, builder="ploc", radius=0):
        """0, or the LJ_ERR_* code of a refused rebuild (the message in self.error); self.rebuilt: 1, or 0 for the no-op"""
        if builder == "lbvh":
            return RebuildTwin.rebuild(self, max_depth4)
        err, done = C.create_string_buffer(512), C.c_int32()
        rc = self.lib.ploc_rebuild(self.h, radius, max_depth4, C.byref(done), err, 512)
        self.error, self.rebuilt = err.value.decode(), done.value
        return rc

    def scene_boxes(self):
        """The padded boxes of the scene's primitives, by global primitive: what either builder starts from"""
        out = np.zeros((self.lib.ploc_scene_boxes(self.h, None), 2, 3), np.float32)
        self.lib.ploc_scene_boxes(self.h, out.ctypes.data_as(C.c_void_p))
        return out


def twin_ploc_build(boxes, radius=0):
    """lj_bvh_build_query_ex(LJ_BUILD_PLOC) on the host: (order, nodes, rounds of clustering)"""
    boxes = np.ascontiguousarray(boxes, np.float32).reshape(-1, 2, 3)
    n = boxes.shape[0]
    order, nodes, rounds = np.zeros(n, np.int32), np.zeros(max(2 * n, 1), lj.BINARY_NODE), C.c_int32()
    got = ploc_lib().ploc_build(n, boxes.ctypes.data_as(C.c_void_p), radius, order.ctypes.data_as(C.c_void_p), nodes.ctypes.data_as(C.c_void_p), nodes.size, C.byref(rounds))
    assert got >= 0
    return order, nodes[:got].copy(), rounds.value


def ploc_emit(boxes, max_depth4, radius=0):
    """emit_wide on the PLOC tree of boxes: (code, message, sizes of nodes / nodes8 / leaf_order and depth4 as the call left them)"""
    boxes = np.ascontiguousarray(boxes, np.float32).reshape(-1, 2, 3)
    out, err = np.zeros(4, np.int64), C.create_string_buffer(512)
    rc = ploc_lib().ploc_emit(len(boxes), boxes.ctypes.data_as(C.c_void_p), radius, max_depth4, out.ctypes.data_as(C.c_void_p), err, 512)
    return rc, err.value.decode(), [int(v) for v in out]


def sheet_boxes(n=64):
    """The boxes of the 2 (n - 1)^2 triangles of a wavy, tilted n x n height field (the field of refit_common.synthetic_scene)"""
    u, v = np.meshgrid(np.linspace(-1, 1, n), np.linspace(-1, 1, n), indexing="xy")
    h = 0.45 * np.sin(5.3 * u + 0.4) * np.cos(4.1 * v - 0.7) + 0.25 * np.sin(11.0 * u * v)
    p = np.stack([u + 0.35 * h, 0.8 * h + 0.3 * u - 0.2 * v, v - 0.3 * h], axis=-1).astype(np.float32)
    a, b, c, d = p[:-1, :-1], p[:-1, 1:], p[1:, 1:], p[1:, :-1]
    tris = np.stack([np.stack([a, c, b], axis=2), np.stack([a, d, c], axis=2)], axis=2).reshape(-1, 3, 3)
    return np.stack([tris.min(1), tris.max(1)], axis=1)


def ploc_inputs(large=False):
    """The box sets of the PLOC tests, by name: query_inputs() (random100003 only when `large`) and three of their own"""
    out = {k: v for k, v in query_inputs().items() if large or k != "random100003"}
    rng = np.random.default_rng(78)
    c, h = rng.uniform(-10, 10, (3000, 3)), rng.uniform(0.01, 0.2, (3000, 3))
    tenth = np.arange(0, 3000, 10)
    h[tenth, rng.integers(0, 3, len(tenth))] = rng.uniform(2.0, 6.0, len(tenth))   # one axis of every tenth box stretched
    out["mixed3000"] = np.stack([c - h, c + h], axis=1).astype(np.float32)
    out["sheet7938"] = sheet_boxes(64)
    half = np.arange(1, 201, dtype=np.float32)[:, None] * np.ones(3, np.float32)
    out["nested200"] = np.stack([-half, half], axis=1)
    return out


def sah_cost(nodes):
    """Sum over inner nodes of A / A_root + sum over leaves of count A / A_root, A a box's half area in float64"""
    e = nodes["hi"].astype(np.float64) - nodes["lo"].astype(np.float64)
    area = e[:, 0] * e[:, 1] + e[:, 1] * e[:, 2] + e[:, 2] * e[:, 0]
    leaf = nodes["left"] < 0
    return float((area[~leaf].sum() + (nodes["count"][leaf] * area[leaf]).sum()) / area[0])


def binary_depth(nodes):
    depth = np.zeros(len(nodes), np.int32)
    depth[0] = 1
    for i, nd in enumerate(nodes):   # (breadth-first: a parent comes before its children)
        if nd["left"] >= 0:
            depth[nd["left"]] = depth[nd["right"]] = depth[i] + 1
    return int(depth.max())
