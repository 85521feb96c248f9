"""Shared by tests/test_rebuild_cpu.py and tests/test_gpu_rebuild.py: the host twin of lj_scene_rebuild_bvh (tests/twin_rebuild, which holds
the twin of the geometry update too), the box inputs of the build query, and the structural checks of a rebuilt scene.  Not a test module."""
import ctypes as C
import glob
import os

import numpy as np

import lajolla_public_amd as lj
from lajolla_public_amd import _abi, build
from refit_common import NODE4, NODE8, PRIM, ROOT, RefitTwin

MAX_STACK_DEPTH = 40   # device/extend.hip max_stack_depth(): inner levels of the BVH4 a traversal can hold
SHIPPED = sorted(os.path.relpath(f, os.path.join(ROOT, "scenes")) for f in glob.glob(os.path.join(ROOT, "scenes", "*", "*.xml")))

_lib = None


def rebuild_lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build.build_twin_rebuild(verbose=False))
        _lib.refit_create.restype = C.c_void_p
        _lib.refit_create.argtypes = [C.POINTER(_abi.LjSceneDesc), C.c_char_p, C.c_int]
        _lib.refit_free.argtypes = [C.c_void_p]
        _lib.refit_update.argtypes = [C.c_void_p, C.POINTER(_abi.LjSceneDesc), C.c_char_p, C.c_int]
        _lib.refit_read.restype = C.c_int64
        _lib.refit_read.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64]
        _lib.refit_bounds.argtypes = [C.c_void_p, C.c_void_p]
        _lib.refit_trace.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.refit_prim_boxes.argtypes = [C.c_void_p, C.c_void_p]
        _lib.rebuild_build.restype = C.c_int64
        _lib.rebuild_build.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
        _lib.rebuild_rebuild.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.c_char_p, C.c_int]
        _lib.rebuild_info.argtypes = [C.c_void_p, C.c_void_p]
        _lib.rebuild_emit_chain.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_char_p, C.c_int]
    return _lib


class RebuildTwin(RefitTwin):
    """The twin of the geometry update, with lj_scene_rebuild_bvh as the host twin runs it."""

    def __init__(self, hs):
        self.hs, self.lib = hs, rebuild_lib()
        err = C.create_string_buffer(512)
        self.h = C.c_void_p(self.lib.refit_create(hs.desc_ptr, err, 512))
        if not self.h:
            raise RuntimeError(err.value.decode())

    def rebuild(self, max_depth4=MAX_STACK_DEPTH):
        """0, or the LJ_ERR_* code of a refused rebuild (the message in self.error); self.rebuilt: 1, or 0 for the no-op"""
        err, done = C.create_string_buffer(512), C.c_int32()
        rc = self.lib.rebuild_rebuild(self.h, max_depth4, C.byref(done), err, 512)
        self.error, self.rebuilt = err.value.decode(), done.value
        return rc

    def info(self):
        out = np.zeros(4, np.int64)
        self.lib.rebuild_info(self.h, out.ctypes.data_as(C.c_void_p))
        return dict(depth4=int(out[0]), depth8=int(out[1]), n_leaves=int(out[2]), n_prims=int(out[3]))


def twin_build(boxes):
    """lj_bvh_build_query on the host: (order, nodes)"""
    boxes = np.ascontiguousarray(boxes, np.float32).reshape(-1, 2, 3)
    n = boxes.shape[0]
    order, nodes = np.zeros(n, np.int32), np.zeros(max(2 * n, 1), lj.BINARY_NODE)
    got = rebuild_lib().rebuild_build(n, boxes.ctypes.data_as(C.c_void_p), order.ctypes.data_as(C.c_void_p), nodes.ctypes.data_as(C.c_void_p), nodes.size)
    assert got >= 0
    return order, nodes[:got].copy()


def emit_chain(links, max_depth4):
    """emit_wide on a chain of `links` inner nodes: (code, message, sizes of nodes / nodes8 / leaf_order and depth4 as the call left them)"""
    out, err = np.zeros(4, np.int64), C.create_string_buffer(512)
    rc = rebuild_lib().rebuild_emit_chain(links, max_depth4, out.ctypes.data_as(C.c_void_p), err, 512)
    return rc, err.value.decode(), [int(v) for v in out]


def query_inputs():
    """The box sets of the build query's test, by name: (n, 2, 3) float32 each"""
    rng = np.random.default_rng(77)

    def random_boxes(n):
        c = rng.uniform(-10, 10, (n, 3))
        h = rng.uniform(0.01, 0.5, (n, 3))
        return np.stack([c - h, c + h], axis=1).astype(np.float32)

    out = {"n%d" % n: random_boxes(n) for n in (0, 1, 2, 4, 5, 8, 9)}
    out["coincident64"] = np.repeat(random_boxes(1), 64, axis=0)
    line = np.zeros((257, 2, 3), np.float32)
    line[:, 0, 1], line[:, 1, 1] = np.arange(257) * 0.37 - 0.1, np.arange(257) * 0.37 + 0.1
    line[:, 0, [0, 2]], line[:, 1, [0, 2]] = -1.0, 1.0
    out["one_axis257"] = line[rng.permutation(257)]
    out["random1000"] = random_boxes(1000)
    out["pairs1000"] = np.repeat(random_boxes(500), 2, axis=0)[rng.permutation(1000)]
    out["random100003"] = random_boxes(100003)
    return out


def check_binary_tree(order, nodes, n):
    """The compacted tree covers the sorted positions once, in leaves of one to four, breadth-first from node 0."""
    assert sorted(order.tolist()) == list(range(n))
    if n == 0:
        assert len(nodes) == 0
        return
    covered, nxt = np.zeros(n, np.int32), 1
    for i, nd in enumerate(nodes):
        if nd["left"] < 0:
            assert nd["right"] < 0 and 1 <= nd["count"] <= 4
            covered[nd["first"]:nd["first"] + nd["count"]] += 1
        else:
            assert (nd["left"], nd["right"]) == (nxt, nxt + 1), "not breadth-first"
            nxt += 2
    assert nxt == len(nodes) and (covered == 1).all()


def _contains(outer_lo, outer_hi, lo, hi):
    return bool(np.all(outer_lo <= lo) and np.all(outer_hi >= hi))


def check_wide_trees(tw):
    """Of a twin's BVH4 and BVH8: every primitive appears once in the leaf order, leaves hold one to four, and every box contains its subtree
    in exact arithmetic — float planes compared as float64, BVH8 planes dequantised as p + q 2^(e - 127) in float64 (the checks of
    tests/test_refit_cpu.py).  Returns the number of leaves."""
    st = tw.structures()
    order = tw.leaf_order()
    n_prims = tw.info()["n_prims"]
    assert sorted(order.tolist()) == list(range(n_prims)), "the leaf order is not a permutation of the primitives"
    lp = tw.table("leaf_prims").view(PRIM)
    assert np.array_equal(lp["gprim"], order)
    boxes = tw.prim_boxes().astype(np.float64)
    assert np.isfinite(boxes).all()
    n4, n8 = st[0].view(NODE4), st[1].view(NODE8)

    def leaf_box(first, count):
        return boxes[first:first + count, 0].min(0), boxes[first:first + count, 1].max(0)

    leaves = []
    seen = np.zeros(len(boxes), np.int32)
    stack = [(0, np.full(3, -np.inf), np.full(3, np.inf))]
    while stack:
        i, alo, ahi = stack.pop()
        for k in range(4):
            lo, hi = n4["lo"][i, :, k].astype(np.float64), n4["hi"][i, :, k].astype(np.float64)
            if not (lo[0] <= hi[0]):
                continue
            assert _contains(alo, ahi, lo, hi), ("bvh4 slot outside its ancestors", i, k)
            c = int(n4["child"][i, k])
            if c >= 0:
                stack.append((c, lo, hi))
            else:
                first, count = (~c) >> 3, ((~c) & 7) + 1
                assert 1 <= count <= 4
                assert _contains(lo, hi, *leaf_box(first, count)), ("bvh4 leaf", i, k)
                seen[first:first + count] += 1
                leaves.append((first, count))
    assert (seen == 1).all()
    seen[:] = 0
    leaves8 = []
    stack = [(0, np.full(3, -np.inf), np.full(3, np.inf))]
    while stack:
        i, alo, ahi = stack.pop()
        nd = n8[i]
        step = np.ldexp(1.0, nd["e"].astype(np.int64) - 127)
        p = nd["p"].astype(np.float64)
        rank = 0
        for s in range(8):
            inner, leaf = (int(nd["imask"]) >> s) & 1, int(nd["meta"][s]) & 0x80
            if not inner and not leaf:
                continue
            lo, hi = p + nd["qlo"][:, s].astype(np.float64) * step, p + nd["qhi"][:, s].astype(np.float64) * step
            lo, hi = np.maximum(alo, lo), np.minimum(ahi, hi)   # (a slot's planes lie on its own node's grid: test_refit_cpu.py)
            if inner:
                stack.append((int(nd["child_base"]) + rank, lo, hi))
                rank += 1
            else:
                m = int(nd["meta"][s])
                first, count = int(nd["prim_base"]) + (m & 31), ((m >> 5) & 3) + 1
                assert _contains(lo, hi, *leaf_box(first, count)), ("bvh8 leaf outside its slot or an ancestor's", i, s)
                seen[first:first + count] += 1
                leaves8.append((first, count))
    assert (seen == 1).all() and sorted(leaves8) == sorted(leaves), "the two trees do not share their leaves"
    return len(leaves)
