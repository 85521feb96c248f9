"""lj_scene_rebuild_bvh_ex with LJ_BUILD_PLOC on the host (tests/twin_ploc: the rule of device/dploc.h run round by round, the product's
compact_ploc_tree, emit_wide and level tables, the refit of device/drefit.h): the twin's trees are trees with exact boxes and equal a slow
numpy implementation of the rule byte for byte; their SAH cost is below the linear BVH's by the margins the rule was chosen for; the rebuilt
trees of every shipped scene hold every primitive once under boxes that contain them, within the traversal stack; hits through them equal the
oracle's bit for bit; a tree too deep for the stack is refused with nothing written."""
import ctypes as C
import os

import numpy as np
import pytest

import lajolla_public_amd as lj
from lajolla_public_amd import _abi
from helpers import Oracle
from refit_common import ROOT, apply_motion, mixed_rays, shadow_rays, snapshot, synthetic_scene
from rebuild_common import MAX_STACK_DEPTH, SHIPPED, check_binary_tree, check_wide_trees, twin_build
from ploc_common import PlocTwin, binary_depth, ploc_emit, ploc_inputs, ploc_lib, sah_cost, twin_ploc_build

INPUTS = ploc_inputs()


@pytest.fixture(scope="module")
def synthetic(tmp_path_factory):
    hs = synthetic_scene(tmp_path_factory.mktemp("ploc"))
    return hs, snapshot(hs)


# ------------------------------------------------------------------ tree structure
@pytest.mark.parametrize("name", list(INPUTS))
def test_the_twins_trees_are_trees_with_exact_boxes(name):
    boxes = INPUTS[name]
    order, nodes, rounds = twin_ploc_build(boxes)
    check_binary_tree(order, nodes, len(boxes))
    for nd in nodes[::-1]:   # every node's box is the union of the boxes below it
        if nd["left"] < 0:
            b = boxes[order[nd["first"]:nd["first"] + nd["count"]]]
            assert np.array_equal(nd["lo"], b[:, 0].min(0)) and np.array_equal(nd["hi"], b[:, 1].max(0))
        else:
            l, r = nodes[nd["left"]], nodes[nd["right"]]
            assert np.array_equal(nd["lo"], np.minimum(l["lo"], r["lo"])) and np.array_equal(nd["hi"], np.maximum(l["hi"], r["hi"]))
            assert nd["count"] == l["count"] + r["count"] > 4 and nd["first"] == l["first"] and r["first"] == l["first"] + l["count"]
    assert rounds == 0 if len(boxes) < 2 else 1 <= rounds <= len(boxes) - 1
    if name == "coincident64":   # the bit-length tie-break pairs a run of coincident boxes (2k, 2k + 1): 64 -> 16 leaves of four in six rounds
        assert np.array_equal(order, np.arange(64)) and len(nodes) == 31 and (nodes["count"][nodes["left"] < 0] == 4).all() and rounds == 6
    if name == "nested200":      # every cube's nearest neighbour is a smaller one: one merge per round, a chain
        assert rounds == 199 and binary_depth(nodes) > 2 * MAX_STACK_DEPTH


# ------------------------------------------------------------------ an independent implementation
def _morton_order(boxes):
    """drebuild.h in numpy: 21 bits per axis of the float64 centroid within the centroid bounds, x highest, a stable sort"""
    c = 0.5 * (boxes[:, 0].astype(np.float64) + boxes[:, 1].astype(np.float64))
    cmin, cmax = c.min(0), c.max(0)
    codes = [0] * len(boxes)
    for k in range(3):
        extent = cmax[k] - cmin[k]
        q = np.clip(np.floor((c[:, k] - cmin[k]) / extent * float(1 << 21)), 0, (1 << 21) - 1).astype(np.int64) if extent > 0 else np.zeros(len(boxes), np.int64)
        for i, v in enumerate(q.tolist()):
            codes[i] |= sum(((v >> b) & 1) << (3 * b + 2 - k) for b in range(21))
    return np.array(sorted(range(len(boxes)), key=lambda i: codes[i]), np.int64)   # (sorted() is stable)


def _union(lo_a, hi_a, lo_b, hi_b):
    """a's box grown by b's, with drefit.h's tie rule (the first argument on a tie)"""
    return np.where(lo_b < lo_a, lo_b, lo_a), np.where(hi_a < hi_b, hi_b, hi_a)


def _slow_ploc(boxes, radius):
    """The rule of the issue, clusters as Python lists: (order, nodes) as lj_bvh_build_query_ex returns them"""
    n = len(boxes)
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(0, lj.BINARY_NODE)
    morton = _morton_order(boxes)
    lo, hi = boxes[morton, 0].copy(), boxes[morton, 1].copy()
    ids, counts = [~p for p in range(n)], [1] * n
    raw = []   # (lo, hi, left, right, count)
    while len(ids) > 1:
        m = len(ids)
        K = 2 * radius
        D, L, J = np.full((m, K), np.inf, np.float32), np.full((m, K), 99, np.int64), np.full((m, K), 1 << 40, np.int64)
        pos = np.arange(m)
        for col, off in enumerate([o for o in range(-radius, radius + 1) if o != 0]):
            j = pos + off
            ok = (j >= 0) & (j < m)
            a, b = np.minimum(pos, j)[ok], np.maximum(pos, j)[ok]   # the lower position's box grows by the higher's
            ulo, uhi = _union(lo[a], hi[a], lo[b], hi[b])
            e = (uhi - ulo).astype(np.float32)
            D[ok, col] = (e[:, 0] * e[:, 1] + e[:, 1] * e[:, 2]) + e[:, 2] * e[:, 0]
            L[ok, col] = [int(x).bit_length() for x in (pos[ok] ^ j[ok])]
            J[ok, col] = j[ok]
        best = np.lexsort((J, L, D), axis=1)[:, 0]   # least (d, bitlen, j)
        nn = J[pos, best]
        mutual = nn[nn] == pos
        nlo, nhi, nids, ncounts = [], [], [], []
        for i in range(m):
            if mutual[i] and nn[i] < i:
                continue
            if mutual[i]:
                j = int(nn[i])
                ulo, uhi = _union(lo[i], hi[i], lo[j], hi[j])
                raw.append((ulo, uhi, ids[i], ids[j], counts[i] + counts[j]))
                nlo.append(ulo); nhi.append(uhi); nids.append(len(raw) - 1); ncounts.append(counts[i] + counts[j])
            else:
                nlo.append(lo[i]); nhi.append(hi[i]); nids.append(ids[i]); ncounts.append(counts[i])
        lo, hi, ids, counts = np.array(nlo), np.array(nhi), nids, ncounts
    # the depth-first order below the root, the breadth-first numbering, leaves of at most four
    order, first, where = [], {}, {}

    def walk(k):
        if k < 0:
            where[~k] = len(order)
            order.append(int(morton[~k]))
        else:
            first[k] = len(order)
            walk(raw[k][2]); walk(raw[k][3])
    out = np.zeros(max(2 * n, 1), lj.BINARY_NODE)
    if n == 1:
        out[0] = (boxes[0, 0], boxes[0, 1], -1, -1, 0, 1)
        return np.zeros(1, np.int32), out[:1]
    import sys
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 4 * n + 100))
    walk(len(raw) - 1)
    queue, used = [len(raw) - 1], 1
    for h, k in enumerate(queue):
        if k < 0:
            g = morton[~k]
            out[h] = (boxes[g, 0], boxes[g, 1], -1, -1, where[~k], 1)
            continue
        rlo, rhi, left, right, count = raw[k]
        if count <= 4:
            out[h] = (rlo, rhi, -1, -1, first[k], count)
        else:
            out[h] = (rlo, rhi, used, used + 1, first[k], count)
            queue += [left, right]
            used += 2
    return np.array(order, np.int32), out[:used].copy()


@pytest.mark.parametrize("radius", [1, 8, 32])
@pytest.mark.parametrize("name", [k for k, v in INPUTS.items() if len(v) <= 1000])
def test_the_twin_equals_a_slow_implementation_of_the_rule(name, radius):
    boxes = INPUTS[name]
    order, nodes, _ = twin_ploc_build(boxes, radius)
    want_order, want_nodes = _slow_ploc(boxes, radius)
    assert order.tobytes() == want_order.tobytes()
    assert nodes.tobytes() == want_nodes.tobytes()


def test_the_default_radius_is_eight():
    boxes = INPUTS["random1000"]
    assert twin_ploc_build(boxes)[1].tobytes() == twin_ploc_build(boxes, 8)[1].tobytes() != twin_ploc_build(boxes, 1)[1].tobytes()


# ------------------------------------------------------------------ quality
SCENE_FILES = {"sponza": "sponza/sponza.xml", "disney_bsdf": "disney_bsdf_test/disney_bsdf.xml", "vol_cbox_teapot": "volpath_test/vol_cbox_teapot.xml"}


@pytest.mark.parametrize("name,bound", [("mixed3000", 0.85), ("sheet7938", 0.97), ("sponza", 0.85), ("disney_bsdf", 0.95), ("vol_cbox_teapot", 0.80)])
def test_sah_cost_against_the_linear_bvh(name, bound):
    boxes = INPUTS[name] if name in INPUTS else PlocTwin(lj.parse_scene(os.path.join(ROOT, "scenes", SCENE_FILES[name]))).scene_boxes()
    _, ploc, rounds = twin_ploc_build(boxes)
    _, lbvh = twin_build(boxes)
    cost, base = sah_cost(ploc), sah_cost(lbvh)
    print("%s: %d boxes, LBVH cost %.2f depth %d, PLOC cost %.2f depth %d in %d rounds: ratio %.3f (required <= %.2f)"
          % (name, len(boxes), base, binary_depth(lbvh), cost, binary_depth(ploc), rounds, cost / base, bound))
    assert cost / base <= bound


# ------------------------------------------------------------------ every shipped scene
def _everything(tw):
    return [x.tobytes() for x in tw.structures()] + [tw.leaf_order().tobytes(), tw.table("leaf_prims").tobytes()]


@pytest.mark.parametrize("name", SHIPPED)
def test_ploc_trees_of_every_shipped_scene(name):
    tw = PlocTwin(lj.parse_scene(os.path.join(ROOT, "scenes", name)))
    before = _everything(tw)
    scan = tw.bounds()["n_scan_used"] > 0
    assert tw.rebuild() == 0, tw.error
    if scan or tw.info()["n_prims"] == 0:   # a leaf-scan scene (or an empty one): the no-op
        assert tw.rebuilt == 0 and _everything(tw) == before
        return
    assert tw.rebuilt == 1 and _everything(tw) != before
    n_leaves = check_wide_trees(tw)
    info = tw.info()
    print(name, info)
    assert info["n_leaves"] == n_leaves and 1 <= info["depth4"] <= MAX_STACK_DEPTH and 1 <= info["depth8"] <= info["depth4"]
    assert len(tw.structures()[2]) == 0
    st = [x.tobytes() for x in tw.structures()]
    assert tw.update(tw.hs) == 0, tw.error
    assert [x.tobytes() for x in tw.structures()] == st, "an update with unchanged positions changed a byte"


# ------------------------------------------------------------------ hits
@pytest.mark.parametrize("motion", ["M1", "M2"])
def test_hits_through_the_ploc_trees_equal_the_oracle(motion, synthetic):
    hs, snap = synthetic
    tw = PlocTwin(apply_motion(hs, snap, "M0"))
    assert tw.update(apply_motion(hs, snap, motion)) == 0, tw.error
    assert tw.rebuild(builder="lbvh") == 0 and tw.rebuilt == 1, tw.error
    linear = [x.tobytes() for x in tw.structures()]
    assert tw.rebuild() == 0 and tw.rebuilt == 1, tw.error
    assert [x.tobytes() for x in tw.structures()] != linear, "the PLOC trees are the linear builder's"
    assert tw.info()["n_prims"] == 1155 == len(tw.leaf_order())
    o = Oracle(hs)
    rays = mixed_rays(hs, snap, 20000, 11, o)
    ho = o.intersect(rays)
    assert (ho["shape_id"] >= 0).mean() > 0.2
    r2 = shadow_rays(hs, 20000, 12, o)
    oo = o.occluded(r2)
    for tree in (0, 1):
        ht = tw.intersect(tree, rays)
        for f in ("t", "u", "v", "shape_id", "prim_id"):
            assert np.array_equal(ho[f].view(np.uint32), ht[f].view(np.uint32)), (tree, f)
        assert np.array_equal(oo, tw.occluded(tree, r2)), tree


# ------------------------------------------------------------------ refusals
def test_a_ploc_tree_deeper_than_the_stack_is_refused_and_nothing_is_written():
    rc, msg, out = ploc_emit(INPUTS["nested200"], MAX_STACK_DEPTH)
    assert rc == _abi.LJ_ERR_UNSUPPORTED and "exceeds the traversal stack" in msg
    assert out == [3, 5, 7, -7], "a refused emit_wide wrote to its outputs"
    rc, _, out = ploc_emit(INPUTS["nested200"], 0)   # the same tree without the bound: its depth
    assert rc == 0 and out[2] == 200 and out[3] > MAX_STACK_DEPTH
    rc, _, out = ploc_emit(INPUTS["random1000"], MAX_STACK_DEPTH)
    assert rc == 0 and out[2] == 1000 and 1 < out[3] <= MAX_STACK_DEPTH


def test_compact_ploc_tree_refuses_what_is_not_a_tree():
    # three positions, two nodes: node 0 = (~0, ~1), node 1 = (0, ~2), the root
    boxes = INPUTS["n4"][:3]
    order = np.arange(3, dtype=np.int32)

    def compact(records):
        raw = np.zeros(2, lj.BINARY_NODE)
        for i, (left, right, count) in enumerate(records):
            raw[i]["left"], raw[i]["right"], raw[i]["count"] = left, right, count
        err = C.create_string_buffer(512)
        return ploc_lib().ploc_compact(3, raw.ctypes.data_as(C.c_void_p), boxes.ctypes.data_as(C.c_void_p), order.ctypes.data_as(C.c_void_p), err, 512)
    assert compact([(~0, ~1, 2), (0, ~2, 3)]) == 0
    assert compact([(~0, ~1, 2), (1, ~2, 3)]) == _abi.LJ_ERR_INTERNAL, "a node that is its own child"
    assert compact([(~0, ~3, 2), (0, ~2, 3)]) == _abi.LJ_ERR_INTERNAL, "a position outside the primitives"
    assert compact([(~0, ~1, 2), (0, ~1, 3)]) == _abi.LJ_ERR_INTERNAL, "a position reached twice"
    assert compact([(~0, ~1, 2), (0, ~2, 4)]) == _abi.LJ_ERR_INTERNAL, "a count that is not the sum of its children's"
    assert compact([(~0, ~1, 2), (~2, ~1, 2)]) == _abi.LJ_ERR_INTERNAL, "a node that is never reached"
