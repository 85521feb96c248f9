"""lj_scene_rebuild_bvh_ex with LJ_BUILD_PLOC on the device: the clustering of ploc.hip — whole-grid rounds, the single-workgroup tail, and
both at every radius — equals the host twin's byte for byte, the rebuilt BVH4 and BVH8 equal the twin's, closest hits and occlusion after
an update and a PLOC rebuild equal the oracle's of the moved description, and every per-sample radiance is bit-identical to a fresh upload
(nothing depends on the tree: tests/test_gpu_rebuild.py).  LJ_BUILD_LBVH is the old call; a leaf-scan scene is left untouched; an unknown
builder and a radius above 32 are refused with nothing written."""
import ctypes as C
import os

import numpy as np
import pytest

import lajolla_public_amd as lj
from lajolla_public_amd import _abi
from helpers import Oracle
from refit_common import ROOT, apply_motion, load_scene, mixed_rays, shadow_rays, snapshot
from rebuild_common import check_binary_tree
from ploc_common import PlocTwin, ploc_inputs, twin_ploc_build

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return lj.Context(0)


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    cache = {}

    def get(name):
        if name not in cache:
            hs = lj.parse_scene(os.path.join(ROOT, "scenes", "volpath_test", name + ".xml")) if name == "vol_cbox_teapot" else load_scene(name, tmp_path_factory.mktemp("ploc"))
            cache[name] = (hs, snapshot(hs))
        hs, snap = cache[name]
        apply_motion(hs, snap, "M0")
        return hs, snap
    return get


@pytest.fixture(scope="module")
def inputs():
    out = ploc_inputs(large=True)
    rng = np.random.default_rng(79)
    for n in (1024, 1025, 5000):   # around the size at which the single-workgroup launch takes over
        c, h = rng.uniform(-10, 10, (n, 3)), rng.uniform(0.01, 0.5, (n, 3))
        out["tail%d" % n] = np.stack([c - h, c + h], axis=1).astype(np.float32)
    return out


def _structures(sc):
    return [lj.read_bvh(sc, w).tobytes() for w in (0, 1, 2)]


def _same_as_the_twin(ctx, boxes, radius=None):
    order, nodes = lj.bvh_build_query(ctx, boxes, builder="ploc", radius=radius)
    want_order, want_nodes, _ = twin_ploc_build(boxes, radius or 0)
    assert order.tobytes() == want_order.tobytes()
    assert nodes.tobytes() == want_nodes.tobytes()
    return order, nodes


@pytest.mark.parametrize("name", ["n0", "n1", "n2", "n4", "n5", "n8", "n9", "coincident64", "one_axis257", "random1000", "pairs1000", "mixed3000", "sheet7938", "nested200",
                                  "tail1024", "tail1025", "tail5000", "random100003"])
def test_build_query_equals_the_twin(name, ctx, inputs):
    boxes = inputs[name]
    order, nodes = _same_as_the_twin(ctx, boxes)
    check_binary_tree(order, nodes, len(boxes))


@pytest.mark.parametrize("radius", [1, 8, 32])
def test_build_query_equals_the_twin_at_every_radius(radius, ctx, inputs):
    _same_as_the_twin(ctx, inputs["random1000"], radius)
    _same_as_the_twin(ctx, inputs["tail5000"], radius)   # (through the whole-grid rounds too: the LDS tile with its halo of `radius`)


def test_the_tail_launch_and_whole_grid_rounds_give_the_same_tree(ctx, inputs, monkeypatch):
    for name in ("random1000", "nested200", "tail1025"):
        with_tail = lj.bvh_build_query(ctx, inputs[name], builder="ploc")
        monkeypatch.setenv("LJ_TUNE_PLOC_TAIL", "1")   # every round a round of whole-grid launches (nested200: 199 of them)
        without = lj.bvh_build_query(ctx, inputs[name], builder="ploc")
        monkeypatch.delenv("LJ_TUNE_PLOC_TAIL")
        assert with_tail[0].tobytes() == without[0].tobytes() and with_tail[1].tobytes() == without[1].tobytes(), name


def test_the_linear_builder_is_the_old_call(ctx, inputs):
    for name in ("n5", "random1000", "tail5000"):
        old = lj.bvh_build_query(ctx, inputs[name])
        new = lj.bvh_build_query(ctx, inputs[name], builder=_abi.LJ_BUILD_LBVH, radius=0)   # (through lj_bvh_build_query_ex)
        assert old[0].tobytes() == new[0].tobytes() and old[1].tobytes() == new[1].tobytes(), name


def test_structures_after_a_ploc_rebuild_equal_the_twins(ctx, scenes):
    hs, snap = scenes("synthetic")
    sc, tw = lj.Scene(ctx, hs), PlocTwin(hs)

    def same(what):
        for w in (0, 1):
            assert lj.read_bvh(sc, w).tobytes() == tw.read(w).tobytes(), (what, w)
        assert len(lj.read_bvh(sc, 2)) == 0
    same("upload")
    apply_motion(hs, snap, "M2")
    sc.update_geometry(hs, rebuild="ploc")
    assert tw.update(hs) == 0 and tw.rebuild() == 0 and tw.rebuilt == 1, tw.error
    assert lj.rebuild_stats(sc).rebuilt == 1 and lj.rebuild_stats(sc).n_prims == 1155
    bs = lj.build_stats(sc)
    assert (bs.builder, bs.radius) == (1, 8) and bs.rounds > 0 and bs.tail_rounds <= bs.rounds and bs.cluster_ms > 0
    same("M2 + PLOC rebuild")
    rebuilt = _structures(sc)
    sc.rebuild_bvh(builder="ploc")
    assert _structures(sc) == rebuilt, "two rebuilds of the same positions differ"
    sc.update_geometry(hs)
    assert _structures(sc) == rebuilt, "an update with unchanged positions changed a byte"
    # the linear builder through the new call is the old call, and the statistics say which builder ran
    sc.rebuild_bvh(builder="lbvh", radius=0)
    linear = _structures(sc)
    bs = lj.build_stats(sc)
    assert (bs.builder, bs.radius, bs.rounds, bs.tail_rounds) == (0, 0, 0, 0) and linear != rebuilt
    sc.rebuild_bvh()
    assert _structures(sc) == linear
    assert tw.rebuild(builder="lbvh") == 0, tw.error
    same("linear rebuild")
    sc.rebuild_bvh(builder="ploc", radius=16)
    assert tw.rebuild(radius=16) == 0, tw.error
    assert lj.build_stats(sc).radius == 16
    same("PLOC at radius 16")


@pytest.mark.parametrize("name,bvh8,motion,n_rays", [("synthetic", 0, "M2", 1 << 16), ("synthetic", 1, "M2", 1 << 16), ("disney_bsdf", 1, "M2", 1 << 17)])
def test_hits_after_a_ploc_rebuild_equal_the_oracle(name, bvh8, motion, n_rays, ctx, scenes, monkeypatch):
    hs, snap = scenes(name)
    monkeypatch.setenv("LJ_TUNE_BVH8", str(bvh8))   # read at upload and again at the rebuild
    sc = lj.Scene(ctx, hs)
    apply_motion(hs, snap, motion)
    sc.update_geometry(hs, rebuild="ploc")
    assert lj.rebuild_stats(sc).rebuilt == 1 and lj.build_stats(sc).builder == 1
    o = Oracle(hs)
    rays = mixed_rays(hs, snap, n_rays, 31, o)
    hg, ho = lj.intersect(sc, rays["org"], rays["dir"], 0.0, np.inf), o.intersect(rays)
    assert (ho["shape_id"] >= 0).mean() > 0.2
    for f in ("t", "u", "v", "shape_id", "prim_id"):
        assert np.array_equal(hg[f].view(np.uint32), ho[f].view(np.uint32)), f
    r2 = shadow_rays(hs, 50000, 32, o)
    assert np.array_equal(lj.occluded(sc, r2["org"], r2["dir"], r2["tnear"], r2["tfar"]), o.occluded(r2))


def _render_pair(sc, fresh, crop, spp, **kw):
    a = lj.render_samples(sc, crop, spp=spp, **kw)
    sa = sc.stats()
    b = lj.render_samples(fresh, crop, spp=spp, **kw)
    sb = fresh.stats()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert (sa.rays_closest, sa.rays_shadow, sa.bounce_iterations) == (sb.rays_closest, sb.rays_shadow, sb.bounce_iterations)
    return a


@pytest.mark.parametrize("bvh8", [0, 1])
def test_renders_after_a_ploc_rebuild_equal_a_fresh_upload(bvh8, ctx, scenes, monkeypatch):
    hs, snap = scenes("synthetic")
    crop = (16, 16, 48, 48)
    monkeypatch.setenv("LJ_TUNE_BVH8", str(bvh8))
    sc = lj.Scene(ctx, hs)
    still = lj.render_samples(sc, crop, spp=8)
    apply_motion(hs, snap, "M2")
    sc.update_geometry(hs, rebuild="ploc")
    assert lj.rebuild_stats(sc).rebuilt == 1 and lj.build_stats(sc).builder == 1
    fresh = lj.Scene(ctx, hs)
    moved = _render_pair(sc, fresh, crop, 8)
    assert not np.array_equal(still, moved), "the motion is not visible in the crop: the comparison shows nothing"
    if bvh8:
        return
    c = hs.desc.camera
    cams = [lj.look_at_camera(o, (0.0, 0.0, 0.0), (0, 1, 0), 45.0, c.width, c.height, c.filter_kind, c.filter_param, c.medium_id) for o in ((0.4, 2.2, 3.4), (-2.0, 2.5, 1.5))]
    a, b = lj.render_views(sc, cams, spp=2, crop=crop), lj.render_views(fresh, cams, spp=2, crop=crop)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and a.any()
    _render_pair(sc, fresh, crop, 2, rng_mode=lj.LJ_RNG_TILE)


def test_volumetric_renders_after_a_ploc_rebuild_equal_a_fresh_upload(ctx, scenes):
    hs, snap = scenes("vol_cbox_teapot")
    crop = (248, 300, 264, 316)
    sc = lj.Scene(ctx, hs)
    still = lj.render_samples(sc, crop, spp=4)
    apply_motion(hs, snap, "M2")
    sc.update_geometry(hs, rebuild="ploc")
    assert lj.rebuild_stats(sc).rebuilt == 1 and lj.build_stats(sc).builder == 1
    moved = _render_pair(sc, lj.Scene(ctx, hs), crop, 4)
    assert moved.any() and not np.array_equal(still, moved)


def test_a_leaf_scan_scene_is_left_untouched(ctx, scenes):
    hs, snap = scenes("cbox")
    sc = lj.Scene(ctx, hs)
    apply_motion(hs, snap, "M2")
    sc.update_geometry(hs)
    before = _structures(sc)
    assert len(before[2]) > 0
    sc.rebuild_bvh(builder="ploc")
    st, bs = lj.rebuild_stats(sc), lj.build_stats(sc)
    assert st.rebuilt == 0 and (bs.builder, bs.radius, bs.rounds) == (0, 0, 0)
    assert _structures(sc) == before


def test_refusals(ctx, scenes, inputs):
    lib = lj.load_library()
    ploc = _abi.LjRebuildArgs(_abi.LJ_BUILD_PLOC, 0)
    assert lib.lj_scene_rebuild_bvh_ex(None, C.byref(ploc)) == _abi.LJ_ERR_INVALID_ARG
    assert lib.lj_get_build_stats(None, None) == _abi.LJ_ERR_INVALID_ARG
    hs, snap = scenes("synthetic")
    sc = lj.Scene(ctx, hs)
    assert lj.build_stats(sc).rounds == 0 and lj.rebuild_stats(sc).rebuilt == 0, "zeros before the first rebuild"
    before = _structures(sc)
    for builder, radius, what in ((2, 0, b"unknown builder"), (-1, 0, b"unknown builder"), (_abi.LJ_BUILD_PLOC, 33, b"radius")):
        with pytest.raises(lj.LajollaError) as e:
            sc.rebuild_bvh(builder=builder, radius=radius)
        assert e.value.code == _abi.LJ_ERR_INVALID_ARG and what in lib.lj_last_error()
        with pytest.raises(lj.LajollaError) as e:
            lj.bvh_build_query(ctx, inputs["n9"], builder=builder, radius=radius)
        assert e.value.code == _abi.LJ_ERR_INVALID_ARG
    assert _structures(sc) == before and lj.rebuild_stats(sc).rebuilt == 0
    with pytest.raises(ValueError):
        sc.rebuild_bvh(builder="sah")
    with pytest.raises(ValueError):
        sc.update_geometry(hs, rebuild="sah")
    # a null or zeroed LjRebuildArgs is lj_scene_rebuild_bvh; radius <= 0 is the default; a radius is ignored by the linear builder
    assert lib.lj_scene_rebuild_bvh_ex(sc._h, None) == 0
    linear = _structures(sc)
    assert lib.lj_scene_rebuild_bvh_ex(sc._h, C.byref(_abi.LjRebuildArgs(0, 99))) == 0 and _structures(sc) == linear
    assert lib.lj_scene_rebuild_bvh_ex(sc._h, C.byref(_abi.LjRebuildArgs(1, -5))) == 0 and lj.build_stats(sc).radius == 8
