"""lj_scene_rebuild_bvh on the device: the linear BVH of rebuild.hip equals the host twin's byte for byte, the rebuilt BVH4 and BVH8 equal
the twin's, closest hits and occlusion after an update and a rebuild equal the oracle's of the moved description, and every per-sample
radiance — through the wavefront kernels over either tree, the camera batch, the per-tile schedule and the volumetric tracer — is
bit-identical to a fresh upload: the closest hit is the minimum of (t, primitive id) over everything a ray tests, so nothing depends on
the tree.  A leaf-scan scene is left untouched."""
import ctypes as C
import os

import numpy as np
import pytest

import lajolla_public_amd as lj
from lajolla_public_amd import _abi
from helpers import Oracle
from refit_common import ROOT, apply_motion, load_scene, mixed_rays, shadow_rays, snapshot
from rebuild_common import RebuildTwin, check_binary_tree, query_inputs, twin_build

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return lj.Context(0)


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    cache = {}

    def get(name):
        if name not in cache:
            hs = lj.parse_scene(os.path.join(ROOT, "scenes", "volpath_test", name + ".xml")) if name == "vol_cbox_teapot" else load_scene(name, tmp_path_factory.mktemp("rebuild"))
            cache[name] = (hs, snapshot(hs))
        hs, snap = cache[name]
        apply_motion(hs, snap, "M0")
        return hs, snap
    return get


@pytest.fixture(scope="module")
def inputs():
    return query_inputs()


def _structures(sc):
    return [lj.read_bvh(sc, w).tobytes() for w in (0, 1, 2)]


def _same_samples(a, sa, b, sb):
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert (sa.rays_closest, sa.rays_shadow, sa.bounce_iterations) == (sb.rays_closest, sb.rays_shadow, sb.bounce_iterations)


def _render_pair(sc, fresh, crop, spp, **kw):
    a = lj.render_samples(sc, crop, spp=spp, **kw)
    sa = sc.stats()
    b = lj.render_samples(fresh, crop, spp=spp, **kw)
    _same_samples(a, sa, b, fresh.stats())
    return a


@pytest.mark.parametrize("name", ["n0", "n1", "n2", "n4", "n5", "n8", "n9", "coincident64", "one_axis257", "random1000", "pairs1000", "random100003"])
def test_build_query_equals_the_twin(name, ctx, inputs):
    boxes = inputs[name]
    order, nodes = lj.bvh_build_query(ctx, boxes)
    want_order, want_nodes = twin_build(boxes)
    assert order.tobytes() == want_order.tobytes()
    assert nodes.tobytes() == want_nodes.tobytes()
    check_binary_tree(order, nodes, len(boxes))


def test_structures_after_a_rebuild_equal_the_twins(ctx, scenes):
    hs, snap = scenes("synthetic")
    sc, tw = lj.Scene(ctx, hs), RebuildTwin(hs)

    def same(what):
        for w in (0, 1):
            assert lj.read_bvh(sc, w).tobytes() == tw.read(w).tobytes(), (what, w)
        assert len(lj.read_bvh(sc, 2)) == 0
    same("upload")
    apply_motion(hs, snap, "M2")
    sc.update_geometry(hs, rebuild=True)
    assert tw.update(hs) == 0 and tw.rebuild() == 0 and tw.rebuilt == 1, tw.error
    assert lj.rebuild_stats(sc).rebuilt == 1
    same("M2 + rebuild")
    # the stored boxes are the refit of the new topology: the same description again changes no byte
    rebuilt = _structures(sc)
    sc.update_geometry(hs)
    assert _structures(sc) == rebuilt
    apply_motion(hs, snap, "M1")
    sc.update_geometry(hs)
    assert tw.update(hs) == 0, tw.error
    same("rebuild + M1 update")
    sc.rebuild_bvh()
    assert tw.rebuild() == 0, tw.error
    same("second rebuild")
    twice = _structures(sc)
    sc.rebuild_bvh()
    assert _structures(sc) == twice, "two rebuilds of the same positions differ"


@pytest.mark.parametrize("name,bvh8,motion,n_rays", [("synthetic", 0, "M1", 1 << 16), ("synthetic", 0, "M2", 1 << 16), ("synthetic", 1, "M1", 1 << 16),
                                                     ("synthetic", 1, "M2", 1 << 16), ("disney_bsdf", 1, "M2", 1 << 17)])
def test_hits_after_a_rebuild_equal_the_oracle(name, bvh8, motion, n_rays, ctx, scenes, monkeypatch):
    hs, snap = scenes(name)
    monkeypatch.setenv("LJ_TUNE_BVH8", str(bvh8))   # read at upload and again at the rebuild
    sc = lj.Scene(ctx, hs)
    apply_motion(hs, snap, motion)
    sc.update_geometry(hs, rebuild=True)
    assert lj.rebuild_stats(sc).rebuilt == 1
    o = Oracle(hs)
    rays = mixed_rays(hs, snap, n_rays, 31, o)
    hg, ho = lj.intersect(sc, rays["org"], rays["dir"], 0.0, np.inf), o.intersect(rays)
    assert (ho["shape_id"] >= 0).mean() > 0.2
    for f in ("t", "u", "v", "shape_id", "prim_id"):
        assert np.array_equal(hg[f].view(np.uint32), ho[f].view(np.uint32)), f
    r2 = shadow_rays(hs, 50000, 32, o)
    assert np.array_equal(lj.occluded(sc, r2["org"], r2["dir"], r2["tnear"], r2["tfar"]), o.occluded(r2))


@pytest.mark.parametrize("bvh8", [0, 1])
def test_renders_after_a_rebuild_equal_a_fresh_upload(bvh8, ctx, scenes, monkeypatch):
    hs, snap = scenes("synthetic")
    crop = (16, 16, 48, 48)
    monkeypatch.setenv("LJ_TUNE_BVH8", str(bvh8))
    sc = lj.Scene(ctx, hs)
    still = lj.render_samples(sc, crop, spp=8)
    apply_motion(hs, snap, "M2")
    sc.update_geometry(hs, rebuild=True)
    assert lj.rebuild_stats(sc).rebuilt == 1
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


def test_volumetric_renders_after_a_rebuild_equal_a_fresh_upload(ctx, scenes):
    hs, snap = scenes("vol_cbox_teapot")
    crop = (248, 300, 264, 316)
    sc = lj.Scene(ctx, hs)
    assert len(lj.read_bvh(sc, 2)) == 0, "a leaf-scan scene"
    still = lj.render_samples(sc, crop, spp=4)
    apply_motion(hs, snap, "M2")
    sc.update_geometry(hs, rebuild=True)
    assert lj.rebuild_stats(sc).rebuilt == 1
    moved = _render_pair(sc, lj.Scene(ctx, hs), crop, 4)
    assert moved.any() and not np.array_equal(still, moved)


def test_a_leaf_scan_scene_is_left_untouched(ctx, scenes):
    hs, snap = scenes("cbox")
    crop = (224, 232, 256, 264)
    sc = lj.Scene(ctx, hs)
    apply_motion(hs, snap, "M2")
    sc.update_geometry(hs)
    before, image = _structures(sc), lj.render_samples(sc, crop, spp=8)
    assert len(before[2]) > 0
    sc.rebuild_bvh()
    st = lj.rebuild_stats(sc)
    assert st.rebuilt == 0 and st.n_nodes4 * 128 == len(before[0]) and st.n_nodes8 * 80 == len(before[1])
    assert _structures(sc) == before
    assert np.array_equal(lj.render_samples(sc, crop, spp=8).view(np.uint32), image.view(np.uint32))


def test_refusals_and_stats(ctx, scenes):
    lib = lj.load_library()
    assert lib.lj_scene_rebuild_bvh(None) == _abi.LJ_ERR_INVALID_ARG
    hs, snap = scenes("synthetic")
    gone = lj.Scene(ctx, hs)
    handle = C.c_void_p(gone._h.value)
    del gone
    assert lib.lj_scene_rebuild_bvh(handle) == _abi.LJ_ERR_INVALID_ARG and b"destroyed" in lib.lj_last_error()
    assert lib.lj_get_rebuild_stats(None, None) == _abi.LJ_ERR_INVALID_ARG
    bad = np.zeros((3, 2, 3), np.float32)
    bad[1, 0, 0] = np.nan
    with pytest.raises(lj.LajollaError) as e:
        lj.bvh_build_query(ctx, bad)
    assert e.value.code == _abi.LJ_ERR_INVALID_ARG
    sc = lj.Scene(ctx, hs)
    assert lj.rebuild_stats(sc).rebuilt == 0 and lj.rebuild_stats(sc).n_prims == 0, "zeros before the first rebuild"
    sc.rebuild_bvh()
    st, tw = lj.rebuild_stats(sc), RebuildTwin(hs)
    assert tw.rebuild() == 0
    info = tw.info()
    assert st.rebuilt == 1 and st.n_prims == 1155 == sc.info.n_triangles + sc.info.n_spheres
    assert st.n_nodes4 * 128 == len(lj.read_bvh(sc, 0)) and st.n_nodes8 * 80 == len(lj.read_bvh(sc, 1)) and st.n_nodes4 == sc.info.n_bvh_nodes
    assert (st.n_leaves, st.depth4, st.depth8) == (info["n_leaves"], info["depth4"], info["depth8"])
    assert st.build_ms > 0 and st.emit_ms > 0 and st.refit_ms > 0
    stats = sc.stats()
    assert stats.render_ms > 0 and stats.generate_ms > 0 and (stats.samples, stats.rays_closest, stats.rays_shadow, stats.extend_launches) == (0, 0, 0, 0)
