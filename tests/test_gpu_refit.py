"""lj_scene_update_geometry on the device: the refitted BVH4, BVH8 and leaf table equal the host twin's byte for byte, closest hits and
occlusion equal the oracle's of the moved description, and every per-sample radiance — through k_mega, the wavefront kernels over either
tree, the camera batch, the per-tile schedule and the volumetric tracer — is bit-identical to a fresh upload of the moved description:
the closest hit is the minimum of (t, primitive id) over everything a ray tests, so nothing depends on the tree a refit leaves behind."""
import ctypes as C

import numpy as np
import pytest

import lajolla_public_amd as lj
from lajolla_public_amd import _abi
from helpers import Oracle
from refit_common import MOTIONS, RefitTwin, apply_motion, load_scene, mixed_rays, shadow_rays, snapshot

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return lj.Context(0)


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    cache = {}

    def get(name):
        if name not in cache:
            hs = load_scene(name, tmp_path_factory.mktemp("refit"))
            cache[name] = (hs, snapshot(hs))
        hs, snap = cache[name]
        apply_motion(hs, snap, "M0")
        return hs, snap
    return get


def _upload(ctx, hs, monkeypatch, bvh8=None, mega=None):
    """A Scene; LJ_TUNE_BVH8 is read at upload, LJ_TUNE_MEGA at every render (the caller keeps it set)."""
    if bvh8 is not None:
        monkeypatch.setenv("LJ_TUNE_BVH8", str(bvh8))
    if mega is not None:
        monkeypatch.setenv("LJ_TUNE_MEGA", str(mega))
    sc = lj.Scene(ctx, hs)
    if bvh8 is not None:
        monkeypatch.delenv("LJ_TUNE_BVH8")
    return sc


def _same_samples(a, sa, b, sb):
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert (sa.rays_closest, sa.rays_shadow, sa.bounce_iterations) == (sb.rays_closest, sb.rays_shadow, sb.bounce_iterations)


def _render_pair(sc, fresh, crop, spp, **kw):
    a = lj.render_samples(sc, crop, spp=spp, **kw)
    sa = sc.stats()
    b = lj.render_samples(fresh, crop, spp=spp, **kw)
    _same_samples(a, sa, b, fresh.stats())
    return a


@pytest.mark.parametrize("name", ["cbox", "synthetic"])
def test_device_structures_equal_the_twins(name, ctx, scenes):
    hs, snap = scenes(name)
    sc, tw = lj.Scene(ctx, hs), RefitTwin(hs)
    for w in (0, 1, 2):
        assert lj.read_bvh(sc, w).tobytes() == tw.read(w).tobytes(), ("upload", w)
    for motion in MOTIONS:
        apply_motion(hs, snap, motion)
        sc.update_geometry(hs)
        assert tw.update(hs) == 0, tw.error
        for w in (0, 1, 2):
            assert lj.read_bvh(sc, w).tobytes() == tw.read(w).tobytes(), (motion, w)


@pytest.mark.parametrize("name,bvh8,motion,n_rays", [("cbox", None, "M1", 1 << 16), ("cbox", None, "M2", 1 << 16), ("veach_mi", None, "M3", 1 << 16), ("veach_mi", None, "M2", 1 << 16),
                                                     ("synthetic", 0, "M2", 1 << 16), ("synthetic", 1, "M2", 1 << 16), ("synthetic", 0, "M1", 1 << 16),
                                                     ("synthetic", 1, "M3", 1 << 16), ("disney_bsdf", 1, "M2", 1 << 17)])
def test_hits_after_an_update_equal_the_oracle(name, bvh8, motion, n_rays, ctx, scenes, monkeypatch):
    hs, snap = scenes(name)
    sc = _upload(ctx, hs, monkeypatch, bvh8=bvh8)
    apply_motion(hs, snap, motion)
    sc.update_geometry(hs)
    o = Oracle(hs)
    assert np.isclose(sc.info.bounds_radius, o.tables()["bounds_radius"], rtol=1e-12) and np.isclose(sc.info.shadow_epsilon, o.tables()["shadow_epsilon"], rtol=1e-12)
    rays = mixed_rays(hs, snap, n_rays, 31, o)
    hg, ho = lj.intersect(sc, rays["org"], rays["dir"], 0.0, np.inf), o.intersect(rays)
    assert (ho["shape_id"] >= 0).mean() > 0.2
    for f in ("t", "u", "v", "shape_id", "prim_id"):
        assert np.array_equal(hg[f].view(np.uint32), ho[f].view(np.uint32)), f
    r2 = shadow_rays(hs, 50000, 32, o)
    assert np.array_equal(lj.occluded(sc, r2["org"], r2["dir"], r2["tnear"], r2["tfar"]), o.occluded(r2))


@pytest.mark.parametrize("name,motion,bvh8,mega,crop", [("cbox", "M2", None, None, (224, 232, 256, 264)), ("cbox", "M2", None, 0, (224, 232, 256, 264)),
                                                        ("cbox", "M1", None, None, (224, 232, 256, 264)), ("veach_mi", "M3", None, None, (300, 200, 332, 232)),
                                                        ("synthetic", "M2", 0, None, (16, 16, 48, 48)), ("synthetic", "M2", 1, None, (16, 16, 48, 48)),
                                                        ("synthetic", "M1", 1, None, (16, 16, 48, 48)), ("cbox", "M4", None, None, (224, 232, 256, 264))])
def test_renders_after_an_update_equal_a_fresh_upload(name, motion, bvh8, mega, crop, ctx, scenes, monkeypatch):
    hs, snap = scenes(name)
    sc = _upload(ctx, hs, monkeypatch, bvh8=bvh8, mega=mega)
    still = lj.render_samples(sc, crop, spp=8)
    apply_motion(hs, snap, motion)
    sc.update_geometry(hs)
    fresh = _upload(ctx, hs, monkeypatch, bvh8=bvh8, mega=mega)
    moved = _render_pair(sc, fresh, crop, 8)
    assert not np.array_equal(still, moved), "the motion is not visible in the crop: the comparison shows nothing"
    assert sc.info.bounds_radius == fresh.info.bounds_radius and list(sc.info.bounds_center) == list(fresh.info.bounds_center)
    assert sc.info.shadow_epsilon == fresh.info.shadow_epsilon
    if motion == "M4":   # the emitter's tables: sampled positions, pdf, pmf
        rng = np.random.default_rng(9)
        q = np.zeros(2000, lj.LIGHT_QUERY)
        q["light_id"] = rng.integers(0, hs.desc.n_lights, len(q))
        q["ref"] = rng.normal(size=(len(q), 3)) * sc.info.bounds_radius * 0.3 + np.array(list(sc.info.bounds_center))
        q["rnd_uv"], q["rnd_w"] = rng.random((len(q), 2)), rng.random(len(q))
        q["view_dir"] = (0.0, -1.0, 0.0)
        a, b = lj.light_queries(sc, q), lj.light_queries(fresh, q)
        assert a.tobytes() == b.tobytes() and np.isfinite(a["pdf"]).all()


def test_other_entry_points_see_the_update(ctx, scenes):
    hs, snap = scenes("cbox")
    sc = lj.Scene(ctx, hs)
    apply_motion(hs, snap, "M1")
    sc.update_geometry(hs)
    fresh = lj.Scene(ctx, hs)
    c = hs.desc.camera
    cams = [lj.look_at_camera(o, (278.0, 273.0, 280.0), (0, 1, 0), 39.3, c.width, c.height, c.filter_kind, c.filter_param, c.medium_id)
            for o in ((278.0, 273.0, -800.0), (60.0, 420.0, -700.0))]   # two views into the box from its open side
    crop = (224, 232, 256, 264)
    a, b = lj.render_views(sc, cams, spp=2, crop=crop), lj.render_views(fresh, cams, spp=2, crop=crop)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and a.any()
    ta = lj.render_samples(sc, crop, spp=2, rng_mode=lj.LJ_RNG_TILE)
    sa = sc.stats()
    tb = lj.render_samples(fresh, crop, spp=2, rng_mode=lj.LJ_RNG_TILE)
    _same_samples(ta, sa, tb, fresh.stats())
    o = Oracle(hs)
    rays = mixed_rays(hs, snap, 8000, 41, o)
    h = lj.intersect(sc, rays["org"], rays["dir"], 0.0, np.inf)
    keep = np.flatnonzero(h["shape_id"] >= 0)[:1000]
    assert len(keep) == 1000
    q = np.zeros(len(keep), lj.HIT_QUERY)
    q["org"], q["dir"] = rays["org"][keep], rays["dir"][keep]
    for f in ("t", "u", "v"):
        q[f] = h[f][keep]
    q["ray_spread"], q["shape_id"], q["primitive_id"] = 1e-3, h["shape_id"][keep], h["prim_id"][keep]
    assert lj.vertex_queries(sc, q).tobytes() == lj.vertex_queries(fresh, q).tobytes()


@pytest.mark.parametrize("name,motion,crop", [("volpath_test4", "M3", (240, 240, 256, 256)), ("vol_cbox", "M2", (248, 300, 264, 316))])
def test_volumetric_renders_after_an_update_equal_a_fresh_upload(name, motion, crop, ctx, scenes):
    hs, snap = scenes(name)
    sc = lj.Scene(ctx, hs)
    apply_motion(hs, snap, motion)
    sc.update_geometry(hs)
    out = _render_pair(sc, lj.Scene(ctx, hs), crop, 4)
    assert out.any()


def test_sequences_refusals_and_bad_handles(ctx, scenes):
    hs, snap = scenes("cbox")
    crop = (224, 232, 256, 264)
    sc = lj.Scene(ctx, hs)
    never = lj.render_samples(sc, crop, spp=8)
    for motion, reset in (("M1", True), ("M2", False), ("M0", True)):   # M5
        apply_motion(hs, snap, motion, reset=reset)
        sc.update_geometry(hs)
    assert np.array_equal(lj.render_samples(sc, crop, spp=8).view(np.uint32), never.view(np.uint32))
    # a refused update: nothing on the device moves
    apply_motion(hs, snap, "M2")
    sc.update_geometry(hs)
    before = [lj.read_bvh(sc, w).tobytes() for w in (0, 1, 2)]
    image, radius = lj.render_samples(sc, crop, spp=8), sc.info.bounds_radius
    apply_motion(hs, snap, "M1")
    keep, hs.desc.indices[4] = hs.desc.indices[4], (hs.desc.indices[4] + 1) % 3
    with pytest.raises(lj.LajollaError) as e:
        sc.update_geometry(hs)
    hs.desc.indices[4] = keep
    assert e.value.code == _abi.LJ_ERR_INVALID_ARG
    hs.desc.positions[7] = float("nan")
    with pytest.raises(lj.LajollaError) as e:
        sc.update_geometry(hs)
    assert e.value.code == _abi.LJ_ERR_INVALID_ARG
    apply_motion(hs, snap, "M0")
    assert [lj.read_bvh(sc, w).tobytes() for w in (0, 1, 2)] == before
    assert np.array_equal(lj.render_samples(sc, crop, spp=8).view(np.uint32), image.view(np.uint32)) and sc.info.bounds_radius == radius
    # null and destroyed handles are errors, not crashes
    lib = lj.load_library()
    n = C.c_int64()
    assert lib.lj_scene_update_geometry(None, hs.desc_ptr) == _abi.LJ_ERR_INVALID_ARG
    assert lib.lj_scene_update_geometry(sc._h, None) == _abi.LJ_ERR_INVALID_ARG
    assert lib.lj_scene_read_bvh(None, 0, None, 0, C.byref(n)) == _abi.LJ_ERR_INVALID_ARG
    gone = lj.Scene(ctx, hs)
    handle = C.c_void_p(gone._h.value)
    del gone
    assert lib.lj_scene_update_geometry(handle, hs.desc_ptr) == _abi.LJ_ERR_INVALID_ARG and b"destroyed" in lib.lj_last_error()
    assert lib.lj_scene_read_bvh(handle, 0, None, 0, C.byref(n)) == _abi.LJ_ERR_INVALID_ARG
