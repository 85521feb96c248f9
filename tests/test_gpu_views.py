"""Camera batches on the device: lj_render_views renders n cameras of one uploaded scene in one pass, lj_scene_set_camera moves the
camera of an uploaded scene.  The yardstick is exact: view v of a batch, and a render after set_camera, must equal — bit for bit — the render
of the scene uploaded with that camera (same pcg32 streams, same arithmetic; the resolve's per-pixel sum order does not depend on where
a pixel sits in the list).  One check against the oracle is independent of the library's single-camera path.

Film 47 x 41 (tests/views_common.py): waves, k_mega's grab ranges and the wavefront blocks' sample ranges all straddle view boundaries."""
import numpy as np
import pytest

import lajolla_public_amd as lj
from lajolla_public_amd import _abi
from helpers import Oracle
from views_common import W, H, cameras_for, host_scene_with, scene_file

pytestmark = pytest.mark.gpu

SPP = 5


@pytest.fixture(scope="module")
def ctx():
    return lj.Context(0)


class Bench:
    """Per scene: the four cameras, the scene uploaded once per camera (the reference route), reference renders computed once."""

    def __init__(self, ctx):
        self.ctx, self.cams, self.scenes, self.renders = ctx, {}, {}, {}

    def cameras(self, name):
        if name not in self.cams:
            hs = lj.parse_scene(scene_file(name))
            radius = None
            if name not in ("cbox", "vol_cbox"):
                radius = lj.Scene(self.ctx, hs).info.bounds_radius
            self.cams[name] = cameras_for(name, hs, radius)
        return self.cams[name]

    def scene(self, name, v, integrator=None):
        key = (name, v, integrator)
        if key not in self.scenes:
            hs = host_scene_with(name, self.cameras(name)[v])
            if integrator is not None:
                hs.desc.options.integrator = integrator
            self.scenes[key] = lj.Scene(self.ctx, hs)
        return self.scenes[key]

    def single(self, name, v, tag="", integrator=None, **kw):
        """render() of the scene uploaded with camera v; `tag` separates renders made under another environment"""
        key = (name, v, tag, integrator, tuple(sorted(kw.items())))
        if key not in self.renders:
            self.renders[key] = lj.render(self.scene(name, v, integrator), **kw)
        return self.renders[key]


@pytest.fixture(scope="module")
def bench(ctx):
    return Bench(ctx)


def same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------- batch == single renders
@pytest.mark.parametrize("name,mega", [("cbox", True), ("cbox", False), ("veach_mi", True), ("disney_bsdf", True), ("vol_cbox", True)])
def test_batch_equals_single_renders(bench, monkeypatch, name, mega):
    if not mega:
        monkeypatch.setenv("LJ_TUNE_MEGA", "0")   # the wavefront kernels over the BVH4 instead of k_mega
    cams = bench.cameras(name)
    sc = bench.scene(name, 0)
    batch = lj.render_views(sc, cams, spp=SPP)
    st = sc.stats()
    assert batch.shape == (4, H, W, 3) and np.isfinite(batch).all()
    assert st.samples == 4 * W * H * SPP
    if name in ("cbox", "veach_mi"):   # what actually ran
        assert (st.mega_launches == 1 and st.shade_launches == 0) if mega else (st.mega_launches == 0 and st.shade_launches > 0)
    if name == "disney_bsdf":
        assert st.mega_launches == 0 and st.shade_launches > 0
    for v in range(4):
        assert same(batch[v], bench.single(name, v, tag="" if mega else "nomega", spp=SPP)), (name, v)
    assert not same(batch[0], batch[1])


@pytest.mark.parametrize("integrator", [_abi.LJ_INTEGRATOR_DEPTH, _abi.LJ_INTEGRATOR_SHADING_NORMAL])
def test_batch_of_auxiliary_buffers(bench, integrator):
    cams = bench.cameras("cbox")
    batch = lj.render_views(bench.scene("cbox", 0, integrator), cams)
    for v in range(4):
        assert same(batch[v], bench.single("cbox", v, integrator=integrator)), v
    assert batch.any() and not same(batch[0], batch[3])


def test_one_view_and_a_repeated_camera(bench):
    cams = bench.cameras("cbox")
    sc = bench.scene("cbox", 0)
    one = lj.render_views(sc, [cams[2]], spp=SPP)
    assert same(one[0], bench.single("cbox", 2, spp=SPP))
    batch = lj.render_views(sc, [cams[1], cams[3], cams[1], cams[0]], spp=SPP)
    assert same(batch[0], batch[2]) and same(batch[0], bench.single("cbox", 1, spp=SPP)) and same(batch[1], bench.single("cbox", 3, spp=SPP))


# ---------------------------------------------------------------- set_camera == re-upload
@pytest.mark.parametrize("name", ["cbox", "disney_bsdf"])
def test_set_camera_equals_reupload(ctx, bench, name):
    cams = bench.cameras(name)
    sc = lj.Scene(ctx, host_scene_with(name, cams[0]))
    crop = (11, 7, 27, 15)   # 16 x 8
    rng = np.random.default_rng(5)
    q = np.zeros(64, lj.PRIMARY_QUERY)
    q["x"], q["y"] = rng.integers(0, W, 64), rng.integers(0, H, 64)
    q["jx"], q["jy"] = rng.random(64), rng.random(64)
    for v in (1, 3, 0):
        sc.set_camera(cams[v])
        ref = bench.scene(name, v)
        assert (sc.info.width, sc.info.height) == (W, H)
        assert same(lj.render(sc, spp=SPP), bench.single(name, v, spp=SPP)), (name, v)
        assert same(lj.render_samples(sc, crop, spp=3), lj.render_samples(ref, crop, spp=3)), (name, v)
        a, b = lj.primary_ray_queries(sc, q), lj.primary_ray_queries(ref, q)
        assert a.tobytes() == b.tobytes(), (name, v)
        assert same(lj.render(sc, rng_mode=lj.LJ_RNG_TILE, spp=2), lj.render(ref, rng_mode=lj.LJ_RNG_TILE, spp=2)), (name, v)


@pytest.mark.parametrize("name", ["cbox", "disney_bsdf"])
def test_set_camera_changes_the_film_size(ctx, bench, name):
    hs0 = lj.parse_scene(scene_file(name))
    radius = bench.scene(name, 0).info.bounds_radius
    small, wide = bench.cameras(name), cameras_for(name, hs0, radius, 64, 32)
    sc = lj.Scene(ctx, host_scene_with(name, small[1]))
    first = lj.render(sc, spp=2)
    sc.set_camera(wide[1])
    assert (sc.info.width, sc.info.height) == (64, 32)
    img = lj.render(sc, spp=2)
    assert img.shape == (32, 64, 3) and same(img, lj.render(lj.Scene(ctx, host_scene_with(name, wide[1])), spp=2))
    sc.set_camera(small[1])
    again = lj.render(sc, spp=2)
    assert same(again, first) and same(again, bench.single(name, 1, spp=2))


# ---------------------------------------------------------------- shapes that can go wrong
def test_pass_boundary_inside_a_view(bench, monkeypatch):
    monkeypatch.setenv("LJ_TUNE_PASS_SAMPLES", "4096")   # 819 pixels a pass: boundaries inside every view
    for name, mega in (("cbox", True), ("cbox", False), ("vol_cbox", True)):
        if not mega:
            monkeypatch.setenv("LJ_TUNE_MEGA", "0")
        else:
            monkeypatch.delenv("LJ_TUNE_MEGA", raising=False)
        cams = bench.cameras(name)[:3]
        sc = bench.scene(name, 0)
        batch = lj.render_views(sc, cams, spp=SPP)
        assert sc.stats().samples == 3 * W * H * SPP and sc.stats().wavefront_steps >= 8
        for v in range(3):
            # (the reference renders are single-pass ones: a sample's value does not depend on the pass it is in)
            assert same(batch[v], bench.single(name, v, tag="" if mega else "nomega", spp=SPP)), (name, mega, v)


@pytest.mark.parametrize("pool", [4096, 5000, 1 << 16])
def test_pool_sizes(bench, monkeypatch, pool):
    for name in ("cbox", "disney_bsdf"):
        if name == "cbox":
            monkeypatch.setenv("LJ_TUNE_MEGA", "0")   # (k_mega has no pool)
        else:
            monkeypatch.delenv("LJ_TUNE_MEGA", raising=False)
        batch = lj.render_views(bench.scene(name, 0), bench.cameras(name), spp=SPP, pool_paths=pool)
        for v in range(4):
            assert same(batch[v], bench.single(name, v, tag="nomega" if name == "cbox" else "", spp=SPP)), (name, pool, v)


@pytest.mark.parametrize("spp", [1, 2, 7])
def test_sample_counts(bench, monkeypatch, spp):
    for name, mega in (("cbox", True), ("cbox", False), ("vol_cbox", True)):
        if not mega:
            monkeypatch.setenv("LJ_TUNE_MEGA", "0")
        else:
            monkeypatch.delenv("LJ_TUNE_MEGA", raising=False)
        batch = lj.render_views(bench.scene(name, 0), bench.cameras(name), spp=spp)
        for v in range(4):
            assert same(batch[v], bench.single(name, v, tag="" if mega else "nomega", spp=spp)), (name, mega, spp, v)


def test_ranks_crop_and_seed(bench):
    for name in ("cbox", "disney_bsdf"):
        cams, sc = bench.cameras(name), bench.scene(name, 0)
        full = lj.render_views(sc, cams, spp=SPP)
        acc = np.zeros_like(full)
        for r in range(3):
            part = lj.render_views(sc, cams, spp=SPP, rank=r, world_size=3)
            for v in range(4):
                assert same(part[v], lj.render(bench.scene(name, v), spp=SPP, rank=r, world_size=3)), (name, r, v)
            acc += part
        assert same(acc, full)
        x0, y0, x1, y1 = crop = (5, 3, 40, 22)
        c = lj.render_views(sc, cams, spp=SPP, crop=crop)
        for v in range(4):
            assert same(c[v], lj.render(bench.scene(name, v), spp=SPP, crop=crop)), (name, v)
            assert same(c[v, y0:y1, x0:x1], full[v, y0:y1, x0:x1])
            outside = c[v].copy()
            outside[y0:y1, x0:x1] = 0
            assert not outside.any()
        s = lj.render_views(sc, cams, spp=SPP, seed=12345)
        assert not same(s, full)
        for v in range(4):
            assert same(s[v], bench.single(name, v, spp=SPP, seed=12345)), (name, v)


def test_render_views_device_into_a_torch_tensor(bench):
    import torch
    cams, sc = bench.cameras("cbox"), bench.scene("cbox", 0)
    out = torch.empty((4, H, W, 3), device="cuda", dtype=torch.float32)
    lj.render_views_device(sc, cams, out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream, spp=SPP)
    got = out.cpu().numpy()   # (on the current stream: ordered behind the render)
    assert same(got, lj.render_views(sc, cams, spp=SPP))


def test_declared_errors(bench):
    cams, sc = bench.cameras("cbox"), bench.scene("cbox", 0)
    hs = lj.parse_scene(scene_file("cbox"))
    wider = cameras_for("cbox", hs, None, W + 1, H)
    with pytest.raises(lj.LajollaError) as e:
        lj.render_views(sc, [cams[0], wider[1]], spp=1)
    assert e.value.code == _abi.LJ_ERR_INVALID_ARG
    bad = cameras_for("cbox", hs)[1]
    bad.cam_to_world[3] = float("nan")
    with pytest.raises(lj.LajollaError) as e:
        lj.render_views(sc, [cams[0], bad], spp=1)
    assert e.value.code == _abi.LJ_ERR_INVALID_ARG
    with pytest.raises(lj.LajollaError) as e:
        lj.render_views(sc, [], spp=1)
    assert e.value.code == _abi.LJ_ERR_INVALID_ARG
    with pytest.raises(lj.LajollaError) as e:
        lj.render_views(sc, cams, spp=1, rng_mode=lj.LJ_RNG_TILE)
    assert e.value.code == _abi.LJ_ERR_UNSUPPORTED
    with pytest.raises(lj.LajollaError) as e:
        sc.set_camera(bad)
    assert e.value.code == _abi.LJ_ERR_INVALID_ARG
    # the scene is as it was
    assert same(lj.render_views(sc, cams[:1], spp=SPP)[0], bench.single("cbox", 0, spp=SPP))


# ---------------------------------------------------------------- against the oracle, independent of the single-camera path
def test_batch_against_the_oracle(bench):
    cams = bench.cameras("cbox")
    spp = 16
    batch = lj.render_views(bench.scene("cbox", 0), [cams[1], cams[3]], spp=spp)
    for i, v in enumerate((1, 3)):
        rc, ref, _, _ = Oracle(host_scene_with("cbox", cams[v])).render(spp=spp, rng_mode=0)
        assert rc == 0
        l2 = np.linalg.norm(batch[i] - ref) / np.linalg.norm(ref)
        mean = abs(batch[i].mean() / ref.mean() - 1)
        print("view", v, "l2", l2, "mean", mean)
        assert l2 <= 1e-2, (v, l2)        # DEFAULT_BARS l2 / img_mean of tests/test_gpu_parity.py
        assert mean < 2e-4, (v, mean)
