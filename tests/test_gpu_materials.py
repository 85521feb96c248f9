"""Every Material alternative and every shading feature set (device/dshade.h: FeatLambert ... FeatAll) inside the GPU integrator, kernel plan
by kernel plan, on the 36-triangle cbox re-materialised as in tests/materials_common.py.

Yardsticks: the oracle's per-sample radiance under the same pcg32 streams, at the bars the host twin is held to (tests/test_materials_parity.py);
and bit-identity — per-sample radiance as uint32 — between everything that must not change a sample: k_mega and the wavefront kernels, the
whole-segment sort, the per-chunk sort and the fused tail, lanes, pool sizes, rank shares, a batch of cameras and its single renders, a table
of rays and the camera samples it was made from, tables staged in LDS and read from global memory, a feature set and FeatAll.

Nothing is forced onto a feature set that does not cover the scene: LJ_TUNE_SHADE_VARIANT is only ever set to 5 (FeatAll), except in the one
test that checks that an uncovering value is ignored.  It is read at upload, so every setting of it gets a scene of its own."""
import numpy as np
import pytest

import lajolla_public_amd as lj
from lajolla_public_amd import _abi
from helpers import Oracle, plan_ran, with_materials
from materials_common import CROP, EXPECTED_VARIANT, MATERIALS, SPP, case_scene, check_against_oracle
from rays_common import camera_sample_rays
from views_common import UP, cbox_cameras, set_host_camera

pytestmark = pytest.mark.gpu

CASES = ["cbox"] + sorted(MATERIALS)
PER_VARIANT = ["cbox", "roughplastic", "lambert_checker", "roughdielectric", "disneybsdf", "disneyglass"]   # variants 0 .. 5
SORTING = ["roughplastic", "roughdielectric", "disneybsdf", "disneyglass"]                                  # variants 1, 3, 4, 5: ShadeSorted
ALL = 5
# Feature sets whose samples are NOT all the bits of FeatAll's (DESIGN.md section 6 has the measured shares and the operation): the three
# without roughplastic.  They are held to the oracle's bars under both sets, and to every bit-identity below under their own.
CONTRACTED_OTHERWISE = (0, 2, 4)
TUNABLES = ("LJ_TUNE_MEGA", "LJ_TUNE_SHADE_SORT", "LJ_TUNE_TAIL", "LJ_TUNE_TAIL_FRAC", "LJ_TUNE_OCTANT_BIN", "LJ_TUNE_LANES", "LJ_TUNE_SHADE_VARIANT")


def same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


class Bench:
    """Per case: the oracle's samples of the crop, computed once, and the scene uploaded once per feature set it is asked for."""

    def __init__(self):
        self.ctx, self.refs, self.scenes, self.natural = lj.Context(0), {}, {}, {}

    def ref(self, name):
        if name not in self.refs:
            rc, _, ps, st = Oracle(case_scene(name)).render(spp=SPP, rng_mode=0, crop=CROP, per_sample=True)
            assert rc == 0
            ps.setflags(write=False)
            self.refs[name] = (ps, st.bounces)
        return self.refs[name]

    def upload(self, monkeypatch, hs, forced=None):
        """lj.Scene of a description, under LJ_TUNE_SHADE_VARIANT=forced (None: unset)."""
        if forced is None:
            monkeypatch.delenv("LJ_TUNE_SHADE_VARIANT", raising=False)
        else:
            monkeypatch.setenv("LJ_TUNE_SHADE_VARIANT", str(forced))
        sc = lj.Scene(self.ctx, hs)
        monkeypatch.delenv("LJ_TUNE_SHADE_VARIANT", raising=False)
        return sc

    def scene(self, monkeypatch, name, forced=None):
        if (name, forced) not in self.scenes:
            self.scenes[(name, forced)] = self.upload(monkeypatch, case_scene(name), forced)
        return self.scenes[(name, forced)]

    def natural_samples(self, monkeypatch, name):
        """The wavefront kernels' samples of the crop under the case's own feature set."""
        if name not in self.natural:
            monkeypatch.setenv("LJ_TUNE_MEGA", "0")
            self.natural[name] = lj.render_samples(self.scene(monkeypatch, name), CROP, spp=SPP)
            self.natural[name].setflags(write=False)
        return self.natural[name]


@pytest.fixture(scope="module")
def bench():
    return Bench()


@pytest.fixture(autouse=True)
def clean_environment(monkeypatch):
    for k in TUNABLES:
        monkeypatch.delenv(k, raising=False)


def use_plan(monkeypatch, plan):
    if plan == "wavefront":
        monkeypatch.setenv("LJ_TUNE_MEGA", "0")
    else:
        monkeypatch.delenv("LJ_TUNE_MEGA", raising=False)


# ---------------------------------------------------------------- a. against the oracle, both plans
@pytest.mark.parametrize("plan", ["mega", "wavefront"])
@pytest.mark.parametrize("name", CASES)
def test_case_against_the_oracle(bench, monkeypatch, name, plan):
    sc = bench.scene(monkeypatch, name)
    assert lj.scene_shade_variant(sc) == EXPECTED_VARIANT[name]
    use_plan(monkeypatch, plan)
    got = lj.render_samples(sc, CROP, spp=SPP)
    st = sc.stats()
    assert plan_ran(st, plan), (name, plan, st.mega_launches, st.shade_launches)
    ps, ref_bounces = bench.ref(name)
    check_against_oracle(name, got, ps, st.bounce_iterations, ref_bounces)


# ---------------------------------------------------------------- b. the same case under FeatAll
@pytest.mark.parametrize("name", CASES)
def test_case_under_the_all_features_set(bench, monkeypatch, name):
    """FeatAll differs from a smaller set only in the code the smaller one leaves out, so the samples must be the same bits."""
    sc = bench.scene(monkeypatch, name, forced=ALL)
    assert lj.scene_shade_variant(sc) == ALL
    natural = bench.natural_samples(monkeypatch, name)
    monkeypatch.setenv("LJ_TUNE_MEGA", "0")
    got = lj.render_samples(sc, CROP, spp=SPP)
    st = sc.stats()
    assert plan_ran(st, "wavefront")
    ps, ref_bounces = bench.ref(name)
    check_against_oracle(name, got, ps, st.bounce_iterations, ref_bounces)
    identical = (got.view(np.uint32) == natural.view(np.uint32)).all(axis=-1).mean()
    print(f"{name}: {100 * identical:.3f} % of the samples under FeatAll are bit-identical to those under variant {EXPECTED_VARIANT[name]}")
    if EXPECTED_VARIANT[name] not in CONTRACTED_OTHERWISE:
        assert identical == 1.0, identical


# ---------------------------------------------------------------- c. plans agree bit for bit, per feature set
@pytest.mark.parametrize("name", PER_VARIANT)
def test_plans_agree_bit_for_bit(bench, monkeypatch, name):
    sc = bench.scene(monkeypatch, name)
    assert lj.scene_shade_variant(sc) == EXPECTED_VARIANT[name]
    spp = 16

    def run(plan, **env):
        use_plan(monkeypatch, plan)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        out = lj.render_samples(sc, CROP, spp=spp)
        st = sc.stats()
        for k in env:
            monkeypatch.delenv(k)
        assert plan_ran(st, plan), (name, plan, env)
        return out, (st.bounce_iterations, st.rays_closest, st.rays_shadow)

    mega, mega_counts = run("mega")
    assert np.isfinite(mega).all() and mega.mean() > 0
    differing = []
    for env in ({}, {"LJ_TUNE_SHADE_SORT": "1"}, {"LJ_TUNE_TAIL": "0"}, {"LJ_TUNE_TAIL_FRAC": "16"}, {"LJ_TUNE_OCTANT_BIN": "1"}):
        out, counts = run("wavefront", **env)
        if not same(out, mega):
            differing.append((env, "samples", int((out.view(np.uint32) != mega.view(np.uint32)).any(axis=-1).sum())))
        if counts != mega_counts:
            differing.append((env, "counters", counts, mega_counts))
    assert not differing, differing


# ---------------------------------------------------------------- d. segments of several chunks
@pytest.mark.parametrize("name", SORTING)
def test_full_frame_of_a_sorting_feature_set(bench, monkeypatch, name):
    """512 x 512 at 8 spp: 2 M samples, two lanes, segments of 1024 slots — the whole-segment sort crosses chunks, which a crop never shows."""
    sc = bench.scene(monkeypatch, name)
    spp = 8
    use_plan(monkeypatch, "wavefront")
    base = lj.render(sc, spp=spp)
    st = sc.stats()
    assert plan_ran(st, "wavefront") and st.samples == 512 * 512 * spp and np.isfinite(base).all()
    differing = []
    monkeypatch.setenv("LJ_TUNE_SHADE_SORT", "1")
    differing += [] if same(base, lj.render(sc, spp=spp)) else ["per-chunk sort"]
    monkeypatch.delenv("LJ_TUNE_SHADE_SORT")
    monkeypatch.setenv("LJ_TUNE_LANES", "1")
    differing += [] if same(base, lj.render(sc, spp=spp)) else ["one lane"]
    monkeypatch.delenv("LJ_TUNE_LANES")
    for pool in (1 << 16, 3 << 18):
        differing += [] if same(base, lj.render(sc, spp=spp, pool_paths=pool)) else [f"pool {pool}"]
    acc = np.zeros_like(base)
    for r in range(3):
        acc += lj.render(sc, spp=spp, rank=r, world_size=3)
    differing += [] if same(base, acc) else ["sum of three rank shares"]
    use_plan(monkeypatch, "mega")
    frame = lj.render(sc, spp=spp)
    assert plan_ran(sc.stats(), "mega")
    differing += [] if same(base, frame) else ["k_mega"]
    assert not differing, differing


# ---------------------------------------------------------------- e. the VIEWS and RAYS instantiations
FILM = (96, 64)
VIEWS = (0, 3)                # the scene's own pose, and one from inside the box
# The rays test needs ray i = sample i of the window (its stream is i * spp + s, rays_common.camera_sample_rays), so the window is the film's
# first rows, and the camera looks at the tall box through a 10 degree lens, so that those rows lie on the re-materialised box
RAYS_CROP, RAYS_SPP = (0, 0, FILM[0], 3), 5   # 96 x 3 pixels at 5 spp: 1440 rays, no multiple of 64
RAYS_VIEW = ((278, 273, -800), (368, 165, 351), 10.0)
ON_FILM = PER_VARIANT[1:]     # variants 1 .. 5 (cbox itself, variant 0: tests/test_gpu_views.py and tests/test_gpu_rays.py)


def film_scene(name, view):
    hs = case_scene(name)
    return set_host_camera(hs, cbox_cameras(hs, *FILM)[view])


@pytest.mark.parametrize("plan", ["mega", "wavefront"])
@pytest.mark.parametrize("name", ON_FILM)
def test_batch_of_cameras_equals_the_single_renders(bench, monkeypatch, name, plan):
    singles = [bench.upload(monkeypatch, film_scene(name, v)) for v in VIEWS]
    cams = [cbox_cameras(case_scene(name), *FILM)[v] for v in VIEWS]
    assert lj.scene_shade_variant(singles[0]) == EXPECTED_VARIANT[name]
    use_plan(monkeypatch, plan)
    batch = lj.render_views(singles[0], cams, spp=5)
    st = singles[0].stats()
    assert plan_ran(st, plan) and st.samples == 2 * FILM[0] * FILM[1] * 5
    assert batch.shape == (2, FILM[1], FILM[0], 3) and np.isfinite(batch).all() and not same(batch[0], batch[1])
    for i, sc in enumerate(singles):
        one = lj.render(sc, spp=5)
        assert plan_ran(sc.stats(), plan)
        assert same(batch[i], one), (name, plan, VIEWS[i])


class SceneQueries:
    """pcg32 and primary-ray queries of an uploaded scene, as rays_common.camera_sample_rays asks for them."""

    def __init__(self, ctx, scene):
        self.ctx, self.scene = ctx, scene

    def pcg32(self, streams, count, seed=0):
        return lj.pcg32_queries(self.ctx, streams, count, seed)

    def primary(self, q):
        return lj.primary_ray_queries(self.scene, q)


@pytest.mark.parametrize("name", ON_FILM)
def test_camera_samples_fed_back_as_rays_are_the_render(bench, monkeypatch, name):
    hs = case_scene(name)
    c = hs.desc.camera
    set_host_camera(hs, lj.look_at_camera(RAYS_VIEW[0], RAYS_VIEW[1], UP, RAYS_VIEW[2], FILM[0], FILM[1], c.filter_kind, c.filter_param, c.medium_id))
    sc = bench.upload(monkeypatch, hs)
    ref = lj.render_samples(sc, RAYS_CROP, spp=RAYS_SPP).reshape(-1, 3)
    assert plan_ran(sc.stats(), "mega") and np.isfinite(ref).all() and ref.max() > 0
    rays = camera_sample_rays(SceneQueries(bench.ctx, sc), hs, crop=RAYS_CROP, spp=RAYS_SPP)
    assert rays.shape == (FILM[0] * 3 * RAYS_SPP, 6)
    out = lj.radiance_rays(sc, rays[:, :3], rays[:, 3:], spp=1, samples=True)
    st = sc.stats()
    assert plan_ran(st, "wavefront") and st.samples == len(rays)
    assert same(out["samples"].reshape(-1, 3), ref)


# ---------------------------------------------------------------- f. tables in global memory, with real materials
def material_dict(m):
    """LjMaterial -> the dict helpers.material_struct builds it from (float32 fields: the round trip is exact)."""
    kind = _abi.MATERIAL_KINDS[m.kind]
    d = dict(kind=kind, eta=m.eta)
    for i, slot in enumerate(_abi.MATERIAL_SLOTS[kind]):
        t = m.tex[i]
        d[slot] = {"kind": ("constant", "image", "checkerboard")[t.kind], "texture_id": t.texture_id, "value": list(t.value), "color1": list(t.color1),
                   "uscale": t.uscale, "vscale": t.vscale, "uoffset": t.uoffset, "voffset": t.voffset}
    return d


def test_material_table_too_large_to_stage(bench, monkeypatch):
    """48 materials of 592 bytes exceed the 24 KiB the shade tables may take of LDS: k_shade<FeatAll, 0> reads them from global memory.  The
    shapes keep materials 0 - 4, so the oracle's samples of "disneybsdf" are the yardstick, and k_shade<FeatAll, 2> on the unpadded scene
    must give the same bits."""
    name = "disneybsdf"
    hs = case_scene(name)
    own = [material_dict(hs.desc.materials[i]) for i in range(hs.desc.n_materials)]
    assert len(own) == 5
    with_materials(hs, [own[i % 5] for i in range(48)])
    assert hs.desc.n_materials == 48
    sc = bench.upload(monkeypatch, hs)
    assert lj.scene_shade_variant(sc) == ALL
    got = lj.render_samples(sc, CROP, spp=SPP)
    st = sc.stats()
    assert plan_ran(st, "wavefront")     # (k_mega is enabled, but takes only scenes whose tables it can stage)
    ps, ref_bounces = bench.ref(name)
    check_against_oracle(name, got, ps, st.bounce_iterations, ref_bounces)
    staged = bench.scene(monkeypatch, name, forced=ALL)
    monkeypatch.setenv("LJ_TUNE_MEGA", "0")
    want = lj.render_samples(staged, CROP, spp=SPP)
    assert plan_ran(staged.stats(), "wavefront")
    assert same(got, want), int((got.view(np.uint32) != want.view(np.uint32)).any(axis=-1).sum())


# ---------------------------------------------------------------- the override takes only a feature set that covers the scene
@pytest.mark.parametrize("forced", [4, 0, 9, -1])
def test_override_that_does_not_cover_the_scene_is_ignored(bench, monkeypatch, forced):
    """FeatDisney (4) has no roughplastic; max(variant, override) used to take it, and the whole-segment sort then had no slot for such a path."""
    name = "roughplastic"
    sc = bench.upload(monkeypatch, case_scene(name), forced=forced)
    assert lj.scene_shade_variant(sc) == EXPECTED_VARIANT[name] == 1
    for plan in ("wavefront", "mega"):
        use_plan(monkeypatch, plan)
        got = lj.render_samples(sc, CROP, spp=SPP)
        assert plan_ran(sc.stats(), plan)
        assert same(got, lj.render_samples(bench.scene(monkeypatch, name), CROP, spp=SPP)), (forced, plan)
