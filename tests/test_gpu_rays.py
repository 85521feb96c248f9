"""lj_radiance_rays / lj_irradiance / lj_probe_ray_queries on the GPU.

Yardsticks: lj_render_samples of the same uploaded scene, bit for bit, for the camera's own samples fed back as rays (cbox: the render runs
k_mega, the rays the wavefront kernels — the cross-plan check); lj_radiance_rays over lj_probe_ray_queries, bit for bit, for lj_irradiance;
the host twin (tests/twin_rays) at the bars tests/test_gpu_parity.py holds the device to against the oracle — median relative difference
< 2e-6, at most 2 % of the samples beyond 1e-3 (3 % volpath) — and 2e-5 on probe directions; float64 recomputation from the samples for the
two reductions, at the bounds of tests/test_gpu_features.py; bit-identical invariances.  564 rays: the first 3 rows of the 47 x 41 film at 4 spp."""
import ctypes as C

import numpy as np
import pytest

import lajolla_public_amd as lj
from lajolla_public_amd import _abi
from features_common import sum_bound, variance64
from rays_common import (CROP, LE, N_RAYS, PI_F, SENTINEL, SPP, TwinRays, bits, buffers, camera_sample_rays, cbox_probes, error_calls, film_scene, table)

pytestmark = pytest.mark.gpu


class SceneQueries:
    """pcg32 and primary-ray queries of an uploaded scene, in the interface of helpers.GpuQueries."""

    def __init__(self, ctx, scene):
        self.ctx, self.scene = ctx, scene

    def pcg32(self, streams, count, seed=0):
        return lj.pcg32_queries(self.ctx, streams, count, seed)

    def primary(self, q):
        return lj.primary_ray_queries(self.scene, q)


class Bench:
    def __init__(self):
        self.ctx = lj.Context(0)
        self._scenes, self._rays = {}, {}

    def scene(self, name):
        if name not in self._scenes:
            hs = film_scene(name)
            self._scenes[name] = (hs, lj.Scene(self.ctx, hs))
        return self._scenes[name]

    def rays(self, name):
        """The camera's samples of the window as rays, and lj_render_samples of the window — once per scene."""
        if name not in self._rays:
            hs, sc = self.scene(name)
            ref = lj.render_samples(sc, CROP, spp=SPP).reshape(-1, 3)
            st = sc.stats()
            self._rays[name] = (camera_sample_rays(SceneQueries(self.ctx, sc), hs), ref, st.mega_launches)
        return self._rays[name]


@pytest.fixture(scope="module")
def bench():
    return Bench()


def medium_of(hs):
    return hs.desc.camera.medium_id if hs.desc.options.integrator == _abi.LJ_INTEGRATOR_VOLPATH else None


@pytest.mark.parametrize("name", ["cbox", "disney", "veach_mi", "volpath_test2", "hetvol"])
def test_camera_samples_fed_back_as_rays_are_the_render_bit_for_bit(bench, name):
    hs, sc = bench.scene(name)
    rays, ref, mega_launches = bench.rays(name)
    assert rays.shape == (N_RAYS, 6) and np.isfinite(ref).all() and ref.max() > 0
    out = lj.radiance_rays(sc, rays[:, :3], rays[:, 3:], spp=1, samples=True, variance=True, medium_id=medium_of(hs))
    st = sc.stats()
    assert np.array_equal(bits(out["samples"].reshape(-1, 3)), bits(ref))
    assert np.array_equal(bits(out["radiance"]), bits(ref)) and not out["variance"].any()
    assert st.samples == N_RAYS and st.mega_launches == 0
    if name == "cbox":   # the cross-plan check: the render took the fused kernel, the rays the wavefront kernels
        assert mega_launches > 0 and st.shade_launches > 0 and st.extend_launches > 0


@pytest.mark.parametrize("name", ["cbox", "vol_cbox"])
def test_irradiance_is_the_radiance_along_its_probe_rays(bench, name):
    hs, sc = bench.scene(name)
    probes = cbox_probes()
    med = medium_of(hs)
    irr = lj.irradiance(sc, probes[:, :3], probes[:, 3:], spp=SPP, samples=True, variance=True, seed=21, medium_id=med)
    org, d = lj.probe_rays(sc, probes[:, :3], probes[:, 3:], SPP, seed=21)
    rad = lj.radiance_rays(sc, org.reshape(-1, 3), d.reshape(-1, 3), spp=1, samples=True, seed=21, medium_id=med)
    assert irr["samples"].max() > 0
    assert np.array_equal(bits(irr["samples"].reshape(-1, 3)), bits(rad["samples"].reshape(-1, 3)))
    s = irr["samples"]
    mean = ((s[:, 0] + s[:, 2]) + (s[:, 1] + s[:, 3])) * np.float32(0.25)   # 4 samples: two butterfly levels, times 1 / 4
    assert np.array_equal(bits(irr["radiance"]), bits(PI_F * mean))
    # pi_f^2 times the variance of the samples: the bound of the float two-pass computation, and 2^-22 for the product pi_f * pi_f and the multiply
    var64, bound = variance64(s)
    pi2 = float(PI_F) ** 2
    assert (np.abs(irr["variance"].astype(np.float64) - pi2 * var64) <= pi2 * bound + 2.0 ** -22 * pi2 * var64).all()


def test_probe_rays_against_the_twin(bench):
    hs, sc = bench.scene("cbox")
    probes = cbox_probes()
    org, d = lj.probe_rays(sc, probes[:, :3], probes[:, 3:], 16, seed=3)
    ref = TwinRays(hs).probe_rays(probes, 16, seed=3)
    assert np.array_equal(bits(org), bits(ref[..., :3]))              # one float multiply and one float add, uncontracted on both sides
    assert np.abs(d.astype(np.float64) - ref[..., 3:]).max() < 2e-5   # the direction bar of the device known-answer tests
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=-1) - 1.0).max() < 2e-5


@pytest.mark.parametrize("name,diverged", [("cbox", 0.02), ("volpath_test2", 0.03)])
def test_radiance_against_the_twin(bench, name, diverged):
    hs, sc = bench.scene(name)
    rays, _, _ = bench.rays(name)
    got = lj.radiance_rays(sc, rays[:, :3], rays[:, 3:], spp=SPP, samples=True, seed=5, medium_id=medium_of(hs))["samples"].astype(np.float64)
    ref = TwinRays(hs).trace(rays, SPP, seed=5, medium_id=medium_of(hs))["samples"].astype(np.float64)
    rel = np.abs(got - ref).max(axis=-1) / np.maximum(np.abs(ref).max(axis=-1), 1e-3)
    print(name, "median", np.median(rel), "diverged", (rel > 1e-3).mean())
    assert np.median(rel) < 2e-6 and (rel > 1e-3).mean() < diverged


@pytest.mark.parametrize("name", ["cbox", "disney", "volpath_test2"])
def test_determinism_and_pass_boundaries(bench, monkeypatch, name):
    hs, sc = bench.scene(name)
    rays, _, _ = bench.rays(name)
    kw = dict(spp=SPP, samples=True, variance=True, seed=9, medium_id=medium_of(hs))
    a = lj.radiance_rays(sc, rays[:, :3], rays[:, 3:], **kw)
    b = lj.radiance_rays(sc, rays[:, :3], rays[:, 3:], **kw)
    steps_one_pass = sc.stats().wavefront_steps
    monkeypatch.setenv("LJ_TUNE_PASS_SAMPLES", "512")   # 128 rays a pass: 564 x 4 samples in five passes
    c = lj.radiance_rays(sc, rays[:, :3], rays[:, 3:], pool_paths=4096, **kw)
    st = sc.stats()
    assert st.samples == N_RAYS * SPP and st.wavefront_steps >= max(3, steps_one_pass)
    monkeypatch.delenv("LJ_TUNE_PASS_SAMPLES")
    d = lj.radiance_rays(sc, rays[:, :3], rays[:, 3:], pool_paths=5000, **kw)
    for k in ("radiance", "variance", "samples"):
        assert np.array_equal(bits(a[k]), bits(b[k])) and np.array_equal(bits(a[k]), bits(c[k])) and np.array_equal(bits(a[k]), bits(d[k])), k
    assert a["variance"].any()


def test_small_tables_and_sample_counts(bench):
    hs, sc = bench.scene("cbox")
    rays, _, _ = bench.rays("cbox")
    kw = dict(samples=True, variance=True, seed=7)
    full = lj.radiance_rays(sc, rays[:, :3], rays[:, 3:], spp=SPP, **kw)
    for m in (1, 65):   # prefix stability: the first m rays of a call are a call of those m
        part = lj.radiance_rays(sc, rays[:m, :3], rays[:m, 3:], spp=SPP, **kw)
        assert sc.stats().samples == m * SPP
        for k in ("radiance", "variance", "samples"):
            assert np.array_equal(bits(full[k][:m]), bits(part[k])), (m, k)
    three = lj.radiance_rays(sc, rays[:100, :3], rays[:100, 3:], spp=3, **kw)
    rep = np.repeat(rays[:100], 3, axis=0)
    ones = lj.radiance_rays(sc, rep[:, :3], rep[:, 3:], spp=1, **kw)
    assert np.array_equal(bits(three["samples"].reshape(-1, 3)), bits(ones["samples"].reshape(-1, 3)))
    assert not ones["variance"].any() and three["variance"].any()
    empty = lj.radiance_rays(sc, np.zeros((0, 3)), np.zeros((0, 3)), spp=SPP, **kw)
    assert empty["radiance"].shape == (0, 3) and sc.stats().samples == 0 and sc.stats().shade_launches == 0


@pytest.mark.parametrize("spp", [SPP, 67])
def test_radiance_and_variance_against_float64(bench, spp):
    hs, sc = bench.scene("cbox")
    rays, _, _ = bench.rays("cbox")
    out = lj.radiance_rays(sc, rays[:130, :3], rays[:130, 3:], spp=spp, samples=True, variance=True, seed=3)
    x = out["samples"].astype(np.float64)
    err, bound = np.abs(out["radiance"].astype(np.float64) - x.mean(-2)), sum_bound(spp, np.abs(x).mean(-2))
    print("radiance spp", spp, "largest error / bound:", float((err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all()
    ref, vbound = variance64(out["samples"])
    print("variance spp", spp, "largest error / bound:", float((np.abs(out["variance"] - ref) / np.maximum(vbound, 1e-300)).max()))
    assert (np.abs(out["variance"].astype(np.float64) - ref) <= vbound).all() and ref.max() > 0


@pytest.mark.parametrize("name", ["furnace", "furnace_vol"])
def test_furnace_known_answer(bench, name):
    hs, sc = bench.scene(name)
    med = medium_of(hs)
    assert (med is None) == (name == "furnace") and (med is None or med >= 0)
    central = lj.radiance_rays(sc, [(0, 0, 0)], [(0, 0, 1)], spp=1, samples=True, medium_id=med)
    assert np.array_equal(central["samples"].reshape(3), LE), "the emitter must face inward"
    rng = np.random.default_rng(1)
    d = rng.normal(size=(200, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    org = rng.uniform(-0.9, 0.9, size=(200, 3)).astype(np.float32)
    out = lj.radiance_rays(sc, org, d, spp=3, samples=True, variance=True, medium_id=med)
    assert np.array_equal(out["samples"], np.broadcast_to(LE, out["samples"].shape))
    assert np.array_equal(out["radiance"], np.broadcast_to(LE, out["radiance"].shape)) and not out["variance"].any()
    nrm = np.array([(0, 1, 0), (1, 0, 0), (0, 0, -1)], np.float32)
    pos = np.array([(0, -1, 0), (-1, 0.3, 0.2), (0.5, 0.5, 1)], np.float32)
    irr = lj.irradiance(sc, pos, nrm, spp=4, samples=True, variance=True, medium_id=med)
    assert np.array_equal(irr["radiance"], np.broadcast_to(PI_F * LE, irr["radiance"].shape))
    assert not irr["variance"].any() and np.array_equal(irr["samples"], np.broadcast_to(LE, irr["samples"].shape))


def test_every_declared_error_leaves_the_buffers_untouched(bench):
    hs, sc = bench.scene("volpath_test2")
    lib = lj.load_library()
    ok = table([(0, 0, 0)] * 4, [(0, 0, 1)] * 4)
    for label, code, probes, args, ra, n, tab, with_bufs, text in error_calls(hs):
        out, b = buffers(4, 1)
        fn = lib.lj_irradiance if probes else lib.lj_radiance_rays
        rc = fn(sc._h, C.byref(args), C.byref(ra) if ra is not None else None, n, tab.ctypes.data_as(C.c_void_p) if tab is not None else None, C.byref(b) if with_bufs else None)
        assert rc == code and text.encode() in lib.lj_last_error(), (label, rc, lib.lj_last_error())
        assert all((a == SENTINEL).all() for a in out.values()), label
    args = lj.make_args(spp=1)
    assert lib.lj_radiance_rays(sc._h, C.byref(args), None, 4, ok.ctypes.data_as(C.c_void_p), C.byref(_abi.LjRadianceBuffers())) == _abi.LJ_ERR_INVALID_ARG
    hs_aux = film_scene("cbox")
    hs_aux.desc.options.integrator = 0
    aux = lj.Scene(bench.ctx, hs_aux)
    out, b = buffers(4, 1)
    assert lib.lj_radiance_rays(aux._h, C.byref(args), None, 4, ok.ctypes.data_as(C.c_void_p), C.byref(b)) == _abi.LJ_ERR_UNSUPPORTED
    assert all((a == SENTINEL).all() for a in out.values())
    # the scene still renders after the refusals
    assert np.isfinite(lj.radiance_rays(sc, ok[:, :3], ok[:, 3:], spp=1)["radiance"]).all()


def test_stats_are_those_of_a_render_of_n_times_spp_samples(bench):
    hs, sc = bench.scene("cbox")
    rays, _, _ = bench.rays("cbox")
    lj.radiance_rays(sc, rays[:, :3], rays[:, 3:], spp=3)
    st = sc.stats()
    assert st.samples == N_RAYS * 3 and st.mega_launches == 0 and st.rays_closest >= st.samples and st.bounce_iterations > 0 and st.render_ms > 0
    lj.render(sc, spp=1)
    assert sc.stats().mega_launches > 0   # the scene's renders still take the fused kernel
