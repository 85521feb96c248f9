"""LJ_RNG_TILE on the GPU (tile.hip: k_tile): the reference's render() schedule — one pcg32 stream per 16x16 tile, consumed pixel by
pixel, sample by sample — held against the oracle's rng_mode = 1 with the bars of the CPU suite (test_tile_schedule.py), and the bit-level
invariances of the bounded launches: runs, launch shapes, step budgets, crops, rank shares and device groups change nothing."""
import os

import numpy as np
import pytest

import lajolla_public_amd as lj
from lajolla_public_amd import _abi
from helpers import Oracle
from test_tile_schedule import CROP4, LIGHT8, matched_prefix, rel_diff, scene

pytestmark = pytest.mark.gpu

TILE = _abi.LJ_RNG_TILE

_ctx = None


def ctx():
    global _ctx
    if _ctx is None:
        _ctx = lj.Context(0)
    return _ctx


def gpu_scene(hs):
    return lj.Scene(ctx(), hs)


class tune:
    """environment overrides read by the render call (LJ_TUNE_TILE_LANES, LJ_TUNE_TILE_STEPS)"""

    def __init__(self, **kw):
        self.kw = {k: str(v) for k, v in kw.items()}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update(self.kw)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("max_depth,crop", [(1, LIGHT8), (2, CROP4)])
def test_fixed_draw_counts_match_the_oracle(max_depth, crop):
    hs = scene("cbox")
    spp = 4
    _, _, po, _ = Oracle(hs).render(spp=spp, rng_mode=1, crop=crop, per_sample=True, max_depth=max_depth)
    sc = gpu_scene(hs)
    pt = lj.render_samples(sc, crop, spp=spp, max_depth=max_depth, rng_mode=TILE)
    rel = rel_diff(pt, po)
    assert np.median(rel) < 2e-6
    assert (rel > 1e-3).mean() <= 0.02
    assert po.any() and sc.stats().samples == (crop[2] - crop[0]) * (crop[3] - crop[1]) * spp


def test_russian_roulette_draw_is_deferred():
    hs = scene("cbox", rr_depth=1)
    spp = 4
    _, _, po, _ = Oracle(hs).render(spp=spp, rng_mode=1, crop=CROP4, per_sample=True, max_depth=4)
    pt = lj.render_samples(gpu_scene(hs), CROP4, spp=spp, max_depth=4, rng_mode=TILE)
    rel = rel_diff(pt, po)
    assert (rel <= 1e-3).mean() >= 0.95
    assert np.median(matched_prefix(rel, spp)) >= 0.25 * 256 * spp


@pytest.mark.parametrize("name", ["cbox", "veach_mi"])
def test_full_depth_tile_means_agree(name):
    hs = scene(name)
    spp = 4
    _, _, po, _ = Oracle(hs).render(spp=spp, rng_mode=1, crop=CROP4, per_sample=True)
    pt = lj.render_samples(gpu_scene(hs), CROP4, spp=spp, rng_mode=TILE)
    for ty in range(0, 32, 16):
        for tx in range(0, 32, 16):
            a = np.minimum(pt[ty:ty + 16, tx:tx + 16], 50.0).reshape(-1, 3)
            b = np.minimum(po[ty:ty + 16, tx:tx + 16], 50.0).reshape(-1, 3)
            se = np.sqrt(a.var(axis=0) / len(a) + b.var(axis=0) / len(b)) + 1e-6
            assert np.all(np.abs(a.mean(axis=0) - b.mean(axis=0)) < 5 * se), (name, ty, tx)
    assert np.median(matched_prefix(rel_diff(pt, po), spp)) >= 0.25 * 256 * spp


@pytest.mark.parametrize("name,max_depth", [("volpath_test/volpath_test3.xml", 3), ("volpath_test/hetvol.xml", 3)])
def test_volpath_matches_the_oracle(name, max_depth):
    hs = scene(name)
    w, h = hs.width, hs.height
    crop = tuple(v - v % 16 for v in (w // 2 - 16, h // 2 - 16, w // 2 + 16, h // 2 + 16))
    spp = 2
    _, _, po, _ = Oracle(hs).render(spp=spp, rng_mode=1, crop=crop, per_sample=True, max_depth=max_depth)
    pt = lj.render_samples(gpu_scene(hs), crop, spp=spp, max_depth=max_depth, rng_mode=TILE)
    rel = rel_diff(pt, po)
    assert np.median(rel) < 2e-6
    assert (rel > 1e-3).mean() < 0.1
    assert np.median(matched_prefix(rel, spp)) >= 0.5 * 256 * spp


def test_runs_launch_shapes_and_step_budgets_are_bit_identical():
    sc = gpu_scene(scene("cbox"))
    crop = (128, 128, 256, 256)
    want = lj.render(sc, spp=4, crop=crop, rng_mode=TILE)
    assert want[128:256, 128:256].any() and not want[:128].any()
    assert np.array_equal(bits(lj.render(sc, spp=4, crop=crop, rng_mode=TILE)), bits(want))
    for kw in (dict(LJ_TUNE_TILE_LANES=64), dict(LJ_TUNE_TILE_LANES=7), dict(LJ_TUNE_TILE_STEPS=3), dict(LJ_TUNE_TILE_STEPS=100000)):
        with tune(**kw):
            got = lj.render(sc, spp=4, crop=crop, rng_mode=TILE)
        assert np.array_equal(bits(got), bits(want)), kw


def test_crop_equals_the_same_pixels_of_the_full_frame():
    hs = scene("cbox")
    sc = gpu_scene(hs)
    full = lj.render(sc, spp=2, rng_mode=TILE)
    st = sc.stats()
    assert st.samples == hs.width * hs.height * 2
    crop = (100, 150, 190, 211)   # not tile-aligned
    part = lj.render(sc, spp=2, crop=crop, rng_mode=TILE)
    x0, y0, x1, y1 = crop
    assert np.array_equal(bits(part[y0:y1, x0:x1]), bits(full[y0:y1, x0:x1]))
    part[y0:y1, x0:x1] = 0
    assert not part.any()
    assert sc.stats().samples == 6 * 5 * 256 * 2   # tiles 6..11 x 9..13 walked whole
    ps = lj.render_samples(sc, crop, spp=2, rng_mode=TILE)
    assert np.array_equal(bits((ps[:, :, 0] + ps[:, :, 1]) / np.float32(2)), bits(full[y0:y1, x0:x1]))   # the pixel's float sum in sample order


def test_rank_shares_and_logical_ranks_sum_to_one_render():
    hs = scene("cbox")
    sc = gpu_scene(hs)
    want = lj.render(sc, spp=1, rng_mode=TILE)
    for world in (2, 3):
        acc = np.zeros_like(want)
        for r in range(world):
            acc += lj.render(sc, spp=1, rank=r, world_size=world, rng_mode=TILE)
        assert np.array_equal(bits(acc), bits(want)), world
    g = lj.DeviceGroup([0, 0, 0])
    got = lj.render_group(lj.GroupScene(g, hs), spp=1, rng_mode=TILE)
    assert np.array_equal(bits(got), bits(want))


def test_tile_and_sample_schedules_agree_statistically():
    """Mirror of test_oracle_modes.py: two unbiased estimators of the same pixels, on different random numbers."""
    sc = gpu_scene(scene("cbox"))
    crop = (128, 128, 160, 160)
    spp = 64
    t = lj.render(sc, spp=spp, crop=crop, rng_mode=TILE)
    ps = lj.render_samples(sc, crop, spp=spp)
    x0, y0, x1, y1 = crop
    t = t[y0:y1, x0:x1]
    n = ps.shape[0] * ps.shape[1] * ps.shape[2]
    stderr = ps.reshape(-1, 3).std(axis=0) / np.sqrt(n)
    assert np.all(np.abs(t.mean(axis=(0, 1)) - ps.mean(axis=(0, 1, 2))) < 5 * np.sqrt(2) * stderr)
    assert not np.allclose(t, ps.mean(axis=2))


@pytest.mark.parametrize("integrator", [0, 1, 2, 3, 4])
def test_aux_integrators_are_the_same_in_both_modes(integrator):
    hs = scene("cbox")
    hs.desc.options.integrator = integrator
    sc = gpu_scene(hs)
    a = lj.render(sc, spp=1, rng_mode=TILE)
    b = lj.render(sc, spp=1)
    assert np.array_equal(bits(a), bits(b))


def test_other_rng_modes_are_refused():
    sc = gpu_scene(scene("cbox"))
    for mode in (2, -1):
        with pytest.raises(lj.LajollaError) as e:
            lj.render(sc, spp=1, rng_mode=mode)
        assert e.value.code == _abi.LJ_ERR_UNSUPPORTED
