"""A short last test round of a pass of k_mega's leaf scan runs split by primitive (mega.hip: scan_trace, dmegapool.h): with M the largest leaf
count of the scene rounded up to a power of two, a last round of m items with m * M <= 64 has lane l test primitive l % M of item r + l / M
(and a round too long for that shares an item among fewer lanes, each walking several primitives).  Which lane tests which primitive must
not show: every render here is held bit for bit, and counter for counter, to the wavefront kernels (LJ_TUNE_MEGA=0), and every ray query to
the BVH traversal.

LJ_TUNE_MEGA_ITEM_CAP shapes the last round.  cbox pools lane-major, so every pass but a wave-step's last holds exactly `cap` items: caps 2,
31, 32 and 33 give last rounds of 2, 31, 32 (the boundary 2 m = 64) and 33 items (never split), caps 65, 96 and 97 a full round followed by
1, 32 and 33; unset, a wave-step is one pass of about 150 items.  Both scenes have leaves of unequal size, which is what exercises the
`primitive < count` predicate of a split round: cbox's table holds seventeen leaves of two triangles and one of four (M = 4), veach_mi's
five leaves of one primitive and six of two (M = 2).  veach_mi (spheres, the Plastic build) pools in rounds of up to 64 and is split only
in the ray queries, which pool lane-major in every build."""
import os

import numpy as np
import pytest

import lajolla_public_amd as lj
from helpers import Oracle, random_rays, scene_path

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return lj.Context(0)


@pytest.fixture(scope="module")
def cbox(ctx):
    return lj.Scene(ctx, lj.parse_scene(scene_path("cbox")))


@pytest.fixture(scope="module")
def veach_mi(ctx):
    return lj.Scene(ctx, lj.parse_scene(scene_path("veach_mi")))


class _env:
    """Environment variables for the duration (the library reads its LJ_TUNE_* knobs per render and per query)."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _counters(sc):
    st = sc.stats()
    return st.samples, st.bounce_iterations, st.rays_closest, st.rays_shadow, st.mega_launches


def _wavefront(sc, crop, spp, cache={}):
    """The reference of a (scene, crop, spp): rendered once by the wavefront kernels, shared by the cases that need it, never written to."""
    key = (id(sc), crop, spp)
    if key not in cache:
        with _env(LJ_TUNE_MEGA="0"):
            img = lj.render_samples(sc, crop, spp=spp)
            c = _counters(sc)
        assert c[4] == 0
        img.setflags(write=False)
        cache[key] = (img, c[:4])
    return cache[key]


def _check(sc, crop, spp, total, tune):
    ref, ref_counters = _wavefront(sc, crop, spp)
    with _env(**tune):
        a = lj.render_samples(sc, crop, spp=spp)
        c = _counters(sc)
    assert c[4] == 1, "not rendered by k_mega"
    assert a.size == total * 3 and c[0] == total
    assert np.array_equal(a.view(np.uint32), ref.view(np.uint32)), f"{np.sum(a != ref)} of {a.size} values differ"
    assert c[:4] == ref_counters, f"samples, bounce iterations, closest rays, shadow rays: {c[:4]} against {ref_counters}"


def _tune(cap):
    return {} if cap is None else {"LJ_TUNE_MEGA_ITEM_CAP": str(cap)}


# (crop, spp, total samples): 3x3, 5x13 and 16x16 pixels of the lit part of the box (the crops of test_gpu_mega_pool.py)
CROPS = [((250, 250, 253, 253), 7, 63), ((250, 250, 255, 263), 1, 65), ((248, 248, 264, 264), 5, 1280)]
CAPS = [2, 31, 32, 33, 65, 96, 97, None]


@pytest.mark.parametrize("cap", CAPS, ids=[f"cap_{c}" if c else "cap_unset" for c in CAPS])
@pytest.mark.parametrize("crop,spp,total", CROPS, ids=[f"{t}_samples" for _, _, t in CROPS])
def test_cbox_crop_equals_wavefront(cbox, crop, spp, total, cap):
    _check(cbox, crop, spp, total, _tune(cap))


@pytest.mark.parametrize("cap", [64, 100])
def test_veach_mi_crop_equals_wavefront(veach_mi, cap):
    _check(veach_mi, (300, 200, 324, 224), 3, 24 * 24 * 3, _tune(cap))


@pytest.mark.parametrize("name", ["cbox", "veach_mi"])
def test_queries_through_the_scan_equal_the_bvh(ctx, name):
    hs = lj.parse_scene(scene_path(name))
    sc = lj.Scene(ctx, hs)
    o = Oracle(hs)
    rays = random_rays(hs, 20000, 13, o)
    tb = o.tables()
    tfar = (np.random.default_rng(6).random(len(rays)) * tb["bounds_radius"]).astype(np.float32)
    tnear = np.float32(tb["shadow_epsilon"])
    with _env(LJ_TUNE_MEGA="0"):
        hit_bvh = lj.intersect(sc, rays["org"], rays["dir"], 0.0, np.inf)
        assert sc.stats().mega_launches == 0
        occ_bvh = lj.occluded(sc, rays["org"], rays["dir"], tnear, tfar)
    assert (hit_bvh["shape_id"] >= 0).mean() > 0.3 and 0.05 < occ_bvh.mean() < 0.95
    for cap in (1, 8, 9, 32, 33):
        with _env(**_tune(cap)):
            hit = lj.intersect(sc, rays["org"], rays["dir"], 0.0, np.inf)
            assert sc.stats().mega_launches == 1, "not answered by the leaf scan"
            occ = lj.occluded(sc, rays["org"], rays["dir"], tnear, tfar)
        for f in ("t", "u", "v", "shape_id", "prim_id"):
            assert np.array_equal(hit[f].view(np.uint32), hit_bvh[f].view(np.uint32)), f"cap {cap}: scan vs BVH: {f}"
        assert np.array_equal(occ, occ_bvh), f"cap {cap}: occluded"
