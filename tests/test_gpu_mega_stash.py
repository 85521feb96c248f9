"""k_mega hands camera samples to lanes through a per-wave stash that all 64 lanes fill at once (mega.hip, dregen.h).  Which lane computes a
sample, and when, must not show: every case here is held bit for bit, and counter for counter, to the wavefront kernels (LJ_TUNE_MEGA=0) at the
smallest sizes where the stash can go wrong — fewer samples than a fill, exactly one fill, one more than a fill, several grabs per wave —
once with the default grid and once with one workgroup per CU taking 64 samples per grab (refill and grab in the same iteration, every time)."""
import os

import numpy as np
import pytest

import lajolla_public_amd as lj
from helpers import scene_path

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return lj.Context(0)


@pytest.fixture(scope="module")
def cbox(ctx):
    return lj.Scene(ctx, lj.parse_scene(scene_path("cbox")))


class _env:
    """Environment variables for the duration (the library reads its LJ_TUNE_* knobs per render)."""

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


# (crop, spp, total samples): 3x3, 8x8, 5x13 and 16x16 pixels of the lit part of the box
CROPS = [((250, 250, 253, 253), 7, 63), ((250, 250, 258, 258), 1, 64), ((250, 250, 255, 263), 1, 65), ((248, 248, 264, 264), 5, 1280)]
TUNES = [{}, {"LJ_TUNE_MEGA_GRAB": "64", "LJ_TUNE_MEGA_BLOCKS_PER_CU": "1"}]


@pytest.mark.parametrize("tune", TUNES, ids=["default", "grab64_one_block_per_cu"])
@pytest.mark.parametrize("crop,spp,total", CROPS, ids=[f"{t}_samples" for _, _, t in CROPS])
def test_cbox_crop_equals_wavefront(cbox, crop, spp, total, tune):
    _check(cbox, crop, spp, total, tune)


def test_veach_mi_crop_equals_wavefront(ctx):
    # spheres and the Plastic instantiation (four waves per SIMD)
    sc = lj.Scene(ctx, lj.parse_scene(scene_path("veach_mi")))
    _check(sc, (300, 200, 324, 224), 3, 24 * 24 * 3, {})


def test_cbox_whole_frame_one_spp_equals_wavefront(cbox):
    # many waves drain the counter together, and most of them meet its end with a part-filled stash
    a = lj.render(cbox, spp=1)
    ca = _counters(cbox)
    with _env(LJ_TUNE_MEGA="0"):
        b = lj.render(cbox, spp=1)
        cb = _counters(cbox)
    assert ca[4] == 1 and cb[4] == 0
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert ca[:4] == cb[:4] and ca[0] == a.shape[0] * a.shape[1]
