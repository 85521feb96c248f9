"""The Material alternatives (material.h:102-110) inside the integrator: cbox with the two boxes (and, for one case, the floor)
re-materialised (tests/materials_common.py), device shading code (host build, float) against the oracle (double) path by path.
Bars as in test_twin_parity.py; transmissive materials get a wider diverged-sample allowance because a refraction /
reflection choice flips whole sub-paths.  tests/test_gpu_materials.py holds the device to the same bars."""
import pytest

from helpers import Oracle, Twin
from materials_common import CROP, DIVERGED, MATERIALS, SPP, case_scene, check_against_oracle


@pytest.mark.parametrize("name", sorted(MATERIALS))
def test_material_in_the_integrator(name):
    hs = case_scene(name)
    o, tw = Oracle(hs), Twin(hs)
    crop, spp = CROP, SPP
    assert (crop, spp) == ((176, 232, 240, 296), 8)
    rc, _, ps, st = o.render(spp=spp, rng_mode=0, crop=crop, per_sample=True)
    assert rc == 0
    pt, bounces = tw.render_samples(crop, spp)
    check_against_oracle(name, pt, ps, bounces, st.bounces)
