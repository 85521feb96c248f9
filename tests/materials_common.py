"""Shared by tests/test_materials_parity.py (host twin) and tests/test_gpu_materials.py (device): cbox with the two boxes (and, for one
case, the floor) re-materialised, one case per Material alternative and at least one per shading feature set (device/dshade.h), the
comparison with the oracle's per-sample radiance, and the feature set each case must be uploaded with."""
import numpy as np

import lajolla_public_amd as lj
from helpers import const, scene_path, set_material

W = [0.8, 0.75, 0.7]
CHECKER = {"kind": "checkerboard", "color0": [0.8, 0.3, 0.2], "color1": [0.2, 0.3, 0.8], "uscale": 4, "vscale": 4, "uoffset": 0, "voffset": 0}
MATERIALS = {
    "roughdielectric": dict(kind="roughdielectric", specular_reflectance=const([1, 1, 1]), specular_transmittance=const([0.9, 0.95, 1.0]), roughness=const(0.2), eta=1.5),
    "disneydiffuse": dict(kind="disneydiffuse", base_color=const(W), roughness=const(0.6), subsurface=const(0.4)),
    "disneymetal": dict(kind="disneymetal", base_color=const([0.9, 0.6, 0.3]), roughness=const(0.3), anisotropic=const(0.5)),
    "disneyglass": dict(kind="disneyglass", base_color=const([0.9, 0.9, 0.95]), roughness=const(0.15), anisotropic=const(0.3), eta=1.45),
    "disneyclearcoat": dict(kind="disneyclearcoat", clearcoat_gloss=const(0.7)),
    "disneysheen": dict(kind="disneysheen", base_color=const(W), sheen_tint=const(0.5)),
    "disneybsdf": dict(kind="disneybsdf", base_color=const([0.82, 0.67, 0.16]), specular_transmission=const(0.5), metallic=const(0.5), subsurface=const(0.5),
                       specular=const(0.5), roughness=const(0.1), specular_tint=const(0.5), anisotropic=const(0.5), sheen=const(0.5), sheen_tint=const(0.5),
                       clearcoat=const(0.5), clearcoat_gloss=const(0.5), eta=1.5),   # the parameter set of scenes/disney_bsdf_test/disney_bsdf.xml
    "disneybsdf_opaque": dict(kind="disneybsdf", base_color=CHECKER,
                              specular_transmission=const(0.0), metallic=const(0.2), subsurface=const(0.3), specular=const(0.8), roughness=const(0.4),
                              specular_tint=const(0.2), anisotropic=const(0.0), sheen=const(1.0), sheen_tint=const(0.3), clearcoat=const(1.0), clearcoat_gloss=const(0.9), eta=1.5),
    # the two feature sets the cases above leave out: FeatPlastic and FeatLambertTex
    "roughplastic": dict(kind="roughplastic", diffuse_reflectance=const([0.5, 0.4, 0.3]), specular_reflectance=const([1, 1, 1]), roughness=const(0.15), eta=1.5),
    "lambert_checker": dict(kind="lambertian", reflectance=CHECKER),
}
DIVERGED = {"roughdielectric": 0.08, "disneyglass": 0.08, "disneybsdf": 0.06}

# the feature set (device/dshade.h: with_shade_variant) lj_scene_upload picks for each case: the first that covers it
EXPECTED_VARIANT = {"cbox": 0, "roughplastic": 1, "lambert_checker": 2, "roughdielectric": 3, "disneybsdf": 4, "disneybsdf_opaque": 4,
                    "disneydiffuse": 5, "disneymetal": 5, "disneyglass": 5, "disneyclearcoat": 5, "disneysheen": 5}

CROP, SPP = (176, 232, 240, 296), 8           # straddles the tall box, its shadow and the floor


def case_scene(name):
    """The HostScene of a case; "cbox" is the scene as it is shipped."""
    hs = lj.parse_scene(scene_path("cbox"))
    if name == "cbox":
        return hs
    set_material(hs, 0, MATERIALS[name])          # "box": both boxes
    if name == "disneybsdf_opaque":
        set_material(hs, 1, MATERIALS[name])      # "white": floor, ceiling, back wall
    return hs


def check_against_oracle(name, got, ref, bounces, ref_bounces):
    """Per-sample radiance `got` (float32) of a window against the oracle's `ref` (float64) under the same pcg32 streams, and the bounce
    counts of the two renders.  Returns (diverged share, median relative difference)."""
    pt, ps = got, ref
    assert np.isfinite(pt).all()
    rel = np.abs(pt - ps).max(axis=-1) / np.maximum(np.abs(ps).max(axis=-1), 1e-3)
    print(f"{name}: diverged {100 * (rel > 1e-3).mean():.2f} %, median relative difference {np.median(rel):.2e}")
    assert np.median(rel) < 5e-6, np.median(rel)
    assert (rel > 1e-3).mean() < DIVERGED.get(name, 0.03), (rel > 1e-3).mean()
    # Diverged paths are still samples of the same estimator, so their differences must be zero-mean: the summed
    # difference has to stay within 4 standard deviations of a zero-mean sum (z-test on the per-sample differences,
    # firefly-clamped at 4 so a handful of caustic paths with values 50-80 cannot decide it), and the means within 1 %.
    d = (np.minimum(pt, 4.0) - np.minimum(ps, 4.0)).sum(axis=-1).ravel()
    assert abs(d.sum()) <= 4.0 * np.sqrt((d * d).sum()) + 1e-6
    assert abs(np.minimum(pt, 4.0).mean() / np.minimum(ps, 4.0).mean() - 1) < 1e-2
    assert abs(bounces / ref_bounces - 1) < 2e-2
    return float((rel > 1e-3).mean()), float(np.median(rel))
