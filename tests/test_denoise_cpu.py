"""lj_denoise on the CPU: the host twin of device/ddenoise.h (tests/twin_denoise — the device kernels call the same functions and equal it bit
for bit, tests/test_gpu_denoise.py) against a float64 numpy model written from the header's text, properties of the filter on the twin, and
the Python wrappers' argument checks.

The bar of the model comparison is measured, not guessed: the largest relative error (floor 1e-6 on the denominator) of the twin over
SIZES x iterations {1, 3, 5} x CASES is MEASURED below; the tests ask for 8 times that."""
import ctypes as C

import numpy as np
import pytest

import lajolla_public_amd as lj
from lajolla_public_amd import _abi
from denoise_common import (CASES, DEFAULTS, OPTIONAL, SIZES, image_of, make_inputs, model_denoise, rel_err, same, subset, twin_denoise)

MEASURED = 4.5e-6   # largest relative error of the float32 twin against the float64 model over the whole set (printed by the test)
BAR = 8 * MEASURED
HUGE = {k: 1e15 for k in DEFAULTS}


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%dx%d" % s)
def test_twin_matches_the_float64_model(size):
    inputs = make_inputs(*size)
    worst = 0.0
    for iterations in (1, 3, 5):
        for drop, demodulate in CASES:
            sub = subset(inputs, *drop)
            got_c, got_v = twin_denoise(sub, iterations, demodulate)
            ref_c, ref_v = model_denoise(sub, iterations, demodulate)
            e = rel_err(got_c, ref_c)
            if ref_v is not None:
                e = max(e, rel_err(got_v, ref_v))
            else:
                assert got_v is None
            worst = max(worst, e)
            assert e <= BAR, (size, iterations, drop, demodulate, e)
    print("size", size, "largest relative error twin vs float64:", worst)


def ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))   # (same sign, finite: the distance in units of the last place)


@pytest.mark.parametrize("iterations", [1, 3, 5])
def test_constant_image_comes_back(iterations):
    inputs = make_inputs(1, 29, 37)
    inputs["rgb"][...] = np.array([0.7, 0.3, 0.9], np.float32)
    inputs["variance"][...] = np.float32(0.01)
    for drop, demodulate in [((), False), (("variance",), False), (OPTIONAL, False)]:
        out, _ = twin_denoise(subset(inputs, *drop), iterations, demodulate)
        d = ulps(out, inputs["rgb"])
        print("iterations", iterations, "without", drop, "largest distance in ulp:", int(d.max()))
        assert d.max() <= iterations, (drop, int(d.max()))


def test_huge_sigmas_give_the_plain_spline_blur():
    inputs = subset(make_inputs(1, 29, 37), "variance")
    got, _ = twin_denoise(inputs, 5, False, **HUGE)
    ref, _ = model_denoise({"rgb": inputs["rgb"]}, 5, False)
    assert rel_err(got, ref) <= BAR
    plain, _ = twin_denoise({"rgb": inputs["rgb"]}, 5, False)
    assert same(got, plain)   # every stopping term is exactly 1


def step_inputs(which, right):
    """20 x 16, a colour step at x = 9 that coincides with a step of one guide; `right`: the colour right of it"""
    h, w = 16, 20
    rng = np.random.default_rng(5)
    rgb = (0.4 + 0.1 * rng.random((1, h, w, 3))).astype(np.float32)
    rgb[:, :, 9:] = np.asarray(right, np.float32) + rgb[:, :, 9:] * np.float32(0.25)
    guide = {"normal": np.zeros((1, h, w, 3), np.float32), "albedo": np.full((1, h, w, 3), 0.2, np.float32), "depth": np.ones((1, h, w), np.float32)}
    guide["normal"][..., 2] = 1.0
    guide["normal"][:, :, 9:] = (1.0, 0.0, 0.0)
    guide["albedo"][:, :, 9:] = 0.8
    guide["depth"][:, :, 9:] = 2.0
    return {"rgb": rgb, which: guide[which]}


@pytest.mark.parametrize("which", ["normal", "depth", "albedo"])
def test_a_guide_step_keeps_the_two_sides_apart(which):
    a, _ = twin_denoise(step_inputs(which, (2.0, 0.1, 0.1)), 5, False)
    b, _ = twin_denoise(step_inputs(which, (0.1, 3.0, 50.0)), 5, False)
    assert same(a[:, :, :9], b[:, :, :9])   # weight 0: the left side never saw a bit of the right one
    assert not same(a[:, :, 9:], b[:, :, 9:])
    # ... and without the guide the sides mix
    a0, _ = twin_denoise({"rgb": step_inputs(which, (2.0, 0.1, 0.1))["rgb"]}, 5, False)
    b0, _ = twin_denoise({"rgb": step_inputs(which, (0.1, 3.0, 50.0))["rgb"]}, 5, False)
    assert not same(a0[:, :, :9], b0[:, :, :9])
    # the same from the other side
    inputs = step_inputs(which, (2.0, 0.1, 0.1))
    c = {k: v.copy() for k, v in inputs.items()}
    c["rgb"][:, :, :9] *= np.float32(3.0)
    assert same(twin_denoise(c, 5, False)[0][:, :, 9:], a[:, :, 9:])


@pytest.mark.parametrize("demodulate", [False, True])
def test_a_batch_is_its_images_filtered_alone(demodulate):
    inputs = make_inputs(2, 16, 20)
    c, v = twin_denoise(inputs, 5, demodulate)
    for i in range(2):
        ci, vi = twin_denoise(image_of(inputs, i), 5, demodulate)
        assert same(ci[0], c[i]) and same(vi[0], v[i])
    assert not same(c[0], c[1])


def dilate(v, r):
    h, w = v.shape[1:3]
    p = np.pad(v, ((0, 0), (r, r), (r, r), (0, 0)), mode="edge")
    return np.max([p[:, dy:dy + h, dx:dx + w] for dy in range(2 * r + 1) for dx in range(2 * r + 1)], axis=0)


def test_variance_shrinks_under_uniform_weights():
    inputs = make_inputs(1, 29, 37)
    sub = {"rgb": inputs["rgb"], "variance": inputs["variance"]}
    _, v = twin_denoise(sub, 1, False, **HUGE)   # no guides, a colour term that never stops: the plain stencil
    # v' = sum w^2 v_q / (sum w)^2 <= max over the 5 x 5 taps (sum w^2 <= (sum w)^2), whatever v is
    assert (v <= dilate(inputs["variance"], 2)).all()
    # ... and on this smooth variance field also the 3 x 3 maximum: sum w^2 / (sum w)^2 <= 0.19 even in a corner
    assert (v <= dilate(inputs["variance"], 1)).all()
    assert (v > 0).all()


def test_left_right_flip():
    inputs = make_inputs(1, 29, 37)
    flipped = {k: np.ascontiguousarray(v[:, :, ::-1]) for k, v in inputs.items()}
    for demodulate in (False, True):
        c, v = twin_denoise(inputs, 5, demodulate)
        cf, vf = twin_denoise(flipped, 5, demodulate)
        # the tap order is fixed, so the sums run the other way round: equal to the float64 bar, not bitwise
        assert rel_err(cf[:, :, ::-1], c.astype(np.float64)) <= BAR and rel_err(vf[:, :, ::-1], v.astype(np.float64)) <= BAR


def test_in_place_twin():
    inputs = make_inputs(1, 5, 7)
    a, _ = twin_denoise(inputs, 3, True)
    b, _ = twin_denoise(inputs, 3, True, in_place=True)
    assert same(a, b)


# ------------------------------------------------------------------ the Python wrappers and the C ABI, without a device
class _NoCtx:
    _h = None
    device = 0


def test_wrapper_argument_checks():
    img = np.zeros((4, 6, 3), np.float32)
    with pytest.raises(ValueError):
        lj.denoise({"albedo": img}, ctx=_NoCtx())                                   # no rgb
    with pytest.raises(ValueError):
        lj.denoise({"rgb": img}, ctx=_NoCtx())                                      # demodulate (the default) without albedo
    with pytest.raises(ValueError):
        lj.denoise({"rgb": img, "beauty": img}, ctx=_NoCtx(), demodulate=False)
    with pytest.raises(ValueError):
        lj.denoise({"rgb": img, "depth": img}, ctx=_NoCtx(), demodulate=False)      # depth is (h, w)
    with pytest.raises(ValueError):
        lj.denoise({"rgb": img[0]}, ctx=_NoCtx(), demodulate=False)
    with pytest.raises(ValueError):
        lj.denoise({"rgb": img}, ctx=_NoCtx(), demodulate=False, iterations=9)
    with pytest.raises(ValueError):
        lj.denoise({"rgb": img}, ctx=_NoCtx(), demodulate=False, sigma_color=-1.0)
    with pytest.raises(ValueError):
        lj.denoise({"rgb": img}, ctx=_NoCtx(), demodulate=False, sigma_normal=float("nan"))
    with pytest.raises(ValueError):
        lj.denoise({"rgb": img}, ctx=_NoCtx(), demodulate=False, sigma_colour=1.0)
    with pytest.raises(ValueError):
        lj.denoise_device(_NoCtx(), {"rgb": 1}, 1, 6, 4, 1, variance_out=1, demodulate=False)   # variance_out without variance
    with pytest.raises(ValueError):
        lj.denoise_device(_NoCtx(), {"rgb": 1}, 1, 6, 4, 0, demodulate=False)
    a = lj.make_denoise_args(3, True, sigma_depth=0.2)
    assert (a.iterations, a.flags, a.sigma_color) == (3, _abi.LJ_DENOISE_DEMODULATE, 0.0) and abs(a.sigma_depth - 0.2) < 1e-7
    assert [f[0] for f in _abi.LjDenoiseArgs._fields_] == ["iterations", "flags", "sigma_color", "sigma_normal", "sigma_depth", "sigma_albedo"]
    assert C.sizeof(_abi.LjDenoiseArgs) == 24 and C.sizeof(_abi.LjDenoiseStats) == 24
    assert {"lj_denoise", "lj_denoise_device", "lj_get_denoise_stats"} <= {n for n, _, _ in _abi.SYMBOLS}


def test_cli_refuses_denoise_where_there_are_no_features(capsys):
    from lajolla_public_amd.__main__ import main
    assert main(["--denoise", "--rng", "tile", "scene.xml"]) == 2
    assert main(["--denoise", "--gpus", "2", "scene.xml"]) == 2
    assert "--denoise" in capsys.readouterr().err


def test_c_abi_is_loud_without_a_context():
    lib = lj.load_library()
    img, out = np.zeros((4, 6, 3), np.float32), np.full((4, 6, 3), 7.0, np.float32)
    bufs = _abi.LjFeatureBuffers()
    bufs.rgb = img.ctypes.data
    for call in (lambda: lib.lj_denoise(None, 1, 6, 4, C.byref(bufs), None, out.ctypes.data_as(C.c_void_p), None),
                 lambda: lib.lj_denoise_device(None, 1, 6, 4, C.byref(bufs), None, out.ctypes.data_as(C.c_void_p), None, None)):
        assert call() in (_abi.LJ_ERR_INVALID_ARG, _abi.LJ_ERR_DEVICE)
        assert b"denoise" in lib.lj_last_error()
    assert (out == 7.0).all()
    assert lib.lj_get_denoise_stats(None, C.byref(_abi.LjDenoiseStats())) == _abi.LJ_ERR_INVALID_ARG
    try:   # where there is no device a context cannot exist, so there is nothing to filter on: lj.denoise raises
        lj.Context(0)
    except lj.LajollaError as e:
        assert e.code == _abi.LJ_ERR_DEVICE
        with pytest.raises(lj.LajollaError):
            lj.denoise({"rgb": img}, demodulate=False)
