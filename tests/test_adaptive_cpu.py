"""lj_render_adaptive on the CPU: the host twin of device/dadaptive.h (tests/twin_adaptive — the device kernels call the same functions and
equal it list for list and bit for bit, tests/test_gpu_adaptive.py) against float64 numpy: the merge against the pooled statistics of all
samples, the selection against a model written from the header's text, and the argument rules.

The bar of the merge is measured, not guessed: the largest relative error (floor 1e-6 on the denominator, the convention of
test_denoise_cpu.py) of the merged mean and variance over BATCHES x three seeds is MEASURED below; the test asks for 8
times that.  The margin is for other seeds, not for another rule."""
import numpy as np
import pytest

from adaptive_common import (SEED_STEP, State, make_state, model_e2, model_select, pairs, rel_err, same, tile_order, twin_error, twin_merge, twin_output, twin_params,
                             twin_seed, twin_select)

MEASURED = 2.95e-7  # largest relative error of the float32 merge against the pooled float64 statistics over the whole set (printed by the test)
BAR = 8 * MEASURED
BATCHES = [(2, 1, 5, 16), (16, 5, 2, 1), (4, 4, 4, 4, 4, 4), (2, 30)]
H, W = 29, 37


def batch_stats(x):
    """mean and sum (x - mean)^2 / (k (k - 1)) of x (h, w, k, 3) in float64, rounded to float32 — what a round's frames hold"""
    k = x.shape[2]
    m = x.mean(axis=2)
    v = ((x - m[:, :, None]) ** 2).sum(axis=2) / (k * (k - 1)) if k > 1 else np.zeros_like(m)
    return m.astype(np.float32), v.astype(np.float32)


@pytest.mark.parametrize("sizes", BATCHES, ids=lambda s: "+".join(map(str, s)))
def test_merge_matches_the_pooled_statistics(sizes):
    worst = 0.0
    lst = tile_order(W, H)
    for seed in (0, 1, 2):
        rng = np.random.default_rng(seed)
        total = sum(sizes)
        # radiance-like samples: a per-pixel level over three decades times a gamma-distributed factor (skewed, positive)
        x = (10.0 ** rng.uniform(-2, 1, size=(H, W, 1, 1))) * rng.gamma(2.0, 0.5, size=(H, W, total, 3))
        st, at = State(H, W), 0
        for r, k in enumerate(sizes):
            b, v = batch_stats(x[:, :, at:at + k])
            twin_merge(st, lst, k, r == 0, b, v)
            at += k
        assert (st.n == total).all()
        rgb, var, samples = twin_output(st)
        assert same(rgb, st.mean) and (samples == total).all()
        m = x.mean(axis=2)
        ref_v = ((x - m[:, :, None]) ** 2).sum(axis=2) / (total * (total - 1))
        e = max(rel_err(rgb, m), rel_err(var, ref_v))
        worst = max(worst, e)
        assert e <= BAR, (sizes, seed, e)
    print("batches", sizes, "largest relative error of the merge vs pooled float64:", worst)


def test_merge_touches_only_the_listed_pixels():
    st = State(5, 7)
    rng = np.random.default_rng(3)
    b, v = rng.random((5, 7, 3)).astype(np.float32), rng.random((5, 7, 3)).astype(np.float32)
    lst = np.array([3, 0, 34, 17], np.uint32)
    twin_merge(st, lst, 4, True, b, v)
    listed = np.zeros(35, bool)
    listed[lst] = True
    assert (st.n.reshape(-1) == np.where(listed, 4, 0)).all()
    assert same(st.mean.reshape(-1, 3)[listed], b.reshape(-1, 3)[listed]) and not st.mean.reshape(-1, 3)[~listed].any()
    assert same(st.m2.reshape(-1, 3)[listed], v.reshape(-1, 3)[listed] * np.float32(12.0)) and not st.m2.reshape(-1, 3)[~listed].any()
    twin_merge(st, lst[:2], 2, False, b, v)   # the same value again: the mean stands, m2 grows by v * 2
    assert (st.n.reshape(-1)[lst] == [6, 6, 4, 4]).all()
    assert same(st.mean.reshape(-1, 3)[lst], b.reshape(-1, 3)[lst])
    assert same(st.m2.reshape(-1, 3)[lst[:2]], v.reshape(-1, 3)[lst[:2]] * np.float32(12.0) + v.reshape(-1, 3)[lst[:2]] * np.float32(2.0))
    rgb, var, samples = twin_output(st)
    assert same(var.reshape(-1, 3)[lst[2:]], st.m2.reshape(-1, 3)[lst[2:]] / np.float32(12.0)) and not var.reshape(-1, 3)[~listed].any()


SELECT_CASES = [(1, 1, 0), (5, 7, 1), (1, 64, 2), (3, 65, 3), (29, 37, 4), (17, 300, 5)]   # (h, w, seed)
TARGET, MAX_SPP, ROUND_SPP = 0.1, 32, 4


@pytest.mark.parametrize("h,w,seed", SELECT_CASES, ids=lambda v: str(v))
def test_selection_matches_the_model(h, w, seed):
    st = make_state(h, w, seed)
    for lst in (np.arange(h * w, dtype=np.uint32), tile_order(w, h), tile_order(w, h)[::3]):
        ref, band = model_select(st, lst, MAX_SPP, ROUND_SPP, TARGET)
        assert band.size == 0, "an input lies in the excluded band: choose another seed"   # so the comparison below excludes nothing
        got = twin_select(st, lst, min_spp=4, max_spp=MAX_SPP, round_spp=ROUND_SPP, target_error=TARGET)
        assert np.array_equal(got, ref)   # the same pixels, in the order of the list
    if h * w >= 64:   # (the last list: every third entry in tile order)
        assert 0 < ref.size < lst.size
    e2, m = twin_error(st), model_e2(st)
    assert rel_err(e2[st.n > 0], m[st.n > 0]) < 1e-5
    assert not e2[st.n == 0].any()


def lone_noisy_pixel(h, w, y, x, n_at=8):
    """a calm film (no variance) with one noisy pixel"""
    st = State(h, w)
    st.n[...] = 8
    st.mean[...] = 0.5
    st.n[y, x] = n_at
    st.m2[y, x] = 1.0 if n_at else 5.0   # (state no render leaves: m2 without samples — it must not be read)
    return st


@pytest.mark.parametrize("y,x", [(0, 0), (0, 6), (4, 0), (4, 6), (0, 3), (2, 0), (2, 3)])
def test_a_noisy_pixel_selects_its_neighbourhood_inside_the_film(y, x):
    st = lone_noisy_pixel(5, 7, y, x)
    got = twin_select(st, min_spp=8, max_spp=64, round_spp=8, target_error=0.05)
    want = [qy * 7 + qx for qy in range(5) for qx in range(7) if abs(qy - y) <= 1 and abs(qx - x) <= 1]
    assert got.tolist() == want
    ref, band = model_select(st, np.arange(35), 64, 8, 0.05)
    assert band.size == 0 and ref.tolist() == want


def test_neighbours_without_samples_are_skipped():
    st = lone_noisy_pixel(5, 7, 2, 3, n_at=0)
    assert twin_select(st, min_spp=8, max_spp=64, round_spp=8, target_error=0.05).size == 0
    # ... and a pixel with one sample counts as calm (V = 0 below two samples), yet takes its neighbours' variance
    st = lone_noisy_pixel(5, 7, 2, 3)
    st.n[2, 4] = 1
    assert (2 * 7 + 4) in twin_select(st, min_spp=8, max_spp=64, round_spp=8, target_error=0.05).tolist()
    st.m2[2, 3] = 0
    st.m2[2, 4] = 1.0
    assert twin_select(st, min_spp=8, max_spp=64, round_spp=8, target_error=0.05).size == 0


def test_the_cut_off_at_max_spp():
    st = lone_noisy_pixel(3, 3, 1, 1)
    st.n[0, :] = (24, 25, 32)
    got = twin_select(st, min_spp=8, max_spp=32, round_spp=8, target_error=0.05).tolist()
    assert got == [0, 3, 4, 5, 6, 7, 8]   # 24 + 8 <= 32 stays; 25 and 32 are full
    assert twin_select(st, min_spp=8, max_spp=8, round_spp=8, target_error=0.05).size == 0


def test_order_is_list_order_and_an_empty_list_is_empty():
    st = make_state(29, 37, 4)
    lst = np.random.default_rng(0).permutation(29 * 37).astype(np.uint32)
    got = twin_select(st, lst, min_spp=4, max_spp=MAX_SPP, round_spp=ROUND_SPP, target_error=TARGET)
    ref, _ = model_select(st, lst, MAX_SPP, ROUND_SPP, TARGET)
    assert np.array_equal(got, ref) and got.size > 0
    assert twin_select(st, lst[:0], min_spp=4, max_spp=MAX_SPP, round_spp=ROUND_SPP, target_error=TARGET).size == 0
    assert twin_select(st, lst, min_spp=4, max_spp=MAX_SPP, round_spp=ROUND_SPP, target_error=1e30).size == 0
    everything = twin_select(st, lst, min_spp=4, max_spp=MAX_SPP, round_spp=ROUND_SPP, target_error=1e-30)
    n = st.n.reshape(-1)[lst]
    assert np.array_equal(everything, lst[(n > 0) & (n + ROUND_SPP <= MAX_SPP)])   # (every pixel of this state has variance)


def test_defaults_and_refusals():
    assert twin_params() == (0, dict(min_spp=16, max_spp=256, round_spp=16, max_rounds=16, target_error=np.float32(0.05)))
    assert twin_params(min_spp=4, target_error=0.25)[1] == dict(min_spp=4, max_spp=64, round_spp=4, max_rounds=16, target_error=0.25)
    assert twin_params(min_spp=8, max_spp=8, round_spp=3, max_rounds=64)[0] == 0
    for bad in (dict(min_spp=1), dict(min_spp=8, max_spp=7), dict(max_spp=15), dict(max_spp=(1 << 20) + 1), dict(max_rounds=65),
                dict(target_error=-0.1), dict(target_error=float("nan")), dict(target_error=float("inf"))):
        assert twin_params(**bad)[0] != 0, bad
    assert twin_params(max_spp=1 << 20)[0] == 0


def test_round_seeds():
    assert twin_seed(5, 0) == 5 and twin_seed(5, 3) == (5 + 3 * SEED_STEP) % (1 << 64)
    assert twin_seed((1 << 64) - SEED_STEP, 1) == 1   # a sum of 0 becomes 1: 0 would ask for the default seed
    assert pairs(5) == 20
