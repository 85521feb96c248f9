"""The candidate pool of k_mega's leaf scan (device/dmegapool.h: one wave prefix sum over the lanes' candidate counts, every lane listing its
own candidates from the index the sum gives it, as many per pass as the pool holds) run on the host as a model of one wave (tests/twin_pool):
64 lanes with given masks, the prefix sum a plain loop.  A wrong end condition would be a wave that never ends on the GPU, and a wrong share
an LDS write past the pool, so they are checked here first: every (lane, kind, leaf) of the masks is listed exactly once over all passes and
nothing else, every pass writes exactly the indices 0 .. n_items - 1 with n_items <= cap, and the pass count is ceil(total / cap)."""
import ctypes as C

import numpy as np
import pytest

from lajolla_public_amd import build

CAPS = [1, 63, 64, 65, 304, 512]
N_USED = [1, 18, 32]

_lib = None


def _twin():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build.build_twin_pool(verbose=False))
        _lib.twin_pool_run.restype = C.c_int
        _lib.twin_pool_run.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    return _lib


def _expected(ms, me, n_used):
    """(lane, kind, leaf) of every set bit: kind 1 is the shadow ray's mask; bit b stands for leaf n_used - 1 - b."""
    out = set()
    for lane in range(64):
        for kind, m in ((1, int(ms[lane])), (0, int(me[lane]))):
            for b in range(32):
                if m >> b & 1:
                    out.add((lane, kind, n_used - 1 - b))
    return out


def _check(ms, me, n_used, cap):
    ms = np.ascontiguousarray(ms, dtype=np.uint32); me = np.ascontiguousarray(me, dtype=np.uint32)
    assert not (ms >> n_used).any() and not (me >> n_used).any() if n_used < 32 else True
    want = _expected(ms, me, n_used)
    total = len(want)
    n_pass = -(-total // cap)
    listed = np.zeros(total + 8, np.uint64)
    n_listed = np.zeros(1, np.uint64)
    pass_items = np.zeros(n_pass + 2, np.uint32)
    faults = np.zeros(4, np.uint64)
    # no pass loop over `total` candidates may need more than ceil(total / cap) passes: one more is the model's stand-in for a hang
    rc = _twin().twin_pool_run(ms.ctypes.data, me.ctypes.data, n_used, cap, n_pass + 1, listed.ctypes.data, len(listed), n_listed.ctypes.data,
                               pass_items.ctypes.data, faults.ctypes.data)
    assert rc >= 0, f"the pass loop was still running after {n_pass + 1} passes"
    assert rc == n_pass, f"{rc} passes for {total} candidates at cap {cap}"
    assert faults[0] == 0, "an index outside [0, n_items) was written"
    assert faults[1] == 0, "a slot was written twice in one pass"
    assert faults[2] == 0, "a slot of [0, n_items) was never written"
    assert faults[3] == 0, "the end test disagreed with the masks"
    assert int(n_listed[0]) == total
    got = [(int(x) & 0xff, int(x) >> 8 & 0xff, int(x) >> 16 & 0xffff) for x in listed[:total]]
    assert len(set(got)) == total, "a candidate was listed twice"
    assert set(got) == want
    # the passes: every one full but the last
    items = [int(x) for x in pass_items[:n_pass]]
    assert all(1 <= n <= cap for n in items) and sum(items) == total
    assert items[:-1] == [cap] * (n_pass - 1) if n_pass else items == []
    # shadow candidates first, lowest bit (highest leaf) first, within every lane; lanes in order
    per_lane = {}
    for lane, kind, leaf in got:
        per_lane.setdefault(lane, []).append((1 - kind, -leaf))
    assert all(v == sorted(v) for v in per_lane.values())
    assert [g[0] for g in got] == sorted(g[0] for g in got)


def _random_masks(rng, n_used, max_bits):
    """Per lane and mask up to max_bits random bits below n_used."""
    ms = np.zeros(64, np.uint32); me = np.zeros(64, np.uint32)
    for m in (ms, me):
        for lane in range(64):
            k = int(rng.integers(0, max_bits + 1))
            for b in rng.integers(0, n_used, k):
                m[lane] |= np.uint32(1) << np.uint32(b)
    return ms, me


def _full(n_used):
    return np.uint32((1 << n_used) - 1)


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("n_used", N_USED)
def test_random_masks_sparse_and_dense(n_used, cap):
    rng = np.random.default_rng(100 * n_used + cap)
    for max_bits in (3, 3, 3, 32):   # 0-6 bits per lane as on cbox (three draws), and dense
        _check(*_random_masks(rng, n_used, max_bits), n_used, cap)


@pytest.mark.parametrize("cap", CAPS)
def test_all_lanes_full_4096_items(cap):
    _check(np.full(64, 0xffffffff, np.uint32), np.full(64, 0xffffffff, np.uint32), 32, cap)


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("n_used", N_USED)
def test_all_lanes_every_leaf(n_used, cap):
    _check(np.full(64, _full(n_used), np.uint32), np.full(64, _full(n_used), np.uint32), n_used, cap)


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("lane", [0, 31, 63])
def test_one_lane_with_64_bits(lane, cap):
    ms = np.zeros(64, np.uint32); me = np.zeros(64, np.uint32)
    ms[lane] = me[lane] = 0xffffffff
    _check(ms, me, 32, cap)


@pytest.mark.parametrize("cap", [63, 64, 65, 304, 512])
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_total_around_the_cap(cap, delta):
    # cap + delta candidates, dealt round the lanes a bit at a time (so that the pass boundary falls inside a lane's candidates)
    total = cap + delta
    ms = np.zeros(64, np.uint32); me = np.zeros(64, np.uint32)
    for i in range(total):
        lane, j = i % 64, i // 64
        (ms if j % 2 == 0 else me)[lane] |= np.uint32(1) << np.uint32(j // 2)
    assert len(_expected(ms, me, 32)) == total
    _check(ms, me, 32, cap)


@pytest.mark.parametrize("cap", CAPS)
def test_empty_masks_run_no_pass(cap):
    z = np.zeros(64, np.uint32)
    faults = np.zeros(4, np.uint64); n_listed = np.ones(1, np.uint64); listed = np.zeros(8, np.uint64); pass_items = np.zeros(2, np.uint32)
    rc = _twin().twin_pool_run(z.ctypes.data, z.ctypes.data, 18, cap, 1, listed.ctypes.data, 8, n_listed.ctypes.data, pass_items.ctypes.data, faults.ctypes.data)
    assert rc == 0 and n_listed[0] == 0 and not faults.any()
