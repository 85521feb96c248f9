"""The test rounds of a pass of k_mega's leaf scan (mega.hip: scan_trace) run on the host as a model of one wave (tests/twin_round) over the
kernel's own round arithmetic (device/dmegapool.h).  A pass walks its items 64 at a time, every lane the primitives of its item's leaf; a last
round of m items with m * M <= 64 — M the largest leaf count of the scene rounded up to a power of two — runs split instead: lane l takes
primitive l % M of item r + l / M.  (A round too long for M lanes per item shares an item among the widest power of two W < M of lanes that
still fits, each walking every W-th primitive: cbox has one leaf of four triangles among seventeen of two.)  A wrong mapping would test a pair twice or not at all (a missed hit), or read the item list beyond the
pass (LDS of the next wave), so it is checked here first: for M in {1, 2, 4, 8}, every m from 0 to 64 alone and behind one or two full
rounds, and leaf counts from 1 to M mixed within a round, the split is taken exactly when m * M <= 64 and M > 1, every (item, primitive
below its leaf's count) pair is tested exactly once and nothing else, and no lane reads an item at or beyond n_items."""
import ctypes as C

import numpy as np
import pytest

from lajolla_public_amd import build

_lib = None


def _twin():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build.build_twin_round(verbose=False))
        _lib.twin_round_split_width.restype = C.c_uint32
        _lib.twin_round_split_width.argtypes = [C.c_uint32]
        _lib.twin_round_run.restype = C.c_uint32
        _lib.twin_round_run.argtypes = [C.c_uint32, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    return _lib


def _run(M, counts, split=True):
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    n = len(counts)
    visits = np.zeros(max(n, 1) * 8, np.uint32)
    round_m = np.zeros(16, np.uint32)
    faults = np.zeros(3, np.uint64)
    rounds = _twin().twin_round_run(M, int(split), n, counts.ctypes.data, visits.ctypes.data, round_m.ctypes.data, len(round_m), faults.ctypes.data)
    return rounds, visits.reshape(-1, 8)[:n], [(int(x) & 0xffff, int(x) >> 16) for x in round_m[:rounds]], faults


def _check(M, counts, split=True):
    n = len(counts)
    rounds, visits, decided, faults = _run(M, counts, split)
    assert faults[0] == 0, "a lane read an item at or beyond n_items"
    assert faults[1] == 0, "a primitive at or beyond its leaf's count was tested"
    assert faults[2] == 0, "a lane of a split round tested more than one primitive"
    assert rounds == -(-n // 64)
    want = (np.arange(8)[None, :] < np.asarray(counts, np.uint32).reshape(-1, 1)).astype(np.uint32)
    assert np.array_equal(visits, want), "an (item, primitive) pair was tested twice or not at all"
    # the decisions: round k is entered with n - 64 k items; it runs one primitive per lane (M lanes per item) exactly when m * M <= 64 and
    # M > 1; a round too long for that takes the widest power of two W < M with m * W <= 64 (W = 1: not split — every round but the last)
    log2m = {1: 0, 2: 1, 4: 2, 8: 3}[M]
    for k, (m, shift) in enumerate(decided):
        assert m == n - 64 * k
        assert (shift == log2m and M > 1) == (split and M > 1 and m * M <= 64), f"round of {m} items at M = {M}: shift {shift}"
        want_shift = max(s for s in range(log2m + 1) if s == 0 or m << s <= 64) if split else 0
        assert shift == want_shift, f"round of {m} items at M = {M}: shift {shift}, expected {want_shift}"
        assert m <= 64 or shift == 0


@pytest.mark.parametrize("M", [1, 2, 4, 8])
def test_every_last_round_after_0_1_2_full_rounds(M):
    rng = np.random.default_rng(7 * M)
    for full in (0, 1, 2):
        for m in range(0, 65):
            n = 64 * full + m
            _check(M, rng.integers(1, M + 1, n))            # counts from 1 to M, mixed within a round
            _check(M, np.full(n, M))                        # every leaf full: every lane of a split round busy
            _check(M, np.full(n, 1))                        # every leaf one primitive: one lane in M busy


@pytest.mark.parametrize("M", [1, 2, 4, 8])
def test_a_build_without_the_split_runs_the_same_tests(M):
    rng = np.random.default_rng(11 * M)
    for n in (0, 1, 7, 8, 32, 33, 64, 65, 96, 97, 150, 304, 512):
        _check(M, rng.integers(1, M + 1, n), split=False)


def test_the_boundary_m_times_M_equals_64():
    for M, m in ((2, 32), (4, 16), (8, 8)):
        assert _run(M, np.full(m, M))[2] == [(m, {2: 1, 4: 2, 8: 3}[M])]
        assert _run(M, np.full(m + 1, M))[2] == [(m + 1, {2: 1, 4: 2, 8: 3}[M] - 1)]   # (one lane per item at M = 2)
        assert _run(M, np.full(64 + m, M))[2] == [(64 + m, 0), (m, {2: 1, 4: 2, 8: 3}[M])]
    for M in (2, 4, 8):
        assert _run(M, np.full(32, M))[2][0][1] >= 1 and _run(M, np.full(33, M))[2] == [(33, 0)]   # above 32 items nothing is shared
    assert _run(1, np.full(1, 1))[2] == [(1, 0)]            # M = 1 never splits


def test_split_width_is_the_count_rounded_up_to_a_power_of_two():
    w = _twin().twin_round_split_width
    assert [w(c) for c in range(0, 10)] == [1, 1, 2, 4, 4, 8, 8, 8, 8, 16]
