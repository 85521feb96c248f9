"""The sample bookkeeping of k_mega (device/dregen.h: the wave's open range off the grid counter and its stash of camera samples generated
64 at a time) run on the host as a model of a persistent grid (tests/twin_regen): several waves of 64 lanes against one shared counter,
every path a seeded random number of steps long.  A wrong end condition would be a hang on the GPU, so it is checked here first:
every sample is handed out exactly once, no refill overwrites an unread slot, and every wave ends within the iterations its own
samples can account for."""
import ctypes as C
import itertools

import numpy as np
import pytest

from lajolla_public_amd import build

MAX_LEN = 12   # steps of the longest path in the model (cbox: 4.02 on average)

_lib = None


def _twin():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build.build_twin_regen(verbose=False))
        _lib.twin_regen_run.restype = C.c_int
        _lib.twin_regen_run.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint64] + [C.c_void_p] * 5
    return _lib


def _run(n, grab, waves, seed, path_len=None):
    rng = np.random.default_rng(seed)
    if path_len is None:   # most paths short, a few long: min of two uniform draws, 1 .. MAX_LEN
        path_len = np.minimum(rng.integers(1, MAX_LEN + 1, n), rng.integers(1, MAX_LEN + 1, n)).astype(np.uint32)
    path_len = np.ascontiguousarray(path_len, dtype=np.uint32)
    handed = np.full(n, 0xffffffff, np.uint32)
    iters, steps, own = (np.zeros(waves, np.uint64) for _ in range(3))
    faults = np.zeros(4, np.uint64)
    # no wave can run more iterations than one per path step of the whole frame, plus the one in which it finds the counter exhausted
    cap = 1 + int(path_len.sum())
    rc = _twin().twin_regen_run(n, grab, waves, seed, path_len.ctypes.data, cap, handed.ctypes.data, iters.ctypes.data, steps.ctypes.data,
                                own.ctypes.data, faults.ctypes.data)
    return rc, path_len, handed, iters, steps, own, faults


CASES = list(itertools.product([1, 63, 64, 65, 1280, 4099], [64, 192, 768], [1, 4, 37]))


@pytest.mark.parametrize("n,grab,waves", CASES)
def test_every_sample_once_no_slot_lost_and_every_wave_ends(n, grab, waves):
    for seed in (1, 2, 3):
        rc, path_len, handed, iters, steps, own, faults = _run(n, grab, waves, seed)
        assert rc == 0, f"a wave was still running after {1 + int(path_len.sum())} iterations"
        assert np.array_equal(handed, np.ones(n, np.uint32)), f"samples not handed out exactly once: {np.flatnonzero(handed != 1)[:8]}"
        assert faults[0] == 0, "a refill overwrote an unread slot"
        assert faults[1] == 0, "a lane was served from a slot that held nothing, or a wave ended with unread slots"
        assert faults[2] == 0, "a sample id beyond the frame was handed out"
        assert faults[3] == 0, "an iteration left no lane live and the wave did not end"
        # every path step of the frame is executed, by the wave that started the path
        assert np.array_equal(steps, own) and int(steps.sum()) == int(path_len.sum())
        # an iteration that does not end the wave leaves a lane live, whose step the next iteration executes: a wave runs at most one
        # iteration per path step of its own samples, plus the last one
        assert (iters <= own + 1).all() and (iters >= 1).all()
        # ... and a wave with all 64 lanes busy cannot need fewer than steps / 64
        assert (iters * 64 >= steps).all()


def test_paths_of_one_step_refill_every_iteration():
    # every lane dies in every step: each iteration serves 64 lanes, the stash is drained and refilled every time
    n, grab, waves = 4099, 192, 4
    rc, path_len, handed, iters, steps, own, faults = _run(n, grab, waves, 5, path_len=np.ones(n, np.uint32))
    assert rc == 0 and not faults.any() and np.array_equal(handed, np.ones(n, np.uint32))
    assert (iters <= own + 1).all() and int(iters.sum()) >= n // 64


def test_one_long_path_keeps_its_wave_and_no_other():
    n, grab, waves = 65, 64, 4
    path_len = np.ones(n, np.uint32); path_len[64] = 1000
    rc, _, handed, iters, steps, own, faults = _run(n, grab, waves, 9, path_len=path_len)
    assert rc == 0 and not faults.any() and np.array_equal(handed, np.ones(n, np.uint32))
    assert sorted(iters)[-1] in (1001, 1002) and sorted(iters)[-2] <= 3
