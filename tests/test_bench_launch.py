"""bench.py's own N-rank launch on CPU: `python bench.py --gpus 2 --dry-launch` must start two ranks as child processes
(torch.distributed.run over 127.0.0.1), rendezvous them (gloo), sum-reduce the per-rank tile frames onto rank 0, relay
rank 0's single JSON line and return the children's exit code — the path the driver's multi-GPU run takes when nothing
wraps bench.py in a launcher.  No rendering happens in a dry launch (the hot path has no CPU form)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["OMP_NUM_THREADS"] = "1"
    return env


def test_bench_starts_its_own_ranks_and_relays_one_json_line():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-launch", "--steps", "2", "--warmup", "0"],
                       env=_env(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["dry_launch"] is True and out["reduce_exact"] is True
    assert out["config"]["parallelism"] == "tiles%2" and "reduce" in out["config"]["collective"]
    assert out["steps"] == 2 and out["ms_per_step"] > 0


def test_bench_refuses_a_world_size_that_contradicts_gpus():
    env = _env()
    env.update(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-launch"], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 2 and "WORLD_SIZE=1" in r.stderr


def test_single_rank_dry_launch_needs_no_process_group():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dry-launch", "--steps", "1"], env=_env(),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert out["n_gpus"] == 1 and out["reduce_exact"] is True


def test_dump_outputs_writes_the_reduced_frame(tmp_path):
    """--dump-outputs DIR: rank 0's reduced frame of the last timed step lands in DIR/frame.npy, float32, bit for bit."""
    import numpy as np
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-launch", "--steps", "2", "--warmup", "0",
                        "--dump-outputs", str(tmp_path)], env=_env(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.load(tmp_path / "frame.npy")
    want = np.arange(512 * 512 * 3, dtype=np.float32).reshape(512, 512, 3) + 1.0
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["frame.npy"]


def test_dump_outputs_samples_a_frame_over_the_size_limit(tmp_path, monkeypatch):
    """A frame larger than the limit is written as a seeded sample of its pixels, the same one every time."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096)
    frame = np.random.default_rng(1).random((64, 48, 3), dtype=np.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), frame)
    a, idx = np.load(tmp_path / "a" / "frame.npy"), np.load(tmp_path / "a" / "pixels.npy")
    assert a.nbytes + idx.nbytes <= 4096 and a.shape == (idx.shape[0], 3) and idx.shape[0] > 0
    assert np.array_equal(a, frame.reshape(-1, 3)[idx.astype(np.int64)])
    assert np.array_equal(a, np.load(tmp_path / "b" / "frame.npy")) and np.array_equal(idx, np.load(tmp_path / "b" / "pixels.npy"))
