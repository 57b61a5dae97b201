"""The bench's N-rank launch path on the CPU (gloo, --selftest-cpu): `bench.py --gpus 2` spawns two
ranks through torch.distributed.run, shards the global batch by rank, takes the max over ranks,
reports n_gpus = 2, and the audio gathered to rank 0 equals the single-rank run's bit for bit.  The gather figures
are legs of `--full`; `--dump-outputs` writes the last timed step's audio."""
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(n, tmp_path, batch=3, extra=()):
    dump = str(tmp_path / f"audio_{n}.npy")
    outdir = tmp_path / f"outputs_{n}"
    env = dict(os.environ, OMP_NUM_THREADS="1")
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--selftest-cpu",
                        "--steps", "2", "--warmup", "1", "--batch", str(batch), "--frames", "4",
                        "--dump-checksum", dump, "--dump-outputs", str(outdir), *extra], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout  # ONE JSON line, from rank 0
    return json.loads(lines[0]), np.load(dump), np.load(outdir / "audio.npy")


def test_two_rank_launch_matches_one_rank(tmp_path):
    one, a1, o1 = _run(1, tmp_path)
    two, a2, o2 = _run(2, tmp_path, extra=("--full",))
    assert one["n_gpus"] == 1 and two["n_gpus"] == 2
    assert two["config"]["global_batch"] == 6 and one["config"]["global_batch"] == 3
    assert two["scaling"] == "weak" and "with_gather" in two and "with_scatter_gather" in two
    assert a2.shape == (6, 1, 2400)
    # weak scaling: rank r holds global utterances [3r, 3r + 3); the single-rank run is utterances 0-2
    assert np.array_equal(a2[:3], a1)
    assert not np.array_equal(a2[3:], a1)
    # a plain run times its steps and nothing else; the result line keeps its headline fields
    assert "with_gather" not in one and "roofline" in one and one["steps"] == 2 and one["ms_per_step"] > 0
    # --dump-outputs: the last timed step (warm-up 1 + 2 steps: seed 1234 + 2), not the checksum's step 0
    assert o1.dtype == np.float32 and o1.shape == a1.shape and o2.shape == a2.shape
    assert np.array_equal(o2[:3], o1) and not np.array_equal(o1, a1)
    ids = torch.arange(3, dtype=torch.float64).reshape(3, 1, 1)
    t = torch.arange(2400, dtype=torch.float64).reshape(1, 1, -1)
    assert np.array_equal(o1, torch.sin(0.001 * t * (ids + 1) + float(1236 % 1000)).float().numpy())


def test_world_size_mismatch_fails_loudly(tmp_path):
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--selftest-cpu"],
                       capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode != 0 and "WORLD_SIZE" in (r.stderr + r.stdout)


def test_dump_outputs_bounds_and_samples(tmp_path, monkeypatch):
    """--dump-outputs writes float32 / float64 only and stays within its byte limit: a larger tensor is written as
    the same ascending sample of its flat values on every call."""
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT", 4000)
    small = torch.arange(12, dtype=torch.float64).reshape(3, 4)
    big = torch.arange(5000, dtype=torch.bfloat16).reshape(2, 1, 2500)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"small": small, "big": big})
    s, b = np.load(tmp_path / "a" / "small.npy"), np.load(tmp_path / "a" / "big.npy")
    assert s.dtype == np.float64 and np.array_equal(s, small.numpy())
    assert b.dtype == np.float32 and b.shape == (500,) and s.nbytes + b.nbytes <= 4000
    idx = np.sort(np.random.default_rng(0).choice(5000, size=500, replace=False))  # the documented sample
    assert np.array_equal(b, big.float().reshape(-1).numpy()[idx])
    assert np.array_equal(b, np.load(tmp_path / "b" / "big.npy"))
