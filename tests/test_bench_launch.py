"""`python3 bench.py --gpus N` as a PLAIN command (no torchrun, no WORLD_SIZE): bench.py starts its own N ranks before
anything touches the GPU and relays rank 0's single JSON line.  --dry_run stops after the rendezvous and the known-answer
collectives (metalign_amd/distributed.py::selfcheck_collectives), so the plumbing is checked here without a GPU; the same
command without --dry_run runs under `-m gpu` in tests/test_pipeline_gpu.py / tests/dist_two_ranks_one_gpu.py."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCH_VARS = ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "LOCAL_WORLD_SIZE", "GROUP_RANK")


def run_bench(*argv, **extra_env):
    env = {k: v for k, v in os.environ.items() if k not in LAUNCH_VARS}
    env.update({"MG_DIST_BACKEND": "gloo", **extra_env})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], env=env, capture_output=True, text=True, timeout=600)
    return p


@pytest.mark.parametrize("world", [2, 3])
def test_plain_command_spawns_its_own_ranks(world):
    p = run_bench("--gpus", str(world), "--dry_run")
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout  # ONE JSON line on stdout, whatever the launcher and gloo print elsewhere
    d = json.loads(lines[0])
    assert d["n_gpus"] == world and d["dry_run"] is True and d["collective_selfcheck"] == "ok" and d["backend"] == "gloo"


def test_one_gpu_dry_run_does_not_launch_anything():
    p = run_bench("--gpus", "1", "--dry_run")
    assert p.returncode == 0, p.stderr[-2000:]
    d = json.loads(p.stdout.strip().splitlines()[-1])
    assert d["n_gpus"] == 1 and d["collective_selfcheck"].startswith("skipped")


def test_a_failing_rank_fails_the_command():
    # an unknown backend makes init_process_group raise in every rank: the plain command must not exit 0 or print a line
    p = run_bench("--gpus", "2", "--dry_run", MG_DIST_BACKEND="no_such_backend")
    assert p.returncode != 0
    assert not [ln for ln in p.stdout.splitlines() if ln.startswith('{"metric"')]


def test_a_plain_run_leaves_the_extras_to_full(monkeypatch):
    """Without --full every part beyond the headline is off; --full turns them on, and a --no_* option still drops its part."""
    import bench
    extras = ("no_definitions", "no_cpu_baseline", "no_kernel_table", "no_secondary", "no_same_workload_n1")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert not a.full and all(getattr(a, x) for x in extras)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--full", "--no_secondary"])
    a = bench.parse()
    assert a.full and a.no_secondary and not any(getattr(a, x) for x in extras if x != "no_secondary")


def test_dump_outputs_are_float64_copies_and_a_seeded_sample_over_the_cap(tmp_path, monkeypatch):
    """--dump-outputs: every array a step returns as float64, exact; over the byte cap the same positions every time."""
    import numpy as np

    import bench
    step = {"hits_k": np.arange(12, dtype=np.uint32).reshape(3, 4), "sizes_k": np.full((3, 4), 9, dtype=np.uint32),
            "containment_k": np.arange(12).reshape(3, 4) / 9.0, "count": np.array([3, 0], dtype=np.uint64),
            "bases": np.array([450, 0], dtype=np.uint64), "first_seen": np.array([5, 2**64 - 1], dtype=np.uint64),
            "sketch_sizes": [77], "tot_rds": 3, "n_ambig": 1}
    arrays = bench.step_outputs(step)
    bench.dump_outputs(arrays, str(tmp_path / "all"))
    for name, a in arrays.items():
        got = np.load(tmp_path / "all" / (name + ".npy"))
        assert got.dtype == np.float64 and np.array_equal(got, a), name
    assert np.array_equal(np.load(tmp_path / "all" / "hits_k.npy"), step["hits_k"])
    assert np.load(tmp_path / "all" / "tot_rds_n_ambig.npy").tolist() == [3.0, 1.0]
    monkeypatch.setattr(bench, "DUMP_BYTES", 480)
    big = {"x": np.arange(100, dtype=np.float64), "y": -np.arange(50, dtype=np.float64)}
    for d in ("s1", "s2"):
        bench.dump_outputs(big, str(tmp_path / d))
    for name in big:
        a1, a2 = np.load(tmp_path / "s1" / (name + ".npy")), np.load(tmp_path / "s2" / (name + ".npy"))
        assert np.array_equal(a1, a2) and 0 < a1.size < big[name].size and np.isin(a1, big[name]).all()
    assert sum(np.load(tmp_path / "s1" / (n + ".npy")).nbytes for n in big) <= 480


def test_selfcheck_catches_misdelivered_data():
    """The known-answer check itself: a transport that swaps two ranks' all-gather contributions must be caught."""
    import numpy as np
    import torch

    from metalign_amd import distributed as mgd

    class OneRank:  # world 1 "transport" that corrupts the all-reduce
        class ReduceOp:
            SUM = 0

        def get_backend(self):
            return "gloo"

        def all_gather(self, outs, t):
            outs[0].copy_(t)

        def all_reduce(self, t, op=None):
            t[0] = t[0] & 0xffffffff  # a 32-bit reduction

    with pytest.raises(RuntimeError, match="all_reduce"):
        mgd.selfcheck_collectives(OneRank(), torch, 0, 1, "cpu")
    assert np  # (numpy is what the check compares with)
