"""bench.py's multi-GPU launcher: ``--gpus N`` starts N ranks as a child
``torch.distributed.run``, and a rank whose WORLD_SIZE differs from --gpus exits non-zero.
CPU only: the launch itself is captured, and the mismatch exits before any HIP call."""
from __future__ import annotations

import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_launch_command_shape():
    cmd = bench.launch_command(8, ["--gpus", "8", "--steps", "5"], 29517)
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nnodes=1" in cmd and "--nproc-per-node=8" in cmd
    assert "--master-addr=127.0.0.1" in cmd and "--master-port=29517" in cmd
    i = cmd.index(os.path.join(ROOT, "bench.py"))
    assert cmd[i + 1:] == ["--gpus", "8", "--steps", "5"]


def test_maybe_launch_spawns_child_and_relays_rc(monkeypatch):
    seen = {}

    class R:
        returncode = 7

    def fake_run(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return R()

    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(bench.subprocess, "run", fake_run)
    args = bench.parse_args(["--gpus", "4", "--steps", "3"])
    assert bench.maybe_launch(args, ["--gpus", "4", "--steps", "3"]) == 7
    assert "--nproc-per-node=4" in seen["cmd"]
    assert seen["cmd"][-4:] == ["--gpus", "4", "--steps", "3"]
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_maybe_launch_single_and_inside_rank(monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert bench.maybe_launch(bench.parse_args([]), []) is None
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert bench.maybe_launch(bench.parse_args(["--gpus", "2"]), []) is None
    assert bench.maybe_launch(bench.parse_args(["--gpus", "1"]), []) == 2
    assert bench.maybe_launch(bench.parse_args(["--gpus", "8"]), []) == 2


@pytest.mark.parametrize("gpus,world", [("1", "2"), ("8", "4")])
def test_world_size_mismatch_exits_nonzero(gpus, world):
    env = dict(os.environ, WORLD_SIZE=world, RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", gpus, "--steps", "1"],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2, r.stderr
    assert f"WORLD_SIZE={world} but --gpus {gpus}" in r.stderr
    assert r.stdout.strip() == ""  # no bench line from a wrong-sized job


def test_dump_outputs_whole_and_sampled(tmp_path):
    """--dump-outputs: small arrays whole, large ones as the same seeded sample every time; float32 out
    (float64 stays float64, integers become float32)."""
    import numpy as np
    import torch

    n = 5 * (bench.DUMP_MAX_ELEMS // 5 + 2469)
    big = torch.arange(n, dtype=torch.float32).reshape(-1, 5)
    outs = {"small": torch.arange(12, dtype=torch.int32).reshape(3, 4), "big": big,
            "count": torch.tensor([7.0], dtype=torch.float64), "absent": None}
    info = bench.dump_outputs(str(tmp_path / "a"), outs)
    bench.dump_outputs(str(tmp_path / "b"), {"big": big + 1.0})
    assert sorted(os.listdir(tmp_path / "a")) == ["big.npy", "count.npy", "small.npy"]
    small, count = np.load(tmp_path / "a" / "small.npy"), np.load(tmp_path / "a" / "count.npy")
    assert small.dtype == np.float32 and small.shape == (3, 4) and small[2, 3] == 11
    assert count.dtype == np.float64 and count.tolist() == [7.0]
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.dtype == np.float32 and a.shape == (bench.DUMP_MAX_ELEMS,)
    np.testing.assert_array_equal(b, a + 1.0)  # the same elements in both dumps
    assert (np.diff(a) >= 0).all() and a[0] >= 0 and a[-1] < n and len(np.unique(a)) > 0.5 * len(a)
    assert info["big"] == {"shape": [n // 5, 5], "written": bench.DUMP_MAX_ELEMS, "sampled": True}
    assert info["small"] == {"shape": [3, 4], "written": 12, "sampled": False}
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) < 64e6


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    """A plain run prints the headline line without the --full figures, runs exactly --steps timed steps and
    writes the last step's outputs; the same arguments give the same image again."""
    import json

    import numpy as np

    def run(d):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup",
                            "1", "--ramp-seconds", "0", "--config", "10k_256_sh0", "--dump-outputs", str(d)],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.strip().splitlines()
        assert len(lines) == 1
        return json.loads(lines[0])

    line = run(tmp_path / "a")
    assert line["full"] is False and line["steps"] == 2 and line["warmup"] == 1
    assert line["unit"] == "Gaussian-splats/s" and line["higher_is_better"] is True and line["dtype"] == "fp32"
    assert line["ms_per_step"] > 0 and abs(line["value"] - 10_000 / (line["ms_per_step"] * 1e-3)) <= 1e-6 * line["value"]
    assert line["host"]["step_wall_ms"]["mean"] > 0 and line["host"]["lib_forward_ms"]["calls"] == 2
    for k in ("roofline", "work", "stage_ms", "cpu_baseline", "cpu_baseline_c"):
        assert k not in line
    names = {"color", "invdepth", "radii", "num_rendered", "dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D",
             "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations"}
    assert set(line["outputs"]["arrays"]) == names
    assert {f[:-4] for f in os.listdir(tmp_path / "a")} == names
    color = np.load(tmp_path / "a" / "color.npy")
    assert color.dtype == np.float32 and color.shape == (3, 256, 256) and np.isfinite(color).all() and color.any()
    assert np.load(tmp_path / "a" / "num_rendered.npy")[0] == line["config"]["num_rendered"]
    assert np.load(tmp_path / "a" / "dL_dsh.npy").shape == (10_000, 1, 3)
    run(tmp_path / "b")
    np.testing.assert_array_equal(np.load(tmp_path / "b" / "color.npy"), color)
    np.testing.assert_array_equal(np.load(tmp_path / "b" / "radii.npy"), np.load(tmp_path / "a" / "radii.npy"))


def test_cpu_threads_affinity(monkeypatch):
    aff = len(os.sched_getaffinity(0))
    monkeypatch.delenv("OMP_NUM_THREADS", raising=False)
    n, facts = bench.cpu_threads()
    assert n == aff and facts["affinity_cpus"] == aff and facts["omp_num_threads"] is None
    monkeypatch.setenv("OMP_NUM_THREADS", "1")
    n, facts = bench.cpu_threads()
    assert n == 1 and facts["omp_num_threads"] == 1
