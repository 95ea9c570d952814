"""bench.py orchestration under gloo on CPU: the
driver's exact torchrun launch shape at world 2 and 8 must run
end-to-end — rank env parsing, plane-aligned layout, halo exchange,
barrier+sync protocol, max-over-ranks reduction, rank-0 JSON line —
before any 8-GPU lease exists.  --smoke-gloo swaps the GPU kernel for a
tiny torch stand-in; it never touches the measured path."""
import json
import os
import socket
import subprocess
import sys

import pytest


def _free_port():
    # a fixed port flakes: TIME_WAIT from the previous world's
    # rendezvous can hold it for ~60 s
    with socket.socket() as sck:
        sck.bind(("127.0.0.1", 0))
        return sck.getsockname()[1]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("world", [2, 8])
def test_bench_smoke_gloo(world):
    env = dict(os.environ)
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, "-m", "torch.distributed.run",
           "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()),
           os.path.join(ROOT, "bench.py"),
           "--gpus", str(world), "--steps", "2", "--warmup", "1",
           "--smoke-gloo"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300,
                         cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    res = json.loads(lines[0])
    assert res["smoke"] is True
    assert res["n_gpus"] == world
    assert res["value"] > 0
    assert res["steps"] == 2
    assert res["config"]["dims"][0] == 64 * world


def test_bench_smoke_gloo_world1():
    env = dict(os.environ)
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"),
           "--gpus", "1", "--steps", "2", "--warmup", "1", "--smoke-gloo"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=180,
                         cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads([ln for ln in out.stdout.splitlines()
                      if ln.startswith("{")][0])
    assert res["smoke"] is True and res["n_gpus"] == 1


def test_bench_dump_outputs_repeatable(tmp_path):
    """--dump-outputs writes the last step's output as float64 .npy, and
    two runs with the same arguments write the same numbers.  A plain
    run carries no cpu_baseline leg and reports ms_per_step."""
    import numpy as np
    env = dict(os.environ)
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    dumps = []
    for name in ("a", "b"):
        d = tmp_path / name
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"),
               "--gpus", "1", "--steps", "3", "--warmup", "1",
               "--smoke-gloo", "--dump-outputs", str(d)]
        out = subprocess.run(cmd, capture_output=True, text=True,
                             timeout=180, cwd=ROOT, env=env)
        assert out.returncode == 0, out.stderr[-2000:]
        res = json.loads([ln for ln in out.stdout.splitlines()
                          if ln.startswith("{")][0])
        assert res["steps"] == 3 and res["ms_per_step"] > 0
        assert res["cpu_baseline"] is None
        files = sorted(p.name for p in d.iterdir())
        assert files == ["z.npy"]
        dumps.append(np.load(d / "z.npy"))
    assert dumps[0].dtype == np.float64
    assert dumps[0].size == 64 * 32 * 16
    assert np.isfinite(dumps[0]).all() and np.abs(dumps[0]).max() > 0
    np.testing.assert_array_equal(dumps[0], dumps[1])


def test_bench_dump_sampling(tmp_path, monkeypatch):
    """An output over the budget is sampled at fixed, seeded positions:
    the same positions every call, every value taken from the array."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    from pylops_mpi_amd.comm import PamComm
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 100)
    t = torch.arange(1000, dtype=torch.float64) * 0.5
    comm = PamComm(0, 1, torch.device("cpu"))
    bench.dump_outputs(str(tmp_path / "a"), {"y": t}, comm)
    bench.dump_outputs(str(tmp_path / "b"), {"y": t + 1.0}, comm)
    a = np.load(tmp_path / "a" / "y.npy")
    b = np.load(tmp_path / "b" / "y.npy")
    assert a.dtype == np.float64 and a.shape == (100,)
    np.testing.assert_array_equal(b, a + 1.0)       # same positions
    assert np.all(np.diff(a) >= 0) and len(np.unique(a)) > 50
    assert np.all((a * 2) == np.round(a * 2)) and a.max() < 500.0
