"""bench.py's own contract: a plain run prints the headline line only, `--full` adds the secondary records, `--dump-outputs`
writes the timed path's outputs (the same files from run to run)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


class _StubRunner:
    """The attributes dump_outputs reads, on host tensors: checkpoint i holds the value i everywhere."""

    def __init__(self, N, K, forward_only=False):
        import torch
        import bench
        self.K, self.forward_only = K, forward_only
        rows = torch.arange(N, dtype=torch.float32)[:, None].expand(N, 3)
        self.states = bench._States([(rows + i, -(rows + i)) for i in range(K + 1)])
        self.xb, self.vb = rows * 2, rows * 3
        self.sbar = torch.arange(2 * K + 1, dtype=torch.float64)


@pytest.mark.parametrize("N,steps,forward_only", [(1000, 7, False), (1000, 20, True), (600000, 13, False)])
def test_dump_outputs_files(tmp_path, N, steps, forward_only):
    import bench
    K = 5
    r = _StubRunner(N, K, forward_only)
    bench.dump_outputs(r, steps, str(tmp_path / "a"))
    bench.dump_outputs(r, steps, str(tmp_path / "b"))
    names = sorted(os.listdir(tmp_path / "a"))
    expect = ["final_disp.npy", "final_vel.npy"] + ([] if forward_only else ["pos_cotangent.npy", "scalar_cotangents.npy", "vel_cotangent.npy"])
    if N > bench.DUMP_ROWS:
        expect.append("row_index.npy")
    assert names == sorted(expect)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in names) <= 64 << 20
    d = {f[:-4]: np.load(tmp_path / "a" / f) for f in names}
    for f in names:                                                  # same arguments, same files
        assert np.array_equal(np.load(tmp_path / "b" / f), d[f[:-4]])
        assert d[f[:-4]].dtype in (np.float32, np.float64)
    rows = d["row_index"].astype(np.int64) if N > bench.DUMP_ROWS else np.arange(N)
    assert len(rows) == min(N, bench.DUMP_ROWS) and len(np.unique(rows)) == len(rows)
    s = (steps - 1) % K + 1                                          # final state of the last replayed block
    assert np.array_equal(d["final_disp"], np.repeat(rows[:, None] + s, 3, 1).astype(np.float32))
    assert np.array_equal(d["final_vel"], -d["final_disp"])
    if not forward_only:
        assert np.array_equal(d["pos_cotangent"], np.repeat(rows[:, None] * 2, 3, 1).astype(np.float32))
        assert np.array_equal(d["vel_cotangent"], np.repeat(rows[:, None] * 3, 3, 1).astype(np.float32))
        assert np.array_equal(d["scalar_cotangents"], np.arange(2 * K + 1, dtype=np.float64))


def _bench(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_same_outputs(gpu, tmp_path):
    """A plain run: the headline keys, `steps` timed steps, none of the --full records; two runs dump the same outputs."""
    args = ["--gpus", "1", "--mesh", "64", "--steps", "13", "--warmup", "2", "--n-steps", "5"]
    lines = [_bench(args + ["--dump-outputs", str(tmp_path / d)]) for d in ("a", "b")]
    for line in lines:
        assert all(k in line for k in HEADLINE) and line["steps"] == 13 and line["value"] > 0
        assert abs(line["ms_per_step"] * line["value"] - 1e3) < 1e3 * 2e-2       # both rounded to 3 decimals
        assert not any(k in line for k in ("stages", "roofline", "force_cycle", "fwd_adj_step", "mesh_256", "cpu_baseline"))
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["final_disp.npy", "final_vel.npy", "pos_cotangent.npy", "scalar_cotangents.npy", "vel_cotangent.npy"]
    for f in names:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.shape == b.shape and np.all(np.isfinite(a)) and np.abs(a).max() > 0
        assert np.allclose(a, b, rtol=1e-6, atol=1e-6 * np.abs(a).max()), f


@pytest.mark.gpu
def test_full_run_keeps_the_secondary_records(gpu):
    args = ["--gpus", "1", "--mesh", "64", "--steps", "3", "--warmup", "1", "--n-steps", "3", "--full", "--no-cpu-baseline",
            "--cpu-mesh", "128"]
    line = _bench(args)
    assert all(k in line for k in HEADLINE) and line["steps"] == 3
    assert line["stages"] and line["roofline"]["kernel"] in line["stages"] and line["fwd_adj_step"]["ms_events"] > 0
    assert line["force_cycle"]["pm_forces_ms"] > 0 and line["mesh_128"]["value"] > 0
