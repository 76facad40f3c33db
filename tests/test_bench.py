"""bench.py's plain run and --dump-outputs: the files hold what the timed steps computed, within the size cap, and a sample
of an output too large for the cap is the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_whole_below_the_cap_and_a_fixed_sample_above(tmp_path, monkeypatch):
    import bench

    rng = np.random.default_rng(3)
    arrays = {"losses": rng.random(7), "g_r": rng.random((5, 16)).astype(np.float32), "c_r": rng.random(4000)}
    bench.dump_outputs(str(tmp_path / "whole"), arrays)
    for k, a in arrays.items():
        b = np.load(tmp_path / "whole" / f"{k}.npy")
        assert b.dtype == a.dtype and np.array_equal(a, b)

    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 12000)
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), arrays)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["c_r.npy", "g_r.npy", "losses.npy"]
    assert sum(np.load(tmp_path / "a" / f).nbytes for f in files) <= 12000
    assert np.array_equal(np.load(tmp_path / "a" / "losses.npy"), arrays["losses"])
    assert np.array_equal(np.load(tmp_path / "a" / "g_r.npy"), arrays["g_r"])
    c = np.load(tmp_path / "a" / "c_r.npy")
    assert c.size == 12000 // 3 // 8 and np.array_equal(c, np.load(tmp_path / "b" / "c_r.npy"))
    where = {v: i for i, v in enumerate(arrays["c_r"])}  # (distinct random values: an element's value names its position)
    assert np.all(np.diff([where[v] for v in c]) > 0)

    with pytest.raises(TypeError):
        bench.dump_outputs(str(tmp_path / "int"), {"n": np.arange(3)})


@pytest.mark.gpu
def test_plain_run_dumps_what_its_timed_steps_computed(tmp_path):
    """A plain run reports the headline alone, and its dump equals the losses of its line and the parameters of a solver
    stepped warmup + steps times on the same seeded problem (bit for bit: every launch form computes the same numbers)."""
    steps, warmup, max_bls = 5, 2, 3000
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
           "--max-bls", str(max_bls), "--dump-outputs", str(tmp_path)]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    res = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + "\n" + res.stderr[-4000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == steps and out["warmup"] == warmup and out["unit"] == "steps/s" and out["dtype"] == "f32"
    assert out["ms_per_step"] == pytest.approx(1e3 / out["value"])
    assert "cpu_baseline" not in out and out["extra"]["shared_layout"] is None and out["extra"]["chi2_evals_per_s"] is None

    losses = np.load(tmp_path / "losses.npy")
    assert losses.dtype == np.float64 and np.array_equal(losses, np.asarray(out["extra"]["losses"]))

    from calamity_amd import synthetic
    from calamity_amd.solver import HipFitSolver

    prob, _, start = synthetic.make_config("hera350", max_bls=max_bls)
    s = HipFitSolver(dtype=np.float32)
    s.set_problem(prob, layout="stream")
    s.set_params(start["g_r"], start["g_i"], start["c_r"], start["c_i"])
    s.set_optimizer("Adam", learning_rate=1e-2)
    s.run(warmup, record=False, tol=0.0)
    ref_losses = s.run(steps, record=True, tol=0.0)[0]
    params = s.get_params()
    s.close()
    assert np.array_equal(losses, ref_losses)
    for name, ref in zip(("g_r", "g_i", "c_r", "c_i"), params):
        got = np.load(tmp_path / f"{name}.npy")
        assert got.dtype == np.float32 and np.array_equal(got, ref), name
