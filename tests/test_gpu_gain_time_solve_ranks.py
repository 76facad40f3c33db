"""cal_solver_solve_gain_time_coeffs across a process boundary: two ranks on one GPU, each with its share of the fitting groups
(distributed.partition_groups), the exchange through cal_solver_set_exchange_hook over gloo between two fresh child processes
(tests/_gain_time_solve_rank.py), in the manner of tests/test_gpu_gain_basis_solve_ranks.py.  fp64, general kernels, 4 times of 5 antennas
x 48 channels as one fit, the 100 ns DPSS basis (K = 10) and the 30 s time basis (L = 3), three sweeps.  Every sweep sums num_r | num_i |
den over the ranks in ONE all-reduce of 3 nants nfreqs doubles (nants = T Na rows) and needs no other collective; y is replicated, so
both ranks then compute the same N_a and the same update: their gains and y agree bit for bit, and with the unsharded solver's to the
fp64 plane tolerance (1e-10 of the plane's largest element: the ranks add their partial sums in another order)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def run_two_ranks(tmp_path):
    port = _free_port()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    outs = [str(tmp_path / f"gains_rank{r}.npz") for r in range(2)]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_gain_time_solve_rank.py"), "--rank", str(r), "--port", str(port),
                               "--out", outs[r]], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(2)]
    logs = []
    try:
        for pr in procs:
            logs.append(pr.communicate(timeout=300)[0])
    finally:  # (whatever ends this, no rank is left behind holding the GPU)
        for q in procs:
            if q.poll() is None:
                q.kill()
    for r, pr in enumerate(procs):
        assert pr.returncode == 0, f"rank {r} failed:\n{logs[r][-4000:]}"
    return [np.load(o) for o in outs]


def test_two_ranks_sum_the_three_planes_once_per_sweep(tmp_path):
    import _gain_time_solve_rank as X
    from calamity_amd import distributed as D

    p, params = X.build_case()
    assert (p.nants, p.nfreqs) == (4 * 5, 48) and X.time_basis().shape == (4, 3)
    ref = X.solved(p, params)
    assert not np.array_equal(ref["g_r"], params["g_r"])
    ranks = run_two_ranks(tmp_path)
    for k in ("g_r", "g_i", "y_r", "y_i"):
        np.testing.assert_array_equal(ranks[0][k], ranks[1][k], err_msg=k)
        err = np.max(np.abs(ranks[0][k] - ref[k])) / np.max(np.abs(ref[k]))
        print(f"{k}: two ranks against the single solver {err:.2e}")
        assert err <= 1e-10, k
    # what the call exchanged: exactly one sum of the stated count of doubles per sweep and nothing else
    want = D.exchange_spec(p.nants, p.nfreqs)["gain_solve_f64"]
    assert want == 3 * 20 * 48
    for out in ranks:
        calls = list(zip([str(d) for d in out["call_dtypes"]], [int(n) for n in out["call_sizes"]], [str(x) for x in out["call_ops"]]))
        assert calls[int(out["calls_before"]):] == [(np.dtype(np.float64).str, want, "sum")] * X.NSWEEPS, calls
        assert (int(out["nsolved"]), int(out["nsingular"])) == (5, 0)  # antennas, not rows
    assert ref["y_r"].shape == (5, 3, 10) and (ref["nsolved"], ref["nsingular"]) == (5, 0)
