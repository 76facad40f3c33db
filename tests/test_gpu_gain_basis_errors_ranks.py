"""cal_solver_gain_basis_errors across a process boundary: two ranks on one GPU, each with its share of the fitting groups, the exchange
through cal_solver_set_exchange_hook over gloo between two fresh child processes (tests/_gain_basis_errors_rank.py), in the manner of
tests/test_gpu_gain_time_solve_ranks.py and on its case: fp64, general kernels, 4 times of 5 antennas x 48 channels, the 100 ns DPSS basis
(K = 10) and the 30 s time basis (L = 3).  y is replicated and den is summed over the ranks, so both ranks compute the same planes: they
agree bit for bit, and with the unsharded solver's to the fp64 plane tolerance (the ranks add their partial sums of den in another
order).  Each call exchanges what its one antenna sweep does -- ONE sum of nants nfreqs doubles -- and nothing else."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_fit_quality import TOL, plane_err
from test_gpu_gain_time_solve_ranks import _free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def run_two_ranks(tmp_path):
    port = _free_port()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    outs = [str(tmp_path / f"errors_rank{r}.npz") for r in range(2)]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_gain_basis_errors_rank.py"), "--rank", str(r), "--port", str(port),
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


def test_two_ranks_compute_the_same_planes_from_one_exchange_per_call(tmp_path):
    import _gain_basis_errors_rank as X
    import _gain_time_solve_rank as case

    p, params = case.build_case()
    assert (p.nants, p.nfreqs) == (4 * 5, 48)
    ref = X.errors_of(p, params)
    ranks = run_two_ranks(tmp_path)
    shapes = {"freq": (20, 10), "both": (5, 3, 10), "time": (5, 3, 48)}
    for config in X.CONFIGS:
        assert ref[f"{config}_y_var"].shape == shapes[config] and np.all(ref[f"{config}_gain_var"] > 0)
        for k in ("gain_var", "y_var", "gain_dof", "nsolved", "nsingular"):
            key = f"{config}_{k}"
            np.testing.assert_array_equal(ranks[0][key], ranks[1][key], err_msg=key)
            err = plane_err(ranks[0][key], ref[key])
            print(f"{key}: two ranks against the single solver {err:.2e}")
            assert err <= TOL[np.dtype(np.float64)]["plane"], key
        for out in ranks:  # antenna_sweep's one all-reduce of the den plane
            assert out[f"{config}_sizes"].tolist() == [p.nants * p.nfreqs] and out[f"{config}_ops"].tolist() == [f"{np.dtype(np.float64).str} sum"]
