"""cal_solver_robust_weights across a process boundary: two ranks on one GPU, each with its share of the fitting groups
(distributed.partition_groups), under cal_solver_set_exchange_hook over gloo between two fresh child processes
(tests/_robust_rank.py), in the manner of tests/test_gpu_fit_quality_ranks.py.  fp64, general kernels, 7 antennas x 200 channels.
The scale is per baseline row, so the call exchanges nothing -- the hook's call log does not grow during it -- and every rank's rows
equal the un-sharded solver's rows bit for bit."""
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
    outs = [str(tmp_path / f"robust_rank{r}.npz") for r in range(2)]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_robust_rank.py"), "--rank", str(r), "--port", str(port),
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


def test_two_ranks_reweight_their_rows_without_an_exchange(tmp_path):
    import _robust_rank as X
    from calamity_amd import distributed as D

    p, params = X.build_case()
    assert (p.nants, p.nfreqs) == (7, 200)
    ref = X.reweight(p, params)
    assert ref["ndown_bl"].sum() > 0 and np.any(ref["w"] < ref["w0"])
    ranks = run_two_ranks(tmp_path)
    shares = D.partition_groups(p.grp_nvec, p.grp_basis, np.diff(p.grp_bl_start), 2)
    for r in range(2):
        rows = np.concatenate([np.arange(p.grp_bl_start[g], p.grp_bl_start[g + 1]) for g in shares[r]])
        assert 0 < len(rows) < p.nbls
        for k in ("w", "w0", "scale_bl", "ndown_bl"):
            np.testing.assert_array_equal(ranks[r][k], ref[k][rows], err_msg=f"rank {r} {k}")
        # the set-up agreement came before; the call itself added nothing to the log
        assert int(ranks[r]["ncalls_before"]) == int(ranks[r]["ncalls_after"]) == 1, (r, ranks[r]["ncalls_before"], ranks[r]["ncalls_after"])
