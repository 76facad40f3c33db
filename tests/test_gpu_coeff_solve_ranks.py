"""cal_solver_solve_coeffs across a process boundary: two ranks on one GPU, each with its share of the fitting groups
(distributed.partition_groups), under cal_solver_set_exchange_hook over gloo between two fresh child processes
(tests/_coeff_solve_rank.py), in the manner of tests/test_gpu_gain_solve_ranks.py.  fp64, general kernels, 7 antennas x 64
channels.  Every fitting group belongs to one rank and the gains are replicated, so the call exchanges NOTHING: each rank's
coefficients equal the NumPy restatement on its own groups (fp64 plane tolerance 1e-10), and an Adam fit continued from there
matches the unsharded solver's to the tolerances of tests/test_gpu_exchange_hook.py (1e-10)."""
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
    outs = [str(tmp_path / f"coeffs_rank{r}.npz") for r in range(2)]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_coeff_solve_rank.py"), "--rank", str(r), "--port", str(port),
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


def relnorm(a, b):
    return np.linalg.norm(np.asarray(a, dtype=np.float64) - b) / max(np.linalg.norm(b), 1e-300)


def test_two_ranks_solve_their_own_groups_without_an_exchange(tmp_path):
    import _coeff_solve_rank as X
    from calamity_amd import distributed as D
    from test_gpu_coeff_solve import COND_MAX, restated
    from test_gpu_fit_quality import plane_err

    p, params = X.build_case()
    assert (p.nants, p.nfreqs) == (7, 64)
    want, _, conds, singular = restated(p, params, np.float64)
    assert max(conds) <= COND_MAX and not singular
    ref = X.solved(p, params)
    assert ref["nsolved"] == p.ngrps and not np.array_equal(ref["c_r"], params["c_r"])
    ranks = run_two_ranks(tmp_path)
    shares = D.partition_groups(p.grp_nvec, p.grp_basis, np.diff(p.grp_bl_start), 2)
    coff = p.grp_coff
    for r, out in enumerate(ranks):
        idx = np.concatenate([np.arange(coff[g], coff[g + 1]) for g in shares[r]])
        errs = (plane_err(out["c_r"], want.real[idx]), plane_err(out["c_i"], want.imag[idx]))
        print(f"rank {r}: {len(shares[r])} groups, against the restatement c_r {errs[0]:.2e}  c_i {errs[1]:.2e}")
        assert max(errs) <= 1e-10
        assert int(out["nsolved"]) == len(shares[r]) and int(out["nsingular"]) == 0
        assert int(out["exchanges_in_solve"]) == 0  # the hook is never invoked by the call
        # the fit continued on both ranks against the fit continued on one solver
        assert len(out["losses"]) == X.NSTEPS
        np.testing.assert_allclose(out["losses"], ref["losses"], rtol=1e-10)
        assert relnorm(out["fit_g_r"], ref["fit_g_r"]) <= 1e-10 and relnorm(out["fit_g_i"], ref["fit_g_i"]) <= 1e-10, r
        assert relnorm(out["fit_c_r"], ref["fit_c_r"][idx]) <= 1e-10 and relnorm(out["fit_c_i"], ref["fit_c_i"][idx]) <= 1e-10, r
    np.testing.assert_array_equal(ranks[0]["fit_g_r"], ranks[1]["fit_g_r"])
    np.testing.assert_array_equal(ranks[0]["losses"], ranks[1]["losses"])
