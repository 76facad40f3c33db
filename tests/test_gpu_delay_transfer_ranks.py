"""cal_solver_delay_transfer across a process boundary: two ranks on one GPU, each with its share of the fitting groups
(distributed.partition_groups), the exchange through cal_solver_set_exchange_hook over gloo between two fresh child processes
(tests/_delay_transfer_rank.py), in the manner of tests/test_gpu_delay_spectrum_ranks.py.  fp64, general kernels, 7 antennas x 64
channels.  absorbed_bin and the counts are summed over the ranks in ONE all-reduce of nbins ndelays + nbins doubles and come out
bit-identical on both, within 1e-10 of the unsharded solver; a group belongs to one rank, so the per-row outputs are the single
solver's rows to the bit."""
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
    outs = [str(tmp_path / f"dtransfer_rank{r}.npz") for r in range(2)]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_delay_transfer_rank.py"), "--rank", str(r), "--port", str(port),
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


def test_two_ranks_sum_the_bins_in_one_exchange(tmp_path):
    import _delay_transfer_rank as X
    from calamity_amd import distributed as D

    p, params, op, _, bins = X.build_case()
    assert (p.nants, p.nfreqs) == (7, 64)
    ref = X.transfer(p, params, op, bins)
    ranks = run_two_ranks(tmp_path)
    for k in ("absorbed_bin", "count_bin"):
        np.testing.assert_array_equal(ranks[0][k], ranks[1][k], err_msg=k)
        err = np.max(np.abs(ranks[0][k] - ref[k])) / np.max(np.abs(ref[k]))
        print(f"{k}: two ranks against the single solver {err:.2e}")
        assert err <= 1e-10, k
    np.testing.assert_array_equal(ranks[0]["count_bin"], ref["count_bin"])
    assert ref["count_bin"].sum() == p.nbls - 1  # one row is left out
    assert sum(int(out["nsolved"]) for out in ranks) == ref["nsolved"] == p.ngrps
    for r in range(2):
        rows = X.rows_of_rank(p, r, 2)
        assert 0 < len(rows) < p.nbls
        for k in ("absorbed_bl", "noise_bl"):
            np.testing.assert_array_equal(ranks[r][k], ref[k][rows], err_msg=f"rank {r} {k}")
    # what was exchanged: the set-up agreement (4 ints, min), then exactly one sum of the stated count of doubles
    want = D.exchange_spec(p.nants, p.nfreqs, delay_transfer=(X.NBINS, X.NDELAYS))["delay_transfer_f64"]
    assert want == X.NBINS * X.NDELAYS + X.NBINS
    for out in ranks:
        calls = list(zip([str(d) for d in out["call_dtypes"]], [int(n) for n in out["call_sizes"]], [str(x) for x in out["call_ops"]]))
        assert calls == [(np.dtype(np.int32).str, 4, "min"), (np.dtype(np.float64).str, want, "sum")], calls
