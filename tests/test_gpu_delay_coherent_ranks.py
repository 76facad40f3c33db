"""cal_solver_delay_coherent_spectrum across a process boundary: two ranks on one GPU, each with its share of the fitting groups and the
ragged groups of its own rows (batched.split_member_groups), the exchange through cal_solver_set_exchange_hook over gloo between two fresh
child processes (tests/_delay_coherent_rank.py), as for the fringe call.  fp64, general kernels, 7 antennas x 64 channels, groups of two
sets (three members and one), two rates.  power_bin | count_bin are summed over the ranks in ONE all-reduce of
nwhat nbins nrates ndelays + nbins doubles and come out bit-identical on both; norm_grp stays each rank's own groups."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def run_two_ranks(tmp_path):
    import subprocess

    from test_gpu_delay_spectrum_ranks import _free_port

    port = _free_port()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    outs = [str(tmp_path / f"dcoherent_rank{r}.npz") for r in range(2)]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_delay_coherent_rank.py"), "--rank", str(r), "--port", str(port),
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
    import _delay_coherent_rank as X
    from calamity_amd import distributed as D

    case = X.build_case()
    p, params, op, norm_f, set_ptr = case[:5]
    ngroups = (len(set_ptr) - 1) // X.NTIMES
    assert (p.nants, p.nfreqs) == (7, 64) and ngroups == p.nbls and case[8].shape == (X.NTIMES, X.NRATES)
    ref = X.coherent(*case)
    ranks = run_two_ranks(tmp_path)
    for k in ("data", "model", "resid", "count_bin"):
        np.testing.assert_array_equal(ranks[0][k], ranks[1][k], err_msg=k)
        assert ref[k].shape == ((X.NBINS,) if k == "count_bin" else (X.NBINS, X.NRATES, X.NDELAYS))
        # the unsharded solver adds a bin's groups in ascending order, the ranks add their own and the exchange adds the two sums: the same
        # non-negative terms in another order, a few roundings of double on the sum
        err = np.max(np.abs(ranks[0][k] - ref[k])) / np.max(np.abs(ref[k]))
        print(f"{k}: two ranks against the single solver {err:.2e}")
        assert err <= 1e-15, k
    np.testing.assert_array_equal(ranks[0]["count_bin"], ref["count_bin"])
    assert 0 < ref["count_bin"].sum() <= ngroups - 1  # one group is left out (and those with an empty common mask)
    seen = np.concatenate([ranks[r]["mine"] for r in range(2)])
    assert sorted(seen) == list(range(ngroups)) and all(0 < len(ranks[r]["mine"]) < ngroups for r in range(2))
    for r in range(2):
        np.testing.assert_array_equal(ranks[r]["norm_grp"], ref["norm_grp"][ranks[r]["mine"]], err_msg=f"rank {r} norm_grp")
    # what was exchanged: the set-up agreement (4 ints, min), then exactly one sum of the stated count of doubles
    want = D.exchange_spec(p.nants, p.nfreqs, delay_coherent=(3, X.NBINS, X.NRATES, X.NDELAYS))["delay_coherent_f64"]
    assert want == 3 * X.NBINS * X.NRATES * X.NDELAYS + X.NBINS
    for out in ranks:
        calls = list(zip([str(d) for d in out["call_dtypes"]], [int(n) for n in out["call_sizes"]], [str(x) for x in out["call_ops"]]))
        assert calls == [(np.dtype(np.int32).str, 4, "min"), (np.dtype(np.float64).str, want, "sum")], calls
