"""The multi-rank algebra on REAL kernels with two ranks on one GPU.

RCCL refuses two ranks on one device, so the exchange goes through cal_solver_set_exchange_hook: wherever the library would
call ncclAllReduce it hands the same buffers and counts to a callback, here a gloo all-reduce between two fresh child
processes that share the GPU (tests/_exchange_rank.py).  Baselines are sharded by whole fitting groups
(calamity_amd/distributed.py); gains are replicated.  Checked against the single-solver fit of the whole problem, fp64,
1e-10: recorded losses, the replicated gains (bit-identical on both ranks), every rank's coefficients -- for the general
and the dense (matrix-core) kernels, without and with the "sum" regulariser (three-part gain payload / the dense path's
extra scalar exchange); a shard that is too small for the dense kernels drags BOTH ranks to the general ones; a tolerance
stop lands on the same step on both; with a gain basis in frequency, and in time and frequency, the ranks exchange the
projected planes and hold identical coefficients ``y``.  (The reference is single-device: calibration.py:1796-1804.)"""
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


def run_two_ranks(case, tmp_path):
    port = _free_port()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    outs = [str(tmp_path / f"{case}_rank{r}.npz") for r in range(2)]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_exchange_rank.py"), "--case", case, "--rank", str(r),
                               "--port", str(port), "--out", outs[r]], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(2)]
    logs = []
    try:
        for pr in procs:
            logs.append(pr.communicate(timeout=300)[0])
    finally:  # (whatever ends this -- a timeout here, pytest-timeout's alarm -- no rank is left behind holding the GPU)
        for q in procs:
            if q.poll() is None:
                q.kill()
    for r, pr in enumerate(procs):
        assert pr.returncode == 0, f"rank {r} failed:\n{logs[r][-4000:]}"
    return [np.load(o) for o in outs]


def relnorm(a, b):
    return np.linalg.norm(np.asarray(a, dtype=np.float64) - b) / max(np.linalg.norm(b), 1e-300)


def reference(case):
    import _exchange_rank as X

    p, start, groups, opts, run, reg = X.build_case(case)
    if case.startswith("fallback"):
        opts = dict(opts, kernel_path="general")
    ref = X.fit(p, start, opts, run, X.priors(p) if reg else None, bases=X.case_bases(case, p))
    return p, start, groups, ref


def shard_coeffs(p, ref, groups, rank):
    from calamity_amd import distributed as D

    if groups is None:
        nbl_g = np.diff(p.grp_bl_start)
        groups_r = D.partition_groups(p.grp_nvec, p.grp_basis, nbl_g, 2)[rank]
    else:
        groups_r = groups[rank]
    coff = p.grp_coff
    idx = np.concatenate([np.arange(coff[g], coff[g + 1]) for g in groups_r])
    return ref["c_r"][idx], ref["c_i"][idx]


@pytest.mark.parametrize("case", ["general_none", "general_sum", "dense_none", "dense_sum", "tolstop_none", "fallback_none", "fallback_sum"])
def test_two_ranks_on_one_gpu_equal_the_single_solver_fit(case, tmp_path):
    p, start, groups, ref = reference(case)
    ranks = run_two_ranks(case, tmp_path)
    want_path = "dense" if case.startswith("dense") else "general"
    assert ref["path"] == want_path
    nrec = len(ref["losses"])
    if case.startswith("tolstop"):
        assert ref["stopped"] and 5 < nrec < 400
    for r, out in enumerate(ranks):
        assert str(out["path"]) == want_path, (case, r)  # fallback: rank 0's share alone would have taken the dense kernels
        assert int(out["nupd"]) == ref["nupd"] and bool(out["stopped"]) == bool(ref["stopped"]) and len(out["losses"]) == nrec, (case, r)
        np.testing.assert_allclose(out["losses"], ref["losses"], rtol=1e-10)
        assert relnorm(out["g_r"], ref["g_r"]) <= 1e-10 and relnorm(out["g_i"], ref["g_i"]) <= 1e-10, (case, r)
        c_r, c_i = shard_coeffs(p, ref, groups, r)
        assert relnorm(out["c_r"], c_r) <= 1e-10 and relnorm(out["c_i"], c_i) <= 1e-10, (case, r)
    # replicated gains: both ranks applied the identical update to the identical all-reduced gradient
    np.testing.assert_array_equal(ranks[0]["g_r"], ranks[1]["g_r"])
    np.testing.assert_array_equal(ranks[0]["g_i"], ranks[1]["g_i"])
    np.testing.assert_array_equal(ranks[0]["losses"], ranks[1]["losses"])
    # what was exchanged: the set-up agreement (4 ints, min), then per step the gain-gradient parts and 4 double scalars
    from calamity_amd import distributed as D

    reg = case.endswith("_sum")
    spec = D.exchange_spec(p.nants, 128, reg_sum=reg and want_path == "general")
    sizes, ops = ranks[0]["call_sizes"], [str(o) for o in ranks[0]["call_ops"]]
    assert sizes[0] == 4 and ops[0] == "min" and all(o == "sum" for o in ops[1:])
    per_step = [spec["gain_grad_reals"], 4] if not (reg and want_path == "dense") else [4, spec["gain_grad_reals"], 4]
    body = list(sizes[1:])
    assert len(body) % len(per_step) == 0 and body == per_step * (len(body) // len(per_step)), (case, body[:8])


def padded_row(nfreqs):
    """fpad: a row of gains is padded to the next power of two up to 128 channels, to a multiple of 128 beyond."""
    return 1 << (nfreqs - 1).bit_length() if nfreqs <= 128 else (nfreqs + 127) // 128 * 128


@pytest.mark.parametrize("case", ["general_gbasis_sum", "general_tbasis_sum"])
def test_two_ranks_with_a_gain_basis_equal_the_single_solver_fit(case, tmp_path):
    """Both gain bases across a process boundary: each rank projects the gain gradient of its share on the basis (and, with a time
    basis, contracts it over the four times) BEFORE the exchange, which then carries the planes of y instead of the per-channel
    ones; both ranks apply the same update to the same summed planes and rebuild identical gains from identical y."""
    import _exchange_rank as X

    p, start, groups, ref = reference(case)
    Bf, Bt = X.case_bases(case, p)
    K = Bf.shape[1]
    kpad = (K + 7) // 8 * 8  # documented: include/calamity_hip.h
    if Bt is None:
        assert (p.nants, p.nfreqs) == (12, 128) and 1 < K < p.nfreqs // 2
        y_shape, with_basis = (p.nants, K), 2 * p.nants * kpad
    else:
        from test_gain_time_basis_host import TIMES_60

        assert np.array_equal(X.TBASIS_TIMES, TIMES_60[:4]) and (p.nants, p.nfreqs) == (4 * 7, 40) and 1 < Bt.shape[1] < 4
        y_shape, with_basis = (7, Bt.shape[1], K), 2 * 7 * Bt.shape[1] * kpad
    assert ref["path"] == "general" and ref["y_r"].shape == y_shape and np.any(ref["y_r"]) and np.any(ref["y_i"])
    ranks = run_two_ranks(case, tmp_path)
    nrec = len(ref["losses"])
    assert nrec == 12
    for r, out in enumerate(ranks):
        assert str(out["path"]) == "general" and int(out["nupd"]) == ref["nupd"] and not bool(out["stopped"]) and len(out["losses"]) == nrec, (case, r)
        c_r, c_i = shard_coeffs(p, ref, groups, r)
        print(f"{case} rank {r}: loss {np.max(np.abs(out['losses'] - ref['losses']) / ref['losses']):.2e}  g {relnorm(out['g_r'], ref['g_r']):.2e} "
              f"{relnorm(out['g_i'], ref['g_i']):.2e}  y {relnorm(out['y_r'], ref['y_r']):.2e} {relnorm(out['y_i'], ref['y_i']):.2e}  "
              f"c {relnorm(out['c_r'], c_r):.2e} {relnorm(out['c_i'], c_i):.2e}")
        np.testing.assert_allclose(out["losses"], ref["losses"], rtol=1e-10)
        assert relnorm(out["g_r"], ref["g_r"]) <= 1e-10 and relnorm(out["g_i"], ref["g_i"]) <= 1e-10, (case, r)
        assert out["y_r"].shape == y_shape and relnorm(out["y_r"], ref["y_r"]) <= 1e-10 and relnorm(out["y_i"], ref["y_i"]) <= 1e-10, (case, r)
        assert relnorm(out["c_r"], c_r) <= 1e-10 and relnorm(out["c_i"], c_i) <= 1e-10, (case, r)
    for k in ("g_r", "g_i", "y_r", "y_i", "losses"):  # replicated: the identical update of the identical all-reduced planes
        np.testing.assert_array_equal(ranks[0][k], ranks[1][k], err_msg=k)
    # what was exchanged: the set-up agreement (4 ints, min), then per step the projected gain-gradient planes and 4 double scalars
    # (the scalars once more in front where the step takes a loss pre-pass) -- the same calls on both ranks
    calls = [list(zip([str(d) for d in o["call_dtypes"]], [int(n) for n in o["call_sizes"]], [str(x) for x in o["call_ops"]])) for o in ranks]
    assert calls[0] == calls[1]
    assert calls[0][0] == (np.dtype(np.int32).str, 4, "min")
    f64 = np.dtype(np.float64).str
    planes = 3  # the "sum" regulariser on the general kernels: three parts, as exchange_spec(reg_sum=True) of the cases above
    grad_calls = [c for c in calls[0][1:] if c[1] > 4]
    assert grad_calls == [(f64, planes * with_basis, "sum")] * 13, (case, grad_calls[:3])  # (1 + 12 train steps)
    assert all(c == (f64, 4, "sum") for c in calls[0][1:] if c[1] <= 4)
    from calamity_amd import distributed as D

    without_basis = D.exchange_spec(p.nants, padded_row(p.nfreqs), reg_sum=True)["gain_grad_reals"]
    assert planes * with_basis < without_basis, (planes * with_basis, without_basis)


def test_two_rank_processes_with_a_wide_block_on_one_take_two_passes(tmp_path):
    """T = 4 time slices per rank (what a rank of ``bench.py --gpus N`` holds), STREAM layout, fp32, "sum" regulariser: rank 0's
    share holds a 230-vector block (its heads: a loss pre-pass), rank 1's not (alone it would take the one-pass form).  The two
    processes agree in set_problem on the two-pass step and issue the same exchanges; against the one-solver fit of all slices
    (fp32: losses 1e-4, parameters 1e-3), gains bit-identical on both ranks (tests/test_gpu_shard_agreement.py: case B)."""
    import _exchange_rank as X
    import _slice_cases as SC

    name, dtype = X.SLICE_CASES["slices_wide32_sum"]
    cd = SC.build(name, dtype)
    sub, rows, cidx = SC.rank_share(cd, 0, 1)
    ref = X.fit_slices(cd, sub, rows, cidx, dtype)
    ranks = run_two_ranks("slices_wide32_sum", tmp_path)
    for r, out in enumerate(ranks):
        np.testing.assert_allclose(out["losses"], ref["losses"], rtol=1e-4)
        assert out["losses"].shape == ref["losses"].shape and np.array_equal(out["nupd"], ref["nupd"]), r
        assert relnorm(out["g_r"], ref["g_r"]) <= 1e-3 and relnorm(out["g_i"], ref["g_i"]) <= 1e-3, r
        _, _, cidx_r = SC.rank_share(cd, r, 2)
        assert relnorm(out["c_r"], ref["c_r"][cidx_r]) <= 1e-3 and relnorm(out["c_i"], ref["c_i"][cidx_r]) <= 1e-3, r
    np.testing.assert_array_equal(ranks[0]["g_r"], ranks[1]["g_r"])
    np.testing.assert_array_equal(ranks[0]["g_i"], ranks[1]["g_i"])
    calls = [list(zip([str(d) for d in o["call_dtypes"]], [int(n) for n in o["call_sizes"]], [str(x) for x in o["call_ops"]])) for o in ranks]
    assert calls[0] == calls[1]
    assert calls[0][0] == (np.dtype(np.int32).str, 4, "min")
    step = SC.per_step("two_pass", cd["nt"], dtype)
    assert calls[0][1:] == step * 13, calls[0][1:4]  # (1 + 12 train steps)
