"""Gains fitted smooth in time and frequency, host side: the DPSS time basis, the arguments, and the NumPy restatement of the
joint fit that the GPU tests (tests/test_gpu_gain_time_basis.py) are measured against.

Parameterisation: T times of Na antennas are ONE fit (antenna ``a`` at time ``t`` is row ``t * Na + a``, the layout of
``distributed.batch_time_slices(per_slice=False)``) and ``g = g0 + einsum("tl,alk,fk->taf", Bt, y, Bf)`` with ``Bt`` real
``[T, L]``, ``Bf`` real ``[F, K]`` and ``y`` (complex ``[Na, L, K]``, zero at the start) the optimizer's variables; chain rule: the
transposed einsum of the per-channel gain gradient.  ``gamma2_fit`` below is that, built from the oracle's public pieces with the
oracle's loop semantics, like ``gamma_fit`` in tests/test_gain_basis_host.py.  With ``Bt = I`` it must BE ``gamma_fit`` on the
batched problem, and with ``Bf = I`` as well the oracle's per-channel fit: the anchors that keep the yardstick honest."""
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from calamity_amd import calibration, distributed, modeling, problem, synthetic  # noqa: E402
from oracle import ref_numpy as R  # noqa: E402
from test_gain_basis_host import gamma_fit, small_case  # noqa: E402


def gamma2_fit(Bt, Bf, g0_r, g0_i, fg_r, fg_i, ch, maxsteps, optimizer, tol=1e-14, use_min=False, freeze_model=False, reg=False, **opt_kwargs):
    """The joint time-and-frequency basis fit in NumPy (float64).  ``g0_*``: ``[T * Na, F]``.  Returns dict(loss, g_r, g_i, y_r, y_i
    (``[Na, L, K]``), fg_r, fg_i): the parameters after the last update or, with ``use_min``, those held right after the update of
    the lowest-loss step."""
    a0, a1 = R.ant_inds_from_corr_inds(ch["corr_inds"])
    Bt, Bf = np.asarray(Bt, dtype=np.float64), np.asarray(Bf, dtype=np.float64)
    g0_r, g0_i = np.array(g0_r, dtype=np.float64), np.array(g0_i, dtype=np.float64)
    T, F = Bt.shape[0], Bf.shape[0]
    na = g0_r.shape[0] // T
    assert g0_r.shape == (T * na, F)
    y_r = np.zeros((na, Bt.shape[1], Bf.shape[1]))
    y_i = np.zeros_like(y_r)
    fg_r = [np.array(a, dtype=np.float64) for a in fg_r]
    fg_i = [np.array(a, dtype=np.float64) for a in fg_i]
    priors = R.prior_sums(ch["sky_model_r"], ch["sky_model_i"], ch["wgts"]) if reg else (None, None)
    opt = R.OPTIMIZERS[optimizer](**opt_kwargs)

    def expand(y):
        return np.einsum("tl,alk,fk->taf", Bt, y, Bf).reshape(T * na, F)

    def project(gg):
        return np.einsum("tl,taf,fk->alk", Bt, gg.reshape(T, na, F), Bf)

    def step():
        loss, gg_r, gg_i, gf_r, gf_i = R.loss_and_grads(g0_r + expand(y_r), g0_i + expand(y_i), fg_r, fg_i, ch["fg_comps"], ch["data_r"],
                                                        ch["data_i"], ch["wgts"], a0, a1, *priors)
        grads = [(project(gg_r), y_r), (project(gg_i), y_i)]
        if not freeze_model:
            grads += list(zip(gf_r, fg_r)) + list(zip(gf_i, fg_i))
        opt.apply_gradients(grads)
        return loss

    def snapshot():
        return dict(y_r=y_r.copy(), y_i=y_i.copy(), fg_r=[a.copy() for a in fg_r], fg_i=[a.copy() for a in fg_i])

    step()  # the unrecorded step
    losses, min_loss, best = [], 9e99, None
    for k in range(maxsteps):
        losses.append(step())
        if use_min and losses[-1] < min_loss:
            min_loss, best = losses[-1], snapshot()
        if k >= 1 and abs(losses[-1] - losses[-2]) < tol:
            break
    out = best if use_min else snapshot()
    out.update(loss=np.asarray(losses), g_r=g0_r + expand(out["y_r"]), g_i=g0_i + expand(out["y_i"]))
    return out


def joint_case(ntimes=3, nants=7, nfreqs=40, with_sky=False, perturb=True, seed=30):
    """``ntimes`` slices of one array as ONE fit: (joint FitProblem, start, chunks, fg_r, fg_i)."""
    cache, parts = {}, []
    for t in range(ntimes):
        p, _, start = synthetic.make_problem(nants, nfreqs, f0=150e6, df=400e3, seed=seed, data_seed=seed + 1 + t, with_sky=with_sky,
                                             operator_cache=cache)
        parts.append((p, start))
    big, start = distributed.batch_time_slices(parts, per_slice=False)
    if perturb:
        rng = np.random.default_rng(seed + 17)
        start["g_r"] = 1.0 + 0.05 * rng.standard_normal((big.nants, big.nfreqs))
        start["g_i"] = 0.05 * rng.standard_normal((big.nants, big.nfreqs))
    ch = problem.chunks_from_problem(big)
    fg_r = problem.coeffs_to_chunks(big, start["c_r"], np.float64)
    fg_i = problem.coeffs_to_chunks(big, start["c_i"], np.float64)
    return big, start, ch, fg_r, fg_i


TIMES_60 = 2458101.25 + np.arange(60) * 10.7 / 86400.0


# ---- 1. the time basis ----------------------------------------------------------------------------------------------------
def test_gain_time_dpss_basis():
    counts = []
    for scale in (600.0, 1800.0):
        Bt = modeling.gain_time_dpss_basis(TIMES_60, scale)
        x = (TIMES_60 - TIMES_60[0]) * 86400.0
        amat, nterms = modeling.dpss_operator(x, [0.0], [1.0 / scale], [1e-10])
        assert Bt.dtype == np.float64 and not np.iscomplexobj(Bt)
        assert Bt.shape == (60, nterms[0]) == amat.shape
        assert np.abs(Bt.T @ Bt - np.eye(Bt.shape[1])).max() <= 1e-10
        assert np.array_equal(Bt, amat.real) and np.abs(amat.imag).max() == 0.0
        counts.append(Bt.shape[1])
    assert counts == [8, 5]
    assert modeling.gain_time_dpss_basis(TIMES_60[:8], 400.0).shape == (8, 4)  # the recovery tests' basis
    assert modeling.gain_time_dpss_basis(TIMES_60, 600.0, eigenval_cutoff=1e-3).shape[1] < 8
    # what dpss_operator cannot give: one time, two times, a scale far beyond the span
    assert np.array_equal(modeling.gain_time_dpss_basis(TIMES_60[:1], 600.0), [[1.0]])
    np.testing.assert_allclose(modeling.gain_time_dpss_basis(TIMES_60[:2], 600.0), np.full((2, 1), 1.0 / np.sqrt(2.0)), rtol=1e-15)
    far = modeling.gain_time_dpss_basis(TIMES_60[:5], 1e12)
    assert far.shape == (5, 1) and np.abs(np.abs(far) - 1.0 / np.sqrt(5.0)).max() <= 1e-6 and abs(far.T @ far - 1.0) <= 1e-10
    for bad_scale in (0.0, -3.0, np.nan):
        with pytest.raises(ValueError):
            modeling.gain_time_dpss_basis(TIMES_60, bad_scale)
    uneven = TIMES_60.copy()
    uneven[7] += 3.0 / 86400.0
    with pytest.raises(ValueError, match="uniform"):
        modeling.gain_time_dpss_basis(uneven, 600.0)
    with pytest.raises(ValueError, match="uniform"):
        modeling.gain_time_dpss_basis(TIMES_60[::-1], 600.0)


# ---- 2. the restatement and its anchors -----------------------------------------------------------------------------------
def close(a, b, rtol=1e-12):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) <= rtol * max(np.linalg.norm(np.asarray(b)), 1e-300)


@pytest.mark.parametrize("optimizer", ["Adam", "Adamax"])
def test_identity_time_basis_restates_the_frequency_basis_fit(optimizer):
    big, start, ch, fg_r, fg_i = joint_case(ntimes=3, with_sky=True)
    Bf = np.array(modeling.gain_dpss_basis(150e6 + 400e3 * np.arange(big.nfreqs), 100.0))
    na = big.nants // 3
    for reg in (False, True):
        ref = gamma_fit(Bf, start["g_r"], start["g_i"], fg_r, fg_i, ch, 20, optimizer, reg=reg, learning_rate=1e-2)
        out = gamma2_fit(np.eye(3), Bf, start["g_r"], start["g_i"], fg_r, fg_i, ch, 20, optimizer, reg=reg, learning_rate=1e-2)
        assert len(out["loss"]) == 20
        np.testing.assert_allclose(out["loss"], ref["loss"], rtol=1e-12)
        assert close(out["g_r"], ref["g_r"]) and close(out["g_i"], ref["g_i"])
        # y[a, t, k] of the joint fit with Bt = I is y[t * Na + a, k] of the batched one
        assert close(out["y_r"].transpose(1, 0, 2).reshape(3 * na, -1), ref["y_r"])
        for a, b in zip(out["fg_r"] + out["fg_i"], ref["fg_r"] + ref["fg_i"]):
            assert close(a, b)


def test_one_time_restates_the_frequency_basis_fit():
    p, start, ch, fg_r, fg_i = small_case()
    Bf = np.array(modeling.gain_dpss_basis(150e6 + 400e3 * np.arange(p.nfreqs), 100.0))
    ref = gamma_fit(Bf, start["g_r"], start["g_i"], fg_r, fg_i, ch, 20, "Adam", learning_rate=1e-2)
    out = gamma2_fit(np.ones((1, 1)), Bf, start["g_r"], start["g_i"], fg_r, fg_i, ch, 20, "Adam", learning_rate=1e-2)
    np.testing.assert_allclose(out["loss"], ref["loss"], rtol=1e-12)
    assert close(out["g_r"], ref["g_r"]) and close(out["g_i"], ref["g_i"]) and close(out["y_r"][:, 0], ref["y_r"])


@pytest.mark.parametrize("optimizer", ["Adam", "Adamax"])
def test_identity_bases_restate_the_oracle(optimizer):
    big, start, ch, fg_r, fg_i = joint_case(ntimes=2)
    ref = R.fit_gains_and_foregrounds(start["g_r"], start["g_i"], fg_r, fg_i, ch["data_r"], ch["data_i"], ch["wgts"], ch["fg_comps"],
                                      ch["corr_inds"], maxsteps=20, optimizer=optimizer, learning_rate=1e-2)
    out = gamma2_fit(np.eye(2), np.eye(big.nfreqs), start["g_r"], start["g_i"], fg_r, fg_i, ch, 20, optimizer, learning_rate=1e-2)
    np.testing.assert_allclose(out["loss"], np.asarray(ref[4]["loss"], dtype=np.float64), rtol=1e-12)
    assert close(out["g_r"], ref[0]) and close(out["g_i"], ref[1])
    for a, b in zip(out["fg_r"] + out["fg_i"], list(ref[2]) + list(ref[3])):
        assert close(a, b)


# ---- 3. the recovery claim ------------------------------------------------------------------------------------------------
def recovery_case(noise=0.05, ntimes=8, nants=7, nfreqs=64, sigma=0.05):
    """8 times of 10.7 s of 7 antennas x 64 channels whose true gains are ``1 + Bt (x) Bf y_true`` (Bf: the 100-ns basis, 12 vectors;
    Bt: the 400-s basis, 4 vectors; y_true of sigma 0.05), noise 0.05 of the data's rms, unity start, the true foreground
    coefficients held fixed.  Returns dict(big, start, ch, fg_r, fg_i, Bt, Bf, prod): ``prod`` the true gain products
    ``g_i conj(g_j)`` of every baseline of the joint problem."""
    cache, parts, truths = {}, [], []
    for t in range(ntimes):
        p, truth, start = synthetic.make_problem(nants, nfreqs, f0=150e6, df=400e3, seed=11, data_seed=100 + t, gain_sigma=0.0, noise_frac=0.0,
                                                 operator_cache=cache)
        parts.append((p, start))
        truths.append(truth)
    Bf = np.array(modeling.gain_dpss_basis(150e6 + 400e3 * np.arange(nfreqs), 100.0))
    Bt = modeling.gain_time_dpss_basis(TIMES_60[:ntimes], 400.0)
    assert Bf.shape == (nfreqs, 12) and Bt.shape == (ntimes, 4)
    rng = np.random.default_rng(5)
    y_true = sigma * (rng.standard_normal((nants, Bt.shape[1], Bf.shape[1])) + 1j * rng.standard_normal((nants, Bt.shape[1], Bf.shape[1])))
    g_true = 1.0 + np.einsum("tl,alk,fk->taf", Bt, y_true, Bf)
    for t, (p, start) in enumerate(parts):
        d = (p.data_r + 1j * p.data_i) * g_true[t][p.bl_ant0] * np.conj(g_true[t][p.bl_ant1])
        d = d + noise * (rng.standard_normal(d.shape) + 1j * rng.standard_normal(d.shape)) / np.sqrt(2.0)  # (the data have unit rms)
        p.data_r, p.data_i = np.ascontiguousarray(d.real), np.ascontiguousarray(d.imag)
        start["c_r"], start["c_i"] = np.ascontiguousarray(truths[t]["c"].real), np.ascontiguousarray(truths[t]["c"].imag)
    big, start = distributed.batch_time_slices(parts, per_slice=False)
    ch = problem.chunks_from_problem(big)
    fg_r = problem.coeffs_to_chunks(big, start["c_r"], np.float64)
    fg_i = problem.coeffs_to_chunks(big, start["c_i"], np.float64)
    g_flat = g_true.reshape(ntimes * nants, nfreqs)
    return dict(big=big, start=start, ch=ch, fg_r=fg_r, fg_i=fg_i, Bt=Bt, Bf=Bf, prod=g_flat[big.bl_ant0] * np.conj(g_flat[big.bl_ant1]))


def product_error(case, g):
    """The gauge-free error of fitted gains: that of the products ``g_i conj(g_j)`` over the baselines, relative to the size of what
    the fit had to find (the true products minus those of the unity start)."""
    big = case["big"]
    return np.linalg.norm(g[big.bl_ant0] * np.conj(g[big.bl_ant1]) - case["prod"]) / np.linalg.norm(case["prod"] - 1.0)


def restated_recovery(case, steps=300):
    """(error of the per-time frequency-basis fit, error of the joint fit) of the restatement, Adam at 1e-2."""
    big, start = case["big"], case["start"]
    errs = []
    for Bt in (np.eye(case["Bt"].shape[0]), case["Bt"]):
        out = gamma2_fit(Bt, case["Bf"], start["g_r"], start["g_i"], case["fg_r"], case["fg_i"], case["ch"], steps, "Adam", tol=0.0,
                         freeze_model=True, learning_rate=1e-2)
        errs.append(product_error(case, out["g_r"] + 1j * out["g_i"]))
    return errs


def test_joint_fit_recovers_smooth_gains_better():
    per_time, joint = restated_recovery(recovery_case())
    print(f"gain-product error: per-time {per_time:.3f}, joint {joint:.3f}, ratio {joint / per_time:.3f}")
    assert joint <= 0.8 * per_time


# ---- 4. arguments -------------------------------------------------------------------------------------------------------
def test_argparser_and_argument_checks(monkeypatch):
    monkeypatch.setattr(sys, "argv", [sys.argv[0], "--input_data_files", "input.uvh5"])
    assert calibration.dpss_fit_argparser().parse_args().gain_time_scale is None
    monkeypatch.setattr(sys, "argv", [sys.argv[0], "--input_data_files", "input.uvh5", "--gain_time_scale", "600"])
    args = calibration.dpss_fit_argparser().parse_args()
    assert args.gain_time_scale == 600.0 and isinstance(args.gain_time_scale, float)
    params = inspect.signature(calibration.calibrate_and_model_tensor).parameters
    assert params["gain_time_basis"].default is None and params["gain_time_scale"].default is None
    # both given: refused before anything is touched (no device, not even a look at the data)
    with pytest.raises(ValueError, match="not both"):
        calibration.calibrate_and_model_tensor(None, {}, gain_time_basis=np.eye(4), gain_time_scale=600.0)
    for kw in (dict(init_guesses_from_previous_time_step=True), dict(batch_slices=False), dict(parallel_fits=2), dict(devices=[0, 1]), dict(devices="all"),
               dict(device_split="groups"), dict(device_split="slices")):
        with pytest.raises(ValueError, match="time basis"):
            calibration.calibrate_and_model_tensor(None, {}, gain_time_scale=600.0, **kw)
        with pytest.raises(ValueError, match="time basis"):
            calibration.calibrate_and_model_tensor(None, {}, gain_time_basis=np.eye(3), **kw)
    uvd, _, _ = synthetic.make_uvdata(nants=4, nfreqs=32, ntimes=3, seed=0)
    for bad, what in ((np.eye(4), "shape"), (np.ones(3), "shape"), (np.ones((3, 4)), "shape"), (np.eye(3) * 1j, "real"),
                      (np.full((3, 2), np.inf), "non-finite")):
        with pytest.raises(ValueError, match=what):
            calibration.calibrate_and_model_tensor(uvd, {}, gain_time_basis=bad)
    with pytest.raises(ValueError, match="positive"):
        calibration.calibrate_and_model_tensor(uvd, {}, gain_time_scale=-1.0)
    # the three times are one fit: a batch of two cannot hold them (a batch of three or more can)
    with pytest.raises(ValueError, match="batch_slices=2"):
        calibration.calibrate_and_model_tensor(uvd, {}, gain_time_basis=np.eye(3)[:, :2], batch_slices=2)
    # the frequency basis is checked as before when both axes are given
    with pytest.raises(ValueError, match="shape"):
        calibration.calibrate_and_model_tensor(uvd, {}, gain_basis=np.eye(31), gain_time_scale=600.0)
    # the solver method refuses on the host what it can: complex, wrong rank (no device: the checks come before the library call)
    from calamity_amd.solver import HipFitSolver

    s = HipFitSolver.__new__(HipFitSolver)
    s.dtype = np.dtype(np.float64)
    for bad in (np.eye(3) * 1j, np.ones(3), np.ones((0, 0))):
        with pytest.raises(ValueError):
            HipFitSolver.set_gain_time_basis(s, bad)
