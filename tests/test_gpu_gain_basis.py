"""Gains fitted in a smooth frequency basis (cal_solver_set_gain_basis) on the GPU: ``g = g0 + B y``, ``y`` the optimizer's
variables, ``grad y = grad g @ B`` (gain_project_kernel), ``g`` rebuilt after every update (gain_expand_kernel).

Yardsticks: the CPU oracle (``oracle.ref_numpy``) for the projected gradient and, with ``B = I``, for the whole fit; the
NumPy restatement of the basis fit (``tests/test_gain_basis_host.py: gamma_fit``, which a CPU test pins to the oracle) for a
DPSS basis.  Tolerances are the project's (tests/test_gpu_parity.py): fp64 loss and gradients 1e-10,
trajectories 1e-8; fp32 loss 1e-5, gradients 1e-4 norm-wise, trajectories 1e-3."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from calamity_amd import _lib, cal_utils, calfits, calibration, distributed, modeling, problem, synthetic, uvcompat  # noqa: E402
from oracle import ref_numpy as R  # noqa: E402
from test_gain_basis_host import gamma_fit  # noqa: E402
from test_gpu_parity import TOL, make_case, make_solver, oracle_inputs, relnorm  # noqa: E402

pytestmark = pytest.mark.gpu


def freqs_of(p):
    return 150e6 + 400e3 * np.arange(p.nfreqs)


def dpss_basis(p, dly_ns=100.0):
    return np.array(modeling.gain_dpss_basis(freqs_of(p), dly_ns))


def cplx(a_r, a_i):
    return np.asarray(a_r, dtype=np.float64) + 1j * np.asarray(a_i, dtype=np.float64)


def out_of_span(B, d):
    """Norm of the part of the rows of d (complex [nants, F]) outside span(B)."""
    P = B @ np.linalg.pinv(B)
    return np.linalg.norm(d - d @ P.T)


# ---- 4. the projected gradient --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("layout", ["stream", "shared"])
@pytest.mark.parametrize("reg", [False, True])
@pytest.mark.parametrize("basis", ["dpss", "random"])
def test_projected_gradient(dtype, layout, reg, basis):
    p, start = make_case(seed=3, with_sky=reg)
    ch, fg_r, fg_i = oracle_inputs(p, start)
    a0, a1 = R.ant_inds_from_corr_inds(ch["corr_inds"])
    priors = R.prior_sums(ch["sky_model_r"], ch["sky_model_i"], ch["wgts"]) if reg else (None, None)
    loss, gg_r, gg_i, _, _ = R.loss_and_grads(start["g_r"], start["g_i"], fg_r, fg_i, ch["fg_comps"], ch["data_r"], ch["data_i"], ch["wgts"],
                                              a0, a1, *priors)
    B = dpss_basis(p) if basis == "dpss" else np.random.default_rng(1).standard_normal((p.nfreqs, 11))  # (not orthogonal, K not a multiple of 8)
    B = B.astype(dtype).astype(np.float64)  # the basis the device holds
    s = make_solver(p, start, dtype, layout, reg)
    s.set_gain_basis(B)
    tol = TOL[dtype]
    l2, gy_r, gy_i = s.eval_gain_coeff_grads()
    assert gy_r.shape == (p.nants, B.shape[1]) and gy_r.dtype == np.dtype(dtype)
    print(f"loss rel {abs(l2 - loss) / abs(loss):.2e}  grad y rel {relnorm(gy_r, gg_r @ B):.2e} {relnorm(gy_i, gg_i @ B):.2e}")
    assert abs(l2 - loss) <= tol["loss"] * abs(loss)
    assert relnorm(gy_r, gg_r @ B) <= tol["grad"]
    assert relnorm(gy_i, gg_i @ B) <= tol["grad"]
    # the per-channel entry point keeps returning the per-channel gradient; nothing has moved
    _, hg_r, hg_i, _, _ = s.eval_grads()
    assert relnorm(hg_r, gg_r) <= tol["grad"] and relnorm(hg_i, gg_i) <= tol["grad"]
    y_r, y_i = s.get_gain_coeffs()
    assert not y_r.any() and not y_i.any()
    np.testing.assert_array_equal(s.get_params()[0], np.asarray(start["g_r"], dtype=dtype))
    s.close()


# ---- 5. / 6. trajectories ---------------------------------------------------------------------------------------------
CASES = {"general": dict(nants=9, nfreqs=40, seed=5, layout="stream", kernel_path="auto"),
         "dense": dict(nants=12, nfreqs=200, seed=6, layout="shared", kernel_path="dense")}


def gpu_fit(p, start, dtype, B, case, optimizer, reg=False, maxsteps=30, lr=1e-2, launch=None, **run_kw):
    s = make_solver(p, start, dtype, case["layout"], reg, kernel_path=case["kernel_path"])
    if launch:
        s.set_launch_mode(launch)
    s.set_gain_basis(B)
    s.set_optimizer(optimizer, learning_rate=lr)
    s.run(1, record=False, freeze_model=run_kw.get("freeze_model", False))
    losses, stopped, nupd = s.run(maxsteps, record=True, **run_kw)
    which = 1 if run_kw.get("use_min") else 0
    g_r, g_i, c_r, c_i = s.get_params(which)
    y_r, y_i = s.get_gain_coeffs(which)
    s.close()
    return dict(loss=losses, stopped=stopped, nupd=nupd, g=cplx(g_r, g_i), c_r=c_r, c_i=c_i, y=cplx(y_r, y_i))


def check_against(out, ref_loss, ref_g, ref_y, ref_c_r, ref_c_i, tol):
    assert len(out["loss"]) == len(ref_loss)
    print(f"loss {np.max(np.abs(out['loss'] - ref_loss) / ref_loss):.2e}  g {relnorm(out['g'], ref_g):.2e}  y {relnorm(out['y'], ref_y):.2e}  "
          f"c {relnorm(out['c_r'], ref_c_r):.2e} {relnorm(out['c_i'], ref_c_i):.2e}")
    np.testing.assert_allclose(out["loss"], ref_loss, rtol=max(tol, 1e-7) if tol > 1e-8 else tol)
    assert relnorm(out["g"], ref_g) <= tol
    assert relnorm(out["y"], ref_y) <= tol
    assert relnorm(out["c_r"], ref_c_r) <= tol and relnorm(out["c_i"], ref_c_i) <= tol


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("optimizer", ["Adam", "Adamax"])
@pytest.mark.parametrize("case", ["general", "dense"])
def test_identity_basis_is_the_per_channel_fit(dtype, optimizer, case):
    cs = CASES[case]
    p, start = make_case(seed=cs["seed"], nants=cs["nants"], nfreqs=cs["nfreqs"], perturb=False)
    ch, fg_r, fg_i = oracle_inputs(p, start)
    ref = R.fit_gains_and_foregrounds(start["g_r"], start["g_i"], fg_r, fg_i, ch["data_r"], ch["data_i"], ch["wgts"], ch["fg_comps"],
                                      ch["corr_inds"], maxsteps=30, optimizer=optimizer, learning_rate=1e-2)
    out = gpu_fit(p, start, dtype, np.eye(p.nfreqs), cs, optimizer, tol=1e-14)
    assert not out["stopped"] and out["nupd"] == 30
    ref_g = cplx(ref[0], ref[1])
    check_against(out, np.asarray(ref[4]["loss"], dtype=np.float64), ref_g, ref_g - cplx(start["g_r"], start["g_i"]),
                  problem.coeffs_from_chunks(p, ref[2]), problem.coeffs_from_chunks(p, ref[3]), TOL[dtype]["traj"])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("optimizer", ["Adam", "Adamax"])
@pytest.mark.parametrize("case", ["general", "dense"])
@pytest.mark.parametrize("reg", [False, True])
def test_dpss_basis_trajectory(dtype, optimizer, case, reg):
    cs = CASES[case]
    p, start = make_case(seed=cs["seed"], nants=cs["nants"], nfreqs=cs["nfreqs"], with_sky=reg, perturb=True)
    ch, fg_r, fg_i = oracle_inputs(p, start)
    B = dpss_basis(p).astype(dtype).astype(np.float64)
    assert 1 < B.shape[1] < p.nfreqs // 2
    ref = gamma_fit(B, start["g_r"], start["g_i"], fg_r, fg_i, ch, 30, optimizer, reg=reg, learning_rate=1e-2)
    out = gpu_fit(p, start, dtype, B, cs, optimizer, reg=reg, tol=1e-14)
    tol = TOL[dtype]["traj"]
    check_against(out, ref["loss"], cplx(ref["g_r"], ref["g_i"]), cplx(ref["y_r"], ref["y_i"]), problem.coeffs_from_chunks(p, ref["fg_r"]),
                  problem.coeffs_from_chunks(p, ref["fg_i"]), tol)
    # the gains the solver returns are g0 + B y of the coefficients it returns; nothing of the correction lies outside span(B)
    g0 = cplx(np.asarray(start["g_r"], dtype=dtype), np.asarray(start["g_i"], dtype=dtype))
    assert relnorm(out["g"], g0 + out["y"] @ B.T) <= tol
    if dtype == np.float64:
        assert out_of_span(B, out["g"] - g0) <= 1e-12 * np.linalg.norm(out["g"])
    assert np.linalg.norm(out["y"]) > 0


def test_dpss_basis_loop_controls():
    """freeze_model, use_min and the tolerance stop with a basis, against the restatement (fp64)."""
    cs = CASES["general"]
    p, start = make_case(seed=7, perturb=False)
    ch, fg_r, fg_i = oracle_inputs(p, start)
    B = dpss_basis(p)
    g0 = cplx(start["g_r"], start["g_i"])
    # tolerance stop: on the same step
    ref = gamma_fit(B, start["g_r"], start["g_i"], fg_r, fg_i, ch, 400, "Adam", tol=1e-6, learning_rate=5e-2)
    assert 2 <= len(ref["loss"]) < 400
    out = gpu_fit(p, start, np.float64, B, cs, "Adam", maxsteps=400, lr=5e-2, tol=1e-6)
    assert out["stopped"] and len(out["loss"]) == len(ref["loss"]) == out["nupd"]
    assert relnorm(out["g"], cplx(ref["g_r"], ref["g_i"])) <= 1e-8
    # use_min: the snapshot is y's; the returned gains are g0 + B y_snap
    ref = gamma_fit(B, start["g_r"], start["g_i"], fg_r, fg_i, ch, 60, "RMSprop", use_min=True, learning_rate=0.1)
    assert np.argmin(ref["loss"]) < 59  # (RMSprop at this step size wanders around the minimum: the snapshot is not the last state)
    out = gpu_fit(p, start, np.float64, B, cs, "RMSprop", maxsteps=60, lr=0.1, use_min=True, tol=1e-14)
    np.testing.assert_allclose(out["loss"], ref["loss"], rtol=1e-8)
    assert relnorm(out["y"], cplx(ref["y_r"], ref["y_i"])) <= 1e-8 and relnorm(out["g"], cplx(ref["g_r"], ref["g_i"])) <= 1e-8
    assert relnorm(out["g"], g0 + out["y"] @ B.T) <= 1e-12
    assert relnorm(out["c_r"], problem.coeffs_from_chunks(p, ref["fg_r"])) <= 1e-8
    # freeze_model: gains only
    ref = gamma_fit(B, start["g_r"], start["g_i"], fg_r, fg_i, ch, 20, "Adam", freeze_model=True, learning_rate=5e-2)
    out = gpu_fit(p, start, np.float64, B, cs, "Adam", maxsteps=20, lr=5e-2, freeze_model=True, tol=1e-14)
    np.testing.assert_allclose(out["loss"], ref["loss"], rtol=1e-8)
    assert relnorm(out["g"], cplx(ref["g_r"], ref["g_i"])) <= 1e-8
    np.testing.assert_array_equal(out["c_r"], start["c_r"])


# ---- 7. slices --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,kernel_path,reg", [("stream", "auto", False), ("stream", "auto", True), ("shared", "dense", False)])
def test_three_slices_equal_three_solvers(layout, kernel_path, reg):
    from calamity_amd.solver import HipFitSolver

    nfreqs = 200 if kernel_path == "dense" else 96
    cache, parts = {}, []
    for t, noise in enumerate((1e-4, 3e-2, 1e-3)):
        p, _, start = synthetic.make_problem(7, nfreqs, f0=150e6, df=400e3, seed=100 + t, noise_frac=noise, with_sky=True, operator_cache=cache)
        parts.append((p, start))
    B = dpss_basis(parts[0][0])
    pri = lambda p: (float(np.sum(p.sky_r * p.wgts)), float(np.sum(p.sky_i * p.wgts)))  # noqa: E731
    run_kw = dict(nsteps=300, record=True, tol=1e-5, use_min=True)
    alone = []
    for p, start in parts:
        s = HipFitSolver(dtype=np.float64)
        s.set_problem(p, layout=layout, kernel_path=kernel_path)
        s.set_params(start["g_r"], start["g_i"], start["c_r"], start["c_i"])
        s.set_regularization("sum" if reg else None, *(pri(p) if reg else (0.0, 0.0)))
        s.set_gain_basis(B)
        s.set_optimizer("Adam", learning_rate=1e-2)
        s.run(1, record=False)
        losses, stopped, nupd = s.run(**run_kw)
        alone.append((losses, stopped, nupd, s.get_params(0), s.get_params(1), s.get_gain_coeffs(0), s.get_gain_coeffs(1)))
        s.close()
    big, start = distributed.batch_time_slices(parts, per_slice=True)
    s = HipFitSolver(dtype=np.float64)
    s.set_problem(big, layout=layout, kernel_path=kernel_path)
    s.set_params(start["g_r"], start["g_i"], start["c_r"], start["c_i"])
    if reg:
        pr = np.asarray([pri(p) for p, _ in parts])
        s.set_regularization("sum", pr[:, 0], pr[:, 1])
    else:
        s.set_regularization(None)
    s.set_gain_basis(B)
    s.set_optimizer("Adam", learning_rate=1e-2)
    s.run_slices(1, record=False)
    res = s.run_slices(**run_kw)
    cur, best, y_cur, y_best = s.get_params(0), s.get_params(1), s.get_gain_coeffs(0), s.get_gain_coeffs(1)
    s.close()
    na = parts[0][0].nants
    n = [len(r[0]) for r in res]
    assert len(set(n)) > 1 and min(n) < 300, n  # the slices stop on their own, at different steps
    for t, (r, a) in enumerate(zip(res, alone)):
        rows = slice(t * na, (t + 1) * na)
        assert len(r[0]) == len(a[0]) and r[1] == a[1] and r[2] == a[2]
        np.testing.assert_allclose(r[0], a[0], rtol=1e-12)
        for k in (0, 1):
            assert relnorm(cur[k][rows], a[3][k]) <= 1e-12 and relnorm(best[k][rows], a[4][k]) <= 1e-12
            assert relnorm(y_cur[k][rows], a[5][k]) <= 1e-12 and relnorm(y_best[k][rows], a[6][k]) <= 1e-12


# ---- 8. launch modes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("case,reg", [("general", False), ("general", True), ("dense", False)])
def test_launch_modes_bit_identical(dtype, case, reg):
    cs = CASES[case]
    p, start = make_case(seed=21, with_sky=reg, nants=cs["nants"], nfreqs=cs["nfreqs"])
    B = dpss_basis(p)
    runs = {}
    for mode in ("kernels", "auto", "one_tail", "graph", "kernels"):
        out = gpu_fit(p, start, dtype, B, cs, "Adam", reg=reg, maxsteps=53, lr=2e-2, launch=mode, use_min=True, tol=0.0)
        assert len(out["loss"]) == 53 and np.all(np.isfinite(out["loss"])) and out["loss"][-1] < out["loss"][0]
        if "kernels" in runs:  # (the second "kernels" run: two runs are bitwise equal)
            for k in ("loss", "g", "y", "c_r", "c_i"):
                np.testing.assert_array_equal(out[k], runs["kernels"][k], err_msg=f"{mode}: {k}")
        runs[mode] = out


# ---- 9. exchange --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("reg", [False, True])
def test_exchange_carries_the_projected_gradient(dtype, reg):
    from calamity_amd.solver import HipFitSolver

    p, start = make_case(seed=3, with_sky=reg)
    B = dpss_basis(p)
    K = B.shape[1]
    kpad = (K + 7) // 8 * 8  # documented: include/calamity_hip.h
    fpad = 64  # 40 channels: rows are padded to min(128, next power of two)
    calls = []
    s = HipFitSolver(dtype=dtype)
    s.set_exchange_hook(lambda arr, op: calls.append((arr.dtype.str, int(arr.size))), 0, 1)
    s.set_problem(p, layout="stream", kernel_path="general")
    s.set_params(start["g_r"], start["g_i"], start["c_r"], start["c_i"])
    if reg:
        s.set_regularization("sum", np.sum(p.sky_r * p.wgts), np.sum(p.sky_i * p.wgts))
    s.set_optimizer("Adam", learning_rate=1e-2)
    real = np.dtype(dtype).str
    planes = 3 if reg else 1
    del calls[:]
    s.run(3, record=False)
    per_channel = [c for c in calls if c[0] == real and c[1] > 4]
    assert [c[1] for c in per_channel] == [planes * 2 * p.nants * fpad] * 3
    s.set_params(start["g_r"], start["g_i"], start["c_r"], start["c_i"])  # back to the start: the basis fit below begins where a fresh solver's does
    s.set_gain_basis(B)  # (moments and iteration count start over)
    del calls[:]
    s.run(1, record=False)
    losses, _, _ = s.run(5, record=True, tol=0.0)
    grad_calls = [c for c in calls if c[0] == real and c[1] > 4]
    assert [c[1] for c in grad_calls] == [planes * 2 * p.nants * kpad] * 6, calls
    assert planes * 2 * p.nants * kpad < 2 * p.nants * fpad
    assert len(calls) == 2 * 6  # per step: the gradient planes and the loss scalars, nothing else
    # ... and the one-rank exchange changes no number
    ref = gpu_fit(p, start, dtype, B, CASES["general"], "Adam", reg=reg, maxsteps=5, launch="kernels", tol=0.0)
    np.testing.assert_array_equal(losses, ref["loss"])
    s.close()


def smooth_gain_uvdata(seed=7, nants=7, nfreqs=64, ntimes=3, dly_ns=60.0, sigma=0.05):
    """synthetic.make_uvdata's array (its gains are unity) with gains that ARE smooth in frequency multiplied in: 1 + B y_true with
    the DPSS basis of ``dly_ns`` (inside the 100 ns the fits below allow), different for every time."""
    uvd, sky, _ = synthetic.make_uvdata(nants=nants, nfreqs=nfreqs, ntimes=ntimes, seed=seed, redundant=True, flag_frac=0.02)
    rng = np.random.default_rng(seed + 1)
    freqs = np.asarray(uvd.freq_array, dtype=np.float64).ravel()
    Bt = np.array(modeling.gain_dpss_basis(freqs, dly_ns))
    ants = np.asarray(cal_utils.blank_uvcal_from_uvdata(uvd).ant_array).tolist()
    vis = uvcompat.vis3(uvd.data_array)
    amp = np.sqrt(np.mean(np.abs(vis) ** 2))
    for k, t in enumerate(np.unique(uvd.time_array)):
        y = sigma * (rng.standard_normal((len(ants), Bt.shape[1])) + 1j * rng.standard_normal((len(ants), Bt.shape[1])))
        g = 1.0 + y @ Bt.T
        sel = np.where(np.isclose(uvd.time_array, t, atol=1e-7, rtol=0.0))[0]
        for n in sel:
            i, j = ants.index(uvd.ant_1_array[n]), ants.index(uvd.ant_2_array[n])
            vis[n, :, 0] *= g[i] * np.conj(g[j])
        noise = amp * 10.0 ** (-3.0 - 0.5 * k)
        vis[sel, :, 0] += noise * (rng.standard_normal((len(sel), nfreqs)) + 1j * rng.standard_normal((len(sel), nfreqs)))
    return uvd, sky, freqs


def same(a, b, rtol):
    assert np.linalg.norm(np.asarray(a) - np.asarray(b)) <= rtol * max(np.linalg.norm(np.asarray(b)), 1e-300)


def equal_outputs(out1, out2, rtol):
    (m1, r1, g1, h1), (m2, r2, g2, h2) = out1, out2
    assert sorted(h1) == sorted(h2)
    for pol in h1:
        assert sorted(h1[pol]) == sorted(h2[pol])
        for ti in h1[pol]:
            l1, l2 = np.asarray(h1[pol][ti]["loss"], dtype=np.float64), np.asarray(h2[pol][ti]["loss"], dtype=np.float64)
            assert len(l1) == len(l2), (pol, ti, len(l1), len(l2))
            np.testing.assert_allclose(l1, l2, rtol=rtol)
    same(m1.data_array, m2.data_array, rtol)
    same(r1.data_array, r2.data_array, rtol * 1e2)  # a difference of nearly equal numbers
    same(g1.gain_array, g2.gain_array, rtol)


def test_two_workers_on_one_gpu_equal_one_worker():
    """devices=[0, 0] (as tests/test_gpu_dropin_batched.py): two workers share the fitting groups and exchange the PROJECTED
    gain gradients through host memory every step -- against the one-worker call, fp64 1e-10."""
    uvd, sky, freqs = smooth_gain_uvdata(seed=13, nants=8)
    kw = dict(min_dly=2.0 / 0.3, offset=2.0 / 0.3, uvdata=uvd, gains=None, sky_model=None, maxsteps=300, tol=3e-9, correct_resid=True,
              optimizer="Adam", learning_rate=1e-2, dtype=np.float64, use_min=True, gain_max_dly=100.0)
    one = calibration.calibrate_and_model_dpss(devices=[0], **kw)
    two = calibration.calibrate_and_model_dpss(devices=[0, 0], device_split="groups", **kw)
    equal_outputs(one, two, 1e-10)
    by_slices = calibration.calibrate_and_model_dpss(devices=[0, 0], device_split="slices", batch_slices=1, **kw)
    equal_outputs(one, by_slices, 1e-10)
    assert np.abs(one[2].gain_array - 1.0).max() > 1e-3


# ---- 10. detach, what is refused ----------------------------------------------------------------------------------------
def test_detach_restores_the_per_channel_fit_and_refusals():
    p, start = make_case(seed=5)
    B = dpss_basis(p)

    def per_channel(s):
        s.set_params(start["g_r"], start["g_i"], start["c_r"], start["c_i"])
        s.set_optimizer("Adam", learning_rate=1e-2)
        s.run(1, record=False)
        losses, _, _ = s.run(40, record=True, tol=0.0, use_min=True)
        return [losses] + list(s.get_params(0)) + list(s.get_params(1))

    for dtype in (np.float64, np.float32):
        plain = make_solver(p, start, dtype)
        want = per_channel(plain)
        s = make_solver(p, start, dtype)
        s.set_gain_basis(B)
        s.set_optimizer("Adam", learning_rate=1e-2)
        s.run(7, record=True, use_min=True)
        with pytest.raises(_lib.CalamityHipError, match="gain basis is not supported") as err:
            s.get_moments()
        assert err.value.code == -5  # CAL_ERR_UNSUPPORTED
        with pytest.raises(_lib.CalamityHipError, match="LAMB") as err:
            s.set_optimizer("LAMB")
        assert err.value.code == -5
        s.set_gain_basis(None)
        with pytest.raises(_lib.CalamityHipError, match="no gain basis"):
            s.get_gain_coeffs()
        got = per_channel(s)
        for a, b in zip(got, want):
            np.testing.assert_array_equal(a, b)
        s.get_moments()  # works again
        # set_params with gains while a basis is set: g0 := those gains, y := 0
        s.set_gain_basis(B)
        s.set_optimizer("Adam", learning_rate=1e-2)
        s.run(5, record=False)
        assert np.any(s.get_gain_coeffs()[0])
        s.set_params(g_r=start["g_r"], g_i=start["g_i"])
        assert not np.any(s.get_gain_coeffs()[0]) and not np.any(s.get_gain_coeffs()[1])
        np.testing.assert_array_equal(s.get_params()[0], np.asarray(start["g_r"], dtype=dtype))
        s.close()
        plain.close()
    s = make_solver(p, start, np.float64)
    for bad in (np.ones((p.nfreqs + 1, 3)), np.ones(p.nfreqs), np.ones((p.nfreqs, 2)) * 1j):
        with pytest.raises(ValueError):
            s.set_gain_basis(bad)
    with pytest.raises(_lib.CalamityHipError):
        s.set_gain_basis(np.full((p.nfreqs, 2), np.nan))
    s.close()


# ---- 11. recovery ---------------------------------------------------------------------------------------------------------
def test_recovery_of_smooth_gains():
    """9 antennas x 64 channels x 400 kHz, true gains 1 + B y_true with the 100-ns basis (y_true of sigma 0.1), noise 1e-4, 5 %
    flags, unity start, Adam lr 1e-2, 300 steps.  The reference's quality criterion rms(data) >= 100 rms(resid) is asserted of the
    fp64 restatement on the same tensors first (about 500: the inputs leave a wide margin), then of the GPU fit."""
    p, truth, start = synthetic.make_problem(9, 64, f0=150e6, df=400e3, seed=11, gain_sigma=0.0, noise_frac=1e-4)  # (unity gains, 5 % flags)
    rng = np.random.default_rng(3)
    B = dpss_basis(p)
    assert B.shape[1] == 12
    y_true = 0.1 * (rng.standard_normal((p.nants, B.shape[1])) + 1j * rng.standard_normal((p.nants, B.shape[1])))
    g_true = 1.0 + y_true @ B.T
    d = (p.data_r + 1j * p.data_i) * g_true[p.bl_ant0] * np.conj(g_true[p.bl_ant1])
    p.data_r, p.data_i = np.ascontiguousarray(d.real), np.ascontiguousarray(d.imag)
    # the fit starts from unity gains and c0 = A^T (d mask) of the new data
    mask = (p.wgts > 0).astype(np.float64)
    c0_r, c0_i = np.empty_like(start["c_r"]), np.empty_like(start["c_i"])
    coff = np.concatenate([[0], np.cumsum([p.basis[u].shape[1] for u in p.grp_basis])])
    for n, u in enumerate(p.grp_basis):
        c0_r[coff[n]:coff[n + 1]] = p.basis[u].T @ (p.data_r[n] * mask[n])
        c0_i[coff[n]:coff[n + 1]] = p.basis[u].T @ (p.data_i[n] * mask[n])
    start = dict(g_r=np.ones((p.nants, p.nfreqs)), g_i=np.zeros((p.nants, p.nfreqs)), c_r=c0_r, c_i=c0_i)
    ch, fg_r, fg_i = oracle_inputs(p, start)
    a0, a1 = R.ant_inds_from_corr_inds(ch["corr_inds"])

    def quality(model_r, model_i):
        resid = (p.data_r - model_r) + 1j * (p.data_i - model_i)
        sel = p.wgts > 0
        return np.sqrt(np.mean(np.abs(p.data_r + 1j * p.data_i)[sel] ** 2)) / np.sqrt(np.mean(np.abs(resid[sel]) ** 2))

    ref = gamma_fit(B, start["g_r"], start["g_i"], fg_r, fg_i, ch, 300, "Adam", tol=0.0, learning_rate=1e-2)
    # the restatement's data model, per baseline: g_i conj(g_j) (A c) -- one baseline per group here
    g_fit = cplx(ref["g_r"], ref["g_i"])
    c_fit = cplx(problem.coeffs_from_chunks(p, ref["fg_r"]), problem.coeffs_from_chunks(p, ref["fg_i"]))
    m = np.stack([g_fit[p.bl_ant0[n]] * np.conj(g_fit[p.bl_ant1[n]]) * (p.basis[u] @ c_fit[coff[n]:coff[n + 1]]) for n, u in enumerate(p.grp_basis)])
    q_ref = quality(m.real, m.imag)
    print(f"restatement: loss {ref['loss'][0]:.3e} -> {ref['loss'][-1]:.3e}, rms(data) / rms(resid) = {q_ref:.1f}")
    assert q_ref >= 100.0
    for dtype in (np.float64, np.float32):
        s = make_solver(p, start, dtype)
        s.set_gain_basis(B)
        s.set_optimizer("Adam", learning_rate=1e-2)
        s.run(1, record=False)
        losses, _, _ = s.run(300, record=True, tol=0.0)
        q = quality(*[np.asarray(a, dtype=np.float64) for a in s.data_model()])
        g_r, g_i, _, _ = s.get_params()
        print(f"{np.dtype(dtype).name}: loss {losses[0]:.3e} -> {losses[-1]:.3e}, rms(data) / rms(resid) = {q:.1f}")
        assert q >= 100.0
        if dtype == np.float64:
            assert out_of_span(B, cplx(g_r, g_i) - 1.0) <= 1e-12 * np.linalg.norm(cplx(g_r, g_i))
        s.close()


# ---- 12. drop-in --------------------------------------------------------------------------------------------------------
def test_dropin_batched_equals_loop_and_stays_in_span(tmp_path, monkeypatch):
    uvd, sky, freqs = smooth_gain_uvdata()
    B = np.array(modeling.gain_dpss_basis(freqs, 100.0))
    kw = dict(min_dly=2.0 / 0.3, offset=2.0 / 0.3, uvdata=uvd, sky_model=None, maxsteps=400, tol=3e-9, correct_resid=True, correct_model=True,
              optimizer="Adam", learning_rate=1e-2, dtype=np.float64, model_regularization="sum", use_min=True)
    loop = calibration.calibrate_and_model_dpss(batch_slices=False, gains=None, gain_max_dly=100.0, **kw)
    batched = calibration.calibrate_and_model_dpss(gains=None, gain_max_dly=100.0, **kw)
    equal_outputs(loop, batched, 1e-10)
    # gain_basis = the same basis given as an array
    given = calibration.calibrate_and_model_dpss(gains=None, gain_basis=B, **kw)
    equal_outputs(batched, given, 1e-10)
    g = uvcompat.gain4(batched[2].gain_array)[:, :, :, 0]  # [ants, freqs, times]
    assert np.abs(g - 1.0).max() > 1e-2
    for ti in range(g.shape[2]):
        assert out_of_span(B, g[:, :, ti] - 1.0) <= 1e-10 * np.linalg.norm(g[:, :, ti])
    # the per-channel fit of the same data does leave span(B): the constraint is what keeps the basis fit inside
    free = calibration.calibrate_and_model_dpss(gains=None, **kw)
    gf = uvcompat.gain4(free[2].gain_array)[:, :, 0, 0]
    assert out_of_span(B, gf - 1.0) > 1e-6 * np.linalg.norm(gf)
    with pytest.raises(ValueError, match="not both"):
        calibration.calibrate_and_model_dpss(gains=None, gain_basis=B, gain_max_dly=100.0, **kw)
    # the chain over times: every time starts from the previous one's gains, so its correction to THOSE lies in span(B) -- and with it
    # the whole of g - 1
    chain = calibration.calibrate_and_model_dpss(gains=None, gain_max_dly=100.0, init_guesses_from_previous_time_step=True, **kw)
    gc = uvcompat.gain4(chain[2].gain_array)[:, :, :, 0]
    for ti in range(gc.shape[2]):
        assert out_of_span(B, gc[:, :, ti] - 1.0) <= 1e-10 * np.linalg.norm(gc[:, :, ti])
    # input gains from a calfits file: g0 is the file's gains (white in frequency here: NOT in span(B)), the correction is in span(B)
    g_in = cal_utils.blank_uvcal_from_uvdata(uvd)
    rng = np.random.default_rng(5)
    g_in.gain_array = g_in.gain_array * (1.0 + 0.02 * rng.standard_normal(g_in.gain_array.shape))
    g_in.x_orientation = "east"
    data, gname = str(tmp_path / "data.uvh5"), str(tmp_path / "in.calfits")
    uvd.write_uvh5(data)
    g_in.write_calfits(gname)
    g_file = uvcompat.gain4(calfits.read_calfits(gname).gain_array)[:, :, :, 0].copy()
    outs = [str(tmp_path / n) for n in ("resid.uvh5", "model.uvh5", "gains.calfits")]
    monkeypatch.setattr(sys, "argv", [sys.argv[0], "--input_data_files", data, "--input_gain_files", gname, "--resid_outfilename", outs[0],
                                      "--model_outfilename", outs[1], "--gain_outfilename", outs[2], "--precision", "64", "--maxsteps", "200",
                                      "--optimizer", "Adam", "--gain_max_dly", "100", "--model_regularization", "sum", "--min_dly", str(2.0 / 0.3), "--offset", str(2.0 / 0.3)])
    # (model_regularization "sum", not the parser's "post_hoc": the post-hoc renormalisation rescales the fitted gains as a whole, input
    # gains included, which is its job and takes g - g_in out of span(B))
    args = calibration.dpss_fit_argparser().parse_args()
    assert args.gain_max_dly == 100.0
    cli = calibration.read_calibrate_and_model_dpss(**vars(args))
    assert cli[3]["calibration_kwargs"]["gain_max_dly"] == 100.0
    g_out = uvcompat.gain4(cli[2].gain_array)[:, :, :, 0]
    assert np.abs(g_out - g_file).max() > 1e-3
    for ti in range(g_out.shape[2]):
        assert out_of_span(B, g_out[:, :, ti] - g_file[:, :, ti]) <= 1e-10 * np.linalg.norm(g_out[:, :, ti])
        assert out_of_span(B, g_file[:, :, ti] - 1.0) > 1e-4 * np.linalg.norm(g_file[:, :, ti])
    # the calfits file the run wrote holds the gains of the API call with the same arguments
    api = calibration.read_calibrate_and_model_dpss(**dict(vars(args), input_gain_files=copy.deepcopy(g_in), resid_outfilename=None,
                                                           model_outfilename=None, gain_outfilename=None))
    assert np.array_equal(calfits.read_calfits(outs[2]).gain_array, cli[2].gain_array)
    same(api[2].gain_array, cli[2].gain_array, 1e-10)
