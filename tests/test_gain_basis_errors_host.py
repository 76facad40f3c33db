"""Host side of the error bars of basis gains (cal_solver_gain_basis_errors; no GPU): the identities and limits of the fp64 restatement
(tests/gain_basis_errors_ref.py), a statistical check of the formula itself, what fp32 costs on the shapes the GPU tests use, the
bookkeeping of ``fit_errors_arrays``, the keyword's refusals, the signatures and the planner's chunks.

The statistical check.  For one antenna with the others and the model held fixed the data are ``d_b[f] = g_a[f] h_b[f] + n_b[f]``,
``h`` the other antenna's gain times the model, ``E|n|^2 = 1 / w``, and ``g_a = B y`` is a linear least-squares problem.  R noise
realisations are solved with ``numpy.linalg.lstsq`` on the stacked weighted design (which never forms N); the empirical variance of
the fitted gain, averaged over the channels as a ratio to the predicted ``gain_var``, has a relative scatter of about ``1 / sqrt(R K)``
(K independent complex numbers per realisation), so it must lie within ``5 / sqrt(R K)`` of 1: R = 400, K = 10 gives 7.9 %."""
import ctypes as C
import inspect

import numpy as np
import pytest

import _plan_cases as pc
from calamity_amd import _lib, calibration, synthetic
from gain_basis_errors_ref import basis_errors, den_of, emulated_fp32_error
from test_gain_basis_solve_host import no_solver  # noqa: F401  (the fixture)
from test_gain_time_basis_host import joint_case
from test_gain_time_solve_host import SHAPES, TIME_ONLY_SHAPES, bases_of, flagged_case, rand_basis
from test_gpu_gain_solve import model_of
from test_solve_plan_host import _case, _row_rule

FREQ_SHAPES = [(7, 200), (12, 129), (5, 48)]
FREQ_WIDTHS = [(shape, K) for shape in FREQ_SHAPES for K in (1, 12, 33, 65, 130) if K <= shape[1]]


def freq_case(shape):
    """``flagged_case`` at one time: antenna 2 (flagged at time 0) and the last antenna are the singular rows."""
    return flagged_case(1, *shape)


# ---- identities at ridge = 0
@pytest.mark.parametrize("shape,K", [((7, 200), 12), ((12, 129), 65), ((5, 48), 33)])
def test_frequency_basis_den_gain_var_adds_up_to_the_vectors(shape, K):
    p, params = freq_case(shape)
    den = den_of(p, params, np.float64)
    out = basis_errors(den, None, rand_basis(shape[1], K, 2), ridge=0.0)
    solved = np.any(out["gain_var"] != 0, axis=1)
    assert out["nsolved"] == solved.sum() == shape[0] - 2 and out["nsingular"] == 2
    np.testing.assert_allclose(np.sum(den * out["gain_var"], axis=1)[solved], K, rtol=1e-10)
    np.testing.assert_allclose(out["gain_dof"][solved], K, rtol=1e-12)
    assert not np.any(out["gain_dof"][~solved]) and not np.any(out["y_var"][~solved])
    assert den[1, 3] == 0 and out["gain_var"][1, 3] > 0  # the basis interpolates across the flagged channel


@pytest.mark.parametrize("shape,kind,LK", [SHAPES[0], SHAPES[3]])
def test_time_frequency_basis_den_gain_var_adds_up_to_the_unknowns(shape, kind, LK):
    T, na, F = shape
    p, params = flagged_case(*shape)
    Bt, B = bases_of(shape, kind, LK)
    den = den_of(p, params, np.float64)
    out = basis_errors(den, Bt, B, ridge=0.0)
    n = Bt.shape[1] * B.shape[1]
    assert (out["nsolved"], out["nsingular"]) == (na - 1, 1)
    total = np.sum((den * out["gain_var"]).reshape(T, na, F), axis=(0, 2))
    np.testing.assert_allclose(total[: na - 1], n, rtol=1e-9)
    np.testing.assert_allclose(out["gain_dof"][: na - 1], n, rtol=1e-12)
    assert total[na - 1] == 0 and out["gain_dof"][na - 1] == 0 and not np.any(out["gain_var"][na - 1 :: na])
    assert not np.any(den[2]) and np.all(out["gain_var"][2] > 0)  # antenna 2 has no data at time 0: the time basis interpolates


@pytest.mark.parametrize("shape,L", TIME_ONLY_SHAPES[:2])
def test_time_basis_alone_den_gain_var_adds_up_per_channel(shape, L):
    T, na, F = shape
    p, params = flagged_case(*shape)
    Bt = bases_of(shape, ("rand",), (L, None))[0]
    den = den_of(p, params, np.float64)
    out = basis_errors(den, Bt, None, ridge=0.0)
    assert (out["nsolved"], out["nsingular"]) == ((na - 1) * F - 1, F + 1)
    per = np.sum((den * out["gain_var"]).reshape(T, na, F), axis=0)
    solved = np.any(out["gain_var"].reshape(T, na, F) != 0, axis=0)
    np.testing.assert_allclose(per[solved], L, rtol=1e-10)
    assert not solved[1, 3] and not np.any(solved[na - 1]) and solved.sum() == out["nsolved"]
    np.testing.assert_allclose(out["gain_dof"], L * solved.sum(axis=1), rtol=1e-12)


# ---- limits
def test_an_identity_basis_gives_one_over_den():
    p, params = joint_case(ntimes=1, nants=6, nfreqs=24)[:2]  # nothing flagged
    den = den_of(p, params, np.float64)
    assert np.all(den > 0)
    out = basis_errors(den, None, np.eye(24), ridge=0.0)
    np.testing.assert_allclose(out["gain_var"], 1.0 / den, rtol=1e-12)
    np.testing.assert_allclose(out["y_var"], 1.0 / den, rtol=1e-12)


def test_one_time_is_the_frequency_basis_ridge_included():
    p, params = freq_case((7, 200))
    den, B = den_of(p, params, np.float64), rand_basis(200, 12, 2)
    a, b = basis_errors(den, np.ones((1, 1)), B, ridge=1e-3), basis_errors(den, None, B, ridge=1e-3)
    np.testing.assert_allclose(a["gain_var"], b["gain_var"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(a["y_var"][:, 0], b["y_var"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(a["gain_dof"], b["gain_dof"], rtol=1e-12, atol=0)
    solved = b["gain_dof"] > 0
    assert np.all(b["gain_dof"][solved] < 12) and np.all(b["gain_dof"][solved] > 11.9)  # a ridge spends less than n


# ---- the formula against noise realisations
def test_the_predicted_variance_is_the_scatter_of_the_least_squares_gain():
    R, K, a = 400, 10, 0
    p, params = freq_case((7, 200))
    F, B = p.nfreqs, rand_basis(200, K, 2)
    g = np.asarray(params["g_r"]) + 1j * np.asarray(params["g_i"])
    m = model_of(p, params, np.float64)
    design = []
    for b in np.where((p.bl_ant0 != p.bl_ant1) & ((p.bl_ant0 == a) | (p.bl_ant1 == a)))[0]:
        # antenna a first: d = g_a conj(g_j) m; second: conj(d) = g_a conj(g_i) conj(m)
        h = np.conj(g[p.bl_ant1[b]]) * m[b] if p.bl_ant0[b] == a else np.conj(g[p.bl_ant0[b]]) * np.conj(m[b])
        w = p.wgts[b]
        keep = w > 0
        design.append((np.sqrt(w) * h)[keep, None] * B[keep])  # (the weighted noise has unit variance)
    A = np.concatenate(design)
    rng = np.random.default_rng(11)
    noise = (rng.standard_normal((A.shape[0], R)) + 1j * rng.standard_normal((A.shape[0], R))) / np.sqrt(2.0)
    y = np.linalg.lstsq(A, noise, rcond=None)[0]  # [K, R]: the fitted coefficients of pure noise
    empirical = np.mean(np.abs(B @ y) ** 2, axis=1)
    predicted = basis_errors(den_of(p, params, np.float64), None, B, ridge=0.0)["gain_var"][a]
    ratio = float(np.mean(empirical / predicted))
    bound = 5.0 / np.sqrt(R * K)
    print(f"empirical / predicted variance, mean over {F} channels: {ratio:.4f} (bound 1 +- {bound:.3f})")
    assert bound < 0.15 and abs(ratio - 1.0) <= bound


# ---- what fp32 costs on the shapes of the GPU tests: under a third of the fp32 bound (1e-4 of the plane's largest element)
@pytest.mark.parametrize("shape,K", FREQ_WIDTHS)
def test_fp32_emulation_on_the_frequency_widths(shape, K):
    p, params = freq_case(shape)
    gv, yv, cond = emulated_fp32_error(den_of(p, params, np.float32), None, rand_basis(shape[1], K, 2))
    print(f"{shape} K = {K}: gain_var {gv:.2e}, y_var {yv:.2e}, cond {cond:.1e}")
    assert max(gv, yv) <= 1e-4 / 3


@pytest.mark.parametrize("shape,kind,LK", SHAPES)
def test_fp32_emulation_on_the_time_frequency_shapes(shape, kind, LK):
    p, params = flagged_case(*shape)
    Bt, B = bases_of(shape, kind, LK)
    gv, yv, cond = emulated_fp32_error(den_of(p, params, np.float32), Bt, B)
    print(f"{shape} L, K = {LK}: gain_var {gv:.2e}, y_var {yv:.2e}, cond {cond:.1e}")
    assert max(gv, yv) <= 1e-4 / 3


# ---- fit_errors_arrays
def test_fit_errors_arrays_charges_gain_dof_and_a_joint_fit_its_share():
    rng = np.random.default_rng(0)
    e = dict(nsamp_bl=np.full(6, 40.0), leverage_bl=np.full(6, 3.0), gain_var=rng.uniform(1.0, 2.0, (4, 40)))
    e["gain_var"][3] = 0.0  # a singular antenna
    chisq = np.full(6, 50.0)
    free = calibration.fit_errors_arrays(e, chisq)
    assert free["p"] == 18.0 + 3 * 40
    dof = np.asarray([9.5, 9.75, 10.0, 0.0])
    one = calibration.fit_errors_arrays(e, chisq, gain_dof=dof)
    assert one["n"] == 240.0 and one["p"] == 18.0 + 29.25 and one["noise_scale"] == 300.0 / (240.0 - 47.25)
    np.testing.assert_array_equal(one["gain_std"], np.sqrt(one["noise_scale"] * e["gain_var"]))
    joint = calibration.fit_errors_arrays(e, chisq, gain_dof=dof, ntimes=3)
    assert joint["p"] == 18.0 + 29.25 / 3 and joint["noise_scale"] < one["noise_scale"]
    # without the argument nothing changes, and the docstring says what a joint fit is charged
    for k in free:
        np.testing.assert_array_equal(calibration.fit_errors_arrays(e, chisq, 1.0, None, 3)[k], free[k])
    assert "1 / ntimes" in calibration.fit_errors_arrays.__doc__
    under = calibration.fit_errors_arrays(e, chisq, gain_dof=np.full(4, 100.0))
    assert under["underdetermined"] and under["noise_scale"] == 1.0


# ---- the keyword
@pytest.mark.parametrize("kw,word", [(dict(gain_basis_errors=True, gain_max_dly=100.0), "fit_errors"),
                                     (dict(gain_basis_errors=True, gain_time_scale=1e6), "fit_errors"),
                                     (dict(gain_basis_errors=True, fit_errors=True), "gain basis"),
                                     (dict(gain_basis_errors=True, fit_errors="samples"), "gain basis")])
def test_the_keyword_needs_fit_errors_and_a_gain_basis(kw, word, no_solver):  # noqa: F811
    uvd, _, comps = synthetic.make_uvdata(nants=4, nfreqs=16, ntimes=2)
    with pytest.raises(ValueError, match=word):
        calibration.calibrate_and_model_tensor(uvdata=uvd, fg_model_comps_dict=comps, **kw)
    with pytest.raises(ValueError, match=word):
        calibration.calibrate_and_model_dpss(uvdata=uvd, **kw)


def test_signatures_and_bindings():
    from calamity_amd.batched import SliceBatchFitter
    from calamity_amd.solver import HipFitSolver

    for fn in (HipFitSolver.gain_basis_errors, SliceBatchFitter.gain_basis_errors):
        params = inspect.signature(fn).parameters
        assert list(params)[1:] == ["ridge", "y_var"] and (params["ridge"].default, params["y_var"].default) == (1e-6, True)
    for fn in (calibration.calibrate_and_model_tensor, calibration.read_calibrate_and_model_dpss):
        assert inspect.signature(fn).parameters["gain_basis_errors"].default is False
    restype, argtypes = _lib.SYMBOLS["cal_solver_gain_basis_errors"]
    assert restype is C.c_int and len(argtypes) == 6 and argtypes[1] is C.c_double
    # a report, not a fit-loop control: no command-line flag
    for ap in (calibration.dpss_fit_argparser(), calibration.fitting_argparser()):
        assert not any("gain_basis_errors" in s for a in ap._actions for s in a.option_strings)


# ---- the planner
def error_row_chunks(prob, dtype, layout, kernel_path, bound, shape, what=31):
    from calamity_amd.solver import problem_desc

    d, keep = problem_desc(prob, dtype, layout, kernel_path)
    code = _lib.CAL_F32 if np.dtype(dtype) == np.float32 else _lib.CAL_F64
    buf, n = np.zeros(256, np.uint8), C.c_int64(0)
    buf[:24].view(np.int64)[:] = shape
    _lib.check(_lib.load().cal_debug_solve_plan(code, C.byref(d), bound, what, buf.ctypes.data_as(C.c_void_p), buf.nbytes, C.byref(n)))
    del keep
    return buf[: n.value].view(np.int64).tolist()


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_the_chunks_count_w_and_the_solves_chunks_stay_where_they_are(dt):
    name = "dense_split2_f32" if dt == "f32" else "dense_f64"  # 26 antennas, 256 channels
    prob, dtype, layout, kernel_path, _, _ = _case(name)
    size, nants, nfreqs = np.dtype(dtype).itemsize, prob.nants, prob.nfreqs
    fewer = 0
    for K, L, T in [(1, 0, 0), (7, 0, 0), (126, 0, 0), (127, 0, 0), (5, 3, 2), (63, 2, 13), (64, 2, 13), (0, 3, 2), (0, pc.TIME_TILE + 1, 13)]:
        n = (L if L else 1) * K
        x_row = ((n + 15) // 16 * 16) ** 2 if K else 0
        solve = _row_rule(K, L, T, nfreqs, size, pc.CS_DEFAULT_BOUND, nants)
        row_bytes = (solve[4] + solve[5] + x_row) * size + solve[6] * 8
        nrows = nants // T if L else nants
        for bound in (0, 1, 3 * max(1, row_bytes) + 1, max(1, row_bytes) * nrows):
            b = bound or pc.CS_DEFAULT_BOUND
            want = _row_rule(K, L, T, nfreqs, size, b, nants)
            assert error_row_chunks(prob, dtype, layout, kernel_path, bound, (K, L, T), what=30) == want  # the solves' chunks
            want_rows = max(1, min(nrows, b // max(1, row_bytes)))
            got = error_row_chunks(prob, dtype, layout, kernel_path, bound, (K, L, T))
            assert got == [want_rows] + want[1:] + [x_row], ((K, L, T), bound, got)
            assert got[0] <= want[0]
            fewer += got[0] < want[0]
    assert fewer > 0
