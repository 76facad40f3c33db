"""Host side of the closed-form sweeps of a gain-basis fit (cal_solver_solve_gain_coeffs; no GPU): the parser flags, the defaults, the
argument checks of the drop-in (raised before any solver exists), the declarations in the header and the bindings, and the fp64 NumPy
restatement that the GPU tests import.

The restatement (include/calamity_hip.h).  num, den are the per-antenna sums of a per-channel sweep from the OLD gains; for antenna
row a with current gains g_a = g0_a + B y_a:

    r_a[f]  = num_a[f] - den_a[f] g_a[f]
    N_a     = B^T diag(den_a) B
    rhs_a   = B^T r_a
    (N_a + ridge (tr N_a / K) I) delta_a = rhs_a
    y_a    <- y_a + damping delta_a          then g = g0 + B y for the whole array

A row with tr N_a <= 0 or a failed Cholesky factorisation keeps its y and counts as singular."""
import ctypes as C
import functools
import inspect
import os
import re

import numpy as np
import pytest

from calamity_amd import _lib, cal_utils, calibration, modeling, synthetic
from calamity_amd.uvcompat import gain4, vis3
from test_gpu_fit_quality import edge_problem, perturbed
from test_gpu_gain_solve import model_of
from test_gpu_gain_solve import restated as restated_per_channel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ["--input_data_files", "data.uvh5"]
FLAGS = ("gain_basis_solve_sweeps", "gain_basis_solve_every", "gain_basis_solve_damping", "gain_basis_solve_ridge")
EDGE_SHAPES = [(5, 48), (7, 200), (12, 129), (6, 300)]


# ---- the restatement
def basis_sweeps(ant0, ant1, d, m, w, g0, y, B, nsweeps=1, damping=0.5, ridge=1e-6):
    """``nsweeps`` sweeps in fp64 on the arrays as given (d, m complex and w real ``[nbls, nfreqs]``; g0 complex ``[nants, nfreqs]``; y complex
    ``[nants, K]``; B real ``[nfreqs, K]``).  Returns (g, y, chi-square after every sweep, den of the first sweep, singular rows of the last)."""
    nants, K = g0.shape[0], B.shape[1]
    y = np.array(y, dtype=np.complex128)
    P, Q = w * d * np.conj(m), w * np.abs(m) ** 2
    cross = np.where(ant0 != ant1)[0]
    g = g0 + y @ B.T
    chisq, den0, nsingular = [], None, 0
    for _ in range(nsweeps):
        num = np.zeros(g0.shape, dtype=np.complex128)
        den = np.zeros(g0.shape)
        for b in cross:
            i, j = int(ant0[b]), int(ant1[b])
            num[i] += P[b] * g[j]
            den[i] += Q[b] * np.abs(g[j]) ** 2
            num[j] += np.conj(P[b]) * g[i]
            den[j] += Q[b] * np.abs(g[i]) ** 2
        den0 = den if den0 is None else den0
        nsingular = 0
        for a in range(nants):
            N = B.T @ (den[a][:, None] * B)
            tr = np.trace(N)
            if not tr > 0:
                nsingular += 1
                continue
            try:
                L = np.linalg.cholesky(N + ridge * (tr / K) * np.eye(K))
            except np.linalg.LinAlgError:
                nsingular += 1
                continue
            rhs = B.T @ (num[a] - den[a] * g[a])
            y[a] += damping * np.linalg.solve(L.T, np.linalg.solve(L, rhs))
        g = g0 + y @ B.T
        chisq.append(float(np.sum(w * np.abs(d - g[ant0] * np.conj(g[ant1]) * m) ** 2)))
    return g, y, chisq, den0, nsingular


def restated_basis(p, params, dtype, B, nsweeps=1, damping=0.5, ridge=1e-6, data=None, y=None):
    """``basis_sweeps`` on the inputs a solver of ``dtype`` holds (cast to it first): g0 = the gains of ``params``, y = 0 unless given."""
    cast = lambda a: np.asarray(a).astype(dtype).astype(np.float64)  # noqa: E731
    d_r, d_i, w = (cast(a) for a in (data if data is not None else (p.data_r, p.data_i, p.wgts)))
    g0 = cast(params["g_r"]) + 1j * cast(params["g_i"])
    Bc = cast(B)
    y0 = np.zeros((p.nants, Bc.shape[1]), dtype=np.complex128) if y is None else y
    return basis_sweeps(p.bl_ant0, p.bl_ant1, d_r + 1j * d_i, model_of(p, params, dtype), w, g0, y0, Bc, nsweeps, damping, ridge)


def dpss_basis(nfreqs, f0=150e6, df=400e3, dly=100.0):
    return np.array(modeling.gain_dpss_basis(f0 + df * np.arange(nfreqs), dly))


def identity_problem():
    p, _, start = synthetic.make_problem(7, 64, f0=150e6, df=400e3, seed=13)
    return p, perturbed(p, start, seed=14)


# ---- the inputs of the drop-in test (tests/test_gpu_gain_basis_solve_dropin.py) and what the restatement reaches on them
@functools.lru_cache(maxsize=None)
def dropin_data_set(ntimes=1):
    """(data, sky, B): data = g_i conj(g_j) x sky with g = 1 + B y, B the 100 ns DPSS basis on the file's channels and y seeded and
    scaled so that g - 1 has rms 0.1 per real part."""
    _, sky, _ = synthetic.make_uvdata(nants=6, nfreqs=64, ntimes=ntimes)
    B = np.array(modeling.gain_dpss_basis(np.asarray(sky.freq_array, dtype=np.float64).ravel(), 100.0))
    true = cal_utils.blank_uvcal_from_uvdata(sky)
    garr = gain4(true.gain_array)  # (Nants, Nfreqs, Ntimes, Njones) view
    rng = np.random.default_rng(5)
    na, nf, nt, nj = garr.shape
    y = rng.standard_normal((na, B.shape[1], nt, nj)) + 1j * rng.standard_normal((na, B.shape[1], nt, nj))
    dg = np.einsum("fk,aktj->aftj", B, y)
    dg *= 0.1 / np.sqrt(np.mean(dg.real ** 2))
    garr[...] = 1.0 + dg
    return cal_utils.apply_gains(sky, true, inverse=True), sky, B


def dropin_restated_ratio(ntimes=1, nsweeps=30, damping=0.5, ridge=1e-6):
    """rms(resid) / rms(data) at unity gains and after ``nsweeps`` sweeps of the restatement, over the times of the data set; the model is
    the sky itself (it is exactly representable in the fit's foreground basis) and the weights are uniform (nothing is flagged)."""
    uvd, sky, B = dropin_data_set(ntimes)
    ants = np.asarray(sorted(set(np.asarray(uvd.ant_1_array).tolist()) | set(np.asarray(uvd.ant_2_array).tolist())))
    index = {int(a): n for n, a in enumerate(ants)}
    num0 = num1 = den = 0.0
    for t in np.unique(uvd.time_array):
        sel = np.where(np.isclose(uvd.time_array, t, atol=1e-7, rtol=0.0))[0]
        a0 = np.asarray([index[int(a)] for a in np.asarray(uvd.ant_1_array)[sel]])
        a1 = np.asarray([index[int(a)] for a in np.asarray(uvd.ant_2_array)[sel]])
        d, m = vis3(uvd.data_array)[sel, :, 0], vis3(sky.data_array)[sel, :, 0]
        w = np.ones(d.shape)
        g0 = np.ones((len(ants), d.shape[1]), dtype=np.complex128)
        _, _, chisq, _, _ = basis_sweeps(a0, a1, d, m, w, g0, np.zeros((len(ants), B.shape[1])), B, nsweeps, damping, ridge)
        num0 += float(np.sum(np.abs(d - m) ** 2))
        num1 += chisq[-1]
        den += float(np.sum(np.abs(d) ** 2))
    return float(np.sqrt(num0 / den)), float(np.sqrt(num1 / den))


# ---- flags, defaults, checks
def test_parser_flags_and_defaults():
    for ap in (calibration.dpss_fit_argparser(), calibration.fitting_argparser()):
        args = ap.parse_args(BASE)
        assert tuple(getattr(args, k) for k in FLAGS) == (0, 0, 0.5, 1e-6)
        args = ap.parse_args(BASE + ["--gain_basis_solve_sweeps", "30", "--gain_basis_solve_every", "5", "--gain_basis_solve_damping", "0.25",
                                     "--gain_basis_solve_ridge", "1e-4"])
        assert tuple(getattr(args, k) for k in FLAGS) == (30, 5, 0.25, 1e-4)
        assert isinstance(args.gain_basis_solve_sweeps, int) and isinstance(args.gain_basis_solve_every, int)


def test_signature_defaults():
    from calamity_amd.batched import SliceBatchFitter
    from calamity_amd.solver import HipFitSolver

    for fn in (calibration.calibrate_and_model_tensor, calibration.fit_gains_and_foregrounds):
        params = inspect.signature(fn).parameters
        assert tuple(params[k].default for k in FLAGS) == (0, 0, 0.5, 1e-6)
    for fn in (HipFitSolver.solve_gain_coeffs, SliceBatchFitter.solve_gain_coeffs):
        params = inspect.signature(fn).parameters
        assert list(params)[1:] == ["nsweeps", "damping", "ridge", "slice_mask", "reset_gain_moments"]
        assert (params["damping"].default, params["ridge"].default, params["slice_mask"].default, params["reset_gain_moments"].default) == (0.5, 1e-6, None, False)


@pytest.fixture
def no_solver(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a solver was asked for")

    monkeypatch.setattr(calibration, "get_solver", refuse)
    monkeypatch.setattr(calibration, "_batch_fitter", refuse)


@pytest.mark.parametrize("bad", [dict(gain_basis_solve_sweeps=-1), dict(gain_basis_solve_every=-2), dict(gain_basis_solve_sweeps=1.5),
                                 dict(gain_basis_solve_sweeps=1, gain_basis_solve_damping=0.0), dict(gain_basis_solve_every=1, gain_basis_solve_damping=1.5),
                                 dict(gain_basis_solve_sweeps=1, gain_basis_solve_ridge=-1e-6), dict(gain_basis_solve_sweeps=1, gain_basis_solve_ridge=float("nan")),
                                 dict(gain_basis_solve_every=1, gain_basis_solve_ridge=float("inf"))])
def test_bad_values_are_refused_before_any_solver_exists(bad, no_solver):
    uvd, _, comps = synthetic.make_uvdata(nants=4, nfreqs=16)
    with pytest.raises(ValueError, match="gain_basis_solve"):
        calibration.calibrate_and_model_tensor(uvdata=uvd, fg_model_comps_dict=comps, gain_max_dly=100.0, **bad)
    with pytest.raises(ValueError, match="gain_basis_solve"):
        calibration.fit_gains_and_foregrounds(np.ones((3, 16)), np.zeros((3, 16)), None, None, None, None, None, None, None, gain_basis=np.ones((16, 1)), **bad)


@pytest.mark.parametrize("solve", [dict(gain_basis_solve_sweeps=3), dict(gain_basis_solve_every=5)])
def test_the_sweeps_need_a_frequency_basis(solve, no_solver):
    uvd, _, comps = synthetic.make_uvdata(nants=4, nfreqs=16)
    with pytest.raises(ValueError, match="gain_basis or\\s+gain_max_dly"):
        calibration.calibrate_and_model_tensor(uvdata=uvd, fg_model_comps_dict=comps, **solve)
    with pytest.raises(ValueError, match="gain_basis or\\s+gain_max_dly"):
        calibration.fit_gains_and_foregrounds(np.ones((3, 16)), np.zeros((3, 16)), None, None, None, None, None, None, None, **solve)


@pytest.mark.parametrize("solve", [dict(gain_basis_solve_sweeps=3), dict(gain_basis_solve_every=5)])
@pytest.mark.parametrize("time_basis", [dict(gain_time_scale=1e6), dict(gain_time_basis=np.ones((2, 1)))])
@pytest.mark.parametrize("freq_basis", [dict(), dict(gain_max_dly=100.0), dict(gain_basis=np.ones((16, 1)))])
def test_a_time_basis_is_refused(freq_basis, time_basis, solve, no_solver):
    uvd, _, comps = synthetic.make_uvdata(nants=4, nfreqs=16, ntimes=2)
    with pytest.raises(ValueError, match="gain_time_basis"):
        calibration.calibrate_and_model_tensor(uvdata=uvd, fg_model_comps_dict=comps, **freq_basis, **time_basis, **solve)


def test_the_per_channel_sweeps_stay_refused_with_a_basis(no_solver):
    uvd, _, comps = synthetic.make_uvdata(nants=4, nfreqs=16)
    with pytest.raises(ValueError, match="gain_solve_sweeps") as err:
        calibration.calibrate_and_model_tensor(uvdata=uvd, fg_model_comps_dict=comps, gain_max_dly=100.0, gain_solve_sweeps=3, gain_basis_solve_sweeps=3)
    assert "basis" in str(err.value) and "gain_basis_solve_sweeps" in str(err.value)


# ---- header, bindings
def test_the_call_is_declared_in_the_header_and_the_bindings():
    with open(os.path.join(ROOT, "include", "calamity_hip.h")) as f:
        header = f.read()
    assert re.search(r"int\s+cal_solver_solve_gain_coeffs\s*\(\s*cal_solver\s*\*\s*s\s*,\s*const\s+cal_gain_coeff_solve_desc\s*\*\s*desc\s*,\s*"
                     r"cal_gain_coeff_solve_result\s*\*\s*result\s*\)\s*;", header)
    fields = re.search(r"typedef struct cal_gain_coeff_solve_desc \{(.*?)\} cal_gain_coeff_solve_desc;", header, re.S).group(1)
    names = ["nsweeps", "reset_gain_moments", "damping", "ridge", "slice_mask"]
    assert re.findall(r"(\w+)\s*;", fields) == names
    assert [n for n, _ in _lib.GainCoeffSolveDesc._fields_] == names
    fields = re.search(r"typedef struct cal_gain_coeff_solve_result \{(.*?)\} cal_gain_coeff_solve_result;", header, re.S).group(1)
    assert re.findall(r"(\w+)\s*;", fields) == [n for n, _ in _lib.GainCoeffSolveResult._fields_] == ["nsolved", "nsingular"]
    assert "cal_solver_solve_gain_coeffs" in _lib.SYMBOLS
    assert C.sizeof(_lib.GainCoeffSolveDesc) == 32  # int32, int32, double, double, pointer
    assert C.sizeof(_lib.GainCoeffSolveResult) == 8
    # the per-channel call keeps its description
    assert [n for n, _ in _lib.GainSolveDesc._fields_] == ["nsweeps", "reset_gain_moments", "damping", "slice_mask"] and C.sizeof(_lib.GainSolveDesc) == 24


# ---- the restatement itself
@pytest.mark.parametrize("shape", EDGE_SHAPES)
def test_the_chi_square_never_rises_over_ten_half_damped_sweeps(shape):
    p, params = edge_problem(*shape)
    B = dpss_basis(p.nfreqs)
    g, y, chisq, den, nsingular = restated_basis(p, params, np.float64, B, nsweeps=10)
    g_start = np.asarray(params["g_r"]) + 1j * np.asarray(params["g_i"])
    d, m = p.data_r + 1j * p.data_i, model_of(p, params, np.float64)
    start = float(np.sum(p.wgts * np.abs(d - g_start[p.bl_ant0] * np.conj(g_start[p.bl_ant1]) * m) ** 2))
    losses = np.asarray([start] + chisq)
    print(f"{shape} K = {B.shape[1]}: chi-square {losses[0]:.4e} -> {losses[-1]:.4e}, largest step up {np.max(np.diff(losses)) / losses[0]:.2e} of the start")
    assert np.all(np.diff(losses) <= 0.0)
    assert nsingular == 1 and not np.any(den[p.nants - 1])  # the antenna without baselines
    assert not np.any(y[p.nants - 1]) and np.array_equal(g[p.nants - 1], g_start[p.nants - 1])
    assert den[1, 3] == 0 and g[1, 3] != g_start[1, 3]  # the flagged channel of antenna 1 moves: the basis interpolates across it
    # the update of every row lies in span(B)
    assert np.max(np.abs((g - g_start) - ((g - g_start) @ B) @ B.T)) <= 1e-12


def test_an_identity_basis_without_ridge_is_the_per_channel_sweep():
    p, params = identity_problem()
    want, _, den = restated_per_channel(p, params, np.float64, nsweeps=3)
    assert np.all(den > 0)
    got = restated_basis(p, params, np.float64, np.eye(p.nfreqs), nsweeps=3, ridge=0.0)[0]
    err = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
    print(f"identity basis against the per-channel restatement: {err:.2e}")
    assert err <= 1e-12


def test_a_full_undamped_step_lands_on_the_per_antenna_minimiser():
    """damping = 1, ridge = 0: the gradient of the chi-square with respect to y_a vanishes at the new y_a with the others at their old gains."""
    p, params = edge_problem(7, 200)
    B = dpss_basis(p.nfreqs)
    g_new, y, _, _, _ = restated_basis(p, params, np.float64, B, nsweeps=1, damping=1.0, ridge=0.0)
    g_old = np.asarray(params["g_r"]) + 1j * np.asarray(params["g_i"])
    d, m, w = p.data_r + 1j * p.data_i, model_of(p, params, np.float64), p.wgts
    a = 2
    g = g_old.copy()
    g[a] = g_new[a]
    num = np.zeros(p.nfreqs, dtype=np.complex128)
    den = np.zeros(p.nfreqs)
    for b in range(p.nbls):
        i, j = int(p.bl_ant0[b]), int(p.bl_ant1[b])
        if i == a:
            num += w[b] * d[b] * np.conj(m[b]) * g_old[j]
            den += w[b] * np.abs(m[b]) ** 2 * np.abs(g_old[j]) ** 2
        if j == a:
            num += np.conj(w[b] * d[b] * np.conj(m[b])) * g_old[i]
            den += w[b] * np.abs(m[b]) ** 2 * np.abs(g_old[i]) ** 2
    grad = B.T @ (num - den * g[a])
    assert np.max(np.abs(grad)) <= 1e-9 * np.max(np.abs(B.T @ num))


@pytest.mark.parametrize("ntimes", [1, 2])
def test_thirty_sweeps_on_the_inputs_of_the_drop_in_test(ntimes):
    """The ratio the drop-in test bounds (3 x this one): recorded here, and at most 1/30 of the ratio at unity gains."""
    r0, r1 = dropin_restated_ratio(ntimes)
    print(f"{ntimes} time(s): rms(resid) / rms(data) {r0:.3e} at unity, {r1:.3e} after 30 sweeps of the restatement: 1/{r0 / r1:.0f}")
    assert r0 > 0.1
    assert r1 <= r0 / 30.0
