"""cal_solver_solve_gain_coeffs on the device against the fp64 NumPy restatement of tests/test_gain_basis_solve_host.py: damped StefCal
sweeps projected on the gain basis g = g0 + B y.

Tolerances are the project's own (``TOL`` of tests/test_gpu_fit_quality.py): fp64 1e-10, fp32 1e-4 of the plane's largest element, on
the real and imaginary planes of the new gains and of y; losses fp64 1e-10, fp32 1e-5.  A CPU emulation of an fp32 Gram in BLAS order
with the solve in fp64 stays at or under 6.6e-6 on every shape and K used here (cond(N_a) <= 4e2), and the device's sequential sums
cost a factor of 2 ... 3 on top of that: the fp32 bound has room."""
import copy

import numpy as np
import pytest

from calamity_amd import _lib, batched, synthetic
from calamity_amd.problem import FitProblem
from test_gain_basis_solve_host import EDGE_SHAPES, dpss_basis, identity_problem, restated_basis
from test_gpu_fit_quality import TOL, edge_problem, perturbed, plane_err, solver_of

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]


def basis_solver(p, params, dtype, B, layout="shared"):
    s = solver_of(p, params, dtype, layout)
    s.set_gain_basis(B)  # g0 = the gains just set, y = 0
    return s


def random_basis(nfreqs, K, seed=3):
    q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((nfreqs, K)))
    return np.ascontiguousarray(q)


def check(s, want_g, want_y, dtype, label):
    g_r, g_i = s.get_params()[:2]
    y_r, y_i = s.get_gain_coeffs()
    errs = (plane_err(g_r, want_g.real), plane_err(g_i, want_g.imag), plane_err(y_r, want_y.real), plane_err(y_i, want_y.imag))
    print(f"{label}: g_r {errs[0]:.2e}  g_i {errs[1]:.2e}  y_r {errs[2]:.2e}  y_i {errs[3]:.2e}")
    for a in (g_r, g_i, y_r, y_i):
        assert np.all(np.isfinite(a)), label
    assert max(errs) <= TOL[np.dtype(dtype)]["plane"], (label, errs)
    return g_r, g_i, y_r, y_i


# ---- parity of ONE sweep
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", ["stream", "shared"])
@pytest.mark.parametrize("shape", EDGE_SHAPES)
def test_one_sweep_equals_the_numpy_restatement(shape, layout, dtype):
    """K = 10, 25, 19, 34 (padded to 16, 32, 24, 40); no band is a multiple of the 32-channel step but (5, 48)'s is no multiple of 32 either."""
    p, params = edge_problem(*shape)
    na = p.nants
    B = dpss_basis(p.nfreqs)
    s = basis_solver(p, params, dtype, B, layout)
    before = s.get_params()
    out = s.solve_gain_coeffs(1)
    want_g, want_y, _, den, nsing = restated_basis(p, params, dtype, B)
    g_r, g_i, y_r, y_i = check(s, want_g, want_y, dtype, f"{shape} K = {B.shape[1]} {layout} {np.dtype(dtype).name}")
    # the antenna without baselines is the one singular row: the bits it had
    assert nsing == 1 and out == {"nsolved": na - 1, "nsingular": 1}
    assert not np.any(den[na - 1]) and not np.any(y_r[na - 1]) and not np.any(y_i[na - 1])
    np.testing.assert_array_equal(g_r[na - 1], before[0][na - 1])
    np.testing.assert_array_equal(g_i[na - 1], before[1][na - 1])
    # the channel flagged on every baseline of antenna 1 moves: the basis interpolates across it
    assert den[1, 3] == 0 and g_r[1, 3] != before[0][1, 3] and g_i[1, 3] != before[1][1, 3]
    # every other antenna moved, coefficients are not touched
    assert all(np.any(g_r[a] != before[0][a]) for a in range(na - 1))
    after = s.get_params()
    np.testing.assert_array_equal(after[2], before[2])
    np.testing.assert_array_equal(after[3], before[3])
    s.close()


# ---- basis widths: one partial MFMA tile, the second 64-block with its off-diagonal block, the factor on both sides of its LDS bound
WIDTHS = [((7, 200), K) for K in (1, 12, 33, 65, 130)] + [((12, 129), K) for K in (1, 12, 33, 65)] + [((5, 48), K) for K in (1, 12, 33)]
WIDTHS += [((7, 200), K) for K in (127, 128)]  # the last factor in LDS and the first in scratch (appended: the case ids above keep their numbers)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,K", WIDTHS)
def test_basis_widths_and_one_row_chunks(shape, K, dtype):
    """K = 127 is the last factor in LDS (128 KB), K = 128 the first in scratch, K = 130 well past it.  The same call through chunks of one
    antenna row gives the same bits."""
    p, params = edge_problem(*shape)
    B = random_basis(p.nfreqs, K)
    want_g, want_y = restated_basis(p, params, dtype, B)[:2]
    got = []
    for bound in (0, 1):
        s = basis_solver(p, params, dtype, B)
        s._set_coeff_solve_scratch(bound)
        out = s.solve_gain_coeffs(1)
        assert out == {"nsolved": p.nants - 1, "nsingular": 1}
        got.append(check(s, want_g, want_y, dtype, f"{shape} K = {K} {np.dtype(dtype).name} scratch bound {bound}"))
        s.close()
    for a, b in zip(*got):
        np.testing.assert_array_equal(a, b)


# ---- the identity basis
@pytest.mark.parametrize("dtype", DTYPES)
def test_an_identity_basis_without_ridge_agrees_with_the_per_channel_sweep(dtype):
    p, params = identity_problem()
    s = basis_solver(p, params, dtype, np.eye(p.nfreqs))
    twin = solver_of(p, params, dtype)
    s.solve_gain_coeffs(1, ridge=0.0)
    twin.solve_gains(1)
    for k, (a, b) in enumerate(zip(s.get_params()[:2], twin.get_params()[:2])):
        err = plane_err(a, b)
        print(f"identity basis {np.dtype(dtype).name} plane {k}: {err:.2e}")
        assert err <= TOL[np.dtype(dtype)]["plane"]
    s.close()
    twin.close()


# ---- several sweeps
@pytest.mark.parametrize("dtype", DTYPES)
def test_three_sweeps_follow_the_restatement_and_repeat_bitwise(dtype):
    p, params = edge_problem(7, 200)
    B = dpss_basis(p.nfreqs)
    want_g, want_y, chisq, _, _ = restated_basis(p, params, dtype, B, nsweeps=3)
    tol = TOL[np.dtype(dtype)]["loss"]
    runs = []
    for calls in ([1, 1, 1], [3]):
        s = basis_solver(p, params, dtype, B, "stream")
        losses = [s.eval_loss()]
        for n in calls:
            s.solve_gain_coeffs(n)
            losses.append(s.eval_loss())
        if len(calls) == 3:
            losses = np.asarray(losses)
            print(f"{np.dtype(dtype).name}: chi-square {losses}, restatement {chisq}")
            assert np.all(np.diff(losses) <= tol * losses[:-1])
            assert np.all(np.abs(losses[1:] - np.asarray(chisq)) <= tol * np.asarray(chisq))
        runs.append(check(s, want_g, want_y, dtype, f"three sweeps as {calls} {np.dtype(dtype).name}"))
        s.close()
    for a, b in zip(*runs):
        np.testing.assert_array_equal(a, b)


# ---- slices, masks, moments
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mask", [[1, 0, 1], [0, 1, 1]])
@pytest.mark.parametrize("optimizer", ["Adam", "Adagrad"])
def test_a_mask_with_reset_gain_moments_restores_the_selected_slices_only(optimizer, mask, dtype):
    """What the batched driver calls.  The selected slices are swept and their y slots start over (Adagrad's accumulator at 0.1); the other
    slice keeps y, gains and slots to the bit; coefficients, their slots and every slice's update count stay."""
    from calamity_amd.solver import HipFitSolver

    T = 3
    parts = [synthetic.make_problem(7, 200, f0=150e6, df=400e3, seed=21, data_seed=30 + t) for t in range(T)]
    p0 = parts[0][0]
    B = dpss_basis(p0.nfreqs)
    data = tuple(np.concatenate([getattr(parts[t][0], k) for t in range(T)]) for k in ("data_r", "data_i", "wgts"))
    pars = [perturbed(parts[t][0], parts[t][2], seed=40 + t) for t in range(T)]
    start = {k: np.concatenate([pars[t][k] for t in range(T)]) for k in ("g_r", "g_i", "c_r", "c_i")}
    sub, _, _ = batched.replicate_slices(p0, T)
    label = f"{optimizer} mask {mask} {np.dtype(dtype).name}"
    s = HipFitSolver(dtype=dtype)
    s.set_problem(sub, layout="stream")
    s.set_data(*data)
    s.set_params(start["g_r"], start["g_i"], start["c_r"], start["c_i"])
    s.set_gain_basis(B)
    s.set_optimizer(optimizer, learning_rate=1e-2)
    fresh = s.get_gain_coeff_moments()
    if optimizer == "Adagrad":
        assert np.all(fresh["yv_r"] == dtype(0.1)) and np.all(fresh["yv_i"] == dtype(0.1)) and not np.any(fresh["ym_r"])
    s.run_slices(4, tol=0.0)
    moved, before, y_before = s.get_gain_coeff_moments(), s.get_params(), s.get_gain_coeffs()
    na = p0.nants
    rows = [slice(t * na, (t + 1) * na) for t in range(T)]
    for part in rows:
        assert np.any(moved["yv_r"][part] != fresh["yv_r"][part]) and np.any(moved["yv_i"][part] != fresh["yv_i"][part])
    # g0 is still the gains the basis was attached at; y and the coefficients are the four steps'
    want_g, want_y = restated_basis(sub, dict(start, c_r=before[2], c_i=before[3]), dtype, B, nsweeps=2, data=data,
                                    y=y_before[0].astype(np.float64) + 1j * y_before[1].astype(np.float64))[:2]
    out = s.solve_gain_coeffs(2, slice_mask=mask, reset_gain_moments=True)
    assert out == {"nsolved": na * sum(mask), "nsingular": 0}
    got, after, y_after = s.get_gain_coeff_moments(), s.get_params(), s.get_gain_coeffs()
    for t, part in enumerate(rows):
        for k in ("ym_r", "ym_i", "yv_r", "yv_i"):
            np.testing.assert_array_equal(got[k][part], (fresh if mask[t] else moved)[k][part], err_msg=f"{k} of slice {t}")
        planes = ((after[0], before[0], want_g.real), (after[1], before[1], want_g.imag), (y_after[0], y_before[0], want_y.real),
                  (y_after[1], y_before[1], want_y.imag))
        for k, (new, old, ref) in enumerate(planes):
            if mask[t]:
                err = plane_err(new[part], ref[part])
                print(f"{label}: slice {t} plane {k} {err:.2e}")
                assert err <= TOL[np.dtype(dtype)]["plane"] and not np.array_equal(new[part], old[part])
            else:
                np.testing.assert_array_equal(new[part], old[part], err_msg=f"plane {k} of slice {t}")
    for k in ("cm_r", "cm_i", "cv_r", "cv_i", "t"):
        np.testing.assert_array_equal(got[k], moved[k], err_msg=k)
    assert np.all(got["t"] == 4)
    np.testing.assert_array_equal(after[2], before[2])
    np.testing.assert_array_equal(after[3], before[3])
    assert len(s.run_slices(2, tol=0.0)[1][0]) == 2  # and the fit goes on
    with pytest.raises(ValueError):
        s.solve_gain_coeffs(1, slice_mask=[1, 0])
    s.close()


@pytest.mark.parametrize("config", ["graph", "kernels"])
def test_a_run_continued_after_an_all_zero_mask_is_bit_identical(config):
    p, params = edge_problem(12, 129)
    B = dpss_basis(p.nfreqs)
    losses, final = {}, {}
    for with_call in (False, True):
        s = basis_solver(p, params, np.float32, B)
        s.set_launch_mode(config)
        s.set_optimizer("Adam", learning_rate=1e-2)
        first = s.run(20, tol=0.0)[0]
        if with_call:
            assert s.solve_gain_coeffs(3, slice_mask=[0], reset_gain_moments=True) == {"nsolved": 0, "nsingular": 0}
        second = s.run(20, tol=0.0)[0]
        losses[with_call] = np.concatenate([first, second])
        final[with_call] = s.get_params() + s.get_gain_coeffs()
        s.close()
    assert len(losses[True]) == 40
    np.testing.assert_array_equal(losses[True], losses[False])
    for a, b in zip(final[True], final[False]):
        np.testing.assert_array_equal(a, b)


# ---- other problem shapes
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", ["stream", "shared"])
def test_one_sweep_on_a_fitting_group_of_several_baselines(layout, dtype):
    p0, _, start0 = synthetic.make_problem(7, 200, f0=150e6, df=400e3, seed=13)
    p, start = synthetic.add_redundant_group(p0, start0, np.random.default_rng(1), nred=3)
    assert np.diff(p.grp_bl_start).max() == 3
    params = perturbed(p, start, seed=14)
    B = dpss_basis(p.nfreqs)
    s = basis_solver(p, params, dtype, B, layout)
    assert s.solve_gain_coeffs(1) == {"nsolved": p.nants, "nsingular": 0}
    check(s, *restated_basis(p, params, dtype, B)[:2], dtype, f"redundant group {layout} {np.dtype(dtype).name}")
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_an_autocorrelation_row_changes_nothing(dtype):
    """The problem with an autocorrelation of antenna 2 appended gives the bits of the problem without it."""
    p0, params0 = edge_problem(5, 48)
    rng = np.random.default_rng(9)
    nv = p0.basis[0].shape[1]
    w_auto = np.full((1, p0.nfreqs), p0.wgts.max())
    p = FitProblem(nants=p0.nants, nfreqs=p0.nfreqs, basis=p0.basis, grp_basis=np.concatenate([p0.grp_basis, [0]]).astype(np.int32),
                   grp_bl_start=np.arange(p0.nbls + 2, dtype=np.int32), bl_ant0=np.concatenate([p0.bl_ant0, [2]]).astype(np.int32),
                   bl_ant1=np.concatenate([p0.bl_ant1, [2]]).astype(np.int32), bl_rowblk=np.zeros(p0.nbls + 1, dtype=np.int32),
                   data_r=np.concatenate([p0.data_r, rng.standard_normal((1, p0.nfreqs))]),
                   data_i=np.concatenate([p0.data_i, rng.standard_normal((1, p0.nfreqs))]), wgts=np.concatenate([p0.wgts, w_auto]))
    p.validate()
    params = dict(params0, c_r=np.concatenate([params0["c_r"], rng.standard_normal(nv)]), c_i=np.concatenate([params0["c_i"], rng.standard_normal(nv)]))
    B = dpss_basis(p.nfreqs)
    s, s0 = basis_solver(p, params, dtype, B), basis_solver(p0, params0, dtype, B)
    s.solve_gain_coeffs(2)
    s0.solve_gain_coeffs(2)
    check(s, *restated_basis(p, params, dtype, B, nsweeps=2)[:2], dtype, f"autocorrelation {np.dtype(dtype).name}")
    for a, b in zip(s.get_params()[:2] + s.get_gain_coeffs(), s0.get_params()[:2] + s0.get_gain_coeffs()):
        np.testing.assert_array_equal(a, b)
    s.close()
    s0.close()


# ---- error codes
def test_wrong_arguments_and_wrong_state_are_reported():
    from calamity_amd.solver import HipFitSolver

    p, params = edge_problem(5, 48)
    B = dpss_basis(p.nfreqs)
    s = solver_of(p, params, np.float64)
    with pytest.raises(_lib.CalamityHipError) as err:  # no basis attached
        s.solve_gain_coeffs(1)
    assert err.value.code == _lib.CAL_ERR_STATE and "basis" in str(err.value)
    s.set_gain_basis(B)
    bad = (dict(nsweeps=0), dict(nsweeps=1, damping=0.0), dict(nsweeps=1, damping=1.5), dict(nsweeps=1, ridge=-1e-6), dict(nsweeps=1, ridge=float("nan")),
           dict(nsweeps=1, ridge=float("inf")))
    for kw in bad:
        with pytest.raises(_lib.CalamityHipError) as err:
            s.solve_gain_coeffs(**kw)
        assert err.value.code == _lib.CAL_ERR_INVALID, kw
    with pytest.raises(_lib.CalamityHipError) as err:  # no optimizer
        s.solve_gain_coeffs(1, reset_gain_moments=True)
    assert err.value.code == _lib.CAL_ERR_STATE
    s.solve_gain_coeffs(1, damping=1.0, ridge=0.0)  # the closed ends
    with pytest.raises(_lib.CalamityHipError) as err:  # the per-channel call still refuses, and points here
        s.solve_gains(1)
    assert err.value.code == _lib.CAL_ERR_UNSUPPORTED and "basis" in str(err.value) and "cal_solver_solve_gain_coeffs" in str(err.value)
    s.close()
    # a time basis attached, with and without a frequency basis
    T = 2
    parts = [synthetic.make_problem(5, 48, f0=150e6, df=400e3, seed=21, data_seed=30 + t) for t in range(T)]
    from calamity_amd import distributed as D

    joint, jstart = D.batch_time_slices([(pt[0], pt[2]) for pt in parts], per_slice=False)
    for with_freq in (True, False):
        s = HipFitSolver(dtype=np.float64)
        s.set_problem(joint)
        s.set_params(jstart["g_r"], jstart["g_i"], jstart["c_r"], jstart["c_i"])
        if with_freq:
            s.set_gain_basis(B)
        s.set_gain_time_basis(np.ones((T, 1)) / np.sqrt(T))
        with pytest.raises(_lib.CalamityHipError) as err:
            s.solve_gain_coeffs(1)
        assert err.value.code == _lib.CAL_ERR_UNSUPPORTED and "time basis" in str(err.value)
        s.close()
    # no gains
    shell = copy.copy(p)
    shell.data_r = shell.data_i = shell.wgts = None
    s = HipFitSolver(dtype=np.float64)
    s.set_problem(shell)
    with pytest.raises(_lib.CalamityHipError) as err:  # no data
        s.solve_gain_coeffs(1)
    assert err.value.code == _lib.CAL_ERR_STATE
    s.set_data(p.data_r, p.data_i, p.wgts)
    s.set_params(c_r=params["c_r"], c_i=params["c_i"])
    with pytest.raises(_lib.CalamityHipError) as err:
        s.solve_gain_coeffs(1)
    assert err.value.code == _lib.CAL_ERR_STATE
    s.close()
