"""cal_solver_solve_gain_time_coeffs on the device against the fp64 NumPy restatement of tests/test_gain_time_solve_host.py: damped StefCal
sweeps taken jointly over the times of a fit with a gain time basis, g = g0 + Bt (x) B y.

Tolerances are the project's own (``TOL`` of tests/test_gpu_fit_quality.py): fp64 1e-10, fp32 1e-4 of the plane's largest element, on
the real and imaginary planes of the new gains and of y; losses fp64 1e-10, fp32 1e-5.  A CPU emulation of an fp32 Gram in BLAS order with
the solve in fp64 stays at or under 2.8e-6 on the shapes used here (cond(N_a + ridge) <= 5e2), which leaves a factor of 35 under the fp32
bound for the 2 ... 3 x that sequential device sums cost.

What the shapes pin ((T, Na, F); L, K, n = L K): (4, 5, 48) 3, 10, 30: kpad != K, one partial tile; (6, 7, 40) 5, 9, 45; (9, 6, 64) 6, 12,
72: n past one 64-block; (7, 5, 48) 6, 12, 72; (15, 4, 40) 14, 9, 126: the factor in LDS, two tiles of time vectors; (2, 4, 200) 1, 127,
127: the last n in LDS; (9, 4, 40) 8, 16, 128: the first n in scratch; (14, 4, 40) 13, 20, 260: past 256, T and L no multiples of 8.
Without a frequency basis: L = 1, 2, 3 and 8 in registers (L = 1 and 2 cut the unrolled loops at their first and second trip), L = 9 in
scratch.  In every problem the last antenna is flagged wholly (the singular
system), antenna 2 at time 0 (it is solved and moves there) and channel 3 of antenna 1 (it moves with a frequency basis only)."""
import functools

import numpy as np
import pytest

from calamity_amd import _lib, modeling
from test_gain_time_basis_host import joint_case
from test_gain_time_solve_host import SHAPES, TIME_ONLY_SHAPES, bases_of, flagged_case, rand_basis, restated_time
from test_gpu_fit_quality import TOL, plane_err, solver_of

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
CASES = SHAPES + [(s, ("rand",), (L, None)) for s, L in TIME_ONLY_SHAPES]


def time_solver(p, params, dtype, Bt, B=None, layout="shared"):
    s = solver_of(p, params, dtype, layout)
    if B is not None:
        s.set_gain_basis(B)
    s.set_gain_time_basis(Bt)  # g0 = the gains just set, y = 0
    return s


@functools.lru_cache(maxsize=None)
def reference(shape, kind, LK, dtype_name, nsweeps):
    p, params = flagged_case(*shape)
    Bt, B = bases_of(shape, kind, LK)
    return restated_time(p, params, np.dtype(dtype_name).type, Bt, B, nsweeps=nsweeps)


def state(s):
    return s.get_params()[:2] + s.get_gain_coeffs()


def check(s, want_g, want_y, dtype, label):
    g_r, g_i, y_r, y_i = state(s)
    errs = (plane_err(g_r, want_g.real), plane_err(g_i, want_g.imag), plane_err(y_r, want_y.real), plane_err(y_i, want_y.imag))
    print(f"{label}: g_r {errs[0]:.2e}  g_i {errs[1]:.2e}  y_r {errs[2]:.2e}  y_i {errs[3]:.2e}")
    for a in (g_r, g_i, y_r, y_i):
        assert np.all(np.isfinite(a)), label
    assert max(errs) <= TOL[np.dtype(dtype)]["plane"], (label, errs)
    return g_r, g_i, y_r, y_i


# ---- parity after one and after three sweeps
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,kind,LK", CASES)
def test_one_and_three_sweeps_equal_the_numpy_restatement(shape, kind, LK, dtype):
    T, na, F = shape
    p, params = flagged_case(*shape)
    Bt, B = bases_of(shape, kind, LK)
    counts = {"nsolved": na - 1, "nsingular": 1} if B is not None else {"nsolved": (na - 1) * F - 1, "nsingular": F + 1}
    s = time_solver(p, params, dtype, Bt, B)
    before = s.get_params()
    tol = TOL[np.dtype(dtype)]["loss"]
    for nsweeps, call in ((1, 1), (3, 2)):
        out = s.solve_gain_time_coeffs(call)
        want_g, want_y, chisq, den, nsing = reference(shape, kind, LK, np.dtype(dtype).name, nsweeps)
        g_r, g_i, y_r, y_i = check(s, want_g, want_y, dtype, f"{shape} L, K = {LK} {np.dtype(dtype).name} after {nsweeps}")
        loss = s.eval_loss()
        print(f"    chi-square {loss:.10e}, restatement {chisq[-1]:.10e}: {abs(loss - chisq[-1]) / chisq[-1]:.2e}")
        assert abs(loss - chisq[-1]) <= tol * chisq[-1]
        assert out == counts and nsing == counts["nsingular"]
        # the antenna without data is the singular system: the bits it had
        assert not np.any(den[na - 1 :: na]) and not np.any(y_r[na - 1]) and not np.any(y_i[na - 1])
        np.testing.assert_array_equal(g_r[na - 1 :: na], before[0][na - 1 :: na])
        np.testing.assert_array_equal(g_i[na - 1 :: na], before[1][na - 1 :: na])
        # antenna 2 has no data at time 0 and moves there: the time basis interpolates
        assert not np.any(den[2]) and np.mean(g_r[2] != before[0][2]) > 0.9 and np.mean(g_i[2] != before[1][2]) > 0.9
        # channel 3 of antenna 1 has no data at any time
        assert not np.any(den[1::na, 3])
        if B is not None:
            assert np.any(g_r[1::na, 3] != before[0][1::na, 3]) and np.any(g_i[1::na, 3] != before[1][1::na, 3])
        else:
            np.testing.assert_array_equal(g_r[1::na, 3], before[0][1::na, 3])
            np.testing.assert_array_equal(g_i[1::na, 3], before[1][1::na, 3])
            assert not np.any(y_r[1, :, 3]) and not np.any(y_i[1, :, 3])
        # every other antenna moved at every time, coefficients are not touched
        assert all(np.any(g_r[r] != before[0][r]) for r in range(T * na) if r % na != na - 1)
    after = s.get_params()
    np.testing.assert_array_equal(after[2], before[2])
    np.testing.assert_array_equal(after[3], before[3])
    s.close()


# ---- the reductions
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [10, 130])
def test_one_time_gives_the_bits_of_the_frequency_basis_sweep(K, dtype):
    p, params = flagged_case(1, 6, 200)
    B = rand_basis(p.nfreqs, K, 2)
    s = time_solver(p, params, dtype, np.ones((1, 1)), B)
    twin = solver_of(p, params, dtype)
    twin.set_gain_basis(B)
    assert s.solve_gain_time_coeffs(2, ridge=1e-3) == twin.solve_gain_coeffs(2, ridge=1e-3) == {"nsolved": 4, "nsingular": 2}  # (antenna 2 is flagged at the one time there is)
    y, y_twin = s.get_gain_coeffs(), twin.get_gain_coeffs()
    assert np.any(y[0]) and y[0].shape == (6, 1, K)
    for a, b in zip(s.get_params()[:2] + (y[0][:, 0], y[1][:, 0]), twin.get_params()[:2] + y_twin):
        np.testing.assert_array_equal(a, b)
    s.close()
    twin.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_an_identity_time_basis_without_ridge_agrees_with_the_sweep_per_time(dtype):
    big, start = joint_case()[:2]  # 3 times of 7 antennas x 40 channels, nothing flagged
    T, na = 3, big.nants // 3
    B = np.array(modeling.gain_dpss_basis(150e6 + 400e3 * np.arange(big.nfreqs), 100.0))
    s = time_solver(big, start, dtype, np.eye(T), B)
    twin = solver_of(big, start, dtype)
    twin.set_gain_basis(B)
    assert s.solve_gain_time_coeffs(2, ridge=0.0) == {"nsolved": na, "nsingular": 0}
    assert twin.solve_gain_coeffs(2, ridge=0.0) == {"nsolved": T * na, "nsingular": 0}
    y, y_twin = s.get_gain_coeffs(), twin.get_gain_coeffs()
    pairs = list(zip(s.get_params()[:2], twin.get_params()[:2])) + [(y[k].transpose(1, 0, 2).reshape(T * na, -1), y_twin[k]) for k in range(2)]
    for k, (a, b) in enumerate(pairs):
        err = plane_err(a, b)
        print(f"identity time basis {np.dtype(dtype).name} plane {k}: {err:.2e}")
        assert err <= TOL[np.dtype(dtype)]["plane"]
    s.close()
    twin.close()


# ---- chunks, repeats
CHUNKED = [CASES[3], CASES[6], CASES[7], CASES[10]]  # n = 72, 128, 260 and the time-only L = 9


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,kind,LK", CHUNKED)
def test_one_antenna_chunks_and_a_second_solver_give_the_same_bits(shape, kind, LK, dtype):
    p, params = flagged_case(*shape)
    Bt, B = bases_of(shape, kind, LK)
    got = []
    for bound in (0, 1, 0):
        s = time_solver(p, params, dtype, Bt, B)
        s._set_coeff_solve_scratch(bound)
        s.solve_gain_time_coeffs(2)
        got.append(state(s))
        s.close()
    assert np.any(got[0][2])
    for other in got[1:]:
        for a, b in zip(got[0], other):
            np.testing.assert_array_equal(a, b)


# ---- moments, the continued run
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_freq", [True, False])
@pytest.mark.parametrize("optimizer", ["Adam", "Adagrad"])
def test_reset_gain_moments_restores_the_y_slots_only(optimizer, with_freq, dtype):
    shape, kind, LK = CASES[0]
    p, params = flagged_case(*shape)
    Bt, B = bases_of(shape, kind, LK)
    s = time_solver(p, params, dtype, Bt, B if with_freq else None)
    s.set_optimizer(optimizer, learning_rate=1e-2)
    fresh = s.get_gain_coeff_moments()
    if optimizer == "Adagrad":
        assert np.all(fresh["yv_r"] == dtype(0.1)) and np.all(fresh["yv_i"] == dtype(0.1)) and not np.any(fresh["ym_r"])
    s.run(4, tol=0.0)
    moved, before = s.get_gain_coeff_moments(), s.get_params()
    assert np.any(moved["yv_r"] != fresh["yv_r"]) and np.any(moved["yv_i"] != fresh["yv_i"])
    s.solve_gain_time_coeffs(1)  # without the flag the slots stay
    kept = s.get_gain_coeff_moments()
    for k in moved:
        np.testing.assert_array_equal(kept[k], moved[k], err_msg=k)
    s.solve_gain_time_coeffs(2, reset_gain_moments=True)
    got, after = s.get_gain_coeff_moments(), s.get_params()
    for k in ("ym_r", "ym_i", "yv_r", "yv_i"):
        np.testing.assert_array_equal(got[k], fresh[k], err_msg=k)
    for k in ("cm_r", "cm_i", "cv_r", "cv_i", "t"):
        np.testing.assert_array_equal(got[k], moved[k], err_msg=k)
    assert np.all(got["t"] == 4) and np.any(after[0] != before[0])
    np.testing.assert_array_equal(after[2], before[2])
    np.testing.assert_array_equal(after[3], before[3])
    assert len(s.run(2, tol=0.0)[0]) == 2  # and the fit goes on
    s.close()


def test_a_run_continued_after_the_call_is_the_same_in_graph_form_and_kernel_by_kernel():
    """The loop state is put back around the model pass: the second run records its 20 losses, the first of them the chi-square at the
    new y, and a replayed graph and single launches agree bit for bit across the call."""
    shape, kind, LK = CASES[1]
    p, params = flagged_case(*shape)
    Bt, B = bases_of(shape, kind, LK)
    losses, final = {}, {}
    for config in ("graph", "kernels"):
        s = time_solver(p, params, np.float32, Bt, B)
        s.set_launch_mode(config)
        s.set_optimizer("Adam", learning_rate=1e-2)
        first = s.run(20, tol=0.0)[0]
        s.solve_gain_time_coeffs(3, reset_gain_moments=True)
        at_new_y = s.eval_loss()
        second = s.run(20, tol=0.0)[0]
        assert len(first) == len(second) == 20 and abs(second[0] - at_new_y) <= 1e-5 * at_new_y
        losses[config] = np.concatenate([first, second])
        final[config] = s.get_params() + s.get_gain_coeffs()
        s.close()
    np.testing.assert_array_equal(losses["graph"], losses["kernels"])
    for a, b in zip(final["graph"], final["kernels"]):
        np.testing.assert_array_equal(a, b)


# ---- error codes, memory
def test_wrong_arguments_and_wrong_state_are_reported_and_the_scratch_is_counted():
    shape, kind, LK = CASES[0]
    p, params = flagged_case(*shape)
    Bt, B = bases_of(shape, kind, LK)
    s = solver_of(p, params, np.float64)
    for attach in (lambda: None, lambda: s.set_gain_basis(B)):  # no time basis attached
        attach()
        with pytest.raises(_lib.CalamityHipError) as err:
            s.solve_gain_time_coeffs(1)
        assert err.value.code == _lib.CAL_ERR_STATE and "time basis" in str(err.value)
    s.set_gain_time_basis(Bt)
    bad = (dict(nsweeps=0), dict(nsweeps=1, damping=0.0), dict(nsweeps=1, damping=1.5), dict(nsweeps=1, ridge=-1e-6), dict(nsweeps=1, ridge=float("nan")),
           dict(nsweeps=1, ridge=float("inf")))
    for kw in bad:
        with pytest.raises(_lib.CalamityHipError) as err:
            s.solve_gain_time_coeffs(**kw)
        assert err.value.code == _lib.CAL_ERR_INVALID, kw
    with pytest.raises(_lib.CalamityHipError) as err:  # no optimizer
        s.solve_gain_time_coeffs(1, reset_gain_moments=True)
    assert err.value.code == _lib.CAL_ERR_STATE
    # the refusals beside it hold
    with pytest.raises(_lib.CalamityHipError) as err:
        s.solve_gain_coeffs(1)
    assert err.value.code == _lib.CAL_ERR_UNSUPPORTED and "time basis" in str(err.value)
    with pytest.raises(_lib.CalamityHipError) as err:
        s.solve_gains(1)
    assert err.value.code == _lib.CAL_ERR_UNSUPPORTED and "basis" in str(err.value)
    # the scratch is counted, and released by a new bound, by either basis setter and sized again by the next call
    s.solve_gain_time_coeffs(1, damping=1.0, ridge=0.0)  # the closed ends
    held = s.memory_bytes()
    s._set_coeff_solve_scratch(0)
    freed = s.memory_bytes()
    assert freed < held
    s.solve_gain_time_coeffs(1)
    assert s.memory_bytes() == held
    s.set_gain_time_basis(Bt)
    assert s.memory_bytes() == freed
    s.solve_gain_time_coeffs(1)
    assert s.memory_bytes() == held
    s.set_gain_basis(B)
    assert s.memory_bytes() == freed
    s.close()
