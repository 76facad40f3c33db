"""cal_solver_gain_basis_errors on the device against the fp64 NumPy restatement of tests/gain_basis_errors_ref.py: the error bars of gains
confined to a frequency basis, a time x frequency basis and a time basis alone.

Tolerances are the project's own (``TOL`` of tests/test_gpu_fit_quality.py): fp64 1e-10, fp32 1e-4 of the plane's largest element on
``gain_var`` and ``y_var``; ``gain_dof`` takes the scalar bound (fp64 1e-10, fp32 1e-5, relative).  A CPU emulation of the fp32 arithmetic
(Gram and W rounded to fp32, the factor in fp64, the product W X in fp32; tests/test_gain_basis_errors_host.py runs it on every shape
used here) stays under a third of the fp32 bound: at worst gain_var 1.5e-5 and y_var 2.5e-5, both on (9, 4, 40) L, K = 8, 16
(cond(N_r) = 3.7e2); 6.9e-6 / 6.7e-6 on (6, 7, 40) 5, 9 (cond 2.8e2); 3.5e-6 / 1.1e-5 on (9, 6, 64) 6, 12 (cond 5.1e2); every frequency
width stays at or under 1.1e-6 / 3.5e-6 (K = 130, cond 62).

What the shapes pin.  Frequency widths K = 1, 12, 33, 65, 130 on (Na, F) = (7, 200), (12, 129), (5, 48), ``flagged_case`` at one time:
kpad != K, W past one 64-row block, a band past one 64-channel piece, nfreqs no multiple of 64; antenna 2 (flagged at the one time) and
the last antenna are the singular rows.  Time x frequency: ``SHAPES`` of tests/test_gain_time_solve_host.py, n = L K = 30, 45, 72, 72, 126,
127 (the last factor in LDS), 128 (the first in scratch), 260 (past 256; T and L no multiples of 8).  Time alone: L = 1, 2, 3, 8 in
registers, 9 in scratch.  In every problem the last antenna is flagged wholly (zeros, singular), antenna 2 at time 0 (a positive
variance there under a time basis) and channel 3 of antenna 1 (a positive variance under a frequency basis)."""
import ctypes as C
import functools

import numpy as np
import pytest

from calamity_amd import _lib
from gain_basis_errors_ref import den_of, restated_errors
from test_gain_basis_errors_host import FREQ_WIDTHS, freq_case
from test_gain_time_basis_host import joint_case
from test_gain_time_solve_host import SHAPES, TIME_ONLY_SHAPES, bases_of, flagged_case, rand_basis
from test_gpu_fit_quality import TOL, plane_err, solver_of

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
TIME_CASES = SHAPES + [(s, ("rand",), (L, None)) for s, L in TIME_ONLY_SHAPES]
KEYS = ("gain_var", "y_var", "gain_dof")


def basis_solver(p, params, dtype, Bt=None, B=None, layout="shared"):
    s = solver_of(p, params, dtype, layout)
    if B is not None:
        s.set_gain_basis(B)
    if Bt is not None:
        s.set_gain_time_basis(Bt)
    return s


@functools.lru_cache(maxsize=None)
def freq_reference(shape, K, dtype_name, ridge=1e-6):
    p, params = freq_case(shape)
    return restated_errors(p, params, np.dtype(dtype_name).type, None, rand_basis(shape[1], K, 2), ridge)


@functools.lru_cache(maxsize=None)
def time_reference(shape, kind, LK, dtype_name, ridge=1e-6):
    p, params = flagged_case(*shape)
    Bt, B = bases_of(shape, kind, LK)
    return restated_errors(p, params, np.dtype(dtype_name).type, Bt, B, ridge)


def check(out, want, dtype, label):
    tol = TOL[np.dtype(dtype)]
    errs = (plane_err(out["gain_var"], want["gain_var"]), plane_err(out["y_var"], want["y_var"].reshape(out["y_var"].shape)),
            float(np.max(np.abs(out["gain_dof"] - want["gain_dof"]) / np.maximum(np.abs(want["gain_dof"]), 1e-300))))
    print(f"{label}: gain_var {errs[0]:.2e}  y_var {errs[1]:.2e}  gain_dof {errs[2]:.2e}")
    for k in KEYS:
        assert out[k].dtype == np.float64 and np.all(np.isfinite(out[k])) and np.all(out[k] >= 0), (label, k)
    assert (out["nsolved"], out["nsingular"]) == (want["nsolved"], want["nsingular"]), label
    assert errs[0] <= tol["plane"] and errs[1] <= tol["plane"] and errs[2] <= tol["loss"], (label, errs)
    # a singular system keeps zeros, nothing else does
    np.testing.assert_array_equal(out["gain_var"] == 0, want["gain_var"] == 0)
    np.testing.assert_array_equal(out["y_var"] == 0, want["y_var"].reshape(out["y_var"].shape) == 0)
    np.testing.assert_array_equal(out["gain_dof"] == 0, want["gain_dof"] == 0)


def same_bits(a, b):
    for k in KEYS + ("nsolved", "nsingular"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


# ---- parity
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,K", FREQ_WIDTHS)
def test_frequency_widths_equal_the_numpy_restatement(shape, K, dtype):
    p, params = freq_case(shape)
    na = shape[0]
    s = basis_solver(p, params, dtype, None, rand_basis(shape[1], K, 2))
    out = s.gain_basis_errors()
    s.close()
    assert out["gain_var"].shape == (na, shape[1]) and out["y_var"].shape == (na, K) and out["gain_dof"].shape == (na,)
    check(out, freq_reference(shape, K, np.dtype(dtype).name), dtype, f"{shape} K = {K} {np.dtype(dtype).name}")
    assert (out["nsolved"], out["nsingular"]) == (na - 2, 2)
    for a in (2, na - 1):  # no unflagged cross-correlation: zeros
        assert not np.any(out["gain_var"][a]) and not np.any(out["y_var"][a]) and out["gain_dof"][a] == 0
    assert out["gain_var"][1, 3] > 0  # the basis interpolates across the flagged channel
    assert np.all(out["gain_var"][[a for a in range(na) if a not in (2, na - 1)]] > 0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,kind,LK", TIME_CASES)
def test_time_bases_equal_the_numpy_restatement(shape, kind, LK, dtype):
    T, na, F = shape
    p, params = flagged_case(*shape)
    Bt, B = bases_of(shape, kind, LK)
    s = basis_solver(p, params, dtype, Bt, B)
    out = s.gain_basis_errors()
    s.close()
    L = Bt.shape[1]
    assert out["gain_var"].shape == (T * na, F) and out["y_var"].shape == (na, L, F if B is None else B.shape[1]) and out["gain_dof"].shape == (na,)
    check(out, time_reference(shape, kind, LK, np.dtype(dtype).name), dtype, f"{shape} L, K = {LK} {np.dtype(dtype).name}")
    counts = (na - 1, 1) if B is not None else ((na - 1) * F - 1, F + 1)
    assert (out["nsolved"], out["nsingular"]) == counts
    # the antenna without data at any time: zeros; antenna 2 has none at time 0 and a positive variance there
    assert not np.any(out["gain_var"][na - 1 :: na]) and not np.any(out["y_var"][na - 1]) and out["gain_dof"][na - 1] == 0
    assert np.all(out["gain_var"][2] > 0)
    # channel 3 of antenna 1 has no data at any time
    if B is not None:
        assert np.all(out["gain_var"][1::na, 3] > 0)
    else:
        assert not np.any(out["gain_var"][1::na, 3]) and not np.any(out["y_var"][1, :, 3])


@pytest.mark.parametrize("dtype", DTYPES)
def test_both_layouts_give_the_same_planes(dtype):
    shape, kind, LK = SHAPES[2]
    p, params = flagged_case(*shape)
    Bt, B = bases_of(shape, kind, LK)
    want = time_reference(shape, kind, LK, np.dtype(dtype).name)
    for layout in ("stream", "shared"):
        s = basis_solver(p, params, dtype, Bt, B, layout)
        check(s.gain_basis_errors(), want, dtype, f"{shape} {layout} {np.dtype(dtype).name}")
        s.close()


# ---- identities at ridge = 0 on the device (bounds of the leverage sums of fit_errors: fp32 1e-5, fp64 1e-12)
@pytest.mark.parametrize("dtype", DTYPES)
def test_without_ridge_den_gain_var_adds_up_to_the_unknowns(dtype):
    bound = 1e-5 if dtype == np.float32 else 1e-12
    # frequency basis: K per antenna
    shape, K = (7, 200), 12
    p, params = freq_case(shape)
    s = basis_solver(p, params, dtype, None, rand_basis(shape[1], K, 2))
    out = s.gain_basis_errors(ridge=0.0)
    s.close()
    den, solved = den_of(p, params, dtype), [0, 1, 3, 4, 5]
    err = np.max(np.abs(np.sum(den * out["gain_var"], axis=1)[solved] / K - 1.0))
    print(f"frequency basis {np.dtype(dtype).name}: {err:.2e}")
    assert err <= bound
    np.testing.assert_array_equal(out["gain_dof"][solved], float(K))
    # time x frequency: L K per antenna
    shape, kind, LK = SHAPES[0]
    T, na, F = shape
    p, params = flagged_case(*shape)
    Bt, B = bases_of(shape, kind, LK)
    s = basis_solver(p, params, dtype, Bt, B)
    out = s.gain_basis_errors(ridge=0.0)
    s.close()
    n = Bt.shape[1] * B.shape[1]
    total = np.sum((den_of(p, params, dtype) * out["gain_var"]).reshape(T, na, F), axis=(0, 2))
    err = np.max(np.abs(total[: na - 1] / n - 1.0))
    print(f"time x frequency {np.dtype(dtype).name}: {err:.2e}")
    assert err <= bound and total[na - 1] == 0
    np.testing.assert_array_equal(out["gain_dof"], [n] * (na - 1) + [0])
    # time basis alone: L per solved (antenna, channel)
    shape, L = TIME_ONLY_SHAPES[0]
    T, na, F = shape
    p, params = flagged_case(*shape)
    Bt = bases_of(shape, ("rand",), (L, None))[0]
    s = basis_solver(p, params, dtype, Bt)
    out = s.gain_basis_errors(ridge=0.0)
    s.close()
    per = np.sum((den_of(p, params, dtype) * out["gain_var"]).reshape(T, na, F), axis=0)
    solved = np.any(out["gain_var"].reshape(T, na, F) != 0, axis=0)
    err = np.max(np.abs(per[solved] / L - 1.0))
    print(f"time basis alone {np.dtype(dtype).name}: {err:.2e}")
    assert err <= bound and solved.sum() == out["nsolved"] == (na - 1) * F - 1
    np.testing.assert_array_equal(out["gain_dof"], L * solved.sum(axis=1))


# ---- limits
@pytest.mark.parametrize("dtype", DTYPES)
def test_an_identity_basis_gives_gain_var_of_fit_errors(dtype):
    p, params = joint_case(ntimes=1, nants=6, nfreqs=24)[:2]  # nothing flagged
    twin = solver_of(p, params, dtype)
    want = twin.fit_errors(model_var=False, coeffs=False)["gain_var"]
    twin.close()
    s = basis_solver(p, params, dtype, None, np.eye(24))
    out = s.gain_basis_errors(ridge=0.0)
    s.close()
    errs = plane_err(out["gain_var"], want), plane_err(out["y_var"], want)
    print(f"identity basis {np.dtype(dtype).name}: gain_var {errs[0]:.2e}, y_var {errs[1]:.2e}")
    assert np.all(want > 0) and max(errs) <= TOL[np.dtype(dtype)]["plane"] and (out["nsolved"], out["nsingular"]) == (6, 0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [10, 130])
def test_one_time_gives_the_bits_of_the_frequency_basis_call(K, dtype):
    p, params = flagged_case(1, 6, 200)
    B = rand_basis(p.nfreqs, K, 2)
    s, twin = basis_solver(p, params, dtype, np.ones((1, 1)), B), basis_solver(p, params, dtype, None, B)
    a, b = s.gain_basis_errors(ridge=1e-3), twin.gain_basis_errors(ridge=1e-3)
    s.close()
    twin.close()
    assert a["y_var"].shape == (6, 1, K) and np.any(a["gain_var"]) and (a["nsolved"], a["nsingular"]) == (4, 2)
    same_bits(dict(a, y_var=a["y_var"][:, 0]), b)


# ---- chunks, repeats
CHUNKED = [((7, 200), None, (None, 130)), SHAPES[3], SHAPES[6], SHAPES[7], TIME_CASES[10]]  # K = 130; n = 72, 128, 260; the time-only L = 9


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,kind,LK", CHUNKED)
def test_one_row_chunks_two_calls_and_a_second_solver_give_the_same_bits(shape, kind, LK, dtype):
    if kind is None:
        (p, params), Bt, B = freq_case(shape), None, rand_basis(shape[1], LK[1], 2)
    else:
        p, params = flagged_case(*shape)
        Bt, B = bases_of(shape, kind, LK)
    got = []
    for bound in (0, 1, 0):
        s = basis_solver(p, params, dtype, Bt, B)
        s._set_coeff_solve_scratch(bound)
        got.append(s.gain_basis_errors())
        if bound == 1:
            got.append(s.gain_basis_errors())
        s.close()
    assert np.any(got[0]["gain_var"]) and np.any(got[0]["y_var"])
    for other in got[1:]:
        same_bits(got[0], other)


# ---- the state is untouched
def state_of(s):
    m = s.get_gain_coeff_moments()
    return s.get_params() + s.get_gain_coeffs() + tuple(m[k] for k in sorted(m))


@pytest.mark.parametrize("with_time", [False, True])
def test_a_run_continued_after_the_call_is_bit_identical_in_graph_form_and_kernel_by_kernel(with_time):
    shape, kind, LK = SHAPES[1]
    p, params = flagged_case(*shape)
    Bt, B = bases_of(shape, kind, LK)
    losses, final = {}, {}
    for config in ("graph", "kernels"):
        for call in (False, True):
            s = basis_solver(p, params, np.float32, Bt if with_time else None, B)
            s.set_launch_mode(config)
            s.set_optimizer("Adam", learning_rate=1e-2)
            first = s.run(20, tol=0.0)[0]
            if call:
                before = state_of(s)
                out = s.gain_basis_errors()
                assert np.any(out["gain_var"])
                for a, b in zip(before, state_of(s)):  # y, gains, coefficients and moments keep their bits
                    np.testing.assert_array_equal(a, b)
            second = s.run(20, tol=0.0)[0]
            assert len(first) == len(second) == 20
            losses[config, call] = np.concatenate([first, second])
            final[config, call] = state_of(s)
            s.close()
    for key in (("graph", True), ("kernels", False), ("kernels", True)):
        np.testing.assert_array_equal(losses[key], losses["graph", False])
        for a, b in zip(final[key], final["graph", False]):
            np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("shape,kind,LK", [SHAPES[0], TIME_CASES[8]])
def test_null_outputs_skip_their_work_and_change_nothing_else(shape, kind, LK):
    p, params = flagged_case(*shape)
    Bt, B = bases_of(shape, kind, LK)
    s = basis_solver(p, params, np.float64, Bt, B)
    full = s.gain_basis_errors()
    part = s.gain_basis_errors(y_var=False)
    assert "y_var" not in part
    for k in ("gain_var", "gain_dof", "nsolved", "nsingular"):
        np.testing.assert_array_equal(part[k], full[k], err_msg=k)
    # through the C interface: every output alone, and none at all
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    for key in KEYS + (None,):
        bufs = {k: (np.full_like(full[k], -1.0) if k == key else None) for k in KEYS}
        cnt = _lib.FitErrorsCounts()
        _lib.check(s._lib.cal_solver_gain_basis_errors(s._h, 1e-6, ptr(bufs["gain_var"]), ptr(bufs["y_var"]), ptr(bufs["gain_dof"]), C.byref(cnt)))
        assert (cnt.nsolved, cnt.nsingular) == (full["nsolved"], full["nsingular"])
        if key is not None:
            np.testing.assert_array_equal(bufs[key], full[key], err_msg=key)
    _lib.check(s._lib.cal_solver_gain_basis_errors(s._h, 1e-6, None, None, None, None))
    s.close()


# ---- error codes, memory
def test_wrong_arguments_and_wrong_state_are_reported_and_the_scratch_is_counted():
    from calamity_amd.solver import HipFitSolver

    shape, kind, LK = SHAPES[0]
    p, params = flagged_case(*shape)
    Bt, B = bases_of(shape, kind, LK)
    s = HipFitSolver(dtype=np.float64)
    s.set_problem(p)
    with pytest.raises(_lib.CalamityHipError) as err:  # no parameters yet: as fit_quality reports it
        s.gain_basis_errors()
    assert err.value.code == _lib.CAL_ERR_STATE and "must be set" in str(err.value)
    s.close()
    s = solver_of(p, params, np.float64)
    with pytest.raises(_lib.CalamityHipError) as err:  # no gain basis
        s.gain_basis_errors()
    assert err.value.code == _lib.CAL_ERR_STATE and "cal_solver_fit_errors" in str(err.value)
    s.set_gain_basis(B)
    for ridge in (-1e-6, float("nan"), float("inf")):
        with pytest.raises(_lib.CalamityHipError) as err:
            s.gain_basis_errors(ridge=ridge)
        assert err.value.code == _lib.CAL_ERR_INVALID, ridge
    with pytest.raises(_lib.CalamityHipError) as err:  # the refusal beside it holds
        s.fit_errors()
    assert err.value.code == _lib.CAL_ERR_UNSUPPORTED
    # the scratch is counted, released by a new bound and by a basis setter, and sized again by the next call: under a frequency
    # basis, both bases, and the time basis alone
    for attach in (lambda: None, lambda: s.set_gain_time_basis(Bt), lambda: s.set_gain_basis(None)):
        attach()
        s.gain_basis_errors()
        held = s.memory_bytes()
        s._set_coeff_solve_scratch(0)
        freed = s.memory_bytes()
        assert freed < held
        s.gain_basis_errors()
        assert s.memory_bytes() == held
    s.set_gain_time_basis(Bt)  # (the same basis: y keeps its shape)
    assert s.memory_bytes() == freed
    s.close()
