"""cal_solver_solve_gains on the device against a plain NumPy restatement (include/calamity_hip.h): damped StefCal sweeps.

Baseline b has antennas (i, j); m = A c at the solver's coefficients, d, w its data and weights, g its gains:

    P[b][f] = w d conj(m)                              Q[b][f] = w |m|^2
    role 0 (a == i):  num[a][f] += P g_j               den[a][f] += Q |g_j|^2
    role 1 (a == j):  num[a][f] += conj(P) g_i         den[a][f] += Q |g_i|^2
    g_new[a][f] = (1 - damping) g[a][f] + damping num / den    where den > 0, else unchanged

An autocorrelation row enters neither sum; all antennas are updated from the OLD gains.  The restatement works in fp64 on the
inputs the solver holds (cast to its dtype first).  Tolerances are the project's own (tests/test_gpu_fp32_families.py): fp64
1e-10; fp32 1e-4 of the plane's largest element (the planes here are the real and imaginary parts of the new gains); the loss
tolerances are those of tests/test_gpu_fit_quality.py (fp64 1e-10, fp32 1e-5)."""
import copy
import functools

import numpy as np
import pytest

from calamity_amd import _lib, batched, modeling, synthetic
from calamity_amd.problem import FitProblem
from test_gpu_fit_quality import TOL, edge_problem, perturbed, plane_err, solver_of, wide_problem

pytestmark = pytest.mark.gpu


def model_of(p, params, dtype):
    cast = lambda a: np.asarray(a).astype(dtype).astype(np.float64)  # noqa: E731
    c = cast(params["c_r"]) + 1j * cast(params["c_i"])
    coff = p.grp_coff
    m = np.empty((p.nbls, p.nfreqs), dtype=np.complex128)
    for grp in range(p.ngrps):
        blk = cast(p.basis[p.grp_basis[grp]])
        for b in range(p.grp_bl_start[grp], p.grp_bl_start[grp + 1]):
            m[b] = blk[p.bl_rowblk[b] * p.nfreqs : (p.bl_rowblk[b] + 1) * p.nfreqs] @ c[coff[grp] : coff[grp + 1]]
    return m


def restated(p, params, dtype, nsweeps=1, damping=0.5, data=None):
    """``nsweeps`` sweeps in fp64 arithmetic on inputs rounded to ``dtype``; returns (g, chi-square after every sweep, first den)."""
    cast = lambda a: np.asarray(a).astype(dtype).astype(np.float64)  # noqa: E731
    d_r, d_i, w = (cast(a) for a in (data if data is not None else (p.data_r, p.data_i, p.wgts)))
    d = d_r + 1j * d_i
    g = cast(params["g_r"]) + 1j * cast(params["g_i"])
    m = model_of(p, params, dtype)
    P, Q = w * d * np.conj(m), w * np.abs(m) ** 2
    cross = p.bl_ant0 != p.bl_ant1
    chisq, den0 = [], None
    for _ in range(nsweeps):
        num = np.zeros((p.nants, p.nfreqs), dtype=np.complex128)
        den = np.zeros((p.nants, p.nfreqs))
        for b in np.where(cross)[0]:
            i, j = int(p.bl_ant0[b]), int(p.bl_ant1[b])
            num[i] += P[b] * g[j]
            den[i] += Q[b] * np.abs(g[j]) ** 2
            num[j] += np.conj(P[b]) * g[i]
            den[j] += Q[b] * np.abs(g[i]) ** 2
        den0 = den if den0 is None else den0
        ok = den > 0
        g = np.where(ok, (1.0 - damping) * g + damping * num / np.where(ok, den, 1.0), g)
        chisq.append(float(np.sum(w * np.abs(d - g[p.bl_ant0] * np.conj(g[p.bl_ant1]) * m) ** 2)))
    return g, chisq, den0


def check_gains(s, want, dtype, label):
    g_r, g_i = s.get_params()[:2]
    errs = (plane_err(g_r, want.real), plane_err(g_i, want.imag))
    print(f"{label}: g_r {errs[0]:.2e}  g_i {errs[1]:.2e}")
    assert np.all(np.isfinite(g_r)) and np.all(np.isfinite(g_i)), label
    assert max(errs) <= TOL[np.dtype(dtype)]["plane"], (label, errs)
    return g_r, g_i


# ---- parity of ONE sweep
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("layout", ["stream", "shared"])
@pytest.mark.parametrize("shape", [(5, 48), (7, 200), (12, 129), (6, 300)])
def test_one_sweep_equals_the_numpy_restatement(shape, layout, dtype):
    """(6, 300): more than one channel block of 64 x 4 channels in fp32."""
    p, params = edge_problem(*shape)
    na = p.nants
    s = solver_of(p, params, dtype, layout)
    before = s.get_params()
    s.solve_gains(1)
    want, _, den = restated(p, params, dtype)
    g_r, g_i = check_gains(s, want, dtype, f"{shape} {layout} {np.dtype(dtype).name}")
    # an antenna without baselines, and the channel flagged on every baseline of antenna 1: the bits they had
    assert not np.any(den[na - 1]) and den[1, 3] == 0
    np.testing.assert_array_equal(g_r[na - 1], before[0][na - 1])
    np.testing.assert_array_equal(g_i[na - 1], before[1][na - 1])
    assert g_r[1, 3] == before[0][1, 3] and g_i[1, 3] == before[1][1, 3]
    # an antenna with one baseline (fewer list entries than waves) and everything else moved
    assert np.sum((p.bl_ant0 == na - 2) | (p.bl_ant1 == na - 2)) == 1
    assert np.all(g_r[na - 2][den[na - 2] > 0] != before[0][na - 2][den[na - 2] > 0])
    assert not np.any(p.wgts[0])  # a wholly flagged baseline is among the rows
    # coefficients are not touched
    np.testing.assert_array_equal(s.get_params()[2], before[2])
    s.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_one_sweep_with_more_baselines_per_antenna_than_the_unroll(dtype):
    """39 baselines on every antenna: each wave's segment of the list is longer than its unroll of four."""
    p, params = wide_problem()
    s = solver_of(p, params, dtype)
    s.solve_gains(1)
    check_gains(s, restated(p, params, dtype)[0], dtype, f"(40, 64) {np.dtype(dtype).name}")
    s.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("layout", ["stream", "shared"])
def test_one_sweep_on_a_fitting_group_of_several_baselines(layout, dtype):
    p0, _, start0 = synthetic.make_problem(7, 200, f0=150e6, df=400e3, seed=13)
    p, start = synthetic.add_redundant_group(p0, start0, np.random.default_rng(1), nred=3)
    assert np.diff(p.grp_bl_start).max() == 3
    params = perturbed(p, start, seed=14)
    s = solver_of(p, params, dtype, layout)
    s.solve_gains(1)
    check_gains(s, restated(p, params, dtype)[0], dtype, f"redundant group {layout} {np.dtype(dtype).name}")
    s.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_an_autocorrelation_row_changes_nothing(dtype):
    """The problem with an autocorrelation of antenna 2 appended gives the bits of the problem without it: the row is in neither sum,
    and the antennas' lists (hence the order of every sum) are those of the cross-correlations."""
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
    s, s0 = solver_of(p, params, dtype), solver_of(p0, params0, dtype)
    s.solve_gains(2)
    s0.solve_gains(2)
    check_gains(s, restated(p, params, dtype, nsweeps=2)[0], dtype, f"autocorrelation {np.dtype(dtype).name}")
    for a, b in zip(s.get_params()[:2], s0.get_params()[:2]):
        np.testing.assert_array_equal(a, b)
    s.close()
    s0.close()


# ---- sweep chaining and reproducibility
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_sweeps_chain_and_repeat_bitwise(dtype):
    p, params = edge_problem(7, 200)
    runs = []
    for calls in ([5], [1] * 5, [5]):
        s = solver_of(p, params, dtype, "stream")
        for n in calls:
            s.solve_gains(n)
        runs.append(s.get_params()[:2])
        s.close()
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            np.testing.assert_array_equal(a, b)
    assert not np.array_equal(runs[0][0], np.asarray(params["g_r"], dtype=dtype))


# ---- convergence
@functools.lru_cache(maxsize=None)
def truth_problem(nants, nfreqs):
    p, truth, start = synthetic.make_problem(nants, nfreqs, f0=150e6, df=400e3, seed=nants + nfreqs)
    return p, dict(g_r=start["g_r"], g_i=start["g_i"], c_r=np.ascontiguousarray(truth["c"].real), c_i=np.ascontiguousarray(truth["c"].imag))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", [(7, 200), (12, 129), (40, 64)])
def test_thirty_half_damped_sweeps_converge_monotonically(shape, dtype):
    """Coefficients at the truth, gains from unity.  The restatement gives 3e-5, 2e-7 and 2e-7 of the starting chi-square after 30
    sweeps for these inputs and never rises; the bound of 1e-2 leaves two orders of margin for fp32."""
    p, params = truth_problem(*shape)
    s = solver_of(p, params, dtype)
    losses = [s.eval_loss()]
    for _ in range(30):
        s.solve_gains(1, damping=0.5)
        losses.append(s.eval_loss())
    s.close()
    losses = np.asarray(losses)
    rises = np.diff(losses) / losses[0]
    print(f"{shape} {np.dtype(dtype).name}: chi-square {losses[0]:.3e} -> {losses[10]:.3e} (10) -> {losses[-1]:.3e} (30), ratio {losses[-1] / losses[0]:.2e}, "
          f"largest rise {rises.max():.2e} of the start")
    assert np.all(np.isfinite(losses))
    assert np.all(np.diff(losses) <= TOL[np.dtype(dtype)]["loss"] * losses[:-1])
    assert losses[-1] <= 1e-2 * losses[0]


# ---- slices
@pytest.mark.parametrize("layout", ["stream", "shared"])
def test_a_masked_slice_keeps_its_bits_and_the_other_equals_the_single_solver(layout):
    from calamity_amd.solver import HipFitSolver

    T, dtype = 2, np.float32
    parts = [synthetic.make_problem(7, 200, f0=150e6, df=400e3, seed=21, data_seed=30 + t) for t in range(T)]
    p0 = parts[0][0]
    data = tuple(np.concatenate([getattr(parts[t][0], k) for t in range(T)]) for k in ("data_r", "data_i", "wgts"))
    pars = [perturbed(parts[t][0], parts[t][2], seed=40 + t) for t in range(T)]
    sub, _, _ = batched.replicate_slices(p0, T)
    s = HipFitSolver(dtype=dtype)
    s.set_problem(sub, layout=layout)
    s.set_data(*data)
    s.set_params(*[np.concatenate([pars[t][k] for t in range(T)]) for k in ("g_r", "g_i", "c_r", "c_i")])
    before = s.get_params()
    s.solve_gains(2, slice_mask=[1, 0])
    after = s.get_params()
    na = p0.nants
    for k in (0, 1):
        np.testing.assert_array_equal(after[k][na:], before[k][na:])
    assert not np.array_equal(after[0][:na], before[0][:na])
    one = solver_of(p0, pars[0], dtype, layout)
    one.solve_gains(2)
    g1 = one.get_params()
    bitwise = all(np.array_equal(a, b[: p0.nbls]) for a, b in zip(one.model(), s.model()))
    for k in (0, 1):
        err = plane_err(after[k][:na], g1[k])
        print(f"{layout} plane {k}: model pass bitwise {bitwise}, error {err:.2e}")
        if bitwise:
            np.testing.assert_array_equal(after[k][:na], g1[k])
        else:
            assert err <= TOL[np.dtype(dtype)]["plane"]
    with pytest.raises(ValueError):
        s.solve_gains(1, slice_mask=[1, 0, 1])
    one.close()
    s.close()


# ---- run continuation and moments
@pytest.mark.parametrize("config", ["adam", "graph", "kernels"])
def test_a_run_continued_after_an_all_zero_mask_is_bit_identical(config):
    p, params = edge_problem(12, 129)
    losses, final = {}, {}
    for with_call in (False, True):
        s = solver_of(p, params, np.float32)
        s.set_launch_mode({"graph": "graph", "kernels": "kernels"}.get(config, "auto"))
        s.set_optimizer("Adam", learning_rate=1e-2)
        first = s.run(20, tol=0.0)[0]
        if with_call:
            s.solve_gains(3, slice_mask=[0])
        second = s.run(20, tol=0.0)[0]
        losses[with_call] = np.concatenate([first, second])
        final[with_call] = s.get_params()
        s.close()
    assert len(losses[True]) == 40
    np.testing.assert_array_equal(losses[True], losses[False])
    for a, b in zip(final[True], final[False]):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("optimizer", ["Adam", "Adagrad"])
def test_reset_gain_moments_restores_the_slots_of_set_optimizer(optimizer):
    """Adagrad's accumulator starts at 0.1, not 0."""
    p, params = edge_problem(7, 200)
    s = solver_of(p, params, np.float64)
    s.set_optimizer(optimizer, learning_rate=1e-2)
    fresh = s.get_moments()
    s.run(5, tol=0.0)
    moved = s.get_moments()
    assert np.any(moved["gm_r"] != fresh["gm_r"]) or np.any(moved["gv_r"] != fresh["gv_r"])
    s.solve_gains(1)  # without the flag: the slots stay
    kept = s.get_moments()
    for k in fresh:
        np.testing.assert_array_equal(kept[k], moved[k], err_msg=k)
    s.solve_gains(1, reset_gain_moments=True)
    got = s.get_moments()
    for k in ("gm_r", "gm_i", "gv_r", "gv_i"):
        np.testing.assert_array_equal(got[k], fresh[k], err_msg=k)
    for k in ("cm_r", "cm_i", "cv_r", "cv_i", "t"):
        np.testing.assert_array_equal(got[k], moved[k], err_msg=k)
    assert got["t"] == 5
    s.run(2, tol=0.0)  # and the fit goes on
    s.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("mask", [[1, 0, 1], [0, 1, 1]])
@pytest.mark.parametrize("optimizer", ["Adam", "Adagrad"])
def test_a_mask_with_reset_gain_moments_restores_the_selected_slices_only(optimizer, mask, dtype):
    """What the batched driver calls: [1, 0, 1] are two runs of one selected slice, [0, 1, 1] one run of two.  The selected slices are
    swept and their gain slots start over; the other slice keeps gains and slots to the bit; coefficients, their slots and t stay."""
    from calamity_amd.solver import HipFitSolver

    T = 3
    parts = [synthetic.make_problem(7, 200, f0=150e6, df=400e3, seed=21, data_seed=30 + t) for t in range(T)]
    p0 = parts[0][0]
    data = tuple(np.concatenate([getattr(parts[t][0], k) for t in range(T)]) for k in ("data_r", "data_i", "wgts"))
    pars = [perturbed(parts[t][0], parts[t][2], seed=40 + t) for t in range(T)]
    sub, _, _ = batched.replicate_slices(p0, T)
    label = f"{optimizer} mask {mask} {np.dtype(dtype).name}"
    s = HipFitSolver(dtype=dtype)
    s.set_problem(sub, layout="stream")
    s.set_data(*data)
    s.set_params(*[np.concatenate([pars[t][k] for t in range(T)]) for k in ("g_r", "g_i", "c_r", "c_i")])
    s.set_optimizer(optimizer, learning_rate=1e-2)
    fresh = s.get_moments()
    if optimizer == "Adagrad":
        assert np.all(fresh["gv_r"] == dtype(0.1)) and np.all(fresh["gv_i"] == dtype(0.1)) and not np.any(fresh["gm_r"])
    s.run_slices(4, tol=0.0)
    moved, before = s.get_moments(), s.get_params()
    na = p0.nants
    rows = [slice(t * na, (t + 1) * na) for t in range(T)]
    for part in rows:
        assert np.any(moved["gv_r"][part] != fresh["gv_r"][part]) and np.any(moved["gv_i"][part] != fresh["gv_i"][part])
    want = restated(sub, dict(zip(("g_r", "g_i", "c_r", "c_i"), before)), dtype, nsweeps=2, data=data)[0]
    s.solve_gains(2, slice_mask=mask, reset_gain_moments=True)
    got, after = s.get_moments(), s.get_params()
    for t, part in enumerate(rows):
        for k in ("gm_r", "gm_i", "gv_r", "gv_i"):
            np.testing.assert_array_equal(got[k][part], (fresh if mask[t] else moved)[k][part], err_msg=f"{k} of slice {t}")
        for k, ref in ((0, want.real), (1, want.imag)):
            if mask[t]:
                err = plane_err(after[k][part], ref[part])
                print(f"{label}: slice {t} plane {k} {err:.2e}")
                assert err <= TOL[np.dtype(dtype)]["plane"] and not np.array_equal(after[k][part], before[k][part])
            else:
                np.testing.assert_array_equal(after[k][part], before[k][part], err_msg=f"plane {k} of slice {t}")
    for k in ("cm_r", "cm_i", "cv_r", "cv_i", "t"):
        np.testing.assert_array_equal(got[k], moved[k], err_msg=k)
    assert got["t"] == 4
    np.testing.assert_array_equal(after[2], before[2])
    np.testing.assert_array_equal(after[3], before[3])
    assert len(s.run_slices(2, tol=0.0)[1][0]) == 2  # and the fit goes on
    s.close()


# ---- error codes
def test_wrong_arguments_and_wrong_state_are_reported():
    from calamity_amd.solver import HipFitSolver

    p, params = edge_problem(5, 48)
    s = solver_of(p, params, np.float64)
    for kw in (dict(nsweeps=1, damping=0.0), dict(nsweeps=1, damping=1.5), dict(nsweeps=0)):
        with pytest.raises(_lib.CalamityHipError) as err:
            s.solve_gains(**kw)
        assert err.value.code == _lib.CAL_ERR_INVALID, kw
    s.solve_gains(1, damping=1.0)  # the closed end of (0, 1]
    s.set_gain_basis(np.array(modeling.gain_dpss_basis(150e6 + 400e3 * np.arange(p.nfreqs), 100.0)))
    with pytest.raises(_lib.CalamityHipError) as err:
        s.solve_gains(1)
    assert err.value.code == _lib.CAL_ERR_UNSUPPORTED and "basis" in str(err.value)
    s.set_gain_basis(None)
    s.solve_gains(1)
    s.close()
    shell = copy.copy(p)
    shell.data_r = shell.data_i = shell.wgts = None
    s = HipFitSolver(dtype=np.float64)
    s.set_problem(shell)
    s.set_data(p.data_r, p.data_i, p.wgts)
    s.set_params(c_r=params["c_r"], c_i=params["c_i"])
    with pytest.raises(_lib.CalamityHipError) as err:  # no gains
        s.solve_gains(1)
    assert err.value.code == _lib.CAL_ERR_STATE
    s.close()


def test_held_slices_stay_stopped_in_a_later_run():
    """``hold_slices``: what the chunked loop of the drop-in (gain_solve_every) keeps a slice that met the tolerance with."""
    from calamity_amd.solver import HipFitSolver

    T, dtype = 2, np.float64
    parts = [synthetic.make_problem(5, 48, f0=150e6, df=400e3, seed=21, data_seed=30 + t) for t in range(T)]
    p0 = parts[0][0]
    sub, _, _ = batched.replicate_slices(p0, T)
    s = HipFitSolver(dtype=dtype)
    s.set_problem(sub)
    s.set_data(*[np.concatenate([getattr(parts[t][0], k) for t in range(T)]) for k in ("data_r", "data_i", "wgts")])
    s.set_params(*[np.concatenate([parts[t][2][k] for t in range(T)]) for k in ("g_r", "g_i", "c_r", "c_i")])
    s.set_optimizer("Adam", learning_rate=1e-2)
    s.run_slices(3, tol=0.0)
    before = s.get_params()
    s.hold_slices([0, 1])
    res = s.run_slices(3, tol=0.0)
    after = s.get_params()
    assert len(res[0][0]) == 3 and len(res[1][0]) == 0 and res[1][1] and res[1][2] == 0
    na = p0.nants
    np.testing.assert_array_equal(after[0][na:], before[0][na:])
    assert not np.array_equal(after[0][:na], before[0][:na])
    s.hold_slices(None)
    assert len(s.run_slices(2, tol=0.0)[1][0]) == 2
    s.close()
