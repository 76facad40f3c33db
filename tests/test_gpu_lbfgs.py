"""cal_solver_lbfgs on the device against the NumPy restatement tests/lbfgs_ref.py (include/calamity_hip.h): L-BFGS with a backtracking
Armijo search over the optimizer's own variables, the two-loop recursion run on the Gram matrix of the history.

The restatement works in fp64 on what the solver holds (inputs, variables, gradient, direction and pairs rounded to its dtype) and runs
the classic recursion on full vectors.  Tolerances are the project's own for a short trajectory (tests/test_gpu_gauss_newton.py): losses
fp64 1e-10, fp32 1e-5; parameters norm-wise fp64 1e-8, fp32 1e-3; fp32 is compared over the first 4 iterations only.  Before a
trajectory is compared the test asserts the restatement's own decision margin (>= 1e-6 for fp64 cases, >= 1e-2 for fp32 cases, over the
iterations that are compared): a condition on the inputs, met by choosing the problems, so that no accept / reject decision lies inside
the device's rounding error.  The closest decision is always the first one: the problems' weights sum to 1, the gradient at the start is
shorter than 1, so the first step -g falls by |g|^2, about a hundredth of the loss.  Where that is under 1e-2 the test gives the problem
four times the weights (``heavier``), which makes that step four times as long in units of the loss."""
import copy
import functools

import numpy as np
import pytest

from calamity_amd import _lib, modeling, synthetic
from gauss_newton_ref import Ref
from lbfgs_ref import LbfgsRef
from test_gain_time_basis_host import joint_case
from test_gpu_fit_quality import perturbed, solver_of
from test_gpu_gauss_newton import KEYS, PATH_CASES, PRIORS, alias_batch, assert_path, base_problem, batch_solver, cast_params, relnorm, three_slices

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
TOL = {np.dtype(np.float64): dict(params=1e-8, loss=1e-10, margin=1e-6), np.dtype(np.float32): dict(params=1e-3, loss=1e-5, margin=1e-2)}
FIRST = 4  # iterations over which an fp32 trajectory is compared
COUNTERS = ("iters", "evals", "status", "pairs_dropped")


def name(dtype):
    return np.dtype(dtype).name


def heavier(p, factor=4.0):
    q = copy.copy(p)
    q.wgts = np.asarray(p.wgts) * factor
    return q


@functools.lru_cache(maxsize=None)
def reference(shape, dtype_name, nsteps, history, reg=False, freeze=False, weight=1.0):
    p, params = base_problem(*shape)
    p = heavier(p, weight)
    dtype = np.dtype(dtype_name).type
    g, c = cast_params(params, dtype)
    return LbfgsRef(Ref(p, dtype=dtype), dtype, priors=PRIORS if reg else None, freeze_model=freeze).run(g, c, nsteps, history=history)


def check_losses(got, want, dtype, label, upto=None):
    n = len(want) if upto is None else upto + 1
    err = float(np.max(np.abs(got[:n] - want[:n]) / np.abs(want[:n])))
    print(f"{label}: losses over {n - 1} iterations {err:.2e}  ({want[0]:.4e} -> {want[n - 1]:.4e})")
    assert np.all(np.isfinite(got[:n])) and err <= TOL[np.dtype(dtype)]["loss"], (label, err)
    return err


def check_params(s, want_g, want_c, dtype, label):
    g_r, g_i, c_r, c_i = s.get_params()
    errs = [relnorm(g_r, want_g.real), relnorm(g_i, want_g.imag), relnorm(c_r, want_c.real), relnorm(c_i, want_c.imag)]
    print(f"{label}: " + "  ".join(f"{k} {e:.2e}" for k, e in zip(KEYS, errs)))
    assert max(errs) <= TOL[np.dtype(dtype)]["params"], (label, errs)


def check_trajectory(s, params, refs, dtype, label, **kw):
    """``refs(nsteps)``: the restatement's run.  fp64: the whole run of 12 iterations.  fp32: the losses of the first FIRST iterations
    of that run, then counters, losses and parameters of a second run of FIRST iterations from the same start."""
    want, short = refs(12), refs(FIRST)
    tol = TOL[np.dtype(dtype)]
    margin = want["margin"] if dtype == np.float64 else short["margin"]
    print(f"{label}: the restatement's decision margin {margin:.2e}")
    assert margin >= tol["margin"], "choose a problem whose decisions are not marginal"
    out = s.lbfgs(12, history=3, **kw)
    if dtype == np.float64:
        for k in COUNTERS:
            assert out[k][0] == want[k], (label, k, out[k][0], want[k])
        check_losses(out["losses"][0], want["losses"], dtype, label)
        check_params(s, s_gains(want), want["c"], dtype, label)
        assert out["loss_after"][0] == out["losses"][0][12] and out["loss_before"][0] == out["losses"][0][0]
        return
    check_losses(out["losses"][0], want["losses"], dtype, label, upto=FIRST)
    s.set_params(*[params[k] for k in KEYS])
    out = s.lbfgs(FIRST, history=3, **kw)
    for k in COUNTERS:
        assert out[k][0] == short[k], (label, k)
    check_losses(out["losses"][0], short["losses"], dtype, label + f" ({FIRST} iterations)")
    check_params(s, s_gains(short), short["c"], dtype, label + f" ({FIRST} iterations)")


def s_gains(run):
    return run["gains"] if "gains" in run else run["v"]


# ---- trajectory parity on every kernel path
@pytest.mark.parametrize("shape,config,dtype", PATH_CASES, ids=[f"{s[0]}x{s[1]}-{c[0]}-{c[1]}-{name(d)}" for s, c, d in PATH_CASES])
def test_trajectory_parity_on_every_kernel_path(shape, config, dtype):
    """12 iterations with 3 stored pairs from the perturbed starts: the ring wraps.  (6, 300): rows padded from 300 to 384 channels,
    more than one block per slice."""
    layout, path, runs = config
    p, params = base_problem(*shape)
    s = solver_of(p, params, dtype, layout, path)
    if runs:
        assert_path(s, runs)
    check_trajectory(s, params, lambda n: reference(shape, name(dtype), n, 3), dtype, f"{shape} {layout}/{path} {name(dtype)}")
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_trajectory_parity_with_the_sum_regulariser(dtype):
    p, params = base_problem(7, 200)
    s = solver_of(heavier(p), params, dtype, "stream")
    s.set_regularization("sum", *PRIORS)
    check_trajectory(s, params, lambda n: reference((7, 200), name(dtype), n, 3, reg=True, weight=4.0), dtype, f"sum regulariser {name(dtype)}")
    s.close()


def test_a_longer_history_reaches_a_lower_loss_and_the_device_follows_both():
    want = {h: reference((7, 200), "float64", 12, h) for h in (1, 8)}
    assert want[8]["losses"][12] < want[1]["losses"][12] and min(want[1]["margin"], want[8]["margin"]) >= 1e-6
    p, params = base_problem(7, 200)
    for h in (1, 8):
        s = solver_of(p, params, np.float64, "stream")
        out = s.lbfgs(12, history=h)
        check_losses(out["losses"][0], want[h]["losses"], np.float64, f"history {h}")
        assert [out[k][0] for k in COUNTERS] == [want[h][k] for k in COUNTERS]
        s.close()


# ---- the smallest shapes that can still break the vector kernels
@functools.lru_cache(maxsize=None)
def tiny_problem():
    p, _, start = synthetic.make_problem(4, 32, f0=150e6, df=400e3, seed=4)
    return p, perturbed(p, start, seed=5)


@pytest.mark.parametrize("freeze", [False, True], ids=["joint", "frozen"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_space_shorter_than_one_blocks_stride(dtype, freeze):
    """4 antennas x 32 channels: fewer 16-byte chunks than one block has threads.  With freeze_model the coefficients keep their bits."""
    p, params = tiny_problem()
    g, c = cast_params(params, dtype)
    want = LbfgsRef(Ref(p, dtype=dtype), dtype, freeze_model=freeze).run(g, c, FIRST, history=3)
    assert want["margin"] >= TOL[np.dtype(dtype)]["margin"]
    s = solver_of(p, params, dtype, "stream")
    before = s.get_params()
    out = s.lbfgs(FIRST, history=3, freeze_model=freeze)
    assert [out[k][0] for k in COUNTERS] == [want[k] for k in COUNTERS]
    check_losses(out["losses"][0], want["losses"], dtype, f"4x32 {name(dtype)} freeze={freeze}")
    check_params(s, want["v"], want["c"], dtype, f"4x32 {name(dtype)} freeze={freeze}")
    after = s.get_params()
    if freeze:
        np.testing.assert_array_equal(after[2], before[2])
        np.testing.assert_array_equal(after[3], before[3])
    assert np.any(after[0] != before[0]) and out["loss_after"][0] < out["loss_before"][0]
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_three_slices_whose_runs_start_off_the_16_byte_grid(dtype):
    """Three slices on shared tiles with 730 coefficients each (groups of 150, 40, 160, .. vectors): in fp32 the runs of slices 1 and 2
    and the second plane start off the 16-byte grid and end inside a vector.  Every slice against the restatement of its own problem.
    (The slices of tests/_slice_cases.py share one geometry, so their coefficient counts are equal; the groups' counts are not.)"""
    sub, data, params, parts = alias_batch(dtype)
    assert parts[0].ncoeffs % 4 == 2
    data = (data[0], data[1], 4.0 * data[2])
    parts = [heavier(q) for q in parts]
    s = batch_solver(sub, data, params, dtype)
    out = s.lbfgs(FIRST, history=2)
    got = s.get_params()
    g, c = cast_params(params, dtype)
    for t, q in enumerate(parts):
        rows, idx = slice(t * q.nants, (t + 1) * q.nants), slice(t * q.ncoeffs, (t + 1) * q.ncoeffs)
        want = LbfgsRef(Ref(q, dtype=dtype), dtype).run(g[rows], c[idx], FIRST, history=2)
        label = f"slice {t} of three {name(dtype)}"
        assert want["margin"] >= TOL[np.dtype(dtype)]["margin"], label
        assert [out[k][t] for k in COUNTERS] == [want[k] for k in COUNTERS], label
        check_losses(out["losses"][t], want["losses"], dtype, label)
        errs = [relnorm(got[0][rows], want["v"].real), relnorm(got[1][rows], want["v"].imag), relnorm(got[2][idx], want["c"].real),
                relnorm(got[3][idx], want["c"].imag)]
        print(f"{label}: " + "  ".join(f"{k} {e:.2e}" for k, e in zip(KEYS, errs)))
        assert max(errs) <= TOL[np.dtype(dtype)]["params"], (label, errs)
    s.close()


# ---- gain bases
def basis_case(kind):
    """(problem, start, B or None, Bt or None)."""
    if kind == "freq":
        p, _, start = synthetic.make_problem(6, 64, f0=150e6, df=400e3, seed=8)
        return heavier(p), perturbed(p, start, seed=9), np.array(modeling.gain_dpss_basis(150e6 + 400e3 * np.arange(64), 200.0)), None
    big, start = joint_case()[:2]  # 3 times of 7 antennas x 40 channels as one fit
    Bt = np.linalg.qr(np.random.default_rng(12).standard_normal((3, 2)))[0]
    B = np.array(modeling.gain_dpss_basis(150e6 + 400e3 * np.arange(40), 200.0)) if kind == "time+freq" else None
    return heavier(big), start, B, Bt


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["freq", "time", "time+freq"])
def test_trajectory_parity_with_gain_bases(kind, dtype):
    """gain_dpss_basis on 64 channels; a joint fit of 3 times with L = 2, alone and on top of the frequency basis.  The variables are y:
    get_gain_coeffs moved, and the gains equal g0 + Bt (x) B y."""
    p, params, B, Bt = basis_case(kind)
    s = solver_of(p, params, dtype, "shared")
    if B is not None:
        s.set_gain_basis(B)
    if Bt is not None:
        s.set_gain_time_basis(Bt)
    g0, c = cast_params(params, dtype)
    y_shape = s.get_gain_coeffs()[0].shape
    lb = LbfgsRef(Ref(p, dtype=dtype), dtype, g0=g0, B=B, Bt=Bt)

    def refs(n):
        out = lb.run(np.zeros(y_shape, dtype=np.complex128), c, n, history=3)
        return dict(out, gains=lb.gains_of(out["v"]))

    check_trajectory(s, params, refs, dtype, f"{kind} basis {name(dtype)}")
    want = refs(12 if dtype == np.float64 else FIRST)
    y_r, y_i = s.get_gain_coeffs()
    assert np.any(y_r != 0) and np.any(y_i != 0)
    errs = [relnorm(y_r, want["v"].real), relnorm(y_i, want["v"].imag)]
    print(f"{kind} basis {name(dtype)}: y_r {errs[0]:.2e}  y_i {errs[1]:.2e}")
    assert max(errs) <= TOL[np.dtype(dtype)]["params"]
    y = np.asarray(y_r, dtype=np.float64) + 1j * np.asarray(y_i, dtype=np.float64)
    g_r, g_i = s.get_params()[:2]
    expanded = LbfgsRef(Ref(p, dtype=dtype), np.float64, g0=g0, B=None if B is None else B.astype(dtype), Bt=None if Bt is None else Bt.astype(dtype)).gains_of(y)
    assert max(relnorm(g_r, expanded.real), relnorm(g_i, expanded.imag)) <= (1e-6 if dtype == np.float32 else 1e-14)
    s.close()


# ---- batched slices
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_slice_of_a_shared_batch_equals_its_single_solver_and_a_masked_slice_keeps_its_bits(dtype):
    """SHARED layout, mask [1, 0, 1]: the selected slices bit for bit (every reduction of the call is cut by the slice's own sizes and
    the SHARED layout fits a slice of a batch with the kernels of a single fit); slice 1 keeps its bits and reports status 4."""
    s, parts, pars = three_slices(dtype, "shared")
    start = s.get_params()
    out = s.lbfgs(5, history=3, slice_mask=[1, 0, 1])
    after = s.get_params()
    p0 = parts[0][0]
    na, nc = p0.nants, p0.ncoeffs
    assert list(out["status"]) == [0, 4, 0] and out["iters"][1] == 0 and out["evals"][1] == 0 and np.all(np.isnan(out["losses"][1]))
    for k in range(4):
        part = slice(na, 2 * na) if k < 2 else slice(nc, 2 * nc)
        np.testing.assert_array_equal(after[k][part], start[k][part])
    for t in (0, 2):
        one = solver_of(parts[t][0], pars[t], dtype, "shared")
        o1 = one.lbfgs(5, history=3)
        got1 = one.get_params()
        for i in range(4):
            part = slice(t * (na if i < 2 else nc), (t + 1) * (na if i < 2 else nc))
            np.testing.assert_array_equal(after[i][part], got1[i], err_msg=f"slice {t} {KEYS[i]}")
        np.testing.assert_array_equal(o1["losses"][0], out["losses"][t])
        assert [o1[k][0] for k in COUNTERS] == [out[k][t] for k in COUNTERS]
        one.close()
    with pytest.raises(ValueError):
        s.lbfgs(2, slice_mask=[1, 0])
    s.close()


def test_slices_stop_at_different_iterations_under_ftol():
    """The slices' data differ, so their losses fall at different rates: with ftol set each stops on its own (status 1) at the iteration
    the restatement of its own problem stops at, and the others go on."""
    dtype, ftol = np.float64, 0.28
    s, parts, pars = three_slices(dtype, "stream")
    s.set_data(*[np.concatenate([np.asarray(getattr(q[0], k)) * (32.0 if k == "wgts" else 1.0) for q in parts]) for k in ("data_r", "data_i", "wgts")])
    wants = [LbfgsRef(Ref(heavier(q[0], 32.0), dtype=dtype), dtype).run(*cast_params(pars[t], dtype), 15, history=4, ftol=ftol) for t, q in enumerate(parts)]
    assert [w["iters"] for w in wants] == [5, 7, 5] and all(w["status"] == 1 for w in wants)  # (32 times the weights: the first step falls by more than ftol)
    assert min(w["margin"] for w in wants) >= 1e-6
    out = s.lbfgs(15, history=4, ftol=ftol)
    print(f"ftol {ftol}: iterations {list(out['iters'])}")
    assert list(out["iters"]) == [w["iters"] for w in wants] and list(out["status"]) == [1, 1, 1] and list(out["evals"]) == [w["evals"] for w in wants]
    for t, w in enumerate(wants):
        assert np.all(np.isnan(out["losses"][t][w["iters"] + 1 :]))
        check_losses(out["losses"][t], w["losses"], dtype, f"slice {t}", upto=w["iters"])
    s.close()


# ---- nothing else moves
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_call_leaves_everything_but_the_parameters_and_a_continued_run_equals_a_fresh_solver(dtype):
    p, params = base_problem(7, 200)
    s = solver_of(p, params, dtype)
    s.set_optimizer("Adam", learning_rate=1e-2)
    s.run(3, tol=0.0)
    loss0 = s.eval_loss()
    mom, w0, w1, sl = s.get_moments(), s.get_weights(0), s.get_weights(1), s.slice_losses()
    out = s.lbfgs(5, history=3)
    assert out["status"][0] == 0 and out["loss_before"][0] == loss0 and out["loss_after"][0] < loss0
    mom2 = s.get_moments()
    for k in mom:
        np.testing.assert_array_equal(mom2[k], mom[k], err_msg=k)  # (t among them)
    np.testing.assert_array_equal(s.get_weights(0), w0)
    np.testing.assert_array_equal(s.get_weights(1), w1)
    np.testing.assert_array_equal(s.slice_losses(), sl)
    assert s.eval_loss() == out["loss_after"][0]
    held = s.get_params()
    cont = s.run(4, tol=0.0)[0]
    final = s.get_params()
    s.close()
    fresh = solver_of(p, dict(zip(KEYS, held)), dtype)
    fresh.set_optimizer("Adam", learning_rate=1e-2)
    fresh.set_moments(**mom)
    np.testing.assert_array_equal(fresh.run(4, tol=0.0)[0], cont)
    for a, b in zip(fresh.get_params(), final):
        np.testing.assert_array_equal(a, b)
    fresh.close()


@pytest.mark.parametrize("basis", [False, True], ids=["gains", "basis"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_stalled_call_returns_status_2_and_changes_no_bit(dtype, basis):
    """max_ls = 1, c1 = 0.999: the one trial along -g cannot meet the bound, so the slice gets the bits of x_k back."""
    p, params = base_problem(7, 200)
    s = solver_of(p, params, dtype)
    if basis:
        s.set_gain_basis(np.array(modeling.gain_dpss_basis(150e6 + 400e3 * np.arange(p.nfreqs), 200.0)))
    s.set_optimizer("Adam", learning_rate=1e-2)
    before, loss0 = s.get_params(), s.eval_loss()
    dm = s.data_model()
    out = s.lbfgs(3, max_ls=1, c1=0.999, reset_moments=True)
    assert out["status"][0] == 2 and out["iters"][0] == 0 and out["evals"][0] == 1 and out["loss_after"][0] == out["loss_before"][0] == loss0
    assert np.all(np.isnan(out["losses"][0][1:]))
    for a, b in zip(s.get_params(), before):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(s.data_model(), dm):
        np.testing.assert_array_equal(a, b)
    if basis:
        assert not np.any(s.get_gain_coeffs()[0]) and not np.any(s.get_gain_coeffs()[1])
    assert s.eval_loss() == loss0
    s.close()


def test_reset_moments_restores_the_slots_of_the_slices_that_moved():
    dtype = np.float64
    s, parts, pars = three_slices(dtype, "stream")
    s.set_optimizer("Adam", learning_rate=1e-2)
    fresh = s.get_moments()
    s.run_slices(4, tol=0.0)
    moved = s.get_moments()
    out = s.lbfgs(2, slice_mask=[1, 0, 1], reset_moments=True)
    got = s.get_moments()
    assert list(out["status"]) == [0, 4, 0]
    p0 = parts[0][0]
    for k in ("gm_r", "gm_i", "gv_r", "gv_i", "cm_r", "cm_i", "cv_r", "cv_i"):
        n = p0.nants if k[0] == "g" else p0.ncoeffs
        for t in range(3):
            part = slice(t * n, (t + 1) * n)
            np.testing.assert_array_equal(got[k][part], (moved if t == 1 else fresh)[k][part], err_msg=f"{k} of slice {t}")
    assert got["t"] == moved["t"] == 4
    s.close()


# ---- refusals
def test_wrong_arguments_and_wrong_state_are_reported_and_the_vectors_are_counted():
    from calamity_amd.solver import HipFitSolver

    p, params = base_problem(7, 200)
    s = solver_of(p, params, np.float32)
    for kw in (dict(nsteps=0), dict(history=0), dict(history=17), dict(max_ls=0), dict(c1=0.0), dict(c1=1.0), dict(shrink=0.0), dict(shrink=1.0),
               dict(ftol=-1.0), dict(ftol=np.inf), dict(curvature_eps=-1e-8), dict(curvature_eps=np.nan)):
        with pytest.raises(_lib.CalamityHipError) as err:
            s.lbfgs(**dict(dict(nsteps=2), **kw))
        assert err.value.code == _lib.CAL_ERR_INVALID and "lbfgs" in str(err.value), kw
    with pytest.raises(_lib.CalamityHipError) as err:  # no optimizer
        s.lbfgs(2, reset_moments=True)
    assert err.value.code == _lib.CAL_ERR_STATE and "optimizer" in str(err.value)
    lib = _lib.load()
    assert lib.cal_solver_lbfgs(s._h, None, None, None) == _lib.CAL_ERR_INVALID
    before = s.memory_bytes()
    s.lbfgs(1, history=5)
    np_ = 2 * p.nants * 256 + 2 * p.ncoeffs
    grown = s.memory_bytes() - before
    assert (2 * 5 + 4) * np_ * 4 <= grown <= (2 * 5 + 4) * np_ * 4 + (16 << 20)  # the vectors, and the partials, sums and state beside them
    s.close()
    # an exchange hook
    s = HipFitSolver(dtype=np.float64)
    s.set_exchange_hook(lambda arr, op: None, 0, 1)
    s.set_problem(p)
    s.set_params(*[params[k] for k in KEYS])
    with pytest.raises(_lib.CalamityHipError) as err:
        s.lbfgs(2)
    assert err.value.code == _lib.CAL_ERR_UNSUPPORTED and "exchange" in str(err.value)
    s.close()
    # no gains
    shell = copy.copy(p)
    shell.data_r = shell.data_i = shell.wgts = None
    s = HipFitSolver(dtype=np.float64)
    s.set_problem(shell)
    s.set_data(p.data_r, p.data_i, p.wgts)
    s.set_params(c_r=params["c_r"], c_i=params["c_i"])
    with pytest.raises(_lib.CalamityHipError) as err:
        s.lbfgs(2)
    assert err.value.code == _lib.CAL_ERR_STATE
    s.close()


# ---- worth having
def test_thirty_iterations_beat_adam_given_the_same_number_of_passes():
    """make_problem(7, 200, seed=207) from unity gains and c0: 30 iterations at history = 8, then Adam (1e-2) on the same start for as
    many steps as L-BFGS spent passes (iters + evals).  The restatement: 2.4e-4 of the start after 30 iterations."""
    p, _, start = synthetic.make_problem(7, 200, seed=207)
    for dtype in DTYPES:
        s = solver_of(p, start, dtype)
        out = s.lbfgs(30, history=8)
        passes = int(out["iters"][0] + out["evals"][0])
        s.set_params(*[start[k] for k in KEYS])
        s.set_optimizer("Adam", learning_rate=1e-2)
        s.run(passes, tol=0.0)
        adam = s.eval_loss()
        print(f"{name(dtype)}: L-BFGS {out['loss_after'][0]:.4e} of {out['loss_before'][0]:.4e} in {passes} passes; Adam after {passes} steps {adam:.4e}; "
              f"ratio {out['loss_after'][0] / adam:.3f}")
        assert out["status"][0] == 0 and out["loss_after"][0] < adam
        s.close()
