"""Host checks of the joint Gauss-Newton step (no GPU): the NumPy restatement tests/gauss_newton_ref.py against the oracle's gradients
and against the densely built matrix, its convergence on the problems the device tests use, the host's damping rule, the C-ABI
structures against the header, every ``ValueError`` of the keywords and the calls ``drive`` issues (calamity_amd/fit_loop.py)."""
import copy
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from calamity_amd import _lib, calibration, synthetic
from calamity_amd.fit_loop import FitControls, FitOptions, GaussNewtonOptions, drive, history_entry, next_lambda
from fit_loop_cases import TOL, UNRECORDED, NewtonFake, going, recorded
from gauss_newton_ref import Ref, dense_normal_matrix, flatten

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def relnorm(got, want):
    return float(np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-300))


@functools.lru_cache(maxsize=None)
def problem(nants, nfreqs, **kw):
    p, _, start = synthetic.make_problem(nants, nfreqs, **kw)
    return p, start["g_r"] + 1j * start["g_i"], start["c_r"] + 1j * start["c_i"]


def perturbed(p, g, c, seed):
    rng = np.random.default_rng(seed)
    return (g + 0.1 * (rng.standard_normal(g.shape) + 1j * rng.standard_normal(g.shape)),
            c * (1.0 + 0.1 * rng.standard_normal(c.shape)) + 0.05j * np.abs(c) * rng.standard_normal(c.shape))


def direction(p, c, seed):
    rng = np.random.default_rng(seed)
    cs = np.sqrt(np.mean(np.abs(c) ** 2))
    return (0.3 * (rng.standard_normal((p.nants, p.nfreqs)) + 1j * rng.standard_normal((p.nants, p.nfreqs))),
            cs * (rng.standard_normal(p.ncoeffs) + 1j * rng.standard_normal(p.ncoeffs)))


# ---- the restatement against the oracle
@pytest.mark.parametrize("reg", [False, True], ids=["none", "sum"])
def test_product_and_rhs_are_minus_half_the_oracles_gradient_differences(reg):
    """N p = -1/2 (grad(G m + J p) - grad(G m)) and rhs = -1/2 (grad(d) - grad(G m)) with the gradients of the C oracle (oracle/ref_c.c);
    with the "sum" regulariser grad(G m) is the regulariser's own gradient and cancels."""
    from oracle.ref_c import CRef

    p, g0, c0 = problem(5, 64, seed=3)
    g, c = perturbed(p, g0, c0, 1)
    ref = Ref(p)
    dg, dc = direction(p, c, 2)
    gm = g[ref.i] * np.conj(g[ref.j]) * ref.model(c)

    def grad(data):
        q = copy.copy(p)
        q.data_r, q.data_i = np.ascontiguousarray(data.real), np.ascontiguousarray(data.imag)
        o = CRef(q, np.float64, nthreads=4)
        o.set_regularization("sum" if reg else None, 1.5 if reg else 0.0, -0.5 if reg else 0.0)
        out = o.loss_grads(np.ascontiguousarray(g.real), np.ascontiguousarray(g.imag), np.ascontiguousarray(c.real), np.ascontiguousarray(c.imag))
        return np.asarray(out[1]) + 1j * np.asarray(out[2]), np.asarray(out[3]) + 1j * np.asarray(out[4])

    base = grad(gm)
    if not reg:
        assert max(np.max(np.abs(base[0])), np.max(np.abs(base[1]))) <= 1e-12
    with_p = grad(gm + ref.jvp(g, c, dg, dc))
    at_d = grad(ref.d)
    want = ref.normal_product(g, c, dg, dc)
    rhs = ref.rhs(g, c)
    for k in range(2):
        assert relnorm(-0.5 * (with_p[k] - base[k]), want[k]) <= 1e-10
        assert relnorm(-0.5 * (at_d[k] - base[k]), rhs[k]) <= 1e-10


def test_product_equals_the_dense_matrix_and_is_symmetric_positive():
    p, g0, c0 = problem(4, 32, seed=4)
    g, c = perturbed(p, g0, c0, 5)
    ref = Ref(p)
    N = dense_normal_matrix(ref, g, c)
    assert np.max(np.abs(N - N.T)) <= 1e-12 * np.max(np.abs(N))
    dirs = [direction(p, c, s) for s in (6, 7)]
    prods = [ref.normal_product(g, c, *d) for d in dirs]
    for d, out in zip(dirs, prods):
        assert relnorm(flatten(*out), N @ flatten(*d)) <= 1e-10
    pq, qp = float(flatten(*dirs[0]) @ flatten(*prods[1])), float(flatten(*dirs[1]) @ flatten(*prods[0]))
    assert abs(pq - qp) <= 1e-12 * max(abs(pq), abs(qp))
    assert all(float(flatten(*d) @ flatten(*out)) >= 0.0 for d, out in zip(dirs, prods))
    # the diagonal the preconditioner estimates
    d_g, d_c = ref.precond(g, c)
    diag = np.diag(N)
    ng = p.nants * p.nfreqs
    np.testing.assert_allclose(diag[:ng], d_g.ravel(), rtol=1e-10)  # (no autocorrelations here: den is the diagonal exactly)
    assert 0.3 <= np.median(diag[2 * ng : 2 * ng + p.ncoeffs] / d_c) <= 3.0


# ---- convergence of the restatement
CASES = [((7, 200), dict(seed=0)), ((7, 200), dict(seed=1)), ((7, 200), dict(seed=2)), ((7, 200), dict(seed=207)), ((5, 64), dict(seed=3)),
         ((4, 32), dict(seed=4)), ((7, 200), dict(seed=207, flag_frac=0.2))]


@pytest.mark.parametrize("shape,kw", CASES, ids=[f"{s[0]}x{s[1]}-" + "-".join(f"{k}{v}" for k, v in kw.items()) for s, kw in CASES])
def test_two_steps_leave_a_thousandth_of_the_chi_square(shape, kw):
    """ncg = 20, lambda = 1e-3 then 1e-4 from unity gains and c0; measured 5e-5 ... 1.5e-4."""
    p, g, c = problem(*shape, **kw)
    ref = Ref(p)
    l0 = ref.loss(g, c)
    for lam in (1e-3, 1e-4):
        st = ref.step(g, c, lam=lam, ncg=20)
        assert st["accepted"]
        g, c = st["g"], st["c"]
    ratio = ref.loss(g, c) / l0
    print(f"{shape} {kw}: {ratio:.2e} of the start")
    assert ratio <= 1e-3


def test_an_undamped_step_from_far_away_is_rejected_and_the_damping_rule_recovers():
    """gain_sigma = 1: lambda = 0 gives a trial of 2.39 against 0.786; from lambda = 1e-3 the host's rule rejects twice (2.13, 1.17), then
    accepts (0.42)."""
    p, g, c = problem(7, 200, seed=207, gain_sigma=1.0)
    ref = Ref(p)
    st = ref.step(g, c, lam=0.0, ncg=20)
    assert not st["accepted"] and st["loss_after"] > st["loss_before"] and st["g"] is g and st["c"] is c
    assert abs(st["loss_after"] - 2.39) < 0.01 and abs(st["loss_before"] - 0.786) < 0.001
    lam, seen = np.asarray([1e-3]), []
    for _ in range(3):
        st = ref.step(g, c, lam=float(lam[0]), ncg=20)
        seen.append((float(lam[0]), st["accepted"], st["loss_after"]))
        lam = next_lambda(lam, [st["accepted"]])
    print(seen)
    assert [s[1] for s in seen] == [False, False, True]
    np.testing.assert_allclose([s[0] for s in seen], [1e-3, 1e-2, 1e-1])
    np.testing.assert_allclose([s[2] for s in seen], [2.13, 1.17, 0.42], atol=0.01)
    np.testing.assert_allclose(lam, [1e-2])
    np.testing.assert_allclose(next_lambda([0.0, 1e-9, 1.0], [False, False, True]), [1e-5, 1e-5, 0.1])


# ---- the C-ABI
def test_structures_follow_the_header():
    header = open(os.path.join(ROOT, "include", "calamity_hip.h")).read()
    fields = re.search(r"typedef struct cal_gauss_newton_desc \{(.*?)\} cal_gauss_newton_desc;", header, re.S).group(1)
    names = re.findall(r"(\w+)\s*;", fields)
    assert names == [n for n, _ in _lib.GaussNewtonDesc._fields_] == ["ncg", "reset_moments", "cg_tol", "lambda", "slice_mask"]
    assert [t for _, t in _lib.GaussNewtonDesc._fields_] == [C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_void_p]
    assert C.sizeof(_lib.GaussNewtonDesc) == 32 and _lib.GaussNewtonDesc.cg_tol.offset == 8 and _lib.GaussNewtonDesc.slice_mask.offset == 24
    fields = re.search(r"typedef struct cal_gauss_newton_result \{(.*?)\} cal_gauss_newton_result;", header, re.S).group(1)
    assert re.findall(r"(\w+)\s*[,;]", fields) == [n for n, _ in _lib.GaussNewtonResult._fields_] == ["loss_before", "loss_after", "cg_residual", "cg_iters",
                                                                                                      "accepted"]
    assert re.search(r"double loss_before, loss_after, cg_residual; int32_t cg_iters, accepted;", fields)
    assert [t for _, t in _lib.GaussNewtonResult._fields_] == [C.c_double] * 3 + [C.c_int32] * 2 and C.sizeof(_lib.GaussNewtonResult) == 32
    assert re.search(r"int cal_solver_gauss_newton_step\(cal_solver\* s, const cal_gauss_newton_desc\* desc, cal_gauss_newton_result\* results", header)
    proto = re.search(r"int cal_solver_normal_product\((.*?)\);", header, re.S).group(1)
    assert re.findall(r"(\w+)\s*(?:,|$)", proto) == ["s", "p_g_r", "p_g_i", "p_c_r", "p_c_i", "out_g_r", "out_g_i", "out_c_r", "out_c_i"]
    assert _lib.SYMBOLS["cal_solver_normal_product"] == (C.c_int, [C.c_void_p] * 9)
    assert _lib.SYMBOLS["cal_solver_gauss_newton_step"] == (C.c_int, [C.c_void_p, C.POINTER(_lib.GaussNewtonDesc), C.POINTER(_lib.GaussNewtonResult)])
    lib = _lib.load()
    assert lib.cal_solver_gauss_newton_step(None, None, None) == -1 and lib.cal_solver_normal_product(*[None] * 9) == -1
    for fn in (calibration.calibrate_and_model_tensor, calibration.fit_gains_and_foregrounds):
        import inspect

        sig = inspect.signature(fn).parameters
        assert [(k, sig[k].default) for k in sig if k.startswith("gauss_newton")] == [
            ("gauss_newton_rounds", 0), ("gauss_newton_every", 0), ("gauss_newton_cg_iters", 20), ("gauss_newton_lambda", 1e-3), ("gauss_newton_cg_tol", 1e-3)]
    args = calibration.dpss_fit_argparser().parse_args(["--input_data_files", "a.uvh5", "--gauss_newton_rounds", "2", "--gauss_newton_every", "50", "--gauss_newton_cg_iters", "7",
                                                        "--gauss_newton_lambda", "0.01", "--gauss_newton_cg_tol", "1e-2"])
    assert (args.gauss_newton_rounds, args.gauss_newton_every, args.gauss_newton_cg_iters, args.gauss_newton_lambda, args.gauss_newton_cg_tol) == (2, 50, 7, 0.01, 1e-2)
    none = calibration.dpss_fit_argparser().parse_args(["--input_data_files", "a.uvh5"])
    assert GaussNewtonOptions.pick(vars(none)) == GaussNewtonOptions()


# ---- the keywords
def test_options_have_the_public_names_and_defaults_and_fit_options_keeps_its_fields():
    import dataclasses

    assert [(f.name, f.default) for f in dataclasses.fields(GaussNewtonOptions)] == [
        ("gauss_newton_rounds", 0), ("gauss_newton_every", 0), ("gauss_newton_cg_iters", 20), ("gauss_newton_lambda", 1e-3), ("gauss_newton_cg_tol", 1e-3)]
    assert len(dataclasses.fields(FitOptions)) == 17 and not GaussNewtonOptions().on
    picked = GaussNewtonOptions.pick(dict(gauss_newton_rounds=2, gauss_newton_every=0, gauss_newton_cg_iters=5, gauss_newton_lambda=0.5,
                                          gauss_newton_cg_tol=0.0, other=1))
    assert picked == GaussNewtonOptions(2, 0, 5, 0.5, 0.0) and picked.on
    with pytest.raises(dataclasses.FrozenInstanceError):
        picked.gauss_newton_rounds = 3


BAD_NUMBERS = [dict(gauss_newton_rounds=-1), dict(gauss_newton_rounds=1.5), dict(gauss_newton_every=-2), dict(gauss_newton_rounds=True),
               dict(gauss_newton_cg_iters=0), dict(gauss_newton_cg_iters=2.5), dict(gauss_newton_lambda=-1e-3), dict(gauss_newton_lambda=np.inf),
               dict(gauss_newton_cg_tol=-1.0), dict(gauss_newton_cg_tol=np.nan)]


@pytest.mark.parametrize("kw", BAD_NUMBERS, ids=[f"{k}={v}" for kw in BAD_NUMBERS for k, v in kw.items()])
def test_bad_numbers_raise_even_with_the_feature_off(kw):
    with pytest.raises(ValueError, match=next(iter(kw))):
        GaussNewtonOptions(**kw).check(FitOptions(), False, False, False)


def test_refused_combinations_raise():
    on = GaussNewtonOptions(gauss_newton_rounds=1)
    plain = FitOptions()
    on.check(plain, False, False, False)
    GaussNewtonOptions().check(plain, True, True, True, groups_split=True)  # off: nothing to refuse
    for args, word in (((True, False, False), "gain_basis"), ((False, True, False), "gain_time"), ((False, False, True), "freeze_model")):
        with pytest.raises(ValueError, match=word):
            on.check(plain, *args)
    with pytest.raises(ValueError, match="device_split"):
        on.check(plain, False, False, False, groups_split=True)
    every = GaussNewtonOptions(gauss_newton_every=5)
    every.check(FitOptions(robust_every=5, gain_solve_every=5), False, False, False)
    for other in (FitOptions(robust_every=4), FitOptions(gain_solve_every=10)):
        with pytest.raises(ValueError, match="same value"):
            every.check(other, False, False, False)
    on.check(FitOptions(robust_every=4), False, False, False)  # (start-up rounds alone share no gap)


def test_public_calls_refuse_before_any_device_work():
    """The public functions raise from the keywords alone: nothing of their other arguments is touched."""
    never = object()
    for kw, word in ((dict(gain_basis=np.eye(4)), "gain_basis"), (dict(freeze_model=True), "freeze_model")):
        with pytest.raises(ValueError, match=word):
            calibration.fit_gains_and_foregrounds(*[never] * 9, gauss_newton_rounds=1, **kw)
    for kw, word in ((dict(gain_max_dly=100.0), "gain_basis"), (dict(gain_basis=np.eye(4)), "gain_basis"), (dict(gain_time_scale=60.0), "gain_time"),
                     (dict(gain_time_basis=np.eye(2)), "gain_time"), (dict(freeze_model=True), "freeze_model"), (dict(robust_every=3), "same value")):
        with pytest.raises(ValueError, match=word):
            calibration.calibrate_and_model_tensor(never, never, gauss_newton_every=7, **kw)
    with pytest.raises(ValueError, match="gauss_newton_cg_iters"):
        calibration.calibrate_and_model_tensor(never, never, gauss_newton_cg_iters=0)


# ---- the calls drive issues
def step(lam, **kw):
    return ("gauss_newton_step", (), dict(ncg=20, cg_tol=1e-3, lam=lam, **kw))


def test_defaults_issue_no_call_and_return_none():
    script = going(7, 2)
    fake = NewtonFake([script], nl=2)
    out = drive(fake, FitControls(newton=GaussNewtonOptions()), 2, 0, 7, TOL, False, False)
    assert fake.log == [UNRECORDED, recorded(7)] and out.loops is script and out.newton is None
    assert "gauss_newton" not in history_entry(FitControls(), out, 0, np.dtype(np.float32))
    fake = NewtonFake([going(7, 2)], nl=2)
    out = drive(fake, FitControls(FitOptions()), 2, 0, 7, TOL, False, False)  # (callers that know nothing of the steps)
    assert out.newton is None and out.lbfgs is None


def test_start_up_rounds_follow_the_solves_and_keep_a_damping_per_slice():
    fake = NewtonFake([going(4, 2)], nl=2, accept=[[1, 0], [1, 1], [0, 1]])
    opts = FitOptions(coeff_solve_rounds=1, gain_solve_sweeps=2)
    newton = GaussNewtonOptions(gauss_newton_rounds=3, gauss_newton_lambda=1e-2)
    out = drive(fake, FitControls(opts, newton), 2, 0, 4, TOL, False, False)
    gn = out.newton
    want = [("solve_coeffs", (), dict(ridge=1e-6)), ("solve_gains", (2,), dict(damping=0.5)), step([1e-2, 1e-2]), step([1e-3, 1e-1]), step([1e-4, 1e-2]),
            UNRECORDED, recorded(4)]
    assert [e[:2] for e in fake.log] == [e[:2] for e in want]
    for got, exp in zip(fake.log, want):
        assert sorted(got[2]) == sorted(exp[2])
        for k in exp[2]:
            np.testing.assert_allclose(got[2][k], exp[2][k], rtol=1e-12, err_msg=k)
    np.testing.assert_allclose(gn["lambda"], [1e-3, 1e-3])
    assert list(gn["steps"]) == [3, 3] and list(gn["accepted"]) == [2, 2]
    # the loss after every step: the trial's where accepted, the loss before where rejected (calls are log entries 3, 4, 5)
    assert gn["loss"] == [[29.0, 39.0, 50.0], [30.0, 39.0, 49.0]] and gn["cg_iters"] == [[3, 4, 5], [3, 4, 5]]
    h = history_entry(FitControls(opts, newton), out, 1, np.dtype(np.float64))
    assert h["gauss_newton"] == {"steps": 3, "accepted": 2, "lambda": pytest.approx(1e-3), "loss": [30.0, 39.0, 49.0], "cg_iters": [3, 4, 5]}


def test_a_step_in_every_gap_comes_last_and_skips_the_loops_that_are_over():
    second = going(5, 3)
    second[1] = (np.arange(3, dtype=np.float64), True, 3)  # loop 1 meets the tolerance inside the second chunk
    fake = NewtonFake([going(5, 3), second, going(2, 3)], nl=3, rows=6, accept=[[1, 1, 1], [1, 0, 0]])
    opts = FitOptions(gain_solve_every=5, coeff_solve_rounds=1, robust_every=5)
    gn = drive(fake, FitControls(opts, GaussNewtonOptions(gauss_newton_every=5)), 3, 2, 12, TOL, False, False).newton
    names = [e[0] for e in fake.log]
    gap = ["hold_slices", "robust_weights", "solve_coeffs", "solve_gains", "gauss_newton_step"]
    assert names == ["solve_coeffs", "run_slices", "run_slices"] + gap + ["run_slices"] + gap + ["run_slices", "hold_slices"]
    steps = [e for e in fake.log if e[0] == "gauss_newton_step"]
    assert steps[0][2] == dict(ncg=20, cg_tol=1e-3, lam=[1e-3] * 3, slice_mask=[1, 1, 1], reset_moments=True)
    assert steps[1][2]["slice_mask"] == [1, 0, 1] and steps[1][2]["reset_moments"] is True
    np.testing.assert_allclose(steps[1][2]["lam"], [1e-4] * 3)
    np.testing.assert_allclose(gn["lambda"], [1e-5, 1e-4, 1e-3])  # loop 1 sat the second step out: its damping stays
    assert list(gn["steps"]) == [2, 1, 2] and list(gn["accepted"]) == [2, 1, 1] and [len(x) for x in gn["loss"]] == [2, 1, 2]


def test_steps_alone_chunk_the_loop():
    fake = NewtonFake([going(4, 1), going(4, 1), going(2, 1)], accept=[[1], [1]])
    gn = drive(fake, FitControls(newton=GaussNewtonOptions(gauss_newton_every=4, gauss_newton_cg_iters=3, gauss_newton_cg_tol=0.0)), 1, 0, 10, TOL, False, False).newton
    assert [e[0] for e in fake.log] == ["run_slices", "run_slices", "hold_slices", "gauss_newton_step", "run_slices", "hold_slices", "gauss_newton_step",
                                        "run_slices", "hold_slices"]
    assert fake.log[3][2] == dict(ncg=3, cg_tol=0.0, lam=[1e-3], slice_mask=[1], reset_moments=True) and list(gn["steps"]) == [2]
