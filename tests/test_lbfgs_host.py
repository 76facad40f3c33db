"""Host checks of the L-BFGS iterations (no GPU): the two-loop recursion on coefficients the device runs (lbfgs_core.hpp through
cal_debug_lbfgs_coefficients) against the classic recursion on full vectors, the NumPy restatement tests/lbfgs_ref.py on a problem the
device tests use, the C-ABI structures against the header, every ``ValueError`` of the keywords and the calls ``drive`` issues
(calamity_amd/fit_loop.py)."""
import ctypes as C
import dataclasses
import inspect
import os
import re

import numpy as np
import pytest

from calamity_amd import _lib, calibration, synthetic
from calamity_amd.fit_loop import FitControls, FitOptions, GaussNewtonOptions, LbfgsOptions, drive, history_entry
from fit_loop_cases import TOL, UNRECORDED, LbfgsFake, going, recorded
from gauss_newton_ref import Ref
from lbfgs_ref import LbfgsRef, two_loop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the recursion
def coefficients(pairs, g):
    """(delta, slope) of cal_debug_lbfgs_coefficients for the Gram matrix of [s_1 .. s_p, y_1 .. y_p, g]."""
    p = len(pairs)
    b = np.array([s for s, _ in pairs] + [y for _, y in pairs] + [g])
    gram = np.ascontiguousarray(b @ b.T)
    delta, slope = np.full(2 * p + 1, np.nan), C.c_double(np.nan)
    _lib.check(_lib.load().cal_debug_lbfgs_coefficients(p, gram.ctypes.data, delta.ctypes.data, C.byref(slope)))
    return delta, slope.value, b


@pytest.mark.parametrize("p", [1, 2, 8, 16])
def test_coefficients_give_the_direction_of_the_classic_two_loop_recursion(p):
    """Random histories of positive curvature (y = H s for a random positive-definite H): d and the slope to 1e-12 relative."""
    rng = np.random.default_rng(100 + p)
    n = 40
    a = rng.standard_normal((n, n))
    hess = a @ a.T / n + 0.5 * np.eye(n)
    pairs = []
    for _ in range(p):
        s = rng.standard_normal(n)
        pairs.append((s, hess @ s))
    g = rng.standard_normal(n)
    delta, slope, b = coefficients(pairs, g)
    want = two_loop(pairs, g)
    d = delta @ b
    assert np.linalg.norm(d - want) <= 1e-12 * np.linalg.norm(want)
    assert abs(slope - g @ want) <= 1e-12 * abs(g @ want) and slope < 0.0


def test_no_pair_gives_minus_the_gradient_and_bad_counts_are_refused():
    g = np.asarray([3.0, -4.0])
    delta, slope, _ = coefficients([], g)
    assert list(delta) == [-1.0] and slope == -25.0
    lib = _lib.load()
    one = np.ones(1)
    for p in (-1, 17):
        assert lib.cal_debug_lbfgs_coefficients(p, one.ctypes.data, one.ctypes.data, C.byref(C.c_double())) != 0
    assert lib.cal_debug_lbfgs_coefficients(0, None, one.ctypes.data, C.byref(C.c_double())) != 0


# ---- the restatement
def test_the_restatement_descends_uses_its_history_and_reports_its_margins():
    p, _, start = synthetic.make_problem(4, 32, seed=4)
    rng = np.random.default_rng(5)
    g = start["g_r"] + 1j * start["g_i"] + 0.1 * (rng.standard_normal((4, 32)) + 1j * rng.standard_normal((4, 32)))
    c = (start["c_r"] + 1j * start["c_i"]) * (1.0 + 0.1 * rng.standard_normal(p.ncoeffs))
    lb = LbfgsRef(Ref(p), np.float64)
    f0, grad = lb.loss_and_grad(g, c)
    # the gradient against central differences of the loss along a random direction
    d = rng.standard_normal(grad.size)
    x = lb.pack(g, c)
    h = 1e-6
    fd = (lb.loss(*lb.unpack(x + h * d, g.shape, c)) - lb.loss(*lb.unpack(x - h * d, g.shape, c))) / (2 * h)
    assert abs(fd - grad @ d) <= 1e-6 * abs(fd)
    long = lb.run(g, c, 12, history=8)
    short = lb.run(g, c, 12, history=1)
    assert long["status"] == short["status"] == 0 and long["iters"] == 12 and long["losses"][0] == f0
    assert np.all(np.diff(long["losses"]) < 0) and long["losses"][-1] < short["losses"][-1] < f0
    assert long["evals"] >= 12 and np.isfinite(long["margin"]) and long["margin"] > 0
    frozen = LbfgsRef(Ref(p), np.float64, freeze_model=True).run(g, c, 5)
    assert frozen["c"] is c and frozen["losses"][5] < f0
    stalled = lb.run(g, c, 3, max_ls=1, c1=0.999)
    assert stalled["status"] == 2 and stalled["iters"] == 0 and stalled["evals"] == 1 and stalled["v"] is g
    early = lb.run(g, c, 12, ftol=0.5)
    assert early["status"] == 1 and early["iters"] < 12 and np.all(np.isnan(early["losses"][early["iters"] + 1 :]))


# ---- the C-ABI
def test_structures_follow_the_header():
    header = open(os.path.join(ROOT, "include", "calamity_hip.h")).read()
    fields = re.search(r"typedef struct cal_lbfgs_desc \{(.*?)\} cal_lbfgs_desc;", header, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = re.findall(r"(\w+)\s*[,;]", fields)
    assert names == [n for n, _ in _lib.LbfgsDesc._fields_] == ["nsteps", "history", "max_ls", "freeze_model", "reset_moments", "reserved", "c1", "shrink",
                                                               "ftol", "curvature_eps", "slice_mask"]
    assert [t for _, t in _lib.LbfgsDesc._fields_] == [C.c_int32] * 6 + [C.c_double] * 4 + [C.c_void_p]
    assert C.sizeof(_lib.LbfgsDesc) == 64 and _lib.LbfgsDesc.c1.offset == 24 and _lib.LbfgsDesc.slice_mask.offset == 56
    fields = re.search(r"typedef struct cal_lbfgs_result \{(.*?)\} cal_lbfgs_result;", header, re.S).group(1)
    assert re.findall(r"(\w+)\s*[,;]", fields) == [n for n, _ in _lib.LbfgsResult._fields_] == ["loss_before", "loss_after", "iters", "evals", "pairs_dropped",
                                                                                                "status"]
    assert re.search(r"double loss_before, loss_after; int32_t iters, evals, pairs_dropped, status;", fields)
    assert [t for _, t in _lib.LbfgsResult._fields_] == [C.c_double] * 2 + [C.c_int32] * 4 and C.sizeof(_lib.LbfgsResult) == 32
    assert re.search(r"int cal_solver_lbfgs\(cal_solver\* s, const cal_lbfgs_desc\* desc, double\* losses_out", header)
    assert re.search(r"int cal_debug_lbfgs_coefficients\(int32_t npairs, const double\* gram, double\* delta, double\* slope\);", header)
    assert _lib.SYMBOLS["cal_solver_lbfgs"] == (C.c_int, [C.c_void_p, C.POINTER(_lib.LbfgsDesc), C.c_void_p, C.POINTER(_lib.LbfgsResult)])
    assert _lib.SYMBOLS["cal_debug_lbfgs_coefficients"] == (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)])
    assert _lib.load().cal_solver_lbfgs(None, None, None, None) == -1
    core = open(os.path.join(ROOT, "calamity_amd", "csrc", "lbfgs_core.hpp")).read()
    assert re.search(r"kLbfgsMaxHistory = 16;", core)


KEYWORDS = [("lbfgs_steps", 0), ("lbfgs_every", 0), ("lbfgs_history", 8), ("lbfgs_max_ls", 20), ("lbfgs_ftol", 0.0)]


def test_public_calls_and_the_command_line_carry_the_keywords():
    for fn in (calibration.calibrate_and_model_tensor, calibration.fit_gains_and_foregrounds):
        sig = inspect.signature(fn).parameters
        assert [(k, sig[k].default) for k in sig if k.startswith("lbfgs")] == KEYWORDS
    args = calibration.dpss_fit_argparser().parse_args(["--input_data_files", "a.uvh5", "--lbfgs_steps", "30", "--lbfgs_every", "50", "--lbfgs_history", "4",
                                                        "--lbfgs_max_ls", "7", "--lbfgs_ftol", "1e-6"])
    assert LbfgsOptions.pick(vars(args)) == LbfgsOptions(30, 50, 4, 7, 1e-6)
    none = calibration.dpss_fit_argparser().parse_args(["--input_data_files", "a.uvh5"])
    assert LbfgsOptions.pick(vars(none)) == LbfgsOptions()


# ---- the keywords
def test_options_have_the_public_names_and_defaults_and_the_others_keep_their_fields():
    assert [(f.name, f.default) for f in dataclasses.fields(LbfgsOptions)] == KEYWORDS
    assert len(dataclasses.fields(FitOptions)) == 17 and len(dataclasses.fields(GaussNewtonOptions)) == 5 and not LbfgsOptions().on
    picked = LbfgsOptions.pick(dict(lbfgs_steps=5, lbfgs_every=0, lbfgs_history=3, lbfgs_max_ls=9, lbfgs_ftol=1e-4, other=1))
    assert picked == LbfgsOptions(5, 0, 3, 9, 1e-4) and picked.on
    with pytest.raises(dataclasses.FrozenInstanceError):
        picked.lbfgs_steps = 3


BAD_NUMBERS = [dict(lbfgs_steps=-1), dict(lbfgs_steps=1.5), dict(lbfgs_steps=True), dict(lbfgs_every=-2), dict(lbfgs_history=0), dict(lbfgs_history=17),
               dict(lbfgs_history=2.5), dict(lbfgs_max_ls=0), dict(lbfgs_max_ls=1.5), dict(lbfgs_ftol=-1e-3), dict(lbfgs_ftol=np.inf), dict(lbfgs_ftol=np.nan)]


@pytest.mark.parametrize("kw", BAD_NUMBERS, ids=[f"{k}={v}" for kw in BAD_NUMBERS for k, v in kw.items()])
def test_bad_numbers_raise_even_with_the_feature_off(kw):
    with pytest.raises(ValueError, match=next(iter(kw))):
        LbfgsOptions(**kw).check(FitOptions())


def test_refused_combinations_raise():
    on = LbfgsOptions(lbfgs_steps=3)
    on.check(FitOptions())
    on.check(FitOptions(), GaussNewtonOptions(gauss_newton_every=4))  # (start-up iterations alone share no gap)
    LbfgsOptions().check(FitOptions(), groups_split=True)  # off: nothing to refuse
    with pytest.raises(ValueError, match="lbfgs.*device_split"):
        on.check(FitOptions(), groups_split=True)
    with pytest.raises(ValueError, match="lbfgs_steps"):
        LbfgsOptions(lbfgs_every=5).check(FitOptions())
    every = LbfgsOptions(lbfgs_steps=2, lbfgs_every=5)
    every.check(FitOptions(robust_every=5, gain_solve_every=5), GaussNewtonOptions(gauss_newton_every=5))
    for opts, newton in ((FitOptions(robust_every=4), None), (FitOptions(gain_basis_solve_every=10), None), (FitOptions(), GaussNewtonOptions(gauss_newton_every=7))):
        with pytest.raises(ValueError, match="same value"):
            every.check(opts, newton)


def test_public_calls_refuse_before_any_device_work():
    """The public functions raise from the keywords alone: nothing of their other arguments is touched."""
    never = object()
    with pytest.raises(ValueError, match="lbfgs_steps"):
        calibration.fit_gains_and_foregrounds(*[never] * 9, lbfgs_every=5)
    with pytest.raises(ValueError, match="lbfgs_history"):
        calibration.fit_gains_and_foregrounds(*[never] * 9, lbfgs_steps=5, lbfgs_history=40)
    for kw, word in ((dict(lbfgs_every=7), "lbfgs_steps"), (dict(lbfgs_steps=2, lbfgs_every=7, robust_every=3), "same value"),
                     (dict(lbfgs_steps=2, lbfgs_every=7, gauss_newton_every=3), "same value"), (dict(lbfgs_steps=2, lbfgs_max_ls=0), "lbfgs_max_ls"),
                     (dict(lbfgs_ftol=-1.0), "lbfgs_ftol")):
        with pytest.raises(ValueError, match=word):
            calibration.calibrate_and_model_tensor(never, never, **kw)


# ---- the calls drive issues
def call(n, **kw):
    return ("lbfgs", (n,), dict(dict(history=8, max_ls=20, ftol=0.0, freeze_model=False), **kw))


def test_defaults_issue_no_call_and_the_tuples_stay_as_they_are():
    script = going(7, 2)
    fake = LbfgsFake([script], nl=2)
    out = drive(fake, FitControls(lbfgs=LbfgsOptions()), 2, 0, 7, TOL, False, False)
    assert fake.log == [UNRECORDED, recorded(7)] and out.loops is script and out.lbfgs is None
    for controls in (FitControls(FitOptions()), FitControls(newton=GaussNewtonOptions()), FitControls(newton=GaussNewtonOptions(), lbfgs=LbfgsOptions())):
        out = drive(LbfgsFake([going(7, 2)], nl=2), controls, 2, 0, 7, TOL, False, False)
        assert out.newton is None and out.lbfgs is None and out.robust is None and out.nsingular is None and out.sweep_singular is None
    assert "lbfgs" not in history_entry(FitControls(), out, 0, np.dtype(np.float32))


def test_start_up_iterations_follow_the_gauss_newton_rounds():
    fake = LbfgsFake([going(4, 2)], nl=2, accept=[[1, 1]])
    opts = FitOptions(coeff_solve_rounds=1, gain_solve_sweeps=2)
    controls = FitControls(opts, GaussNewtonOptions(gauss_newton_rounds=1), LbfgsOptions(lbfgs_steps=6, lbfgs_history=3, lbfgs_max_ls=5, lbfgs_ftol=1e-7))
    out = drive(fake, controls, 2, 0, 4, TOL, False, False)
    gn, lb = out.newton, out.lbfgs
    assert [e[0] for e in fake.log] == ["solve_coeffs", "solve_gains", "gauss_newton_step", "lbfgs", "run_slices", "run_slices"]
    assert fake.log[3] == call(6, history=3, max_ls=5, ftol=1e-7) and fake.log[4] == UNRECORDED
    assert list(gn["steps"]) == [1, 1]
    assert list(lb["calls"]) == [1, 1] and list(lb["iters"]) == [6, 6] and list(lb["evals"]) == [7, 7] and lb["loss"] == [[39.0], [39.0]]
    out.newton = None  # (the entry of a fit without the steps)
    h = history_entry(controls, out, 1, np.dtype(np.float64))
    assert h["lbfgs"] == {"calls": 1, "iters": 6, "evals": 7, "loss": [39.0], "status": 0} and "gauss_newton" not in h


def test_the_iterations_of_a_gap_come_last_and_skip_the_loops_that_are_over():
    second = going(5, 3)
    second[1] = (np.arange(3, dtype=np.float64), True, 3)  # loop 1 meets the tolerance inside the second chunk
    fake = LbfgsFake([going(5, 3), second, going(2, 3)], nl=3, rows=6, accept=[[1, 1, 1], [1, 0, 0]])
    opts = FitOptions(gain_solve_every=5, coeff_solve_rounds=1, robust_every=5)
    lb = drive(fake, FitControls(opts, GaussNewtonOptions(gauss_newton_every=5), LbfgsOptions(lbfgs_steps=2, lbfgs_every=5)), 3, 2, 12, TOL, False, True).lbfgs
    names = [e[0] for e in fake.log]
    gap = ["hold_slices", "robust_weights", "solve_coeffs", "solve_gains", "gauss_newton_step", "lbfgs"]
    assert names == ["solve_coeffs", "lbfgs", "run_slices", "run_slices"] + gap + ["run_slices"] + gap + ["run_slices", "hold_slices"]
    calls = [e for e in fake.log if e[0] == "lbfgs"]
    assert calls[0] == call(2, freeze_model=True)  # (drive's own freeze_model)
    assert calls[1] == call(2, freeze_model=True, slice_mask=[1, 1, 1], reset_moments=True)
    assert calls[2] == call(2, freeze_model=True, slice_mask=[1, 0, 1], reset_moments=True)
    assert list(lb["calls"]) == [3, 2, 3] and list(lb["iters"]) == [6, 4, 6] and [len(x) for x in lb["loss"]] == [3, 2, 3] and list(lb["status"]) == [0, 0, 0]


def test_iterations_alone_chunk_the_loop():
    fake = LbfgsFake([going(4, 1), going(4, 1), going(2, 1)])
    lb = drive(fake, FitControls(lbfgs=LbfgsOptions(lbfgs_steps=3, lbfgs_every=4)), 1, 0, 10, TOL, False, False).lbfgs
    assert [e[0] for e in fake.log] == ["lbfgs", "run_slices", "run_slices", "hold_slices", "lbfgs", "run_slices", "hold_slices", "lbfgs", "run_slices",
                                        "hold_slices"]
    assert fake.log[4] == call(3, slice_mask=[1], reset_moments=True) and list(lb["calls"]) == [3]
