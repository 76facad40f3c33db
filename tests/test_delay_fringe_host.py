"""The delay / fringe-rate plane without a device: the float64 restatement (tests/delay_fringe_ref.py) against a plain numpy.fft route
along both axes and against what the plane is for (Parseval, a signal constant in time sits at rate 0, noise is white in rate); the
transform along time, the windows and the refusals of the drop-in keywords; the sharing of groups over workers; the host plan of
cal_solver_delay_fringe_spectrum through cal_debug_report_plan (calamity_amd/csrc/report_plan.hpp) against its rule restated in NumPy;
the build guard."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import test_report_plan_host as RP
from calamity_amd import _lib, batched, calibration, distributed, modeling, solver
from delay_fringe_ref import bin_groups, common_mask, restated
from delay_spectrum_ref import NAMES
from delay_spectrum_ref import restated as spectrum_restated

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F0, DF = 150e6, 400e3


def noise(rng, shape):
    """Unit complex noise: variance 1/2 per part."""
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)


def slices(rng, nb, nf, T, signal=1.0, sigma=1.0, flag_frac=0.0):
    """T nb rows: every slice holds slice 0's signal and its own noise.  (d, m, G, w, rows) with m = 0.6 of the signal and random G."""
    s = signal * noise(rng, (nb, nf))
    d = np.concatenate([s + sigma * noise(rng, (nb, nf)) for _ in range(T)])
    G = np.exp(2j * np.pi * rng.uniform(size=(T * nb, nf))) * rng.uniform(0.8, 1.2, size=(T * nb, nf))
    m = 0.6 * np.concatenate([s] * T) / G
    w = (rng.uniform(size=(T * nb, nf)) >= flag_frac).astype(np.float64)
    return d, m, G, w, np.stack([t * nb + np.arange(nb) for t in range(T)], axis=1)


def unitary(T):
    """numpy.fft's forward transform along time as an operator, divided by sqrt(T)."""
    return np.exp(-2j * np.pi * np.outer(np.arange(T), np.arange(T)) / T) / np.sqrt(T)


@pytest.mark.parametrize("T", [5, 8])
@pytest.mark.parametrize("nf", [61, 64])
def test_the_restatement_against_a_plain_fft_route_along_both_axes(nf, T):
    rng = np.random.default_rng(nf + T)
    d, m, G, w, rows = slices(rng, 9, nf, T, flag_frac=0.03)
    scale = rng.uniform(0.5, 2.0, size=rows.shape)
    op = np.exp(-2j * np.pi * np.outer(np.arange(nf), np.arange(nf)) / nf)  # numpy.fft's forward transform as an operator
    opt = unitary(T) * np.sqrt(T)
    ref = restated(d, m, G, w, op, np.ones(nf), rows, opt, scale)
    common = common_mask(w, rows)
    assert common.sum(axis=1).min() * 3 >= nf
    q = {"data": d, "model": G * m, "resid": d - G * m}
    n = common.sum(axis=1)[:, None, None]
    for k in NAMES:
        Y = scale[:, :, None] * np.fft.fft(np.where(common[:, None, :], q[k][rows], 0.0), axis=2)  # [groups, T, delays]
        Z = np.fft.fft(Y, axis=1)  # along time
        np.testing.assert_allclose(ref["per_group"][k], np.abs(Z) ** 2 / n, rtol=0, atol=1e-11 * np.max(np.abs(Z)) ** 2 / n.min())
    np.testing.assert_array_equal(ref["norm_grp"], common.sum(axis=1))


@pytest.mark.parametrize("T", [5, 8])
def test_parseval_over_all_rates(T):
    """With the untapered unitary opt and all rates the powers of the rates add up to the T single-row powers under the common mask."""
    rng = np.random.default_rng(T)
    nb, nf = 6, 61
    d, m, G, w, rows = slices(rng, nb, nf, T, flag_frac=0.03)
    op, norm_f, _ = modeling.delay_transform(F0 + DF * np.arange(nf))
    ref = restated(d, m, G, w, op, norm_f, rows, unitary(T))
    common = common_mask(w, rows).astype(np.float64)
    for k in NAMES:
        single = sum(spectrum_restated(d[rows[:, t]], m[rows[:, t]], G[rows[:, t]], common, op, norm_f)["per_baseline"][k] for t in range(T))
        np.testing.assert_allclose(ref["per_group"][k].sum(axis=1), single, rtol=1e-12, atol=0)


def test_a_signal_constant_in_time_sits_at_rate_zero():
    rng = np.random.default_rng(1)
    nb, nf, T = 6, 61, 8
    d, m, G, w, rows = slices(rng, nb, nf, T, sigma=0.0, flag_frac=0.03)
    G[:], m[:] = np.tile(G[:nb], (T, 1)), np.tile(m[:nb], (T, 1))  # the same gains and model at every time: every quantity is constant
    op, norm_f, _ = modeling.delay_transform(F0 + DF * np.arange(nf))
    opt, rates = modeling.fringe_rate_transform(T, 10.0, taper="none")
    zero = int(np.flatnonzero(rates == 0)[0])
    ref = restated(d, m, G, w, op, norm_f, rows, opt * np.sqrt(T))  # plain sums over time
    common = common_mask(w, rows).astype(np.float64)
    auto = spectrum_restated(d[:nb], m[:nb], G[:nb], common, op, norm_f)
    for k in NAMES:
        P = ref["per_group"][k]
        np.testing.assert_allclose(P[:, zero], T * T * auto["per_baseline"][k], rtol=1e-12, atol=0)  # |T X|^2 / norm
        others = np.delete(P, zero, axis=1)
        assert np.all(others <= 1e-24 * P[:, zero].max())
    # with the unit-norm operator: T |X|^2 / norm
    unit = restated(d, m, G, w, op, norm_f, rows, opt)
    np.testing.assert_allclose(unit["per_group"]["data"][:, zero], T * auto["per_baseline"]["data"], rtol=1e-12, atol=0)


def test_independent_noise_is_white_in_fringe_rate():
    """78 groups x 61 channels of independent unit complex noise, 8 times, no flags, no tapers, all delays and rates: per sample the
    power is exponential with mean 1 and variance 1, so the mean over the N = 78 x 61 samples of a rate lies within 5 / sqrt(N) of 1."""
    nb, nf, T = 78, 61, 8
    N = nb * nf
    rng = np.random.default_rng(0)
    d = noise(rng, (T * nb, nf))
    op, norm_f, _ = modeling.delay_transform(F0 + DF * np.arange(nf), taper="none")
    opt, _ = modeling.fringe_rate_transform(T, 10.0, taper="none")
    rows = np.stack([t * nb + np.arange(nb) for t in range(T)], axis=1)
    ref = restated(d, np.zeros_like(d), np.ones_like(d), np.ones((T * nb, nf)), op, norm_f, rows, opt)
    means = ref["per_group"]["data"].mean(axis=(0, 2))
    print("mean power per rate " + " ".join(f"{v:.4f}" for v in means) + f" (bound {5 / np.sqrt(N):.4f})")
    assert means.shape == (T,) and np.all(np.abs(means - 1.0) < 5.0 / np.sqrt(N))
    # and under a taper along time, normalised by fringe_rate_transform
    opt, _ = modeling.fringe_rate_transform(T, 10.0, taper="bh4")
    means = restated(d, np.zeros_like(d), np.ones_like(d), np.ones((T * nb, nf)), op, norm_f, rows, opt)["per_group"]["data"].mean(axis=(0, 2))
    assert np.all(np.abs(means - 1.0) < 5.0 / np.sqrt(N))  # (neighbouring rates are correlated; each rate's mean is over independent samples)


def test_only_the_common_channels_enter_and_empty_groups_enter_no_bin():
    rng = np.random.default_rng(2)
    nb, nf, T = 4, 61, 3
    d, m, G, w, rows = slices(rng, nb, nf, T)
    w[0, 5:20] = 0.0          # flagged at time 0 only
    w[2 * nb, 30:41] = 0.0    # at time 2 only
    w[nb + 1, :] = 0.0        # one row wholly flagged
    w[2, 0::2], w[nb + 2, 1::2] = 0.0, 0.0  # disjoint masks
    op, norm_f, _ = modeling.delay_transform(F0 + DF * np.arange(nf))
    opt, _ = modeling.fringe_rate_transform(T, 10.0)
    bins = np.zeros(nb, dtype=np.int32)
    ref = restated(d, m, G, w, op, norm_f, rows, opt, bin_of_group=bins, nbins=1)
    gone = np.zeros(nf, bool)
    gone[5:20] = gone[30:41] = True
    d2, m2 = d.copy(), m.copy()
    d2[rows[0][:, None], gone] = 0.0
    m2[rows[0][:, None], gone] = 0.0
    by_hand = restated(d2, m2, G, np.ones_like(w), op, norm_f, rows[:1], opt)
    assert ref["norm_grp"][0] == norm_f[~gone].sum()
    for k in NAMES:
        np.testing.assert_allclose(ref["per_group"][k][0] * ref["norm_grp"][0], by_hand["per_group"][k][0] * by_hand["norm_grp"][0], rtol=1e-12, atol=1e-18)
        assert not np.any(ref["per_group"][k][1]) and not np.any(ref["per_group"][k][2])
    assert ref["norm_grp"][1] == 0 and ref["norm_grp"][2] == 0 and list(ref["count_bin"]) == [2]
    own = bin_groups(ref["per_group"], ref["norm_grp"], bins, 1)
    np.testing.assert_array_equal(own["resid"][0], ref["per_group"]["resid"][0] + ref["per_group"]["resid"][3])


# ---- the transform along time -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("taper", ["bh4", "none"])
@pytest.mark.parametrize("T", [2, 3, 8, 64])
def test_the_transform_along_time(T, taper):
    dt = 10.7
    opt, rates = modeling.fringe_rate_transform(T, dt, taper=taper)
    assert opt.shape == (T, T) and opt.dtype == np.complex128 and rates.shape == (T,)
    np.testing.assert_allclose(np.sum(np.abs(opt) ** 2, axis=0), 1.0, rtol=1e-14)  # white noise of unit variance: expected power 1 per rate
    np.testing.assert_allclose(rates, (np.arange(T) - T // 2) / (T * dt), rtol=1e-15)
    assert np.all(np.diff(rates) > 0) and rates[T // 2] == 0
    w = modeling.delay_taper(T, taper)
    y = noise(np.random.default_rng(T), T)
    np.testing.assert_allclose(y @ opt, np.fft.fftshift(np.fft.fft(w * y)) / np.sqrt(np.sum(w * w)), rtol=0, atol=1e-13)
    some, r2 = modeling.fringe_rate_transform(T, dt, taper=taper, rates=rates[[0, T - 1]])
    np.testing.assert_allclose(some, opt[:, [0, T - 1]], rtol=0, atol=1e-13)
    np.testing.assert_array_equal(r2, rates[[0, T - 1]])
    for bad in (dict(ntimes=0), dict(ntimes=65), dict(dt=0.0), dict(dt=np.nan), dict(taper="hann"), dict(rates=[]), dict(rates=[np.inf])):
        with pytest.raises(ValueError):
            modeling.fringe_rate_transform(**{"ntimes": T, "dt": dt, **bad})


# ---- the drop-in keywords -----------------------------------------------------------------------------------------------------------------
def test_the_windows():
    win = calibration.delay_fringe_windows
    assert win([0] * 6, [0, 1, 2, 3, 4, 5], 3) == [(0, 1, 2), (3, 4, 5)]
    assert win([0] * 7, range(7), 3) == [(0, 1, 2), (3, 4, 5)]  # a remainder: the last slice belongs to no window
    assert win([0, 0, 0, 1, 1, 1], [0, 1, 2, 0, 1, 2], 3) == [(0, 1, 2), (3, 4, 5)]
    assert win([0, 0, 1, 1, 1, 1], [1, 2, 0, 1, 2, 3], 3) == [(2, 3, 4)]  # mixed polarizations: a window does not cross the boundary
    assert win([0] * 6, [0, 1, 3, 4, 5, 6], 3) == [(2, 3, 4)]  # a gap in time_index (a skipped slice): the run starts again behind it
    assert win([0] * 5, [0, 2, 3, 4, 6], 3) == [(1, 2, 3)]
    assert win([0] * 4, [0, 1, 2, 3], 2) == [(0, 1), (2, 3)]  # windows do not overlap
    assert win([0, 0], [0, 1], 3) == [] and win([], [], 2) == [] and win([0, 0], [0, 2], 2) == []
    times = 2459000.0 + 1e-4 * np.arange(8)
    assert win([0] * 6, range(6), 3, times, 1e-4) == [(0, 1, 2), (3, 4, 5)]
    uneven = times.copy()
    uneven[4] += 0.05e-4  # 5 % of the spacing
    with pytest.raises(ValueError, match="not evenly spaced") as err:
        win([0] * 6, range(6), 3, uneven, 1e-4)
    assert repr(float(uneven[4])) in str(err.value)  # the times are named
    assert win([0] * 3, range(3), 3, uneven, 1e-4) == [(0, 1, 2)]  # the first window is even
    uneven[4] = times[4] + 0.005e-4  # half a per cent: within the 1 %
    assert win([0] * 6, range(6), 3, uneven, 1e-4) == [(0, 1, 2), (3, 4, 5)]
    setup = calibration.delay_fringe_setup(times, 4, "bh4", True)
    assert setup["ntimes"] == 4 and setup["per_group"] is True and setup["opt"].shape == (4, 4)
    np.testing.assert_allclose(setup["dt"], 1e-4, rtol=4 * np.spacing(2459000.0) / 1e-4)  # (a Julian day resolves 4.7e-10 days)
    np.testing.assert_allclose(setup["rates_hz"], (np.arange(4) - 2) / (4 * setup["dt"] * 86400.0), rtol=1e-12)
    dspec = dict(nbins=2, bin_of_bl=np.array([0, 1, 1], dtype=np.int32))
    rows, scale, bins = calibration.delay_fringe_rows([(0, 1, 2), (4, 5, 6)], dspec, [2.0, 3.0, 9.0, 5.0, 7.0, 1.0, 4.0], 3)
    np.testing.assert_array_equal(rows, [[0, 3, 6], [1, 4, 7], [2, 5, 8], [12, 15, 18], [13, 16, 19], [14, 17, 20]])
    np.testing.assert_array_equal(scale, [[2.0, 3.0, 9.0]] * 3 + [[7.0, 1.0, 4.0]] * 3)
    np.testing.assert_array_equal(bins, [0, 1, 1, 2, 3, 3])
    assert rows.dtype == np.int32 and bins.dtype == np.int32


CALLS = ["calibrate_and_model_tensor", "calibrate_and_model_mixed", "calibrate_and_model_dpss", "read_calibrate_and_model_dpss"]
ON = dict(delay_fringe_spectrum=True, delay_spectrum=True)


@pytest.mark.parametrize("bad", [dict(delay_fringe_spectrum=True), dict(ON, batch_slices=False), dict(ON, batch_slices=7),
                                 dict(ON, delay_fringe_times=3, batch_slices=2), dict(ON, delay_spectrum="baselines", init_guesses_from_previous_time_step=True),
                                 dict(ON, delay_fringe_times=1), dict(ON, delay_fringe_times=65), dict(ON, delay_fringe_times=2.5),
                                 dict(ON, delay_fringe_taper="hann"), dict(delay_fringe_spectrum="yes", delay_spectrum=True)])
@pytest.mark.parametrize("name", CALLS)
def test_bad_keywords_are_refused_before_anything_is_touched(name, bad):
    call = getattr(calibration, name)
    with pytest.raises(ValueError, match="delay_fringe_spectrum"):
        call(None, {}, **bad) if name == "calibrate_and_model_tensor" else call(None, **bad)  # (no data, no device: the check comes first)


@pytest.mark.parametrize("name", CALLS)
def test_the_keywords_are_off_by_default_in_their_place_and_python_keywords_only(name):
    params = inspect.signature(getattr(calibration, name)).parameters
    assert params["delay_fringe_spectrum"].default is False and params["delay_fringe_times"].default == 8 and params["delay_fringe_taper"].default == "bh4"
    names = list(params)
    at = names.index("delay_cross_spectrum")
    assert names[at - 3 : at] == ["delay_fringe_spectrum", "delay_fringe_times", "delay_fringe_taper"]  # directly in front of delay_cross_spectrum
    assert not any(n.startswith("delay_spectrum") and "fringe" in n for n in names)
    from calamity_amd.fit_loop import FitControls

    assert not any("fringe" in f for f in FitControls().keywords())
    assert not any("fringe" in a.dest for a in calibration.dpss_fit_argparser()._actions)


def test_the_methods_and_the_binding():
    for cls in (solver.HipFitSolver, batched.SliceBatchFitter):
        params = inspect.signature(cls.delay_fringe_spectrum).parameters
        assert list(params)[1:] == ["op", "norm_f", "rows", "opt", "scale", "what", "calibrated", "bin_of_group", "nbins", "per_group", "g_r", "g_i"]
        assert params["scale"].default is None and params["what"].default == ("data", "model", "resid") and params["calibrated"].default is False
        assert params["nbins"].default == 0 and params["per_group"].default is False and params["bin_of_group"].default is None
    names = [f[0] for f in _lib.DelayFringeDesc._fields_]
    assert names == ["ndelays", "what", "calibrated", "ngroups", "ntimes", "nrates", "rows", "scale", "nbins", "bin_of_group", "op_r", "op_i", "norm_f",
                     "opt_r", "opt_i"]
    text = open(os.path.join(ROOT, "include", "calamity_hip.h")).read()
    fields = text.split("typedef struct cal_delay_fringe_desc {")[1].split("}")[0]
    assert re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", fields)) == names
    for word in ("cal_solver_delay_fringe_spectrum(", "the COMMON mask of all T rows", "ONE all-reduce of\n * nwhat nbins nrates ndelays + nbins doubles",
                 "what = 70 .. 76", "const struct cal_delay_fringe_desc* fringe", "enters no bin", "there is no norm_t",
                 "re += (opt_r yr - opt_i yi) and im += (opt_r yi + opt_i yr)", "not the weights as set"):
        assert word in text, word
    assert hasattr(_lib.load(), "cal_solver_delay_fringe_spectrum")
    # the plan descriptions: each adds its pointer behind its parent's fields
    assert [f[0] for f in _lib.CrossReportPlanDesc._fields_] == ["cross"] and [f[0] for f in _lib.FringeReportPlanDesc._fields_] == ["fringe"]
    assert issubclass(_lib.FringeReportPlanDesc, _lib.CrossReportPlanDesc) and issubclass(_lib.CrossReportPlanDesc, _lib.ReportPlanDesc)
    plan = text.split("typedef struct cal_report_plan_desc {")[1].split("}")[0]
    assert re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", plan)) == [f[0] for f in _lib.ReportPlanDesc._fields_] + ["cross", "fringe"]
    spec = distributed.exchange_spec(7, 64, delay_fringe=(3, 5, 8, 37))
    assert spec["delay_fringe_f64"] == 3 * 5 * 8 * 37 + 5
    assert {k: v for k, v in spec.items() if k != "delay_fringe_f64"} == distributed.exchange_spec(7, 64)
    assert "delay_fringe_f64" not in distributed.exchange_spec(7, 64, delay_cross=(2, 3, 5, 37))


def test_groups_are_shared_out_over_the_workers_that_hold_all_their_rows():
    rows = [np.array([4, 5, 0, 1]), np.array([2, 3, 6, 7])]  # two workers, their global rows in local order
    groups = np.array([[0, 4, 1], [2, 6, 3], [1, 5, 5], [3, 3, 3], [7, 6, 2]])
    sel, local = batched.split_groups(groups, rows, 8)
    np.testing.assert_array_equal(sel[0], [0, 2])
    np.testing.assert_array_equal(sel[1], [1, 3, 4])
    np.testing.assert_array_equal(local[0], [[2, 0, 3], [3, 1, 1]])
    np.testing.assert_array_equal(local[1], [[0, 2, 1], [1, 1, 1], [3, 2, 0]])
    assert local[0].dtype == np.int32
    with pytest.raises(ValueError, match="several workers"):
        batched.split_groups(np.array([[0, 4, 1], [1, 5, 2]]), rows, 8)
    with pytest.raises(ValueError, match="holds no group"):
        batched.split_groups(np.array([[0, 4, 5]]), rows, 8)


# ---- the plan -----------------------------------------------------------------------------------------------------------------------------
FRINGE = {70: ("scalars", np.int64), 71: ("bin_ent", np.int32), 72: ("chunk_ptr", np.int32), 73: ("image", None), 74: ("norm_f", np.float64),
          75: ("scale", np.float64), 76: ("opt", np.float64)}
SCALARS = "nq xpitch ndpad cgroups nchunks n_x n_ypow n_out".split()


def fringe_desc(dtype, op, norm_f, rows, opt, scale=None, what=7, nbins=0, bin_of_group=None, ngroups=None, ntimes=None, nrates=None, opt_i=True):
    arr = lambda a, t: None if a is None else np.ascontiguousarray(a, t)  # noqa: E731
    keep = [arr(op.real, dtype), arr(op.imag, dtype), arr(norm_f, np.float64), arr(bin_of_group, np.int32), arr(rows, np.int32), arr(scale, np.float64),
            None if opt is None else arr(np.asarray(opt).real, np.float64), None if opt is None or not opt_i else arr(np.asarray(opt).imag, np.float64)]
    ng = np.shape(rows)[0] if ngroups is None else ngroups
    nt = np.shape(rows)[1] if ntimes is None else ntimes
    nr = np.shape(opt)[1] if nrates is None else nrates
    return _lib.DelayFringeDesc(op.shape[1], what, 0, ng, nt, nr, RP.ptr(keep[4]), RP.ptr(keep[5]), nbins, RP.ptr(keep[3]), RP.ptr(keep[0]), RP.ptr(keep[1]),
                                RP.ptr(keep[2]), RP.ptr(keep[6]), RP.ptr(keep[7])), keep


def fringe_plan(prob, dtype, op, norm_f, rows, opt, bound=0, **kw):
    desc, keep = fringe_desc(dtype, op, norm_f, rows, opt, **kw)
    report = _lib.FringeReportPlanDesc(fringe=C.pointer(desc), scratch_bytes=bound)
    out = {}
    for what, (name, dt) in FRINGE.items():
        rc, got, _ = RP.raw_call(prob, dtype, report, what)
        _lib.check(rc)
        out[name] = got.view(dtype if dt is None else dt).copy()
    return out


def fringe_rule(ngroups, T, nr, fpad, dtype, nd, what=7, nbins=0, bin_of_group=None, bound=0):
    size = np.dtype(dtype).itemsize
    nq = bin(what).count("1")
    xpitch, ndpad = -(-fpad // RP.DS_STEP) * RP.DS_STEP, -(-nd // RP.DS_COLS) * RP.DS_COLS
    group_bytes = nq * 2 * T * xpitch * size + nq * 2 * T * nd * 8 + nq * nr * nd * 8
    cgroups = min(max(1, (bound or RP.DEFAULT_BOUND) // group_bytes), ngroups)
    nchunks = -(-ngroups // cgroups)
    lists = [np.flatnonzero(np.asarray(bin_of_group) == n) for n in range(nbins)]  # ascending groups
    start = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(int)
    ptr = np.zeros((nchunks, nbins, 2), np.int32)
    for c in range(nchunks):
        for n in range(nbins):
            ptr[c, n] = [start[n] + np.searchsorted(lists[n], c * cgroups), start[n] + np.searchsorted(lists[n], min(ngroups, (c + 1) * cgroups))]
    scalars = [nq, xpitch, ndpad, cgroups, nchunks, nq * 2 * cgroups * T * xpitch, nq * 2 * cgroups * T * nd + nq * cgroups * nr * nd,
               ngroups + nq * nbins * nr * nd + nbins]
    return dict(scalars=np.asarray(scalars, np.int64), bin_ent=np.concatenate(lists).astype(np.int32) if nbins else np.zeros(0, np.int32), chunk_ptr=ptr.ravel())


@pytest.mark.parametrize("dtype", RP.DTYPES)
@pytest.mark.parametrize("ngroups,T,bound_groups", [(300, 3, 0), (300, 3, 200), (300, 3, 7), (300, 3, 1), (5, 17, -1), (1, 64, 0)])
def test_the_plan_cuts_whole_groups_and_never_below_one(ngroups, T, bound_groups, dtype):
    prob = RP.rows22()
    fpad, nd, nr = RP.fpad_of(prob, dtype), 37, min(T, 5)
    rng = np.random.default_rng(3)
    op, norm_f = rng.standard_normal((prob.nfreqs, nd)) + 1j * rng.standard_normal((prob.nfreqs, nd)), rng.uniform(size=prob.nfreqs)
    opt = rng.standard_normal((T, nr)) + 1j * rng.standard_normal((T, nr))
    rows = rng.integers(0, prob.nbls, size=(ngroups, T)).astype(np.int32)
    bins = (np.arange(ngroups) % 4 - (np.arange(ngroups) % 9 == 0)).astype(np.int32)  # -1 .. 3; bin 4 stays empty
    xpitch = -(-fpad // 32) * 32
    per_group = 3 * 2 * T * xpitch * np.dtype(dtype).itemsize + 3 * 2 * T * nd * 8 + 3 * nr * nd * 8
    bound = 1 if bound_groups < 0 else bound_groups * per_group + (per_group // 2 if bound_groups else 0)  # (-1: a bound of one byte)
    got = fringe_plan(prob, dtype, op, norm_f, rows, opt, bound=bound, nbins=5, bin_of_group=bins)
    want = fringe_rule(ngroups, T, nr, fpad, dtype, nd, nbins=5, bin_of_group=bins, bound=bound)
    for k in ("scalars", "bin_ent", "chunk_ptr"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    s = dict(zip(SCALARS, got["scalars"]))
    assert s["cgroups"] == {0: ngroups, 200: 200, 7: 7, 1: 1, -1: 1}[bound_groups] and s["cgroups"] >= 1
    assert s["nchunks"] == -(-ngroups // s["cgroups"])
    ptr = got["chunk_ptr"].reshape(s["nchunks"], 5, 2)
    for n in range(5):  # every bin's pieces over the chunks tile its list
        assert np.all(ptr[1:, n, 0] == ptr[:-1, n, 1]) and ptr[-1, n, 1] - ptr[0, n, 0] == np.count_nonzero(bins == n)
    assert ptr[0, 4, 0] == ptr[-1, 4, 1]  # the empty bin
    image = got["image"].reshape(2, s["xpitch"], s["ndpad"])  # the operator image and norm_f are the spectrum's
    np.testing.assert_array_equal(image[0, : prob.nfreqs, :nd], op.real.astype(dtype))
    np.testing.assert_array_equal(image[1, : prob.nfreqs, :nd], op.imag.astype(dtype))
    assert not np.any(image[:, prob.nfreqs :]) and not np.any(image[:, :, nd:])
    np.testing.assert_array_equal(got["norm_f"], np.concatenate([norm_f, np.zeros(s["xpitch"] - prob.nfreqs)]))
    np.testing.assert_array_equal(got["scale"], np.ones(ngroups * T))  # no scales are ones
    np.testing.assert_array_equal(got["opt"], np.concatenate([opt.real.ravel(), opt.imag.ravel()]))
    scale = rng.uniform(0.5, 2.0, size=(ngroups, T))
    np.testing.assert_array_equal(fringe_plan(prob, dtype, op, norm_f, rows, opt, scale=scale, what=5)["scale"], scale.ravel())
    one = dict(zip(SCALARS, fringe_plan(prob, dtype, op, norm_f, rows, opt, what=5)["scalars"]))
    assert (one["nq"], one["n_out"]) == (2, ngroups)


def test_the_planner_refuses_what_the_call_refuses():
    prob = RP.rows22()
    nd = 8
    op, norm_f = np.zeros((prob.nfreqs, nd), np.complex128), np.ones(prob.nfreqs)
    rows = np.array([[0, 1], [2, 21]], np.int32)
    opt = np.array([[1.0, 1.0], [1.0, -1.0]], np.complex128)

    def refused(selector=70, bound=0, **kw):
        desc, keep = fringe_desc(np.float32, op, norm_f, **{"rows": rows, "opt": opt, **kw})
        rc, _, _ = RP.raw_call(prob, np.float32, _lib.FringeReportPlanDesc(fringe=C.pointer(desc), scratch_bytes=bound), selector)
        return rc, _lib.load().cal_last_error().decode()

    assert refused()[0] == 0
    INV = _lib.CAL_ERR_INVALID
    bad_opt = opt.copy()
    bad_opt[1, 0] = np.nan
    bad_imag = opt.copy()
    bad_imag[1, 0] = complex(1.0, np.inf)
    wide = np.zeros((2, 65), np.int32)
    for kw, text in ((dict(ngroups=0), "delay_fringe_spectrum: ngroups = 0 (at least 1)"),
                     (dict(ntimes=0), "delay_fringe_spectrum: ntimes = 0 lies outside [1, 64]"),
                     (dict(rows=wide, opt=np.ones((65, 2))), "delay_fringe_spectrum: ntimes = 65 lies outside [1, 64]"),
                     (dict(nrates=0), "delay_fringe_spectrum: nrates = 0 lies outside [1, 64]"),
                     (dict(opt=np.ones((2, 65))), "delay_fringe_spectrum: nrates = 65 lies outside [1, 64]"),
                     (dict(rows=None, ngroups=2, ntimes=2), "delay_fringe_spectrum: null rows"),
                     (dict(opt=None, nrates=2), "delay_fringe_spectrum: null opt"), (dict(opt_i=False), "delay_fringe_spectrum: null opt"),
                     (dict(rows=np.array([[0, 1], [2, 22]])), "delay_fringe_spectrum: rows[1][1] = 22 lies outside [0, 22)"),
                     (dict(rows=np.array([[-1, 1]])), "delay_fringe_spectrum: rows[0][0] = -1 lies outside [0, 22)"),
                     (dict(scale=np.array([[1.0, 1.0], [np.inf, 1.0]])), "delay_fringe_spectrum: scale[1][0] is not finite"),
                     (dict(scale=np.array([[1.0, np.nan], [1.0, 1.0]])), "delay_fringe_spectrum: scale[0][1] is not finite"),
                     (dict(opt=bad_opt), "delay_fringe_spectrum: opt[1][0] is not finite"),
                     (dict(opt=bad_imag), "delay_fringe_spectrum: opt[1][0] is not finite"),
                     (dict(nbins=2, bin_of_group=[0, 2]), "delay_fringe_spectrum: bin_of_group[1] = 2 lies outside [-1, 2)"),
                     (dict(nbins=2, bin_of_group=[-2, 0]), "delay_fringe_spectrum: bin_of_group[0] = -2 lies outside [-1, 2)")):
        rc, msg = refused(**kw)
        assert rc == INV and msg == text, (kw, msg)
    for kw in (dict(what=0), dict(what=8), dict(nbins=-1), dict(nbins=2), dict(bin_of_group=[0, 0])):
        rc, msg = refused(**kw)
        assert rc == INV and "takes a fringe description cal_solver_delay_fringe_spectrum would plan for" in msg, (kw, msg)
    assert refused(bound=-1)[0] == INV
    rc, _, _ = RP.raw_call(prob, np.float32, _lib.FringeReportPlanDesc(), 70)  # no description
    assert rc == INV
    assert refused(selector=77)[0] == INV and refused(selector=69)[0] == INV  # the range is 70 .. 76


# ---- the build guard ----------------------------------------------------------------------------------------------------------------------
def test_the_build_guard_refuses_a_spilling_fringe_kernel():
    script = os.path.join(ROOT, "calamity_amd", "csrc", "check_resources.py")

    def remarks(name, scratch, vspill, occ=2):
        return (f"./x.hpp:1:1: remark: Function Name: {name} [-Rpass-analysis=kernel-resource-usage]\n"
                f"./x.hpp:1:1: remark:     VGPRs: 250 [-Rpass-analysis=kernel-resource-usage]\n"
                f"./x.hpp:1:1: remark:     ScratchSize [bytes/lane]: {scratch} [-Rpass-analysis=kernel-resource-usage]\n"
                f"./x.hpp:1:1: remark:     Occupancy [waves/SIMD]: {occ} [-Rpass-analysis=kernel-resource-usage]\n"
                f"./x.hpp:1:1: remark:     SGPRs Spill: 0 [-Rpass-analysis=kernel-resource-usage]\n"
                f"./x.hpp:1:1: remark:     VGPRs Spill: {vspill} [-Rpass-analysis=kernel-resource-usage]\n")

    def run(text):
        return subprocess.run([sys.executable, script], input=text, capture_output=True, text=True)

    dense = remarks("_ZN4calk18fused_dense_kernelILb1EEEvNS_8MfmaArgsE", 0, 0)
    names = {f"{k}<{t}>": f"_ZN4calk{len(k)}{k}I{t}EEvPKT_" for k in ("dfringe_rows_kernel", "dfringe_transform_kernel") for t in "fd"}
    names["dfringe_time_kernel"] = "_ZN4calk19dfringe_time_kernelEPKdS1_S1_S1_iiiiPd"
    assert run(dense + "".join(remarks(n, 0, 0) for n in names.values())).returncode == 0
    for k, n in names.items():
        for scratch, vspill in ((16, 0), (0, 4)):
            bad = run(dense + remarks(n, scratch, vspill))
            assert bad.returncode != 0 and k.split("<")[0] in bad.stdout + bad.stderr, (k, scratch, vspill)
    for k in ("dfringe_transform_kernel<f>", "dfringe_transform_kernel<d>", "dfringe_time_kernel"):
        low = run(dense + remarks(names[k], 0, 0, occ=1))
        assert low.returncode != 0 and "occupancy" in low.stdout + low.stderr
    for t in "fd":
        assert run(dense + remarks(names[f"dfringe_rows_kernel<{t}>"], 0, 0, occ=1)).returncode == 0  # no occupancy rule for the rows kernel
    # the transforms whose loop the fringe transform shares keep their own rules
    for other in ("_ZN4calk22dspec_transform_kernelIfEEvPKT_", "_ZN4calk23dcross_transform_kernelIfEEvPKT_"):
        assert run(dense + remarks(other, 0, 4)).returncode != 0 and run(dense + remarks(other, 0, 0, occ=1)).returncode != 0
