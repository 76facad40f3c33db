"""The cross spectrum of paired times without a device: the float64 restatement (tests/delay_cross_ref.py) against a plain numpy.fft
route and against what the estimator is for (a common signal survives, independent noise averages out, the half difference measures
the noise); the pairing rule and the refusals of the drop-in keyword; the host plan of cal_solver_delay_cross_spectrum through
cal_debug_report_plan (calamity_amd/csrc/report_plan.hpp) against its rule restated in NumPy; the build guard."""
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
from delay_cross_ref import STATS, bin_pairs, restated
from delay_spectrum_ref import NAMES
from delay_spectrum_ref import restated as spectrum_restated

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DC_PAIRS = 64  # kDcPairs (delay_cross_kernels.hpp)
F0, DF = 150e6, 400e3


def noise(rng, shape):
    """Unit complex noise: variance 1/2 per part."""
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)


def two_slices(rng, nb, nf, signal=1.0, sigma=1.0, flag_frac=0.0):
    """2 nb rows: slice 1 holds slice 0's signal and its own noise.  (d, m, G, w, pairs) with m = 0.6 of the signal and random G."""
    s = signal * noise(rng, (nb, nf))
    d = np.concatenate([s + sigma * noise(rng, (nb, nf)), s + sigma * noise(rng, (nb, nf))])
    G = np.exp(2j * np.pi * rng.uniform(size=(2 * nb, nf))) * rng.uniform(0.8, 1.2, size=(2 * nb, nf))
    m = 0.6 * np.concatenate([s, s]) / G
    w = (rng.uniform(size=(2 * nb, nf)) >= flag_frac).astype(np.float64)
    return d, m, G, w, np.stack([np.arange(nb), nb + np.arange(nb)], axis=1)


@pytest.mark.parametrize("nf", [61, 64])
def test_the_restatement_against_a_plain_fft_route(nf):
    rng = np.random.default_rng(nf)
    d, m, G, w, pairs = two_slices(rng, 9, nf, flag_frac=0.1)
    scale = rng.uniform(0.5, 2.0, size=pairs.shape)
    op = np.exp(-2j * np.pi * np.outer(np.arange(nf), np.arange(nf)) / nf)  # numpy.fft's forward transform as an operator
    norm_f = np.ones(nf)
    ref = restated(d, m, G, w, op, norm_f, pairs, scale)
    common = (w[pairs[:, 0]] != 0) & (w[pairs[:, 1]] != 0)
    q = {"data": d, "model": G * m, "resid": d - G * m}
    for k in NAMES:
        Y0 = scale[:, :1] * np.fft.fft(np.where(common, q[k][pairs[:, 0]], 0.0), axis=1)
        Y1 = scale[:, 1:] * np.fft.fft(np.where(common, q[k][pairs[:, 1]], 0.0), axis=1)
        n = common.sum(axis=1)[:, None]
        np.testing.assert_allclose(ref["per_pair"]["cross"][k], (Y0 * np.conj(Y1)).real / n, rtol=0, atol=1e-11 * np.max(np.abs(Y0)) ** 2 / n.min())
        np.testing.assert_allclose(ref["per_pair"]["diff"][k], np.abs(Y0 - Y1) ** 2 / (2 * n), rtol=0, atol=1e-11 * np.max(np.abs(Y0)) ** 2 / n.min())
    np.testing.assert_array_equal(ref["norm_pair"], common.sum(axis=1))


def test_a_common_signal_without_noise_survives_whole():
    rng = np.random.default_rng(1)
    nb, nf = 6, 61
    d, m, G, w, pairs = two_slices(rng, nb, nf, sigma=0.0, flag_frac=0.1)
    G[nb:], m[nb:] = G[:nb], m[:nb]  # the same gains and model on both sides: every quantity is common
    op, norm_f, _ = modeling.delay_transform(F0 + DF * np.arange(nf))
    ref = restated(d, m, G, w, op, norm_f, pairs)
    common = ((w[:nb] != 0) & (w[nb:] != 0)).astype(np.float64)
    auto = spectrum_restated(d[:nb], m[:nb], G[:nb], common, op, norm_f)  # the auto power under the COMMON mask
    for k in NAMES:
        # (Re Y^2 + Im Y^2 here, |Y|^2 through hypot there: a few roundings of float64 apart)
        np.testing.assert_allclose(ref["per_pair"]["cross"][k], auto["per_baseline"][k], rtol=8 * 2.0 ** -53, atol=0)
        assert not np.any(ref["per_pair"]["diff"][k])
    np.testing.assert_array_equal(ref["norm_pair"], auto["norm_bl"])


def test_independent_noise_averages_out_of_the_cross_power_and_the_half_difference_measures_it():
    """78 pairs x 61 channels of independent unit complex noise, no flags, no taper, all delays: per sample the cross power has mean 0
    and variance 1/2, the half-difference power mean 1 and variance 1.  (Seed 0: 0.0084 and 0.9838 against the bounds 0.0513 and 0.0725.)"""
    nb, nf = 78, 61
    N = nb * nf
    rng = np.random.default_rng(0)
    d = noise(rng, (2 * nb, nf))
    op, norm_f, _ = modeling.delay_transform(F0 + DF * np.arange(nf), taper="none")
    assert op.shape == (nf, nf) and np.all(norm_f == 1.0)
    pairs = np.stack([np.arange(nb), nb + np.arange(nb)], axis=1)
    ref = restated(d, np.zeros_like(d), np.ones_like(d), np.ones((2 * nb, nf)), op, norm_f, pairs)
    cross, diff = ref["per_pair"]["cross"]["data"], ref["per_pair"]["diff"]["data"]
    print(f"mean cross {cross.mean():.4f} (bound {5 * np.sqrt(1 / (2 * N)):.4f})  mean diff {diff.mean():.4f} (bound {5 / np.sqrt(N):.4f})")
    assert abs(cross.mean()) < 5.0 * np.sqrt(1.0 / (2.0 * N))
    assert abs(diff.mean() - 1.0) < 5.0 / np.sqrt(N)
    auto = spectrum_restated(d, np.zeros_like(d), np.ones_like(d), np.ones((2 * nb, nf)), op, norm_f)["per_baseline"]["data"]
    assert abs(auto.mean() - 1.0) < 5.0 / np.sqrt(2 * N)  # the auto power carries the whole noise


def test_only_the_common_channels_enter():
    rng = np.random.default_rng(2)
    nb, nf = 4, 61
    d, m, G, w, pairs = two_slices(rng, nb, nf)
    w[0, 5:20] = 0.0     # flagged on side 0 only
    w[nb, 30:41] = 0.0   # on side 1 only
    w[1, :] = 0.0        # one side wholly flagged
    w[2, 0::2], w[nb + 2, 1::2] = 0.0, 0.0  # disjoint masks
    op, norm_f, _ = modeling.delay_transform(F0 + DF * np.arange(nf))
    bins = np.zeros(nb, dtype=np.int32)
    ref = restated(d, m, G, w, op, norm_f, pairs, bin_of_pair=bins, nbins=1)
    # the same as data zeroed by hand on the union of the flags, both sides unflagged
    d2 = d.copy()
    gone = np.zeros(nf, bool)
    gone[5:20] = gone[30:41] = True
    d2[0, gone] = d2[nb, gone] = 0.0
    m2 = m.copy()
    m2[0, gone] = m2[nb, gone] = 0.0
    by_hand = restated(d2, m2, G, np.ones_like(w), op, norm_f, pairs[:1])
    assert ref["norm_pair"][0] == norm_f[~gone].sum()
    for k in NAMES:
        for st in STATS:
            np.testing.assert_allclose(ref["per_pair"][st][k][0] * ref["norm_pair"][0], by_hand["per_pair"][st][k][0] * by_hand["norm_pair"][0], rtol=1e-12, atol=1e-18)
            assert not np.any(ref["per_pair"][st][k][1]) and not np.any(ref["per_pair"][st][k][2])
    assert ref["norm_pair"][1] == 0 and ref["norm_pair"][2] == 0 and list(ref["count_bin"]) == [2]
    own = bin_pairs(ref["per_pair"]["cross"], ref["norm_pair"], bins, 1)
    np.testing.assert_array_equal(own["resid"][0], ref["per_pair"]["cross"]["resid"][0] + ref["per_pair"]["cross"]["resid"][3])


# ---- the drop-in keyword ------------------------------------------------------------------------------------------------------------------
def test_the_pairing_rule():
    pair = calibration.delay_cross_pairing
    assert pair([0, 0, 0, 0], [0, 1, 2, 3]) == [(0, 1), (2, 3)]
    assert pair([0, 0, 0], [0, 1, 2]) == [(0, 1)]  # an odd batch: the last slice stays alone
    assert pair([0, 0, 0, 1, 1, 1], [0, 1, 2, 0, 1, 2]) == [(0, 1), (3, 4)]  # a polarization boundary inside a batch is no pair
    assert pair([0, 1, 1], [2, 0, 1]) == [(1, 2)]
    assert pair([0, 0, 0, 0], [0, 2, 3, 4]) == [(1, 2)]  # time 1 was skipped: 0 stays alone, (2, 3) pair, 4 stays alone
    assert pair([0, 0], [0, 2]) == [] and pair([0], [0]) == [] and pair([], []) == []
    dspec = dict(nbins=2, bin_of_bl=np.array([0, 1, 1], dtype=np.int32))
    pairs, scale, bins = calibration.delay_cross_rows([(0, 1), (3, 4)], dspec, [2.0, 3.0, 9.0, 5.0, 7.0], 3)
    np.testing.assert_array_equal(pairs, [[0, 3], [1, 4], [2, 5], [9, 12], [10, 13], [11, 14]])
    np.testing.assert_array_equal(scale, [[2.0, 3.0]] * 3 + [[5.0, 7.0]] * 3)
    np.testing.assert_array_equal(bins, [0, 1, 1, 2, 3, 3])
    assert pairs.dtype == np.int32 and bins.dtype == np.int32


CALLS = ["calibrate_and_model_tensor", "calibrate_and_model_mixed", "calibrate_and_model_dpss", "read_calibrate_and_model_dpss"]


@pytest.mark.parametrize("bad", [dict(delay_cross_spectrum=True), dict(delay_cross_spectrum=True, delay_spectrum=True, batch_slices=False),
                                 dict(delay_cross_spectrum=True, delay_spectrum=True, batch_slices=1),
                                 dict(delay_cross_spectrum=True, delay_spectrum="baselines", init_guesses_from_previous_time_step=True),
                                 dict(delay_cross_spectrum="yes", delay_spectrum=True)])
@pytest.mark.parametrize("name", CALLS)
def test_bad_keywords_are_refused_before_anything_is_touched(name, bad):
    call = getattr(calibration, name)
    with pytest.raises(ValueError, match="delay_cross_spectrum"):
        call(None, {}, **bad) if name == "calibrate_and_model_tensor" else call(None, **bad)  # (no data, no device: the check comes first)


@pytest.mark.parametrize("name", CALLS)
def test_the_keyword_is_off_by_default_and_a_python_keyword_only(name):
    params = inspect.signature(getattr(calibration, name)).parameters
    assert params["delay_cross_spectrum"].default is False
    from calamity_amd.fit_loop import FitControls

    assert not any("delay_cross" in f for f in FitControls().keywords())
    assert not any("delay_cross" in a.dest for a in calibration.dpss_fit_argparser()._actions)


def test_the_methods_and_the_binding():
    for cls in (solver.HipFitSolver, batched.SliceBatchFitter):
        params = inspect.signature(cls.delay_cross_spectrum).parameters
        assert list(params)[1:] == ["op", "norm_f", "pairs", "scale", "what", "stats", "calibrated", "bin_of_pair", "nbins", "per_pair", "g_r", "g_i"]
        assert params["scale"].default is None and params["stats"].default == ("cross", "diff") and params["calibrated"].default is False
        assert params["nbins"].default == 0 and params["per_pair"].default is False and params["bin_of_pair"].default is None
    names = [f[0] for f in _lib.DelayCrossDesc._fields_]
    assert names == ["ndelays", "what", "calibrated", "npairs", "pairs", "scale", "stats", "nbins", "bin_of_pair", "op_r", "op_i", "norm_f"]
    text = open(os.path.join(ROOT, "include", "calamity_hip.h")).read()
    fields = text.split("typedef struct cal_delay_cross_desc {")[1].split("}")[0]
    assert re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", fields)) == names
    for word in ("cal_solver_delay_cross_spectrum(", "the COMMON mask", "ONE\n * all-reduce of nstat nwhat nbins ndelays + nbins", "what = 60 .. 65",
                 "const struct cal_delay_cross_desc* cross", "bit-identical to one without it", "power_bl[b] to the bit"):
        assert word in text, word
    assert hasattr(_lib.load(), "cal_solver_delay_cross_spectrum")
    spec = distributed.exchange_spec(7, 64, delay_cross=(2, 3, 5, 37))
    assert spec["delay_cross_f64"] == 2 * 3 * 5 * 37 + 5
    assert {k: v for k, v in spec.items() if k != "delay_cross_f64"} == distributed.exchange_spec(7, 64)


def test_pairs_are_shared_out_over_the_workers_that_hold_both_rows():
    rows = [np.array([4, 5, 0, 1]), np.array([2, 3, 6, 7])]  # two workers, their global rows in local order
    pairs = np.array([[0, 4], [2, 6], [1, 5], [3, 3], [7, 6]])
    sel, local = batched.split_pairs(pairs, rows, 8)
    np.testing.assert_array_equal(sel[0], [0, 2])
    np.testing.assert_array_equal(sel[1], [1, 3, 4])
    np.testing.assert_array_equal(local[0], [[2, 0], [3, 1]])
    np.testing.assert_array_equal(local[1], [[0, 2], [1, 1], [3, 2]])
    with pytest.raises(ValueError, match="two workers"):
        batched.split_pairs(np.array([[0, 4], [1, 2]]), rows, 8)
    with pytest.raises(ValueError, match="holds no pair"):
        batched.split_pairs(np.array([[0, 4]]), rows, 8)


# ---- the plan -----------------------------------------------------------------------------------------------------------------------------
CROSS = {60: ("scalars", np.int64), 61: ("bin_ent", np.int32), 62: ("chunk_ptr", np.int32), 63: ("image", None), 64: ("norm_f", np.float64),
         65: ("scale", np.float64)}
SCALARS = "nq nstat xpitch ndpad cpairs nchunks n_x n_pow n_out".split()


def cross_desc(dtype, op, norm_f, pairs, scale=None, what=7, stats=3, nbins=0, bin_of_pair=None, npairs=None):
    keep = [np.ascontiguousarray(op.real, dtype), np.ascontiguousarray(op.imag, dtype), np.ascontiguousarray(norm_f, np.float64),
            None if bin_of_pair is None else np.ascontiguousarray(bin_of_pair, np.int32), None if pairs is None else np.ascontiguousarray(pairs, np.int32),
            None if scale is None else np.ascontiguousarray(scale, np.float64)]
    n = len(pairs) if npairs is None else npairs
    return _lib.DelayCrossDesc(op.shape[1], what, 0, n, RP.ptr(keep[4]), RP.ptr(keep[5]), stats, nbins, RP.ptr(keep[3]), RP.ptr(keep[0]), RP.ptr(keep[1]),
                               RP.ptr(keep[2])), keep


def cross_plan(prob, dtype, op, norm_f, pairs, bound=0, **kw):
    desc, keep = cross_desc(dtype, op, norm_f, pairs, **kw)
    report = _lib.CrossReportPlanDesc(cross=C.pointer(desc), scratch_bytes=bound)
    out = {}
    for what, (name, dt) in CROSS.items():
        rc, got, _ = RP.raw_call(prob, dtype, report, what)
        _lib.check(rc)
        out[name] = got.view(dtype if dt is None else dt).copy()
    return out


def cross_rule(npairs, fpad, dtype, nd, what=7, stats=3, nbins=0, bin_of_pair=None, bound=0):
    size = np.dtype(dtype).itemsize
    nq, nstat = bin(what).count("1"), bin(stats).count("1")
    xpitch, ndpad = -(-fpad // RP.DS_STEP) * RP.DS_STEP, -(-nd // RP.DS_COLS) * RP.DS_COLS
    pair_bytes = nq * 2 * 2 * xpitch * size + nstat * nq * nd * 8
    cpairs = max(1, (bound or RP.DEFAULT_BOUND) // pair_bytes)
    if cpairs > DC_PAIRS:
        cpairs -= cpairs % DC_PAIRS
    cpairs = min(cpairs, npairs)
    nchunks = -(-npairs // cpairs)
    lists = [np.flatnonzero(np.asarray(bin_of_pair) == n) for n in range(nbins)]  # ascending pairs
    start = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(int)
    ptr = np.zeros((nchunks, nbins, 2), np.int32)
    for c in range(nchunks):
        for n in range(nbins):
            ptr[c, n] = [start[n] + np.searchsorted(lists[n], c * cpairs), start[n] + np.searchsorted(lists[n], min(npairs, (c + 1) * cpairs))]
    scalars = [nq, nstat, xpitch, ndpad, cpairs, nchunks, nq * 2 * 2 * cpairs * xpitch, nstat * nq * cpairs * nd, npairs + nstat * nq * nbins * nd + nbins]
    return dict(scalars=np.asarray(scalars, np.int64), bin_ent=np.concatenate(lists).astype(np.int32) if nbins else np.zeros(0, np.int32), chunk_ptr=ptr.ravel())


def pairs_of(prob, npairs, seed=0):
    return np.random.default_rng(seed).integers(0, prob.nbls, size=(npairs, 2)).astype(np.int32)


@pytest.mark.parametrize("dtype", RP.DTYPES)
@pytest.mark.parametrize("npairs,bound_pairs", [(300, 0), (300, 200), (300, 64), (300, 7), (5, 1), (1, 0)])
def test_the_plan_cuts_pairs_at_multiples_of_64_and_never_below_one(npairs, bound_pairs, dtype):
    prob = RP.rows22()
    fpad, nd = RP.fpad_of(prob, dtype), 37
    rng = np.random.default_rng(3)
    op, norm_f = rng.standard_normal((prob.nfreqs, nd)) + 1j * rng.standard_normal((prob.nfreqs, nd)), rng.uniform(size=prob.nfreqs)
    pairs = pairs_of(prob, npairs)
    bins = (np.arange(npairs) % 4 - (np.arange(npairs) % 9 == 0)).astype(np.int32)  # -1 .. 3; bin 4 stays empty
    xpitch = -(-fpad // 32) * 32
    per_pair = 3 * 2 * 2 * xpitch * np.dtype(dtype).itemsize + 2 * 3 * nd * 8
    bound = bound_pairs * per_pair + (per_pair // 2 if bound_pairs else 0)
    got = cross_plan(prob, dtype, op, norm_f, pairs, bound=bound, nbins=5, bin_of_pair=bins)
    want = cross_rule(npairs, fpad, dtype, nd, nbins=5, bin_of_pair=bins, bound=bound)
    for k in ("scalars", "bin_ent", "chunk_ptr"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    s = dict(zip(SCALARS, got["scalars"]))
    assert s["cpairs"] == {0: min(npairs, 300), 200: 192, 64: 64, 7: 7, 1: 1}[bound_pairs] and s["cpairs"] >= 1
    assert s["nchunks"] == -(-npairs // s["cpairs"])
    # every bin's pieces over the chunks tile its list
    ptr = got["chunk_ptr"].reshape(s["nchunks"], 5, 2)
    for n in range(5):
        assert np.all(ptr[1:, n, 0] == ptr[:-1, n, 1]) and ptr[-1, n, 1] - ptr[0, n, 0] == np.count_nonzero(bins == n)
    assert ptr[0, 4, 0] == ptr[-1, 4, 1]  # the empty bin
    # the operator image and norm_f are the spectrum's; no scales are ones
    image = got["image"].reshape(2, s["xpitch"], s["ndpad"])
    np.testing.assert_array_equal(image[0, : prob.nfreqs, :nd], op.real.astype(dtype))
    np.testing.assert_array_equal(image[1, : prob.nfreqs, :nd], op.imag.astype(dtype))
    assert not np.any(image[:, prob.nfreqs :]) and not np.any(image[:, :, nd:])
    np.testing.assert_array_equal(got["norm_f"], np.concatenate([norm_f, np.zeros(s["xpitch"] - prob.nfreqs)]))
    np.testing.assert_array_equal(got["scale"], np.ones(2 * npairs))
    scale = rng.uniform(0.5, 2.0, size=(npairs, 2))
    np.testing.assert_array_equal(cross_plan(prob, dtype, op, norm_f, pairs, scale=scale, stats=2, what=5)["scale"], scale.ravel())
    one = dict(zip(SCALARS, cross_plan(prob, dtype, op, norm_f, pairs, stats=2, what=5)["scalars"]))
    assert (one["nq"], one["nstat"], one["n_out"]) == (2, 1, npairs)


def test_the_planner_refuses_what_the_call_refuses():
    prob = RP.rows22()
    nd = 8
    op, norm_f = np.zeros((prob.nfreqs, nd), np.complex128), np.ones(prob.nfreqs)
    pairs = np.array([[0, 1], [2, 21]], np.int32)

    def refused(selector=60, bound=0, **kw):
        desc, keep = cross_desc(np.float32, op, norm_f, **{"pairs": pairs, **kw})
        rc, _, _ = RP.raw_call(prob, np.float32, _lib.CrossReportPlanDesc(cross=C.pointer(desc), scratch_bytes=bound), selector)
        return rc, _lib.load().cal_last_error().decode()

    assert refused()[0] == 0
    INV = _lib.CAL_ERR_INVALID
    for kw, text in ((dict(npairs=0), "delay_cross_spectrum: npairs = 0 (at least 1)"), (dict(pairs=None, npairs=2), "delay_cross_spectrum: null pairs"),
                     (dict(pairs=np.array([[0, 1], [2, 22]])), "delay_cross_spectrum: pairs[1][1] = 22 lies outside [0, 22)"),
                     (dict(pairs=np.array([[-1, 1]])), "delay_cross_spectrum: pairs[0][0] = -1 lies outside [0, 22)"),
                     (dict(stats=0), "delay_cross_spectrum: stats = 0: bits 0 (cross), 1 (diff), at least one"),
                     (dict(stats=4), "delay_cross_spectrum: stats = 4: bits 0 (cross), 1 (diff), at least one"),
                     (dict(scale=np.array([[1.0, 1.0], [np.inf, 1.0]])), "delay_cross_spectrum: scale[1][0] is not finite"),
                     (dict(scale=np.array([[1.0, np.nan], [1.0, 1.0]])), "delay_cross_spectrum: scale[0][1] is not finite"),
                     (dict(nbins=2, bin_of_pair=[0, 2]), "delay_cross_spectrum: bin_of_pair[1] = 2 lies outside [-1, 2)"),
                     (dict(nbins=2, bin_of_pair=[-2, 0]), "delay_cross_spectrum: bin_of_pair[0] = -2 lies outside [-1, 2)")):
        rc, msg = refused(**kw)
        assert rc == INV and msg == text, (kw, msg)
    for kw in (dict(what=0), dict(what=8), dict(nbins=-1), dict(nbins=2), dict(bin_of_pair=[0, 0])):
        rc, msg = refused(**kw)
        assert rc == INV and "takes a cross description cal_solver_delay_cross_spectrum would plan for" in msg, (kw, msg)
    assert refused(bound=-1)[0] == INV
    rc, _, _ = RP.raw_call(prob, np.float32, _lib.CrossReportPlanDesc(), 60)  # no description
    assert rc == INV
    assert refused(selector=66)[0] == INV and refused(selector=59)[0] == INV  # the range is 60 .. 65


# ---- the build guard ----------------------------------------------------------------------------------------------------------------------
def test_the_build_guard_refuses_a_spilling_cross_kernel():
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
    names = {f"{k}<{t}>": f"_ZN4calk{len(k)}{k}I{t}EEvPKT_" for k in ("dcross_rows_kernel", "dcross_transform_kernel") for t in "fd"}
    assert run(dense + "".join(remarks(n, 0, 0) for n in names.values())).returncode == 0
    for k, n in names.items():
        for scratch, vspill in ((16, 0), (0, 4)):
            bad = run(dense + remarks(n, scratch, vspill))
            assert bad.returncode != 0 and k.split("<")[0] in bad.stdout + bad.stderr, (k, scratch, vspill)
    for t in "fd":
        low = run(dense + remarks(names[f"dcross_transform_kernel<{t}>"], 0, 0, occ=1))
        assert low.returncode != 0 and "occupancy" in low.stdout + low.stderr
        assert run(dense + remarks(names[f"dcross_rows_kernel<{t}>"], 0, 0, occ=1)).returncode == 0  # no occupancy rule for the rows kernel
    # the spectrum's transform, whose loop the cross transform shares, keeps its own rule
    spec = "_ZN4calk22dspec_transform_kernelIfEEvPKT_"
    assert run(dense + remarks(spec, 0, 4)).returncode != 0 and run(dense + remarks(spec, 0, 0, occ=1)).returncode != 0
