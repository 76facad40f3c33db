"""calibrate_and_model_dpss(..., delay_spectrum=..., delay_cross_spectrum=True | "baselines"): the ``"cross"`` entries of
``fit_history[pol][t]["delay_spectrum"]`` against the restatement (tests/delay_cross_ref.py) applied to the call's OWN outputs -- the
input data and flags, the returned model (before gains) and the returned gains of both times of a pair, in the data's units -- for
four times (two pairs), three times (the third has no partner), calibrated, and for a joint time-basis fit.  fp64; the bound is the
restatement's, per pair, and a bin's mean is held to the mean of its pairs' bounds.  With the keyword off the key is absent and
nothing else changes by a bit."""
import functools

import numpy as np
import pytest

from calamity_amd import calibration, modeling, synthetic, uvcompat
from delay_cross_ref import restated
from delay_spectrum_ref import NAMES, UNIT
from test_gpu_delay_spectrum_dropin import KW, WIDTH

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def data_set(ntimes):
    uvd, _, _ = synthetic.make_uvdata(nants=6, nfreqs=48, ntimes=ntimes, flag_frac=0.05)
    return uvd


@functools.lru_cache(maxsize=None)
def fitted(ntimes, cross, calibrated=False, joint=False):
    uvd = data_set(ntimes)
    kw = dict(KW, **({"gain_time_scale": 1.0e6} if joint else {}))
    kw.update(delay_spectrum="baselines", delay_spectrum_bllen_bin=WIDTH, delay_spectrum_calibrated=calibrated)
    if cross is not False:
        kw.update(delay_cross_spectrum=cross)
    return uvd, calibration.calibrate_and_model_dpss(uvdata=uvd, **kw)


def rows_of_time(uvd, out, t, fit_pairs):
    """{antenna pair the way round the fit holds it: (d, m, G, w)} of time index ``t`` (a row held as (j, i) is conjugated)."""
    model, _, gains, _ = out
    times, ants = np.unique(uvd.time_array), np.asarray(gains.ant_array)
    rows = np.where(np.isclose(uvd.time_array, times[t], atol=1e-7, rtol=0.0))[0]
    d = np.array(uvcompat.vis3(uvd.data_array)[rows, :, 0])
    m = np.array(uvcompat.vis3(model.data_array)[rows, :, 0])
    w = (~uvcompat.vis3(uvd.flag_array)[rows, :, 0]).astype(np.float64)
    g = uvcompat.gain4(gains.gain_array)[:, :, t, 0]
    table = {}
    for n, (a, b) in enumerate(zip(uvd.ant_1_array[rows], uvd.ant_2_array[rows])):
        a, b = int(a), int(b)
        G = g[int(np.where(ants == a)[0][0])] * np.conj(g[int(np.where(ants == b)[0][0])])
        if (a, b) in fit_pairs:
            table[a, b] = (d[n], m[n], G, w[n])
        else:
            assert (b, a) in fit_pairs
            table[b, a] = (np.conj(d[n]), np.conj(m[n]), np.conj(G), w[n])
    return table


def check_pair(uvd, out, t0, t1, label, calibrated=False, per_baseline=False):
    hist = out[3][0]
    e0, e1 = hist[t0]["delay_spectrum"]["cross"], hist[t1]["delay_spectrum"]["cross"]
    # both members carry the same arrays and each other's index
    assert e0["partner_time_index"] == t1 and e1["partner_time_index"] == t0
    for k in NAMES:
        np.testing.assert_array_equal(e0[k], e1[k])
        np.testing.assert_array_equal(e0["noise"][k], e1["noise"][k])
    np.testing.assert_array_equal(e0["nbls"], e1["nbls"])
    fit_pairs = list(hist[t0]["delay_spectrum"]["per_baseline"])
    sides = [rows_of_time(uvd, out, t, frozenset(fit_pairs)) for t in (t0, t1)]
    nb = len(fit_pairs)
    d, m, G, w = (np.array([sides[s][ap][k] for s in (0, 1) for ap in fit_pairs]) for k in range(4))
    op, norm_f, delays = modeling.delay_transform(np.asarray(uvd.freq_array).ravel())
    pairs = np.stack([np.arange(nb), nb + np.arange(nb)], axis=1)
    ref = restated(d, m, G, w, op, norm_f, pairs, None, calibrated)
    t_0, t_1 = UNIT[np.dtype(np.float64)] * ref["tau_per_unit"]
    norm = np.where(ref["norm_pair"] > 0, ref["norm_pair"], 1.0)[:, None]
    pos = {int(a): x for a, x in zip(uvd.antenna_numbers, uvd.antenna_positions)}
    lengths = np.asarray([np.linalg.norm(pos[a] - pos[b]) for a, b in fit_pairs])
    idx = np.floor(lengths / WIDTH).astype(int)
    used = np.unique(idx)
    assert e0["data"].shape == (len(used), len(delays))
    worst = 0.0
    for k in NAMES:
        Y0, Y1 = ref["Y"][k]
        bound = {"cross": (np.abs(Y0) * t_1 + np.abs(Y1) * t_0 + t_0 * t_1) / norm,
                 "diff": (2.0 * np.abs(Y0 - Y1) + t_0 + t_1) * (t_0 + t_1) / (2.0 * norm)}
        for n, u in enumerate(used):
            sel = (idx == u) & (ref["norm_pair"] > 0)
            assert e0["nbls"][n] == sel.sum() > 0
            for st, got in (("cross", e0[k][n]), ("diff", e0["noise"][k][n])):
                want = ref["per_pair"][st][k][sel].mean(axis=0)
                worst = max(worst, float(np.max(np.abs(got - want) / bound[st][sel].mean(axis=0))))
        assert ("per_baseline" in e0) == per_baseline
        if per_baseline:
            assert set(e0["per_baseline"]) == set(fit_pairs)
            for b, ap in enumerate(fit_pairs):
                live = bound["cross"][b] > 0
                for st, got in (("cross", e0["per_baseline"][ap][k]), ("diff", e0["per_baseline"][ap]["noise"][k])):
                    err = np.abs(got - ref["per_pair"][st][k][b])
                    worst = max(worst, float(np.max(err[live] / bound[st][b][live], initial=0.0)))
                    assert not np.any(err[~live])
    # the noise spectrum is a power; the residual's cross power is far below its auto power's noise floor or of its order, never above the data's
    assert all(np.all(e0["noise"][k] >= 0) for k in NAMES)
    print(f"{label} times ({t0}, {t1}): error / bound {worst:.3f}")
    assert worst <= 1.0, label


@pytest.mark.parametrize("mode", [True, "baselines"])
def test_four_times_make_two_pairs(mode):
    uvd, out = fitted(4, mode)
    assert sorted(out[3][0]) == [0, 1, 2, 3]
    for t0, t1 in ((0, 1), (2, 3)):
        check_pair(uvd, out, t0, t1, f"four times {mode}", per_baseline=mode == "baselines")
    a, b = (out[3][0][t]["delay_spectrum"]["cross"]["resid"] for t in (0, 2))
    assert not np.array_equal(a, b)


def test_the_third_of_three_times_has_no_partner():
    uvd, out = fitted(3, "baselines")
    assert sorted(out[3][0]) == [0, 1, 2]
    check_pair(uvd, out, 0, 1, "three times", per_baseline=True)
    assert "cross" not in out[3][0][2]["delay_spectrum"] and "resid" in out[3][0][2]["delay_spectrum"]


def test_calibrated_cross_spectra():
    uvd, out = fitted(4, "baselines", calibrated=True)
    for t0, t1 in ((0, 1), (2, 3)):
        check_pair(uvd, out, t0, t1, "calibrated", calibrated=True, per_baseline=True)


def test_a_joint_time_basis_fit_pairs_the_same_way():
    uvd, out = fitted(4, "baselines", joint=True)
    assert sorted(out[3][0]) == [0, 1, 2, 3]
    for t0, t1 in ((0, 1), (2, 3)):
        check_pair(uvd, out, t0, t1, "joint", per_baseline=True)


@pytest.mark.parametrize("ntimes", [3, 4])
def test_the_keyword_changes_nothing_else(ntimes):
    _, on = fitted(ntimes, "baselines")
    _, off = fitted(ntimes, False)
    np.testing.assert_array_equal(on[0].data_array, off[0].data_array)
    np.testing.assert_array_equal(on[1].data_array, off[1].data_array)
    np.testing.assert_array_equal(on[2].gain_array, off[2].gain_array)
    for t in off[3][0]:
        a, b = on[3][0][t], off[3][0][t]
        assert set(a) == set(b) and a["loss"] == b["loss"]
        assert set(a["delay_spectrum"]) - {"cross"} == set(b["delay_spectrum"]) and "cross" not in b["delay_spectrum"]
        for k in ("data", "model", "resid", "nbls"):
            np.testing.assert_array_equal(a["delay_spectrum"][k], b["delay_spectrum"][k])
        for ap, rows in b["delay_spectrum"]["per_baseline"].items():
            for k in rows:
                np.testing.assert_array_equal(a["delay_spectrum"]["per_baseline"][ap][k], rows[k])


def test_the_keyword_is_refused_before_anything_is_touched():
    uvd = data_set(3)
    kw = dict(KW, delay_spectrum=True, delay_cross_spectrum=True)
    for bad in (dict(delay_spectrum=False), dict(batch_slices=False), dict(batch_slices=1), dict(init_guesses_from_previous_time_step=True),
                dict(delay_cross_spectrum="rows")):
        with pytest.raises(ValueError):
            calibration.calibrate_and_model_dpss(uvdata=uvd, **dict(kw, **bad))


def test_the_file_driver_writes_the_entries(tmp_path):
    uvd = data_set(3)
    path = str(tmp_path / "spectra.npz")
    kw = {k: v for k, v in KW.items() if k not in ("dtype", "sky_model", "gains", "weights")}
    out = calibration.read_calibrate_and_model_dpss(uvd, precision=64, delay_spectrum="baselines", delay_spectrum_bllen_bin=WIDTH,
                                                    delay_cross_spectrum="baselines", delay_spectrum_outfile=path, **kw)
    hist = out[3]
    with np.load(path) as z:
        tables = {k: z[k] for k in z.files}
    first = hist[0][0]["delay_spectrum"]["cross"]
    nbins, nd = first["data"].shape
    assert list(tables["cross_partner"][0]) == [1, 0, -1]
    assert tables["cross_resid"].shape == tables["cross_noise_resid"].shape == (1, 3, nbins, nd)
    assert np.all(np.isnan(tables["cross_resid"][0, 2])) and not np.any(tables["cross_nbls"][0, 2])
    for t in (0, 1):
        e = hist[0][t]["delay_spectrum"]["cross"]
        np.testing.assert_array_equal(tables["cross_nbls"][0, t], e["nbls"])
        for k in NAMES:
            np.testing.assert_array_equal(tables["cross_" + k][0, t], e[k])
            np.testing.assert_array_equal(tables["cross_noise_" + k][0, t], e["noise"][k])
            for n, ap in enumerate(map(tuple, tables["cross_antpairs"])):
                np.testing.assert_array_equal(tables["cross_" + k + "_bl"][0, t, n], e["per_baseline"][ap][k])
                np.testing.assert_array_equal(tables["cross_noise_" + k + "_bl"][0, t, n], e["per_baseline"][ap]["noise"][k])
    # without the keyword the archive holds what it held
    path2 = str(tmp_path / "plain.npz")
    calibration.read_calibrate_and_model_dpss(uvd, precision=64, delay_spectrum="baselines", delay_spectrum_bllen_bin=WIDTH, delay_spectrum_outfile=path2, **kw)
    with np.load(path2) as z:
        assert not any(k.startswith("cross") for k in z.files) and set(z.files) == {k for k in tables if not k.startswith("cross")}
