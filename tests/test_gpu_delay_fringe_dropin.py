"""calibrate_and_model_dpss(..., delay_spectrum=..., delay_fringe_spectrum=True | "baselines", delay_fringe_times=3): the ``"fringe"``
entries of ``fit_history[pol][t]["delay_spectrum"]`` against the restatement (tests/delay_fringe_ref.py) applied to the call's OWN
outputs -- the input data and flags, the returned model (before gains) and the returned gains of the three times of a window, in the
data's units.  fp64, 7 antennas x 64 channels x 6 times: two windows, also of a joint time-basis fit.  The bound is the restatement's, per group, and a bin's mean is
held to the mean of its groups' bounds.  With the keyword off the key is absent and nothing else changes by a bit."""
import functools

import numpy as np
import pytest

from calamity_amd import calibration, modeling, synthetic
from delay_fringe_ref import bound_plane, restated
from delay_spectrum_ref import NAMES
from test_gpu_delay_cross_dropin import rows_of_time
from test_gpu_delay_spectrum_dropin import KW, WIDTH

pytestmark = pytest.mark.gpu
N = 3


@functools.lru_cache(maxsize=None)
def data_set():
    uvd, _, _ = synthetic.make_uvdata(nants=7, nfreqs=64, ntimes=6, flag_frac=0.05)
    return uvd


@functools.lru_cache(maxsize=None)
def fitted(fringe, joint=False):
    uvd = data_set()
    kw = dict(KW, delay_spectrum="baselines", delay_spectrum_bllen_bin=WIDTH, **({"gain_time_scale": 1.0e6} if joint else {}))
    if fringe is not False:
        kw.update(delay_fringe_spectrum=fringe, delay_fringe_times=N)
    return uvd, calibration.calibrate_and_model_dpss(uvdata=uvd, **kw)


def check_window(uvd, out, window, label, per_baseline=False):
    hist = out[3][0]
    entries = [hist[t]["delay_spectrum"]["fringe"] for t in window]
    e0 = entries[0]
    times = np.unique(uvd.time_array)
    dt = float(np.median(np.diff(times))) * 86400.0
    opt, rates = modeling.fringe_rate_transform(N, dt, taper="bh4")
    for e in entries:  # every member carries the same arrays
        assert e["time_indices"] == list(window)
        np.testing.assert_array_equal(e["fringe_rates"], rates)
        np.testing.assert_array_equal(e["nbls"], e0["nbls"])
        for k in NAMES:
            np.testing.assert_array_equal(e[k], e0[k])
    assert np.all(np.diff(e0["fringe_rates"]) > 0) and e0["fringe_rates"][N // 2] == 0
    fit_pairs = list(hist[window[0]]["delay_spectrum"]["per_baseline"])
    sides = [rows_of_time(uvd, out, t, frozenset(fit_pairs)) for t in window]
    nb = len(fit_pairs)
    d, m, G, w = (np.array([sides[s][ap][k] for s in range(N) for ap in fit_pairs]) for k in range(4))
    op, norm_f, delays = modeling.delay_transform(np.asarray(uvd.freq_array).ravel())
    rows = np.stack([t * nb + np.arange(nb) for t in range(N)], axis=1)
    ref = restated(d, m, G, w, op, norm_f, rows, opt)
    norm = np.where(ref["norm_grp"] > 0, ref["norm_grp"], 1.0)[:, None, None]
    pos = {int(a): x for a, x in zip(uvd.antenna_numbers, uvd.antenna_positions)}
    lengths = np.asarray([np.linalg.norm(pos[a] - pos[b]) for a, b in fit_pairs])
    idx = np.floor(lengths / WIDTH).astype(int)
    used = np.unique(idx)
    assert e0["data"].shape == (len(used), N, len(delays))
    worst = 0.0
    for k in NAMES:
        bound = bound_plane(ref, k, np.float64) / norm
        for n, u in enumerate(used):
            sel = (idx == u) & (ref["norm_grp"] > 0)
            assert e0["nbls"][n] == sel.sum() > 0
            want = ref["per_group"][k][sel].mean(axis=0)
            worst = max(worst, float(np.max(np.abs(e0[k][n] - want) / bound[sel].mean(axis=0))))
        assert ("per_baseline" in e0) == per_baseline
        if per_baseline:
            assert set(e0["per_baseline"]) == set(fit_pairs)
            for b, ap in enumerate(fit_pairs):
                live = bound[b] > 0
                err = np.abs(e0["per_baseline"][ap][k] - ref["per_group"][k][b])
                worst = max(worst, float(np.max(err[live] / bound[b][live], initial=0.0)))
                assert not np.any(err[~live])
    assert all(np.all(e0[k] >= 0) and np.any(e0[k] > 0) for k in NAMES)
    print(f"{label} times {window}: error / bound {worst:.3f}")
    assert worst <= 1.0, label


@pytest.mark.parametrize("mode", [True, "baselines"])
def test_six_times_make_two_windows(mode):
    uvd, out = fitted(mode)
    assert sorted(out[3][0]) == [0, 1, 2, 3, 4, 5]
    for window in ((0, 1, 2), (3, 4, 5)):
        check_window(uvd, out, window, f"six times {mode}", per_baseline=mode == "baselines")
    a, b = (out[3][0][t]["delay_spectrum"]["fringe"]["resid"] for t in (0, 3))
    assert not np.array_equal(a, b)


def test_a_joint_time_basis_fit_is_cut_into_the_same_windows():
    uvd, out = fitted("baselines", joint=True)
    assert sorted(out[3][0]) == [0, 1, 2, 3, 4, 5]
    for window in ((0, 1, 2), (3, 4, 5)):
        check_window(uvd, out, window, "joint", per_baseline=True)


def test_the_keyword_changes_nothing_else():
    _, on = fitted("baselines")
    _, off = fitted(False)
    np.testing.assert_array_equal(on[0].data_array, off[0].data_array)
    np.testing.assert_array_equal(on[1].data_array, off[1].data_array)
    np.testing.assert_array_equal(on[2].gain_array, off[2].gain_array)
    for t in off[3][0]:
        a, b = on[3][0][t], off[3][0][t]
        assert set(a) == set(b) and a["loss"] == b["loss"]
        for k in b:
            if k != "delay_spectrum" and isinstance(b[k], (np.ndarray, float, int)):
                np.testing.assert_array_equal(a[k], b[k], err_msg=k)
        assert set(a["delay_spectrum"]) - {"fringe"} == set(b["delay_spectrum"]) and "fringe" not in b["delay_spectrum"]
        for k in ("data", "model", "resid", "nbls"):
            np.testing.assert_array_equal(a["delay_spectrum"][k], b["delay_spectrum"][k])
        for ap, rows in b["delay_spectrum"]["per_baseline"].items():
            for k in rows:
                np.testing.assert_array_equal(a["delay_spectrum"]["per_baseline"][ap][k], rows[k])


def test_the_keywords_are_refused_before_anything_is_touched():
    uvd = data_set()
    kw = dict(KW, delay_spectrum=True, delay_fringe_spectrum=True, delay_fringe_times=N)
    for bad in (dict(delay_spectrum=False), dict(batch_slices=False), dict(batch_slices=2), dict(init_guesses_from_previous_time_step=True),
                dict(delay_fringe_spectrum="rows"), dict(delay_fringe_times=1), dict(delay_fringe_times=65), dict(delay_fringe_taper="hann")):
        with pytest.raises(ValueError):
            calibration.calibrate_and_model_dpss(uvdata=uvd, **dict(kw, **bad))


def test_the_file_driver_writes_the_entries(tmp_path):
    uvd = data_set()
    path = str(tmp_path / "spectra.npz")
    kw = {k: v for k, v in KW.items() if k not in ("dtype", "sky_model", "gains", "weights")}
    out = calibration.read_calibrate_and_model_dpss(uvd, precision=64, delay_spectrum="baselines", delay_spectrum_bllen_bin=WIDTH,
                                                    delay_fringe_spectrum="baselines", delay_fringe_times=4, delay_spectrum_outfile=path, **kw)
    hist = out[3]
    with np.load(path) as z:
        tables = {k: z[k] for k in z.files}
    first = hist[0][0]["delay_spectrum"]["fringe"]
    nbins, nr, nd = first["data"].shape
    assert nr == 4 and tables["fringe_rates"].shape == (4,)
    np.testing.assert_array_equal(tables["fringe_window"][0], [[0, 1, 2, 3]] * 4 + [[-1] * 4] * 2)  # one window of four; two times left over
    assert tables["fringe_resid"].shape == (1, 6, nbins, nr, nd)
    assert np.all(np.isnan(tables["fringe_resid"][0, 4:])) and not np.any(tables["fringe_nbls"][0, 4:])
    assert "fringe" not in hist[0][4]["delay_spectrum"] and "fringe" not in hist[0][5]["delay_spectrum"]
    for t in range(4):
        e = hist[0][t]["delay_spectrum"]["fringe"]
        np.testing.assert_array_equal(tables["fringe_nbls"][0, t], e["nbls"])
        for k in NAMES:
            np.testing.assert_array_equal(tables["fringe_" + k][0, t], e[k])
            for n, ap in enumerate(map(tuple, tables["fringe_antpairs"])):
                np.testing.assert_array_equal(tables["fringe_" + k + "_bl"][0, t, n], e["per_baseline"][ap][k])
    # without the keyword the archive holds what it held
    path2 = str(tmp_path / "plain.npz")
    calibration.read_calibrate_and_model_dpss(uvd, precision=64, delay_spectrum="baselines", delay_spectrum_bllen_bin=WIDTH, delay_spectrum_outfile=path2, **kw)
    with np.load(path2) as z:
        assert not any(k.startswith("fringe") for k in z.files) and set(z.files) == {k for k in tables if not k.startswith("fringe")}
