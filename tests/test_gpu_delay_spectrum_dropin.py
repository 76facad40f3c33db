"""calibrate_and_model_dpss(..., delay_spectrum=True | "baselines"): ``fit_history[pol][t]["delay_spectrum"]`` against the restatement
(tests/delay_spectrum_ref.py) applied to the call's OWN outputs -- the input data and flags, the returned model (before gains:
``correct_model=True``) and the returned gains -- looped and batched, calibrated, and for a joint time-basis fit (entries per time).
fp64; the bound is the restatement's, |P - P_ref| norm_b <= (2 |X_ref| + tau) tau with tau = 8 u (nfreqs + 16) sum_f mask
(|d| + |G| |m|) |op| in the data's units (the power scales with rms^2, tau with rms, norm_b not at all); a bin's mean is held to the
mean of its rows' bounds.  With the keyword off the key is absent and nothing else changes by a bit."""
import functools

import numpy as np
import pytest

from calamity_amd import calibration, modeling, synthetic, uvcompat
from delay_spectrum_ref import NAMES, UNIT, restated

pytestmark = pytest.mark.gpu

KW = dict(min_dly=2.0 / 0.3, offset=2.0 / 0.3, sky_model=None, maxsteps=60, tol=1e-14, correct_resid=False, weights=None, optimizer="Adam",
          learning_rate=1e-2, dtype=np.float64, model_regularization="sum", gains=None)
WIDTH = 20.0  # metres per baseline-length bin: several baselines per bin on the 60 m field of make_uvdata


def data_set():
    uvd, _, _ = synthetic.make_uvdata(nants=6, nfreqs=48, ntimes=2, flag_frac=0.05)
    return uvd


@functools.lru_cache(maxsize=None)
def fitted(route, mode, calibrated=False, joint=False):
    uvd = data_set()
    kw = dict(KW, **({"batch_slices": False} if route == "loop" else {}), **({"gain_time_scale": 1.0e6} if joint else {}))
    if mode is not False:
        kw.update(delay_spectrum=mode, delay_spectrum_bllen_bin=WIDTH, delay_spectrum_calibrated=calibrated)
    return uvd, calibration.calibrate_and_model_dpss(uvdata=uvd, **kw)


@functools.lru_cache(maxsize=None)
def fit_pairs():
    """The antenna pairs of the fit's rows: the modeling components may hold a baseline as (j, i), its data conjugated, and the
    spectrum of a conjugated row is the mirror image in delay.  The keys of ``per_baseline`` say which way round every row is."""
    _, out = fitted("batched", "baselines")
    return frozenset(out[3][0][0]["delay_spectrum"]["per_baseline"])


def expected(uvd, out, t, calibrated):
    """The restatement on the rows of time index ``t``, every row the way round the fit holds it: ``(antenna pairs, lengths, restated
    dict, delays)``."""
    model, _, gains, _ = out
    times, ants = np.unique(uvd.time_array), np.asarray(gains.ant_array)
    rows = np.where(np.isclose(uvd.time_array, times[t], atol=1e-7, rtol=0.0))[0]
    d = np.array(uvcompat.vis3(uvd.data_array)[rows, :, 0])
    m = np.array(uvcompat.vis3(model.data_array)[rows, :, 0])
    w = (~uvcompat.vis3(uvd.flag_array)[rows, :, 0]).astype(np.float64)
    g = uvcompat.gain4(gains.gain_array)[:, :, t, 0]
    ia = [int(np.where(ants == a)[0][0]) for a in uvd.ant_1_array[rows]]
    ib = [int(np.where(ants == a)[0][0]) for a in uvd.ant_2_array[rows]]
    op, norm_f, delays = modeling.delay_transform(np.asarray(uvd.freq_array).ravel())
    pairs = [(int(a), int(b)) for a, b in zip(uvd.ant_1_array[rows], uvd.ant_2_array[rows])]
    G = g[ia] * np.conj(g[ib])
    for n, (a, b) in enumerate(pairs):
        if (a, b) not in fit_pairs():
            assert (b, a) in fit_pairs()
            pairs[n], d[n], m[n], G[n] = (b, a), np.conj(d[n]), np.conj(m[n]), np.conj(G[n])
    ref = restated(d, m, G, w, op, norm_f, calibrated)
    pos = {int(a): x for a, x in zip(uvd.antenna_numbers, uvd.antenna_positions)}
    return pairs, np.asarray([np.linalg.norm(pos[a] - pos[b]) for a, b in pairs]), ref, delays


def check(uvd, out, label, calibrated=False, per_baseline=False):
    hist = out[3]
    worst_bin = worst_bl = 0.0
    for t in sorted(hist[0]):
        e = hist[0][t]["delay_spectrum"]
        pairs, lengths, ref, delays = expected(uvd, out, t, calibrated)
        np.testing.assert_allclose(e["delays_ns"], delays, rtol=1e-12)
        tau = UNIT[np.dtype(np.float64)] * ref["tau_per_unit"]
        bound = {k: (2.0 * np.abs(ref["X"][k]) + tau) * tau / np.where(ref["norm_bl"] > 0, ref["norm_bl"], 1.0)[:, None] for k in NAMES}
        idx = np.floor(lengths / WIDTH).astype(int)
        used = np.unique(idx)
        assert len(used) >= 2 and e["data"].shape == (len(used), len(delays)) and len(e["bllen_m"]) == len(used)
        for n, u in enumerate(used):
            sel = (idx == u) & (ref["norm_bl"] > 0)
            assert e["nbls"][n] == sel.sum() and abs(e["bllen_m"][n] - lengths[idx == u].mean()) <= 1e-9
            for k in NAMES:
                want = ref["per_baseline"][k][sel].mean(axis=0)
                assert want.max() > 0
                worst_bin = max(worst_bin, float(np.max(np.abs(e[k][n] - want) / bound[k][sel].mean(axis=0))))
        assert ("per_baseline" in e) == per_baseline
        if per_baseline:
            assert len(e["per_baseline"]) == len(pairs)
            for b, (a0, a1) in enumerate(pairs):
                for k in NAMES:
                    got = e["per_baseline"][(a0, a1)][k]
                    worst_bl = max(worst_bl, float(np.max(np.abs(got - ref["per_baseline"][k][b]) / bound[k][b])))
    print(f"{label}: error / bound  bins {worst_bin:.3f}  per baseline {worst_bl:.3f}")
    assert worst_bin <= 1.0 and worst_bl <= 1.0, label


@pytest.mark.parametrize("mode", [True, "baselines"])
@pytest.mark.parametrize("route", ["batched", "loop"])
def test_the_entries_match_the_returned_data_model_and_gains(route, mode):
    uvd, out = fitted(route, mode)
    assert sorted(out[3][0]) == [0, 1]
    check(uvd, out, f"{route} {mode}", per_baseline=mode == "baselines")


@pytest.mark.parametrize("route", ["batched", "loop"])
def test_the_keyword_changes_nothing_else(route):
    _, on = fitted(route, "baselines")
    _, off = fitted(route, False)
    np.testing.assert_array_equal(on[0].data_array, off[0].data_array)
    np.testing.assert_array_equal(on[1].data_array, off[1].data_array)
    np.testing.assert_array_equal(on[2].gain_array, off[2].gain_array)
    for t in off[3][0]:
        assert "delay_spectrum" not in off[3][0][t] and "delay_spectrum" in on[3][0][t]
        assert set(on[3][0][t]) - {"delay_spectrum"} == set(off[3][0][t])
        assert on[3][0][t]["loss"] == off[3][0][t]["loss"]


def test_calibrated_spectra():
    uvd, out = fitted("batched", "baselines", calibrated=True)
    check(uvd, out, "calibrated", calibrated=True, per_baseline=True)


def test_a_joint_time_basis_fit_reports_every_time():
    uvd, out = fitted("batched", "baselines", joint=True)
    assert sorted(out[3][0]) == [0, 1]
    check(uvd, out, "joint", per_baseline=True)
    a, b = (out[3][0][t]["delay_spectrum"]["resid"] for t in (0, 1))
    assert not np.array_equal(a, b)  # per time, not one sum over the joint fit


def test_the_file_driver_writes_the_entries(tmp_path):
    uvd = data_set()
    path = str(tmp_path / "spectra.npz")
    kw = {k: v for k, v in KW.items() if k not in ("dtype", "sky_model", "gains", "weights")}
    out = calibration.read_calibrate_and_model_dpss(uvd, precision=64, delay_spectrum="baselines", delay_spectrum_bllen_bin=WIDTH,
                                                    delay_spectrum_outfile=path, **kw)
    hist = out[3]
    with np.load(path) as z:
        tables = {k: z[k] for k in z.files}
    first = hist[0][0]["delay_spectrum"]
    nbins, nd = first["data"].shape
    assert tables["data"].shape == (1, 2, nbins, nd) and tables["nbls"].shape == (1, 2, nbins)
    assert tables["antpairs"].shape == (len(first["per_baseline"]), 2) and tables["resid_bl"].shape == (1, 2, len(first["per_baseline"]), nd)
    np.testing.assert_array_equal(tables["delays_ns"], first["delays_ns"])
    np.testing.assert_array_equal(tables["bllen_m"], first["bllen_m"])
    for t in (0, 1):
        e = hist[0][t]["delay_spectrum"]
        np.testing.assert_array_equal(tables["nbls"][0, t], e["nbls"])
        for k in NAMES:
            np.testing.assert_array_equal(tables[k][0, t], e[k])
            for n, ap in enumerate(map(tuple, tables["antpairs"])):
                np.testing.assert_array_equal(tables[k + "_bl"][0, t, n], e["per_baseline"][ap][k])
    with pytest.raises(IOError):  # no clobber
        calibration.read_calibrate_and_model_dpss(uvd, precision=64, delay_spectrum=True, delay_spectrum_outfile=path, **kw)
