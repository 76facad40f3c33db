"""calibrate_and_model_dpss(..., delay_spectrum=..., delay_transfer=True): the ``"transfer"`` entries of
``fit_history[pol][t]["delay_spectrum"]`` against the restatement (tests/delay_transfer_ref.py) applied to the call's OWN outputs -- the
input flags and nsamples (the weights the fit used, up to one factor that cancels), the returned gains and the DPSS blocks the call fits
-- batched and looped, calibrated, and for a joint time-basis fit (entries per time).  fp64: every entry within 1e-10 (the project's
TOL for planes; the entries lie in [0, 1]).  With the keyword off the keys are absent and nothing else changes by a bit."""
import functools

import numpy as np
import pytest

from calamity_amd import calibration, modeling, synthetic, uvcompat
from delay_transfer_ref import core, samples
from test_gpu_delay_spectrum_dropin import KW, WIDTH, data_set

pytestmark = pytest.mark.gpu

RIDGE = 1e-6
TOL = 1e-10
KEYS = ("transfer", "transfer_nsingular", "transfer_per_baseline")


@functools.lru_cache(maxsize=None)
def fitted(route, mode, calibrated=False, joint=False, transfer=True):
    uvd = data_set()
    kw = dict(KW, **({"batch_slices": False} if route == "loop" else {}), **({"gain_time_scale": 1.0e6} if joint else {}))
    kw.update(delay_spectrum=mode, delay_spectrum_bllen_bin=WIDTH, delay_spectrum_calibrated=calibrated)
    if transfer:
        kw.update(delay_transfer=True, delay_transfer_ridge=RIDGE)
    return uvd, calibration.calibrate_and_model_dpss(uvdata=uvd, **kw)


@functools.lru_cache(maxsize=None)
def blocks():
    """{antenna pair, either way round: the DPSS block [Nfreqs, nvec] the call fits it with}"""
    comps = modeling.yield_pbl_dpss_model_comps(data_set(), min_dly=KW["min_dly"], offset=KW["offset"])
    out = {}
    for (grp,), blk in comps.items():
        assert len(grp) == 1  # every baseline is a fitting group of its own
        out[tuple(grp[0])] = out[tuple(grp[0])[::-1]] = np.asarray(blk, dtype=np.float64)
    return out


def expected(uvd, out, t, calibrated, fit_pairs):
    """``(antenna pairs the way round the fit holds them, lengths, absorbed [rows, ndelays], valid [rows])`` of time index ``t``."""
    _, _, gains, _ = out
    times, ants = np.unique(uvd.time_array), np.asarray(gains.ant_array)
    rows = np.where(np.isclose(uvd.time_array, times[t], atol=1e-7, rtol=0.0))[0]
    w = (~uvcompat.vis3(uvd.flag_array)[rows, :, 0]).astype(np.float64) * uvcompat.vis3(uvd.nsample_array)[rows, :, 0]
    w = w / w.sum()
    g = np.asarray(uvcompat.gain4(gains.gain_array)[:, :, t, 0])
    pairs = [(int(a), int(b)) for a, b in zip(uvd.ant_1_array[rows], uvd.ant_2_array[rows])]
    pairs = [p if p in fit_pairs else p[::-1] for p in pairs]  # a row held as (j, i) has G conjugated: its antennas change places
    assert all(p in fit_pairs for p in pairs)
    ia = np.asarray([int(np.where(ants == a)[0][0]) for a, _ in pairs])
    ib = np.asarray([int(np.where(ants == b)[0][0]) for _, b in pairs])
    q, s, v, mask = samples(g, ia, ib, w, np.float64, calibrated)
    op, _, _ = modeling.delay_transform(np.asarray(uvd.freq_array).ravel())
    absorbed = np.zeros((len(pairs), op.shape[1]))
    for b, ap in enumerate(pairs):
        res = core([blocks()[ap]], q[b : b + 1], s[b : b + 1], v[b : b + 1], op, RIDGE)
        assert res is not None
        absorbed[b] = np.where(res[1][0] != 0, res[0][0] / np.where(res[1][0] != 0, res[1][0], 1.0), 0.0)
    pos = {int(a): x for a, x in zip(uvd.antenna_numbers, uvd.antenna_positions)}
    return pairs, np.asarray([np.linalg.norm(pos[a] - pos[b]) for a, b in pairs]), absorbed, mask.any(axis=1)


def check(uvd, out, label, calibrated=False, per_baseline=False):
    hist = out[3]
    worst_bin = worst_bl = 0.0
    # which way round the fit holds every row: the keys of a per-baseline report (a row held as (j, i) has its data and G conjugated)
    fit_pairs = frozenset(fitted("batched", "baselines")[1][3][0][0]["delay_spectrum"]["transfer_per_baseline"])
    for t in sorted(hist[0]):
        e = hist[0][t]["delay_spectrum"]
        pairs, lengths, absorbed, valid = expected(uvd, out, t, calibrated, fit_pairs)
        idx = np.floor(lengths / WIDTH).astype(int)
        used = np.unique(idx)
        assert e["transfer"].shape == e["resid"].shape == (len(used), absorbed.shape[1]) and e["transfer_nsingular"] == 0
        assert np.all(e["transfer"] >= 0.0) and np.all(e["transfer"] <= 1.0) and e["transfer"].min() < 0.9  # the basis does absorb
        for n, u in enumerate(used):
            sel = (idx == u) & valid
            assert e["nbls"][n] == sel.sum() > 0
            worst_bin = max(worst_bin, float(np.max(np.abs(e["transfer"][n] - (1.0 - absorbed[sel].mean(axis=0))))))
        assert ("transfer_per_baseline" in e) == per_baseline
        if per_baseline:
            assert set(e["transfer_per_baseline"]) == set(e["per_baseline"]) and len(pairs) == len(e["per_baseline"])
            for b, ap in enumerate(pairs):
                worst_bl = max(worst_bl, float(np.max(np.abs(e["transfer_per_baseline"][ap] - (1.0 - absorbed[b])))))
    print(f"{label}: largest error  bins {worst_bin:.2e}  per baseline {worst_bl:.2e}")
    assert worst_bin <= TOL and worst_bl <= TOL, label


@pytest.mark.parametrize("mode", [True, "baselines"])
@pytest.mark.parametrize("route", ["batched", "loop"])
def test_the_entries_match_the_returned_gains_and_the_fitted_blocks(route, mode):
    uvd, out = fitted(route, mode)
    assert sorted(out[3][0]) == [0, 1]
    check(uvd, out, f"{route} {mode}", per_baseline=mode == "baselines")


@pytest.mark.parametrize("route", ["batched", "loop"])
def test_the_keyword_changes_nothing_else(route):
    _, on = fitted(route, "baselines")
    _, off = fitted(route, "baselines", transfer=False)
    np.testing.assert_array_equal(on[0].data_array, off[0].data_array)
    np.testing.assert_array_equal(on[1].data_array, off[1].data_array)
    np.testing.assert_array_equal(on[2].gain_array, off[2].gain_array)
    for t in off[3][0]:
        a, b = on[3][0][t], off[3][0][t]
        assert set(a) == set(b) and a["loss"] == b["loss"]
        assert set(a["delay_spectrum"]) - set(KEYS) == set(b["delay_spectrum"]) and set(KEYS) <= set(a["delay_spectrum"])
        for k in ("data", "model", "resid", "nbls"):
            np.testing.assert_array_equal(a["delay_spectrum"][k], b["delay_spectrum"][k])
        for ap, rows in b["delay_spectrum"]["per_baseline"].items():
            for k in rows:
                np.testing.assert_array_equal(a["delay_spectrum"]["per_baseline"][ap][k], rows[k])


def test_calibrated_transfer():
    uvd, out = fitted("batched", "baselines", calibrated=True)
    check(uvd, out, "calibrated", calibrated=True, per_baseline=True)


def test_a_joint_time_basis_fit_reports_every_time():
    uvd, out = fitted("batched", "baselines", joint=True)
    assert sorted(out[3][0]) == [0, 1]
    check(uvd, out, "joint", per_baseline=True)
    a, b = (out[3][0][t]["delay_spectrum"]["transfer"] for t in (0, 1))
    assert not np.array_equal(a, b)  # per time, not one sum over the joint fit


def test_the_file_driver_writes_the_entries(tmp_path):
    uvd = data_set()
    path = str(tmp_path / "spectra.npz")
    kw = {k: v for k, v in KW.items() if k not in ("dtype", "sky_model", "gains", "weights")}
    out = calibration.read_calibrate_and_model_dpss(uvd, precision=64, delay_spectrum="baselines", delay_spectrum_bllen_bin=WIDTH, delay_transfer=True,
                                                    delay_transfer_ridge=RIDGE, delay_spectrum_outfile=path, **kw)
    hist = out[3]
    with np.load(path) as z:
        tables = {k: z[k] for k in z.files}
    first = hist[0][0]["delay_spectrum"]
    nbins, nd = first["transfer"].shape
    assert tables["transfer"].shape == (1, 2, nbins, nd) and tables["transfer_nsingular"].shape == (1, 2)
    assert tables["transfer_bl"].shape == (1, 2, len(first["transfer_per_baseline"]), nd)
    for t in (0, 1):
        e = hist[0][t]["delay_spectrum"]
        np.testing.assert_array_equal(tables["transfer"][0, t], e["transfer"])
        assert tables["transfer_nsingular"][0, t] == e["transfer_nsingular"] == 0
        for n, ap in enumerate(map(tuple, tables["antpairs"])):
            np.testing.assert_array_equal(tables["transfer_bl"][0, t, n], e["transfer_per_baseline"][ap])
    # without the keyword the archive holds what it held
    path2 = str(tmp_path / "plain.npz")
    calibration.read_calibrate_and_model_dpss(uvd, precision=64, delay_spectrum="baselines", delay_spectrum_bllen_bin=WIDTH, delay_spectrum_outfile=path2, **kw)
    with np.load(path2) as z:
        assert not any(k.startswith("transfer") for k in z.files) and set(z.files) == set(tables) - {"transfer", "transfer_nsingular", "transfer_bl"}
