"""calibrate_and_model_dpss(..., fit_quality=True): the quality arrays of the returned gains and the per-baseline dict of the fit
history against the call's OWN outputs.  With ``weights=None`` the weights are uniform over the unflagged samples, so

    quality_array[a, f, t, p]              = mean over the unflagged baselines b that hold a of |resid[b, f, t, p]|^2
    total_quality_array[f, t, p]           = the same mean over all (antenna, baseline) incidences
    fit_history[p][t]["chisq_per_baseline"] = {(ant0, ant1): mean over the unflagged channels of |resid|^2}

with ``resid`` the returned residual (``correct_resid=False``: data minus gains times model) and the input flags.  fp64, 1e-8 relative
to each array's largest element, in every path the fit can take; ``fit_quality=False`` changes nothing and leaves the zeros."""
import copy
import sys

import numpy as np
import pytest

from calamity_amd import calfits, calibration, synthetic, uvcompat

pytestmark = pytest.mark.gpu

KW = dict(min_dly=2.0 / 0.3, offset=2.0 / 0.3, sky_model=None, maxsteps=200, tol=1e-14, correct_resid=False, weights=None, optimizer="Adam",
          learning_rate=1e-2, dtype=np.float64, model_regularization="sum", gains=None)


def data_set(skip=None):
    uvd, _, _ = synthetic.make_uvdata(nants=7, nfreqs=64, ntimes=3, flag_frac=0.05)
    if skip is not None:
        times = np.unique(uvd.time_array)
        uvd.flag_array[np.isclose(uvd.time_array, times[skip], atol=1e-7, rtol=0.0)] = True
    return uvd


def expected(uvd, resid, gains):
    """(quality [ants, freqs, times, 1], total [freqs, times, 1], {time index: {(a0, a1): value}}) from the residual and the flags."""
    r2 = np.abs(uvcompat.vis3(resid.data_array)[:, :, 0]) ** 2
    ok = ~uvcompat.vis3(uvd.flag_array)[:, :, 0]
    times, ants = np.unique(uvd.time_array), np.asarray(gains.ant_array)
    num, den = np.zeros((len(ants), uvd.Nfreqs, len(times), 1)), np.zeros((len(ants), uvd.Nfreqs, len(times), 1))
    per_bl = {t: {} for t in range(len(times))}
    for n in range(uvd.Nblts):
        t = int(np.where(np.isclose(times, uvd.time_array[n], atol=1e-7, rtol=0.0))[0][0])
        a0, a1 = int(uvd.ant_1_array[n]), int(uvd.ant_2_array[n])
        for a in {a0, a1}:
            ia = int(np.where(ants == a)[0][0])
            num[ia, :, t, 0] += np.where(ok[n], r2[n], 0.0)
            den[ia, :, t, 0] += ok[n]
        per_bl[t][(a0, a1)] = float(np.sum(r2[n][ok[n]]) / max(np.sum(ok[n]), 1)) if np.any(ok[n]) else 0.0
    div = lambda a, b: np.divide(a, b, out=np.zeros_like(a), where=b != 0)  # noqa: E731
    return div(num, den), div(num.sum(axis=0), den.sum(axis=0)), per_bl


def check(uvd, out, label, skipped=()):
    model, resid, gains, hist = out
    q_want, tot_want, bl_want = expected(uvd, resid, gains)
    ntimes = q_want.shape[2]
    fitted = [t for t in range(ntimes) if t not in skipped]
    q = uvcompat.gain4(gains.quality_array)
    tot = np.asarray(gains.total_quality_array)
    assert q.shape == q_want.shape and tot.shape == (uvd.Nfreqs, ntimes, 1), (label, q.shape, tot.shape)
    assert q_want[:, :, fitted].max() > 0
    for t in skipped:  # a skipped slice keeps zeros and has no dict
        assert not np.any(q[:, :, t]) and not np.any(tot[:, t]) and t not in hist[0], (label, t)
        q_want[:, :, t], tot_want[:, t] = 0.0, 0.0
    e_q = np.max(np.abs(q - q_want)) / q_want.max()
    e_tot = np.max(np.abs(tot - tot_want)) / tot_want.max()
    e_bl = 0.0
    for t in fitted:
        got = hist[0][t]["chisq_per_baseline"]
        assert len(got) == len(bl_want[t]) and all(isinstance(k[0], int) and isinstance(k[1], int) for k in got), label
        top = max(bl_want[t].values())
        for (a0, a1), v in got.items():
            want = bl_want[t][(a0, a1)] if (a0, a1) in bl_want[t] else bl_want[t][(a1, a0)]
            e_bl = max(e_bl, abs(v - want) / top)
    print(f"{label}: quality {e_q:.2e}  total {e_tot:.2e}  per baseline {e_bl:.2e}")
    assert e_q <= 1e-8 and e_tot <= 1e-8 and e_bl <= 1e-8, label


PATHS = {
    "batched": {},
    "loop": dict(batch_slices=False),
    "use_min": dict(use_min=True),
    "gain_max_dly": dict(gain_max_dly=100.0),
    "gain_time_scale": dict(gain_time_scale=1.0e6),
    "freeze_model": dict(freeze_model=True),
    "post_hoc": dict(model_regularization="post_hoc"),
}


@pytest.mark.parametrize("path", list(PATHS))
def test_quality_arrays_match_the_returned_residual(path):
    uvd = data_set()
    out = calibration.calibrate_and_model_dpss(uvdata=uvd, fit_quality=True, **dict(KW, **PATHS[path]))
    check(uvd, out, path)


def test_a_skipped_time_keeps_zeros_and_has_no_dict():
    uvd = data_set(skip=1)
    out = calibration.calibrate_and_model_dpss(uvdata=uvd, fit_quality=True, **KW)
    assert sorted(out[3][0]) == [0, 2]
    check(uvd, out, "one time flagged", skipped=(1,))


def test_the_flag_changes_nothing_else():
    uvd = data_set()
    on = calibration.calibrate_and_model_dpss(uvdata=uvd, fit_quality=True, **KW)
    off = calibration.calibrate_and_model_dpss(uvdata=uvd, **KW)
    np.testing.assert_array_equal(on[0].data_array, off[0].data_array)
    np.testing.assert_array_equal(on[1].data_array, off[1].data_array)
    np.testing.assert_array_equal(on[2].gain_array, off[2].gain_array)
    for t in off[3][0]:
        assert on[3][0][t]["loss"] == off[3][0][t]["loss"] and "chisq_per_baseline" not in off[3][0][t]
    assert not np.any(off[2].quality_array) and getattr(off[2], "total_quality_array", None) is None
    assert np.any(on[2].quality_array)


def test_command_line_writes_the_quality_column_and_totqlty(tmp_path, monkeypatch):
    uvd = data_set()
    data = str(tmp_path / "data.uvh5")
    uvd.write_uvh5(data)
    out = str(tmp_path / "gains.calfits")
    monkeypatch.setattr(sys, "argv", [sys.argv[0], "--input_data_files", data, "--gain_outfilename", out, "--precision", "64", "--maxsteps", "100",
                                      "--optimizer", "Adam", "--model_regularization", "sum", "--min_dly", str(2.0 / 0.3), "--offset", str(2.0 / 0.3),
                                      "--fit_quality"])
    args = calibration.dpss_fit_argparser().parse_args()
    assert args.fit_quality is True
    cli = calibration.read_calibrate_and_model_dpss(**vars(args))
    assert cli[3]["calibration_kwargs"]["fit_quality"] is True
    back = calfits.read_calfits(out)
    q, tot = np.asarray(cli[2].quality_array), np.asarray(cli[2].total_quality_array)
    assert np.any(q > 0) and np.any(tot > 0)
    np.testing.assert_array_equal(np.asarray(back.quality_array).reshape(q.shape), q)
    np.testing.assert_array_equal(np.asarray(back.total_quality_array).reshape(tot.shape), tot)
    check(copy.deepcopy(uvd), cli, "command line")
