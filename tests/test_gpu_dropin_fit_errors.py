"""``fit_errors`` through the drop-in calls, on the tiny arrays of tests/test_gpu_dropin.py: the feature changes nothing it does not
add, the loop, the batched call and the file driver report the same tables, and what is absent (model_std without "samples", the
leverage tables of a frozen model, gain_std with a gain basis, the .npz without the feature) is absent."""
import os

import numpy as np
import pytest

from calamity_amd import cal_utils, calibration, synthetic, uvcompat
from calamity_amd.uvcompat import gain4

pytestmark = pytest.mark.gpu

KW = dict(min_dly=2.0 / 0.3, offset=2.0 / 0.3, gains=None, sky_model=None, maxsteps=60, tol=1e-12, correct_resid=True, correct_model=True,
          optimizer="Adam", learning_rate=1e-2)


@pytest.fixture(scope="module")
def sets():
    return synthetic.make_uvdata(nants=6, nfreqs=64, ntimes=2, seed=3, flag_frac=0.02)


@pytest.fixture(scope="module")
def fits(sets):
    """The same fit without the feature, with it, with "samples", and in the loop."""
    uvd = sets[0]
    return {name: calibration.calibrate_and_model_dpss(uvdata=uvd, **KW, **kw)
            for name, kw in (("off", {}), ("on", dict(fit_errors=True)), ("samples", dict(fit_errors="samples")),
                             ("loop", dict(fit_errors=True, batch_slices=False)))}


def test_the_feature_changes_nothing_it_does_not_add(fits):
    (m0, r0, g0, h0), (m1, r1, g1, h1) = fits["off"], fits["on"]
    assert np.array_equal(m0.data_array, m1.data_array) and np.array_equal(r0.data_array, r1.data_array)
    assert np.array_equal(g0.gain_array, g1.gain_array) and np.array_equal(g0.flag_array, g1.flag_array)
    assert np.array_equal(g0.quality_array, g1.quality_array)
    assert set(h1) - set(h0) == {"gain_std"} and "gain_std" not in h0
    for pol in h0:
        assert sorted(h0[pol]) == sorted(h1[pol])
        for t in h0[pol]:
            assert set(h1[pol][t]) - set(h0[pol][t]) == {"errors"} and "errors" not in h0[pol][t]
            for k in h0[pol][t]:
                assert np.array_equal(h0[pol][t][k], h1[pol][t][k]), k


def test_gain_std_and_the_tables(fits, sets):
    _, _, gains, hist = fits["on"]
    std = hist["gain_std"]
    flags = gain4(gains.flag_array)
    assert std.shape == gain4(gains.gain_array).shape and std.dtype == np.float64 and np.all(np.isfinite(std))
    assert np.all(std[~flags] > 0) and not np.any(std[flags])
    npairs = len(sets[0].get_antpairs())
    for t in hist[0]:
        err = hist[0][t]["errors"]
        assert set(err) == {"noise_scale", "underdetermined", "nsingular", "leverage_per_baseline", "chisq_red_per_baseline"}
        assert err["nsingular"] == 0 and err["underdetermined"] is False and err["noise_scale"] > 0
        assert len(err["leverage_per_baseline"]) == npairs and set(err["leverage_per_baseline"]) == set(err["chisq_red_per_baseline"])
        lev, red = np.array(list(err["leverage_per_baseline"].values())), np.array(list(err["chisq_red_per_baseline"].values()))
        assert np.all(lev > 0) and np.all(lev <= 64) and np.all(red > 0)


def test_the_batched_call_equals_the_loop(fits):
    """The fits are the same kernels in the same order (tests/test_gpu_dropin.py); the error pass reads the same parameters."""
    (_, _, ga, ha), (_, _, gb, hb) = fits["on"], fits["loop"]
    assert np.array_equal(ga.gain_array, gb.gain_array)
    np.testing.assert_array_equal(ha["gain_std"], hb["gain_std"])
    for t in ha[0]:
        ea, eb = ha[0][t]["errors"], hb[0][t]["errors"]
        assert ea["noise_scale"] == eb["noise_scale"] and ea["leverage_per_baseline"] == eb["leverage_per_baseline"]
        assert ea["chisq_red_per_baseline"] == eb["chisq_red_per_baseline"]


def test_samples_adds_model_std(fits, sets):
    _, _, _, hist = fits["samples"]
    for t in hist[0]:
        err, plain = hist[0][t]["errors"], fits["on"][3][0][t]["errors"]
        assert "model_std" not in plain and "antpairs" not in plain
        assert err["model_std"].dtype == np.float32 and err["model_std"].shape == (len(err["antpairs"]), 64) and np.all(np.isfinite(err["model_std"]))
        assert err["antpairs"] == list(err["leverage_per_baseline"]) and np.all(err["model_std"] > 0)
        assert err["leverage_per_baseline"] == plain["leverage_per_baseline"]


def test_a_frozen_model_gives_gain_std_only(sets):
    uvd, sky, _ = sets
    _, _, gains, hist = calibration.calibrate_and_model_dpss(uvdata=uvd, **dict(KW, sky_model=sky, model_regularization=None), freeze_model=True,
                                                             fit_errors="samples")
    assert np.all(hist["gain_std"][~gain4(gains.flag_array)] > 0)
    for t in hist[0]:
        assert set(hist[0][t]["errors"]) == {"noise_scale", "underdetermined", "nsingular"}


def test_a_gain_basis_gives_no_gain_std(sets):
    _, _, _, hist = calibration.calibrate_and_model_dpss(uvdata=sets[0], **KW, gain_max_dly=100.0, fit_errors=True)
    assert "gain_std" not in hist and all("leverage_per_baseline" in hist[0][t]["errors"] for t in hist[0])


def test_the_file_driver_writes_the_archive_only_when_asked(tmp_path, sets):
    uvd = sets[0]
    path = str(tmp_path / "fit_info.npz")
    kw = dict(input_data_files=uvd, fitted_info_outfilename=path, maxsteps=30, min_dly=2.0 / 0.3, offset=2.0 / 0.3)
    calibration.read_calibrate_and_model_dpss(**kw)
    assert not os.path.exists(path)  # as ever: nothing is written to that name
    _, _, gains, info = calibration.read_calibrate_and_model_dpss(**kw, fit_errors=True)
    assert os.path.exists(path)
    with np.load(path) as z:
        assert set(z.files) == {"noise_scale", "antpairs", "leverage_per_baseline", "chisq_red_per_baseline", "gain_std"}
        np.testing.assert_array_equal(z["gain_std"], info["gain_std"])
        assert z["leverage_per_baseline"].shape == (1, 2, len(uvd.get_antpairs())) and z["noise_scale"].shape == (1, 2)
        assert z["antpairs"].tolist() == [list(ap) for ap in info[0][0]["errors"]["leverage_per_baseline"]]
    with pytest.raises(IOError):
        calibration.read_calibrate_and_model_dpss(**kw, fit_errors=True)
