"""The host side of the fit errors (no GPU): the pure conversions of calibration.py against hand-computed values, the parser flags,
the keywords of the drop-in calls and the library's symbol."""
import inspect
import types

import numpy as np
import pytest

from calamity_amd import _lib, calibration

BASE = ["--input_data_files", "x.uvh5"]


def test_conversions_against_hand_computed_values():
    e = dict(nsamp_bl=np.array([10.0, 8.0, 0.0]), leverage_bl=np.array([4.0, 8.0, 0.0]), gain_var=np.array([[0.25, 0.0], [1.0, 4.0]]),
             model_var=np.array([[1.0, 4.0], [9.0, 0.0], [0.0, 0.0]]))
    a = calibration.fit_errors_arrays(e, chisq_bl=np.array([12.0, 3.0, 0.0]), rms=2.0)
    # n = 18 samples, p = 12 (leverage) + 3 (gains with den > 0) = 15, chi-square 15: noise scale 15 / 3 = 5
    assert (a["n"], a["p"], a["noise_scale"], a["underdetermined"]) == (18.0, 15.0, 5.0, False)
    np.testing.assert_array_equal(a["leverage_bl"], [4.0, 8.0, 0.0])
    assert a["chisq_red_bl"][0] == 2.0 and np.isnan(a["chisq_red_bl"][1]) and np.isnan(a["chisq_red_bl"][2])  # 12 / (10 - 4); 8 - 8 = 0; 0 - 0
    np.testing.assert_allclose(a["gain_std"], np.sqrt(5.0 * e["gain_var"]), rtol=1e-15)
    assert a["gain_std"][0, 1] == 0.0
    assert a["model_std"].dtype == np.float32
    np.testing.assert_allclose(a["model_std"], 2.0 * np.sqrt(5.0) * np.array([[1.0, 2.0], [3.0, 0.0], [0.0, 0.0]]), rtol=1e-6)


def test_a_fit_without_degrees_of_freedom_is_reported_as_such():
    e = dict(nsamp_bl=np.array([4.0, 4.0]), leverage_bl=np.array([3.5, 3.0]), gain_var=np.array([[1.0]]))
    a = calibration.fit_errors_arrays(e, chisq_bl=np.array([1.0, 1.0]))
    assert a["n"] - a["p"] == 0.5 and a["underdetermined"] is True and a["noise_scale"] == 1.0  # n - p < 1
    np.testing.assert_array_equal(a["gain_std"], [[1.0]])
    np.testing.assert_array_equal(a["chisq_red_bl"], [2.0, 1.0])
    # the gain part alone (a frozen model): no leverage tables, p counts the gains
    a = calibration.fit_errors_arrays(dict(nsamp_bl=np.array([6.0]), gain_var=np.array([[0.5, 0.0]])), chisq_bl=np.array([10.0]))
    assert "leverage_bl" not in a and "chisq_red_bl" not in a and a["p"] == 1.0 and a["noise_scale"] == 2.0
    np.testing.assert_array_equal(a["gain_std"], [[1.0, 0.0]])


def test_a_slice_is_filed_under_antenna_numbers():
    uvcal = types.SimpleNamespace(ant_array=np.array([10, 11, 12]), jones_array=np.array([-5]), x_orientation="east", time_array=np.array([2.5]))
    prob = types.SimpleNamespace(bl_ant0=np.array([0, 1]), bl_ant1=np.array([1, 2]))
    e = dict(nsamp_bl=np.array([10.0, 10.0]), leverage_bl=np.array([2.0, 4.0]), gain_var=np.full((3, 2), 0.5), model_var=np.ones((2, 2)), nsingular=1)
    gain_std, hist = np.zeros((3, 2, 1, 1)), {}
    calibration.insert_fit_errors(gain_std, uvcal, hist, 2.5, "xx", e, np.array([8.0, 6.0]), 1.0, prob)
    err = hist["errors"]
    assert err["noise_scale"] == 14.0 / (20.0 - 6.0 - 6.0) and err["nsingular"] == 1 and err["underdetermined"] is False
    assert err["leverage_per_baseline"] == {(10, 11): 2.0, (11, 12): 4.0} and err["chisq_red_per_baseline"] == {(10, 11): 1.0, (11, 12): 1.0}
    assert err["antpairs"] == [(10, 11), (11, 12)] and err["model_std"].shape == (2, 2)
    np.testing.assert_allclose(gain_std[:, :, 0, 0], np.sqrt(1.75 * 0.5))
    tables = calibration.fit_errors_tables({0: {0: hist}, "gain_std": gain_std})
    assert tables["antpairs"].tolist() == [[10, 11], [11, 12]] and tables["leverage_per_baseline"].tolist() == [[[2.0, 4.0]]]
    assert tables["noise_scale"].tolist() == [[1.75]] and tables["gain_std"].shape == (3, 2, 1, 1)


def test_parser_flags_and_keywords():
    for ap in (calibration.dpss_fit_argparser(), calibration.fitting_argparser()):
        args = ap.parse_args(BASE)
        assert args.fit_errors is False and args.fit_errors_samples is False and args.fit_errors_ridge == 1e-6
        args = ap.parse_args(BASE + ["--fit_errors", "--fit_errors_samples", "--fit_errors_ridge", "1e-3"])
        assert args.fit_errors is True and args.fit_errors_samples is True and args.fit_errors_ridge == 1e-3
    params = inspect.signature(calibration.calibrate_and_model_tensor).parameters
    assert params["fit_errors"].default is False and params["fit_errors_ridge"].default == 1e-6
    params = inspect.signature(calibration.read_calibrate_and_model_dpss).parameters
    assert params["fit_errors"].default is False and params["fit_errors_samples"].default is False and params["fit_errors_ridge"].default == 1e-6
    with pytest.raises(ValueError, match="fit_errors"):
        calibration._fit_errors_mode("all")


def test_the_library_exposes_the_symbol():
    assert "cal_solver_fit_errors" in _lib.SYMBOLS
    lib = _lib.load()
    assert lib.cal_solver_fit_errors.argtypes[1] is __import__("ctypes").c_double and len(lib.cal_solver_fit_errors.argtypes) == 8
    from calamity_amd import batched, solver

    assert inspect.signature(solver.HipFitSolver.fit_errors).parameters["ridge"].default == 1e-6
    assert set(inspect.signature(batched.SliceBatchFitter.fit_errors).parameters) >= {"ridge", "model_var", "gain_var"}
