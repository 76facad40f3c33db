"""Host side of the closed-form coefficient solves (coeff_solve_rounds / coeff_solve_ridge): the command-line flags, the defaults and
the argument checks, which are raised before any solver is created (no device is touched here)."""
import inspect
import sys

import numpy as np
import pytest

from calamity_amd import _lib, calibration


def test_parser_flags_and_defaults(monkeypatch):
    monkeypatch.setattr(sys, "argv", [sys.argv[0], "--input_data_files", "input.uvh5"])
    args = calibration.dpss_fit_argparser().parse_args()
    assert args.coeff_solve_rounds == 0 and args.coeff_solve_ridge == 1e-6
    monkeypatch.setattr(sys, "argv", [sys.argv[0], "--input_data_files", "input.uvh5", "--coeff_solve_rounds", "3", "--coeff_solve_ridge", "1e-4"])
    args = calibration.dpss_fit_argparser().parse_args()
    assert args.coeff_solve_rounds == 3 and isinstance(args.coeff_solve_rounds, int)
    assert args.coeff_solve_ridge == 1e-4 and isinstance(args.coeff_solve_ridge, float)
    for fn in (calibration.calibrate_and_model_tensor, calibration.fit_gains_and_foregrounds):
        params = inspect.signature(fn).parameters
        assert params["coeff_solve_rounds"].default == 0 and params["coeff_solve_ridge"].default == 1e-6


def test_the_binding_mirrors_the_header():
    names = [f[0] for f in _lib.CoeffSolveDesc._fields_]
    assert names == ["niters", "reset_coeff_moments", "damping", "ridge", "slice_mask"]
    assert [f[0] for f in _lib.CoeffSolveResult._fields_] == ["nsolved", "nsingular"]
    assert "cal_solver_solve_coeffs" in _lib.SYMBOLS


def test_freeze_model_is_refused_before_any_solver_exists(monkeypatch):
    def no_solver(*a, **k):
        raise AssertionError("a solver was asked for")

    monkeypatch.setattr(calibration, "get_solver", no_solver)
    monkeypatch.setattr(calibration, "_batch_fitter", no_solver)
    with pytest.raises(ValueError, match="freeze_model"):
        calibration.calibrate_and_model_tensor(None, {}, coeff_solve_rounds=1, freeze_model=True)
    z = np.zeros((2, 4))
    with pytest.raises(ValueError, match="freeze_model"):
        calibration.fit_gains_and_foregrounds(z, z, [], [], [], [], [], None, None, coeff_solve_rounds=2, freeze_model=True)
    # the sweeps stay refused with a gain basis, whatever the coefficient solves do
    with pytest.raises(ValueError, match="gain_solve_sweeps"):
        calibration.calibrate_and_model_tensor(None, {}, coeff_solve_rounds=1, gain_solve_sweeps=5, gain_max_dly=100.0)


@pytest.mark.parametrize("rounds", [-1, 1.5, "two"])
def test_bad_round_counts_are_rejected(rounds):
    with pytest.raises((ValueError, TypeError)):
        calibration.calibrate_and_model_tensor(None, {}, coeff_solve_rounds=rounds)


@pytest.mark.parametrize("ridge", [-1e-6, float("nan"), float("inf")])
def test_bad_ridges_are_rejected(ridge):
    with pytest.raises(ValueError, match="coeff_solve_ridge"):
        calibration.calibrate_and_model_tensor(None, {}, coeff_solve_rounds=1, coeff_solve_ridge=ridge)
