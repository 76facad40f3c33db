"""Host side of the closed-form gain solve (no GPU): the argument checks of the drop-in, the three parser flags, the exchange payload
and the declarations of cal_solver_solve_gains in the header and the bindings."""
import os
import re

import numpy as np
import pytest

from calamity_amd import _lib, calibration, synthetic
from calamity_amd import distributed as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ["--input_data_files", "data.uvh5"]


def test_parser_flags_and_defaults():
    for ap in (calibration.dpss_fit_argparser(), calibration.fitting_argparser()):
        args = ap.parse_args(BASE)
        assert (args.gain_solve_sweeps, args.gain_solve_every, args.gain_solve_damping) == (0, 0, 0.5)
        args = ap.parse_args(BASE + ["--gain_solve_sweeps", "30", "--gain_solve_every", "5", "--gain_solve_damping", "0.25"])
        assert (args.gain_solve_sweeps, args.gain_solve_every, args.gain_solve_damping) == (30, 5, 0.25)
        assert isinstance(args.gain_solve_sweeps, int) and isinstance(args.gain_solve_every, int)


@pytest.mark.parametrize("solve", [dict(gain_solve_sweeps=3), dict(gain_solve_every=5)])
@pytest.mark.parametrize("basis", ["gain_basis", "gain_max_dly", "gain_time_scale", "gain_time_basis"])
def test_a_gain_basis_and_the_closed_form_are_refused_together(solve, basis):
    uvd, _, comps = synthetic.make_uvdata(nants=4, nfreqs=16, ntimes=2)
    value = {"gain_basis": np.ones((16, 1)), "gain_max_dly": 100.0, "gain_time_scale": 1e6, "gain_time_basis": np.ones((2, 1))}[basis]
    with pytest.raises(ValueError, match="gain_solve"):  # before any device work: this test has no GPU
        calibration.calibrate_and_model_tensor(uvdata=uvd, fg_model_comps_dict=comps, **{basis: value}, **solve)


@pytest.mark.parametrize("bad", [dict(gain_solve_sweeps=-1), dict(gain_solve_every=-2), dict(gain_solve_sweeps=1.5),
                                 dict(gain_solve_sweeps=1, gain_solve_damping=0.0), dict(gain_solve_every=1, gain_solve_damping=1.5)])
def test_bad_values_are_refused(bad):
    uvd, _, comps = synthetic.make_uvdata(nants=4, nfreqs=16)
    with pytest.raises(ValueError, match="gain_solve"):
        calibration.calibrate_and_model_tensor(uvdata=uvd, fg_model_comps_dict=comps, **bad)
    with pytest.raises(ValueError, match="gain_solve"):
        calibration.fit_gains_and_foregrounds(None, None, None, None, None, None, None, None, None, **bad)


def test_fit_gains_and_foregrounds_refuses_the_combination_too():
    with pytest.raises(ValueError, match="gain_solve"):
        calibration.fit_gains_and_foregrounds(np.ones((3, 8)), np.zeros((3, 8)), None, None, None, None, None, None, None, gain_basis=np.ones((8, 1)),
                                              gain_solve_sweeps=2)


def test_exchange_spec_names_the_payload():
    spec = D.exchange_spec(7, 64)
    assert spec["gain_solve_f64"] == 3 * 7 * 64  # num_r | num_i | den, unpadded, one all-reduce per sweep
    assert D.exchange_spec(350, 1024, reg_sum=True)["gain_solve_f64"] == 3 * 350 * 1024
    assert spec["fit_quality_f64"] == 2 * 7 * 64 and spec["scalars_f64"] == 4  # the others as before


def test_the_call_is_declared_in_the_header_and_the_bindings():
    with open(os.path.join(ROOT, "include", "calamity_hip.h")) as f:
        header = f.read()
    assert re.search(r"int\s+cal_solver_solve_gains\s*\(\s*cal_solver\s*\*\s*s\s*,\s*const\s+cal_gain_solve_desc\s*\*\s*desc\s*\)\s*;", header)
    fields = re.search(r"typedef struct cal_gain_solve_desc \{(.*?)\} cal_gain_solve_desc;", header, re.S).group(1)
    assert [m for m in re.findall(r"(\w+)\s*;", fields)] == ["nsweeps", "reset_gain_moments", "damping", "slice_mask"]
    assert [n for n, _ in _lib.GainSolveDesc._fields_] == ["nsweeps", "reset_gain_moments", "damping", "slice_mask"]
    with open(os.path.join(ROOT, "calamity_amd", "_lib.py")) as f:
        assert '"cal_solver_solve_gains"' in f.read()
    import ctypes as C

    assert C.sizeof(_lib.GainSolveDesc) == 24  # int32, int32, double, pointer
