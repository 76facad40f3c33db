"""calibrate_and_model_dpss(..., gain_max_dly=100, gain_time_scale=S, gain_time_solve_sweeps=N, gain_time_solve_every=K): the closed-form
sweeps of the joint fit over the times, before and between the descent steps.

The data are the projected sky of ``synthetic.make_uvdata(nants=6, nfreqs=64, ntimes=4)`` times true gains
``1 + sum_l Bt[t, l] B y_l``, ``B`` the 100 ns DPSS basis on the file's channels, ``Bt`` the DPSS time basis of ``DROPIN_TIME_SCALE``
seconds on its times and ``y`` seeded and scaled so that ``g - 1`` has rms 0.1 per real part (tests/test_gain_time_solve_host.py:
``dropin_time_data_set``); the call gets that sky as ``sky_model`` with ``freeze_model=True`` and starts from unity gains.  With
``learning_rate=1e-7`` and ``maxsteps=2`` the descent moves nothing, so what the residual loses is the sweeps' doing.  The fp64
restatement of 30 half-damped joint sweeps on these very inputs brings rms(resid) / rms(data) from 0.19 to 1/57 of that; the call must
come within a factor 3 of the restatement's ratio (fp32, and the drop-in's own write-back)."""
import copy
import sys

import numpy as np
import pytest

from calamity_amd import calibration
from test_gain_time_solve_host import DROPIN_TIME_SCALE, dropin_time_data_set, dropin_time_restated_ratio

pytestmark = pytest.mark.gpu

DPSS = dict(min_dly=2.0 / 0.3, offset=2.0 / 0.3)
STILL = dict(freeze_model=True, learning_rate=1e-7, maxsteps=2, gains=None, gain_max_dly=100.0, gain_time_scale=DROPIN_TIME_SCALE, **DPSS)
NT = 4


def data_set():
    uvd, sky = dropin_time_data_set(NT)[:2]
    return copy.deepcopy(uvd), copy.deepcopy(sky)


def resid_ratio(out, uvd):
    return float(np.sqrt(np.mean(np.abs(out[1].data_array) ** 2)) / np.sqrt(np.mean(np.abs(uvd.data_array) ** 2)))


def test_thirty_joint_sweeps_reach_the_restatement():
    uvd, sky = data_set()
    without = calibration.calibrate_and_model_dpss(uvdata=uvd, sky_model=sky, **STILL)
    with_sweeps = calibration.calibrate_and_model_dpss(uvdata=uvd, sky_model=sky, gain_time_solve_sweeps=30, **STILL)
    r0, r1 = resid_ratio(without, uvd), resid_ratio(with_sweeps, uvd)
    ref = dropin_time_restated_ratio(NT)[1]
    print(f"rms(resid) / rms(data) {r0:.3e} without, {r1:.3e} with 30 joint sweeps (1/{r0 / r1:.0f}); the restatement reaches {ref:.3e}")
    assert r0 > 0.1  # the descent has moved nothing
    assert r1 <= 3.0 * ref
    assert sorted(with_sweeps[3][0]) == list(range(NT))
    for pol in with_sweeps[3]:
        for t in with_sweeps[3][pol]:
            assert len(with_sweeps[3][pol][t]["loss"]) == len(without[3][pol][t]["loss"]) == 2
            assert with_sweeps[3][pol][t]["gain_time_solve_singular"] == 0 and "gain_time_solve_singular" not in without[3][pol][t]


def test_joint_sweeps_every_five_steps_and_in_rounds_with_the_coefficient_solve():
    """20 recorded steps in chunks of 5 with one joint sweep between the chunks: 20 losses for the one loop of the joint fit, a final loss
    not above the plain descent's.  Without ``freeze_model``, two rounds of [coefficient solve, 2 sweeps] run and record their counts."""
    uvd, sky = data_set()
    kw = dict(uvdata=uvd, sky_model=sky, freeze_model=True, maxsteps=20, gains=None, gain_max_dly=100.0, gain_time_scale=DROPIN_TIME_SCALE, **DPSS)
    plain = calibration.calibrate_and_model_dpss(**kw)
    chunks = calibration.calibrate_and_model_dpss(gain_time_solve_every=5, **kw)
    for t in range(NT):
        l_plain, l_chunks = (np.asarray(o[3][0][t]["loss"], dtype=np.float64) for o in (plain, chunks))
        assert len(l_plain) == len(l_chunks) == 20 and l_chunks[-1] <= l_plain[-1]
        assert chunks[3][0][t] == chunks[3][0][0] and chunks[3][0][t]["gain_time_solve_singular"] == 0
    print(f"final loss {l_plain[-1]:.3e} plain, {l_chunks[-1]:.3e} with a joint sweep every 5 steps")
    kw = dict(kw, freeze_model=False, maxsteps=2, learning_rate=1e-7, model_regularization=None)
    rounds = calibration.calibrate_and_model_dpss(coeff_solve_rounds=2, gain_time_solve_sweeps=2, **kw)
    neither = calibration.calibrate_and_model_dpss(**kw)
    first = [float(o[3][0][0]["loss"][0]) for o in (rounds, neither)]
    print(f"first recorded loss: {first[0]:.3e} after two rounds, {first[1]:.3e} without")
    assert first[0] < first[1]
    assert rounds[3][0][0]["gain_time_solve_singular"] == 0 and rounds[3][0][0]["coeff_solve_singular"] == 0


def test_the_defaults_change_nothing():
    uvd, sky = data_set()
    kw = dict(uvdata=uvd, sky_model=sky, maxsteps=10, gains=None, gain_max_dly=100.0, gain_time_scale=DROPIN_TIME_SCALE, **DPSS)
    named = calibration.calibrate_and_model_dpss(gain_time_solve_sweeps=0, gain_time_solve_every=0, gain_time_solve_damping=0.5,
                                                 gain_time_solve_ridge=1e-6, **kw)
    plain = calibration.calibrate_and_model_dpss(**kw)
    for k in (0, 1):
        np.testing.assert_array_equal(named[k].data_array, plain[k].data_array)
    np.testing.assert_array_equal(named[2].gain_array, plain[2].gain_array)
    for t in plain[3][0]:
        assert named[3][0][t] == plain[3][0][t] and "gain_time_solve_singular" not in named[3][0][t]


def test_command_line_flags_reach_the_fit(tmp_path, monkeypatch):
    uvd, sky = data_set()
    data, model = str(tmp_path / "data.uvh5"), str(tmp_path / "model.uvh5")
    uvd.write_uvh5(data)
    sky.write_uvh5(model)
    base = [sys.argv[0], "--input_data_files", data, "--input_model_files", model, "--maxsteps", "2", "--learning_rate", "1e-7",
            "--model_regularization", "sum", "--min_dly", str(2.0 / 0.3), "--offset", str(2.0 / 0.3), "--gain_max_dly", "100",
            "--gain_time_scale", str(DROPIN_TIME_SCALE)]
    ratios = []
    for extra in ([], ["--gain_time_solve_sweeps", "30", "--gain_time_solve_every", "0", "--gain_time_solve_damping", "0.5", "--gain_time_solve_ridge", "1e-6"]):
        monkeypatch.setattr(sys, "argv", base + extra)
        args = calibration.dpss_fit_argparser().parse_args()
        out = calibration.read_calibrate_and_model_dpss(**vars(args))
        ck = out[3]["calibration_kwargs"]
        assert (ck["gain_time_solve_sweeps"], ck["gain_time_solve_every"], ck["gain_time_solve_damping"], ck["gain_time_solve_ridge"]) == (
            30 if extra else 0, 0, 0.5, 1e-6)
        ratios.append(resid_ratio(out, copy.deepcopy(uvd)))
    print(f"command line: rms(resid) / rms(data) {ratios[0]:.3e} -> {ratios[1]:.3e}")
    assert ratios[0] > 0.1 and ratios[1] <= 3.0 * dropin_time_restated_ratio(NT)[1]
