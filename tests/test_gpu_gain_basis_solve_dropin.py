"""calibrate_and_model_dpss(..., gain_max_dly=100, gain_basis_solve_sweeps=N, gain_basis_solve_every=K): the closed-form sweeps of a fit
whose gains live in a frequency basis, before and between the descent steps.

The data are the projected sky of ``synthetic.make_uvdata(nants=6, nfreqs=64)`` times true gains ``1 + B y``, ``B`` the 100 ns DPSS basis
on the file's channels and ``y`` seeded and scaled so that ``g - 1`` has rms 0.1 per real part
(tests/test_gain_basis_solve_host.py: ``dropin_data_set``); the call gets that sky as ``sky_model`` with ``freeze_model=True`` and starts
from unity gains.  With ``learning_rate=1e-7`` and ``maxsteps=2`` the descent moves nothing, so what the residual loses is the sweeps'
doing.  The fp64 restatement of 30 half-damped sweeps on these very inputs brings rms(resid) / rms(data) from 0.21 (0.22 with two times)
to 1/84 (1/65) of that; the call must come within a factor 3 of the restatement's ratio (fp32, and the drop-in's own write-back)."""
import copy
import sys

import numpy as np
import pytest

from calamity_amd import calibration
from test_gain_basis_solve_host import dropin_data_set, dropin_restated_ratio

pytestmark = pytest.mark.gpu

DPSS = dict(min_dly=2.0 / 0.3, offset=2.0 / 0.3)
STILL = dict(freeze_model=True, learning_rate=1e-7, maxsteps=2, gains=None, gain_max_dly=100.0, **DPSS)


def data_set(ntimes=1):
    uvd, sky, _ = dropin_data_set(ntimes)
    return copy.deepcopy(uvd), copy.deepcopy(sky)


def resid_ratio(out, uvd):
    return float(np.sqrt(np.mean(np.abs(out[1].data_array) ** 2)) / np.sqrt(np.mean(np.abs(uvd.data_array) ** 2)))


def check_sweeps_reach_the_restatement(fn, ntimes, label, **kw):
    uvd, sky = data_set(ntimes)
    without = fn(uvdata=uvd, sky_model=sky, **STILL, **kw)
    with_sweeps = fn(uvdata=uvd, sky_model=sky, gain_basis_solve_sweeps=30, **STILL, **kw)
    r0, r1 = resid_ratio(without, uvd), resid_ratio(with_sweeps, uvd)
    ref = dropin_restated_ratio(ntimes)[1]
    print(f"{label}: rms(resid) / rms(data) {r0:.3e} without, {r1:.3e} with 30 sweeps (1/{r0 / r1:.0f}); the restatement reaches {ref:.3e}")
    assert r0 > 0.1  # the descent has moved nothing
    assert r1 <= 3.0 * ref, label
    for pol in with_sweeps[3]:
        for t in with_sweeps[3][pol]:
            assert len(with_sweeps[3][pol][t]["loss"]) == len(without[3][pol][t]["loss"]) == 2
            assert with_sweeps[3][pol][t]["gain_basis_solve_singular"] == 0 and "gain_basis_solve_singular" not in without[3][pol][t]
    return with_sweeps


def test_thirty_sweeps_in_the_loop():
    check_sweeps_reach_the_restatement(calibration.calibrate_and_model_dpss, 1, "loop", batch_slices=False)


def test_thirty_sweeps_in_a_batch_of_two_times():
    out = check_sweeps_reach_the_restatement(calibration.calibrate_and_model_dpss, 2, "batched, two times")
    assert sorted(out[3][0]) == [0, 1]


def test_thirty_sweeps_with_the_fitting_groups_on_two_workers():
    """Two workers on the one GPU (exchange through host memory): every sweep sums the three planes over them; in fp64 their gains agree
    with one worker's to 1e-10."""
    uvd, sky = data_set(2)
    one = calibration.calibrate_and_model_dpss(uvdata=uvd, sky_model=sky, gain_basis_solve_sweeps=30, dtype=np.float64, **STILL)
    two = check_sweeps_reach_the_restatement(calibration.calibrate_and_model_dpss, 2, "two workers", devices=[0, 0], device_split="groups",
                                             dtype=np.float64)
    g1, g2 = np.asarray(one[2].gain_array), np.asarray(two[2].gain_array)
    err = np.max(np.abs(g1 - g2)) / np.max(np.abs(g1))
    print(f"two workers against one, fp64: {err:.2e}")
    assert err <= 1e-10


def test_thirty_sweeps_through_calibrate_and_model_mixed():
    check_sweeps_reach_the_restatement(calibration.calibrate_and_model_mixed, 1, "mixed", ant_dly=2.0 / 0.3, red_tol_freq=0.5)


def test_sweeps_every_five_steps():
    """20 recorded steps in chunks of 5 with one sweep between the chunks: 20 losses per slice, a final loss not above the plain descent's,
    and the loop and the batch give identical results."""
    uvd, sky = data_set(2)
    kw = dict(uvdata=uvd, sky_model=sky, freeze_model=True, maxsteps=20, gains=None, gain_max_dly=100.0, **DPSS)
    plain = calibration.calibrate_and_model_dpss(**kw)
    batch = calibration.calibrate_and_model_dpss(gain_basis_solve_every=5, **kw)
    loop = calibration.calibrate_and_model_dpss(gain_basis_solve_every=5, batch_slices=False, **kw)
    for t in (0, 1):
        l_plain, l_batch, l_loop = (np.asarray(o[3][0][t]["loss"], dtype=np.float64) for o in (plain, batch, loop))
        print(f"time {t}: final loss {l_plain[-1]:.3e} plain, {l_batch[-1]:.3e} with a sweep every 5 steps")
        assert len(l_plain) == len(l_batch) == len(l_loop) == 20
        assert l_batch[-1] <= l_plain[-1]
        print(f"time {t}: loop against batch, largest loss difference {np.max(np.abs(l_batch - l_loop)):.2e}")
    for t in (0, 1):
        assert batch[3][0][t] == loop[3][0][t] and batch[3][0][t]["gain_basis_solve_singular"] == 0
    for k in (0, 1):
        np.testing.assert_array_equal(batch[k].data_array, loop[k].data_array)
    np.testing.assert_array_equal(batch[2].gain_array, loop[2].gain_array)


def test_alternating_least_squares_for_a_basis_fit():
    """Without ``freeze_model``: two rounds of [coefficient solve, 2 sweeps] end at a lower first recorded loss than two coefficient solves
    alone and than 2 sweeps alone.  No regulariser, so that the recorded loss is the chi-square both closed forms minimise.

    Why 2 sweeps.  The sky model of this data set is the true sky, so sweeps alone converge to the noise floor when given enough of
    them, while a coefficient solve at unity gains moves part of the gain error into the foregrounds (the joint problem is degenerate
    there): the comparison with the sweeps alone says something only while they are unconverged.  The fp64 restatement of the whole
    sequence on these inputs (per-baseline solves of DESIGN 3.10 and the sweeps of 3.11; chi-square of the unscaled data, 892.6 at the
    start) gives: coefficients alone 10.76; with 1, 2, 3 sweeps per round: sweeps alone 137.0, 44.6, 18.8 against both 8.68, 8.18, 7.94;
    with 5, 10, 30 sweeps: sweeps alone 4.68, 0.40, 0.13 against both 7.73, 7.60, 7.56."""
    uvd, sky = data_set(1)
    kw = dict(uvdata=uvd, sky_model=sky, learning_rate=1e-7, maxsteps=2, gains=None, gain_max_dly=100.0, model_regularization=None, **DPSS)
    first = {}
    for label, extra in (("both", dict(coeff_solve_rounds=2, gain_basis_solve_sweeps=2)), ("coefficients", dict(coeff_solve_rounds=2)),
                         ("sweeps", dict(gain_basis_solve_sweeps=2)), ("neither", dict())):
        first[label] = float(calibration.calibrate_and_model_dpss(**kw, **extra)[3][0][0]["loss"][0])
    print("first recorded loss: " + ", ".join(f"{k} {v:.3e}" for k, v in first.items()))
    assert first["both"] < first["coefficients"] and first["both"] < first["sweeps"]


def test_the_defaults_change_nothing():
    uvd, sky = data_set(2)
    kw = dict(uvdata=uvd, sky_model=sky, maxsteps=10, gains=None, gain_max_dly=100.0, **DPSS)
    for path in (dict(), dict(batch_slices=False)):
        named = calibration.calibrate_and_model_dpss(gain_basis_solve_sweeps=0, gain_basis_solve_every=0, gain_basis_solve_damping=0.5,
                                                     gain_basis_solve_ridge=1e-6, **kw, **path)
        plain = calibration.calibrate_and_model_dpss(**kw, **path)
        for k in (0, 1):
            np.testing.assert_array_equal(named[k].data_array, plain[k].data_array)
        np.testing.assert_array_equal(named[2].gain_array, plain[2].gain_array)
        for t in plain[3][0]:
            assert named[3][0][t] == plain[3][0][t] and "gain_basis_solve_singular" not in named[3][0][t]


def test_command_line_flags_reach_the_fit(tmp_path, monkeypatch):
    uvd, sky = data_set(1)
    data, model = str(tmp_path / "data.uvh5"), str(tmp_path / "model.uvh5")
    uvd.write_uvh5(data)
    sky.write_uvh5(model)
    base = [sys.argv[0], "--input_data_files", data, "--input_model_files", model, "--maxsteps", "2", "--learning_rate", "1e-7",
            "--model_regularization", "sum", "--min_dly", str(2.0 / 0.3), "--offset", str(2.0 / 0.3), "--gain_max_dly", "100"]
    ratios = []
    for extra in ([], ["--gain_basis_solve_sweeps", "30", "--gain_basis_solve_every", "0", "--gain_basis_solve_damping", "0.5", "--gain_basis_solve_ridge", "1e-6"]):
        monkeypatch.setattr(sys, "argv", base + extra)
        args = calibration.dpss_fit_argparser().parse_args()
        out = calibration.read_calibrate_and_model_dpss(**vars(args))
        ck = out[3]["calibration_kwargs"]
        assert (ck["gain_basis_solve_sweeps"], ck["gain_basis_solve_every"], ck["gain_basis_solve_damping"], ck["gain_basis_solve_ridge"]) == (
            30 if extra else 0, 0, 0.5, 1e-6)
        ratios.append(resid_ratio(out, copy.deepcopy(uvd)))
    print(f"command line: rms(resid) / rms(data) {ratios[0]:.3e} -> {ratios[1]:.3e}")
    assert ratios[0] > 0.1 and ratios[1] <= 3.0 * dropin_restated_ratio(1)[1]
