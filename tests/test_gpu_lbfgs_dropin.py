"""The L-BFGS iterations through the drop-in entry points (``lbfgs_steps``, ``lbfgs_every``, ...), on the tiny arrays of
tests/test_gpu_dropin.py (6 antennas, 64 channels, 2 times).

* With the five keywords at their defaults nothing changes by a bit.
* ``lbfgs_steps=10`` files ``fit_history[...]["lbfgs"]`` and ends on a lower loss than the same call without it.
* Batches and the loop over the times agree bit for bit, the history entry included.
* It runs together with ``gain_max_dly``, with ``gain_time_scale`` and with ``freeze_model=True``: the fits the Gauss-Newton step refuses.
* Several devices that share out the fitting groups are refused; the file driver and the command line pass the keywords on."""
import sys

import numpy as np
import pytest

from calamity_amd import calibration, synthetic, uvcompat

pytestmark = pytest.mark.gpu

KW = dict(min_dly=2.0 / 0.3, offset=2.0 / 0.3, sky_model=None, tol=1e-14, correct_resid=False, weights=None, optimizer="Adam",
          learning_rate=1e-2, dtype=np.float64, model_regularization="sum", gains=None)
KEYS = ["calls", "evals", "iters", "loss", "status"]


def small_set():
    return synthetic.make_uvdata(nants=6, nfreqs=64, ntimes=2, seed=3)[0]


def check_history(hist, calls, steps):
    for pol in hist:
        for t, h in hist[pol].items():
            lb = h["lbfgs"]
            assert sorted(lb) == KEYS, sorted(lb)
            assert lb["calls"] == calls and 0 < lb["iters"] <= calls * steps and lb["evals"] >= lb["iters"] and len(lb["loss"]) == calls
            assert all(isinstance(x, float) and np.isfinite(x) for x in lb["loss"]) and lb["status"] in (0, 1, 2)


def test_the_defaults_change_nothing():
    uvd = small_set()
    kw = dict(KW, maxsteps=40)
    off = calibration.calibrate_and_model_dpss(uvdata=uvd, **kw)
    on = calibration.calibrate_and_model_dpss(uvdata=uvd, lbfgs_steps=0, lbfgs_every=0, lbfgs_history=8, lbfgs_max_ls=20, lbfgs_ftol=0.0, **kw)
    for k in range(2):
        np.testing.assert_array_equal(on[k].data_array, off[k].data_array)
    np.testing.assert_array_equal(on[2].gain_array, off[2].gain_array)
    for pol in off[3]:
        for t in off[3][pol]:
            assert sorted(on[3][pol][t]) == sorted(off[3][pol][t]) and "lbfgs" not in on[3][pol][t]
            assert on[3][pol][t]["loss"] == off[3][pol][t]["loss"]


def test_ten_iterations_end_lower_and_batches_equal_the_loop():
    uvd = small_set()
    kw = dict(KW, maxsteps=30, uvdata=uvd)
    plain = calibration.calibrate_and_model_dpss(**kw)
    (m1, r1, g1, h1), (m2, r2, g2, h2) = (calibration.calibrate_and_model_dpss(batch_slices=False, lbfgs_steps=10, **kw),
                                          calibration.calibrate_and_model_dpss(lbfgs_steps=10, **kw))
    check_history(h2, 1, 10)
    for pol in h2:
        for t in h2[pol]:
            assert "lbfgs" not in plain[3][pol][t]
            a, b = float(h2[pol][t]["loss"][-1]), float(plain[3][pol][t]["loss"][-1])
            print(f"pol {pol} time {t}: final loss {a:.4e} with the iterations, {b:.4e} without; {h2[pol][t]['lbfgs']}")
            assert a < b
            assert h1[pol][t]["lbfgs"] == h2[pol][t]["lbfgs"] and h1[pol][t]["loss"] == h2[pol][t]["loss"], (pol, t)
    np.testing.assert_array_equal(m2.data_array, m1.data_array)
    np.testing.assert_array_equal(r2.data_array, r1.data_array)
    np.testing.assert_array_equal(g2.gain_array, g1.gain_array)


@pytest.mark.parametrize("extra", [dict(gain_max_dly=200.0), dict(gain_time_scale=600.0), dict(freeze_model=True),
                                   dict(gain_max_dly=200.0, gain_time_scale=600.0, freeze_model=True)],
                         ids=["gain_max_dly", "gain_time_scale", "freeze_model", "all three"])
def test_together_with_gain_bases_and_a_frozen_model(extra):
    uvd = small_set()
    kw = dict(KW, maxsteps=20, uvdata=uvd, lbfgs_steps=4, lbfgs_every=10, lbfgs_history=3, **extra)
    out = calibration.calibrate_and_model_dpss(**kw)
    check_history(out[3], 2, 4)
    assert all(len(h["loss"]) == 20 for h in out[3][0].values())
    assert np.all(np.isfinite(uvcompat.gain4(out[2].gain_array)))


def test_refusals_of_the_keywords():
    uvd = small_set()
    kw = dict(KW, maxsteps=20, uvdata=uvd, lbfgs_steps=2)
    with pytest.raises(ValueError, match="lbfgs.*device_split"):
        calibration.calibrate_and_model_dpss(**dict(kw, devices=[0, 0], device_split="groups"))
    with pytest.raises(ValueError, match="same value"):
        calibration.calibrate_and_model_dpss(**dict(kw, lbfgs_every=10, robust_every=5))
    with pytest.raises(ValueError, match="lbfgs_steps"):
        calibration.calibrate_and_model_dpss(**dict(kw, lbfgs_steps=0, lbfgs_every=10))


def test_the_file_driver_and_the_command_line_pass_the_keywords_on(tmp_path, monkeypatch):
    uvd = small_set()
    data_path = str(tmp_path / "data.uvh5")
    uvd.write_uvh5(data_path)
    out = calibration.read_calibrate_and_model_dpss(input_data_files=data_path, maxsteps=10, lbfgs_steps=3, lbfgs_history=2, lbfgs_max_ls=9, lbfgs_ftol=1e-9)
    check_history({0: out[3][0]}, 1, 3)
    assert out[3]["calibration_kwargs"]["lbfgs_steps"] == 3
    monkeypatch.setattr(sys, "argv", [sys.argv[0], "--input_data_files", data_path, "--maxsteps", "10", "--lbfgs_steps", "3", "--lbfgs_history", "2",
                                      "--lbfgs_max_ls", "9", "--lbfgs_ftol", "1e-9", "--gpu_index", "0"])
    args = calibration.dpss_fit_argparser().parse_args()
    again = calibration.read_calibrate_and_model_dpss(**vars(args))
    check_history({0: again[3][0]}, 1, 3)
    # (the parser's defaults of the other arguments are its own, so the numbers differ: the shape of the entry is what the flags decide)
    assert sorted(again[3][0]) == sorted(out[3][0]) and all(h["lbfgs"]["iters"] <= 3 for h in again[3][0].values())
    assert again[3]["calibration_kwargs"]["lbfgs_history"] == 2 and again[3]["calibration_kwargs"]["lbfgs_max_ls"] == 9
