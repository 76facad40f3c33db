"""calibrate_and_model_dpss(robust_every=K, ...): iteratively reweighted least squares through the kept entry point.

* With the four keywords at their defaults nothing changes by a bit, in the loop over the times and in batches.
* Contamination at tutorial scale (20 antennas x 64 channels, two times, fp64; noise 30 dB below the sky): (A) a fit of clean data,
  (B) the same data with 2 % of the samples moved by 30 sigma, fitted plainly, (C) the contaminated data fitted with
  ``robust_every=50, robust_kind="huber"``.  With ``g_i conj(g_j) m`` = data - residual, its rms difference to (A)'s over the
  uncontaminated unflagged samples must be strictly smaller for (C) than for (B).  The size of the improvement is not asserted; both
  figures are printed (DESIGN.md section 3.13 records a run).
* ``fit_history[pol][t]["robust"]`` has the documented keys; batches, the loop over the times and two workers agree to the
  tolerance of tests/test_gpu_dropin_batched.py (fp64: 1e-10, the residual 1e-8); the reweighting runs together with
  ``gain_solve_every`` at one chunk length and on the joint fit of a gain time basis."""
import numpy as np
import pytest

from calamity_amd import calibration, synthetic, uvcompat

pytestmark = pytest.mark.gpu

KW = dict(min_dly=2.0 / 0.3, offset=2.0 / 0.3, sky_model=None, tol=1e-14, correct_resid=False, weights=None, optimizer="Adam",
          learning_rate=1e-2, dtype=np.float64, model_regularization="sum", gains=None)
EOR_DB = -30.0


def contaminate(uvd, clean_sky, frac=0.02, nsigma=30.0, seed=1):
    """2 % of the samples moved by ``nsigma`` times the noise rms per complex sample, random phase: (contaminated copy, mask)."""
    rng = np.random.default_rng(seed)
    sigma = np.sqrt(np.mean(np.abs(clean_sky.data_array) ** 2)) * 10.0 ** (EOR_DB / 20.0)
    bad = rng.random(uvd.data_array.shape) < frac
    out = synthetic.copy_uvdata(uvd)
    out.data_array = uvd.data_array + np.where(bad, nsigma * sigma * np.exp(2j * np.pi * rng.random(uvd.data_array.shape)), 0.0)
    return out, bad


def small_set():
    uvd, sky, _ = synthetic.make_uvdata(nants=7, nfreqs=64, ntimes=3, flag_frac=0.05, eor_db=EOR_DB)
    return contaminate(uvd, sky)[0]


def same(a, b, rtol):
    assert np.linalg.norm(np.asarray(a) - np.asarray(b)) <= rtol * max(np.linalg.norm(np.asarray(b)), 1e-300)


def check_history(hist, uvd, every, maxsteps):
    nbls = len(uvd.get_antpairs())
    ants = set(int(a) for a in np.unique(np.concatenate([uvd.ant_1_array, uvd.ant_2_array])))
    for pol in hist:
        for t, h in hist[pol].items():
            rb = h["robust"]
            assert sorted(rb) == ["downweighted", "rounds", "scale"], sorted(rb)
            assert isinstance(rb["rounds"], int) and 1 <= rb["rounds"] <= (maxsteps - 1) // every
            assert len(rb["downweighted"]) == len(rb["scale"]) == nbls and sorted(rb["downweighted"]) == sorted(rb["scale"])
            for (a0, a1), n in rb["downweighted"].items():
                assert a0 in ants and a1 in ants and isinstance(n, int) and 0 <= n <= uvd.Nfreqs
            assert all(isinstance(v, float) and np.isfinite(v) and v >= 0 for v in rb["scale"].values())
            assert sum(rb["downweighted"].values()) > 0 and max(rb["scale"].values()) > 0
            assert len(h["loss"]) == maxsteps and np.all(np.isfinite(np.asarray(h["loss"], dtype=np.float64)))


@pytest.mark.parametrize("path", [dict(batch_slices=False), dict()], ids=["loop", "batched"])
def test_the_defaults_change_nothing(path):
    uvd = small_set()
    kw = dict(KW, maxsteps=100, **path)
    off = calibration.calibrate_and_model_dpss(uvdata=uvd, **kw)
    on = calibration.calibrate_and_model_dpss(uvdata=uvd, robust_every=0, robust_rounds=0, robust_kind="huber", robust_threshold=3.0, **kw)
    for k in range(2):
        np.testing.assert_array_equal(on[k].data_array, off[k].data_array)
        np.testing.assert_array_equal(on[k].flag_array, off[k].flag_array)
    np.testing.assert_array_equal(on[2].gain_array, off[2].gain_array)
    assert sorted(on[3]) == sorted(off[3])
    for pol in off[3]:
        assert sorted(on[3][pol]) == sorted(off[3][pol])
        for t in off[3][pol]:
            assert sorted(on[3][pol][t]) == sorted(off[3][pol][t]) and "robust" not in on[3][pol][t]
            assert on[3][pol][t]["loss"] == off[3][pol][t]["loss"]


def test_reweighting_brings_a_contaminated_fit_closer_to_the_clean_one():
    uvd, sky, _ = synthetic.make_uvdata(nants=20, nfreqs=64, ntimes=2, f0=150e6, df=200e3, flag_frac=0.05, eor_db=EOR_DB)
    dirty, bad = contaminate(uvd, sky)
    kw = dict(KW, maxsteps=300)
    fits = {"A": calibration.calibrate_and_model_dpss(uvdata=uvd, **kw), "B": calibration.calibrate_and_model_dpss(uvdata=dirty, **kw),
            "C": calibration.calibrate_and_model_dpss(uvdata=dirty, robust_every=50, robust_kind="huber", **kw)}
    gm = {k: (uvd if k == "A" else dirty).data_array - fits[k][1].data_array for k in fits}  # g_i conj(g_j) m = data - residual
    sel = ~bad & ~np.asarray(uvd.flag_array)
    rms = {k: float(np.sqrt(np.mean(np.abs(gm[k][sel] - gm["A"][sel]) ** 2))) for k in ("B", "C")}
    sigma = float(np.sqrt(np.mean(np.abs(sky.data_array) ** 2)) * 10.0 ** (EOR_DB / 20.0))
    print(f"rms of g g* m minus the clean fit's over {int(sel.sum())} clean samples (noise sigma {sigma:.3e}): plain {rms['B']:.4e}, "
          f"robust {rms['C']:.4e}, ratio {rms['C'] / rms['B']:.3f}")
    assert rms["C"] < rms["B"]
    check_history(fits["C"][3], dirty, 50, 300)
    for k in ("A", "B"):
        assert all("robust" not in h for pol in fits[k][3].values() for h in pol.values())
    # the outputs stay what they are: no sample is flagged by the reweighting
    for k in range(2):
        np.testing.assert_array_equal(fits["C"][k].flag_array, fits["B"][k].flag_array)
    np.testing.assert_array_equal(fits["C"][2].flag_array, fits["B"][2].flag_array)


def test_batches_the_loop_and_two_workers_agree():
    uvd = small_set()
    kw = dict(KW, maxsteps=200, uvdata=uvd, robust_every=50, robust_kind="huber", correct_resid=True)
    outs = {"loop": calibration.calibrate_and_model_dpss(batch_slices=False, **kw), "batched": calibration.calibrate_and_model_dpss(**kw),
            "two workers": calibration.calibrate_and_model_dpss(devices=[0, 0], **kw)}
    check_history(outs["batched"][3], uvd, 50, 200)
    (m1, r1, g1, h1) = outs["loop"]
    for name in ("batched", "two workers"):
        m2, r2, g2, h2 = outs[name]
        for pol in h1:
            assert sorted(h1[pol]) == sorted(h2[pol])
            for t in h1[pol]:
                np.testing.assert_allclose(np.asarray(h2[pol][t]["loss"], dtype=np.float64), np.asarray(h1[pol][t]["loss"], dtype=np.float64), rtol=1e-10)
                a, b = h1[pol][t]["robust"], h2[pol][t]["robust"]
                assert a["rounds"] == b["rounds"] == 3
                np.testing.assert_allclose([b["scale"][k] for k in sorted(a["scale"])], [a["scale"][k] for k in sorted(a["scale"])], rtol=1e-8)
        same(m2.data_array, m1.data_array, 1e-10)
        same(r2.data_array, r1.data_array, 1e-8)
        same(g2.gain_array, g1.gain_array, 1e-10)


def test_robust_rounds_bounds_the_reweights_and_fit_quality_reports_under_the_new_weights():
    uvd = small_set()
    kw = dict(KW, maxsteps=200, uvdata=uvd, robust_every=50, robust_kind="clip")
    for path in (dict(batch_slices=False), dict()):
        out = calibration.calibrate_and_model_dpss(robust_rounds=1, fit_quality=True, **kw, **path)
        plain = calibration.calibrate_and_model_dpss(fit_quality=True, **dict(KW, maxsteps=200, uvdata=uvd), **path)
        for t, h in out[3][0].items():
            assert h["robust"]["rounds"] == 1
            # clipped samples carry no weight: the weighted mean squared residual of a baseline with clipped outliers goes down
            down = [k for k, n in h["robust"]["downweighted"].items() if n > 0]
            assert down and sum(h["chisq_per_baseline"][k] for k in down) < sum(plain[3][0][t]["chisq_per_baseline"][k] for k in down)


def test_together_with_the_gain_sweeps_at_one_chunk_length():
    uvd = small_set()
    kw = dict(KW, maxsteps=200, uvdata=uvd, robust_every=50, gain_solve_every=50, gain_solve_sweeps=2, coeff_solve_rounds=1)
    for path in (dict(batch_slices=False), dict()):
        out = calibration.calibrate_and_model_dpss(**kw, **path)
        check_history(out[3], uvd, 50, 200)
        assert np.all(np.isfinite(uvcompat.gain4(out[2].gain_array)))
    with pytest.raises(ValueError, match="robust_every"):
        calibration.calibrate_and_model_dpss(**dict(kw, gain_solve_every=25))


def test_the_joint_fit_of_a_gain_time_basis():
    uvd = small_set()
    out = calibration.calibrate_and_model_dpss(uvdata=uvd, maxsteps=200, robust_every=50, gain_time_scale=1.0e6, **KW)
    check_history(out[3], uvd, 50, 200)
    rounds = {h["robust"]["rounds"] for h in out[3][0].values()}
    assert rounds == {3}  # one loop: every time reports its reweights
    out = calibration.calibrate_and_model_dpss(uvdata=uvd, maxsteps=200, robust_every=50, gain_time_scale=1.0e6, gain_time_solve_every=50,
                                               gain_time_solve_sweeps=1, **KW)
    check_history(out[3], uvd, 50, 200)
