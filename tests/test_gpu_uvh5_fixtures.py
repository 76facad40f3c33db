"""The reference's integration tests on the reference's own inputs: its uvh5 fixtures (tests/golden/uvh5/), read with this
package's uvh5 reader, through the HIP fit.  Set-ups are those of test_calibration.py:17-220 (projection of the sky onto
the DPSS vectors, randomised gains, unit weights, the redundant array); acceptance criteria are the reference's own
(rms(model) and rms(data) >= 100 x rms(resid), finite outputs, model = sky to 1e-5 x rms with the model frozen).  Last,
parity of the HIP fit with the C oracle on two problems made from these files."""
import glob
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from calamity_amd import cal_utils, calibration, hdf5, modeling, problem, uvcompat, uvh5
from oracle import ref_numpy as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "uvh5")
NANT6 = "Garray_antenna_diameter2.0_fractional_spacing1.0_nant6_nf200_df100.000kHz_f0100.000MHzcompressed_True_autosFalse_{}.uvh5"
REDUNDANT = "garray_3ant_2_copies_ntimes_1compressed_False_autosTrue_{}.uvh5"
MWA = "mwa_noise_sim_realistic_flags.uvh5"


def read(name):
    return uvh5.read_uvh5(os.path.join(GOLDEN, name))


def rms(x):
    return np.sqrt(np.mean(np.abs(x) ** 2.0))


def without_autos(uvd):
    uvd.select(bls=[ap for ap in uvd.get_antpairs() if ap[0] != ap[1]], inplace=True)
    return uvd


def projected(sky, vecs):
    """test_calibration.py:140-152: every baseline's visibilities projected onto its DPSS vectors."""
    for ap in sky.get_antpairs():
        dinds = sky.antpair2ind(ap)
        if ((ap,),) not in vecs:
            ap = ap[::-1]
        apk = ((ap,),)
        sky.data_array[dinds, 0, :, 0] = (vecs[apk] @ (sky.data_array[dinds, 0, :, 0] @ vecs[apk]).T).T
    return sky


def randomized_gains(uvd, seed):
    g = cal_utils.blank_uvcal_from_uvdata(uvd)
    rng = np.random.default_rng(seed)
    g.gain_array = g.gain_array + 1e-2 * rng.standard_normal(g.gain_array.shape) + 1e-2j * rng.standard_normal(g.gain_array.shape)
    return g


@pytest.fixture(scope="module")
def nant6():
    """(sky_model_projected, uvdata = eor file + projected sky, unit weights) of test_calibration.py:17-28, :140-152, :186-198."""
    sky = without_autos(read(NANT6.format("gsm")))
    vecs = modeling.yield_pbl_dpss_model_comps(sky, offset=2.0 / 0.3, min_dly=2.0 / 0.3)
    sky = projected(sky, vecs)
    uvd = read(NANT6.format("eor_-50.0dB"))
    uvd.data_array = uvd.data_array + sky.data_array
    return sky, uvd, vecs


@pytest.fixture(scope="module")
def redundant():
    """(sky_model_projected_redundant, uvdata_redundant) of test_calibration.py:31-37, :166-178, :200-218."""
    sky = without_autos(read(REDUNDANT.format("eor_0.0dB")))
    vecs = modeling.yield_pbl_dpss_model_comps(sky, offset=2.0 / 0.3, min_dly=2.0 / 0.3)
    sky = projected(sky, vecs)
    uvd = without_autos(read(REDUNDANT.format("eor_0.0dB")))
    uvd.data_array *= 1e-4 / rms(uvd.data_array) * rms(sky.data_array)
    uvd.data_array = uvd.data_array + sky.data_array
    return sky, uvd


def weights_of(uvd):
    return uvcompat.SimpleUVFlag(uvd, mode="flag")


def test_fixture_geometry_reaches_the_fit(nant6):
    sky, uvd, vecs = nant6
    assert sky.Nbls == 15 and sky.Nfreqs == 200 and len(vecs) == 15
    assert np.allclose(sky.antenna_positions[:, 0] - sky.antenna_positions[0, 0], 2.0 * np.array([0, 1, 4, 10, 12, 17]), atol=1e-6)


@pytest.mark.parametrize("noweights, perfect_data, use_min", [(True, True, False), (True, False, False), (False, False, True), (True, True, False)])
def test_calibrate_and_model_dpss(nant6, noweights, perfect_data, use_min):
    """test_calibration.py:553-596."""
    sky, uvd, _ = nant6
    weight = None if noweights else weights_of(sky)
    if perfect_data:
        data, g0, w = sky, cal_utils.blank_uvcal_from_uvdata(sky), weight
    else:
        data, g0, w = uvd, randomized_gains(sky, 1), weights_of(sky)  # (the reference passes its weights here either way)
    model, resid, gains, fit_history = calibration.calibrate_and_model_dpss(
        min_dly=2.0 / 0.3, offset=2.0 / 0.3, uvdata=data, gains=g0, use_redundancy=False, sky_model=None, maxsteps=3000,
        tol=1e-10, correct_resid=True, correct_model=True, weights=w, use_min=use_min,
    )
    assert rms(model.data_array) >= 1e2 * rms(resid.data_array)
    assert rms(uvd.data_array) >= 1e2 * rms(resid.data_array)
    assert len(fit_history) == 1 and len(fit_history[0]) == 1


def test_calibrate_and_model_dpss_with_rfi_flags():
    """test_calibration.py:519-538 on the MWA file (2 polarizations, 2 times, realistic flags): all outputs finite."""
    uvd = read(MWA)
    assert 0 < uvd.flag_array.mean() < 1
    model, resid, gains, fit_history = calibration.calibrate_and_model_dpss(
        min_dly=4.0 / 0.3, offset=100.0, uvdata=uvd, gains=None, use_redundancy=False, sky_model=None, maxsteps=200, tol=1e-10,
        correct_resid=True, correct_model=True, weights=None, use_min=False, red_tol=0.3,
    )
    assert np.all(np.isfinite(resid.data_array)) and np.all(np.isfinite(model.data_array)) and np.all(np.isfinite(gains.gain_array))


@pytest.mark.parametrize("use_redundancy, graph_mode, nsamples_in_weights, use_model_snr_weights",
                         [(True, False, True, False), (False, False, False, False), (True, True, True, False), (False, True, False, True)])
def test_calibrate_and_model_dpss_redundant(redundant, use_redundancy, graph_mode, nsamples_in_weights, use_model_snr_weights):
    """test_calibration.py:660-696."""
    sky, uvd = redundant
    model, resid, gains, fit_history = calibration.calibrate_and_model_dpss(
        min_dly=2.0 / 0.3, offset=2.0 / 0.3, uvdata=uvd, gains=randomized_gains(sky, 2), use_redundancy=use_redundancy,
        sky_model=None, maxsteps=3000, tol=1e-10, correct_resid=False, correct_model=False, graph_mode=graph_mode,
        model_regularization="sum", use_model_snr_weights=use_model_snr_weights, nsamples_in_weights=nsamples_in_weights,
    )
    resid = cal_utils.apply_gains(resid, gains)
    model = cal_utils.apply_gains(model, gains)
    assert rms(model.data_array) >= 1e2 * rms(resid.data_array)
    assert rms(uvd.data_array) >= 1e2 * rms(resid.data_array)
    assert len(fit_history) == 1 and len(fit_history[0]) == 1


def test_calibrate_and_model_dpss_dont_correct_resid(nant6):
    """test_calibration.py:699-727."""
    sky, uvd, _ = nant6
    model, resid, gains, fit_history = calibration.calibrate_and_model_dpss(
        min_dly=2.0 / 0.3, offset=2.0 / 0.3, uvdata=uvd, gains=randomized_gains(sky, 3), use_redundancy=False, sky_model=None,
        maxsteps=3000, tol=1e-10, correct_resid=False, correct_model=False, weights=weights_of(sky),
    )
    resid = cal_utils.apply_gains(resid, gains)
    model = cal_utils.apply_gains(model, gains)
    assert rms(model.data_array) >= 1e2 * rms(resid.data_array)
    assert rms(uvd.data_array) >= 1e2 * rms(resid.data_array)
    assert len(fit_history) == 1 and len(fit_history[0]) == 1


def test_calibrate_and_model_dpss_freeze_model(nant6):
    """test_calibration.py:730-755 (its gain assertion compares the object the fit mutated with itself and is left out)."""
    sky, uvd, _ = nant6
    model, resid, gains, fit_history = calibration.calibrate_and_model_dpss(
        min_dly=2.0 / 0.3, offset=2.0 / 0.3, uvdata=sky, gains=randomized_gains(sky, 4), use_redundancy=False, sky_model=sky,
        freeze_model=True, maxsteps=3000, tol=1e-10, correct_resid=True, correct_model=True, weights=weights_of(sky),
    )
    assert rms(model.data_array) >= 1e2 * rms(resid.data_array)
    assert np.allclose(model.data_array, sky.data_array, atol=1e-5 * rms(model.data_array))
    assert len(fit_history) == 1 and len(fit_history[0]) == 1


@pytest.mark.parametrize("n_profile_steps, model_regularization, graph_mode", [(10, "post_hoc", True), (0, "post_hoc", True), (0, "sum", False)])
def test_calibrate_and_model_mixed(nant6, tmp_path, n_profile_steps, model_regularization, graph_mode):
    """test_calibration.py:772-825."""
    sky, uvd, _ = nant6
    logdir = str(tmp_path / "logdir")
    model, resid, gains, fit_history = calibration.calibrate_and_model_mixed(
        min_dly=0.0, offset=0.0, ant_dly=2.0 / 3.0, red_tol_freq=0.5, uvdata=uvd, gains=randomized_gains(sky, 5), use_redundancy=False,
        sky_model=None, freeze_model=True, maxsteps=3000, tol=1e-10, correct_resid=False, correct_model=False, weights=weights_of(sky),
        grp_size_threshold=1, graph_mode=graph_mode, n_profile_steps=n_profile_steps, profile_log_dir=logdir,
        model_regularization=model_regularization,
    )
    resid = cal_utils.apply_gains(resid, gains)
    model = cal_utils.apply_gains(model, gains)
    assert rms(model.data_array) >= 1e2 * rms(resid.data_array)
    assert rms(uvd.data_array) >= 1e2 * rms(resid.data_array)
    assert len(fit_history) == 1 and len(fit_history[0]) == 1
    if n_profile_steps > 0:
        assert len(glob.glob(logdir + "/*")) > 0


@pytest.mark.parametrize("perfect_data", [True, False])
def test_calibrate_and_model_mixed_redundant(redundant, perfect_data):
    """test_calibration.py:828-880."""
    sky, uvd = redundant
    kw = dict(min_dly=0.0, offset=0.0, ant_dly=2.0 / 0.3, red_tol_freq=0.5, use_redundancy=False, freeze_model=True, maxsteps=3000,
              correct_resid=False, correct_model=False, weights=weights_of(sky))
    if perfect_data:
        model, resid, gains, fit_history = calibration.calibrate_and_model_mixed(uvdata=sky, sky_model=sky, gains=None, **kw)
    else:
        model, resid, gains, fit_history = calibration.calibrate_and_model_mixed(uvdata=uvd, gains=randomized_gains(sky, 6), **kw)
    assert rms(model.data_array) >= 1e2 * rms(resid.data_array)
    assert rms(uvd.data_array) >= 1e2 * rms(resid.data_array)
    assert len(fit_history) == 1 and len(fit_history[0]) == 1


def h5dump_lists(path):
    exe = shutil.which("h5dump") or ("/opt/conda/bin/h5dump" if os.path.exists("/opt/conda/bin/h5dump") else None)
    if exe is None:
        return None
    out = subprocess.run([exe, "-H", path], check=True, capture_output=True, text=True).stdout
    return sorted(line.split('"')[1] for line in out.splitlines() if "DATASET" in line)


def test_read_calibrate_and_model_dpss(tmp_path, monkeypatch):
    """test_calibration.py:882-940: paths in (the reference's own input file), files out; the uvh5 outputs re-read with the
    native reader (and opened by h5dump where it is installed); then the same through the argument parser with
    --precision 64 --use_autocorrs_in_weights."""
    input_data = os.path.join(GOLDEN, REDUNDANT.format("fg_True_gleam_True_nsrc_10000"))
    gains_in = cal_utils.blank_uvcal_from_uvdata(without_autos(read(REDUNDANT.format("eor_0.0dB"))))
    gains_in.x_orientation = "east"
    gname = str(tmp_path / "gains_input.calfits")
    gains_in.write_calfits(gname)
    outs = [str(tmp_path / n) for n in ("resid_fit.uvh5", "model_fit.uvh5", "gains_fit.calfits")]
    model, resid, gains, info = calibration.read_calibrate_and_model_dpss(
        input_data_files=input_data, input_model_files=input_data, input_gain_files=gname, resid_outfilename=outs[0],
        model_outfilename=outs[1], gain_outfilename=outs[2],
    )
    names_in = sorted(f"{g}/{k}" for f in [hdf5.open(input_data)] for g in f.keys() for k in f[g].keys())
    for fn, obj in zip(outs[:2], (resid, model)):
        back = uvh5.read_uvh5(fn)
        assert np.array_equal(back.data_array, obj.data_array) and back.get_antpairs() == obj.get_antpairs()
        assert np.array_equal(back.flag_array, obj.flag_array)
        f = hdf5.open(fn)
        assert sorted(f"{g}/{k}" for g in f.keys() for k in f[g].keys()) == names_in
        listed = h5dump_lists(fn)
        assert listed is None or listed == sorted(n.split("/")[1] for n in names_in)
    assert np.all(np.isfinite(resid.data_array))
    for fn in outs:
        assert os.path.exists(fn)
        os.remove(fn)
    monkeypatch.setattr(sys, "argv", [sys.argv[0], "--input_data_files", input_data, "--input_model_files", input_data,
                                      "--input_gain_files", gname, "--resid_outfilename", outs[0], "--model_outfilename", outs[1],
                                      "--gain_outfilename", outs[2], "--precision", "64", "--use_autocorrs_in_weights"])
    args = calibration.dpss_fit_argparser().parse_args()
    _, resid2, _, info = calibration.read_calibrate_and_model_dpss(**vars(args))
    assert info["calibration_kwargs"]["dtype"] == np.float64
    for fn in outs:
        assert os.path.exists(fn)
    assert np.array_equal(uvh5.read_uvh5(outs[0]).data_array, resid2.data_array)


# ---- parity with the C oracle on problems made from the fixtures ------------------------------------------------------
def relnorm(a, b):
    a = np.asarray(a, dtype=np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def fixture_problem(uvd, vecs, pol, seed):
    """One (time, polarization) of a fixture as a FitProblem via problem_from_chunks (the reference's chunk tensors), with
    a start: gains 5 % off unity, least-squares coefficients."""
    gains = cal_utils.blank_uvcal_from_uvdata(uvd)
    ants_map = {a: i for i, a in enumerate(gains.ant_array)}
    comps, corr_inds = calibration.tensorize_fg_model_comps_dict(vecs, ants_map, nfreqs=uvd.Nfreqs, dtype=np.float64)
    padded = problem.chunks_from_problem(comps)["fg_comps"]
    t0 = np.unique(uvd.time_array)[0]
    data_r, data_i, wgts = calibration.tensorize_data(uvd, corr_inds, ants_map, polarization=pol, time=t0, dtype=np.float64,
                                                      data_scale_factor=rms(uvd.data_array))
    p = problem.problem_from_chunks(len(ants_map), padded, corr_inds, data_r, data_i, wgts)
    rng = np.random.default_rng(seed)
    start = dict(g_r=1.0 + 0.05 * rng.standard_normal((p.nants, p.nfreqs)), g_i=0.05 * rng.standard_normal((p.nants, p.nfreqs)),
                 c_r=problem.coeffs_from_chunks(p, R.tensorize_fg_coeffs(data_r, wgts, padded)),
                 c_i=problem.coeffs_from_chunks(p, R.tensorize_fg_coeffs(data_i, wgts, padded)))
    return p, start


@pytest.fixture(scope="module")
def parity_problems(nant6):
    sky, _, vecs = nant6
    out = [("nant6_xx", *fixture_problem(sky, vecs, "xx", 7))]
    mwa = read(MWA)
    mvecs = modeling.yield_pbl_dpss_model_comps(mwa, offset=100.0, min_dly=4.0 / 0.3)
    for n, pol in enumerate(("xx", "yy")):
        out.append((f"mwa_{pol}", *fixture_problem(mwa, mvecs, pol, 8 + n)))
    return out


def test_parity_with_the_c_oracle(parity_problems):
    """The 6-antenna projected sky and both polarizations of the MWA file (flagged samples at weight 0): loss and every
    gradient at the start, then 20 Adam steps, fp64 against the C oracle at 1e-10; fp32 at 1e-5 (loss) / 1e-4 (gradients)
    at the start and the fp32 trajectory tolerances of test_gpu_fullsize.py over 5 steps (losses, gains, coefficients)."""
    from calamity_amd.solver import HipFitSolver
    from oracle.ref_c import CRef

    for name, p, start in parity_problems:
        assert np.any(p.wgts == 0) == name.startswith("mwa"), name
        c = CRef(p, np.float64, nthreads=16)
        loss, og_r, og_i, oc_r, oc_i = c.loss_grads(start["g_r"], start["g_i"], start["c_r"], start["c_i"])
        fg_r, fg_i, fc_r, fc_i, flosses, _ = c.fit(start["g_r"], start["g_i"], start["c_r"], start["c_i"], 20, optimizer="Adam", learning_rate=1e-2)
        for dtype, tl, tg in ((np.float64, 1e-10, 1e-10), (np.float32, 1e-5, 1e-4)):
            s = HipFitSolver(dtype=dtype)
            s.set_problem(p)
            s.set_params(start["g_r"], start["g_i"], start["c_r"], start["c_i"])
            l2, hg_r, hg_i, hc_r, hc_i = s.eval_grads()
            assert abs(l2 - loss) <= tl * abs(loss), (name, dtype)
            assert relnorm(hg_r, og_r) <= tg and relnorm(hg_i, og_i) <= tg, (name, dtype)
            assert relnorm(hc_r, oc_r) <= tg and relnorm(hc_i, oc_i) <= tg, (name, dtype)
            s.set_optimizer("Adam", learning_rate=1e-2)
            nsteps = 20 if dtype == np.float64 else 5
            losses, stopped, nupd = s.run(nsteps, record=True, tol=0.0)
            g_r, g_i, c_r, c_i = s.get_params()
            if dtype == np.float64:
                np.testing.assert_allclose(losses, flosses, rtol=1e-10)
                assert relnorm(g_r, fg_r) <= 1e-10 and relnorm(g_i, fg_i) <= 1e-10, name
                assert relnorm(c_r, fc_r) <= 1e-10 and relnorm(c_i, fc_i) <= 1e-10, name
            else:
                og5_r, og5_i, oc5_r, oc5_i, olosses5, _ = c.fit(start["g_r"], start["g_i"], start["c_r"], start["c_i"], 5, optimizer="Adam",
                                                                learning_rate=1e-2)
                np.testing.assert_allclose(losses, olosses5, rtol=1e-4)
                # gains and coefficients after the 5 steps, at the fp32 trajectory tolerance of test_gpu_fullsize.py
                assert relnorm(g_r, og5_r) <= 1e-3 and relnorm(c_r, oc5_r) <= 1e-3 and relnorm(c_i, oc5_i) <= 1e-3, name
                dg = np.hypot(np.asarray(g_r, np.float64) - og5_r, np.asarray(g_i, np.float64) - og5_i)
                assert np.linalg.norm(dg) <= 1e-3 * np.linalg.norm(np.hypot(og5_r, og5_i)), name  # complex gains, |g - g_oracle|
            s.close()
