"""calibrate_and_model_dpss(..., fix_degeneracies=True | "band"): the written gains and model refer to the sky model.

Set-up: a 7-antenna hexagon (redundant fitting groups: ``use_redundancy``, so the classic degeneracies are all that is free), two
times, data = true gains x (sky + noise 80 dB down), the sky model handed over, the starting gains moved away from the true ones by a
known amplitude and tilt (1 rad on the longest baseline), different at the two times.  One closed-form coefficient solve at the
starting gains (``coeff_solve_rounds=1``) puts the model on sky x (the inverse transformation); the descent steps behind it polish.
With the model free the fit cannot remove the offset: the oracle's fit on the CPU (oracle.ref_numpy, the same set-up in solver units,
noise 1e-4) ends with the amplitude offset 0.200 and the tilt 1.009 rad it was given, and the restatement of the fix brings them to
1e-4 and 2e-4 rad.

The tolerance of the written gains is measured, not assumed: the restatement (tests/degeneracy_ref.py) applied to the raw outputs of the
run WITHOUT the keyword must give the run with it, at the parity tolerance of tests/test_gpu_degeneracy.py (fp64: 1e-10).

Batched against looped: the fits themselves agree to rounding only (a batch runs the multi-slice kernels; tests/test_gpu_dropin_batched.py
holds them to 1e-9), so the outputs are compared bit for bit where the raw fits are bit-identical and at that 1e-9 otherwise; that the fix
itself gives a slice of a batch the bits of the slice alone is tests/test_gpu_degeneracy.py::test_two_slices_equal_two_solvers_bit_for_bit."""
import copy
import functools

import numpy as np
import pytest

import degeneracy_ref as R
from calamity_amd import cal_utils, calibration, synthetic, uvcompat

pytestmark = pytest.mark.gpu

NA, NF, NT = 7, 32, 2
ETA0 = (0.2, -0.15)  # per time


@functools.lru_cache(maxsize=None)
def data_set():
    uvd, sky, _ = synthetic.make_uvdata(nants=NA, nfreqs=NF, ntimes=NT, redundant=True, eor_db=-80.0, flag_frac=0.05)
    rng = np.random.default_rng(7)
    gains = cal_utils.blank_uvcal_from_uvdata(uvd)
    ants = np.asarray(gains.ant_array)
    pos = {int(a): np.asarray(x, dtype=np.float64)[:2] for a, x in zip(uvd.antenna_numbers, uvd.antenna_positions)}
    antpos = np.asarray([pos[int(a)] for a in ants])
    g_true = (1 + 0.05 * rng.normal(size=(NA, NF))) * np.exp(0.2j * rng.normal(size=(NA, NF)))
    row = {int(a): n for n, a in enumerate(ants)}
    i1 = np.asarray([row[int(a)] for a in uvd.ant_1_array])
    i2 = np.asarray([row[int(a)] for a in uvd.ant_2_array])
    vis = uvcompat.vis3(uvd.data_array)
    vis[:, :, 0] *= g_true[i1] * np.conj(g_true[i2])
    longest = max(np.linalg.norm(antpos[a] - antpos[b]) for a in range(NA) for b in range(NA))
    start = np.empty((NA, NF, NT), dtype=np.complex128)
    for t in range(NT):
        phi = rng.normal(size=2)
        phi *= 1.0 / (np.linalg.norm(phi) * longest)  # 1 rad over the longest baseline along the tilt
        start[:, :, t] = g_true * np.exp(ETA0[t]) * np.exp(1j * (antpos @ phi))[:, None]
    uvcompat.gain4(gains.gain_array)[:, :, :, 0] = start
    return dict(uvd=uvd, sky=sky, gains=gains, g_true=g_true, antpos=antpos, start=start, i1=i1, i2=i2, longest=longest)


KW = dict(min_dly=2.0 / 0.3, offset=2.0 / 0.3, maxsteps=200, tol=0.0, correct_resid=False, weights=None, optimizer="Adam", learning_rate=1e-3,
          model_regularization=None, use_redundancy=True, coeff_solve_rounds=1)


@functools.lru_cache(maxsize=None)
def fitted(route, mode, dtype="float64", errors=False):
    ds = data_set()
    kw = dict(KW, dtype=np.dtype(dtype).type, sky_model=ds["sky"], gains=copy.deepcopy(ds["gains"]), **({"batch_slices": False} if route == "loop" else {}),
              **({"fit_errors": True} if errors else {}))
    if mode is not False:
        kw.update(fix_degeneracies=mode)
    return calibration.calibrate_and_model_dpss(uvdata=ds["uvd"], **kw)


def gains_at(out, t):
    return np.array(uvcompat.gain4(out[2].gain_array)[:, :, t, 0])


def rows_at(t):
    uvd = data_set()["uvd"]
    return np.where(np.isclose(uvd.time_array, np.unique(uvd.time_array)[t], atol=1e-7, rtol=0.0))[0]


def offsets(g, t):
    """The largest amplitude offset (mean over the antennas of log |g / g_true|) and array phase gradient (a plane through the phases
    of g / g_true over the antenna positions, times the longest baseline: radians) over the channels."""
    ds = data_set()
    rho = g / ds["g_true"]
    amp = np.abs(np.mean(np.log(np.abs(rho)), axis=0)).max()
    ph = np.angle(rho * np.conj(rho.mean(axis=0))[None, :])
    sol = np.linalg.lstsq(np.c_[ds["antpos"], np.ones(NA)], ph, rcond=None)[0]
    return float(amp), float((np.hypot(sol[0], sol[1]) * ds["longest"]).max())


def restated(off, t, mode="channel"):
    """The restatement on the raw outputs of the run without the keyword, time index ``t``."""
    ds = data_set()
    uvd, sky, rows = ds["uvd"], ds["sky"], rows_at(t)
    m = np.array(uvcompat.vis3(off[0].data_array)[rows, :, 0])
    s = np.array(uvcompat.vis3(sky.data_array)[rows, :, 0])
    w = (~uvcompat.vis3(uvd.flag_array)[rows, :, 0] & ~uvcompat.vis3(sky.flag_array)[rows, :, 0]).astype(np.float64)
    return R.fix_degeneracies(m, s, w, gains_at(off, t), ds["i1"][rows], ds["i2"][rows], ds["antpos"], iters=6, mode=mode,
                              freqs=np.asarray(uvd.freq_array, dtype=np.float64).ravel(), gref=ds["start"][:, :, t]), rows


def nerr(got, want):
    return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))


@pytest.mark.parametrize("route", ["batched", "loop"])
def test_the_written_gains_refer_to_the_sky_model(route):
    on, off = fitted(route, True, errors=True), fitted(route, False, errors=True)
    assert sorted(on[3][0]) == [0, 1]
    for t in range(NT):
        ref, rows = restated(off, t)
        e = on[3][0][t]["degeneracies"]
        errs = dict(g=nerr(gains_at(on, t), ref["g"]), model=nerr(np.array(uvcompat.vis3(on[0].data_array)[rows, :, 0]), ref["model"]),
                    amplitude=nerr(e["amplitude"], np.exp(ref["eta"])), tilt=nerr(e["tilt"], ref["tilt"]),
                    phase=float(np.max(np.abs(np.angle(np.exp(1j * (e["phase"] - ref["psi"])))))))
        raw, fixed = offsets(gains_at(off, t), t), offsets(gains_at(on, t), t)
        print(f"{route} time {t}: " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f"  offsets (amplitude, gradient) raw {raw} fixed {fixed}")
        assert max(errs.values()) <= 1e-10, (route, t, errs)
        np.testing.assert_array_equal(e["nsamples"], ref["nsamples"])
        assert raw[0] >= 0.1 and raw[1] >= 0.5, "the fit kept the offset it was started with"
        assert fixed[0] <= raw[0] / 100.0 and fixed[1] <= raw[1] / 100.0, (route, t, raw, fixed)
        assert e["last_step"].max() < 1e-6


@pytest.mark.parametrize("dtype,tol", [("float64", 1e-11), ("float32", 1e-5)])
def test_the_residual_does_not_change(dtype, tol):
    on, off = fitted("batched", True, dtype), fitted("batched", False, dtype)
    rms = np.sqrt(np.mean(np.abs(data_set()["uvd"].data_array) ** 2))
    diff = float(np.max(np.abs(np.asarray(on[1].data_array) - np.asarray(off[1].data_array))) / rms)
    print(f"{dtype}: largest change of the residual / data rms {diff:.2e}")
    assert diff <= tol
    assert not np.array_equal(on[2].gain_array, off[2].gain_array)


def test_batched_equals_looped():
    on_b, on_l, off_b, off_l = (fitted(r, m, errors=True) for r, m in (("batched", True), ("loop", True), ("batched", False), ("loop", False)))
    raw_equal = np.array_equal(off_b[2].gain_array, off_l[2].gain_array) and np.array_equal(off_b[0].data_array, off_l[0].data_array)
    print("the raw fits of the two routes are", "bit-identical" if raw_equal else "equal to rounding only")
    pairs = [(on_b[2].gain_array, on_l[2].gain_array), (on_b[0].data_array, on_l[0].data_array)]
    pairs += [(on_b[3][0][t]["degeneracies"][k], on_l[3][0][t]["degeneracies"][k]) for t in range(NT) for k in ("amplitude", "phase", "tilt", "last_step")]
    for a, b in pairs:
        if raw_equal:
            np.testing.assert_array_equal(a, b)
        else:
            assert np.linalg.norm(np.asarray(a) - np.asarray(b)) <= 1e-9 * max(np.linalg.norm(np.asarray(b)), 1e-300) + 1e-12
    for t in range(NT):
        np.testing.assert_array_equal(on_b[3][0][t]["degeneracies"]["nsamples"], on_l[3][0][t]["degeneracies"]["nsamples"])


def test_band_mode_is_one_amplitude_and_a_phase_linear_in_frequency():
    on, off = fitted("batched", "band"), fitted("batched", False)
    ds = data_set()
    freqs = np.asarray(ds["uvd"].freq_array, dtype=np.float64).ravel()
    for t in range(NT):
        e = on[3][0][t]["degeneracies"]
        assert e["mode"] == "band" and np.ptp(e["amplitude"]) == 0.0
        rho = gains_at(on, t) / gains_at(off, t)  # e^{-eta} e^{-i (Phi(f).r_a + psi(f))}
        assert np.max(np.abs(np.abs(rho) * e["amplitude"][None, :] - 1.0)) <= 1e-12
        tilt = np.angle(rho[1:] * np.conj(rho[:1])) / freqs[None, :]  # -(Phi_0 / nu_ref).(r_a - r_0): the same at every channel
        assert np.max(np.abs(tilt - tilt[:, :1])) * freqs.mean() <= 1e-10
        ref, _ = restated(off, t, mode="band")
        assert nerr(gains_at(on, t), ref["g"]) <= 1e-10 and nerr(e["tilt"], ref["tilt"]) <= 1e-10


def test_the_history_entry_and_gain_std():
    on, off = fitted("batched", True, errors=True), fitted("batched", False, errors=True)
    for t in range(NT):
        assert "degeneracies" not in off[3][0][t]
        e = on[3][0][t]["degeneracies"]
        assert set(e) == {"mode", "amplitude", "phase", "tilt", "nsamples", "iters", "last_step"}
        assert e["mode"] == "channel" and e["iters"] == 6
        assert all(e[k].shape == (NF,) for k in ("amplitude", "phase", "nsamples", "last_step")) and e["tilt"].shape == (NF, 2)
        assert set(on[3][0][t]) - {"degeneracies"} == set(off[3][0][t])
        assert on[3][0][t]["loss"] == off[3][0][t]["loss"]
        s_on, s_off = on[3]["gain_std"][:, :, t, 0], off[3]["gain_std"][:, :, t, 0]
        assert np.any(s_off > 0)
        np.testing.assert_allclose(s_on, s_off / e["amplitude"][None, :], rtol=1e-13)


def test_the_file_driver_forwards_the_keywords():
    ds = data_set()
    kw = {k: v for k, v in KW.items() if k != "weights"}
    out = calibration.read_calibrate_and_model_dpss(copy.deepcopy(ds["uvd"]), input_model_files=copy.deepcopy(ds["sky"]),
                                                    input_gain_files=copy.deepcopy(ds["gains"]), precision=64, fix_degeneracies="band",
                                                    degeneracy_iters=4, degeneracy_phase_ref=False, **kw)
    for t in range(NT):
        e = out[3][0][t]["degeneracies"]
        assert e["mode"] == "band" and e["iters"] == 4 and not e["phase"].any()
    with pytest.raises(ValueError, match="sky_model"):
        calibration.read_calibrate_and_model_dpss(copy.deepcopy(ds["uvd"]), precision=64, fix_degeneracies=True, **kw)
