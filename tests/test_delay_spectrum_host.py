"""The host side of the delay spectrum: modeling.delay_transform against numpy's FFT, the taper, the baseline-length bins and their
(time, bin) encoding, the keyword surface of the four calls, the header text and the build guard.  No device."""
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

from calamity_amd import _lib, batched, calibration, distributed, modeling, solver
from delay_spectrum_ref import bin_rows, restated

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F0, DF = 150e6, 400e3


@pytest.mark.parametrize("taper", ["bh4", "none", "array"])
@pytest.mark.parametrize("n", [64, 61])
def test_the_transform_is_the_shifted_fft_of_the_tapered_row(n, taper):
    rng = np.random.default_rng(n)
    x = rng.standard_normal((3, n)) + 1j * rng.standard_normal((3, n))
    t_in = rng.uniform(0.5, 1.0, n) if taper == "array" else taper
    op, norm_f, delays = modeling.delay_transform(F0 + DF * np.arange(n), taper=t_in)
    t = modeling.delay_taper(n, t_in)
    assert op.shape == (n, n) and op.dtype == np.complex128
    want = np.fft.fftshift(np.fft.fft(t * x, axis=1), axes=1)
    assert np.max(np.abs(x @ op - want)) <= 1e-12 * np.max(np.abs(want))
    np.testing.assert_array_equal(norm_f, t * t)
    np.testing.assert_allclose(delays, np.fft.fftshift(np.fft.fftfreq(n, d=DF)) * 1e9, rtol=1e-12, atol=1e-9)
    assert delays[n // 2] == 0.0


@pytest.mark.parametrize("n", [64, 61])
def test_a_pure_tone_peaks_at_its_delay(n):
    op, _, delays = modeling.delay_transform(F0 + DF * np.arange(n))
    for kp in (-n // 4, 0, 5):
        x = np.exp(2j * np.pi * np.arange(n) * kp / n)
        k = int(np.argmax(np.abs(x @ op)))
        assert k - n // 2 == kp and abs(delays[k] - kp / (n * DF) * 1e9) <= 1e-9


def test_max_delay_keeps_the_columns_inside():
    n = 64
    full = modeling.delay_transform(F0 + DF * np.arange(n))
    cut = modeling.delay_transform(F0 + DF * np.arange(n), max_delay_ns=400.0)
    keep = np.abs(full[2]) <= 400.0
    assert 0 < keep.sum() < n and keep.sum() % 2 == 1  # symmetric about zero delay
    np.testing.assert_array_equal(cut[2], full[2][keep])
    np.testing.assert_array_equal(cut[0], full[0][:, keep])
    np.testing.assert_array_equal(cut[1], full[1])
    assert modeling.delay_transform(F0 + DF * np.arange(n), max_delay_ns=0.0)[0].shape == (n, 1)


def test_bh4_is_the_four_term_blackman_harris_window():
    from scipy.signal import windows

    assert modeling.BH4_COEFFS == (0.35875, 0.48829, 0.14128, 0.01168)
    for n in (61, 64):
        t = modeling.delay_taper(n, "bh4")
        np.testing.assert_allclose(t, windows.blackmanharris(n, sym=True), rtol=0, atol=1e-15)
        assert abs(t[0] - (0.35875 - 0.48829 + 0.14128 - 0.01168)) < 1e-15 and abs(t.max() - 1.0) < 2e-3
    np.testing.assert_array_equal(modeling.delay_taper(5, "none"), np.ones(5))


def test_baseline_length_bins_and_their_time_encoding():
    lengths = np.asarray([14.6, 14.6, 29.2, 25.3, 14.9, 43.8, 0.0])
    bins, bllen = calibration.baseline_length_bins(lengths, 1.0)
    np.testing.assert_array_equal(bins, [1, 1, 3, 2, 1, 4, 0])  # floor(length / width), only the bins in use, ascending
    np.testing.assert_allclose(bllen, [0.0, (14.6 + 14.6 + 14.9) / 3, 25.3, 29.2, 43.8])
    bins, bllen = calibration.baseline_length_bins(lengths, 15.0)
    np.testing.assert_array_equal(bins, [0, 0, 1, 1, 0, 2, 0])
    dspec = dict(bin_of_bl=bins, nbins=3)
    enc = calibration.delay_spectrum_slice_bins(dspec, 3)
    assert enc.dtype == np.int32 and enc.shape == (21,)
    for t in range(3):
        np.testing.assert_array_equal(enc[7 * t : 7 * t + 7], 3 * t + bins)
    # a batch's binned arrays cut back into the slices', and the entry's mean in the data's units
    rng = np.random.default_rng(0)
    spectra = {k: rng.uniform(size=(9, 4)) for k in ("data", "model", "resid")}
    spectra["count_bin"] = np.asarray([3, 2, 1, 3, 0, 1, 3, 2, 1], dtype=np.float64)
    one = calibration.delay_spectrum_of_slice(spectra, dspec, 1, 7)
    np.testing.assert_array_equal(one["data"], spectra["data"][3:6])
    entry = calibration.delay_spectrum_entry(one, dict(dspec, delays_ns=np.arange(4.0), bllen_m=bllen), 2.0, None, None)
    np.testing.assert_array_equal(entry["nbls"], [3, 0, 1])
    np.testing.assert_allclose(entry["resid"][0], 4.0 * spectra["resid"][3] / 3.0)
    assert not np.any(entry["resid"][1])  # a bin whose rows are all flagged


def test_the_restatement_bins_sequentially_and_leaves_flagged_rows_out():
    rng = np.random.default_rng(1)
    nb, nf = 5, 8
    d, m = (rng.standard_normal((2, nb, nf)) + 1j * rng.standard_normal((2, nb, nf)))
    G = rng.standard_normal((nb, nf)) + 1j * rng.standard_normal((nb, nf))
    w = np.ones((nb, nf))
    w[2] = 0.0
    w[0, 3] = 0.0
    G[1, 2] = 0.0
    op, norm_f, _ = modeling.delay_transform(F0 + DF * np.arange(nf))
    bins = np.asarray([0, 1, 0, -1, 0])
    ref = restated(d, m, G, w, op, norm_f, bin_of_bl=bins, nbins=3)
    np.testing.assert_allclose(ref["norm_bl"], [norm_f.sum() - norm_f[3], norm_f.sum(), 0.0, norm_f.sum(), norm_f.sum()])
    np.testing.assert_array_equal(ref["count_bin"], [2, 1, 0])
    np.testing.assert_array_equal(ref["resid"][0], ref["per_baseline"]["resid"][0] + ref["per_baseline"]["resid"][4])
    assert not np.any(ref["per_baseline"]["data"][2]) and not np.any(ref["data"][2])
    x0 = np.where(w[0] != 0, d[0] - G[0] * m[0], 0.0)
    np.testing.assert_allclose(ref["per_baseline"]["resid"][0], np.abs(np.fft.fftshift(np.fft.fft(np.sqrt(norm_f) * x0))) ** 2 / ref["norm_bl"][0])
    cal = restated(d, m, G, w, op, norm_f, calibrated=True)
    assert cal["X"]["data"].shape == (nb, nf)
    x1 = np.where(np.arange(nf) == 2, 0.0, d[1] / np.where(G[1] != 0, G[1], 1.0))  # zero where |G|^2 == 0
    np.testing.assert_allclose(cal["X"]["data"][1], x1 @ op)
    assert bin_rows({"a": np.ones((2, 3))}, np.asarray([1.0, 0.0]), [0, 0], 1)["a"].tolist() == [[1.0, 1.0, 1.0]]


@pytest.mark.parametrize("bad", [dict(delay_spectrum=True, delay_spectrum_taper="hann"), dict(delay_spectrum=True, delay_spectrum_bllen_bin=0.0),
                                 dict(delay_spectrum=True, delay_spectrum_bllen_bin=-1.0), dict(delay_spectrum=True, delay_spectrum_max_dly=-5.0),
                                 dict(delay_spectrum="all")])
def test_bad_keywords_are_refused_before_anything_is_touched(bad):
    with pytest.raises(ValueError, match="delay_spectrum"):
        calibration.calibrate_and_model_tensor(None, {}, **bad)  # (no data, no device: the check comes first)
    with pytest.raises(ValueError, match="delay_spectrum"):
        calibration.calibrate_and_model_dpss(None, **bad)
    with pytest.raises(ValueError, match="delay_spectrum"):
        calibration.calibrate_and_model_mixed(None, **bad)
    with pytest.raises(ValueError, match="delay_spectrum"):
        calibration.read_calibrate_and_model_dpss(None, **bad)


def test_the_taper_and_the_delays_are_checked():
    with pytest.raises(ValueError):
        modeling.delay_transform(F0 + DF * np.arange(8), taper="hann")
    with pytest.raises(ValueError):
        modeling.delay_transform(F0 + DF * np.arange(8), taper=np.ones(7))
    with pytest.raises(ValueError):
        modeling.delay_transform(F0 + DF * np.arange(8), max_delay_ns=-1.0)
    with pytest.raises(ValueError, match="delay_spectrum_outfile"):
        calibration.read_calibrate_and_model_dpss(None, delay_spectrum_outfile="x.npz")


FIRST = {
    "calibrate_and_model_tensor": ["uvdata", "fg_model_comps_dict", "gains", "freeze_model", "optimizer", "tol", "maxsteps", "include_autos"],
    "calibrate_and_model_mixed": ["uvdata", "horizon", "min_dly", "offset", "ant_dly", "include_autos", "verbose", "red_tol"],
    "calibrate_and_model_dpss": ["uvdata", "horizon", "min_dly", "offset", "include_autos", "verbose", "red_tol", "notebook_progressbar",
                                 "fg_model_comps_dict"],
    "read_calibrate_and_model_dpss": ["input_data_files", "input_model_files", "input_gain_files", "resid_outfilename", "gain_outfilename",
                                      "model_outfilename", "fitted_info_outfilename", "x_orientation", "clobber"],
}
KEYWORDS = [("delay_spectrum", False), ("delay_spectrum_taper", "bh4"), ("delay_spectrum_max_dly", None), ("delay_spectrum_bllen_bin", 1.0),
            ("delay_spectrum_calibrated", False)]


@pytest.mark.parametrize("name", list(FIRST))
def test_the_keywords_sit_behind_the_existing_ones(name):
    params = inspect.signature(getattr(calibration, name)).parameters
    names = list(params)
    assert names[: len(FIRST[name])] == FIRST[name]  # no positional call changes
    mine = [(k, params[k].default) for k in names if k.startswith("delay_spectrum") and k != "delay_spectrum_outfile"]
    assert mine == KEYWORDS
    assert params[names[-1]].kind is inspect.Parameter.VAR_KEYWORD
    others = [k for k in names[:-1] if not k.startswith("delay_spectrum")]
    assert names[: len(others)] == others  # behind every keyword the call had
    if name == "read_calibrate_and_model_dpss":
        assert params["delay_spectrum_outfile"].default is None
    # not fit-loop controls, and no command-line flag yet
    from calamity_amd.fit_loop import FitControls

    assert not any(f.startswith("delay_spectrum") for f in FitControls().keywords())
    assert not any("delay_spectrum" in a.dest for a in calibration.dpss_fit_argparser()._actions)


def test_the_methods_and_the_binding():
    for cls in (solver.HipFitSolver, batched.SliceBatchFitter):
        params = inspect.signature(cls.delay_spectrum).parameters
        assert list(params)[1:] == ["op", "norm_f", "what", "calibrated", "bin_of_bl", "nbins", "per_baseline", "g_r", "g_i"]
        assert params["what"].default == ("data", "model", "resid") and params["calibrated"].default is False and params["nbins"].default == 0
        assert params["per_baseline"].default is False and params["bin_of_bl"].default is None
        assert hasattr(cls, "_set_delay_spectrum_scratch")
    assert [f[0] for f in _lib.DelaySpectrumDesc._fields_] == ["ndelays", "what", "calibrated", "nbins", "bin_of_bl", "op_r", "op_i", "norm_f"]
    assert _lib.DELAY_SPECTRUM_WHAT == {"data": 1, "model": 2, "resid": 4}
    lib = _lib.load()
    assert hasattr(lib, "cal_solver_delay_spectrum") and hasattr(lib, "cal_solver_set_delay_spectrum_scratch")
    spec = distributed.exchange_spec(7, 64, delay_spectrum=(3, 5, 37))
    assert spec["delay_spectrum_f64"] == 3 * 5 * 37 + 5
    assert "delay_spectrum_f64" not in distributed.exchange_spec(7, 64)  # every existing key keeps its value, and no new one appears
    assert {k: v for k, v in spec.items() if k != "delay_spectrum_f64"} == distributed.exchange_spec(7, 64)


def test_the_header_documents_the_call():
    text = open(os.path.join(ROOT, "include", "calamity_hip.h")).read()
    for word in ("cal_solver_delay_spectrum(", "cal_solver_set_delay_spectrum_scratch(", "typedef struct cal_delay_spectrum_desc", "bin_of_bl", "norm_f",
                 "power_bl[q][b][k]", "power_bin[q][n][k]", "count_bin[n]", "ONE all-reduce of", "nwhat nbins ndelays + nbins doubles", "in ascending b",
                 "bit-identical to one without it", "two calls give the same bits", "CAL_ERR_STATE", "CAL_ERR_INVALID", "|G|^2 == 0"):
        assert word in text, word


def test_the_build_guard_refuses_a_spilling_transform_kernel():
    script = os.path.join(ROOT, "calamity_amd", "csrc", "check_resources.py")

    def remarks(name, scratch, vspill, occ=2):
        return (f"./x.hpp:1:1: remark: Function Name: {name} [-Rpass-analysis=kernel-resource-usage]\n"
                f"./x.hpp:1:1: remark:     VGPRs: 250 [-Rpass-analysis=kernel-resource-usage]\n"
                f"./x.hpp:1:1: remark:     ScratchSize [bytes/lane]: {scratch} [-Rpass-analysis=kernel-resource-usage]\n"
                f"./x.hpp:1:1: remark:     Occupancy [waves/SIMD]: {occ} [-Rpass-analysis=kernel-resource-usage]\n"
                f"./x.hpp:1:1: remark:     SGPRs Spill: 0 [-Rpass-analysis=kernel-resource-usage]\n"
                f"./x.hpp:1:1: remark:     VGPRs Spill: {vspill} [-Rpass-analysis=kernel-resource-usage]\n")

    def run(text):
        return subprocess.run([sys.executable, script], input=text, capture_output=True, text=True)

    dense = remarks("_ZN4calk18fused_dense_kernelILb1EEEvNS_8MfmaArgsE", 0, 0)
    names = {k: f"_ZN4calk{len(k)}{k}IfEEvPKT_" for k in ("dspec_rows_kernel", "dspec_transform_kernel")}
    names["dspec_bin_kernel"] = "_ZN4calk16dspec_bin_kernelEPKdS1_PKiS3_iiiiiPdS4_"
    assert run(dense + "".join(remarks(n, 0, 0) for n in names.values())).returncode == 0
    for k, n in names.items():
        for scratch, vspill in ((16, 0), (0, 4)):
            bad = run(dense + remarks(n, scratch, vspill))
            assert bad.returncode != 0 and k in bad.stdout + bad.stderr, (k, scratch, vspill)
    low = run(dense + remarks(names["dspec_transform_kernel"], 0, 0, occ=1))
    assert low.returncode != 0 and "occupancy" in low.stdout + low.stderr
