"""Host side of the fit-quality report (no GPU): the parser flag, the arithmetic that turns the four sums of cal_solver_fit_quality
into quality_array, total_quality_array and the per-baseline dict (known answers by hand, zero denominators, a polarization and a
time index other than 0), and the exchange payload listed by distributed.exchange_spec."""
import types

import numpy as np

from calamity_amd import calibration
from calamity_amd import distributed as D

BASE = ["--input_data_files", "x.uvh5"]


def test_parser_flag_is_off_by_default():
    ap = calibration.dpss_fit_argparser()
    assert ap.parse_args(BASE).fit_quality is False
    assert ap.parse_args(BASE + ["--fit_quality"]).fit_quality is True
    assert calibration.fitting_argparser().parse_args(BASE + ["--fit_quality"]).fit_quality is True


def sums():
    # 3 antennas, 2 channels, 2 baselines; antenna 2 has no weight in channel 1 and baseline 1 none at all
    return dict(chisq_ant=np.array([[2.0, 4.0], [1.0, 3.0], [6.0, 0.0]]), wsum_ant=np.array([[0.5, 1.0], [0.25, 0.5], [2.0, 0.0]]),
                chisq_bl=np.array([3.0, 0.0]), wsum_bl=np.array([1.5, 0.0]))


def test_known_answers_with_zero_denominators():
    per_ant, total, per_bl = calibration.fit_quality_arrays(sums(), rms=2.0)
    np.testing.assert_array_equal(per_ant, 4.0 * np.array([[4.0, 4.0], [4.0, 6.0], [3.0, 0.0]]))
    np.testing.assert_array_equal(total, 4.0 * np.array([9.0 / 2.75, 7.0 / 1.5]))
    np.testing.assert_array_equal(per_bl, np.array([8.0, 0.0]))
    assert np.all(np.isfinite(per_ant)) and np.all(np.isfinite(per_bl))
    # no weight anywhere: zeros, not NaN
    z = {k: np.zeros_like(v) for k, v in sums().items()}
    assert all(not np.any(a) and np.all(np.isfinite(a)) for a in calibration.fit_quality_arrays(z, rms=3.0))


def gains_object(total=None, spw_axis=False):
    shape = (3, 1, 2, 4, 2) if spw_axis else (3, 2, 4, 2)  # ants, (spw,) freqs, times, jones
    return types.SimpleNamespace(jones_array=np.array([-5, -6]), x_orientation="east", time_array=2458000.0 + 0.5 * np.arange(4),
                                 ant_array=np.array([10, 11, 57]), quality_array=np.zeros(shape), total_quality_array=total)


def test_insert_at_a_polarization_and_time_other_than_the_first():
    prob = types.SimpleNamespace(bl_ant0=np.array([0, 1]), bl_ant1=np.array([2, 2]))
    for spw_axis in (False, True):
        g, hist = gains_object(spw_axis=spw_axis), {"loss": [1.0]}
        calibration.insert_fit_quality(g, hist, g.time_array[2], "yy", sums(), 2.0, prob)
        q = g.quality_array[:, 0] if spw_axis else g.quality_array
        want = 4.0 * np.array([[4.0, 4.0], [4.0, 6.0], [3.0, 0.0]])
        np.testing.assert_array_equal(q[:, :, 2, 1], want)
        assert np.count_nonzero(q) == np.count_nonzero(want)  # nothing else was written
        assert g.total_quality_array.shape == (2, 4, 2)  # created: (Nfreqs, Ntimes, Njones)
        np.testing.assert_array_equal(g.total_quality_array[:, 2, 1], 4.0 * np.array([9.0 / 2.75, 7.0 / 1.5]))
        assert np.count_nonzero(g.total_quality_array) == 2
        assert hist == {"loss": [1.0], "chisq_per_baseline": {(10, 57): 8.0, (11, 57): 0.0}}  # antenna NUMBERS
    # an existing total (here with the file's spw axis) is filled in place, its other entries stay
    tot = np.full((1, 2, 4, 2), 7.0)
    g = gains_object(total=tot)
    calibration.insert_fit_quality(g, {}, g.time_array[0], "xx", sums(), 1.0, prob)
    assert g.total_quality_array is tot and tot[0, 0, 0, 0] == 9.0 / 2.75 and tot[0, 1, 0, 0] == 7.0 / 1.5 and np.count_nonzero(tot == 7.0) == 14


def test_exchange_spec_lists_the_quality_payload():
    spec = D.exchange_spec(7, 200)
    assert spec["fit_quality_f64"] == 2 * 7 * 200  # chisq_ant | wsum_ant, unpadded, one all-reduce per call
    assert spec["gain_grad_reals"] == 2 * 7 * 200 and spec["scalars_f64"] == 4  # (what a train step exchanges: unchanged)
    assert D.exchange_spec(350, 1024, reg_sum=True)["fit_quality_f64"] == 2 * 350 * 1024
