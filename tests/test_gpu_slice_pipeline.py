"""The loop over the times against batches of one: ``calibrate_and_model_tensor(batch_slices=False)`` fits every slice on a
``HipFitSolver``, ``batch_slices=1`` on a ``SliceBatchFitter`` of one slice (``replicate_slices``); both go through the stages of
``calamity_amd.slice_pipeline``.  With every report switched on -- quality, errors, delay spectra, degeneracies -- and one time
skipped, the two calls must file the same ``fit_history`` and write the same arrays."""
import numpy as np
import pytest

from calamity_amd import calibration, synthetic

pytestmark = pytest.mark.gpu


def _flat(x, path, out):
    """Every number of a nested ``fit_history`` under its path."""
    if isinstance(x, dict):
        for k, v in x.items():
            _flat(v, f"{path}/{k}", out)
    else:
        out[path] = np.asarray(x)
    return out


@pytest.fixture(scope="module")
def calls():
    uvd, sky, _ = synthetic.make_uvdata(nants=7, nfreqs=64, ntimes=3, seed=5, redundant=True, flag_frac=0.02)
    times = np.unique(uvd.time_array)
    uvd.flag_array[np.isclose(uvd.time_array, times[1], atol=1e-7, rtol=0.0)] = True  # time 1: skipped
    # one baseline of time 0 wholly flagged: a singular group, so that the errors' nsingular is not trivially 0
    uvd.flag_array[np.isclose(uvd.time_array, times[0], atol=1e-7, rtol=0.0) & (uvd.ant_1_array == 0) & (uvd.ant_2_array == 1)] = True
    kw = dict(uvdata=uvd, min_dly=2.0 / 0.3, offset=2.0 / 0.3, gains=None, sky_model=sky, maxsteps=40, tol=1e-30, optimizer="Adam", learning_rate=1e-2,
              dtype=np.float64, correct_resid=True, fit_quality=True, fit_errors=True, delay_spectrum=True, fix_degeneracies=True)
    return calibration.calibrate_and_model_dpss(batch_slices=False, **kw), calibration.calibrate_and_model_dpss(batch_slices=1, **kw)


def test_the_loop_and_batches_of_one_file_the_same_history(calls):
    (_, _, _, h_loop), (_, _, _, h_one) = calls
    assert set(h_loop) == set(h_one) == {0, "gain_std"}
    assert sorted(h_loop[0]) == sorted(h_one[0]) == [0, 2]  # the skipped time has no entry
    for t in h_loop[0]:
        assert list(h_loop[0][t]) == list(h_one[0][t]) == ["loss", "chisq_per_baseline", "errors", "degeneracies", "delay_spectrum"]
    assert h_loop[0][0]["errors"]["nsingular"] == 1 and h_loop[0][2]["errors"]["nsingular"] == 0


def test_the_loop_equals_batches_of_one_to_the_bit(calls):
    """Measured on the parent of the commit that introduced ``slice_pipeline`` (MI355X): all 169 arrays of the two calls --
    model, residual, gains, their flags, quality and every number of ``fit_history`` -- were bit-equal, so equality is what is asserted."""
    (m_loop, r_loop, g_loop, h_loop), (m_one, r_one, g_one, h_one) = calls
    for name in ("data_array", "flag_array"):
        np.testing.assert_array_equal(getattr(m_loop, name), getattr(m_one, name), err_msg=f"model.{name}")
        np.testing.assert_array_equal(getattr(r_loop, name), getattr(r_one, name), err_msg=f"resid.{name}")
    for name in ("gain_array", "flag_array", "quality_array", "total_quality_array"):
        np.testing.assert_array_equal(getattr(g_loop, name), getattr(g_one, name), err_msg=f"gains.{name}")
    a, b = _flat(h_loop, "fit_history", {}), _flat(h_one, "fit_history", {})
    assert list(a) == list(b) and len(a) > 100
    for path in a:
        np.testing.assert_array_equal(a[path], b[path], err_msg=path)  # (NaNs in the same places compare equal here)
    assert np.any(m_loop.data_array) and len(h_loop[0][0]["loss"]) == 40
