"""Gains through real calfits files on the GPU path: the reference's file-driver test (test_calibration.py:882-940) on its
own uvh5 input with a non-unity input-gain calfits, checked bit for bit against the same fit seeded from the gain
object in memory; several input gain files; gain application with gains read back from a file."""
import copy
import os
import sys

import numpy as np
import pytest

from calamity_amd import cal_utils, calfits, calibration, fits, synthetic, utils, uvcompat, uvh5

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "uvh5")
INPUT = os.path.join(GOLDEN, "garray_3ant_2_copies_ntimes_1compressed_False_autosTrue_fg_True_gleam_True_nsrc_10000.uvh5")
MAXSTEPS = 1000


def assert_identical(a, b, where="fit_history"):
    """Nested dicts / lists of numbers and arrays, equal bit for bit."""
    if isinstance(a, dict):
        assert isinstance(b, dict) and sorted(map(str, a)) == sorted(map(str, b)), where
        for k in a:
            assert_identical(a[k], b[k], f"{where}[{k!r}]")
    elif isinstance(a, (list, tuple)):
        assert isinstance(b, (list, tuple)) and len(a) == len(b), where
        for n, (x, y) in enumerate(zip(a, b)):
            assert_identical(x, y, f"{where}[{n}]")
    elif isinstance(a, (np.ndarray, np.generic, float, int)):
        assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=np.asarray(a).dtype.kind in "fc"), where
    else:
        assert a == b, where


def assert_same_fit(got, want):
    (m1, r1, g1, h1), (m2, r2, g2, h2) = got, want
    assert np.array_equal(g1.gain_array, g2.gain_array) and np.array_equal(g1.flag_array, g2.flag_array)
    assert np.array_equal(m1.data_array, m2.data_array) and np.array_equal(r1.data_array, r2.data_array)
    assert np.array_equal(r1.flag_array, r2.flag_array)
    # (the driver adds the arguments it was called with under "calibration_kwargs")
    assert len(h1) > 0
    assert_identical(*({k: v for k, v in h.items() if k != "calibration_kwargs"} for h in (h1, h2)))


def input_gains():
    """Non-unity gains for the reference input: unity gains perturbed by 1 % (fixed seed), x_orientation east."""
    uvd = uvh5.read_uvh5(INPUT)
    uvd.select(bls=[ap for ap in uvd.get_antpairs() if ap[0] != ap[1]], inplace=True)
    g = cal_utils.blank_uvcal_from_uvdata(uvd)
    rng = np.random.default_rng(11)
    g.gain_array = g.gain_array + 1e-2 * rng.standard_normal(g.gain_array.shape) + 1e-2j * rng.standard_normal(g.gain_array.shape)
    g.x_orientation = "east"
    return g


def in_memory_fit(gains, precision, **kw):
    """What read_calibrate_and_model_dpss does with its default cuts, with the gain object itself in place of a file."""
    uvd = uvh5.read_uvh5(INPUT)
    utils.select_baselines(uvd, bllen_min=0.0, bllen_max=np.inf, bl_ew_min=0.0, ex_ants=None, select_ants=None)
    model = uvh5.read_uvh5(INPUT)
    utils.select_baselines(uvd, bllen_min=0.0, bllen_max=np.inf, bl_ew_min=0.0)
    dtype = {32: np.float32, 64: np.float64}[precision]
    return calibration.calibrate_and_model_dpss(uvdata=uvd, sky_model=model, gains=copy.deepcopy(gains), dtype=dtype, weights=None, **kw)


@pytest.mark.parametrize("precision", [32, 64])
def test_read_calibrate_and_model_dpss_with_calfits(tmp_path, monkeypatch, precision):
    g = input_gains()
    assert np.abs(g.gain_array - 1.0).max() > 1e-3
    gname = str(tmp_path / "gains_input.calfits")
    g.write_calfits(gname)
    outs = [str(tmp_path / n) for n in ("resid_fit.uvh5", "model_fit.uvh5", "gains_fit.calfits")]
    got = calibration.read_calibrate_and_model_dpss(
        input_data_files=INPUT, input_model_files=INPUT, input_gain_files=gname, resid_outfilename=outs[0],
        model_outfilename=outs[1], gain_outfilename=outs[2], precision=precision, maxsteps=MAXSTEPS,
    )
    want = in_memory_fit(g, precision, maxsteps=MAXSTEPS)
    # the gains read from the file seed the device fit exactly as the object does
    assert_same_fit(got, want)
    assert np.abs(got[2].gain_array - 1.0).max() > 1e-3 and np.all(np.isfinite(got[1].data_array))
    # the gain output is a calfits file holding the returned gains
    with open(outs[2], "rb") as f:
        assert f.read(30) == fits.SIMPLE_CARD
    back = uvcompat.read_container(outs[2])
    for name in ("gain_array", "flag_array", "quality_array"):
        assert np.array_equal(getattr(back, name), getattr(got[2], name)), name
    assert back.x_orientation == "east" and np.max(np.abs(back.time_array - got[2].time_array)) <= 1e-9
    assert np.array_equal(uvh5.read_uvh5(outs[0]).data_array, got[1].data_array)
    if precision != 64:
        return
    # the same through the argument parser
    for fn in outs:
        os.remove(fn)
    monkeypatch.setattr(sys, "argv", [sys.argv[0], "--input_data_files", INPUT, "--input_model_files", INPUT, "--input_gain_files",
                                      gname, "--resid_outfilename", outs[0], "--model_outfilename", outs[1], "--gain_outfilename",
                                      outs[2], "--precision", "64", "--maxsteps", str(MAXSTEPS)])
    args = calibration.dpss_fit_argparser().parse_args()
    cli = calibration.read_calibrate_and_model_dpss(**vars(args))
    assert cli[3]["calibration_kwargs"]["dtype"] == np.float64
    # (the parser's defaults are not calibrate_and_model_dpss's: the reference is the driver with the same arguments and
    # the gain object in place of the file)
    same = dict(vars(args), input_gain_files=copy.deepcopy(g), resid_outfilename=None, model_outfilename=None, gain_outfilename=None)
    assert_same_fit(cli, calibration.read_calibrate_and_model_dpss(**same))
    assert np.array_equal(calfits.read_calfits(outs[2]).gain_array, cli[2].gain_array)


def split_times(g, keep):
    out = copy.deepcopy(g)
    tax = np.ndim(g.gain_array) - 2
    for name in ("gain_array", "flag_array", "quality_array"):
        setattr(out, name, np.compress(keep, getattr(g, name), axis=tax))
    out.time_array, out.lst_array = g.time_array[keep], g.lst_array[keep]
    out.Ntimes = int(np.sum(keep))
    return out


@pytest.mark.parametrize("future_shapes", [False, True], ids=["spw_axis", "future_shapes"])
def test_several_gain_files(tmp_path, future_shapes):
    """Two times whose gains come in two calfits files fit exactly as with one file holding both."""
    uvd, _, _ = synthetic.make_uvdata(nants=6, nfreqs=64, ntimes=2, seed=3, future_shapes=future_shapes)
    data = str(tmp_path / "data.uvh5")
    uvd.write_uvh5(data)
    g = cal_utils.blank_uvcal_from_uvdata(uvd)
    rng = np.random.default_rng(5)
    g.gain_array = g.gain_array * (1.0 + 0.02 * rng.standard_normal(g.gain_array.shape))
    g.x_orientation = "east"
    whole, first, second = (str(tmp_path / n) for n in ("whole.calfits", "t0.calfits", "t1.calfits"))
    g.write_calfits(whole)
    split_times(g, np.array([True, False])).write_calfits(first)
    split_times(g, np.array([False, True])).write_calfits(second)
    kw = dict(input_data_files=data, maxsteps=300, precision=64)
    one = calibration.read_calibrate_and_model_dpss(input_gain_files=whole, **kw)
    two = calibration.read_calibrate_and_model_dpss(input_gain_files=[second, first], **kw)
    assert len(one[3]) > 0 and np.abs(one[2].gain_array - 1.0).max() > 1e-3
    assert_same_fit(two, one)
    with pytest.raises(ValueError, match="holds a time"):
        calibration.read_calibrate_and_model_dpss(input_gain_files=[whole, first], **kw)


def test_apply_gains_from_calfits(tmp_path):
    """Gains of a device fit, written and read back, calibrate visibilities exactly as the returned object does."""
    uvd, _, _ = synthetic.make_uvdata(nants=6, nfreqs=64, ntimes=2, seed=7, flag_frac=0.02)
    model, resid, gains, _ = calibration.calibrate_and_model_dpss(
        min_dly=2.0 / 0.3, offset=2.0 / 0.3, uvdata=uvd, gains=None, sky_model=None, maxsteps=300, tol=1e-12,
        correct_resid=False, correct_model=False,
    )
    gains.flag_array[1, ..., 5, 0, 0] = True
    path = str(tmp_path / "fit.calfits")
    gains.write_calfits(path)
    back = calfits.read_calfits(path)
    for obj in (resid, model, uvd):
        for inverse in (False, True):
            a = cal_utils.apply_gains(obj, back, inverse=inverse)
            b = cal_utils.apply_gains(obj, gains, inverse=inverse)
            assert np.array_equal(a.data_array, b.data_array) and np.array_equal(a.flag_array, b.flag_array)
    assert cal_utils.apply_gains(uvd, back).flag_array.any()
