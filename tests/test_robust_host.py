"""Host side of the robust reweighting (no GPU): the NumPy restatement of the arithmetic (tests/robust_ref.py) against a brute-force
sort, rows with NaN and infinite samples included; its second selector (the kernel's bisection on the bit pattern) against
``np.partition`` on every row of tests/robust_families.py; the argument checks of the drop-in, the command-line flags, and that the call
adds nothing to what the ranks exchange."""
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import robust_families as RF  # noqa: E402
import robust_ref as R  # noqa: E402

from calamity_amd import calibration, synthetic  # noqa: E402
from calamity_amd import distributed as D  # noqa: E402

FLAGS = ("robust_every", "robust_rounds", "robust_kind", "robust_threshold")
DEFAULTS = (0, 0, "huber", 3.0)
BASE = ["--input_data_files", "x.uvh5"]


def brute(e_row, w_row, kind, k):
    """One row, by sorting: (weights, scale, count)."""
    idx = [f for f in range(len(e_row)) if w_row[f] > 0]
    w = np.array(w_row, dtype=np.float64)
    if not idx:
        return w, 0.0, 0
    med = sorted((float(e_row[f]) for f in idx), key=lambda v: (v != v, v))[(len(idx) + 1) // 2 - 1]  # (a NaN above every number)
    if not med > 0:
        return w, 0.0, 0
    scale, n = med / np.log(2.0), 0
    for f in idx:
        z2 = e_row[f] / scale
        if kind == "huber":
            psi = 1.0 if z2 <= k * k else k / np.sqrt(z2)
        elif kind == "cauchy":
            psi = 1.0 / (1.0 + z2 / (k * k))
        else:
            psi = 1.0 if z2 <= k * k else 0.0
        n += psi < 1.0
        w[f] = w_row[f] * psi
    return w, scale, n


@pytest.mark.parametrize("kind", R.KINDS)
def test_restatement_matches_a_brute_force_sort(kind):
    rng = np.random.default_rng(0)
    nf = 11
    good = [0, 1, 2, 7, 10, 11]  # n_b: none, one, two, odd, even, all
    e = rng.exponential(size=(len(good), nf)) * np.array([1.0, 1.0, 1.0, 1.0, 30.0, 1.0])[:, None]
    w0 = np.zeros((len(good), nf))
    for b, n in enumerate(good):
        w0[b, rng.permutation(nf)[:n]] = rng.uniform(0.5, 1.5, n)
    e[3, np.flatnonzero(w0[3])[0]] = 400.0  # an outlier among the good channels
    out = R.robust_weights(e, w0, kind, 2.0)
    for b, n in enumerate(good):
        w, scale, nd = brute(e[b], w0[b], kind, 2.0)
        np.testing.assert_array_equal(out["w"][b], w)
        assert out["scale_bl"][b] == scale and out["ndown_bl"][b] == nd, (b, n)
        if n:
            sel = w0[b] > 0
            assert scale * np.log(2.0) in e[b][sel]  # an element of the row, never an average
            assert np.sum(e[b][sel] <= scale * np.log(2.0)) >= (n + 1) // 2 > np.sum(e[b][sel] < scale * np.log(2.0))
    assert out["scale_bl"][0] == 0 and np.array_equal(out["w"][0], w0[0])
    assert out["ndown_bl"][3] >= 1
    # one and two good channels: the median is the (smaller) sample itself, z2 = ln 2 there
    assert out["scale_bl"][1] == e[1][w0[1] > 0][0] / np.log(2.0)
    assert out["scale_bl"][2] == e[2][w0[2] > 0].min() / np.log(2.0)


def test_a_row_whose_median_is_zero_keeps_its_weights():
    e = np.array([[0.0, 0.0, 5.0]])
    w0 = np.ones((1, 3))
    for kind in R.KINDS:
        out = R.robust_weights(e, w0, kind, 3.0)
        assert np.array_equal(out["w"], w0) and out["scale_bl"][0] == 0 and out["ndown_bl"][0] == 0


def same(a, b):
    """Equal, a NaN equal to a NaN."""
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


@pytest.mark.parametrize("kind", R.KINDS)
def test_restatement_matches_a_brute_force_sort_with_nan_and_inf_samples(kind):
    """Rows of 11 good channels out of 13: two NaN and an Inf (the median is a number), five NaN (the median is the largest number), six
    and nine NaN (the median is a NaN: the row keeps w0), four Inf and no NaN."""
    rng = np.random.default_rng(1)
    nf, k = 13, 2.0
    e = rng.exponential(size=(5, nf))
    w0 = rng.uniform(0.5, 1.5, (5, nf))
    w0[:, [4, 9]] = 0.0
    e[:, 4] = np.nan  # (flagged: never looked at)
    good = np.flatnonzero(w0[0])
    for b, (nnan, ninf) in enumerate([(2, 1), (5, 0), (6, 0), (9, 0), (0, 4)]):
        at = rng.permutation(good)
        e[b, at[:nnan]] = np.nan
        e[b, at[nnan : nnan + ninf]] = np.inf
    with np.errstate(invalid="ignore", divide="ignore"):
        out = R.robust_weights(e, w0, kind, k)
        for b in range(5):
            w, scale, nd = brute(e[b], w0[b], kind, k)
            assert same(out["w"][b], w) and out["scale_bl"][b] == scale and out["ndown_bl"][b] == nd, b
    for b in (2, 3):
        assert out["scale_bl"][b] == 0 and out["ndown_bl"][b] == 0 and np.array_equal(out["w"][b], w0[b])
    sel = w0[1] > 0
    assert out["scale_bl"][1] == np.nanmax(e[1][sel]) / np.log(2.0)
    for b in (0, 1, 4):
        sel = w0[b] > 0
        nan, inf, w = np.isnan(e[b]) & sel, np.isinf(e[b]) & sel, out["w"][b]
        assert np.isfinite(out["scale_bl"][b]) and out["scale_bl"][b] > 0
        assert np.all(w[inf] == 0)  # psi = 0 under every kind, and counted
        if kind == "clip":  # z2 <= k^2 is false for a NaN: weight 0, counted like every clipped sample
            assert np.all(w[nan] == 0) and out["ndown_bl"][b] == np.sum(w[sel] == 0) >= nan.sum() + inf.sum()
        else:  # psi is a NaN, and psi < 1 is false: not counted
            assert np.all(np.isnan(w[nan])) and np.all(np.isfinite(w[sel & ~nan]))
            assert out["ndown_bl"][b] == np.sum(w[sel & ~nan] < w0[b][sel & ~nan])


FAMILIES = [(np.dtype(dt).name, name) for dt in (np.float32, np.float64) for name in RF.all_families(np.float32)]


@pytest.mark.parametrize("dtype_name,family", FAMILIES, ids=["-".join(f) for f in FAMILIES])
def test_the_bit_pattern_selector_equals_np_partition(dtype_name, family):
    """``lower_median_bits`` (the kernel's bisection, restated) against ``np.partition`` on ``e`` of every row the device tests use."""
    dtype = np.dtype(dtype_name).type
    d_r, d_i, w0 = RF.all_families(dtype)[family]
    e = R.residual_power_exact(d_r, d_i, w0, dtype)
    assert e.dtype == np.dtype(dtype)
    nrows = 0
    for b in range(len(e)):
        x = e[b][w0[b] > 0]
        if not len(x):
            continue
        got, want = R.lower_median_bits(x, dtype), R.lower_median(x)
        assert got.dtype == np.dtype(dtype)
        assert same(got, want), (family, b, got, want)
        assert np.isnan(got) or got in x
        nrows += 1
    assert nrows == len(e)


def test_the_bit_pattern_selector_on_small_rows():
    for dtype in (np.float32, np.float64):
        x = np.array([3.0, 1.0, 2.0, 4.0], dtype=dtype)
        assert R.lower_median_bits(x, dtype) == 2.0 and R.lower_median_bits(x[:3], dtype) == 2.0 and R.lower_median_bits(x[:1], dtype) == 3.0
        assert R.lower_median_bits(np.array([0.0, np.inf], dtype=dtype), dtype) == 0.0
        assert R.lower_median_bits(np.array([np.inf, np.nan, 1.0], dtype=dtype), dtype) == np.inf
        assert np.isnan(R.lower_median_bits(np.array([np.nan, np.nan, 1.0], dtype=dtype), dtype))
        tiny = np.finfo(dtype).smallest_subnormal
        assert R.lower_median_bits(np.array([2 * tiny, tiny, 0.0], dtype=dtype), dtype) == tiny


def test_the_row_families_hold_what_their_names_say():
    for dtype in (np.float32, np.float64):
        fams = RF.all_families(dtype)
        fi = np.finfo(dtype)
        v, wave = RF.lanes(dtype)
        e = {name: R.residual_power_exact(*rows, dtype) for name, rows in fams.items()}
        # ties: about ten values, the median inside a run of duplicates; the one-ulp pair
        vals, cnt = np.unique(e["ties"][0], return_counts=True)
        assert 8 <= len(vals) <= 12 and cnt[list(vals).index(R.lower_median(e["ties"][0]))] > 5
        assert len(np.unique(e["ties"][2])) == 1
        srt = np.sort(e["ties"][3])
        assert srt[100] == np.nextafter(srt[99], dtype(2)) and R.lower_median(e["ties"][3]) == srt[99]
        srt = np.sort(e["ties"][4][fams["ties"][2][4] > 0])
        assert len(srt) == 199 and srt[98] == np.nextafter(srt[99], dtype(0)) and srt[99] == srt[119] == R.lower_median(srt) < srt[120]
        for name, n in (("counts_W+1", wave + 1), ("counts_2W+3", 2 * wave + 3)):
            nb = sorted(int(np.sum(w > 0)) for w in fams[name][2])
            assert set(nb) == {1, 2, 3, wave - 1, wave, wave + 1} | ({2 * wave} if n > 2 * wave else set()), (name, nb)
            assert fams[name][0].shape == (8, n)
        x = e["whole_range"][0]
        sub = (x > 0) & (x < fi.tiny)
        assert sub.sum() >= 3 and np.isinf(x).sum() > 10 and np.isinf(x).sum() < len(x) // 2 and np.sum((x >= fi.tiny) & np.isfinite(x)) > 50
        ut = {4: np.uint32, 8: np.uint64}[np.dtype(dtype).itemsize]
        keys = e["whole_range"][2].view(ut)
        assert len(np.unique(keys >> ut(8))) == 1 and len(np.unique(keys)) > 100
        for b, med in enumerate(e["zero_median"]):
            sel = fams["zero_median"][2][b] > 0
            assert (R.lower_median(med[sel]) == 0) == (b != 2) and (b != 2 or R.lower_median(med[sel]) == np.min(med[sel][med[sel] > 0]))
        for b, row in enumerate(e["non_finite"]):
            sel = fams["non_finite"][2][b] > 0
            assert np.isnan(R.lower_median(row[sel])) == (b >= 2)
        assert np.isinf(e["non_finite"][0]).sum() == 5
        assert R.lower_median(e["non_finite"][1][fams["non_finite"][2][1] > 0]) == np.nanmax(e["non_finite"][1][fams["non_finite"][2][1] > 0])


def test_parser_flags_and_defaults():
    for ap in (calibration.dpss_fit_argparser(), calibration.fitting_argparser()):
        args = ap.parse_args(BASE)
        assert tuple(getattr(args, k) for k in FLAGS) == DEFAULTS
        args = ap.parse_args(BASE + ["--robust_every", "50", "--robust_rounds", "3", "--robust_kind", "cauchy", "--robust_threshold", "2.5"])
        assert tuple(getattr(args, k) for k in FLAGS) == (50, 3, "cauchy", 2.5)
        assert isinstance(args.robust_every, int) and isinstance(args.robust_rounds, int)


def test_signature_defaults():
    from calamity_amd.batched import SliceBatchFitter
    from calamity_amd.solver import HipFitSolver

    for fn in (calibration.calibrate_and_model_tensor, calibration.fit_gains_and_foregrounds):
        params = inspect.signature(fn).parameters
        assert tuple(params[k].default for k in FLAGS) == DEFAULTS
    for fn in (HipFitSolver.robust_weights, SliceBatchFitter.robust_weights):
        params = inspect.signature(fn).parameters
        assert list(params)[1:] == ["kind", "threshold", "slice_mask"]
        assert (params["kind"].default, params["threshold"].default, params["slice_mask"].default) == ("huber", 3.0, None)
    for fn in (HipFitSolver.get_weights, SliceBatchFitter.get_weights):
        assert inspect.signature(fn).parameters["which"].default == 0


@pytest.mark.parametrize("bad", [dict(robust_every=-1), dict(robust_rounds=-1), dict(robust_every=1.5), dict(robust_every=5, robust_kind="tukey"),
                                 dict(robust_kind="none"), dict(robust_every=5, robust_threshold=0.0), dict(robust_threshold=-3.0),
                                 dict(robust_every=5, robust_threshold=float("nan")), dict(robust_every=5, use_min=True),
                                 dict(robust_every=5, gain_solve_every=10), dict(robust_every=5, gain_basis_solve_every=4, gain_max_dly=100.0)])
def test_bad_values_are_refused_before_any_device_work(bad):
    uvd, _, comps = synthetic.make_uvdata(nants=4, nfreqs=16, ntimes=2)
    with pytest.raises(ValueError, match="robust_"):
        calibration.calibrate_and_model_tensor(uvdata=uvd, fg_model_comps_dict=comps, **bad)
    loop = dict(bad)
    if loop.pop("gain_max_dly", None) is not None:
        loop["gain_basis"] = np.ones((16, 2))
    with pytest.raises(ValueError, match="robust_"):
        calibration.fit_gains_and_foregrounds(np.ones((3, 16)), np.zeros((3, 16)), None, None, None, None, None, None, None, **loop)


def test_the_solver_refuses_an_unknown_kind_without_a_device():
    from calamity_amd.solver import HipFitSolver

    s = object.__new__(HipFitSolver)  # (the check comes before anything touches the library)
    with pytest.raises(ValueError, match="kind"):
        HipFitSolver.robust_weights(s, kind="tukey")


def test_the_call_adds_nothing_to_the_exchange():
    spec = D.exchange_spec(7, 200)
    assert sorted(spec) == ["fit_quality_f64", "gain_grad_reals", "gain_solve_f64", "scalars_f64"]
    assert not any("robust" in k or "weight" in k for k in spec)
