"""Host side of the robust reweighting (no GPU): the NumPy restatement of the arithmetic (tests/robust_ref.py) against a brute-force
sort, the argument checks of the drop-in, the command-line flags, and that the call adds nothing to what the ranks exchange."""
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
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
    med = sorted(float(e_row[f]) for f in idx)[(len(idx) + 1) // 2 - 1]
    if med == 0:
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
