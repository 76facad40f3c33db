"""The three ways in which ``fit_loop.drive`` addresses a one-slice ``HipFitSolver`` differently from the loop it replaced in
``fit_gains_and_foregrounds``: ``run_slices`` for ``run``, a one-entry mask of ones for no mask, ``hold_slices`` with nothing held.
Each gives the bits of the other: equalities, no tolerance.  The problem is the drop-in tests' ``synthetic.make_uvdata(nants=6,
nfreqs=64)`` (15 baselines), tensorized as ``calibrate_and_model_tensor`` does, gains 10 % off unity, coefficients from
``init_coeffs``, Adamax; every case starts two solvers from that same state."""
import functools

import numpy as np
import pytest

from calamity_amd import cal_utils, calibration, modeling, synthetic

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]


@functools.lru_cache(maxsize=None)
def problem():
    uvd, _, comps = synthetic.make_uvdata(nants=6, nfreqs=64)
    ants_map = {ant: i for i, ant in enumerate(np.asarray(cal_utils.blank_uvcal_from_uvdata(uvd).ant_array).tolist())}
    prob, _ = calibration.tensorize_fg_model_comps_dict(comps, ants_map, nfreqs=uvd.Nfreqs, dtype=np.float64)
    rms = float(np.sqrt(np.mean(np.abs(uvd.data_array) ** 2)))
    data = calibration._tensorize_flat(uvd, prob, ants_map, "xx", uvd.time_array[0], data_scale_factor=rms, dtype=np.float64)
    rng = np.random.default_rng(3)
    gains = 1.0 + 0.1 * rng.standard_normal((2, prob.nants, prob.nfreqs))
    basis = np.array(modeling.gain_dpss_basis(np.asarray(uvd.freq_array, dtype=np.float64).ravel(), 20.0))  # 5 vectors
    assert prob.nbls == 15 and basis.shape == (64, 5)
    return prob, data, gains, basis


@pytest.fixture
def pair():
    """``pair(dtype, with_basis=False)``: two solvers in the same state, closed when the test ends."""
    from calamity_amd.solver import HipFitSolver

    def start(dtype, with_basis=False):
        prob, (d_r, d_i, w), gains, basis = problem()
        for _ in range(2):
            s = HipFitSolver(dtype=dtype)
            made.append(s)
            s.set_problem(prob, layout="shared")
            s.set_data(d_r, d_i, w)
            s.init_coeffs(d_r, d_i)
            s.set_params(gains[0], gains[1])
            if with_basis:
                s.set_gain_basis(basis)
            s.set_regularization(None)
            s.set_optimizer("Adamax")
        return made[-2:]

    made = []
    yield start
    for s in made:
        s.close()


def same(a, b):
    if isinstance(a, dict):
        assert sorted(a) == sorted(b)
        a, b = [a[k] for k in sorted(a)], [b[k] for k in sorted(b)]
    if isinstance(a, (list, tuple)):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            same(x, y)
    elif a is None:
        assert b is None
    else:
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b))


def same_state(a, b, moments=True):
    same(a.get_params(), b.get_params())
    same(a.get_weights(), b.get_weights())
    if moments:
        same(a.get_moments(), b.get_moments())


@pytest.mark.parametrize("dtype", DTYPES)
def test_run_slices_is_run(pair, dtype):
    a, b = pair(dtype)
    ra, (rb,) = a.run(20, tol=0.0), b.run_slices(20, tol=0.0)
    assert len(ra[0]) == 20 and ra[0][-1] < ra[0][0]
    same(ra, rb)
    same_state(a, b)


CALLS = {"solve_gains": lambda s, **kw: s.solve_gains(2, **kw), "solve_coeffs": lambda s, **kw: s.solve_coeffs(**kw),
         "solve_gain_coeffs": lambda s, **kw: s.solve_gain_coeffs(2, **kw), "robust_weights": lambda s, **kw: s.robust_weights("huber", 3.0, **kw)}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("call", list(CALLS))
def test_a_mask_of_ones_is_no_mask(pair, dtype, call):
    a, b = pair(dtype, with_basis=call == "solve_gain_coeffs")
    before = (*a.get_params(), a.get_weights())
    same(CALLS[call](a), CALLS[call](b, slice_mask=[1]))
    same_state(a, b, moments=False)
    assert any(not np.array_equal(x, y) for x, y in zip(before, (*a.get_params(), a.get_weights())))  # the call did something


@pytest.mark.parametrize("dtype", DTYPES)
def test_nothing_held_is_no_hold(pair, dtype):
    a, b = pair(dtype)
    b.hold_slices([0])
    same(a.run(10), b.run(10))
    same_state(a, b)
    b.hold_slices(None)
    same(a.run(3), b.run(3))
