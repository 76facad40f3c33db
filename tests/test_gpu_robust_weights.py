"""cal_solver_robust_weights on the device against the NumPy restatement of tests/robust_ref.py (include/calamity_hip.h):

    e = w0 |d - g_i conj(g_j) (A c)|^2,  med_b = lower median of e over the row's samples with w0 > 0,  scale_b = med_b / ln 2,
    z2 = e / scale_b,  huber / cauchy / clip psi(z2; k),  w = w0 psi

The restatement is evaluated in float64 from ``solver.model()``, the data, ``w0`` (``get_weights(1)``) and the gains the solver holds, so
the only difference to the device is that the device forms ``e`` in its dtype.  Parameters are the start values perturbed by about
10 % (|residual| ~ |data|, no cancellation).  Tolerances: ``scale_bl`` and the Huber and Cauchy weights, both continuous in ``e``,
rtol 1e-10 in fp64 and 1e-4 in fp32.  Clip weights and ``ndown_bl`` are exact except for samples whose reference ``z2`` lies within 1e-3
relative of ``k^2``: those are left out and must be at most 0.1 % of the samples.  The padding channels [nfreqs, fpad) cannot be read
through the interface; that they stay zero shows in the loss, which sums over them.

Problems: 8 antennas (28 baselines) x {37, 300} channels, seed 0, an autocorrelation row appended (29 rows: not a multiple of the four
rows of a block), row 0 fully flagged, row 1 with one good channel, row 2 with two.

What this file leaves to others.  The tolerances above cannot see a median that is one rank off or a bit dropped in the last rounds of
the bisection, and the samples near the threshold are left out: tests/test_gpu_robust_exact.py compares the device bit for bit where ``e``
can be reproduced exactly (ties at the median, every count around a trip of the wave, the whole key range, zero medians, NaN and
infinite samples, both forms at the LDS limit, a descent continued behind the form that keeps its keys in the model plane).
tests/test_gpu_robust_consumers.py checks what reads the rewritten plane: fit quality, the four closed-form solves, ``init_coeffs``, the
loss and the gradients on every kernel path."""
import copy
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import robust_ref as R  # noqa: E402

from calamity_amd import _lib, batched, modeling, synthetic  # noqa: E402
from calamity_amd.problem import FitProblem  # noqa: E402

pytestmark = pytest.mark.gpu

RTOL = {np.dtype(np.float64): 1e-10, np.dtype(np.float32): 1e-4}
LOSS_TOL = {np.dtype(np.float64): 1e-10, np.dtype(np.float32): 1e-5}  # sums of the loss kind (tests/test_gpu_fit_quality.py)
K = 3.0
DTYPES = [np.float32, np.float64]


def perturbed(p, start, seed):
    rng = np.random.default_rng(seed)
    gs = (p.nants, p.nfreqs)
    return dict(g_r=start["g_r"] + 0.1 * rng.standard_normal(gs), g_i=start["g_i"] + 0.1 * rng.standard_normal(gs),
                c_r=start["c_r"] * (1.0 + 0.1 * rng.standard_normal(p.ncoeffs)), c_i=start["c_i"] * (1.0 + 0.1 * rng.standard_normal(p.ncoeffs)))


def edge_flags(p):
    p.wgts = p.wgts.copy()
    p.wgts[0, :] = 0.0
    keep = p.wgts[1, 5]
    p.wgts[1, :] = 0.0
    p.wgts[1, 5] = keep if keep > 0 else p.wgts.max()
    p.wgts[2, :] = 0.0
    p.wgts[2, [3, p.nfreqs - 1]] = p.wgts.max()
    return p


@functools.lru_cache(maxsize=None)
def edge_problem(nfreqs, autos=True):
    p0, _, start = synthetic.make_problem(8, nfreqs, f0=150e6, df=400e3, seed=0)
    params = perturbed(p0, start, seed=6)
    if not autos:
        return edge_flags(p0), params
    rng = np.random.default_rng(9)
    nv = p0.basis[0].shape[1]
    p = FitProblem(nants=p0.nants, nfreqs=p0.nfreqs, basis=p0.basis, grp_basis=np.concatenate([p0.grp_basis, [0]]).astype(np.int32),
                   grp_bl_start=np.arange(p0.nbls + 2, dtype=np.int32), bl_ant0=np.concatenate([p0.bl_ant0, [2]]).astype(np.int32),
                   bl_ant1=np.concatenate([p0.bl_ant1, [2]]).astype(np.int32), bl_rowblk=np.zeros(p0.nbls + 1, dtype=np.int32),
                   data_r=np.concatenate([p0.data_r, rng.standard_normal((1, p0.nfreqs))]),
                   data_i=np.concatenate([p0.data_i, rng.standard_normal((1, p0.nfreqs))]),
                   wgts=np.concatenate([p0.wgts, np.full((1, p0.nfreqs), p0.wgts.max())]))
    p.validate()
    params = dict(params, c_r=np.concatenate([params["c_r"], rng.standard_normal(nv)]), c_i=np.concatenate([params["c_i"], rng.standard_normal(nv)]))
    return edge_flags(p), params


def solver_of(p, params, dtype, layout="shared", kernel_path="auto"):
    from calamity_amd.solver import HipFitSolver

    s = HipFitSolver(dtype=dtype)
    s.set_problem(p, layout=layout, kernel_path=kernel_path)
    s.set_params(params["g_r"], params["g_i"], params["c_r"], params["c_i"])
    return s


def reference(s, p, kind, k=K, data=None):
    """The restatement at what the solver holds now: its model, gains and w0; the data as the solver rounded them."""
    d_r, d_i = (np.asarray(a).astype(s.dtype) for a in (data if data is not None else (p.data_r, p.data_i)))
    m_r, m_i = s.model()
    g_r, g_i = s.get_params()[:2]
    w0 = s.get_weights(1)
    e = R.residual_power(m_r, m_i, d_r, d_i, w0, g_r, g_i, p.bl_ant0, p.bl_ant1)
    return dict(R.robust_weights(e, w0, kind, k), e=e, w0=w0.astype(np.float64))


def check(out, w, ref, kind, dtype, label, rows=None, k=K):
    """Device outputs against the restatement on ``rows`` (default: all); returns the largest relative errors seen."""
    rows = np.arange(len(ref["w"])) if rows is None else np.asarray(rows)
    rtol = RTOL[np.dtype(dtype)]
    w, rw = np.asarray(w, dtype=np.float64)[rows], ref["w"][rows]
    scale, rscale = out["scale_bl"][rows], ref["scale_bl"][rows]
    assert out["scale_bl"].dtype == np.float64 and out["ndown_bl"].dtype == np.float64
    e_scale = float(np.max(np.abs(scale - rscale) / np.where(rscale > 0, rscale, 1.0)))
    z2 = ref["z2"][rows]
    near = np.abs(z2 - k * k) <= 1e-3 * k * k  # (NaN outside S_b: False)
    n_samples = int(np.sum(np.isfinite(z2)))
    if kind == "clip":
        e_w = float(np.max(np.abs(w - rw)[~near], initial=0.0))
    else:
        e_w = float(np.max((np.abs(w - rw) / np.where(rw != 0, np.abs(rw), 1.0)), initial=0.0))
    # the count with the near-threshold samples left out on both sides (Huber and clip; Cauchy has no threshold)
    thr = kind != "cauchy"
    got_down = (w < ref["w0"][rows]) & ~(near & thr)
    want_down = (rw < ref["w0"][rows]) & ~(near & thr)
    print(f"{label} {kind}: scale {e_scale:.2e}  weights {e_w:.2e}  near the threshold {int(near.sum())} of {n_samples}")
    assert np.all((rscale > 0) == (scale > 0)), label
    assert e_scale <= rtol, (label, kind, e_scale)
    assert near.sum() <= 1e-3 * max(n_samples, 1), (label, int(near.sum()), n_samples)
    if kind == "clip":
        assert e_w == 0.0, (label, e_w)
        np.testing.assert_array_equal(got_down, want_down, err_msg=label)
    else:
        assert e_w <= rtol, (label, kind, e_w)
    if thr:
        slack = np.sum(near, axis=1)
        assert np.all(np.abs(out["ndown_bl"][rows] - ref["ndown_bl"][rows]) <= slack), (label, kind)
    else:
        np.testing.assert_array_equal(out["ndown_bl"][rows], ref["ndown_bl"][rows], err_msg=label)
    flagged = ref["w0"][rows] <= 0
    assert np.all(w[flagged] == 0.0), label  # flagged samples keep their zero
    return e_scale, e_w


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", ["stream", "shared"])
@pytest.mark.parametrize("nfreqs", [37, 300])
def test_parity_with_the_numpy_restatement(nfreqs, layout, dtype):
    p, params = edge_problem(nfreqs)
    assert p.nbls == 29 and p.bl_ant0[-1] == p.bl_ant1[-1]
    s = solver_of(p, params, dtype, layout)
    w_in = s.get_weights(0)
    np.testing.assert_array_equal(w_in, p.wgts.astype(dtype))
    np.testing.assert_array_equal(s.get_weights(1), w_in)  # before any call w0 is the plane itself
    loss0 = s.eval_loss()
    for kind in R.KINDS:
        ref = reference(s, p, kind)
        out = s.robust_weights(kind=kind, threshold=K)
        w = s.get_weights(0)
        assert w.dtype == np.dtype(dtype) and w.shape == (p.nbls, p.nfreqs)
        check(out, w, ref, kind, dtype, f"({nfreqs}) {layout} {np.dtype(dtype).name}")
        np.testing.assert_array_equal(s.get_weights(1), w_in)  # every call starts from w0 and leaves it alone
        # the rows without a median to speak of: none, one and two good channels
        assert out["scale_bl"][0] == 0 and out["ndown_bl"][0] == 0 and not np.any(w[0])
        assert out["scale_bl"][1] > 0 and out["scale_bl"][2] > 0
        if kind != "cauchy":
            assert out["ndown_bl"][1] == 0 and w[1, 5] == w_in[1, 5]  # z2 = ln 2 at the row's own median
        # every kernel path reads this plane: the loss is the chi-square under the new weights (and sums over the padding)
        want = float(np.sum(ref["e"] * np.divide(w.astype(np.float64), ref["w0"], out=np.zeros_like(ref["e"]), where=ref["w0"] > 0)))
        loss = s.eval_loss()
        assert abs(loss - want) <= LOSS_TOL[np.dtype(dtype)] * want, (kind, loss, want)
        assert loss < loss0 or kind != "clip" or out["ndown_bl"].sum() == 0
    # kind "none" puts w0 back bit for bit, and with it the loss
    out = s.robust_weights(kind="none")
    np.testing.assert_array_equal(s.get_weights(0), w_in)
    assert not np.any(out["scale_bl"]) and not np.any(out["ndown_bl"])
    assert s.eval_loss() == loss0
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_dense_kernel_path(dtype):
    """SHARED layout, one baseline per group, 300 channels: the matrix-core kernels (no silent fall-back), which read the same plane."""
    p, params = edge_problem(300, autos=False)
    s = solver_of(p, params, dtype, "shared", "dense")
    assert s.timing_get()["kernel_path"] == "dense"
    for kind in ("huber", "clip"):
        ref = reference(s, p, kind)
        out = s.robust_weights(kind=kind)
        w = s.get_weights()
        check(out, w, ref, kind, dtype, f"dense {np.dtype(dtype).name}")
        want = float(np.sum(ref["e"] * np.divide(w.astype(np.float64), ref["w0"], out=np.zeros_like(ref["e"]), where=ref["w0"] > 0)))
        loss = s.eval_loss()
        assert abs(loss - want) <= LOSS_TOL[np.dtype(dtype)] * want, (kind, loss, want)
    s.close()


def test_rows_longer_than_the_lds_form():
    """fp64 keeps rows of up to 2048 padded channels in LDS; 2100 channels take the form that keeps the keys in the model plane."""
    p, _, start = synthetic.make_problem(4, 2100, f0=150e6, df=40e3, seed=0)
    params = perturbed(p, start, seed=5)
    s = solver_of(p, params, np.float64)
    for kind in ("huber", "clip"):
        ref = reference(s, p, kind)
        first = s.robust_weights(kind=kind)
        w = s.get_weights()
        check(first, w, ref, kind, np.float64, "2100 channels float64")
        again = s.robust_weights(kind=kind)
        np.testing.assert_array_equal(s.get_weights(), w)
        np.testing.assert_array_equal(again["scale_bl"], first["scale_bl"])
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_calls_give_the_same_bits_and_nothing_else_changes(dtype):
    p, params = edge_problem(300)
    s = solver_of(p, params, dtype, "stream")
    s.set_optimizer("Adam", learning_rate=1e-2)
    s.run(3)
    before = s.get_params(0)
    for kind in R.KINDS:
        a = s.robust_weights(kind=kind)
        wa = s.get_weights()
        b = s.robust_weights(kind=kind)
        np.testing.assert_array_equal(s.get_weights(), wa)
        for k in ("scale_bl", "ndown_bl"):
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    for x, y in zip(before, s.get_params(0)):
        np.testing.assert_array_equal(x, y)
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_second_call_after_a_descent_step_starts_from_w0(dtype):
    p, params = edge_problem(300)
    s = solver_of(p, params, dtype)
    s.set_optimizer("Adam", learning_rate=1e-2)
    first = s.robust_weights(kind="huber", threshold=2.0)
    w_first = s.get_weights()
    assert first["ndown_bl"].sum() > 0 and np.any(w_first < p.wgts.astype(dtype))
    s.run(5, tol=0.0)
    ref = reference(s, p, "huber", k=2.0)  # at the new parameters
    np.testing.assert_array_equal(ref["w0"], p.wgts.astype(dtype).astype(np.float64))
    second = s.robust_weights(kind="huber", threshold=2.0)
    w_second = s.get_weights()
    # (cumulative shrinking would have given w_first psi, not w0 psi)
    check(second, w_second, ref, "huber", dtype, f"second call {np.dtype(dtype).name}", k=2.0)
    assert not np.array_equal(w_first, w_second)
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_set_data_after_a_call_gives_the_next_call_new_weights(dtype):
    p, params = edge_problem(37)
    s = solver_of(p, params, dtype)
    s.robust_weights(kind="clip", threshold=1.0)
    rng = np.random.default_rng(3)
    w_new = p.wgts * rng.uniform(0.5, 1.5, p.wgts.shape)
    s.set_data(p.data_r, p.data_i, w_new)
    np.testing.assert_array_equal(s.get_weights(0), w_new.astype(dtype))
    np.testing.assert_array_equal(s.get_weights(1), w_new.astype(dtype))
    ref = reference(s, p, "huber")
    out = s.robust_weights(kind="huber")
    np.testing.assert_array_equal(s.get_weights(1), w_new.astype(dtype))
    check(out, s.get_weights(), ref, "huber", dtype, f"after set_data {np.dtype(dtype).name}")
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", ["stream", "shared"])
def test_fitting_groups_of_several_baselines(layout, dtype):
    p0, _, start0 = synthetic.make_problem(7, 200, f0=150e6, df=400e3, seed=13)
    p, start = synthetic.add_redundant_group(p0, start0, np.random.default_rng(1), nred=3)
    assert np.diff(p.grp_bl_start).max() == 3 and p.nbls % 4 != 0
    params = perturbed(p, start, seed=14)
    s = solver_of(p, params, dtype, layout)
    for kind in ("huber", "cauchy"):
        ref = reference(s, p, kind)
        out = s.robust_weights(kind=kind)
        check(out, s.get_weights(), ref, kind, dtype, f"redundant group {layout} {np.dtype(dtype).name}")
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_with_a_frequency_gain_basis_attached(dtype):
    p, params = edge_problem(300)
    s = solver_of(p, params, dtype)
    s.set_gain_basis(np.array(modeling.gain_dpss_basis(150e6 + 400e3 * np.arange(p.nfreqs), 100.0)))
    s.set_optimizer("Adam", learning_rate=1e-2)
    s.run(4, tol=0.0)  # y moves: the gains are g0 + B y
    assert np.any(s.get_gain_coeffs()[0] != 0)
    ref = reference(s, p, "huber")
    out = s.robust_weights(kind="huber")
    check(out, s.get_weights(), ref, "huber", dtype, f"gain basis {np.dtype(dtype).name}")
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", ["stream", "shared"])
def test_three_slices_with_a_mask_on_the_middle_one(layout, dtype):
    from calamity_amd.solver import HipFitSolver

    T = 3
    parts = [synthetic.make_problem(7, 200, f0=150e6, df=400e3, seed=21, data_seed=30 + t) for t in range(T)]
    p0 = parts[0][0]
    data = tuple(np.concatenate([getattr(parts[t][0], k) for t in range(T)]) for k in ("data_r", "data_i", "wgts"))
    pars = [perturbed(parts[t][0], parts[t][2], seed=40 + t) for t in range(T)]
    sub, _, _ = batched.replicate_slices(p0, T)
    s = HipFitSolver(dtype=dtype)
    s.set_problem(sub, layout=layout)
    s.set_data(*data)
    s.set_params(*[np.concatenate([pars[t][k] for t in range(T)]) for k in ("g_r", "g_i", "c_r", "c_i")])
    assert s.nslices == 3
    nb = p0.nbls
    w_in = s.get_weights()
    ref = reference(s, sub, "huber", data=data[:2])
    out = s.robust_weights(kind="huber", slice_mask=[0, 1, 0])
    w = s.get_weights()
    mid = np.arange(nb, 2 * nb)
    check(out, w, ref, "huber", dtype, f"middle slice {layout} {np.dtype(dtype).name}", rows=mid)
    assert np.sum(out["ndown_bl"][mid]) > 0
    for rows in (slice(0, nb), slice(2 * nb, 3 * nb)):  # the unselected slices keep their bits and report nothing
        np.testing.assert_array_equal(w[rows], w_in[rows])
        assert not np.any(out["scale_bl"][rows]) and not np.any(out["ndown_bl"][rows])
    # then all slices, then the first alone put back
    out = s.robust_weights(kind="huber")
    w_all = s.get_weights()
    check(out, w_all, ref, "huber", dtype, f"all slices {layout} {np.dtype(dtype).name}")
    np.testing.assert_array_equal(w_all[mid], w[mid])
    s.robust_weights(kind="none", slice_mask=[1, 0, 0])
    w_back = s.get_weights()
    np.testing.assert_array_equal(w_back[:nb], w_in[:nb])
    np.testing.assert_array_equal(w_back[nb:], w_all[nb:])
    s.close()


@pytest.mark.parametrize("config", ["adam", "graph", "kernels"])
def test_a_run_continued_after_an_all_zero_mask_call_is_bit_identical(config):
    p, params = edge_problem(300)
    losses, final = {}, {}
    for with_call in (False, True):
        s = solver_of(p, params, np.float32)
        s.set_launch_mode({"graph": "graph", "kernels": "kernels"}.get(config, "auto"))
        s.set_optimizer("Adam", learning_rate=1e-2)
        first = s.run(20, tol=0.0)[0]
        if with_call:
            out = s.robust_weights(kind="huber", slice_mask=[0])
            assert not np.any(out["scale_bl"]) and not np.any(out["ndown_bl"])
        second = s.run(20, tol=0.0)[0]
        losses[with_call] = np.concatenate([first, second])
        final[with_call] = s.get_params()
        s.close()
    assert len(losses[True]) == 40
    np.testing.assert_array_equal(losses[True], losses[False])
    for a, b in zip(final[True], final[False]):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("mode", ["auto", "graph", "kernels"])
def test_a_recorded_loop_sees_the_new_weights(mode):
    """The pointers stay: a step graph recorded before the call runs on the rewritten plane.  A run continued after the call equals, bit
    for bit, a run continued after the same weights were uploaded with set_data."""
    p, params = edge_problem(300)
    got, w_clip = {}, None
    for how in ("call", "upload"):
        s = solver_of(p, params, np.float32)
        s.set_launch_mode(mode)
        s.set_optimizer("Adam", learning_rate=1e-2)
        first = s.run(20, tol=0.0)[0]
        if how == "call":
            s.robust_weights(kind="clip", threshold=1.0)
            w_clip = s.get_weights()
        else:
            s.set_data(p.data_r, p.data_i, w_clip)
        got[how] = np.concatenate([first, s.run(20, tol=0.0)[0]])
        s.close()
    np.testing.assert_array_equal(got["call"], got["upload"])
    assert got["call"][20] < 0.9 * got["call"][19]  # the clipped chi-square is visibly smaller


@pytest.mark.parametrize("dtype", DTYPES)
def test_clipping_finds_the_outliers_and_spares_the_clean_samples(dtype):
    """Parameters at the synthetic truth, complex Gaussian noise of variance 1 / w0, w0 uniform in [0.5, 1.5] with 10 % flagged, 5 % of
    the samples with an added outlier of 30 sigma; k = 3, clip.  For the exponential law P(z2 > 9) = e^-9 ~ 1.2e-4, so at least 99 % of
    the outliers at weight 0 and at most 1 % of the clean samples are conditions with wide margins."""
    p, truth, _ = synthetic.make_problem(8, 300, f0=150e6, df=400e3, seed=0)
    s = solver_of(p, dict(g_r=truth["g"].real, g_i=truth["g"].imag, c_r=truth["c"].real, c_i=truth["c"].imag), dtype)
    m_r, m_i = s.data_model()
    rng = np.random.default_rng(0)
    shape = (p.nbls, p.nfreqs)
    w0 = rng.uniform(0.5, 1.5, shape)
    flagged = rng.random(shape) < 0.10
    sigma = 1.0 / np.sqrt(w0)
    noise = sigma * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)
    is_out = rng.random(shape) < 0.05
    spike = np.where(is_out, 30.0 * sigma * np.exp(2j * np.pi * rng.random(shape)), 0.0)
    d = (m_r.astype(np.float64) + 1j * m_i.astype(np.float64)) + noise + spike
    s.set_data(d.real, d.imag, np.where(flagged, 0.0, w0))
    out = s.robust_weights(kind="clip", threshold=3.0)
    w = s.get_weights()
    good = ~flagged
    n_out, n_clean = int(np.sum(is_out & good)), int(np.sum(~is_out & good))
    missed = int(np.sum((w != 0) & is_out & good))
    clipped = int(np.sum((w == 0) & ~is_out & good))
    print(f"{np.dtype(dtype).name}: {missed} of {n_out} outliers missed, {clipped} of {n_clean} clean samples clipped")
    assert n_out > 300 and n_clean > 7000
    assert n_out - missed >= 0.99 * n_out
    assert clipped <= 0.01 * n_clean
    assert out["ndown_bl"].sum() == np.sum((w == 0) & good)
    s.close()


def test_wrong_state_and_bad_arguments_are_reported():
    from calamity_amd.solver import HipFitSolver

    p, params = edge_problem(37)
    shell = copy.copy(p)
    shell.data_r = shell.data_i = shell.wgts = None
    s = HipFitSolver(dtype=np.float64)
    s.set_problem(shell)
    s.set_params(params["g_r"], params["g_i"], params["c_r"], params["c_i"])
    with pytest.raises(_lib.CalamityHipError) as err:  # no data
        s.robust_weights()
    assert err.value.code == _lib.CAL_ERR_STATE
    with pytest.raises(_lib.CalamityHipError) as err:
        s.get_weights()
    assert err.value.code == _lib.CAL_ERR_STATE
    s.set_problem(shell)
    s.set_data(p.data_r, p.data_i, p.wgts)
    s.set_params(params["g_r"], params["g_i"])
    with pytest.raises(_lib.CalamityHipError) as err:  # no coefficients
        s.robust_weights()
    assert err.value.code == _lib.CAL_ERR_STATE
    s.set_problem(shell)
    s.set_data(p.data_r, p.data_i, p.wgts)
    s.set_params(c_r=params["c_r"], c_i=params["c_i"])
    with pytest.raises(_lib.CalamityHipError) as err:  # no gains
        s.robust_weights()
    assert err.value.code == _lib.CAL_ERR_STATE
    s.set_params(params["g_r"], params["g_i"])
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(_lib.CalamityHipError) as err:
            s.robust_weights(threshold=bad)
        assert err.value.code == _lib.CAL_ERR_INVALID
    d = _lib.RobustDesc(7, 3.0, None)  # an unknown kind, past the Python check
    import ctypes as C

    assert s._lib.cal_solver_robust_weights(s._h, C.byref(d), None, None) == _lib.CAL_ERR_INVALID
    with pytest.raises(_lib.CalamityHipError) as err:
        s.get_weights(2)
    assert err.value.code == _lib.CAL_ERR_INVALID
    with pytest.raises(ValueError):
        s.robust_weights(slice_mask=[1, 0])
    # both outputs may be NULL
    d = _lib.RobustDesc(_lib.ROBUST_KINDS["huber"], 3.0, None)
    assert s._lib.cal_solver_robust_weights(s._h, C.byref(d), None, None) == 0
    np.testing.assert_array_equal(s.get_weights(1), p.wgts)
    s.close()
