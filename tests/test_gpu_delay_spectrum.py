"""cal_solver_delay_spectrum on the device against the float64 restatement of the header text (tests/delay_spectrum_ref.py), at the
smallest shapes that reach every branch: make_problem(7, 61) (fpad 64: a ragged tail of the operator's depth; 21 + 1 rows) with 37
delays (a partial column block) and 61; make_problem(7, 200) with 200 delays (several staged pieces of the operator and four column
blocks).  One row is flagged wholly by hand, one is an autocorrelation.

The bound is derived, not tuned (delay_spectrum_ref.py): tau = 8 u (nfreqs + 16) sum_f mask (|d| + |G| |m|) |op|, and the power must
satisfy |P - P_ref| norm_b <= (2 |X_ref| + tau) tau.  Every case prints its largest ratio of error to bound."""
import functools

import numpy as np
import pytest

from calamity_amd import _lib, batched, modeling, synthetic
from calamity_amd.problem import FitProblem
from delay_spectrum_ref import NAMES, bin_rows, bound_ratio, model_of, restated

pytestmark = pytest.mark.gpu

F0, DF = 150e6, 400e3


def perturbed(p, start, seed):
    rng = np.random.default_rng(seed)
    gs = (p.nants, p.nfreqs)
    return dict(g_r=start["g_r"] + 0.1 * rng.standard_normal(gs), g_i=start["g_i"] + 0.1 * rng.standard_normal(gs),
                c_r=start["c_r"] * (1.0 + 0.1 * rng.standard_normal(p.ncoeffs)), c_i=start["c_i"] * (1.0 + 0.1 * rng.standard_normal(p.ncoeffs)))


def with_auto_and_flagged_row(p0, start0, seed):
    """``p0`` plus an autocorrelation row of antenna 2 (a group of its own on basis 0); row 1 flagged wholly."""
    rng = np.random.default_rng(seed)
    nv = p0.basis[p0.grp_basis[0]].shape[1]
    ngrp_bl = np.diff(p0.grp_bl_start)
    w = np.concatenate([p0.wgts, np.full((1, p0.nfreqs), p0.wgts.max())])
    w[1, :] = 0.0
    p = FitProblem(nants=p0.nants, nfreqs=p0.nfreqs, basis=p0.basis, grp_basis=np.concatenate([p0.grp_basis, [p0.grp_basis[0]]]).astype(np.int32),
                   grp_bl_start=np.concatenate([[0], np.cumsum(np.concatenate([ngrp_bl, [1]]))]).astype(np.int32),
                   bl_ant0=np.concatenate([p0.bl_ant0, [2]]).astype(np.int32), bl_ant1=np.concatenate([p0.bl_ant1, [2]]).astype(np.int32),
                   bl_rowblk=np.concatenate([p0.bl_rowblk, [0]]).astype(np.int32),
                   data_r=np.concatenate([p0.data_r, rng.standard_normal((1, p0.nfreqs))]),
                   data_i=np.concatenate([p0.data_i, rng.standard_normal((1, p0.nfreqs))]), wgts=w)
    p.validate()
    start = dict(start0, c_r=np.concatenate([start0["c_r"], rng.standard_normal(nv)]), c_i=np.concatenate([start0["c_i"], rng.standard_normal(nv)]))
    return p, start


@functools.lru_cache(maxsize=None)
def problem(nants, nfreqs, redundant=False):
    p0, _, start0 = synthetic.make_problem(nants, nfreqs, f0=F0, df=DF, seed=nants + nfreqs, flag_frac=0.05)
    if redundant:
        p0, start0 = synthetic.add_redundant_group(p0, start0, np.random.default_rng(1), nred=3)
        assert np.diff(p0.grp_bl_start).max() == 3
    p, start = with_auto_and_flagged_row(p0, start0, seed=3)
    assert np.any(p.wgts[2:-1] == 0)  # flags from flag_frac
    return p, perturbed(p, start, seed=5)


@functools.lru_cache(maxsize=None)
def operator(nfreqs, ndelays):
    op, norm_f, delays = modeling.delay_transform(F0 + DF * np.arange(nfreqs))
    lo = (nfreqs - ndelays) // 2
    return np.ascontiguousarray(op[:, lo : lo + ndelays]), norm_f


def bins_of(p, nbins=4):
    """Rows dealt over the bins 0 .. nbins - 2 (bin nbins - 1 stays empty); row 3 is left out (-1)."""
    b = (np.arange(p.nbls) % (nbins - 1)).astype(np.int32)
    b[3] = -1
    return b, nbins


def solver_of(p, params, dtype, layout="shared", kernel_path="auto"):
    from calamity_amd.solver import HipFitSolver

    s = HipFitSolver(dtype=dtype)
    s.set_problem(p, layout=layout, kernel_path=kernel_path)
    s.set_params(params["g_r"], params["g_i"], params["c_r"], params["c_i"])
    return s


def reference(p, params, dtype, op, norm_f, calibrated=False, data=None):
    cast = lambda a: np.asarray(a).astype(dtype).astype(np.float64)  # noqa: E731
    d_r, d_i, w = (cast(a) for a in (data if data is not None else (p.data_r, p.data_i, p.wgts)))
    g = cast(params["g_r"]) + 1j * cast(params["g_i"])
    G = g[p.bl_ant0] * np.conj(g[p.bl_ant1])
    op_t = cast(op.real) + 1j * cast(op.imag)
    bins, nbins = bins_of(p)
    return restated(d_r + 1j * d_i, model_of(p, params["c_r"], params["c_i"], dtype), G, w, op_t, norm_f, calibrated, bins, nbins)


def check(out, ref, p, dtype, label, names=NAMES):
    worst = {}
    for k in names:
        P = out["per_baseline"][k]
        assert P.dtype == np.float64 and P.shape == ref["per_baseline"][k].shape and np.all(np.isfinite(P)), (label, k)
        worst[k] = bound_ratio(P, ref, k, dtype)
    print(f"{label}: error / bound  " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, (label, worst)
    np.testing.assert_allclose(out["norm_bl"], ref["norm_bl"], rtol=1e-13, atol=0)
    # the wholly flagged row: no power, in no bin
    assert out["norm_bl"][1] == 0
    for k in names:
        assert not np.any(out["per_baseline"][k][1])
    if "count_bin" in out:
        bins, nbins = bins_of(p)
        np.testing.assert_array_equal(out["count_bin"], ref["count_bin"])
        own = bin_rows({k: out["per_baseline"][k] for k in names}, out["norm_bl"], bins, nbins)
        for k in names:
            # the bins against the sequential double sum of the device's own rows, ascending: the same additions
            scale = np.max(np.abs(own[k]))
            assert np.max(np.abs(out[k] - own[k])) <= p.nbls * 2.0 ** -53 * scale, (label, k)
            assert not np.any(out[k][nbins - 1]) and out["count_bin"][nbins - 1] == 0  # a bin without rows
        assert out["count_bin"].sum() == p.nbls - 2  # row 3 is left out (-1), row 1 is flagged
    return worst


def call(s, p, op, norm_f, **kw):
    bins, nbins = bins_of(p)
    return s.delay_spectrum(op, norm_f, bin_of_bl=bins, nbins=nbins, per_baseline=True, **kw)


GENERAL = [(np.float32, "stream", "auto"), (np.float32, "shared", "general"), (np.float64, "stream", "auto"), (np.float64, "shared", "general")]
DENSE = [(np.float32, "shared", "dense"), (np.float32, "shared", "dense_split1"), (np.float32, "shared", "dense_f32"), (np.float64, "shared", "dense")]


def config_id(c):
    return f"{np.dtype(c[0]).name}-{c[1]}-{c[2]}"


@pytest.mark.parametrize("config", GENERAL, ids=config_id)
@pytest.mark.parametrize("shape,ndelays", [((7, 61), 37), ((7, 61), 61), ((7, 200), 200)])
@pytest.mark.parametrize("calibrated", [False, True], ids=["raw", "calibrated"])
def test_parity_with_the_restatement(shape, ndelays, calibrated, config):
    dtype, layout, path = config
    p, params = problem(*shape)
    assert p.nbls == 22 and p.bl_ant0[-1] == p.bl_ant1[-1]
    op, norm_f = operator(shape[1], ndelays)
    s = solver_of(p, params, dtype, layout, path)
    out = call(s, p, op, norm_f, calibrated=calibrated)
    check(out, reference(p, params, dtype, op, norm_f, calibrated), p, dtype, f"{shape} {ndelays} {config_id(config)} calibrated={calibrated}")
    s.close()


@pytest.mark.parametrize("config", DENSE, ids=config_id)
def test_parity_on_the_shared_dense_paths(config):
    dtype, layout, path = config
    p, params = problem(7, 200)
    op, norm_f = operator(200, 200)
    s = solver_of(p, params, dtype, layout, path)
    assert s.timing_get()["kernel_path"] == path
    out = call(s, p, op, norm_f)
    check(out, reference(p, params, dtype, op, norm_f), p, dtype, f"(7, 200) 200 {config_id(config)}")
    s.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("layout", ["stream", "shared"])
def test_fitting_groups_of_several_baselines(layout, dtype):
    p, params = problem(7, 61, redundant=True)
    op, norm_f = operator(61, 37)
    s = solver_of(p, params, dtype, layout)
    check(call(s, p, op, norm_f), reference(p, params, dtype, op, norm_f), p, dtype, f"redundant group {layout} {np.dtype(dtype).name}")
    s.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_each_quantity_alone_equals_its_plane_of_all_three(dtype):
    p, params = problem(7, 61)
    op, norm_f = operator(61, 37)
    s = solver_of(p, params, dtype)
    full = call(s, p, op, norm_f)
    for what in (("data",), ("model",), ("resid",), ("resid", "data")):
        one = call(s, p, op, norm_f, what=what)
        assert set(one["per_baseline"]) == set(what)
        for k in what:
            np.testing.assert_array_equal(one["per_baseline"][k], full["per_baseline"][k], err_msg=str(what))
            np.testing.assert_array_equal(one[k], full[k], err_msg=str(what))
        np.testing.assert_array_equal(one["count_bin"], full["count_bin"])
    # binned only (the normal call), per baseline only, neither
    bins, nbins = bins_of(p)
    only_bins = s.delay_spectrum(op, norm_f, bin_of_bl=bins, nbins=nbins)
    assert "per_baseline" not in only_bins
    only_rows = s.delay_spectrum(op, norm_f, per_baseline=True)
    assert "count_bin" not in only_rows and "data" not in only_rows
    neither = s.delay_spectrum(op, norm_f)
    for k in NAMES:
        np.testing.assert_array_equal(only_bins[k], full[k])
        np.testing.assert_array_equal(only_rows["per_baseline"][k], full["per_baseline"][k])
    np.testing.assert_array_equal(neither["norm_bl"], full["norm_bl"])
    s.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape,ndelays", [((7, 61), 37), ((7, 200), 200)])
def test_chunks_and_repeated_calls_give_the_same_bits(shape, ndelays, dtype):
    p, params = problem(*shape)
    op, norm_f = operator(shape[1], ndelays)
    s = solver_of(p, params, dtype)
    one = call(s, p, op, norm_f)
    again = call(s, p, op, norm_f)
    fpad = -(-shape[1] // 32) * 32  # at least the row pitch of the masked planes
    per_row = 3 * 2 * fpad * np.dtype(dtype).itemsize + 3 * ndelays * 8
    for rows in (7, 1):
        s._set_delay_spectrum_scratch(rows * per_row + per_row // 2)  # 22 rows: four chunks of seven at the most, then one row each
        cut = call(s, p, op, norm_f)
        for a, b in ((one, again), (one, cut)):
            np.testing.assert_array_equal(a["norm_bl"], b["norm_bl"])
            np.testing.assert_array_equal(a["count_bin"], b["count_bin"])
            for k in NAMES:
                np.testing.assert_array_equal(a[k], b[k], err_msg=f"{rows} rows per chunk, bins of {k}")
                np.testing.assert_array_equal(a["per_baseline"][k], b["per_baseline"][k], err_msg=f"{rows} rows per chunk, {k}")
    s._set_delay_spectrum_scratch(0)
    with pytest.raises(_lib.CalamityHipError) as err:
        s._set_delay_spectrum_scratch(-1)
    assert err.value.code == _lib.CAL_ERR_INVALID
    s.close()


def test_slices_of_one_solver():
    """nslices = 3 with bl_alias (batched.replicate_slices): a row is a row, bin_of_bl encodes (slice, bin)."""
    from calamity_amd.solver import HipFitSolver

    T, dtype = 3, np.float64
    parts = [synthetic.make_problem(7, 61, f0=F0, df=DF, seed=21, data_seed=30 + t) for t in range(T)]
    p0 = parts[0][0]
    data = tuple(np.concatenate([getattr(parts[t][0], k) for t in range(T)]) for k in ("data_r", "data_i", "wgts"))
    pars = [perturbed(parts[t][0], parts[t][2], seed=40 + t) for t in range(T)]
    allp = {k: np.concatenate([pars[t][k] for t in range(T)]) for k in ("g_r", "g_i", "c_r", "c_i")}
    sub, _, _ = batched.replicate_slices(p0, T)
    assert sub.bl_alias is not None
    op, norm_f = operator(61, 37)
    for layout in ("stream", "shared"):
        s = HipFitSolver(dtype=dtype)
        s.set_problem(sub, layout=layout)
        s.set_data(*data)
        s.set_params(allp["g_r"], allp["g_i"], allp["c_r"], allp["c_i"])
        nb = p0.nbls
        bins = (np.repeat(np.arange(T), nb) * 2 + np.tile(np.arange(nb) % 2, T)).astype(np.int32)
        out = s.delay_spectrum(op, norm_f, bin_of_bl=bins, nbins=2 * T, per_baseline=True)
        for t in range(T):
            g = pars[t]["g_r"] + 1j * pars[t]["g_i"]
            G = g[p0.bl_ant0] * np.conj(g[p0.bl_ant1])
            pt = parts[t][0]
            ref = restated(pt.data_r + 1j * pt.data_i, model_of(p0, pars[t]["c_r"], pars[t]["c_i"], dtype), G, pt.wgts, op, norm_f,
                           bin_of_bl=np.arange(nb) % 2, nbins=2)
            rows = slice(t * nb, (t + 1) * nb)
            worst = max(bound_ratio(out["per_baseline"][k][rows], ref, k, dtype) for k in NAMES)
            print(f"slice {t} {layout}: error / bound {worst:.3f}")
            assert worst <= 1.0
            np.testing.assert_array_equal(out["count_bin"][2 * t : 2 * t + 2], ref["count_bin"])
            for k in NAMES:
                np.testing.assert_allclose(out[k][2 * t : 2 * t + 2], ref[k], rtol=0, atol=1e-10 * np.max(ref[k]))
        s.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_given_gains_and_the_expanded_gains_of_a_basis(dtype):
    p, params = problem(7, 61)
    op, norm_f = operator(61, 37)
    other = perturbed(p, dict(params), seed=11)
    s = solver_of(p, params, dtype)
    given = call(s, p, op, norm_f, g_r=other["g_r"], g_i=other["g_i"])
    np.testing.assert_array_equal(s.get_params()[0], np.asarray(params["g_r"], dtype=dtype))  # the solver's own gains stay
    s.set_params(other["g_r"], other["g_i"])
    as_set = call(s, p, op, norm_f)
    for k in NAMES:
        np.testing.assert_array_equal(given["per_baseline"][k], as_set["per_baseline"][k], err_msg=k)
        np.testing.assert_array_equal(given[k], as_set[k], err_msg=k)
    with pytest.raises(ValueError):
        s.delay_spectrum(op, norm_f, g_r=other["g_r"])
    s.close()
    # a frequency gain basis with y != 0: NULL gains are the expanded ones
    s = solver_of(p, params, dtype)
    s.set_gain_basis(np.array(modeling.gain_dpss_basis(F0 + DF * np.arange(p.nfreqs), 100.0)))
    s.set_optimizer("Adam", learning_rate=1e-2)
    s.run(3, tol=0.0)
    assert np.any(s.get_gain_coeffs()[0] != 0)
    g_r, g_i, c_r, c_i = s.get_params()
    out = call(s, p, op, norm_f)
    now = dict(g_r=g_r, g_i=g_i, c_r=c_r, c_i=c_i)
    check(out, reference(p, now, dtype, op, norm_f), p, dtype, f"gain basis {np.dtype(dtype).name}")
    s.close()


@pytest.mark.parametrize("config", ["adam", "graph", "kernels", "gain_basis"])
def test_a_run_continued_after_the_call_is_bit_identical(config):
    p, params = problem(7, 200)
    op, norm_f = operator(200, 200)
    losses, final, moments = {}, {}, {}
    for with_call in (False, True):
        s = solver_of(p, params, np.float32)
        if config == "gain_basis":
            s.set_gain_basis(np.array(modeling.gain_dpss_basis(F0 + DF * np.arange(p.nfreqs), 100.0)))
        s.set_launch_mode({"graph": "graph", "kernels": "kernels"}.get(config, "auto"))
        s.set_optimizer("Adam", learning_rate=1e-2)
        first = s.run(20, tol=0.0)[0]
        if with_call:
            out = call(s, p, op, norm_f)
            assert out["resid"].sum() > 0
        second = s.run(20, tol=0.0)[0]
        losses[with_call] = np.concatenate([first, second])
        final[with_call] = s.get_params()
        moments[with_call] = s.get_gain_coeff_moments() if config == "gain_basis" else s.get_moments()
        s.close()
    assert len(losses[True]) == 40
    np.testing.assert_array_equal(losses[True], losses[False])
    for a, b in zip(final[True], final[False]):
        np.testing.assert_array_equal(a, b)
    ma, mb = moments[True], moments[False]
    for a, b in zip(ma.values() if isinstance(ma, dict) else ma, mb.values() if isinstance(mb, dict) else mb):
        np.testing.assert_array_equal(a, b)


def test_errors_are_reported():
    import copy
    import ctypes as C

    from calamity_amd.solver import HipFitSolver

    p, params = problem(7, 61)
    op, norm_f = operator(61, 37)
    shell = copy.copy(p)
    shell.data_r = shell.data_i = shell.wgts = None
    s = HipFitSolver(dtype=np.float64)
    s.set_problem(shell)
    s.set_params(params["g_r"], params["g_i"], params["c_r"], params["c_i"])
    with pytest.raises(_lib.CalamityHipError) as err:  # no data
        s.delay_spectrum(op, norm_f)
    assert err.value.code == _lib.CAL_ERR_STATE
    s.set_problem(shell)
    s.set_data(p.data_r, p.data_i, p.wgts)
    s.set_params(params["g_r"], params["g_i"])
    with pytest.raises(_lib.CalamityHipError) as err:  # no coefficients
        s.delay_spectrum(op, norm_f)
    assert err.value.code == _lib.CAL_ERR_STATE
    s.set_problem(shell)
    s.set_data(p.data_r, p.data_i, p.wgts)
    s.set_params(c_r=params["c_r"], c_i=params["c_i"])
    with pytest.raises(_lib.CalamityHipError) as err:  # gains neither set nor given
        s.delay_spectrum(op, norm_f)
    assert err.value.code == _lib.CAL_ERR_STATE
    assert np.all(s.delay_spectrum(op, norm_f, g_r=params["g_r"], g_i=params["g_i"])["norm_bl"][[0, 2]] > 0)  # given: enough
    # bad descriptions, at the C boundary
    s.set_params(params["g_r"], params["g_i"])
    op_r, op_i = np.ascontiguousarray(op.real), np.ascontiguousarray(op.imag)
    bins = np.zeros(p.nbls, dtype=np.int32)
    norm = np.empty(p.nbls)

    def code(ndelays=37, what=7, calibrated=0, nbins=0, bin_of_bl=None, op_r=op_r.ctypes.data, norm_f=norm_f.ctypes.data):
        d = _lib.DelaySpectrumDesc(ndelays, what, calibrated, nbins, bin_of_bl, op_r, op_i.ctypes.data, norm_f)
        return s._lib.cal_solver_delay_spectrum(s._h, C.byref(d), None, None, None, norm.ctypes.data, None, None)

    assert code() == 0
    assert code(what=0) == _lib.CAL_ERR_INVALID and code(what=8) == _lib.CAL_ERR_INVALID
    assert code(ndelays=0) == _lib.CAL_ERR_INVALID and code(ndelays=4097) == _lib.CAL_ERR_INVALID
    assert code(op_r=None) == _lib.CAL_ERR_INVALID and code(norm_f=None) == _lib.CAL_ERR_INVALID
    assert code(calibrated=2) == _lib.CAL_ERR_INVALID
    assert code(nbins=2) == _lib.CAL_ERR_INVALID  # bins without bin_of_bl
    assert code(nbins=2, bin_of_bl=bins.ctypes.data) == 0
    bins[5] = 2
    assert code(nbins=2, bin_of_bl=bins.ctypes.data) == _lib.CAL_ERR_INVALID  # an index out of range
    bins[5] = -2
    assert code(nbins=2, bin_of_bl=bins.ctypes.data) == _lib.CAL_ERR_INVALID
    assert s._lib.cal_solver_delay_spectrum(s._h, None, None, None, None, None, None, None) == _lib.CAL_ERR_INVALID
    s.close()
