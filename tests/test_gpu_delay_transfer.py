"""cal_solver_delay_transfer on the device against the float64 restatement of the header text (tests/delay_transfer_ref.py), at the
smallest shapes that reach every branch of the two kernels: the problems of test_gpu_delay_spectrum.py (a partial column block, a padded
band, four column blocks; a wholly flagged row), the edge problems of test_gpu_fit_quality.py and the shape cases of
test_gpu_coeff_solve_shapes.py (the factor's LDS bound and the edge of a pass of 128 vectors, every tile width on a padded band, runs
that are interrupted, folded tiles, up to 896 vectors = seven passes).

Bounds (not tuned): ``absorbed_bl`` and ``num = absorbed_bl noise_bl`` within the project's TOL of the plane's largest element (fp32
1e-4, fp64 1e-10: what DESIGN 3.15 holds |W a|^2 to on the same cores with the same W), ``noise_bl`` within 1e-12 relative (s and v
are formed alike on both sides; the sums differ by their order), ``count_bin`` equal, the bins within nbls 2^-53 of the sequential sum
of the device's own rows.  Every case prints its largest errors.

The autocorrelation row of the spectrum's problems is a group of its own with G = |g|^2 > 0: by the definitions it is a row like any
other (it is factored, counted, and compared with the restatement like every row); the wholly flagged row is the one singular group:
zeros, in no bin."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

from calamity_amd import _lib, batched, modeling, synthetic
from delay_transfer_ref import bin_rows, restated
from test_gpu_coeff_solve import COND_MAX
from test_gpu_coeff_solve_shapes import FLAGGED, alternating_case, boundary_case, folded_1024, narrow_case, wide_case
from test_gpu_delay_spectrum import DENSE, DF, F0, GENERAL, bins_of, config_id, operator, perturbed, problem
from test_gpu_fit_quality import TOL, edge_problem, plane_err, solver_of

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
ROWS = ("absorbed_bl", "noise_bl")


def call(s, p, op, **kw):
    bins, nbins = bins_of(p)
    return s.delay_transfer(op, bin_of_bl=bins, nbins=nbins, per_baseline=True, **kw)


def reference(p, params, dtype, op, **kw):
    bins, nbins = bins_of(p)
    return restated(p, params["g_r"], params["g_i"], dtype, op, bin_of_bl=bins, nbins=nbins, **kw)


def check(out, ref, p, dtype, label, binned=True):
    tol = TOL[np.dtype(dtype)]["plane"]
    for k in ROWS:
        assert out[k].dtype == np.float64 and out[k].shape == ref[k].shape and np.all(np.isfinite(out[k])), (label, k)
    errs = dict(absorbed=plane_err(out["absorbed_bl"], ref["absorbed_bl"]), num=plane_err(out["absorbed_bl"] * out["noise_bl"], ref["num"]))
    live = ref["noise_bl"] != 0
    errs["noise"] = float(np.max(np.abs(out["noise_bl"] - ref["noise_bl"])[live] / ref["noise_bl"][live])) if live.any() else 0.0
    print(f"{label}: " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f"  absorbed in [{out['absorbed_bl'].min():.3e}, {out['absorbed_bl'].max():.9f}]")
    assert (out["nsolved"], out["nsingular"]) == (ref["nsolved"], ref["nsingular"]), (label, out["nsolved"], out["nsingular"])
    assert errs["absorbed"] <= tol and errs["num"] <= tol and errs["noise"] <= 1e-12, (label, errs)
    np.testing.assert_array_equal(out["noise_bl"] == 0, ref["noise_bl"] == 0)
    assert out["absorbed_bl"].min() >= 0.0 and out["absorbed_bl"].max() <= 1.0 + tol, label
    dead = ~ref["valid"]
    assert not np.any(out["absorbed_bl"][dead]) and not np.any(out["noise_bl"][dead]), label  # singular groups, rows without a sample: zeros
    if binned:
        bins, nbins = bins_of(p)
        np.testing.assert_array_equal(out["count_bin"], ref["count_bin"])
        own, _ = bin_rows(out["absorbed_bl"], ref["valid"], bins, nbins)
        # the bins against the sequential double sum of the device's own rows, ascending: the same additions
        assert np.max(np.abs(out["absorbed_bin"] - own)) <= p.nbls * 2.0 ** -53 * max(np.max(np.abs(own)), 1e-300), label
        assert not np.any(out["absorbed_bin"][nbins - 1]) and out["count_bin"][nbins - 1] == 0  # a bin without rows
    return errs


# ---- 1. parity at the spectrum's shapes: a partial column block, a padded band, four column blocks; raw and calibrated
@pytest.mark.parametrize("config", GENERAL, ids=config_id)
@pytest.mark.parametrize("shape,ndelays", [((7, 61), 37), ((7, 61), 61), ((7, 200), 200)])
@pytest.mark.parametrize("calibrated", [False, True], ids=["raw", "calibrated"])
def test_parity_with_the_restatement(shape, ndelays, calibrated, config):
    dtype, layout, path = config
    p, params = problem(*shape)
    assert p.nbls == 22 and p.bl_ant0[-1] == p.bl_ant1[-1] and not np.any(p.wgts[1])
    op, _ = operator(shape[1], ndelays)
    ref = reference(p, params, dtype, op, calibrated=calibrated)
    assert max(ref["conds"]) <= COND_MAX and ref["singular"] == [1]
    s = solver_of(p, params, dtype, layout, path)
    out = call(s, p, op, calibrated=calibrated)
    s.close()
    check(out, ref, p, dtype, f"{shape} {ndelays} {config_id(config)} calibrated={calibrated}")
    # the wholly flagged row is not counted; row 3 is left out (-1); the autocorrelation row is a row like any other
    assert out["count_bin"].sum() == p.nbls - 2 and np.all(out["absorbed_bl"][-1] > 0)


@pytest.mark.parametrize("config", DENSE, ids=config_id)
def test_parity_on_the_shared_dense_paths(config):
    dtype, layout, path = config
    p, params = problem(7, 200)
    op, _ = operator(200, 200)
    s = solver_of(p, params, dtype, layout, path)
    assert s.timing_get()["kernel_path"] == path
    out = call(s, p, op)
    s.close()
    check(out, reference(p, params, dtype, op), p, dtype, f"(7, 200) 200 {config_id(config)}")


@pytest.mark.parametrize("ridge", [0.0, 1e-6])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", ["stream", "shared"])
@pytest.mark.parametrize("shape", [(5, 48), (7, 200), (12, 129), (6, 300)])
def test_parity_on_the_edge_problems(shape, layout, dtype, ridge):
    p, params = edge_problem(*shape)
    op, _ = operator(shape[1], shape[1])
    ref = reference(p, params, dtype, op, ridge=ridge)
    assert max(ref["conds"]) <= COND_MAX and ref["singular"] == [0]
    s = solver_of(p, params, dtype, layout)
    out = call(s, p, op, ridge=ridge)
    s.close()
    check(out, ref, p, dtype, f"edge {shape} {layout} {np.dtype(dtype).name} ridge {ridge:g}")


# ---- 2. shapes the two kernels can go wrong at
@functools.lru_cache(maxsize=None)
def case_reference(builder, dtype, ndelays, calibrated=False):
    p, start = builder()
    op, _ = operator(p.nfreqs, ndelays)
    return p, start, op, reference(p, start, dtype, op, calibrated=calibrated)


def run_case(builder, dtype, label, ndelays, layout="shared", path="auto", folded=None, scratch=None, calibrated=False):
    p, start, op, ref = case_reference(builder, dtype, ndelays, calibrated)
    print(f"{label}: nvec {sorted({b.shape[1] for b in p.basis})}, largest cond(N) {max(ref['conds']):.2e}")
    assert max(ref["conds"]) <= COND_MAX and ref["singular"] == []
    s = solver_of(p, start, dtype, layout, path)
    if folded is not None:
        assert s.timing_get()["basis_folded"] == folded, label
    if scratch is not None:
        s._set_delay_transfer_scratch(scratch)
    out = call(s, p, op, calibrated=calibrated)
    s.close()
    check(out, ref, p, dtype, label)
    return out


def same_bits(a, b, label):
    for k in ROWS + ("absorbed_bin", "count_bin"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{label}: {k}")
    assert (a["nsolved"], a["nsingular"]) == (b["nsolved"], b["nsingular"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_both_sides_of_the_lds_bound_and_of_a_vector_pass(dtype):
    """126 and 127 vectors keep the factor in LDS, 128 is the first in scratch and the last that is one pass of the power kernel's 128
    vectors without a padded row; with a scratch bound of one byte every group is a chunk of its own: the same bits."""
    got = [run_case(boundary_case, dtype, f"boundary scratch {bound} {np.dtype(dtype).name}", 200, scratch=bound) for bound in (0, 1)]
    same_bits(got[0], got[1], "one group per chunk")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", ["stream", "shared"])
def test_both_sides_of_every_tile_width_on_a_padded_band(layout, dtype):
    run_case(narrow_case, dtype, f"narrow {layout} {np.dtype(dtype).name}", 300, layout=layout, folded=0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_runs_that_are_interrupted_and_come_back(dtype):
    """Row blocks 0 0 1 1 0 2 inside one group, a wholly flagged row inside a merged run: it has S like its neighbour and zeros out."""
    for layout in ("stream", "shared"):
        p = alternating_case()[0]
        out = run_case(alternating_case, dtype, f"alternating {layout} {np.dtype(dtype).name}", p.nfreqs, layout=layout)
        assert not np.any(out["absorbed_bl"][1 + FLAGGED]) and not np.any(out["noise_bl"][1 + FLAGGED]) and np.any(out["absorbed_bl"][FLAGGED])


@pytest.mark.parametrize("dtype", DTYPES)
def test_folded_and_full_tiles(dtype):
    got = {}
    for path, folded in (("auto", 1), ("general_full", 0)):
        got[path] = run_case(folded_1024, dtype, f"folded_1024 {path} {np.dtype(dtype).name}", 64, layout="stream", path=path, folded=folded)
    errs = {k: plane_err(got["auto"][k], got["general_full"][k]) for k in ROWS}
    print(f"folded_1024 {np.dtype(dtype).name}: folded against full " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert errs["noise_bl"] == 0.0 and errs["absorbed_bl"] <= (1e-10 if dtype == np.float64 else TOL[np.dtype(dtype)]["plane"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_wide_blocks(dtype):
    """Up to 896 vectors: seven passes of the power kernel, 14 row blocks of the basis kernel, three baselines on three row blocks per group."""
    run_case(wide_case, dtype, f"wide shared {np.dtype(dtype).name}", 64, layout="shared", folded=0)


@pytest.mark.parametrize("calibrated", [False, True], ids=["raw", "calibrated"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", ["stream", "shared"])
def test_fitting_groups_of_several_baselines(layout, dtype, calibrated):
    p, params = problem(7, 61, redundant=True)
    assert np.diff(p.grp_bl_start).max() == 3
    op, _ = operator(61, 37)
    ref = reference(p, params, dtype, op, calibrated=calibrated)
    s = solver_of(p, params, dtype, layout)
    out = call(s, p, op, calibrated=calibrated)
    s.close()
    check(out, ref, p, dtype, f"redundant group {layout} {np.dtype(dtype).name} calibrated={calibrated}")
    assert not np.array_equal(out["absorbed_bl"][0], out["absorbed_bl"][1])  # the rows of the group differ by their gains and weights


def test_slices_of_one_solver():
    """nslices = 3 with bl_alias (batched.replicate_slices): a row is a row, bin_of_bl encodes (slice, bin)."""
    from calamity_amd.solver import HipFitSolver

    T, dtype = 3, np.float64
    parts = [synthetic.make_problem(7, 61, f0=F0, df=DF, seed=21, data_seed=30 + t, flag_frac=0.05) for t in range(T)]
    p0 = parts[0][0]
    data = tuple(np.concatenate([getattr(parts[t][0], k) for t in range(T)]) for k in ("data_r", "data_i", "wgts"))
    pars = [perturbed(parts[t][0], parts[t][2], seed=40 + t) for t in range(T)]
    allp = {k: np.concatenate([pars[t][k] for t in range(T)]) for k in ("g_r", "g_i", "c_r", "c_i")}
    sub, _, _ = batched.replicate_slices(p0, T)
    assert sub.bl_alias is not None
    op, _ = operator(61, 37)
    nb = p0.nbls
    for layout in ("stream", "shared"):
        s = HipFitSolver(dtype=dtype)
        s.set_problem(sub, layout=layout)
        s.set_data(*data)
        s.set_params(allp["g_r"], allp["g_i"], allp["c_r"], allp["c_i"])
        bins = (np.repeat(np.arange(T), nb) * 2 + np.tile(np.arange(nb) % 2, T)).astype(np.int32)
        out = s.delay_transfer(op, bin_of_bl=bins, nbins=2 * T, per_baseline=True)
        s.close()
        assert (out["nsolved"], out["nsingular"]) == (T * p0.ngrps, 0)
        for t in range(T):
            ref = restated(p0, pars[t]["g_r"], pars[t]["g_i"], dtype, op, bin_of_bl=np.arange(nb) % 2, nbins=2, wgts=parts[t][0].wgts)
            rows = slice(t * nb, (t + 1) * nb)
            errs = {k: plane_err(out[k][rows], ref[k]) for k in ROWS}
            print(f"slice {t} {layout}: " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
            assert max(errs.values()) <= TOL[np.dtype(dtype)]["plane"]
            np.testing.assert_array_equal(out["count_bin"][2 * t : 2 * t + 2], ref["count_bin"])
            np.testing.assert_allclose(out["absorbed_bin"][2 * t : 2 * t + 2], ref["absorbed_bin"], rtol=0, atol=1e-10 * np.max(ref["absorbed_bin"]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_given_gains_and_the_expanded_gains_of_a_basis(dtype):
    p, params = problem(7, 61)
    op, _ = operator(61, 37)
    other = perturbed(p, dict(params), seed=11)
    s = solver_of(p, params, dtype)
    given = call(s, p, op, g_r=other["g_r"], g_i=other["g_i"])
    np.testing.assert_array_equal(s.get_params()[0], np.asarray(params["g_r"], dtype=dtype))  # the solver's own gains stay
    s.set_params(other["g_r"], other["g_i"])
    same_bits(given, call(s, p, op), "given against set gains")
    check(given, reference(p, other, dtype, op), p, dtype, f"given gains {np.dtype(dtype).name}")
    with pytest.raises(ValueError):
        s.delay_transfer(op, g_r=other["g_r"])
    s.close()
    # a frequency gain basis with y != 0: NULL gains are the expanded ones
    s = solver_of(p, params, dtype)
    s.set_gain_basis(np.array(modeling.gain_dpss_basis(F0 + DF * np.arange(p.nfreqs), 100.0)))
    s.set_optimizer("Adam", learning_rate=1e-2)
    s.run(3, tol=0.0)
    assert np.any(s.get_gain_coeffs()[0] != 0)
    g_r, g_i, c_r, c_i = s.get_params()
    out = call(s, p, op)
    s.close()
    check(out, reference(p, dict(g_r=g_r, g_i=g_i), dtype, op), p, dtype, f"gain basis {np.dtype(dtype).name}")


# ---- 3. outputs, chunks, state
@pytest.mark.parametrize("dtype", DTYPES)
def test_null_subsets_of_the_outputs_chunks_and_repeated_calls_give_the_same_bits(dtype):
    p, params = problem(7, 200)
    op, _ = operator(200, 200)
    bins, nbins = bins_of(p)
    s = solver_of(p, params, dtype)
    full = call(s, p, op)
    same_bits(full, call(s, p, op), "two calls")
    s._set_delay_transfer_scratch(1)  # one group per chunk
    same_bits(full, call(s, p, op), "a bound of one byte")
    s._set_delay_transfer_scratch(0)
    with pytest.raises(_lib.CalamityHipError) as err:
        s._set_delay_transfer_scratch(-1)
    assert err.value.code == _lib.CAL_ERR_INVALID
    only_bins = s.delay_transfer(op, bin_of_bl=bins, nbins=nbins)
    assert "absorbed_bl" not in only_bins and "noise_bl" not in only_bins
    only_rows = s.delay_transfer(op, per_baseline=True)
    assert "count_bin" not in only_rows and "absorbed_bin" not in only_rows
    np.testing.assert_array_equal(only_bins["absorbed_bin"], full["absorbed_bin"])
    np.testing.assert_array_equal(only_bins["count_bin"], full["count_bin"])
    for k in ROWS:
        np.testing.assert_array_equal(only_rows[k], full[k])
    # every single output alone, at the C boundary
    op_r, op_i = (np.ascontiguousarray(a, dtype=dtype) for a in (op.real, op.imag))
    d = _lib.DelayTransferDesc(200, 0, nbins, bins.ctypes.data, op_r.ctypes.data, op_i.ctypes.data, 1e-6)
    shapes = dict(absorbed_bl=(p.nbls, 200), noise_bl=(p.nbls, 200), absorbed_bin=(nbins, 200), count_bin=(nbins,))
    for k in shapes:
        bufs = {n: (np.full(shapes[n], np.nan) if n == k else None) for n in shapes}
        cnt = _lib.FitErrorsCounts()
        rc = s._lib.cal_solver_delay_transfer(s._h, C.byref(d), None, None, *(None if bufs[n] is None else bufs[n].ctypes.data for n in shapes),
                                              C.byref(cnt) if k == "count_bin" else None)
        assert rc == 0
        np.testing.assert_array_equal(bufs[k], full[k], err_msg=k)
    assert (cnt.nsolved, cnt.nsingular) == (full["nsolved"], full["nsingular"])
    assert s._lib.cal_solver_delay_transfer(s._h, C.byref(d), None, None, None, None, None, None, None) == 0  # nothing asked for
    s.close()


def test_the_memory_count_holds_the_new_buffers():
    p, params = problem(7, 61)
    op, _ = operator(61, 37)
    s = solver_of(p, params, np.float32)
    before = s.memory_bytes()
    call(s, p, op)
    after = s.memory_bytes()
    s.close()
    # at least the rows of absorbed and noise (doubles) and S of the 22 runs ([fe_pad(nvec)][64] floats each)
    nv = min(b.shape[1] for b in p.basis)
    assert after - before >= 2 * p.nbls * 37 * 8 + p.nbls * nv * 64 * 4, (before, after)


@pytest.mark.parametrize("config", ["adam", "graph", "kernels", "gain_basis"])
def test_a_run_continued_after_the_call_is_bit_identical(config):
    p, params = problem(7, 200)
    op, _ = operator(200, 200)
    losses, final, moments = {}, {}, {}
    for with_call in (False, True):
        s = solver_of(p, params, np.float32)
        if config == "gain_basis":
            s.set_gain_basis(np.array(modeling.gain_dpss_basis(F0 + DF * np.arange(p.nfreqs), 100.0)))
        s.set_launch_mode({"graph": "graph", "kernels": "kernels"}.get(config, "auto"))
        s.set_optimizer("Adam", learning_rate=1e-2)
        first = s.run(20, tol=0.0)[0]
        if with_call:
            out = call(s, p, op)
            assert out["absorbed_bin"].sum() > 0
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
    from calamity_amd.solver import HipFitSolver

    p, params = problem(7, 61)
    op, _ = operator(61, 37)
    shell = copy.copy(p)
    shell.data_r = shell.data_i = shell.wgts = None
    s = HipFitSolver(dtype=np.float64)
    s.set_problem(shell)
    s.set_params(params["g_r"], params["g_i"], params["c_r"], params["c_i"])
    with pytest.raises(_lib.CalamityHipError) as err:  # no data
        s.delay_transfer(op)
    assert err.value.code == _lib.CAL_ERR_STATE
    s.set_problem(shell)
    s.set_data(p.data_r, p.data_i, p.wgts)
    s.set_params(params["g_r"], params["g_i"])
    with pytest.raises(_lib.CalamityHipError) as err:  # no coefficients
        s.delay_transfer(op)
    assert err.value.code == _lib.CAL_ERR_STATE
    s.set_problem(shell)
    s.set_data(p.data_r, p.data_i, p.wgts)
    s.set_params(c_r=params["c_r"], c_i=params["c_i"])
    with pytest.raises(_lib.CalamityHipError) as err:  # gains neither set nor given
        s.delay_transfer(op)
    assert err.value.code == _lib.CAL_ERR_STATE
    assert s.delay_transfer(op, g_r=params["g_r"], g_i=params["g_i"])["nsolved"] == p.ngrps - 1  # given: enough
    # bad descriptions, at the C boundary
    s.set_params(params["g_r"], params["g_i"])
    op_r, op_i = np.ascontiguousarray(op.real), np.ascontiguousarray(op.imag)
    bins = np.zeros(p.nbls, dtype=np.int32)
    rows = np.empty((p.nbls, 37))
    binned = np.empty((2, 37))

    def code(ndelays=37, calibrated=0, nbins=0, bin_of_bl=None, op_r=op_r.ctypes.data, ridge=1e-6, absorbed_bin=None):
        d = _lib.DelayTransferDesc(ndelays, calibrated, nbins, bin_of_bl, op_r, op_i.ctypes.data, ridge)
        return s._lib.cal_solver_delay_transfer(s._h, C.byref(d), None, None, rows.ctypes.data, None, absorbed_bin, None, None)

    assert code() == 0
    assert code(ndelays=0) == _lib.CAL_ERR_INVALID and code(ndelays=4097) == _lib.CAL_ERR_INVALID
    assert code(op_r=None) == _lib.CAL_ERR_INVALID
    assert code(calibrated=2) == _lib.CAL_ERR_INVALID
    assert code(ridge=-1e-6) == _lib.CAL_ERR_INVALID and code(ridge=np.inf) == _lib.CAL_ERR_INVALID and code(ridge=np.nan) == _lib.CAL_ERR_INVALID
    assert code(ridge=0.0) == 0
    assert code(nbins=2) == _lib.CAL_ERR_INVALID  # bins without bin_of_bl
    assert code(absorbed_bin=binned.ctypes.data) == _lib.CAL_ERR_INVALID  # binned outputs without bins
    assert code(nbins=2, bin_of_bl=bins.ctypes.data, absorbed_bin=binned.ctypes.data) == 0
    bins[5] = 2
    assert code(nbins=2, bin_of_bl=bins.ctypes.data) == _lib.CAL_ERR_INVALID  # an index out of range
    bins[5] = -2
    assert code(nbins=2, bin_of_bl=bins.ctypes.data) == _lib.CAL_ERR_INVALID
    d = _lib.DelayTransferDesc(37, 0, 0, None, op_r.ctypes.data, op_i.ctypes.data, 1e-6)
    assert s._lib.cal_solver_delay_transfer(s._h, C.byref(d), params["g_r"].ctypes.data, None, None, None, None, None, None) == _lib.CAL_ERR_INVALID
    assert s._lib.cal_solver_delay_transfer(s._h, None, None, None, None, None, None, None, None) == _lib.CAL_ERR_INVALID
    s.close()
