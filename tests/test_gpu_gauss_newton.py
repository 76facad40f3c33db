"""cal_solver_normal_product and cal_solver_gauss_newton_step on the device against the NumPy restatement tests/gauss_newton_ref.py
(include/calamity_hip.h):

    (J p)[b][f] = (dg_i conj(g_j) + g_i conj(dg_j)) m + G (A dc)
    N p = J^H W J p,   rhs = J^H W (d - G m),   (N + lambda D) p = rhs by conjugate gradients preconditioned with D from p = 0

The restatement works in fp64 on the inputs the solver holds (cast to its dtype first).  Tolerances are the project's own.  The product
is a gradient: norm-wise per plane fp64 1e-10, fp32 1e-4 (tests/test_gpu_parity.py).  A step is a short
trajectory: parameters norm-wise fp64 1e-8, fp32 1e-3; losses fp64 1e-10, fp32 1e-5 (tests/test_gpu_fit_quality.py)."""
import copy
import functools

import numpy as np
import pytest

import _slice_cases
from calamity_amd import _lib, batched, modeling, synthetic
from gauss_newton_ref import Ref
from test_gpu_fit_quality import perturbed, solver_of
from test_gpu_fold import mirror_block, small_problem

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
TOL = {np.dtype(np.float64): dict(product=1e-10, params=1e-8, loss=1e-10), np.dtype(np.float32): dict(product=1e-4, params=1e-3, loss=1e-5)}
PRIORS = (1.5, -0.5)  # of the "sum" regulariser
KEYS = ("g_r", "g_i", "c_r", "c_i")


def relnorm(got, want):
    return float(np.linalg.norm(np.asarray(got, dtype=np.float64) - want) / max(np.linalg.norm(want), 1e-300))


def cplx(a_r, a_i):
    return np.asarray(a_r, dtype=np.float64) + 1j * np.asarray(a_i, dtype=np.float64)


def cast_params(params, dtype):
    """(g, c) complex128 as a solver of ``dtype`` holds them."""
    f = lambda a: np.asarray(a).astype(dtype).astype(np.float64)  # noqa: E731
    return f(params["g_r"]) + 1j * f(params["g_i"]), f(params["c_r"]) + 1j * f(params["c_i"])


def direction(p, params, dtype, seed, size=1.0):
    """A random direction of the parameters' own size times ``size``, rounded to ``dtype`` (what the call is handed)."""
    rng = np.random.default_rng(seed)
    gs = (p.nants, p.nfreqs)
    cs = np.sqrt(np.mean(np.asarray(params["c_r"]) ** 2 + np.asarray(params["c_i"]) ** 2))
    return [(size * a).astype(dtype) for a in (0.3 * rng.standard_normal(gs), 0.3 * rng.standard_normal(gs), cs * rng.standard_normal(p.ncoeffs),
                                              cs * rng.standard_normal(p.ncoeffs))]


def slice_refs(p, params, dtype, parts=None):
    """[(Ref, g, c, gain rows, coefficient indices)] per slice: one for a single fit; for a batch the slices' own problems."""
    g, c = cast_params(params, dtype)
    if parts is None:
        return [(Ref(p, dtype=dtype), g, c, slice(0, p.nants), slice(0, p.ncoeffs))]
    out = []
    for t, q in enumerate(parts):
        rows, idx = slice(t * q.nants, (t + 1) * q.nants), slice(t * q.ncoeffs, (t + 1) * q.ncoeffs)
        out.append((Ref(q, dtype=dtype), g[rows], c[idx], rows, idx))
    return out


def check_product(s, refs, p, params, dtype, label, seed=3):
    """Parity of the product for a random direction and for the same direction times 1e-6 (the scaling test), regulariser off and on;
    afterwards the loss, the weights and the data model have the bits they had."""
    tol = TOL[np.dtype(dtype)]["product"]
    worst = 0.0
    for reg in (False, True):
        s.set_regularization("sum" if reg else None, *((PRIORS if s.nslices == 1 else (np.full(s.nslices, PRIORS[0]), np.full(s.nslices, PRIORS[1]))) if reg else (0.0, 0.0)))
        loss0, w0, dm0 = s.eval_loss(), s.get_weights(0), s.data_model()
        for size in (1.0, 1e-6):
            d = direction(p, params, dtype, seed, size)
            got = s.normal_product(*d)
            dg, dc = cplx(d[0], d[1]), cplx(d[2], d[3])
            want_g, want_c = np.empty_like(dg), np.empty_like(dc)
            for ref, g, c, rows, idx in refs:
                want_g[rows], want_c[idx] = ref.normal_product(g, c, dg[rows], dc[idx])
            errs = [relnorm(got[0], want_g.real), relnorm(got[1], want_g.imag), relnorm(got[2], want_c.real), relnorm(got[3], want_c.imag)]
            print(f"{label} reg={'sum' if reg else 'none'} size={size:g}: " + "  ".join(f"{k} {e:.2e}" for k, e in zip(KEYS, errs)))
            assert all(np.all(np.isfinite(a)) for a in got), label
            assert max(errs) <= tol, (label, reg, size, errs)
            worst = max(worst, max(errs))
        assert s.eval_loss() == loss0, label
        np.testing.assert_array_equal(s.get_weights(0), w0)
        for a, b in zip(s.data_model(), dm0):
            np.testing.assert_array_equal(a, b)
    s.set_regularization(None)
    return worst


@functools.lru_cache(maxsize=None)
def base_problem(nants, nfreqs, seed=0):
    p, _, start = synthetic.make_problem(nants, nfreqs, f0=150e6, df=400e3, seed=seed)
    return p, perturbed(p, start, seed=seed + 1)


def assert_path(s, path):
    got = s.timing_get()["kernel_path"]
    assert got == path, f"asked for the {path} kernels, the solver runs {got}"


# ---- the product
CONFIGS = [("stream", "auto", None), ("shared", "general", "general"), ("shared", "dense", "dense"), ("shared", "dense_f32", "dense_f32"),
           ("shared", "dense_split1", "dense_split1")]


PATH_CASES = [(shape, config, dtype) for shape in [(7, 200), (6, 300)] for config in CONFIGS for dtype in DTYPES
              if dtype == np.float32 or config[1] not in ("dense_f32", "dense_split1")]  # (those two kernel paths are fp32 only)


@pytest.mark.parametrize("shape,config,dtype", PATH_CASES, ids=[f"{s[0]}x{s[1]}-{c[0]}-{c[1]}-{np.dtype(d).name}" for s, c, d in PATH_CASES])
def test_product_parity_on_every_kernel_path(shape, config, dtype):
    """(6, 300): rows padded from 300 to 384 channels."""
    layout, path, runs = config
    p, params = base_problem(*shape)
    s = solver_of(p, params, dtype, layout, path)
    if runs:
        assert_path(s, runs)
    check_product(s, slice_refs(p, params, dtype), p, params, dtype, f"{shape} {layout}/{path} {np.dtype(dtype).name}")
    s.close()


@functools.lru_cache(maxsize=None)
def folded_problem():
    rng = np.random.default_rng(10)
    blocks = [mirror_block(rng, 1024, n) for n in (40, 100, 200)]
    return small_problem(blocks, [0, 1, 2] * 3, seed=11)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("path", ["auto", "general_full"])
def test_product_parity_on_folded_and_full_tiles(path, dtype):
    p, params = folded_problem()
    s = solver_of(p, params, dtype, "stream", path)
    assert s.timing_get()["basis_folded"] == (1 if path == "auto" else 0)
    check_product(s, slice_refs(p, params, dtype), p, params, dtype, f"1024 channels stream/{path} {np.dtype(dtype).name}")
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", ["stream", "shared"])
def test_product_parity_on_a_fitting_group_of_several_baselines(layout, dtype):
    p0, _, start0 = synthetic.make_problem(7, 200, f0=150e6, df=400e3, seed=13)
    p, start = synthetic.add_redundant_group(p0, start0, np.random.default_rng(1), nred=3)
    assert np.diff(p.grp_bl_start).max() == 3
    params = perturbed(p, start, seed=14)
    s = solver_of(p, params, dtype, layout)
    check_product(s, slice_refs(p, params, dtype), p, params, dtype, f"redundant group {layout} {np.dtype(dtype).name}")
    s.close()


def alias_batch(dtype, nt=3):
    """Three slices on shared tiles (bl_alias) from tests/_slice_cases.py: (batch problem, data, params, the slices' own problems)."""
    case = _slice_cases.build("uniform", dtype, nt=nt)
    sub, _, _ = batched.replicate_slices(case["prob"], nt)
    assert sub.bl_alias is not None and sub.nslices == nt
    return sub, tuple(case[k] for k in ("data_r", "data_i", "wgts")), {k: case[k] for k in KEYS}, [q for q, _ in case["parts"]]


def batch_solver(sub, data, params, dtype, layout="stream"):
    from calamity_amd.solver import HipFitSolver

    s = HipFitSolver(dtype=dtype)
    s.set_problem(sub, layout=layout)
    s.set_data(*data)
    s.set_params(*[params[k] for k in KEYS])
    return s


@pytest.mark.parametrize("dtype", DTYPES)
def test_product_parity_on_three_slices_that_share_tiles(dtype):
    sub, data, params, parts = alias_batch(dtype)
    s = batch_solver(sub, data, params, dtype)
    check_product(s, slice_refs(sub, params, dtype, parts), sub, params, dtype, f"three slices, bl_alias {np.dtype(dtype).name}")
    s.close()


# ---- one step
@functools.lru_cache(maxsize=None)
def start_problem(seed=207, **kw):
    p, _, start = synthetic.make_problem(7, 200, seed=seed, **kw)
    return p, start


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("reg", [False, True], ids=["none", "sum"])
@pytest.mark.parametrize("config", CONFIGS[:3], ids=[f"{c[0]}-{c[1]}" for c in CONFIGS[:3]])
def test_step_parity_with_five_iterations(config, reg, dtype):
    """ncg = 5, lambda = 1e-3 from unity gains and c0: the short-trajectory contract."""
    layout, path, runs = config
    p, start = start_problem()
    tol = TOL[np.dtype(dtype)]
    s = solver_of(p, start, dtype, layout, path)
    if runs:
        assert_path(s, runs)
    if reg:
        s.set_regularization("sum", *PRIORS)
    out = s.gauss_newton_step(ncg=5, lam=1e-3, cg_tol=0.0)
    g, c = cast_params(start, dtype)
    want = Ref(p, dtype=dtype).step(g, c, lam=1e-3, ncg=5, cg_tol=0.0, priors=PRIORS if reg else None)
    got = s.get_params()
    errs = [relnorm(got[0], want["g"].real), relnorm(got[1], want["g"].imag), relnorm(got[2], want["c"].real), relnorm(got[3], want["c"].imag)]
    lerr = [abs(out[k][0] - want[k]) / want[k] for k in ("loss_before", "loss_after")]
    print(f"{layout}/{path} reg={reg} {np.dtype(dtype).name}: " + "  ".join(f"{k} {e:.2e}" for k, e in zip(KEYS, errs))
          + f"  loss_before {lerr[0]:.2e}  loss_after {lerr[1]:.2e}  ({out['loss_before'][0]:.4e} -> {out['loss_after'][0]:.4e}, "
          f"residual {out['cg_residual'][0]:.3e} against {want['cg_residual']:.3e})")
    assert want["accepted"] and out["accepted"][0] and out["cg_iters"][0] == want["cg_iters"] == 5
    assert max(errs) <= tol["params"], errs
    assert max(lerr) <= tol["loss"], lerr
    assert s.eval_loss() == out["loss_after"][0]
    s.close()


# ---- convergence
@pytest.mark.parametrize("dtype", DTYPES)
def test_two_steps_converge_below_six_rounds_of_alternating_least_squares(dtype):
    """make_problem(7, 200, seed=207): the restatement leaves 5.6e-5 of the starting chi-square after two steps (2.4e-6 against 4.2e-2);
    six rounds of (solve_coeffs, five half-damped sweeps) reach about 3e-5."""
    p, start = start_problem()
    s = solver_of(p, start, dtype)
    l0 = s.eval_loss()
    outs = [s.gauss_newton_step(ncg=20, lam=lam) for lam in (1e-3, 1e-4)]
    l2 = s.eval_loss()
    als = solver_of(p, start, dtype)
    for _ in range(6):
        als.solve_coeffs()
        als.solve_gains(5, damping=0.5)
    l_als = als.eval_loss()
    print(f"{np.dtype(dtype).name}: chi-square {l0:.3e} -> {outs[0]['loss_after'][0]:.3e} -> {l2:.3e} (ratio {l2 / l0:.2e}); six ALS rounds {l_als:.3e}")
    assert all(o["accepted"][0] for o in outs) and outs[1]["loss_after"][0] == l2
    assert l2 <= 1e-3 * l0
    assert l2 < l_als
    s.close()
    als.close()


# ---- rejection
@pytest.mark.parametrize("dtype", DTYPES)
def test_an_undamped_step_from_far_away_is_rejected_and_changes_no_bit(dtype):
    """gain_sigma = 1, lambda = 0: the restatement's trial has 2.39 against 0.786 before."""
    p, start = start_problem(gain_sigma=1.0)
    s = solver_of(p, start, dtype)
    s.set_optimizer("Adam", learning_rate=1e-2)
    before, mom = s.get_params(), s.get_moments()
    out = s.gauss_newton_step(ncg=20, lam=0.0, reset_moments=True)
    print(f"{np.dtype(dtype).name}: trial {out['loss_after'][0]:.3f} against {out['loss_before'][0]:.3f}")
    assert not out["accepted"][0] and out["loss_after"][0] > out["loss_before"][0]
    for a, b in zip(s.get_params(), before):
        np.testing.assert_array_equal(a, b)
    after = s.get_moments()
    for k in mom:
        np.testing.assert_array_equal(after[k], mom[k], err_msg=k)
    assert s.eval_loss() == out["loss_before"][0]
    s.close()


# ---- masks
def three_slices(dtype, layout):
    T = 3
    parts = [synthetic.make_problem(7, 200, f0=150e6, df=400e3, seed=21, data_seed=30 + t) for t in range(T)]
    p0 = parts[0][0]
    data = tuple(np.concatenate([getattr(parts[t][0], k) for t in range(T)]) for k in ("data_r", "data_i", "wgts"))
    pars = [parts[t][2] for t in range(T)]
    sub, _, _ = batched.replicate_slices(p0, T)
    s = batch_solver(sub, data, {k: np.concatenate([pars[t][k] for t in range(T)]) for k in KEYS}, dtype, layout)
    return s, parts, pars


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", ["stream", "shared"])
def test_a_masked_slice_keeps_its_bits_and_the_others_equal_single_solvers(layout, dtype):
    """Mask [1, 0, 1].  The selected slices against one-slice solvers: bit for bit where the batch's gradient pass gives a slice the bits
    the one-slice solver's gives it (every reduction of the step itself is cut by the slice's own sizes); under the multi-slice kernels
    of shared tiles the passes differ in rounding and the step is held to the short-trajectory bound."""
    s, parts, pars = three_slices(dtype, layout)
    s.set_optimizer("Adam", learning_rate=1e-2)
    s.run_slices(3, tol=0.0)
    start = s.get_params()
    mom = s.get_moments()
    grads = s.eval_grads()
    out = s.gauss_newton_step(ncg=5, lam=[1e-3, 1e-2, 1e-3], slice_mask=[1, 0, 1])
    after, mom2 = s.get_params(), s.get_moments()
    p0 = parts[0][0]
    na, nc = p0.nants, p0.ncoeffs
    assert list(out["accepted"]) == [True, False, True] and out["cg_iters"][1] == 0 and out["loss_after"][1] == out["loss_before"][1]
    for k in range(4):
        part = slice(na, 2 * na) if k < 2 else slice(nc, 2 * nc)
        np.testing.assert_array_equal(after[k][part], start[k][part])
    for k in mom:
        np.testing.assert_array_equal(mom2[k], mom[k], err_msg=k)  # (no reset asked for: every slot stays)
    for t in (0, 2):
        one = solver_of(parts[t][0], {k: start[i][t * (na if i < 2 else nc):(t + 1) * (na if i < 2 else nc)] for i, k in enumerate(KEYS)}, dtype, layout)
        g1 = one.eval_grads()
        bitwise = all(np.array_equal(g1[1 + i], grads[1 + i][t * (na if i < 2 else nc):(t + 1) * (na if i < 2 else nc)]) for i in range(4))
        assert bitwise or layout == "stream", "the SHARED layout fits a slice of a batch with the kernels of a single fit"
        o1 = one.gauss_newton_step(ncg=5, lam=1e-3)
        got1 = one.get_params()
        for i in range(4):
            part = slice(t * (na if i < 2 else nc), (t + 1) * (na if i < 2 else nc))
            err = relnorm(after[i][part], np.asarray(got1[i], dtype=np.float64))
            print(f"{layout} {np.dtype(dtype).name} slice {t} {KEYS[i]}: gradient pass bitwise {bitwise}, error {err:.2e}")
            if bitwise:
                np.testing.assert_array_equal(after[i][part], got1[i])
            else:
                assert err <= TOL[np.dtype(dtype)]["params"]
        if bitwise:
            assert o1["loss_after"][0] == out["loss_after"][t] and o1["cg_residual"][0] == out["cg_residual"][t]
        one.close()
    with pytest.raises(ValueError):
        s.gauss_newton_step(slice_mask=[1, 0])
    s.close()


@pytest.mark.parametrize("optimizer", ["Adam", "Adagrad"])
def test_reset_moments_restores_the_accepted_slices_slots_and_leaves_t(optimizer):
    """Mask [1, 0, 1], both selected slices accepted: their gain and coefficient slots are what set_optimizer leaves (Adagrad's
    accumulator starts at 0.1, not 0), slice 1 keeps its slots, t stays."""
    dtype = np.float64
    s, parts, pars = three_slices(dtype, "stream")
    s.set_optimizer(optimizer, learning_rate=1e-2)
    fresh = s.get_moments()
    s.run_slices(4, tol=0.0)
    moved = s.get_moments()
    out = s.gauss_newton_step(ncg=3, lam=1e-3, slice_mask=[1, 0, 1], reset_moments=True)
    got = s.get_moments()
    assert list(out["accepted"]) == [True, False, True]
    p0 = parts[0][0]
    for k in ("gm_r", "gm_i", "gv_r", "gv_i", "cm_r", "cm_i", "cv_r", "cv_i"):
        n = p0.nants if k[0] == "g" else p0.ncoeffs
        assert np.any(moved[k] != fresh[k]) or (optimizer == "Adagrad" and k[1] == "m"), k  # (Adagrad leaves its first slot unused)
        for t in range(3):
            part = slice(t * n, (t + 1) * n)
            np.testing.assert_array_equal(got[k][part], (moved if t == 1 else fresh)[k][part], err_msg=f"{k} of slice {t}")
    assert got["t"] == moved["t"] == 4
    assert len(s.run_slices(2, tol=0.0)[0][0]) == 2  # and the fit goes on
    s.close()


# ---- a continued run
@pytest.mark.parametrize("config", ["adam", "graph", "kernels"])
def test_a_run_continued_after_an_all_zero_mask_is_bit_identical(config):
    p, params = base_problem(7, 200)
    losses, final = {}, {}
    for with_call in (False, True):
        s = solver_of(p, params, np.float32)
        s.set_launch_mode({"graph": "graph", "kernels": "kernels"}.get(config, "auto"))
        s.set_optimizer("Adam", learning_rate=1e-2)
        first = s.run(20, tol=0.0)[0]
        if with_call:
            out = s.gauss_newton_step(ncg=3, slice_mask=[0], reset_moments=True)
            assert not out["accepted"][0] and out["cg_iters"][0] == 0
            s.normal_product(*direction(p, params, np.float32, 5))
        second = s.run(20, tol=0.0)[0]
        losses[with_call] = np.concatenate([first, second])
        final[with_call] = (s.get_params(), s.get_moments())
        s.close()
    assert len(losses[True]) == 40
    np.testing.assert_array_equal(losses[True], losses[False])
    for a, b in zip(final[True][0], final[False][0]):
        np.testing.assert_array_equal(a, b)
    for k in final[True][1]:
        np.testing.assert_array_equal(final[True][1][k], final[False][1][k], err_msg=k)


# ---- reproducibility
@pytest.mark.parametrize("dtype", DTYPES)
def test_two_fresh_solvers_give_the_same_bits(dtype):
    p, start = start_problem()
    runs = []
    for _ in range(2):
        s = solver_of(p, start, dtype, "stream")
        out = s.gauss_newton_step(ncg=6, lam=1e-3)
        prod = s.normal_product(*direction(p, start, dtype, 8))
        runs.append((out, s.get_params(), prod))
        s.close()
    for k in runs[0][0]:
        np.testing.assert_array_equal(runs[0][0][k], runs[1][0][k], err_msg=k)
    for a, b in zip(runs[0][1] + runs[0][2], runs[1][1] + runs[1][2]):
        np.testing.assert_array_equal(a, b)
    assert runs[0][0]["accepted"][0]


# ---- refusals
def test_wrong_arguments_and_wrong_state_are_reported():
    from calamity_amd.solver import HipFitSolver

    p, params = base_problem(7, 200)
    s = solver_of(p, params, np.float64)
    for kw in (dict(ncg=0), dict(cg_tol=-1.0), dict(cg_tol=np.inf), dict(lam=-1e-3), dict(lam=np.nan)):
        with pytest.raises(_lib.CalamityHipError) as err:
            s.gauss_newton_step(**kw)
        assert err.value.code == _lib.CAL_ERR_INVALID and "gauss_newton_step" in str(err.value), kw
    with pytest.raises(_lib.CalamityHipError) as err:  # no optimizer
        s.gauss_newton_step(reset_moments=True)
    assert err.value.code == _lib.CAL_ERR_STATE and "optimizer" in str(err.value)
    d = direction(p, params, np.float64, 1)
    lib = _lib.load()
    assert lib.cal_solver_normal_product(s._h, None, None, None, None, None, None, None, None) == _lib.CAL_ERR_INVALID
    assert lib.cal_solver_gauss_newton_step(s._h, None, None) == _lib.CAL_ERR_INVALID
    s.set_gain_basis(np.array(modeling.gain_dpss_basis(150e6 + 400e3 * np.arange(p.nfreqs), 100.0)))
    for call in (lambda: s.gauss_newton_step(), lambda: s.normal_product(*d)):
        with pytest.raises(_lib.CalamityHipError) as err:
            call()
        assert err.value.code == _lib.CAL_ERR_UNSUPPORTED and "basis" in str(err.value)
    s.set_gain_basis(None)
    assert s.gauss_newton_step(ncg=2)["cg_iters"][0] == 2
    s.close()
    # an exchange hook
    s = HipFitSolver(dtype=np.float64)
    s.set_exchange_hook(lambda arr, op: None, 0, 1)
    s.set_problem(p)
    s.set_params(*[params[k] for k in KEYS])
    for call in (lambda: s.gauss_newton_step(), lambda: s.normal_product(*d)):
        with pytest.raises(_lib.CalamityHipError) as err:
            call()
        assert err.value.code == _lib.CAL_ERR_UNSUPPORTED and "exchange" in str(err.value)
    s.close()
    # no gains
    shell = copy.copy(p)
    shell.data_r = shell.data_i = shell.wgts = None
    s = HipFitSolver(dtype=np.float64)
    s.set_problem(shell)
    s.set_data(p.data_r, p.data_i, p.wgts)
    s.set_params(c_r=params["c_r"], c_i=params["c_i"])
    for call in (lambda: s.gauss_newton_step(), lambda: s.normal_product(*d)):
        with pytest.raises(_lib.CalamityHipError) as err:
            call()
        assert err.value.code == _lib.CAL_ERR_STATE
    s.close()


def test_memory_bytes_counts_the_step_buffers():
    p, params = base_problem(7, 200)
    s = solver_of(p, params, np.float32)
    before = s.memory_bytes()
    s.gauss_newton_step(ncg=1)
    # at least: three T and four double vectors of the parameter space, m and the saved data planes
    np_ = 2 * p.nants * 256 + 2 * p.ncoeffs
    assert s.memory_bytes() - before >= np_ * (3 * 4 + 4 * 8) + 4 * p.nbls * 256 * 4
    s.close()
