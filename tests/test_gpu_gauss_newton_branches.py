"""cal_solver_gauss_newton_step where its kernels branch and past one trip of their loops (csrc/gauss_newton_kernels.hpp, gauss_newton_step
in csrc/calamity_hip.hip), against the NumPy restatement tests/gauss_newton_ref.py.  tests/test_gpu_gauss_newton.py follows the call in
which every selected slice runs all its iterations on 7 antennas; here the inputs take the device through everything else:

    1  conjugate gradients that stop at cg_tol: gn_scalar2_kernel freezes the slice and the launches after it move nothing
    2  three slices that stop at different iterations in one call: a frozen slice beside live ones, above and below
    3  a slice frozen at the start by gn_scalar0_kernel for rz = 0 (all weights zero) and for a rz that is not finite (a NaN in its data)
    4  gn_fix_diag: a fully flagged antenna (den = 0) and fully flagged groups (row sum 0) get D = 1 and a direction of exactly 0
    5  gn_precond_coeff_kernel over a fitting group of three baselines, in an accepted and in a rejected step
    6  276 rows in 276 groups and 37 496 reals a slice: the second trip of every vector kernel (also for t > 0), gn_scale_kernel with
       two rows a thread and empty runs, gn_precond_coeff_kernel's second block

Tolerances are TOL of tests/test_gpu_gauss_newton.py and nothing new (parameters norm-wise fp64 1e-8, fp32 1e-3; losses fp64 1e-10,
fp32 1e-5; the product fp64 1e-10, fp32 1e-4), but for one measured bound: cg_residual against the restatement's, RESID_BOUND below.
Every comparison first asserts the decisions of the RESTATEMENT and their margins (``planned``): the residual of every iteration it went
on from is at least 1.5 cg_tol, the residual it stopped at is at most cg_tol / 1.5, and the trial's loss differs from the loss before by
at least 1e-2 of it.  The expected iteration counts and acceptances are written down in PLAN and asserted of the restatement; none is read
off the device.  The host parts (PLAN, the margins, the sizes of case 6) run without a GPU in tests/test_gauss_newton_branches_host.py.

"Both layouts" are the kernel paths ("stream", "auto") and ("shared", "dense") for one slice.  The batches come from ``three_slices``,
which takes a layout only: STREAM and SHARED with the path the solver chooses.  Case 5 runs ("shared", "auto") because set_problem
refuses the dense path for a fitting group of several baselines.

cg_residual: |device - restatement| / restatement, the largest value over every test of this file on an MI355X:
    fp64  1.29e-15  (case 4, STREAM; every other value between 0 and 1.01e-15)
    fp32  5.21e-07  (case 2, SHARED, lambda = 1e-3; then 2.16e-07 case 2 STREAM, 1.82e-07 case 1 dense, 1.07e-07 case 3, 8.10e-08 case 4,
                     4.80e-08 case 6, 2.57e-08 case 5)
RESID_BOUND is ten times that rounded up to a power of ten, fp64 1e-13 and fp32 1e-5: the quantity is the root of a ratio of two sums,
each of which can differ by an ulp of the gradient pass per term.

Measured on an MI355X, the largest error over the layouts of a case, fp64 / fp32 (bounds: parameters 1e-8 / 1e-3, losses 1e-10 / 1e-5,
product 1e-10 / 1e-4):
    case  parameters           losses               besides
    1     5.9e-16 / 2.0e-07    4.3e-16 / 1.4e-07    the three calls agree bit for bit where they must
    2     2.0e-15 / 6.3e-07    2.3e-15 / 7.1e-07    one-slice solvers: SHARED bit for bit, STREAM 1.6e-15 / 7.1e-07
    3     8.3e-16 / 2.8e-07    1.1e-15 / 1.9e-07    one-slice solvers as in 2 (5.3e-16 / 2.5e-07); the product afterwards 3.7e-16 / 1.5e-07
    4     9.3e-16 / 3.3e-07    1.1e-15 / 1.3e-06
    5     6.5e-16 / 2.2e-07    4.1e-16 / 3.7e-08
    6     6.4e-16 / 2.2e-07    7.2e-16 / 3.6e-07    the product 9.3e-16 / 7.1e-07

What the file is worth was tried with deliberately wrong (memory-safe) builds: gn_update1_kernel making one trip only fails the three step
tests of case 6; D of a group from its first row only fails all of case 5; gn_update1_kernel ignoring the freeze fails all of cases 1 and
2; a scale s_t of 1 throughout fails the fp32 product tests of case 6.  gn_scale_kernel dropping the rows past 256 from s_t fails nothing: s_t
cancels from N p, see test_product_parity_past_256_rows.

Left out: the freeze at s.Ns <= 0 in gn_scalar1_kernel (N + lambda D is positive semi-definite with D > 0; s.Ns <= 0 needs s = 0, which
rz = 0 has caught already: not reachable from finite data); a damping so large that the fp32 trial rounds back to the start (the accept
decision is then marginal by construction); anything under a communicator or a gain basis (gn_check refuses both, tested in
tests/test_gpu_gauss_newton.py)."""
import copy
import functools
import types

import numpy as np
import pytest

from calamity_amd import batched, synthetic
from gauss_newton_ref import Ref
from test_gpu_fit_quality import perturbed, solver_of
from test_gpu_gauss_newton import CONFIGS, KEYS, TOL, assert_path, batch_solver, cast_params, check_product, direction, relnorm, slice_refs, start_problem, three_slices

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
TWO_PATHS = [c for c in CONFIGS if (c[0], c[1]) in (("stream", "auto"), ("shared", "dense"))]
GROUP_PATHS = [("stream", "auto", None), ("shared", "auto", None)]  # (the dense path takes one baseline a group)
CG_TOL = 7e-4
STOP_MARGIN, ACCEPT_MARGIN = 1.5, 1e-2
RESID_BOUND = {np.dtype(np.float64): 1e-13, np.dtype(np.float32): 1e-5}
# csrc/gauss_newton_kernels.hpp: the vector kernels run kGnBlocks blocks of 256 threads a slice, gn_scale_kernel 256 threads a slice,
# gn_precond_coeff_kernel 256 groups a block; csrc/problem_plan.hpp: rows are padded to a multiple of min(128, next_pow2(nfreqs))
GN_BLOCKS, GN_THREADS = 128, 256


def name(dtype):
    return np.dtype(dtype).name


def path_id(config):
    return f"{config[0]}-{config[1]}"


# ---- the problems
def spoiled(q, how):
    q = copy.copy(q)
    if how == "nan":
        d = np.array(q.data_r)
        b, f = np.argwhere(np.asarray(q.wgts) > 0)[5]
        d[b, f] = np.nan
        q.data_r = d
    elif how == "zero_weights":
        q.wgts = np.zeros_like(np.asarray(q.wgts))
    return q


@functools.lru_cache(maxsize=None)
def slice_problem(t, how=None):
    """Slice ``t`` of ``three_slices`` and its start values."""
    p, _, start = synthetic.make_problem(7, 200, f0=150e6, df=400e3, seed=21, data_seed=30 + t)
    return spoiled(p, how), start


FLAGGED_ANTENNA = 3


@functools.lru_cache(maxsize=None)
def flagged_problem():
    """``start_problem`` with every row of antenna 3 flagged: six rows, each its own group."""
    p, start = start_problem()
    q = copy.copy(p)
    w = np.array(p.wgts)
    w[flagged_rows(p)] = 0.0
    q.wgts = w
    return q, start


def flagged_rows(p):
    return np.where((np.asarray(p.bl_ant0) == FLAGGED_ANTENNA) | (np.asarray(p.bl_ant1) == FLAGGED_ANTENNA))[0]


@functools.lru_cache(maxsize=None)
def redundant_problem():
    p0, _, start0 = synthetic.make_problem(7, 200, f0=150e6, df=400e3, seed=13)
    return synthetic.add_redundant_group(p0, start0, np.random.default_rng(1), nred=3)


@functools.lru_cache(maxsize=None)
def big_problem(data_seed=None):
    p, _, start = synthetic.make_problem(24, 260, f0=150e6, df=400e3, seed=5, data_seed=data_seed)
    return p, start


def problem_of(key):
    return {"slice": slice_problem, "flagged": flagged_problem, "redundant": redundant_problem, "big": big_problem}[key[0]](*key[1:])


def fpad_of(nfreqs):
    pw = 8
    while pw < 128 and pw < nfreqs:
        pw *= 2
    return -(-nfreqs // pw) * pw


def big_sizes(p):
    """The sizes case 6 exists for, asserted from the problem: more rows than gn_scale_kernel has threads, more groups than a block of
    gn_precond_coeff_kernel, more reals a slice than one trip of the vector kernels, and the second trip inside the coefficients."""
    fpad = fpad_of(p.nfreqs)
    ng, nreals = 2 * p.nants * fpad, 2 * p.nants * fpad + 2 * p.ncoeffs
    per = -(-p.nbls // GN_THREADS)
    sizes = dict(nbls=p.nbls, ngrps=p.ngrps, ncoeffs=p.ncoeffs, fpad=fpad, gain_reals=ng, reals=nreals, rows_per_thread=per,
                 empty_runs=GN_THREADS - -(-p.nbls // per))
    assert p.nbls > GN_THREADS and p.ngrps > GN_THREADS and nreals > GN_BLOCKS * GN_THREADS, sizes
    # the first trip crosses from the gains into the real and on into the imaginary coefficient plane, the second trip lies in the imaginary one
    assert ng + p.ncoeffs < GN_BLOCKS * GN_THREADS < nreals, sizes
    assert per > 1 and sizes["empty_runs"] > 0, sizes
    return sizes


# ---- the restatement's decisions
# label: (problem, lambda, ncg, cg_tol, the restatement's cg_iters, accepted)
PLAN = {
    "stop": (("slice", 0), 1.0, 10, CG_TOL, 6, True),
    "stop, ncg 5": (("slice", 0), 1.0, 5, CG_TOL, 5, True),
    "stop, ncg 6, cg_tol 0": (("slice", 0), 1.0, 6, 0.0, 6, True),
    "batch 1": (("slice", 1), 0.1, 10, CG_TOL, 10, True),
    "batch 2": (("slice", 2), 1e-3, 10, CG_TOL, 10, True),
    "reversed 0": (("slice", 0), 1e-3, 10, CG_TOL, 10, True),
    "reversed 2": (("slice", 2), 1.0, 10, CG_TOL, 6, True),
    "beside 0": (("slice", 0), 1e-3, 5, 0.0, 5, True),
    "beside 2": (("slice", 2), 1e-3, 5, 0.0, 5, True),
    "zero_weights": (("slice", 1, "zero_weights"), 1e-3, 5, 0.0, 0, False),
    "nan": (("slice", 1, "nan"), 1e-3, 5, 0.0, 0, False),
    "flagged": (("flagged",), 1e-3, 5, 0.0, 5, True),
    "group, accepted": (("redundant",), 0.1, 5, 0.0, 5, True),
    "group, rejected": (("redundant",), 1e-3, 5, 0.0, 5, False),
    "big": (("big",), 1e-3, 5, 0.0, 5, True),
    "big, second slice": (("big", 6), 1e-3, 5, 0.0, 5, True),
}
BATCH = (("stop", "batch 1", "batch 2"), ("reversed 0", "batch 1", "reversed 2"))


@functools.lru_cache(maxsize=None)
def restated(key, dtype_name, lam, ncg, cg_tol):
    p, start = problem_of(key)
    dtype = np.dtype(dtype_name).type
    return Ref(p, dtype=dtype).step(*cast_params(start, dtype), lam=lam, ncg=ncg, cg_tol=cg_tol)


def margins(want, cg_tol):
    """(the smallest residual the restatement went on from over cg_tol, cg_tol over the residual it stopped at, |trial - before| / before);
    inf where there is no such decision."""
    r = want["residuals"]
    stopped = len(r) > 0 and r[-1] <= cg_tol
    on = r[:-1] if stopped else r
    went_on = min(on) / cg_tol if cg_tol > 0 and len(on) else np.inf
    stop = cg_tol / r[-1] if stopped else np.inf
    before, after = want["loss_before"], want["loss_after"]
    accept = abs(after - before) / before if np.isfinite(after) and before > 0 else np.inf  # (0 < 0 and NaN < NaN are no close calls)
    return went_on, stop, accept


def planned(label, dtype):
    """The restatement of PLAN[label]: prints its counters and margins, asserts the margins and that it decided as PLAN says."""
    key, lam, ncg, cg_tol, iters, accepted = PLAN[label]
    want = restated(key, name(dtype), lam, ncg, cg_tol)
    went_on, stop, accept = margins(want, cg_tol)
    print(f"{label} {name(dtype)}: the restatement: cg_iters {want['cg_iters']} of {ncg}, residuals " + " ".join(f"{r:.3e}" for r in want["residuals"])
          + f"; {'accepted' if want['accepted'] else 'rejected'} {want['loss_before']:.4e} -> {want['loss_after']:.4e}; margins: went on {went_on:.2f} x cg_tol, "
          f"stopped {stop:.2f} x under, trial {accept:.2e}")
    assert went_on >= STOP_MARGIN and stop >= STOP_MARGIN and accept >= ACCEPT_MARGIN, "choose an input whose decisions are not marginal"
    assert (want["cg_iters"], want["accepted"]) == (iters, accepted), label
    assert len(want["residuals"]) == iters and (want["cg_residual"] == want["residuals"][-1] if iters else want["cg_residual"] == 0.0)
    return want


# ---- the device against the restatement
def fresh(p, start, dtype, config):
    layout, path, runs = config
    s = solver_of(p, start, dtype, layout, path)
    if runs:
        assert_path(s, runs)
    return s


def cut(i, t, na, nc):
    """Slice ``t`` of plane ``i`` of (g_r, g_i, c_r, c_i)."""
    n = na if i < 2 else nc
    return slice(t * n, (t + 1) * n)


def check_residual(label, got, want, dtype):
    if want == 0.0:
        assert got == 0.0, label
        return
    err = abs(got - want) / want
    print(f"{label}: cg_residual {got:.6e} against {want:.6e}, |device - restatement| / restatement {err:.2e}")
    assert err <= RESID_BOUND[np.dtype(dtype)], (label, err)


def check_slice(label, out, got, want, dtype, t=0, na=None, nc=None, params=True):
    """Slice ``t`` of a call's results ``out`` and of the parameters ``got`` after it against the restatement ``want``."""
    tol = TOL[np.dtype(dtype)]
    assert out["cg_iters"][t] == want["cg_iters"] and bool(out["accepted"][t]) == want["accepted"], (label, out["cg_iters"][t], out["accepted"][t])
    lerr = [abs(out[k][t] - want[k]) / want[k] for k in ("loss_before", "loss_after")]
    na, nc = want["g"].shape[0] if na is None else na, want["c"].shape[0] if nc is None else nc
    errs = [relnorm(got[i][cut(i, t, na, nc)], w) for i, w in enumerate((want["g"].real, want["g"].imag, want["c"].real, want["c"].imag))]
    print(f"{label}: " + "  ".join(f"{k} {e:.2e}" for k, e in zip(KEYS, errs)) + f"  loss_before {lerr[0]:.2e}  loss_after {lerr[1]:.2e}  "
          f"({out['loss_before'][t]:.4e} -> {out['loss_after'][t]:.4e}, cg_iters {out['cg_iters'][t]})")
    check_residual(label, out["cg_residual"][t], want["cg_residual"], dtype)
    assert max(lerr) <= tol["loss"], (label, lerr)
    if params:
        assert max(errs) <= tol["params"], (label, errs)
    return errs


# ---- 1: conjugate gradients that stop at cg_tol
@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("config", TWO_PATHS, ids=path_id)
def test_conjugate_gradients_stop_at_cg_tol_and_the_launches_after_move_nothing(config, dtype):
    """gn_scalar2_kernel: frozen once sqrt(rz / rz0) <= tol; gn_diff_kernel, gn_update1_kernel, gn_update2_kernel, gn_scalar1_kernel and
    gn_scalar2_kernel return for the slice in the four rounds the host still launches.  Slice 0 of three_slices, lambda = 1,
    cg_tol = 7e-4, ncg = 10: the restatement's residual is 1.272e-3 after iteration 5 and 4.46e-4 after iteration 6.  A solver with
    ncg = 5 must still be above cg_tol (the stop is not one iteration early), and a solver with ncg = 6, cg_tol = 0 must leave the bits
    the stopped call leaves (the stop is not late, and nothing moves after it)."""
    p, start = problem_of(("slice", 0))
    runs = {}
    for label in ("stop", "stop, ncg 5", "stop, ncg 6, cg_tol 0"):
        want = planned(label, dtype)
        _, lam, ncg, cg_tol = PLAN[label][:4]
        s = fresh(p, start, dtype, config)
        out = s.gauss_newton_step(ncg=ncg, lam=lam, cg_tol=cg_tol)
        got = s.get_params()
        check_slice(f"{label} {path_id(config)} {name(dtype)}", out, got, want, dtype)
        assert s.eval_loss() == out["loss_after"][0]
        runs[label] = (out, got)
        s.close()
    stop, short, exact = (runs[k] for k in ("stop", "stop, ncg 5", "stop, ncg 6, cg_tol 0"))
    assert stop[0]["cg_iters"][0] == 6 and stop[0]["accepted"][0] and stop[0]["cg_residual"][0] <= CG_TOL
    assert short[0]["cg_iters"][0] == 5 and short[0]["cg_residual"][0] > CG_TOL
    for a, b in zip(stop[1], exact[1]):
        np.testing.assert_array_equal(a, b)
    for k in ("loss_before", "loss_after", "cg_residual", "cg_iters", "accepted"):
        np.testing.assert_array_equal(stop[0][k], exact[0][k], err_msg=k)


# ---- 2: slices that stop at different iterations in one call
def against_single_solvers(s_out, after, grads, parts, pars, lams, call, dtype, layout, label):
    """Every slice ``t`` with PLAN entry or None in ``lams`` against a one-slice solver given the same call: bit for bit where the batch's
    gradient pass gives the slice the bits of the one-slice solver's (the rule and the probe of
    test_a_masked_slice_keeps_its_bits_and_the_others_equal_single_solvers), at the parameter tolerance otherwise."""
    na, nc = parts[0][0].nants, parts[0][0].ncoeffs
    for t, lam in enumerate(lams):
        if lam is None:
            continue
        one = solver_of(parts[t][0], pars[t], dtype, layout)
        g1 = one.eval_grads()
        bitwise = all(np.array_equal(g1[1 + i], grads[1 + i][cut(i, t, na, nc)]) for i in range(4))
        assert bitwise or layout == "stream", "the SHARED layout fits a slice of a batch with the kernels of a single fit"
        o1 = one.gauss_newton_step(lam=lam, **call)
        got1 = one.get_params()
        assert o1["cg_iters"][0] == s_out["cg_iters"][t] and o1["accepted"][0] == s_out["accepted"][t], (label, t)
        for i in range(4):
            err = relnorm(after[i][cut(i, t, na, nc)], np.asarray(got1[i], dtype=np.float64))
            print(f"{label} slice {t} {KEYS[i]} against its one-slice solver: gradient pass bitwise {bitwise}, error {err:.2e}")
            if bitwise:
                np.testing.assert_array_equal(after[i][cut(i, t, na, nc)], got1[i])
            else:
                assert err <= TOL[np.dtype(dtype)]["params"], (label, t, KEYS[i], err)
        if bitwise:
            assert o1["loss_after"][0] == s_out["loss_after"][t] and o1["cg_residual"][0] == s_out["cg_residual"][t]
        one.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("layout", ["stream", "shared"])
@pytest.mark.parametrize("order", [0, 1], ids=["early-stop-first", "early-stop-last"])
def test_three_slices_stop_at_different_iterations_in_one_call(order, layout, dtype):
    """three_slices from its start values, ncg = 10, cg_tol = 7e-4, lambda = [1, 0.1, 1e-3]: the restatement stops slice 0 after 6
    iterations (4.46e-4) and runs slices 1 and 2 to the end (2.12e-3, 9.07e-3: 3 and 13 times the threshold).  For four rounds the
    frozen slice's part[] lines and s are stale, the passes still run over it and gn_scale_kernel still writes its scale: none of it
    may reach x of any slice.  With the list reversed the frozen slice is the last one, below live neighbours."""
    labels = BATCH[order]
    wants = [planned(k, dtype) for k in labels]
    lams = [PLAN[k][1] for k in labels]
    assert [w["cg_iters"] for w in wants] == ([6, 10, 10] if order == 0 else [10, 10, 6]) and all(w["accepted"] for w in wants)
    s, parts, pars = three_slices(dtype, layout)
    grads = s.eval_grads()
    call = dict(ncg=10, cg_tol=CG_TOL)
    out = s.gauss_newton_step(lam=lams, **call)
    after = s.get_params()
    label = f"lambda {lams} {layout} {name(dtype)}"
    print(f"{label}: cg_iters {list(out['cg_iters'])} accepted {list(out['accepted'])} cg_residual {list(out['cg_residual'])}")
    for t, want in enumerate(wants):
        check_slice(f"{label} slice {t}", out, after, want, dtype, t=t)
        assert (out["cg_residual"][t] <= CG_TOL) == (want["cg_iters"] < 10)
    s.eval_loss()
    np.testing.assert_array_equal(s.slice_losses(), out["loss_after"])
    against_single_solvers(out, after, grads, parts, pars, lams, call, dtype, layout, label)
    s.close()


# ---- 3: a slice with nothing to solve
NOTHING = [("zero_weights", "stream"), ("zero_weights", "shared"), ("nan", "stream")]


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("how,layout", NOTHING, ids=[f"{h}-{l}" for h, l in NOTHING])
def test_a_slice_with_nothing_to_solve_starts_frozen_and_its_neighbours_run_on(how, layout, dtype):
    """gn_scalar0_kernel: frozen where !(rz > 0 && isfinite(rz)) with every mask byte set.  Slice 1 of three_slices has all its weights zero
    (rz = 0: both losses 0, and 0 < 0 rejects) or one NaN in data_r where its weight is positive (rz NaN: loss_before NaN).  The NaN is
    ordinary data: nothing here faults.  s of the frozen slice holds 0 or NaN through all five rounds of passes over the whole batch;
    slices 0 and 2 must run as if alone, slice 1 keeps every bit of its parameters and, under reset_moments, of its moment slots, and
    afterwards the data planes are back: normal_product and the loss of slices 0 and 2 are what their parameters give."""
    wants = [planned("beside 0", dtype), planned(how, dtype), planned("beside 2", dtype)]
    assert wants[1]["cg_iters"] == 0 and wants[1]["cg_residual"] == 0.0 and not wants[1]["accepted"] and not wants[1]["rz0"] > 0
    s, parts, pars = three_slices(dtype, layout)
    grads = s.eval_grads()  # (the probe of the gradient pass, on the good data: slices 0 and 2 keep theirs)
    s.set_optimizer("Adam", learning_rate=1e-2)
    fresh_m = s.get_moments()
    s.set_moments(*[fresh_m[k] + 0.25 for k in ("gm_r", "gm_i", "gv_r", "gv_i", "cm_r", "cm_i", "cv_r", "cv_i")], 4)
    moved = s.get_moments()
    qs = [parts[0][0], problem_of(PLAN[how][0])[0], parts[2][0]]
    s.set_data(*[np.concatenate([np.asarray(getattr(q, k)) for q in qs]) for k in ("data_r", "data_i", "wgts")])
    before = s.get_params()
    call = dict(ncg=5, cg_tol=0.0)
    out = s.gauss_newton_step(lam=1e-3, reset_moments=True, **call)
    after, mom = s.get_params(), s.get_moments()
    label = f"{how} {layout} {name(dtype)}"
    print(f"{label}: cg_iters {list(out['cg_iters'])} accepted {list(out['accepted'])} cg_residual {list(out['cg_residual'])} "
          f"loss_before {list(out['loss_before'])} loss_after {list(out['loss_after'])}")
    assert list(out["cg_iters"]) == [5, 0, 5] and list(out["accepted"]) == [True, False, True] and out["cg_residual"][1] == 0.0
    if how == "nan":
        assert np.isnan(out["loss_before"][1]) and np.isnan(wants[1]["loss_before"])
    else:
        assert out["loss_before"][1] == out["loss_after"][1] == 0.0 and wants[1]["loss_before"] == wants[1]["loss_after"] == 0.0 and wants[1]["rz0"] == 0.0
    na, nc = qs[0].nants, qs[0].ncoeffs
    for i in range(4):
        np.testing.assert_array_equal(after[i][cut(i, 1, na, nc)], before[i][cut(i, 1, na, nc)], err_msg=f"slice 1 {KEYS[i]}")
    for k in ("gm_r", "gm_i", "gv_r", "gv_i", "cm_r", "cm_i", "cv_r", "cv_i"):
        i = 0 if k[0] == "g" else 2
        assert np.all(moved[k] != fresh_m[k]), k
        for t in range(3):
            np.testing.assert_array_equal(mom[k][cut(i, t, na, nc)], (moved if t == 1 else fresh_m)[k][cut(i, t, na, nc)], err_msg=f"{k} of slice {t}")
    assert mom["t"] == moved["t"] == 4
    for t in (0, 2):
        check_slice(f"{label} slice {t}", out, after, wants[t], dtype, t=t)
    against_single_solvers(out, after, grads, parts, pars, [1e-3, None, 1e-3], call, dtype, layout, label)
    # afterwards: the data planes are the caller's again
    s.eval_loss()
    losses = s.slice_losses()
    d = direction(types.SimpleNamespace(nants=s.nants, nfreqs=s.nfreqs, ncoeffs=s.ncoeffs), dict(zip(KEYS, after)), dtype, 9)
    prod = s.normal_product(*d)
    for t in (0, 2):
        assert losses[t] == out["loss_after"][t]
        cuts = [cut(i, t, na, nc) for i in range(4)]
        g, c = cast_params({k: after[i][cuts[i]] for i, k in enumerate(KEYS)}, dtype)
        dg, dc = cast_params({k: d[i][cuts[i]] for i, k in enumerate(KEYS)}, dtype)
        want_g, want_c = Ref(qs[t], dtype=dtype).normal_product(g, c, dg, dc)
        errs = [relnorm(prod[i][cuts[i]], w) for i, w in enumerate((want_g.real, want_g.imag, want_c.real, want_c.imag))]
        print(f"{label} slice {t}: the product afterwards " + "  ".join(f"{k} {e:.2e}" for k, e in zip(KEYS, errs)))
        assert all(np.all(np.isfinite(prod[i][cuts[i]])) for i in range(4)) and max(errs) <= TOL[np.dtype(dtype)]["product"], (label, t, errs)
    s.close()


# ---- 4: preconditioner entries replaced by 1
@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("config", TWO_PATHS, ids=path_id)
def test_a_flagged_antenna_and_its_groups_get_unit_preconditioner_entries_and_keep_their_bits(config, dtype):
    """gn_fix_diag in gn_precond_gain_kernel (den = 0 for every channel of antenna 3) and in gn_precond_coeff_kernel (row sum 0 for its
    six groups): D = 1 there, rhs = 0 there, so s, N s and x stay exactly 0 and the accepted step leaves the bits of those gains and
    coefficients.  A D of 0 or a D not replaced gives 0 / 0 = NaN in gn_init_kernel and the whole slice freezes at the start."""
    want = planned("flagged", dtype)
    p, start = flagged_problem()
    rows = flagged_rows(p)
    coff = np.asarray(p.grp_coff)
    assert len(rows) == 6 and np.all(np.diff(p.grp_bl_start) == 1)
    idx = np.concatenate([np.arange(coff[g], coff[g + 1]) for g in rows])
    assert np.all(want["dg"][FLAGGED_ANTENNA] == 0) and np.all(want["dc"][idx] == 0) and np.all(want["dc"][np.setdiff1d(np.arange(p.ncoeffs), idx)] != 0)
    s = fresh(p, start, dtype, config)
    before = s.get_params()
    out = s.gauss_newton_step(ncg=5, lam=1e-3, cg_tol=0.0)
    got = s.get_params()
    check_slice(f"antenna {FLAGGED_ANTENNA} flagged {path_id(config)} {name(dtype)}", out, got, want, dtype)
    for i in range(4):
        part = FLAGGED_ANTENNA if i < 2 else idx
        np.testing.assert_array_equal(got[i][part], before[i][part], err_msg=KEYS[i])
    assert np.any(got[2] != before[2]) and np.any(got[0] != before[0])
    assert s.eval_loss() == out["loss_after"][0]
    s.close()


# ---- 5: a fitting group of several baselines
@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("config", GROUP_PATHS, ids=path_id)
@pytest.mark.parametrize("label", ["group, accepted", "group, rejected"])
def test_a_step_with_a_fitting_group_of_three_baselines(label, config, dtype):
    """gn_precond_coeff_kernel sums rowq over b0 .. b1 with b1 - b0 = 3.  lambda = 0.1: the restatement accepts, 0.2124 -> 0.1353.
    lambda = 1e-3: it rejects, the trial has 0.3436; the device keeps every bit and reports the trial's loss, which depends on D of
    the three-row group through all five iterations (D from the first row alone moves it far beyond the loss tolerance)."""
    want = planned(label, dtype)
    p, start = redundant_problem()
    assert np.diff(p.grp_bl_start).max() == 3
    s = fresh(p, start, dtype, config)
    before = s.get_params()
    out = s.gauss_newton_step(ncg=5, lam=PLAN[label][1], cg_tol=0.0)
    got = s.get_params()
    check_slice(f"{label} {path_id(config)} {name(dtype)}", out, got, want, dtype)  # (rejected: want["g"], want["c"] are the start)
    if not want["accepted"]:
        assert out["loss_after"][0] > out["loss_before"][0]
        for a, b in zip(got, before):
            np.testing.assert_array_equal(a, b)
    assert s.eval_loss() == out["loss_after" if want["accepted"] else "loss_before"][0]
    s.close()


# ---- 6: past one trip, 256 rows and 256 groups
@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("config", TWO_PATHS, ids=path_id)
def test_product_parity_past_256_rows(config, dtype):
    """gn_scale_kernel with per = 2 (138 runs of two rows, 118 empty runs) and gn_diff_kernel's second trip (D == nullptr), from perturbed
    parameters.  s_t only conditions the difference of two gradients and cancels from N p: a build that drops the rows past 256 from
    s_t passes this test and every other here (tried on an MI355X), so no parity test can pin the cut itself.  What fails here is a
    run that leaves s_t unusable (0, NaN or the fall-back 1 for the direction of size 1e-6, which costs fp32 its digits) and a second
    trip of gn_diff_kernel that skips or repeats elements of N p."""
    p, start = big_problem()
    sizes = big_sizes(p)
    params = perturbed(p, start, seed=6)
    s = fresh(p, params, dtype, config)
    worst = check_product(s, slice_refs(p, params, dtype), p, params, dtype, f"24 x 260 {path_id(config)} {name(dtype)}")
    print(f"sizes {sizes}; worst product error {worst:.2e}")
    s.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("config", TWO_PATHS, ids=path_id)
def test_a_step_past_one_trip_of_the_vector_kernels(config, dtype):
    """make_problem(24, 260): 18 432 gain reals and 19 064 coefficient reals a slice against 128 x 256 = 32 768 threads: gn_rhs_kernel,
    gn_init_kernel, gn_diff_kernel, gn_update1_kernel, gn_update2_kernel and gn_apply_kernel make a second trip, over the last 4728 reals of the
    imaginary coefficient plane (the first trip crosses the gains and both planes' starts); gn_precond_coeff_kernel runs a second block (276 groups).  A second trip
    that reads the first trip's elements again, or coefficients past 32 768 left out of a dot product, miss the parameter bound."""
    want = planned("big", dtype)
    p, start = big_problem()
    sizes = big_sizes(p)
    assert (sizes["nbls"], sizes["ngrps"], sizes["ncoeffs"], sizes["fpad"], sizes["reals"]) == (276, 276, 9532, 384, 37496)
    s = fresh(p, start, dtype, config)
    out = s.gauss_newton_step(ncg=5, lam=1e-3, cg_tol=0.0)
    check_slice(f"24 x 260 {path_id(config)} {name(dtype)}", out, s.get_params(), want, dtype)
    assert s.eval_loss() == out["loss_after"][0]
    s.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_the_second_trip_of_the_second_slice(dtype):
    """Two slices of make_problem(24, 260) in one solver (the second with its own data), mask [0, 1]: gn_index on a second trip for
    t = 1, where the flat index adds t ng to the gains and coff[t] to both coefficient planes, and gn_scale_kernel's runs from
    row_ptr[1] = 276.  Slice 1 against the restatement of its own problem; slice 0 keeps every bit."""
    want = planned("big, second slice", dtype)
    (p, start), (p2, start2) = big_problem(), big_problem(6)
    big_sizes(p2)
    sub, _, _ = batched.replicate_slices(p, 2)
    data = tuple(np.concatenate([getattr(q, k) for q in (p, p2)]) for k in ("data_r", "data_i", "wgts"))
    s = batch_solver(sub, data, {k: np.concatenate([start[k], start2[k]]) for k in KEYS}, dtype, "stream")
    before = s.get_params()
    out = s.gauss_newton_step(ncg=5, lam=1e-3, cg_tol=0.0, slice_mask=[0, 1])
    got = s.get_params()
    assert not out["accepted"][0] and out["cg_iters"][0] == 0 and out["loss_after"][0] == out["loss_before"][0]
    for i in range(4):
        np.testing.assert_array_equal(got[i][cut(i, 0, p.nants, p.ncoeffs)], before[i][cut(i, 0, p.nants, p.ncoeffs)], err_msg=f"slice 0 {KEYS[i]}")
    check_slice(f"two slices of 24 x 260, slice 1, {name(dtype)}", out, got, want, dtype, t=1)
    s.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_two_fresh_solvers_give_the_same_bits_past_one_trip(dtype):
    """The fixed-order sums with two terms a thread (gn_block_sum's partials over two trips, gn_scale_kernel's runs of two rows)."""
    p, start = big_problem()
    big_sizes(p)
    d = direction(p, start, dtype, 8)
    runs = []
    for _ in range(2):
        s = solver_of(p, start, dtype, "stream")
        out = s.gauss_newton_step(ncg=5, lam=1e-3, cg_tol=0.0)
        runs.append((out, s.get_params(), s.normal_product(*d)))
        s.close()
    for k in runs[0][0]:
        np.testing.assert_array_equal(runs[0][0][k], runs[1][0][k], err_msg=k)
    for a, b in zip(runs[0][1] + runs[0][2], runs[1][1] + runs[1][2]):
        np.testing.assert_array_equal(a, b)
    assert runs[0][0]["accepted"][0] and runs[0][0]["cg_iters"][0] == 5
