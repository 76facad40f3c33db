"""The closed-form calls and fit quality on the solver configurations production runs them in: the dense matrix-core kernel paths, a
descent continued through a call at graph length, the "sum" regulariser set on the solver; and the two branches of the solve kernels
that nothing else reaches by construction (an exact-zero pivot part-way through a factorisation).

Every solver built here asserts that ``timing_get()["kernel_path"]`` is the path it asked for: a silent fall-back to the general
kernels fails the test.  The dense paths need the SHARED layout, one baseline per fitting group and more than 64 channels; the
problems are the smallest the suite has that qualify (``edge_problem(7, 200)``, ``edge_problem(12, 129)``, ``flagged_case`` with 72
channels).

Tolerances are the project's own (``TOL`` of tests/test_gpu_fit_quality.py): planes fp64 1e-10, fp32 1e-4 of the plane's largest
element; losses fp64 1e-10, fp32 1e-5; the drop-in comparison of two layouts the fp64 trajectory bar of 1e-8.  Everything else is
bit for bit, for a reason in the code: every call goes through ``model_pass``, which launches the general
MODE_MODEL kernels on the tile buffer whatever kernels the descent runs on, and the row, Gram and solve kernels behind it read that
model, the data and the plan scalars, none of which depends on the kernel path; the closed forms minimise the chi-square term alone
and fit quality is unregularised, so neither reads the regulariser; and a call puts the loop state back where it found it."""
import functools

import numpy as np
import pytest

from calamity_amd import batched, calibration, synthetic, uvcompat
from test_gain_basis_solve_host import dpss_basis, restated_basis
from test_gain_time_solve_host import bases_of, flagged_case, rand_basis, restated_time
from test_gpu_coeff_solve import restated as restated_coeffs
from test_gpu_fit_quality import TOL, check_parity, edge_problem, perturbed, plane_err, solver_of
from test_gpu_fit_quality import restated as restated_quality
from test_gpu_fold import mirror_block, small_problem
from test_gpu_gain_solve import restated as restated_gains

pytestmark = pytest.mark.gpu

PATHS = [(np.float32, "general"), (np.float32, "dense"), (np.float32, "dense_split1"), (np.float32, "dense_f32"), (np.float64, "general"),
         (np.float64, "dense")]
DENSE = [pp for pp in PATHS if pp[1] != "general"]
REG_PATHS = [pp for pp in PATHS if pp[1] in ("general", "dense")]
DTYPES = [np.float32, np.float64]
PRIORS = (1.5, -0.5)  # of the "sum" regulariser: the sums of the model's real and imaginary parts it pulls towards


def path_id(pp):
    return f"{np.dtype(pp[0]).name}-{pp[1]}"


def assert_path(s, path):
    got = s.timing_get()["kernel_path"]
    assert got == path, f"asked for the {path} kernels, the solver runs {got}"


def path_solver(p, params, dtype, path, B=None, Bt=None, reg=False):
    """SHARED layout, the kernel path asked for and no other; ``B`` / ``Bt``: a frequency / time gain basis (g0 = the gains, y = 0)."""
    s = solver_of(p, params, dtype, "shared", path)
    if B is not None:
        s.set_gain_basis(B)
    if Bt is not None:
        s.set_gain_time_basis(Bt)
    if reg:
        s.set_regularization("sum", *PRIORS)
    assert_path(s, path)
    return s


def assert_same_bits(got, want, label):
    assert sorted(got) == sorted(want), label
    for k in want:
        if isinstance(want[k], dict) or np.isscalar(want[k]):
            assert got[k] == want[k], (label, k, got[k], want[k])
        else:
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"{label}: {k}")


def check_planes(pairs, dtype, label):
    errs = {k: plane_err(got, want) for k, (got, want) in pairs.items()}
    print(f"{label}: " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, (got, _) in pairs.items():
        assert np.all(np.isfinite(got)), (label, k)
    assert max(errs.values()) <= TOL[np.dtype(dtype)]["plane"], (label, errs)


def check_loss(got, want, dtype, label):
    err = abs(got - want) / want
    print(f"{label}: chi-square {got:.10e}, restatement {want:.10e}: {err:.2e}")
    assert err <= TOL[np.dtype(dtype)]["loss"], (label, err)


# ---- 1. the calls do not depend on the kernels the descent runs on
TIME_LK = {"time_freq": (3, 10), "time": (3, None)}
CASES = [("fit_quality", (7, 200)), ("fit_quality", (12, 129)), ("solve_gains", (7, 200)), ("solve_gains", (12, 129)), ("solve_coeffs", (7, 200)),
         ("solve_coeffs", (12, 129)), ("solve_coeffs_basis", (12, 129)), ("solve_gain_coeffs", (7, 200)), ("solve_gain_coeffs", (12, 129)),
         ("time_freq", (4, 5, 72)), ("time", (4, 5, 72))]
# Three times under three time vectors: Bt is square, so the systems of an antenna flagged at one time have rank 2 and stand on the ridge
# alone (cond(N + ridge) = 2.7e6 against 1.6e2 with four times).  Two correct fp64 factorisations then agree to cond x 1.1e-16 = 3e-10
# only, which says nothing about the kernel at the fp64 bound of 1e-10 (measured 1.4e-10, the same on every path): the shape is
# compared bit for bit between the paths and with the regulariser, where no tolerance enters, and not with the restatement.
BIT_CASES = CASES + [("time", (3, 5, 72))]


def case_ids(cases):
    return [f"{kind}-{'x'.join(map(str, shape))}" for kind, shape in cases]


CASE_IDS = case_ids(CASES)


@functools.lru_cache(maxsize=None)
def inputs(kind, shape):
    """(problem, params, frequency basis or None, time basis or None)."""
    if kind in TIME_LK:
        p, params = flagged_case(*shape)
        Bt, B = bases_of(shape, ("rand",), TIME_LK[kind])
        return p, params, B, Bt
    p, params = edge_problem(*shape)
    return p, params, dpss_basis(p.nfreqs) if kind in ("solve_coeffs_basis", "solve_gain_coeffs") else None, None


@functools.lru_cache(maxsize=None)
def outputs(kind, shape, dtype_name, path, reg=False):
    """One call on a fresh solver: everything it returns and leaves behind, and fit quality and the loss afterwards."""
    dtype = np.dtype(dtype_name).type
    p, params, B, Bt = inputs(kind, shape)
    s = path_solver(p, params, dtype, path, B, Bt, reg)
    out = {}
    if kind == "solve_gains":
        s.solve_gains(2)
    elif kind == "solve_coeffs":
        out["counts"] = s.solve_coeffs()
    elif kind == "solve_coeffs_basis":
        s.solve_gain_coeffs(1)  # y != 0: the gains the solve reads are g0 + B y
        out["y_before_r"], out["y_before_i"] = s.get_gain_coeffs()
        out["counts"] = s.solve_coeffs()
    elif kind == "solve_gain_coeffs":
        out["counts"] = s.solve_gain_coeffs(2)
    elif kind in TIME_LK:
        out["counts"] = s.solve_gain_time_coeffs(2)
    out.update(zip(("g_r", "g_i", "c_r", "c_i"), s.get_params()))
    if B is not None or Bt is not None:
        out["y_r"], out["y_i"] = s.get_gain_coeffs()
    out.update(s.fit_quality())
    out["loss"] = s.eval_loss()
    assert_path(s, path)
    s.close()
    return out


@functools.lru_cache(maxsize=None)
def reference(kind, shape, dtype_name):
    dtype = np.dtype(dtype_name).type
    p, params, B, Bt = inputs(kind, shape)
    if kind == "fit_quality":
        return restated_quality(p, params, dtype)
    if kind == "solve_gains":
        return restated_gains(p, params, dtype, nsweeps=2)
    if kind == "solve_coeffs":
        return restated_coeffs(p, params, dtype)
    if kind == "solve_coeffs_basis":
        return restated_basis(p, params, dtype, B, nsweeps=1)
    if kind == "solve_gain_coeffs":
        return restated_basis(p, params, dtype, B, nsweeps=2)
    return restated_time(p, params, dtype, Bt, B, nsweeps=2)


def planes_of(z, prefix):
    return {f"{prefix}_r": np.ascontiguousarray(z.real), f"{prefix}_i": np.ascontiguousarray(z.imag)}


@pytest.mark.parametrize("dtype,path", PATHS, ids=map(path_id, PATHS))
@pytest.mark.parametrize("kind,shape", CASES, ids=CASE_IDS)
def test_every_call_equals_the_restatement_on_every_path(kind, shape, dtype, path):
    p, params, B, Bt = inputs(kind, shape)
    out = outputs(kind, shape, np.dtype(dtype).name, path)
    ref = reference(kind, shape, np.dtype(dtype).name)
    label = f"{kind} {shape} {path} {np.dtype(dtype).name}"
    start = {k: np.asarray(params[k], dtype=dtype) for k in ("g_r", "g_i", "c_r", "c_i")}
    if kind == "fit_quality":
        check_parity(out, ref, dtype, label)
        want, counts, chisq = {}, None, float(ref["chisq_bl"].sum())
    elif kind == "solve_gains":
        want, counts, chisq = planes_of(ref[0], "g"), None, ref[1][-1]
    elif kind == "solve_coeffs":
        c, chisq, conds, singular = ref
        assert max(conds) <= 1e4 and singular == [0]
        want, counts = planes_of(c, "c"), {"nsolved": p.ngrps - 1, "nsingular": 1}
    elif kind == "solve_coeffs_basis":
        # the sweep against its restatement; the solve against the restatement at the gains the DEVICE holds behind the sweep (as
        # tests/test_gpu_coeff_solve.py does: the fp32 gains of the restated sweep are not the device's to the bit)
        g, y, _, _, nsing = ref
        check_planes({k: (out[k.replace("y_", "y_before_")], v) for k, v in planes_of(y, "y").items()}, dtype, label + " sweep")
        c, chisq, conds, singular = restated_coeffs(p, params, dtype, gains=(out["g_r"], out["g_i"]))
        assert max(conds) <= 1e4 and singular == [0] and nsing == 1
        want, counts = dict(planes_of(c, "c"), **planes_of(g, "g")), {"nsolved": p.ngrps - 1, "nsingular": 1}
        np.testing.assert_array_equal(out["y_r"], out["y_before_r"])  # the solve writes neither y nor the gains
        np.testing.assert_array_equal(out["y_i"], out["y_before_i"])
    else:
        g, y, chis, _, nsing = ref
        nsys = p.nants if kind == "solve_gain_coeffs" else (p.nants // Bt.shape[0]) * (1 if B is not None else p.nfreqs)
        want, counts, chisq = dict(planes_of(g, "g"), **planes_of(y, "y")), {"nsolved": nsys - nsing, "nsingular": nsing}, chis[-1]
        assert nsing == {"solve_gain_coeffs": 1, "time_freq": 1, "time": p.nfreqs + 1}[kind]
    if want:
        check_planes({k: (out[k], v) for k, v in want.items()}, dtype, label)
    assert out.get("counts") == counts, (label, out.get("counts"), counts)
    check_loss(out["loss"], chisq, dtype, label)
    check_loss(float(out["chisq_bl"].sum()), chisq, dtype, label + " (fit quality afterwards)")
    for k in ("g_r", "g_i", "c_r", "c_i"):  # what the call does not solve keeps its bits
        if k not in want:
            np.testing.assert_array_equal(out[k], start[k], err_msg=f"{label}: {k}")
        else:
            assert np.any(out[k] != start[k]), (label, k)


@pytest.mark.parametrize("dtype,path", DENSE, ids=map(path_id, DENSE))
@pytest.mark.parametrize("kind,shape", BIT_CASES, ids=case_ids(BIT_CASES))
def test_every_call_gives_the_bits_of_the_general_path(kind, shape, dtype, path):
    """The model pass (general MODE_MODEL kernels on the shared tiles), the row kernels and the solve kernels read the same tile buffer
    and plan scalars whatever kernels the descent runs on.  ``eval_loss`` afterwards is no output of the call: it is the loss pass of the
    path's OWN kernels (``enqueue_pass``), and the dense kernels sum the chi-square on the matrix cores in another order than the general
    ones (by design: tests/test_gpu_fp32_families.py bounds every family against the oracle).  It is held to the loss tolerance."""
    name = np.dtype(dtype).name
    got, want = dict(outputs(kind, shape, name, path)), dict(outputs(kind, shape, name, "general"))
    loss, loss_general = got.pop("loss"), want.pop("loss")
    assert_same_bits(got, want, f"{kind} {shape} {path} {name}")
    err = abs(loss - loss_general) / loss_general
    print(f"{kind} {shape} {path} {name}: eval_loss {loss:.17e}, on the general path {loss_general:.17e}: {err:.2e}")
    assert err <= TOL[np.dtype(dtype)]["loss"]


@pytest.mark.parametrize("dtype,path", REG_PATHS, ids=map(path_id, REG_PATHS))
@pytest.mark.parametrize("kind,shape", BIT_CASES, ids=case_ids(BIT_CASES))
def test_the_sum_regulariser_changes_no_bit_of_any_call(kind, shape, dtype, path):
    """The closed forms minimise the chi-square term and fit quality is unregularised (DESIGN.md sections 3.8 to 3.12).  ``eval_loss``
    is the one output that is DEFINED with the regulariser: its term (the squared distances of the model's sums from the priors) is
    added on top of the same chi-square, so it is compared with the fit-quality sum instead of bit for bit."""
    name = np.dtype(dtype).name
    with_reg, without = dict(outputs(kind, shape, name, path, True)), dict(outputs(kind, shape, name, path))
    loss_reg, loss = with_reg.pop("loss"), without.pop("loss")
    assert_same_bits(with_reg, without, f"{kind} {shape} {path} {name} with the regulariser")
    assert loss_reg > loss  # (the priors are far from the model's sums: the regulariser is on)
    check_loss(float(with_reg["chisq_bl"].sum()), loss, dtype, f"{kind} {shape} {path} {name}: fit quality under the regulariser")


# ---- several slices
@functools.lru_cache(maxsize=None)
def three_slices():
    T = 3
    parts = [synthetic.make_problem(7, 200, f0=150e6, df=400e3, seed=21, data_seed=30 + t) for t in range(T)]
    p0 = parts[0][0]
    data = tuple(np.concatenate([getattr(parts[t][0], k) for t in range(T)]) for k in ("data_r", "data_i", "wgts"))
    pars = [perturbed(parts[t][0], parts[t][2], seed=40 + t) for t in range(T)]
    start = {k: np.concatenate([pars[t][k] for t in range(T)]) for k in ("g_r", "g_i", "c_r", "c_i")}
    sub, _, _ = batched.replicate_slices(p0, T)
    return p0, sub, data, start


SLICE_CALLS = {"solve_gains": lambda s, mask: s.solve_gains(2, slice_mask=mask), "solve_coeffs": lambda s, mask: s.solve_coeffs(slice_mask=mask),
               "solve_gain_coeffs": lambda s, mask: s.solve_gain_coeffs(2, slice_mask=mask)}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mask", [[1, 0, 1], [0, 1, 1]])
@pytest.mark.parametrize("call", list(SLICE_CALLS))
def test_a_masked_slice_keeps_its_bits_and_the_others_equal_the_general_solver(call, mask, dtype):
    from calamity_amd.solver import HipFitSolver

    p0, sub, data, start = three_slices()
    basis = call == "solve_gain_coeffs"
    got = {}
    for path in ("dense", "general"):
        s = HipFitSolver(dtype=dtype)
        s.set_problem(sub, layout="shared", kernel_path=path)
        s.set_data(*data)
        s.set_params(start["g_r"], start["g_i"], start["c_r"], start["c_i"])
        if basis:
            s.set_gain_basis(dpss_basis(p0.nfreqs))
            s.solve_gain_coeffs(1)  # y != 0 in every slice before the masked call
        assert_path(s, path)
        before = list(s.get_params()) + (list(s.get_gain_coeffs()) if basis else [])
        counts = SLICE_CALLS[call](s, mask)
        after = list(s.get_params()) + (list(s.get_gain_coeffs()) if basis else [])
        s.close()
        na, nc = p0.nants, p0.ncoeffs
        moved = {"solve_gains": (0, 1), "solve_coeffs": (2, 3), "solve_gain_coeffs": (0, 1, 4, 5)}[call]
        for t in range(3):
            for k, (new, old) in enumerate(zip(after, before)):
                part = slice(t * nc, (t + 1) * nc) if k in (2, 3) else slice(t * na, (t + 1) * na)
                if mask[t] and k in moved:
                    assert not np.array_equal(new[part], old[part]), (path, t, k)
                else:
                    np.testing.assert_array_equal(new[part], old[part], err_msg=f"{path}: plane {k} of slice {t}")
        if call == "solve_coeffs":
            assert counts == {"nsolved": sum(mask) * p0.ngrps, "nsingular": 0}
        if call == "solve_gain_coeffs":
            assert counts == {"nsolved": sum(mask) * na, "nsingular": 0}
        got[path] = (after, counts)
    assert got["dense"][1] == got["general"][1]
    for k, (a, b) in enumerate(zip(got["dense"][0], got["general"][0])):
        np.testing.assert_array_equal(a, b, err_msg=f"plane {k}")


# ---- 2. a descent continued through a call, on the dense paths
NSTEPS = 256  # from here on a run of the dense path replays a hipGraph in the default launch mode
REGS = [False, True]
REG_IDS = ["chisq", "sum_reg"]


@functools.lru_cache(maxsize=None)
def descent_inputs(kind):
    if kind == "time":
        shape = (4, 5, 72)
        p, params = flagged_case(*shape)
        Bt, B = bases_of(shape, ("rand",), (3, 10))
        return p, params, B, Bt
    p, params = edge_problem(12, 129)
    return p, params, dpss_basis(p.nfreqs) if kind == "basis" else None, None


def descent_solver(kind, dtype, path, reg, mode="auto"):
    p, params, B, Bt = descent_inputs(kind)
    s = path_solver(p, params, dtype, path, B, Bt, reg)
    s.set_launch_mode(mode)
    s.set_optimizer("Adam", learning_rate=1e-2)
    return s


def full_state(s, kind):
    """Parameters, y where there is a basis, and the optimizer's slots."""
    out = dict(zip(("g_r", "g_i", "c_r", "c_i"), s.get_params()))
    if kind != "free":
        out["y_r"], out["y_i"] = s.get_gain_coeffs()
    out.update(s.get_moments() if kind == "free" else s.get_gain_coeff_moments())
    return out


def assert_same_state(got, want, label):
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{label}: {k}")


NULL_CALLS = {"fit_quality": ("free", lambda s: s.fit_quality()), "solve_gains": ("free", lambda s: s.solve_gains(3, slice_mask=[0])),
              "solve_coeffs": ("free", lambda s: s.solve_coeffs(slice_mask=[0])),
              "solve_gain_coeffs": ("basis", lambda s: s.solve_gain_coeffs(2, slice_mask=[0]))}


@functools.lru_cache(maxsize=None)
def two_runs(kind, dtype_name, path, reg, call=None):
    s = descent_solver(kind, np.dtype(dtype_name).type, path, reg)
    first = s.run(NSTEPS, tol=0.0)[0]
    if call is not None:
        NULL_CALLS[call][1](s)
    second = s.run(NSTEPS, tol=0.0)[0]
    state = full_state(s, kind)
    assert_path(s, path)
    s.close()
    losses = np.concatenate([first, second])
    assert len(losses) == 2 * NSTEPS and np.all(np.isfinite(losses))
    return losses, state


@pytest.mark.parametrize("reg", REGS, ids=REG_IDS)
@pytest.mark.parametrize("dtype,path", DENSE, ids=map(path_id, DENSE))
@pytest.mark.parametrize("call", list(NULL_CALLS))
def test_a_call_that_selects_nothing_changes_nothing_of_a_replayed_descent(call, dtype, path, reg):
    """run(256), call, run(256) in the default launch mode (both runs replay a graph) against run(256), run(256): the call overwrites
    the device loop state for its model pass and puts it back."""
    kind = NULL_CALLS[call][0]
    name = np.dtype(dtype).name
    losses, state = two_runs(kind, name, path, reg, call)
    plain_losses, plain_state = two_runs(kind, name, path, reg)
    np.testing.assert_array_equal(losses, plain_losses)
    assert_same_state(state, plain_state, f"{call} {path} {name}")
    assert losses[-1] < losses[0]


REAL_CALLS = {"fit_quality": ("free", lambda s: s.fit_quality()), "solve_gains": ("free", lambda s: s.solve_gains(3, reset_gain_moments=True)),
              "solve_coeffs": ("free", lambda s: s.solve_coeffs(reset_coeff_moments=True)),
              "solve_gain_coeffs": ("basis", lambda s: s.solve_gain_coeffs(2, reset_gain_moments=True)),
              "solve_gain_time_coeffs": ("time", lambda s: s.solve_gain_time_coeffs(2, reset_gain_moments=True))}


@pytest.mark.parametrize("reg", REGS, ids=REG_IDS)
@pytest.mark.parametrize("dtype,path", DENSE, ids=map(path_id, DENSE))
@pytest.mark.parametrize("call", list(REAL_CALLS))
def test_graph_replay_equals_single_launches_across_a_real_call(call, dtype, path, reg):
    kind, fn = REAL_CALLS[call]
    losses, final = {}, {}
    for mode in ("kernels", "auto"):
        s = descent_solver(kind, dtype, path, reg, mode)
        first = s.run(NSTEPS, tol=0.0)[0]
        before = s.get_params()
        fn(s)
        at_call = s.eval_loss()
        after = s.get_params()
        second = s.run(NSTEPS, tol=0.0)[0]
        assert len(first) == len(second) == NSTEPS
        err = abs(second[0] - at_call) / at_call
        print(f"{call} {path} {np.dtype(dtype).name} {mode}: first loss behind the call {second[0]:.10e}, eval_loss {at_call:.10e}: {err:.2e}")
        assert err <= TOL[np.dtype(dtype)]["loss"]
        if call != "fit_quality":
            assert any(not np.array_equal(a, b) for a, b in zip(after, before))  # a real call: something moved
        losses[mode] = np.concatenate([first, second])
        final[mode] = full_state(s, kind)
        assert_path(s, path)
        s.close()
    assert np.all(np.isfinite(losses["auto"]))
    np.testing.assert_array_equal(losses["auto"], losses["kernels"])
    assert_same_state(final["auto"], final["kernels"], f"{call} {path} {np.dtype(dtype).name}")


RESUME_CALLS = {"solve_gains": lambda s, reset: s.solve_gains(3, reset_gain_moments=reset),
                "solve_coeffs": lambda s, reset: s.solve_coeffs(reset_coeff_moments=reset)}


@pytest.mark.parametrize("reset", [False, True], ids=["slots_kept", "slots_reset"])
@pytest.mark.parametrize("reg", REGS, ids=REG_IDS)
@pytest.mark.parametrize("dtype,path", DENSE, ids=map(path_id, DENSE))
@pytest.mark.parametrize("call", list(RESUME_CALLS))
def test_nothing_stale_is_left_behind_a_call(call, dtype, path, reg, reset):
    """run(40), call; a fresh solver given the parameters and the slots read behind the call takes the same next 40 steps."""
    s = descent_solver("free", dtype, path, reg)
    s.run(40, tol=0.0)
    RESUME_CALLS[call](s, reset)
    params, moments = s.get_params(), s.get_moments()
    want_losses, want = s.run(40, tol=0.0)[0], s.get_params()
    s.close()
    p, start = descent_inputs("free")[:2]
    fresh = path_solver(p, start, dtype, path, reg=reg)
    fresh.set_params(*params)
    fresh.set_optimizer("Adam", learning_rate=1e-2)
    t = moments.pop("t")
    assert t == 40
    fresh.set_moments(**moments, t=t)
    got_losses, got = fresh.run(40, tol=0.0)[0], fresh.get_params()
    assert_path(fresh, path)
    fresh.close()
    assert len(want_losses) == 40
    np.testing.assert_array_equal(got_losses, want_losses)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)


# ---- 3. the exact-zero pivot
def zero_column(basis, col):
    """The setters check only that a basis is finite.  A zero column makes that column's diagonal element of every system, and every
    contribution to its pivot, exactly zero -- on the device as in NumPy."""
    out = np.array(basis)
    out[:, col] = 0.0
    return out


# (T, Na, F), (L, K), the basis with the zero column, the column.  A zero pivot part-way through a factorisation, and one at the LAST
# column: there no later pivot (not finite behind a division by a zero root) can stand in for the test of the pivot itself.  In a system
# over (l, k) only L = 1 with the last column of B zeroed puts the one zero pivot last.  gain_basis_chol_kernel at L > 1 in LDS (n = 30, 10) and
# in scratch (n = 128); gain_time_chan_kernel in registers (L = 3) and in scratch (L = 9)
ZERO_TIME = [((4, 5, 48), (3, 10), "Bt", 1), ((9, 4, 72), (8, 16), "Bt", 3), ((3, 5, 72), (1, 10), "B", 9), ((2, 4, 200), (1, 128), "B", 127),
             ((4, 5, 48), (3, None), "Bt", 1), ((4, 5, 48), (3, None), "Bt", 2), ((10, 5, 72), (9, None), "Bt", 4), ((10, 5, 72), (9, None), "Bt", 8)]


def state_of(s):
    return s.get_params()[:2] + s.get_gain_coeffs()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,LK,which,col", ZERO_TIME, ids=[f"{'x'.join(map(str, s))}-L{lk[0]}-K{lk[1]}-{w}{c}" for s, lk, w, c in ZERO_TIME])
def test_a_zero_column_of_the_time_or_frequency_basis_of_a_joint_fit(shape, LK, which, col, dtype):
    T, na, F = shape
    p, params = flagged_case(*shape)
    Bt, B = bases_of(shape, ("rand",), LK)
    if which == "Bt":
        Bt = zero_column(Bt, col)
    else:
        B = zero_column(B, col)
    nsys = na if B is not None else na * F
    label = f"{shape} L, K = {LK} zero column {col} of {which} {np.dtype(dtype).name}"
    # without ridge every system meets the zero pivot: nothing moves
    assert restated_time(p, params, dtype, Bt, B, ridge=0.0)[4] == nsys
    s = path_solver(p, params, dtype, "general", B, Bt)
    before = state_of(s)
    assert s.solve_gain_time_coeffs(1, ridge=0.0) == {"nsolved": 0, "nsingular": nsys}, label
    for a, b in zip(state_of(s), before):
        np.testing.assert_array_equal(a, b)
    # with it the rest are solved and the zero column's y stays exactly zero; the usual systems stay singular: the antenna without data
    # and, without a frequency basis, channel 3 of antenna 1
    want_g, want_y, chisq, _, nsing = restated_time(p, params, dtype, Bt, B, ridge=1e-6)
    assert nsing == (1 if B is not None else F + 1)
    assert s.solve_gain_time_coeffs(1, ridge=1e-6) == {"nsolved": nsys - nsing, "nsingular": nsing}, label
    g_r, g_i, y_r, y_i = state_of(s)
    check_planes(dict(g_r=(g_r, want_g.real), g_i=(g_i, want_g.imag), y_r=(y_r, want_y.real), y_i=(y_i, want_y.imag)), dtype, label)
    check_loss(s.eval_loss(), chisq[-1], dtype, label)
    zero = (slice(None), col) if which == "Bt" else (slice(None), slice(None), col)
    assert not np.any(y_r[zero]) and not np.any(y_i[zero]) and np.any(y_r)
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("col", [5, 11], ids=["part_way", "last"])
def test_a_zero_column_of_the_frequency_basis(col, dtype):
    """gain_basis_chol_kernel at K = 12: the pivot of the zero column is exactly zero in every antenna row."""
    p, params = edge_problem(7, 200)
    B = zero_column(rand_basis(200, 12, 3), col)
    label = f"(7, 200) K = 12 zero column {col} {np.dtype(dtype).name}"
    assert restated_basis(p, params, dtype, B, ridge=0.0)[4] == p.nants
    s = path_solver(p, params, dtype, "general", B)
    before = state_of(s)
    assert s.solve_gain_coeffs(1, ridge=0.0) == {"nsolved": 0, "nsingular": p.nants}, label
    for a, b in zip(state_of(s), before):
        np.testing.assert_array_equal(a, b)
    want_g, want_y, chisq, _, nsing = restated_basis(p, params, dtype, B, ridge=1e-6)
    assert nsing == 1
    assert s.solve_gain_coeffs(1, ridge=1e-6) == {"nsolved": p.nants - 1, "nsingular": 1}, label
    g_r, g_i, y_r, y_i = state_of(s)
    check_planes(dict(g_r=(g_r, want_g.real), g_i=(g_i, want_g.imag), y_r=(y_r, want_y.real), y_i=(y_i, want_y.imag)), dtype, label)
    check_loss(s.eval_loss(), chisq[-1], dtype, label)
    assert not np.any(y_r[:, col]) and not np.any(y_i[:, col]) and np.any(y_r)
    s.close()


@functools.lru_cache(maxsize=None)
def zero_vector_problems(vec):
    """Two blocks of 15 and 31 vectors on 256 channels, eight groups; the second problem has vector ``vec`` of block 1 zeroed."""
    rng = np.random.default_rng(286)
    blocks = [mirror_block(rng, 256, n) for n in (15, 31)]
    zeroed = [blocks[0], zero_column(blocks[1], vec)]
    full, start = small_problem(blocks, [0, 1, 0, 1] * 2, seed=287)
    holed, start_again = small_problem(zeroed, [0, 1, 0, 1] * 2, seed=287)
    assert all(np.array_equal(start[k], start_again[k]) for k in start) and np.array_equal(full.data_r, holed.data_r)
    return full, holed, start


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("vec", [7, 30], ids=["part_way", "last"])
def test_a_zero_vector_of_a_foreground_block(vec, dtype):
    """coeff_chol_kernel: without ridge the groups on the block with the zero vector keep their bits and count as singular while the
    others are solved (a group's system holds its own block alone, so their restatement is that of the problem without the hole);
    with the ridge all are solved and the zero vector's coefficient keeps its bits."""
    full, holed, start = zero_vector_problems(vec)
    coff, on_hole = holed.grp_coff, np.where(holed.grp_basis == 1)[0]
    hole = np.asarray([coff[g] + vec for g in on_hole])
    rest = np.concatenate([np.arange(coff[g], coff[g + 1]) for g in range(holed.ngrps) if holed.grp_basis[g] == 0])
    label = f"zero vector {vec} {np.dtype(dtype).name}"
    want, _, conds, singular = restated_coeffs(full, start, dtype, ridge=0.0)
    assert max(conds) <= 1e4 and not singular
    s = path_solver(holed, start, dtype, "general")
    before = s.get_params()
    assert s.solve_coeffs(ridge=0.0) == {"nsolved": holed.ngrps - len(on_hole), "nsingular": len(on_hole)}, label
    after = s.get_params()
    for g in on_hole:
        for k in (2, 3):
            np.testing.assert_array_equal(after[k][coff[g] : coff[g + 1]], before[k][coff[g] : coff[g + 1]], err_msg=f"group {g}")
    check_planes(dict(c_r=(after[2][rest], want.real[rest]), c_i=(after[3][rest], want.imag[rest])), dtype, label + " ridge 0")
    assert np.all(after[2][rest] != before[2][rest])
    s.close()
    want, chisq, _, singular = restated_coeffs(holed, start, dtype, ridge=1e-6)
    assert not singular
    s = path_solver(holed, start, dtype, "general")
    assert s.solve_coeffs(ridge=1e-6) == {"nsolved": holed.ngrps, "nsingular": 0}, label
    after = s.get_params()
    check_planes(dict(c_r=(after[2], want.real), c_i=(after[3], want.imag)), dtype, label + " ridge 1e-6")
    check_loss(s.eval_loss(), chisq, dtype, label)
    for k in (2, 3):
        np.testing.assert_array_equal(after[k][hole], before[k][hole])
    others = np.setdiff1d(np.arange(holed.ncoeffs), hole)
    assert np.all(after[2][others] != before[2][others])
    s.close()


# ---- 5. one drop-in call that really reaches the dense path
@functools.lru_cache(maxsize=None)
def array_of_65():
    """65 antennas are 2080 baselines: the smallest array for which "auto" picks the dense kernels (from 2048 baselines)."""
    return synthetic.make_uvdata(nants=65, nfreqs=72)[0]


def test_one_drop_in_fit_on_the_dense_path_equals_the_streaming_layout(monkeypatch):
    """fp64, 10 steps with a coefficient solve and two gain sweeps before them, a sweep every 5 steps and fit quality behind them:
    the SHARED layout (dense kernels) against the STREAM layout (which has no dense path), at the fp64 trajectory bar of 1e-8."""
    uvd = array_of_65()
    assert uvd.Nbls >= 2048
    used = []
    real = calibration.get_solver

    def spy(*args, **kwargs):
        s = real(*args, **kwargs)
        if all(s is not u for u in used):
            used.append(s)
        return s

    monkeypatch.setattr(calibration, "get_solver", spy)
    kw = dict(uvdata=uvd, gains=None, dtype=np.float64, maxsteps=10, coeff_solve_rounds=1, gain_solve_sweeps=2, gain_solve_every=5, fit_quality=True,
              batch_slices=False, min_dly=2.0 / 0.3, offset=2.0 / 0.3)
    out, paths = {}, {}
    for layout in ("shared", "stream"):
        del used[:]
        out[layout] = calibration.calibrate_and_model_dpss(layout=layout, **kw)
        paths[layout] = [s.timing_get()["kernel_path"] for s in used]
    assert paths["shared"] and set(paths["shared"]) == {"dense"}, paths
    assert paths["stream"] and set(paths["stream"]) == {"general"}, paths
    a, b = out["shared"], out["stream"]
    ha, hb = a[3][0][0], b[3][0][0]
    la, lb = np.asarray(ha["loss"], dtype=np.float64), np.asarray(hb["loss"], dtype=np.float64)
    assert len(la) == len(lb) == 10
    errs = dict(loss=float(np.max(np.abs(la - lb) / np.abs(lb))), gains=plane_err(np.asarray(a[2].gain_array), np.asarray(b[2].gain_array)),
                quality=plane_err(uvcompat.gain4(a[2].quality_array), uvcompat.gain4(b[2].quality_array)),
                total_quality=plane_err(np.asarray(a[2].total_quality_array), np.asarray(b[2].total_quality_array)))
    assert sorted(ha["chisq_per_baseline"]) == sorted(hb["chisq_per_baseline"]) and len(ha["chisq_per_baseline"]) == uvd.Nbls
    keys = sorted(ha["chisq_per_baseline"])
    errs["chisq_per_baseline"] = plane_err(np.asarray([ha["chisq_per_baseline"][k] for k in keys]), np.asarray([hb["chisq_per_baseline"][k] for k in keys]))
    print("shared (dense) against stream: " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert np.any(uvcompat.gain4(a[2].quality_array) > 0)
    assert max(errs.values()) <= 1e-8, errs
    assert ha["coeff_solve_singular"] == hb["coeff_solve_singular"]
