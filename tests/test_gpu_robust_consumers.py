"""Every reader of the weight plane behind a ``robust_weights`` call (include/calamity_hip.h promises that fit quality, the four
closed-form solves and every kernel path read the plane the call rewrites in place; tests/test_gpu_robust_weights.py checks the loss,
tests/test_gpu_solve_paths.py never reweights).

Solver A calls ``robust_weights`` and then a reader; solver B is a fresh solver given A's weights through ``set_data`` and calls the
same reader.  B has never seen ``w0``, so a reader of A that took anything from the plane of ``w0``, from a copy made before the call
or from a stale cache differs from B.  Everything is compared bit for bit: both solvers hold the same planes and run the same kernels.
The solvers, shapes and kernel paths are those of tests/test_gpu_solve_paths.py (``path_solver`` asserts the path it asked for):
shapes (7, 200) and (12, 129), the joint time-and-frequency case (4, 5, 72); fp32 ``general`` / ``dense`` / ``dense_split1`` /
``dense_f32``, fp64 ``general`` / ``dense``.  The reweight is ``clip`` at k = 2 (weights become zero where ``w0`` has none; ``init_coeffs``
reads the weights as a mask only) and Huber at k = 2 once.

On ``general`` and ``dense`` the readers are also held to their fp64 NumPy restatements evaluated on a copy of the problem whose
weights are A's, at ``TOL`` of tests/test_gpu_fit_quality.py.  That comparison could pass for a reader of ``w0`` if the new weights
changed little, so each test first asserts that the restatement under the new weights differs from the one under ``w0`` by more than
100 x ``TOL`` in every plane and in the chi-square (the planes differ by 6.6e-2 and more of their largest element, the bound being 1e-2
in fp32, and the chi-square by 47 % and more; 11 to 15 % of the samples are clipped at the 10 % perturbation of ``edge_problem``)."""
import copy

import numpy as np
import pytest

from test_gpu_fit_quality import TOL, check_parity, plane_err
from test_gpu_solve_paths import (DTYPES, PATHS, REG_PATHS, assert_path, assert_same_bits, check_loss, check_planes, inputs, path_id, path_solver,
                                  planes_of, restated_basis, restated_coeffs, restated_gains, restated_quality, restated_time, three_slices)

pytestmark = pytest.mark.gpu

CLIP = ("clip", 2.0)
HUBER = ("huber", 2.0)
SHAPES = [(7, 200), (12, 129)]
SOLVES = ["fit_quality", "solve_gains", "solve_coeffs", "solve_gain_coeffs"]
READERS = SOLVES + ["init_coeffs", "eval"]
CASES = [(kind, shape, CLIP) for kind in READERS for shape in SHAPES] + [("time_freq", (4, 5, 72), CLIP), ("fit_quality", (7, 200), HUBER)]
RESTATED = [(kind, shape) for kind in SOLVES for shape in SHAPES] + [("time_freq", (4, 5, 72))]
INPUTS_OF = {"init_coeffs": "fit_quality", "eval": "fit_quality"}  # (neither takes a gain basis)


def case_id(case):
    return f"{case[0]}-{'x'.join(map(str, case[1]))}" + (f"-{case[2][0]}" if len(case) > 2 else "")


def inputs_of(kind, shape):
    return inputs(INPUTS_OF.get(kind, kind), shape)


def reweighted(kind, shape, dtype, path, how=CLIP, given=None):
    """Solver A behind its ``robust_weights`` call: (solver, the weights it holds now, w0).  ``given``: (problem, params, frequency
    basis or None, time basis or None) of a caller with inputs of its own, in place of ``inputs_of(kind, shape)``."""
    p, params, B, Bt = given if given is not None else inputs_of(kind, shape)
    s = path_solver(p, params, dtype, path, B, Bt)
    w0 = s.get_weights()
    np.testing.assert_array_equal(w0, np.asarray(p.wgts).astype(dtype))
    out = s.robust_weights(*how)
    w = s.get_weights()
    assert out["ndown_bl"].sum() > 0 and np.any(w < w0) and not np.any(w > w0)
    if how[0] == "clip":
        assert out["ndown_bl"].sum() == np.sum((w == 0) & (w0 > 0))  # zeros where w0 has none
    else:
        assert not np.any((w == 0) & (w0 > 0))
    np.testing.assert_array_equal(s.get_weights(1), w0)
    return s, w, w0


def uploaded(kind, shape, dtype, path, w, given=None):
    """Solver B: a fresh solver that is given the weights ``w`` through ``set_data`` and never reweights (``given`` as above)."""
    p, params, B, Bt = given if given is not None else inputs_of(kind, shape)
    s = path_solver(p, params, dtype, path, B, Bt)
    s.set_data(p.data_r, p.data_i, w)
    np.testing.assert_array_equal(s.get_weights(), w)
    return s


def read(s, kind, shape):
    """One reader of the weight plane: what it returns and leaves behind, then fit quality and the loss."""
    p, _, B, Bt = inputs_of(kind, shape)
    out = {}
    if kind == "fit_quality":
        out.update({f"first_{k}": v for k, v in s.fit_quality().items()})
    elif kind == "solve_gains":
        s.solve_gains(2)
    elif kind == "solve_coeffs":
        out["counts"] = s.solve_coeffs()
    elif kind == "solve_gain_coeffs":
        out["counts"] = s.solve_gain_coeffs(2)
    elif kind == "time_freq":
        out["counts"] = s.solve_gain_time_coeffs(2)
    elif kind == "init_coeffs":
        s.init_coeffs(p.data_r, p.data_i)
    elif kind == "eval":
        out["eval_loss"] = s.eval_loss()
        out.update(zip(("grad_loss", "gg_r", "gg_i", "gc_r", "gc_i"), s.eval_grads()))
    out.update(zip(("g_r", "g_i", "c_r", "c_i"), s.get_params()))
    if B is not None or Bt is not None:
        out["y_r"], out["y_i"] = s.get_gain_coeffs()
    out.update(s.fit_quality())
    out["loss"] = s.eval_loss()
    return out


@pytest.mark.parametrize("dtype,path", PATHS, ids=map(path_id, PATHS))
@pytest.mark.parametrize("case", CASES, ids=map(case_id, CASES))
def test_a_reader_behind_the_call_equals_a_fresh_solver_given_the_same_weights(case, dtype, path):
    kind, shape, how = case
    a, w, _ = reweighted(kind, shape, dtype, path, how)
    b = uploaded(kind, shape, dtype, path, w)
    got, want = read(a, kind, shape), read(b, kind, shape)
    for s in (a, b):
        assert_path(s, path)
        s.close()
    assert np.all(np.isfinite(got["chisq_bl"])) and got["loss"] > 0
    assert_same_bits(got, want, f"{kind} {shape} {path} {np.dtype(dtype).name} behind {how[0]}")
    moved = {"solve_gains": "g_r", "solve_coeffs": "c_r", "solve_gain_coeffs": "g_r", "time_freq": "g_r", "init_coeffs": "c_r"}.get(kind)
    assert moved is None or np.any(got[moved] != np.asarray(inputs_of(kind, shape)[1][moved], dtype=dtype))  # a real call: something moved


def restatement(kind, p, params, dtype, B, Bt):
    """(planes, chi-square afterwards, counts) of one reader in fp64 NumPy on the inputs a solver of ``dtype`` holds."""
    if kind == "fit_quality":
        ref = restated_quality(p, params, dtype)
        return {k: ref[k] for k in ("chisq_ant", "wsum_ant", "chisq_bl", "wsum_bl")}, float(ref["chisq_bl"].sum()), None
    if kind == "solve_gains":
        g, chis, _ = restated_gains(p, params, dtype, nsweeps=2)
        return planes_of(g, "g"), chis[-1], None
    if kind == "solve_coeffs":
        c, chisq, conds, singular = restated_coeffs(p, params, dtype)
        assert max(conds) <= 1e4
        return planes_of(c, "c"), chisq, {"nsolved": p.ngrps - len(singular), "nsingular": len(singular)}
    if kind == "solve_gain_coeffs":
        g, y, chis, _, nsing = restated_basis(p, params, dtype, B, nsweeps=2)
        return dict(planes_of(g, "g"), **planes_of(y, "y")), chis[-1], {"nsolved": p.nants - nsing, "nsingular": nsing}
    g, y, chis, _, nsing = restated_time(p, params, dtype, Bt, B, nsweeps=2)
    nsys = p.nants // Bt.shape[0]
    return dict(planes_of(g, "g"), **planes_of(y, "y")), chis[-1], {"nsolved": nsys - nsing, "nsingular": nsing}


def assert_the_weights_matter(new, old, dtype, label):
    """The restatement under the new weights against the one under w0: more than 100 x TOL apart, or reading w0 would pass."""
    tol = TOL[np.dtype(dtype)]
    moved = {k: plane_err(new[0][k], old[0][k]) for k in new[0]}
    loss = abs(new[1] - old[1]) / old[1]
    print(f"{label}: the new weights move the restatement by " + "  ".join(f"{k} {v:.1e}" for k, v in moved.items()) + f"  chi-square {loss:.1e}")
    assert min(moved.values()) > 100 * tol["plane"] and loss > 100 * tol["loss"], (label, moved, loss)


@pytest.mark.parametrize("dtype,path", REG_PATHS, ids=map(path_id, REG_PATHS))
@pytest.mark.parametrize("kind,shape", RESTATED, ids=map(case_id, RESTATED))
def test_a_reader_behind_the_call_equals_its_restatement_under_the_new_weights(kind, shape, dtype, path):
    p, params, B, Bt = inputs_of(kind, shape)
    label = f"{kind} {shape} {path} {np.dtype(dtype).name}"
    a, w, w0 = reweighted(kind, shape, dtype, path)
    p_new = copy.copy(p)
    p_new.wgts = w.astype(np.float64)
    new, old = restatement(kind, p_new, params, dtype, B, Bt), restatement(kind, p, params, dtype, B, Bt)
    assert_the_weights_matter(new, old, dtype, label)
    got = read(a, kind, shape)
    assert_path(a, path)
    a.close()
    planes, chisq, counts = new
    if kind == "fit_quality":
        check_parity({k: got[f"first_{k}"] for k in planes}, planes, dtype, label)
    else:
        check_planes({k: (got[k], v) for k, v in planes.items()}, dtype, label)
    assert got.get("counts") == counts, (label, got.get("counts"), counts)
    check_loss(got["loss"], chisq, dtype, label)
    check_loss(float(got["chisq_bl"].sum()), chisq, dtype, label + " (fit quality afterwards)")
    want_wsum = w.astype(np.float64).sum(axis=1)
    assert np.max(np.abs(got["wsum_bl"] - want_wsum)) <= TOL[np.dtype(dtype)]["loss"] * np.max(want_wsum), label
    assert np.max(np.abs(want_wsum - w0.astype(np.float64).sum(axis=1))) > 100 * TOL[np.dtype(dtype)]["loss"] * np.max(want_wsum)


# ---- three slices, the middle one reweighted
def slice_solver(dtype, path, wgts=None):
    from calamity_amd.solver import HipFitSolver

    p0, sub, data, start = three_slices()
    s = HipFitSolver(dtype=dtype)
    s.set_problem(sub, layout="shared", kernel_path=path)
    s.set_data(data[0], data[1], data[2] if wgts is None else wgts)
    s.set_params(start["g_r"], start["g_i"], start["c_r"], start["c_i"])
    assert_path(s, path)
    return s


SLICE_READERS = {"solve_gains": (lambda s: s.solve_gains(2), (0, 1)), "solve_coeffs": (lambda s: s.solve_coeffs(), (2, 3))}


@pytest.mark.parametrize("dtype,path", REG_PATHS, ids=map(path_id, REG_PATHS))
@pytest.mark.parametrize("call", list(SLICE_READERS))
def test_three_slices_with_the_middle_one_reweighted(call, dtype, path):
    """Mask [0, 1, 0], then the reader over all slices: equal to a solver uploaded with the mixed plane; the outer slices equal to a
    solver that never reweighted, the middle one not."""
    p0 = three_slices()[0]
    nb, na, nc = p0.nbls, p0.nants, p0.ncoeffs
    fn, planes = SLICE_READERS[call]
    a = slice_solver(dtype, path)
    w_in = a.get_weights()
    out = a.robust_weights(*CLIP, slice_mask=[0, 1, 0])
    w = a.get_weights()
    mid = slice(nb, 2 * nb)
    assert out["ndown_bl"][mid].sum() > 0 and np.any((w[mid] == 0) & (w_in[mid] > 0))
    for rows in (slice(0, nb), slice(2 * nb, 3 * nb)):
        np.testing.assert_array_equal(w[rows], w_in[rows])
        assert not np.any(out["ndown_bl"][rows]) and not np.any(out["scale_bl"][rows])
    b, c = slice_solver(dtype, path, wgts=w), slice_solver(dtype, path)
    results = []
    for s in (a, b, c):
        counts = fn(s)
        results.append((counts, s.get_params(), s.fit_quality(), s.eval_loss()))
        assert_path(s, path)
        s.close()
    (counts_a, par_a, q_a, loss_a), (counts_b, par_b, q_b, loss_b), (_, par_c, _, _) = results
    assert counts_a == counts_b and loss_a == loss_b
    for x, y in zip(par_a, par_b):
        np.testing.assert_array_equal(x, y)
    assert_same_bits(q_a, q_b, f"{call} {path} {np.dtype(dtype).name}: fit quality afterwards")
    for k in planes:
        n = na if k < 2 else nc
        for t in (0, 2):
            np.testing.assert_array_equal(par_a[k][t * n : (t + 1) * n], par_c[k][t * n : (t + 1) * n], err_msg=f"plane {k} of slice {t}")
        assert not np.array_equal(par_a[k][n : 2 * n], par_c[k][n : 2 * n]), k


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_later_call_starts_from_w0_behind_a_closed_form_solve(dtype):
    """clip, ``solve_coeffs()``, then Huber: the weights and scales of a solver at the same parameters that calls Huber for the first
    time (from the clipped plane the Huber weights of the clipped samples would be zero)."""
    kind, shape = "solve_coeffs", (12, 129)
    p, params, _, _ = inputs_of(kind, shape)
    a, w_clip, w0 = reweighted(kind, shape, dtype, "general")
    a.solve_coeffs()
    second = a.robust_weights(*HUBER)
    w_second = a.get_weights()
    par = a.get_params()
    a.close()
    c = path_solver(p, params, dtype, "general")
    c.set_params(*par)
    first = c.robust_weights(*HUBER)
    w_first = c.get_weights()
    c.close()
    assert_same_bits(second, first, f"{np.dtype(dtype).name}: the outputs of the later call")
    np.testing.assert_array_equal(w_second, w_first)
    clipped = (w_clip == 0) & (w0 > 0)
    assert np.all(w_second[clipped] > 0) and np.any(w_second < w0)
