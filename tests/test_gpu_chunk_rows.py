"""The closed-form calls at chunks of SEVERAL rows (or groups) and a shorter last chunk: solve_gain_coeffs, solve_gain_time_coeffs and
gain_basis_errors (row chunks), solve_coeffs and fit_errors (group chunks) at the scratch bounds of tests/chunk_rows_cases.py, whose plans
tests/test_chunk_rows_host.py pins.  The other files move the bound to 0 (one chunk: a0 = 0, rel = a) and to 1 (one row per chunk:
rel = 0, a0 = a) only, where every address f(a0) + g(rel) has one term at zero and ca == rows in every chunk.

Every output of a call at the case's bound equals, to the bit, the same call of a fresh solver at bound 0 -- which the calls' own files
hold against their fp64 NumPy restatements, so no tolerance is set here; once per call family the chunked result is also held against
that restatement directly, with the imported ``check`` and ``TOL`` of the family's file (two wrong chunked results cannot vouch for each
other).  The singular systems the builders plant keep their zeros, or their bits.  Under a slice mask a chunk that straddles a slice
boundary with one side masked leaves the masked side's y, gains and moments alone and counts the selected slices only.  One solver moved
across bounds (3 rows, sweep, errors, 2 rows, errors, sweep) gives what a solver at bound 0 gives: the shared, grown-only buffers carry no
stale chunk length.

Shown once, on scratch copies of the library (nothing of it is kept): four deliberately wrong builds, each inside its allocated buffers
(the destination of M1 ends at ((T - 1) rows + ca) K K <= rows T K K elements, the size pg_m is reserved with; M2 ... M4 read or write a
row of the chunk that precedes the right one).  Under each of them the six files that moved the bound before this one
(test_gpu_gain_basis_solve.py, test_gpu_gain_time_solve.py, test_gpu_gain_basis_errors.py, test_gpu_gain_systems_shared.py,
test_gpu_fit_errors.py, test_gpu_coeff_solve.py) pass as they do on the parent; of this file's tests there fail

    M1  enqueue_gain_systems: the per-time Gram of a chunk written to pg_m + t * rows * K * K instead of t * ca * K * K
        30 tests: every "both" case of the sweeps (12) and of the error bars (12) but the even cut (9, 4, 40) rows 2, where ca == rows in
        every chunk; test_chunked_error_bars_equal_the_restatement[both] (2), the moved solver on (6, 7, 40) (2) and
        test_a_chunked_time_basis_sweep_equals_the_restatement[both] (2) -- the last by its counts alone: the one row of its last chunk
        is the flagged antenna, whose right-hand side is zero whatever its matrix, so the planes agree and a stale matrix only makes
        the singular row count as solved
    M2  gain_error_var_kernel: W read at wmat + (a0 ? 0 : rel) * np * np (the first row's W for every row of a later chunk)
        24 tests: the error bars of every "freq", "slices" and "both" case whose later chunks hold two or more solved rows (18),
        test_chunked_error_bars_equal_the_restatement[freq] (2), the moved solver under a frequency basis and under both (4)
    M3  gain_basis_gram_kernel: the mask byte of the chunk's first row for every row of a later chunk, slice_mask[(a0 + (a0 ? 0 : rel)) / na_slice]
        4 tests: test_a_chunk_that_straddles_a_masked_slice_leaves_it_alone, both masks, both precisions
    M4  gain_time_chan_kernel: a = a0 + (a0 ? 0 : rel) (every channel system of a later chunk is its first antenna's)
        18 tests: the sweeps of every "time" case at 2 and 3 rows per chunk (12; at 4 rows the one later chunk holds one row),
        test_a_chunked_time_basis_sweep_equals_the_restatement[time] (2), the moved solver under a time basis alone (4)

The group calls have no such build: their kernels take every offset (noff, doff, woff, w0, l0) from the planner's tables, which
tests/test_solve_plan_host.py pins byte for byte; what this file adds for them is the first run on the device of a later chunk of several
groups.  130 tests in 6.5 s on one MI355X, none above 0.6 s.
"""
import functools

import numpy as np
import pytest

import chunk_rows_cases as C
import test_gpu_coeff_solve_shapes as coeff_file
import test_gpu_fit_errors as fit_errors_file
import test_gpu_gain_basis_errors as errors_file
import test_gpu_gain_basis_solve as freq_file
import test_gpu_gain_time_solve as time_file
from test_gain_basis_solve_host import restated_basis
from test_gpu_fit_quality import solver_of

pytestmark = pytest.mark.gpu

NSWEEPS = 2
ERROR_KEYS = ("gain_var", "y_var", "gain_dof")


def frozen(arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


def sweep_outputs(s, sweep, nsweeps=NSWEEPS, **kw):
    """[nsolved, nsingular, g_r, g_i, y_r, y_i] of one call of ``nsweeps`` sweeps."""
    counts = getattr(s, sweep)(nsweeps, **kw)
    return [counts["nsolved"], counts["nsingular"], *s.get_params()[:2], *s.get_gain_coeffs()]


def error_outputs(s):
    out = s.gain_basis_errors()
    return [out["nsolved"], out["nsingular"]] + [out[k] for k in ERROR_KEYS]


def row_call(case, errors, dtype, bound):
    """(outputs of the call at ``bound`` on a fresh solver, the gains and coefficients before it)."""
    s, sweep = C.row_solver(case, dtype, errors)
    s._set_coeff_solve_scratch(bound)
    before = s.get_params()
    out = error_outputs(s) if errors else sweep_outputs(s, sweep)
    s.close()
    return frozen(out), frozen(list(before))


@functools.lru_cache(maxsize=None)
def _row_reference(form, shape, bases, errors, dtype_name):
    """The call at bound 0, once per problem, call and dtype: shared by the cases that differ in their rows per chunk only."""
    case = C.RowCase(form, shape, bases, 0, (), True, False)
    return row_call(case, errors, np.dtype(dtype_name).type, 0)


def row_reference(case, errors, dtype):
    return _row_reference(case.form, case.shape, case.bases, errors, np.dtype(dtype).name)


def assert_same(got, want, label):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        if isinstance(b, np.ndarray):
            assert a.dtype == b.dtype and a.shape == b.shape, (label, k)
            np.testing.assert_array_equal(a, b, err_msg=f"{label}: output {k}")
        else:
            assert a == b, (label, k, a, b)


# ---- the sweeps
@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.case_id)
@pytest.mark.parametrize("case", C.SOLVE_CASES, ids=C.case_id)
def test_sweeps_in_chunks_of_several_rows_give_the_bits_of_one_chunk(case, dtype):
    c, _ = case
    got, before = row_call(c, False, dtype, C.row_bound(c, dtype, False))
    want, _ = row_reference(c, False, dtype)
    assert_same(got, want, C.case_id(case))
    nsolved, nsingular, g_r, g_i, y_r, y_i = got
    assert np.any(y_r) and np.any(y_i)
    if c.form == "slices":  # nothing flagged
        assert (nsolved, nsingular) == (15, 0) and all(np.any(y_r[a]) for a in range(15))
        return
    if c.form == "freq":  # edge_problem: the last antenna has no baseline
        na = c.shape[0]
        assert (nsolved, nsingular) == (na - 1, 1)
        assert not np.any(y_r[na - 1]) and not np.any(y_i[na - 1]) and all(np.any(y_r[a]) for a in range(na - 1))
        np.testing.assert_array_equal(g_r[na - 1], before[0][na - 1])
        np.testing.assert_array_equal(g_i[na - 1], before[1][na - 1])
        return
    # flagged_case: the last antenna is flagged wholly, antenna 2 at time 0 (it is solved and moves there), channel 3 of antenna 1
    T, na, F = c.shape
    assert not np.any(y_r[na - 1]) and not np.any(y_i[na - 1]) and all(np.any(y_r[a]) for a in range(na - 1))
    np.testing.assert_array_equal(g_r[na - 1 :: na], before[0][na - 1 :: na])
    np.testing.assert_array_equal(g_i[na - 1 :: na], before[1][na - 1 :: na])
    assert np.mean(g_r[2] != before[0][2]) > 0.9
    if c.form == "both":
        assert (nsolved, nsingular) == (na - 1, 1) and np.any(g_r[1::na, 3] != before[0][1::na, 3])
    else:
        assert (nsolved, nsingular) == ((na - 1) * F - 1, F + 1)
        np.testing.assert_array_equal(g_r[1::na, 3], before[0][1::na, 3])
        np.testing.assert_array_equal(g_i[1::na, 3], before[1][1::na, 3])
        assert not np.any(y_r[1, :, 3]) and not np.any(y_i[1, :, 3])


# ---- the error bars
@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.case_id)
@pytest.mark.parametrize("case", C.ERROR_CASES, ids=C.case_id)
def test_error_bars_in_chunks_of_several_rows_give_the_bits_of_one_chunk(case, dtype):
    c, _ = case
    got, _ = row_call(c, True, dtype, C.row_bound(c, dtype, True))
    want, _ = row_reference(c, True, dtype)
    assert_same(got, want, C.case_id(case))
    nsolved, nsingular, gain_var, y_var, gain_dof = got
    if c.form == "slices":
        assert (nsolved, nsingular) == (15, 0) and np.all(gain_var > 0) and np.all(y_var > 0) and np.all(gain_dof > 0)
        return
    if c.form == "freq":  # freq_case: antenna 2 (flagged at the one time) and the last antenna are the singular rows
        na = c.shape[0]
        assert (nsolved, nsingular) == (na - 2, 2)
        for a in range(na):
            zero = a in (2, na - 1)
            assert np.all((gain_var[a] == 0) == zero) and np.all((y_var[a] == 0) == zero) and (gain_dof[a] == 0) == zero, a
        return
    T, na, F = c.shape
    assert not np.any(gain_var[na - 1 :: na]) and not np.any(y_var[na - 1]) and gain_dof[na - 1] == 0
    assert np.all(gain_var[2] > 0) and np.all(gain_dof[: na - 1] > 0)
    if c.form == "both":
        assert (nsolved, nsingular) == (na - 1, 1) and np.all(gain_var[: na - 1] > 0) and np.all(y_var[: na - 1] > 0)
    else:
        assert (nsolved, nsingular) == ((na - 1) * F - 1, F + 1)
        assert not np.any(gain_var[1::na, 3]) and not np.any(y_var[1, :, 3])
        live = np.ones((na, F), bool)
        live[na - 1], live[1, 3] = False, False
        assert np.all((gain_var.reshape(T, na, F) > 0) == live[None]) and np.all((y_var > 0) == live[:, None, :])


# ---- masked slices: chunks of 4 rows on slices of 5, the second and the third chunk straddle a boundary
SLICES = next(c for c in C.ROW_CASES if c.form == "slices")


def masked_call(dtype, mask, bound):
    """Three Adam steps (y and its moments move in every slice), then two sweeps of the selected slices with their moments reset."""
    s, sweep = C.row_solver(SLICES, dtype, False)
    s.set_optimizer("Adam", learning_rate=1e-2)
    s.run_slices(3, tol=0.0)
    s._set_coeff_solve_scratch(bound)
    state = lambda: frozen(list(s.get_params()) + list(s.get_gain_coeffs()) + [v for _, v in sorted(s.get_gain_coeff_moments().items())])  # noqa: E731
    keys = ["g_r", "g_i", "c_r", "c_i", "y_r", "y_i"] + sorted(s.get_gain_coeff_moments())
    before = state()
    counts = s.solve_gain_coeffs(NSWEEPS, slice_mask=mask, reset_gain_moments=True)
    after = state()
    s.close()
    return keys, before, after, counts


@functools.lru_cache(maxsize=None)
def masked_reference(dtype_name, mask):
    return masked_call(np.dtype(dtype_name).type, list(mask), 0)


@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.case_id)
@pytest.mark.parametrize("mask", C.MASKS[1:], ids=lambda m: "mask" + "".join(str(v) for v in m))
def test_a_chunk_that_straddles_a_masked_slice_leaves_it_alone(mask, dtype):
    na = SLICES.shape[0]
    keys, before, after, counts = masked_call(dtype, mask, C.row_bound(SLICES, dtype, False))
    _, before0, after0, counts0 = masked_reference(np.dtype(dtype).name, tuple(mask))
    assert counts == counts0 == {"nsolved": na * sum(mask), "nsingular": 0}  # the selected slices only
    assert_same(before, before0, "before the call")
    assert_same(after, after0, f"mask {mask}")
    per_row = [k for k in keys if k not in ("c_r", "c_i", "cm_r", "cm_i", "cv_r", "cv_i", "t")]
    assert {"g_r", "g_i", "y_r", "y_i", "ym_r", "ym_i", "yv_r", "yv_i"} <= set(per_row)
    for t in range(3):
        rows = slice(t * na, (t + 1) * na)
        for k in per_row:
            new, old = after[keys.index(k)][rows], before[keys.index(k)][rows]
            assert np.any(old), (k, t)  # the steps moved it, so the call has something to keep, or to reset
            if mask[t]:
                assert not np.array_equal(new, old), (k, t)
            else:
                np.testing.assert_array_equal(new, old, err_msg=f"{k} of the masked slice {t}")
    for k in ("c_r", "c_i", "cm_r", "cm_i", "cv_r", "cv_i", "t"):
        np.testing.assert_array_equal(after[keys.index(k)], before[keys.index(k)], err_msg=k)


# ---- the group calls
def group_call(case, dtype, bound):
    p, params = case.builder()
    s = solver_of(p, params, dtype, C.LAYOUT)
    s._set_coeff_solve_scratch(bound)
    if case.call == "solve_coeffs":
        counts = s.solve_coeffs()
        out = [counts["nsolved"], counts["nsingular"], *s.get_params()[2:]]
    else:
        e = s.fit_errors()
        out = [e["nsolved"], e["nsingular"]] + [e[k] for k in fit_errors_file.OUTPUTS]
    s.close()
    return frozen(out)


@functools.lru_cache(maxsize=None)
def group_reference(call, builder, dtype_name):
    return group_call(C.GroupCase(call, "", builder, (0, 0), ()), np.dtype(dtype_name).type, 0)


@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.case_id)
@pytest.mark.parametrize("case", C.GROUP_CASES, ids=C.case_id)
def test_groups_in_chunks_of_several_give_the_bits_of_one_chunk(case, dtype):
    got = group_call(case, dtype, C.group_bound(case, dtype))
    assert_same(got, group_reference(case.call, case.builder, np.dtype(dtype).name), C.case_id(case))
    p, params = case.builder()
    nv0 = p.grp_coff[1]
    planted = int(case.name == "edge")  # edge_problem: baseline 0, the first group, is flagged wholly
    assert (got[0], got[1]) == (p.ngrps - planted, planted)
    if case.call == "solve_coeffs":
        start = [np.asarray(params[k], dtype=dtype) for k in ("c_r", "c_i")]
        for new, old in zip(got[2:], start):
            assert np.all(new[nv0 * planted :] != old[nv0 * planted :])
            np.testing.assert_array_equal(new[: nv0 * planted], old[: nv0 * planted])  # the singular group: the bits it had
    else:
        e = dict(zip(fit_errors_file.OUTPUTS, got[2:]))
        assert np.all(e["coeff_var"][nv0 * planted :] > 0) and np.all(e["leverage_bl"][planted:] > 0) and np.all(np.any(e["model_var"][planted:], axis=1))
        if planted:
            assert not np.any(e["coeff_var"][:nv0]) and not np.any(e["model_var"][0]) and e["leverage_bl"][0] == 0 and e["nsamp_bl"][0] == 0


# ---- once per call family: the chunked call against the family's own restatement, within the family's own bound
def pick(form, shape0, rows):
    return next(c for c in C.ROW_CASES if c.form == form and c.shape[0] == shape0 and c.rows == rows)


PARITY_FREQ = pick("freq", 7, 3)._replace(bases=130, in_lds=False, d_row=True)
assert PARITY_FREQ in C.ROW_CASES
PARITY_BOTH = next(c for c in C.ROW_CASES if c.form == "both" and c.bases[1] == (8, 16) and c.rows == 3)  # n = 128: the factor in scratch
PARITY_TIME = next(c for c in C.ROW_CASES if c.form == "time" and c.bases[1][0] == 9 and c.rows == 3)  # L = 9: the systems in scratch


@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.case_id)
def test_a_chunked_frequency_basis_sweep_equals_the_restatement(dtype):
    c = PARITY_FREQ
    p, params, _, _, B = C.inputs(c, False)
    s, sweep = C.row_solver(c, dtype, False)
    s._set_coeff_solve_scratch(C.row_bound(c, dtype, False))
    assert getattr(s, sweep)(NSWEEPS) == {"nsolved": p.nants - 1, "nsingular": 1}
    want_g, want_y = restated_basis(p, params, dtype, B, nsweeps=NSWEEPS)[:2]
    freq_file.check(s, want_g, want_y, dtype, f"{C.case_id((c, False))} {np.dtype(dtype).name}")
    s.close()


@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.case_id)
@pytest.mark.parametrize("c", [PARITY_BOTH, PARITY_TIME], ids=["both", "time"])
def test_a_chunked_time_basis_sweep_equals_the_restatement(c, dtype):
    s, sweep = C.row_solver(c, dtype, False)
    s._set_coeff_solve_scratch(C.row_bound(c, dtype, False))
    T, na, F = c.shape
    assert getattr(s, sweep)(1) == ({"nsolved": na - 1, "nsingular": 1} if c.form == "both" else {"nsolved": (na - 1) * F - 1, "nsingular": F + 1})
    want_g, want_y = time_file.reference(c.shape, *c.bases, np.dtype(dtype).name, 1)[:2]
    time_file.check(s, want_g, want_y, dtype, f"{C.case_id((c, False))} {np.dtype(dtype).name}")
    s.close()


@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.case_id)
@pytest.mark.parametrize("c", [PARITY_FREQ, PARITY_BOTH, PARITY_TIME], ids=["freq", "both", "time"])
def test_chunked_error_bars_equal_the_restatement(c, dtype):
    s, _ = C.row_solver(c, dtype, True)
    s._set_coeff_solve_scratch(C.row_bound(c, dtype, True))
    out = s.gain_basis_errors()
    s.close()
    name = np.dtype(dtype).name
    want = errors_file.freq_reference(c.shape, c.bases, name) if c.form == "freq" else errors_file.time_reference(c.shape, *c.bases, name)
    errors_file.check(out, want, dtype, f"{C.case_id((c, True))} {name}")


@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.case_id)
@pytest.mark.parametrize("case", [g for g in C.GROUP_CASES if g.name == "boundary_tail"], ids=C.case_id)
def test_chunked_group_calls_equal_the_restatement(case, dtype):
    """128 vectors alone, then 127 and 126 in one later chunk."""
    label = f"{C.case_id(case)} {np.dtype(dtype).name}"
    if case.call == "solve_coeffs":
        coeff_file.solve_and_check(case.builder, dtype, label, scratch=C.group_bound(case, dtype))
    else:
        fit_errors_file.run_case(case.builder, dtype, label, scratch=C.group_bound(case, dtype))


# ---- one solver moved across bounds
def moved_call(s, what, sweep):
    return frozen(sweep_outputs(s, sweep) if what == "sweep" else error_outputs(s))


@functools.lru_cache(maxsize=None)
def moved_reference(form, shape, bases, dtype_name, nsweeps_before, what):
    """``what`` on a solver that reached its parameters by ``nsweeps_before`` calls of two sweeps, all at bound 0."""
    s, sweep = C.row_solver(C.RowCase(form, shape, bases, 0, (), True, False), np.dtype(dtype_name).type, True)
    for _ in range(nsweeps_before):
        getattr(s, sweep)(NSWEEPS)
    out = moved_call(s, what, sweep)
    s.close()
    return out


@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.case_id)
@pytest.mark.parametrize("moved", C.MOVED_CASES, ids=C.case_id)
def test_one_solver_moved_across_bounds_carries_no_stale_chunk_length(moved, dtype):
    """Bound for 3 rows of the errors, sweep, errors, bound for 2 rows, errors, sweep: between two bounds the sweep and the errors cut
    different chunks into the same buffers, which only grow."""
    c = moved.case
    s, sweep = C.row_solver(c, dtype, True)
    nsweeps = 0
    for step, what in enumerate([3, "sweep", "errors", 2, "errors", "sweep"]):
        if isinstance(what, int):
            s._set_coeff_solve_scratch(C.row_bound(c, dtype, True, what))
            continue
        got = moved_call(s, what, sweep)
        want = moved_reference(c.form, c.shape, c.bases, np.dtype(dtype).name, nsweeps, what)
        assert got[0] > 0 and all(np.any(a) for a in got[2:]), (step, what)
        assert_same(got, want, f"{C.case_id(moved)} step {step} ({what})")
        nsweeps += what == "sweep"
    s.close()
