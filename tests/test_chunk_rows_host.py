"""What the planner really gives at the bounds of tests/chunk_rows_cases.py (`cal_debug_solve_plan`: csrc/solve_plan.hpp run with no
device), so that no case of tests/test_gpu_chunk_rows.py can quietly stop reaching its branch: the rows per chunk are the wanted ones
and lie strictly between one row and all rows, the chunk lengths are the listed ones (a shorter last chunk, or the one even cut), the
factor is on the listed side of its LDS bound, the channel systems of a time basis alone are in registers or in scratch as listed; for
the group calls a later chunk of several groups and a last chunk shorter than the first.  The bound is exact: one byte less holds one
row less."""
import numpy as np
import pytest

import _plan_cases as pc
import chunk_rows_cases as C


@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.case_id)
@pytest.mark.parametrize("case", C.SOLVE_CASES + C.ERROR_CASES, ids=C.case_id)
def test_the_bound_gives_the_rows_and_the_branch_of_the_case(case, dtype):
    c, errors = case
    (K, L, T), nrows = C.klt(c, errors)
    per_row = C.row_bytes(c, dtype, errors)
    bound = C.row_bound(c, dtype, errors)
    assert bound == c.rows * per_row and 1 < bound < pc.CS_DEFAULT_BOUND
    r = C.row_plan(c, dtype, bound, errors)
    print(f"{C.case_id(case)} {np.dtype(dtype).name}: (K, L, T) = {(K, L, T)}, {nrows} rows, {per_row} bytes a row, bound {bound}: {r}")
    assert r["rows"] == c.rows and 1 < r["rows"] < nrows
    lengths = C.chunk_lengths(nrows, r["rows"])
    assert lengths == list(c.chunks) and sum(lengths) == nrows and len(lengths) >= 2
    assert lengths[-1] < lengths[0] or (c.form, c.rows, nrows) == ("both", 2, 4)  # a ragged tail, but for the one even cut
    assert bool(r["in_lds"]) == c.in_lds and (r["d_row"] > 0) == c.d_row
    assert r["n"] == (L if L else 1) * K
    # the ends the other files test are elsewhere: all rows at bound 0, one row at bound 1
    assert C.row_plan(c, dtype, 0, errors)["rows"] == nrows and C.row_plan(c, dtype, 1, errors)["rows"] == 1
    # the bound is exact
    assert C.row_plan(c, dtype, bound - 1, errors)["rows"] == c.rows - 1
    assert C.row_plan(c, dtype, bound + per_row - 1, errors)["rows"] == c.rows
    if errors:
        assert r["x_row"] == (((r["n"] + 15) // 16 * 16) ** 2 if K else 0)
        if K:  # W counted: a row of the errors takes more than a row of the solves
            assert per_row > C.row_bytes(c, dtype, False)
    if c.form == "time":
        assert K == 0 and (per_row == 1) == (L <= pc.TIME_TILE) and c.d_row == (L > pc.TIME_TILE)
        if L > pc.TIME_TILE:  # ca nfreqs systems over blocks of 256: the last block partly live
            assert lengths[0] * c.shape[2] == {2: 258, 3: 387}[c.rows] and lengths[-1] * c.shape[2] in (129, 258)
    if c.form == "slices":
        na_slice = c.shape[0]
        starts = np.cumsum([0] + lengths)
        straddling = [(a0, a1) for a0, a1 in zip(starts[:-1], starts[1:]) if a0 // na_slice != (a1 - 1) // na_slice]
        assert nrows == 3 * na_slice and len(straddling) == 2, straddling


@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.case_id)
@pytest.mark.parametrize("moved", C.MOVED_CASES, ids=C.case_id)
def test_the_bounds_of_the_moved_solver_chunk_both_calls(moved, dtype):
    """Bounds that hold 3 and 2 rows of gain_basis_errors: the sweep between them is cut into other chunks, of several rows too."""
    c = moved.case
    nrows = C.klt(c, True)[1]
    for rows, want in ((3, moved.rows_at_3), (2, moved.rows_at_2)):
        bound = C.row_bound(c, dtype, True, rows)
        got = (C.row_plan(c, dtype, bound, False)["rows"], C.row_plan(c, dtype, bound, True)["rows"])
        print(f"{C.case_id(moved)} {np.dtype(dtype).name}: bound {bound}: rows of a sweep {got[0]}, of the errors {got[1]}, of {nrows}")
        assert got == want and got[1] == rows and all(1 < r < nrows for r in got)
        if c.form != "time":
            assert got[0] > got[1]  # one bound, two chunkings: what a stale ca in the shared buffers would need


def test_the_table_holds_the_cases_it_is_there_for():
    forms = {(c.form, c.in_lds, c.d_row) for c in C.ROW_CASES}
    assert forms == {("freq", True, False), ("freq", False, True), ("slices", True, False), ("both", True, False), ("both", False, True),
                     ("time", True, False), ("time", True, True)}
    assert len(C.SOLVE_CASES) == 22 and len(C.ERROR_CASES) == 23
    ids = [C.case_id(c) for c in C.SOLVE_CASES + C.ERROR_CASES]
    assert len(set(ids)) == len(ids)


@pytest.mark.parametrize("dtype", C.DTYPES, ids=C.case_id)
@pytest.mark.parametrize("case", C.GROUP_CASES, ids=C.case_id)
def test_the_group_bound_gives_the_chunks_of_the_case(case, dtype):
    nvec = C.group_nvec(case)
    bound = C.group_bound(case, dtype)
    assert 1 < bound < pc.CS_DEFAULT_BOUND
    ch = C.group_plan(case, dtype, bound)
    counts = (ch[:, 1] - ch[:, 0]).tolist()
    print(f"{C.case_id(case)} {np.dtype(dtype).name}: nvec {np.sort(nvec)[::-1].tolist()}, bound {bound}: groups per chunk {counts}, chunks {ch.tolist()}")
    assert counts == list(case.chunks) and sum(counts) == len(nvec) and len(counts) >= 2
    assert ch[0, 0] == 0 and (ch[1:, 0] == ch[:-1, 1]).all() and (ch[1:, 2] == ch[:-1, 3]).all() and (ch[1:, 2] > 0).all()
    fe = case.call == "fit_errors"
    assert ((ch[1:, 4] > 0).all() and (ch[:, 5] > ch[:, 4]).all()) if fe else not ch[:, 4:6].any()
    # the ends the other files test are elsewhere
    assert len(C.group_plan(case, dtype, 0)) == 1 and len(C.group_plan(case, dtype, 1)) == len(nvec)
    later_of_several, shorter_tail = any(n >= 2 for n in counts[1:]), counts[-1] < counts[0]
    if case.name == "edge":  # five or more groups of unequal nvec: both at one bound
        assert len(nvec) >= 5 and len(set(nvec.tolist())) >= 3 and later_of_several and shorter_tail
    else:  # three groups: one of the two at each bound, the factor of the widest in scratch and the others' in LDS
        assert sorted(nvec.tolist()) == [126, 127, 128] and (later_of_several, shorter_tail) == ((False, True) if case.name == "boundary_head" else (True, False))
        assert ch[0, 6] == pc.CS_LDS_DOUBLES * 8 and ch[-1, 6] < pc.CS_LDS_DOUBLES * 8
