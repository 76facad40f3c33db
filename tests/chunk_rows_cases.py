"""The cases of tests/test_chunk_rows_host.py and tests/test_gpu_chunk_rows.py: the closed-form calls at scratch bounds (``cs_bound``,
set through ``_set_coeff_solve_scratch``) that give chunks of SEVERAL rows, or groups, and a shorter last chunk.  The suite's other
files move the bound to 0 (everything in one chunk: ``a0 = 0``) and to 1 (one row per chunk: ``rel = 0``) only.

No problem is generated here: every case names a builder and a shape the suite already has --

    form "freq"    a frequency basis alone.  solve_gain_coeffs on ``edge_problem`` (``EDGE_SHAPES``) with ``random_basis``, as
                   test_gpu_gain_basis_solve.py; gain_basis_errors on ``freq_case`` (``FREQ_WIDTHS``) with ``rand_basis``, as
                   test_gpu_gain_basis_errors.py -- each call on the inputs its own file holds a restatement for
    form "slices"  three time slices in one solver, built as ``three_slices`` of test_gpu_solve_paths.py but of 5 antennas x 48 channels
                   (``na_slice`` = 5, 15 rows), the 100 ns DPSS basis
    form "both"    a time basis over a frequency basis: ``flagged_case`` and ``bases_of`` on ``SHAPES`` of test_gain_time_solve_host.py
    form "time"    a time basis alone: the same on ``TIME_ONLY_SHAPES``
    groups         solve_coeffs and fit_errors on ``boundary_case`` (126, 127, 128 vectors) and on ``edge_problem(7, 200)`` (eleven
                   groups of 7 ... 34 vectors, the first of them flagged wholly: the parity problem of both calls' own files)

-- and the rows per chunk wanted.  The bound is computed, never written down: ``rows * row_bytes`` with ``row_bytes`` from the row scalars
``cal_debug_solve_plan`` returns at bound 0 (what = 30 for the solves, 31 for gain_basis_errors, whose rows also hold W), and for the
group calls the bytes of a run of groups in the planner's order, in the manner of ``_plan_cases.solve_bounds``."""
import collections
import functools

import numpy as np

import _plan_cases as pc
from calamity_amd import _lib, batched, synthetic
from test_gain_basis_errors_host import FREQ_WIDTHS, error_row_chunks, freq_case
from test_gain_basis_solve_host import EDGE_SHAPES, dpss_basis
from test_gain_time_solve_host import SHAPES, TIME_ONLY_SHAPES, bases_of, flagged_case, rand_basis
from test_gpu_coeff_solve_shapes import boundary_case
from test_gpu_fit_quality import edge_problem, perturbed, solver_of
from test_gpu_gain_basis_solve import random_basis
from test_solve_plan_host import _chunks

DTYPES = [np.float32, np.float64]
LAYOUT, KERNEL_PATH = "shared", "auto"

# ---- row chunks ---------------------------------------------------------------------------------------------------------------------
# form, shape, bases, rows per chunk, the chunk lengths, the factor in LDS, doubles of scratch per row (d_row > 0)
RowCase = collections.namedtuple("RowCase", "form shape bases rows chunks in_lds d_row")


def _time_only(k):
    shape, L = TIME_ONLY_SHAPES[k]
    return shape, (("rand",), (L, None))


def _both(k):
    shape, kind, LK = SHAPES[k]
    return shape, (kind, LK)


assert EDGE_SHAPES[1] == (7, 200) and EDGE_SHAPES[2] == (12, 129) and EDGE_SHAPES[0] == (5, 48)
assert all(w in FREQ_WIDTHS for w in (((7, 200), 12), ((7, 200), 65), ((7, 200), 130), ((12, 129), 33)))

ROW_CASES = [
    # a frequency basis alone, one slice: 7 rows, the factor in LDS (K = 12) and in scratch (K = 130); 12 rows at K = 33
    RowCase("freq", (7, 200), 12, 2, [2, 2, 2, 1], True, False),
    RowCase("freq", (7, 200), 12, 3, [3, 3, 1], True, False),
    RowCase("freq", (7, 200), 12, 6, [6, 1], True, False),
    RowCase("freq", (7, 200), 130, 2, [2, 2, 2, 1], False, True),
    RowCase("freq", (7, 200), 130, 3, [3, 3, 1], False, True),
    RowCase("freq", (12, 129), 33, 5, [5, 5, 2], True, False),
    # three slices of 5 rows: the second and the third chunk straddle a slice boundary
    RowCase("slices", (5, 48), "dpss", 4, [4, 4, 4, 3], True, False),
    # both bases: n = 30 and 45 (LDS), 128 and 260 (scratch)
    RowCase("both", *_both(0), 2, [2, 2, 1], True, False),
    RowCase("both", *_both(0), 3, [3, 2], True, False),
    RowCase("both", *_both(0), 4, [4, 1], True, False),
    RowCase("both", *_both(1), 3, [3, 3, 1], True, False),
    RowCase("both", *_both(6), 2, [2, 2], False, True),  # (an even cut: ca == rows in every chunk, a0 > 0 and rel > 0 together)
    RowCase("both", *_both(6), 3, [3, 1], False, True),
    RowCase("both", *_both(7), 3, [3, 1], False, True),
    # a time basis alone: the channel systems in registers (L = 3, 8: row_bytes = 1, the bound is the row count) and in scratch (L = 9:
    # ca nfreqs = 258 and 387 systems, the second or third block of 256 partly live)
    RowCase("time", *_time_only(0), 2, [2, 2, 1], True, False),
    RowCase("time", *_time_only(0), 3, [3, 2], True, False),
    RowCase("time", *_time_only(0), 4, [4, 1], True, False),
    RowCase("time", *_time_only(1), 2, [2, 2, 1], True, False),
    RowCase("time", *_time_only(1), 3, [3, 2], True, False),
    RowCase("time", *_time_only(1), 4, [4, 1], True, False),
    RowCase("time", *_time_only(2), 2, [2, 2, 1], True, True),
    RowCase("time", *_time_only(2), 3, [3, 2], True, True),
]
# gain_basis_errors alone: W past one 64-row block under a frequency basis alone
ERROR_ONLY_CASES = [RowCase("freq", (7, 200), 65, 3, [3, 3, 1], True, False)]

# One solver moved across bounds: the bound that holds 3 rows of gain_basis_errors, then the one that holds 2.  A row of a sweep is
# lighter (no W), so the sweeps at these bounds cut other chunks than the errors between them: (rows of the sweep, of the errors) at
# either bound, which the host test reads back.  The shapes have enough rows for every one of them to lie between one and all.
MovedCase = collections.namedtuple("MovedCase", "case rows_at_3 rows_at_2")
MOVED_CASES = [MovedCase(RowCase("freq", (12, 129), 33, 3, [3, 3, 3, 3], True, False), (9, 3), (6, 2)),
               MovedCase(RowCase("both", *_both(1), 3, [3, 3, 1], True, False), (5, 3), (3, 2)),
               MovedCase(RowCase("time", *_time_only(1), 3, [3, 2], True, False), (3, 3), (2, 2)),
               MovedCase(RowCase("time", *_time_only(2), 3, [3, 2], True, True), (3, 3), (2, 2))]

SOLVE_CASES = [(c, False) for c in ROW_CASES]
ERROR_CASES = [(c, True) for c in ROW_CASES + ERROR_ONLY_CASES]
MASKS = [None, [1, 0, 1], [0, 1, 1]]


def case_id(arg):
    if isinstance(arg, tuple) and len(arg) == 2 and isinstance(arg[0], RowCase):
        c, errors = arg
        bases = c.bases if c.form in ("freq", "slices") else "x".join(str(v) for v in c.bases[1])
        return f"{'errors' if errors else 'solve'}-{c.form}-{'x'.join(str(v) for v in c.shape)}-{bases}-rows{c.rows}"
    if isinstance(arg, MovedCase):
        return case_id((arg.case, True)).split("-", 1)[1].rsplit("-", 1)[0]
    if isinstance(arg, GroupCase):
        return f"{arg.call}-{arg.name}"
    if isinstance(arg, type):
        return np.dtype(arg).name
    return None


@functools.lru_cache(maxsize=None)
def three_slices_of(nants, nfreqs):
    """``three_slices`` of tests/test_gpu_solve_paths.py at another shape: (one slice's problem, the problem of three, data, start)."""
    T = 3
    parts = [synthetic.make_problem(nants, nfreqs, f0=150e6, df=400e3, seed=21, data_seed=30 + t) for t in range(T)]
    p0 = parts[0][0]
    data = tuple(np.concatenate([getattr(parts[t][0], k) for t in range(T)]) for k in ("data_r", "data_i", "wgts"))
    pars = [perturbed(parts[t][0], parts[t][2], seed=40 + t) for t in range(T)]
    start = {k: np.concatenate([pars[t][k] for t in range(T)]) for k in ("g_r", "g_i", "c_r", "c_i")}
    sub, _, _ = batched.replicate_slices(p0, T)
    return p0, sub, data, start


def inputs(case, errors):
    """(problem, params or None, data or None, Bt or None, B or None) of a row case for the call."""
    if case.form == "freq":
        if errors:
            p, params = freq_case(case.shape)
            return p, params, None, None, rand_basis(case.shape[1], case.bases, 2)
        p, params = edge_problem(*case.shape)
        return p, params, None, None, random_basis(case.shape[1], case.bases)
    if case.form == "slices":
        _, sub, data, start = three_slices_of(*case.shape)
        return sub, start, data, None, dpss_basis(case.shape[1])
    p, params = flagged_case(*case.shape)
    Bt, B = bases_of(case.shape, *case.bases)
    return p, params, None, Bt, B


def klt(case, errors=False):
    """(K, L, T) as cal_debug_solve_plan takes them, and the rows the call cuts into chunks."""
    p, _, _, Bt, B = inputs(case, errors)
    K = 0 if B is None else B.shape[1]
    if Bt is None:
        return (K, 0, 0), p.nants
    return (K, Bt.shape[1], Bt.shape[0]), p.nants // Bt.shape[0]


def row_plan(case, dtype, bound, errors):
    """The row scalars of the planner at ``bound`` as a dict (``x_row`` with ``errors``)."""
    p = inputs(case, errors)[0]
    shape = klt(case, errors)[0]
    if errors:
        got = error_row_chunks(p, dtype, LAYOUT, KERNEL_PATH, bound, shape)
        return dict(zip(pc.ROW_SCALARS + ["x_row"], got))
    got = pc.solve_plan(_lib.load().cal_debug_solve_plan, p, dtype, LAYOUT, KERNEL_PATH, bound, [pc.WHAT_ROW_CHUNKS], shape)["row_chunks"]
    return dict(zip(pc.ROW_SCALARS, got.tolist()))


@functools.lru_cache(maxsize=None)
def _row_bytes(case_key, dtype_name, errors):
    case, dtype = RowCase(*case_key), np.dtype(dtype_name).type
    r = row_plan(case, dtype, 0, errors)
    return max(1, (r["m_row"] + r["n_row"] + r.get("x_row", 0)) * np.dtype(dtype).itemsize + r["d_row"] * 8)


def _key(case):
    return tuple(tuple(v) if isinstance(v, list) else v for v in case)


def row_bytes(case, dtype, errors):
    """What a row takes of the bound: from the planner's own scalars at bound 0 (1 where a row keeps nothing in scratch)."""
    return _row_bytes(_key(case), np.dtype(dtype).name, errors)


def row_bound(case, dtype, errors, rows=None):
    """The scratch bound in bytes that holds ``rows`` rows (the case's own by default) and not one more."""
    return (case.rows if rows is None else rows) * row_bytes(case, dtype, errors)


def chunk_lengths(nrows, rows):
    """The ``ca`` of the calls' loops ``for a0 in range(0, nrows, rows)``."""
    return [min(rows, nrows - a0) for a0 in range(0, nrows, rows)]


def row_solver(case, dtype, errors):
    """A solver on the SHARED layout with the case's problem, parameters and bases; and the name of its sweep."""
    from calamity_amd.solver import HipFitSolver

    p, params, data, Bt, B = inputs(case, errors)
    if data is None:
        s = solver_of(p, params, dtype, LAYOUT)
    else:
        s = HipFitSolver(dtype=dtype)
        s.set_problem(p, layout=LAYOUT)
        s.set_data(*data)
        s.set_params(params["g_r"], params["g_i"], params["c_r"], params["c_i"])
    if B is not None:
        s.set_gain_basis(B)
    if Bt is not None:
        s.set_gain_time_basis(Bt)
    return s, ("solve_gain_coeffs" if Bt is None else "solve_gain_time_coeffs")


# ---- group chunks -------------------------------------------------------------------------------------------------------------------
# call, name, builder, the run [i, j) of groups (heaviest first) whose bytes are the bound, the groups per chunk
GroupCase = collections.namedtuple("GroupCase", "call name builder run chunks")


def edge_7_200():
    return edge_problem(7, 200)


def group_bytes(nvec, itemsize, fe):
    """Bytes of a group in a chunk, by the count of ``_plan_cases.solve_bounds``: N in the dtype and the factor in double; fit_errors'
    W, padded to whole 16 x 16 tiles, on top."""
    n = np.asarray(nvec, np.int64)
    pad = (n + 15) // 16 * 16
    return n * n * itemsize + (n + 2) * n * 8 + (pad * pad * itemsize if fe else 0)


def group_nvec(case):
    p = case.builder()[0]
    return np.asarray([p.basis[u].shape[1] for u in p.grp_basis])


def group_bound(case, dtype):
    """The bytes of the groups ``case.run`` of the planner's order (heaviest first, stable)."""
    heavy = np.sort(group_nvec(case))[::-1]
    b = group_bytes(heavy, np.dtype(dtype).itemsize, case.call == "fit_errors")
    return int(b[case.run[0] : case.run[1]].sum())


def group_plan(case, dtype, bound):
    """Rows (g0, g1, w0, w1, l0, l1, lds) of the chunks the call's planner cuts at ``bound``."""
    p = case.builder()[0]
    what = 14 if case.call == "fit_errors" else 4
    got = pc.solve_plan(_lib.load().cal_debug_solve_plan, p, dtype, LAYOUT, KERNEL_PATH, bound, [what])
    return _chunks(got[pc.SOLVE_ARRAYS[what][0]])


# boundary: the two heaviest (128: in scratch, 127) and then 126 alone; 128 alone and then 127 with 126 -- with three groups a later
# chunk of two and a shorter last chunk exclude each other, so each bound gives one of them.  edge (nvec 25, 23, 23 and eight of 16; W
# counted, fit_errors cuts elsewhere): both at one bound -- later chunks of several groups with w0, l0, noff, doff and woff all
# non-zero, and a last chunk shorter than the first.
GROUP_CASES = [GroupCase(call, name, boundary_case, run, chunks) for call in ("solve_coeffs", "fit_errors")
               for name, run, chunks in (("boundary_head", (0, 2), [2, 1]), ("boundary_tail", (1, 3), [1, 2]))]
GROUP_CASES += [GroupCase("solve_coeffs", "edge", edge_7_200, (0, 3), [3, 6, 2]), GroupCase("fit_errors", "edge", edge_7_200, (0, 2), [2, 3, 5, 1])]