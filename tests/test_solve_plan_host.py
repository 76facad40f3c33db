"""The planner of the closed-form calls on the host (`cal_debug_solve_plan`: calamity_amd/csrc/solve_plan.hpp run with no device).

The group plans of solve_coeffs and fit_errors and the antenna lists without autocorrelations equal, byte for byte, what the planning
loops of commit cbff279 -- written inside the solver, between its allocations and launches -- computed for the same problems
(tests/golden/solve_plan/*.npz).  The fixtures were recorded on the CPU: a program over that commit's problem_plan.hpp held its three
loop bodies unchanged, its two device read-backs replaced by the planner's host `bl_tile` and the description's antenna pairs.  The order
of the groups and of the block pairs is the order the kernels work in, so an unchanged plan is what keeps results bit for bit.

The row chunks of solve_gain_coeffs and solve_gain_time_coeffs are compared with the rule restated here."""
import ctypes as C
import os

import numpy as np
import pytest

import _plan_cases as pc
from calamity_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solve_plan")
TAGS = ("default", "one", "two_cs", "two_fe")
GROUP_WHATS = [w for w in pc.SOLVE_ARRAYS if w not in pc.SOLVE_LISTS]
_cache = {}


def _case(name):
    """(problem, dtype, layout, kernel_path, nvec per group, bounds), built once per case."""
    if name not in _cache:
        prob, dtype, layout, kernel_path = pc.CASES[name]()
        nvec = np.asarray([prob.basis[u].shape[1] for u in prob.grp_basis])
        _cache[name] = (prob, dtype, layout, kernel_path, nvec, pc.solve_bounds(nvec, np.dtype(dtype).itemsize))
    return _cache[name]


def _chunks(a):
    """chunk records -> rows of (g0, g1, w0, w1, l0, l1, lds): six int32 and one int64"""
    r = a.reshape(-1, 8)
    return np.column_stack([r[:, :6].astype(np.int64), r[:, 6:].copy().view(np.int64)[:, 0]])


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("name", pc.SOLVE_CASES)
def test_group_plans_equal_recorded(name, tag):
    gold = np.load(os.path.join(GOLDEN, name + ".npz"))
    assert str(gold["parent"]) == "cbff279"
    prob, dtype, layout, kernel_path, _, bounds = _case(name)
    assert [bounds[k] for k in sorted(bounds)] == gold["bounds"].tolist()
    got = pc.solve_plan(_lib.load().cal_debug_solve_plan, prob, dtype, layout, kernel_path, bounds[tag], GROUP_WHATS)
    for nm in sorted(got):
        want = gold[tag + "." + nm]
        assert got[nm].dtype == want.dtype and got[nm].shape == want.shape, nm
        assert got[nm].tobytes() == want.tobytes(), (nm, np.flatnonzero(got[nm] != want)[:8])


@pytest.mark.parametrize("name", pc.SOLVE_CASES)
def test_antenna_lists_equal_recorded(name):
    gold = np.load(os.path.join(GOLDEN, name + ".npz"))
    prob, dtype, layout, kernel_path, _, bounds = _case(name)
    for bound in (0, 1):  # the lists do not depend on the bound
        got = pc.solve_plan(_lib.load().cal_debug_solve_plan, prob, dtype, layout, kernel_path, bound, list(pc.SOLVE_LISTS))
        for nm in ("gs_ptr", "gs_ent"):
            assert got[nm].dtype == gold[nm].dtype and got[nm].tobytes() == gold[nm].tobytes(), nm
    assert len(got["gs_ptr"]) == prob.nants + 1 and got["gs_ptr"][-1] == 2 * int(np.sum(prob.bl_ant0 != prob.bl_ant1))


@pytest.mark.parametrize("name", pc.SOLVE_CASES)
def test_recorded_plans_reach_the_branches(name):
    """The bounds cut where they are meant to, and the cases are of the kind each is there for."""
    gold = np.load(os.path.join(GOLDEN, name + ".npz"))
    prob, dtype, _, _, nvec, bounds = _case(name)
    ngrps = len(nvec)
    heavy = np.sort(nvec)[::-1]
    assert bounds["default"] == 0 and bounds["one"] == 1 and 1 < bounds["two_cs"] < bounds["two_fe"] < pc.CS_DEFAULT_BOUND
    for kind in ("cs", "fe"):
        sc = {t: dict(zip(pc.SOLVE_SCALARS, gold[f"{t}.{kind}_scalars"].tolist())) for t in TAGS}
        ch = {t: _chunks(gold[f"{t}.{kind}_chunks"]) for t in TAGS}
        assert sc["default"]["nchunks"] == 1 and ch["default"][0, :2].tolist() == [0, ngrps]
        assert sc["one"]["nchunks"] == ngrps and (ch["one"][:, 1] - ch["one"][:, 0] == 1).all()  # a group alone may exceed the bound
        assert ch["two_" + kind][0, :2].tolist() == [0, 2]  # the two heaviest groups, not a third
        for t in TAGS:
            order = gold[f"{t}.{kind}_order"]
            assert (nvec[order] == heavy).all() and (np.diff(order)[np.diff(nvec[order]) == 0] > 0).all()  # heaviest first, stable
            assert ch[t][0, 0] == 0 and ch[t][-1, 1] == ngrps and (ch[t][1:, 0] == ch[t][:-1, 1]).all()
            assert (sc[t]["x_max"] > 0) == (kind == "fe") and (sc[t]["npieces"] > 0) == (kind == "fe")
            assert (len(gold[f"{t}.{kind}_lwork"]) > 0) == (kind == "fe") and (len(gold[f"{t}.{kind}_woff"]) > 0) == (kind == "fe")
    # W counted: fit_errors' chunks are cut elsewhere than solve_coeffs' at the same bound
    cs, fe = _chunks(gold["two_fe.cs_chunks"])[:, :2], _chunks(gold["two_fe.fe_chunks"])[:, :2]
    assert cs.shape != fe.shape or (cs != fe).any()
    lwork = gold["default.fe_lwork"].reshape(-1, 4)
    npieces = int(gold["default.fe_scalars"][3])
    if name.startswith("groups"):  # multi-baseline groups over two row blocks: runs of equal tiles, several per group
        runs = lwork[lwork[:, 3] == 0]
        assert (runs[:, 2] - runs[:, 1]).max() > 1 and len(runs) > ngrps
    if name == "stream_fold_f32":  # the pieces cover the half band
        assert npieces == -(-(prob.nfreqs // 2) // 64)
    if name.startswith("dense"):  # two slices; blocks whose factor leaves LDS
        assert prob.nslices == 2 and 200 in nvec
        lds = _chunks(gold["one.cs_chunks"])[:, 6]
        assert lds.max() == pc.CS_LDS_DOUBLES * 8 and lds.min() < pc.CS_LDS_DOUBLES * 8


def _row_rule(K, L, T, nfreqs, itemsize, bound, nants):
    """solve_gain_coeffs (L = 0) / solve_gain_time_coeffs: what a row of a chunk takes, and the rows that stay under the bound."""
    n = (L if L else 1) * K
    want = (n + 2) * (n | 1)
    in_lds = want <= pc.CS_LDS_DOUBLES
    m_row = n_row = d_row = 0
    if K:
        m_row, n_row, d_row = (T * K * K if L else 0), n * n, (0 if in_lds else (n + 2) * n)
    elif L > pc.TIME_TILE:
        d_row = nfreqs * (L * (L + 1) // 2 + 2 * L)
    nrows = nants // T if L else nants
    rows = max(1, min(nrows, bound // max(1, (m_row + n_row) * itemsize + d_row * 8)))
    return [rows, int(in_lds), min(want, pc.CS_LDS_DOUBLES) * 8, n, m_row, n_row, d_row]


def _k_cross():
    """the largest K whose factor ([K + 2] rows of K | 1 doubles) stays in LDS"""
    K = 1
    while (K + 3) * ((K + 1) | 1) <= pc.CS_LDS_DOUBLES:
        K += 1
    return K


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_row_chunks_follow_the_rule(dt):
    name = "dense_split2_f32" if dt == "f32" else "dense_f64"  # 26 antennas, 256 channels
    prob, dtype, layout, kernel_path, _, _ = _case(name)
    size, nants, nfreqs = np.dtype(dtype).itemsize, prob.nants, prob.nfreqs
    kc = _k_cross()
    assert (kc + 2) * (kc | 1) <= pc.CS_LDS_DOUBLES < (kc + 3) * ((kc + 1) | 1)
    # (K, L, T): a frequency basis alone on both sides of the LDS bound; a time basis over one (n = L K on both sides) and alone, L
    # on both sides of kTimeTile
    shapes = [(1, 0, 0), (7, 0, 0), (kc, 0, 0), (kc + 1, 0, 0), (5, 3, 2), (kc // 2, 2, 13), (kc // 2 + 1, 2, 13), (0, 3, 2),
              (0, pc.TIME_TILE, 13), (0, pc.TIME_TILE + 1, 13)]
    seen = set()
    for K, L, T in shapes:
        one_row = _row_rule(K, L, T, nfreqs, size, pc.CS_DEFAULT_BOUND, nants)
        row_bytes = (one_row[4] + one_row[5]) * size + one_row[6] * 8
        nrows = nants // T if L else nants
        for bound in (0, 1, 3 * max(1, row_bytes) + 1, max(1, row_bytes) * nrows):
            got = pc.solve_plan(_lib.load().cal_debug_solve_plan, prob, dtype, layout, kernel_path, bound, [pc.WHAT_ROW_CHUNKS], (K, L, T))["row_chunks"]
            want = _row_rule(K, L, T, nfreqs, size, bound or pc.CS_DEFAULT_BOUND, nants)
            assert got.tolist() == want, ((K, L, T), bound, dict(zip(pc.ROW_SCALARS, got.tolist())))
            seen.add((want[0] == 1, 1 < want[0] < nrows, want[0] == nrows, bool(want[1]), want[6] > 0))
    assert {s[:3] for s in seen} >= {(True, False, False), (False, True, False), (False, False, True)}  # one row, several, all
    assert {s[3] for s in seen} == {True, False} and {s[4] for s in seen} == {True, False}


def test_refusals():
    from calamity_amd.solver import problem_desc

    prob, dtype, layout, kernel_path, _, _ = _case("groups_stream_f32")
    d, keep = problem_desc(prob, dtype, layout, kernel_path)
    lib = _lib.load()
    buf, n = np.zeros(1 << 16, np.uint8), C.c_int64(0)

    def call(bound, what):
        return lib.cal_debug_solve_plan(_lib.CAL_F32, C.byref(d), bound, what, buf.ctypes.data_as(C.c_void_p), buf.nbytes, C.byref(n))

    for bound, what, message in ((-1, 0, "cal_debug_solve_plan: negative bound"), (0, 7, "cal_debug_solve_plan: what = 7"),
                                 (0, 22, "cal_debug_solve_plan: what = 22"), (0, -1, "cal_debug_solve_plan: what = -1"),
                                 (0, 30, "cal_debug_solve_plan: what = 30 takes K, L, T (K + L > 0; T divides nants) in the first 24 bytes of out")):
        assert call(bound, what) == _lib.CAL_ERR_INVALID
        assert lib.cal_last_error().decode() == message
    # a bound of 0 is the default bound, as in set_coeff_solve_scratch
    for what in GROUP_WHATS:
        assert call(0, what) == 0
        a = buf[: n.value].tobytes()
        assert call(pc.CS_DEFAULT_BOUND, what) == 0 and buf[: n.value].tobytes() == a
    del keep
