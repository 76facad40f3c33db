"""cal_solver_solve_coeffs on the device against a plain NumPy restatement (include/calamity_hip.h): the foreground coefficients in
closed form, one symmetric solve per fitting group with the gains held fixed.

Group gamma has nvec complex coefficients c; its baselines b have antennas (i, j) and the row block A_b [nfreqs][nvec]; m = A c at
the solver's coefficients, d, w its data and weights, g its full gains:

    G = g_i conj(g_j)        u = w conj(G) (d - G m)        q = w |G|^2
    N = sum_b A_b^T diag(q_b) A_b        rhs = sum_b A_b^T u_b        (N + ridge tr N / nvec I) delta = rhs
    c_new = c + damping delta            a group with tr N <= 0 keeps its coefficients

The restatement works in fp64 on the inputs the solver holds (cast to its dtype first).  Tolerances are the project's own
(tests/test_gpu_fit_quality.py: TOL): planes (c_r and c_i after the call) fp64 1e-10, fp32 1e-4 of the plane's largest element;
losses fp64 1e-10, fp32 1e-5.  Every parity input is asserted to have cond(N) <= 1e4, so that an ill-conditioned input cannot pass as
a tolerance problem (an fp32 Gram with an fp64 factorisation stays at 2e-8 ... 4e-6 of the plane on these shapes; the wider blocks of
tests/test_gpu_coeff_solve_shapes.py reach 1.6e-5 at cond(N) = 1e3)."""
import copy
import functools

import numpy as np
import pytest

from calamity_amd import _lib, batched, modeling, synthetic
from calamity_amd.problem import FitProblem
from test_gpu_fit_quality import TOL, edge_problem, perturbed, plane_err, solver_of, wide_problem
from test_gpu_fold import mirror_block, small_problem

pytestmark = pytest.mark.gpu

COND_MAX = 1e4


def restated(p, params, dtype, ridge=1e-6, damping=1.0, gains=None, niters=1):
    """One call in fp64 arithmetic on inputs rounded to ``dtype``.  Returns (c_new, chi-square after, cond(N) of the solved groups,
    indices of the singular groups).  ``gains``: (g_r, g_i) to evaluate at instead of the parameters' (a gain basis: the expanded ones)."""
    cast = lambda a: np.asarray(a).astype(dtype).astype(np.float64)  # noqa: E731
    d = cast(p.data_r) + 1j * cast(p.data_i)
    w = cast(p.wgts)
    g_r, g_i = gains if gains is not None else (params["g_r"], params["g_i"])
    g = cast(g_r) + 1j * cast(g_i)
    c = cast(params["c_r"]) + 1j * cast(params["c_i"])
    G = g[p.bl_ant0] * np.conj(g[p.bl_ant1])
    q = w * np.abs(G) ** 2
    coff = p.grp_coff
    F = p.nfreqs
    blocks = [cast(blk) for blk in p.basis]
    rows = lambda b, grp: blocks[p.grp_basis[grp]][p.bl_rowblk[b] * F : (p.bl_rowblk[b] + 1) * F]  # noqa: E731

    def model(cc):
        m = np.empty((p.nbls, F), dtype=np.complex128)
        for grp in range(p.ngrps):
            for b in range(p.grp_bl_start[grp], p.grp_bl_start[grp + 1]):
                m[b] = rows(b, grp) @ cc[coff[grp] : coff[grp + 1]]
        return m

    for _ in range(niters):
        u = w * np.conj(G) * (d - G * model(c))
        conds, singular = [], []
        c_new = c.copy()
        for grp in range(p.ngrps):
            nv = coff[grp + 1] - coff[grp]
            N = np.zeros((nv, nv))
            rhs = np.zeros(nv, dtype=np.complex128)
            for b in range(p.grp_bl_start[grp], p.grp_bl_start[grp + 1]):
                A = rows(b, grp)
                N += A.T @ (q[b][:, None] * A)
                rhs += A.T @ u[b]
            tr = np.trace(N)
            if not tr > 0:
                singular.append(grp)
                continue
            conds.append(np.linalg.cond(N))
            c_new[coff[grp] : coff[grp + 1]] += damping * np.linalg.solve(N + ridge * tr / nv * np.eye(nv), rhs)
        c = c_new
    chisq = float(np.sum(w * np.abs(d - G * model(c)) ** 2))
    return c, chisq, conds, singular


def check_coeffs(s, want, dtype, label):
    c_r, c_i = s.get_params()[2:]
    errs = (plane_err(c_r, want.real), plane_err(c_i, want.imag))
    print(f"{label}: c_r {errs[0]:.2e}  c_i {errs[1]:.2e}")
    assert np.all(np.isfinite(c_r)) and np.all(np.isfinite(c_i)), label
    assert max(errs) <= TOL[np.dtype(dtype)]["plane"], (label, errs)
    return c_r, c_i


def check_loss(s, want, dtype, label):
    got = float(s.fit_quality()["chisq_bl"].sum())
    err = abs(got - want) / want
    print(f"{label}: chi-square {got:.6e} against {want:.6e}: {err:.2e}")
    assert err <= TOL[np.dtype(dtype)]["loss"], (label, err)
    return got


# ---- parity of ONE solve
@pytest.mark.parametrize("ridge", [0.0, 1e-6])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("layout", ["stream", "shared"])
@pytest.mark.parametrize("shape", [(5, 48), (7, 200), (12, 129), (6, 300)])
def test_one_solve_equals_the_numpy_restatement(shape, layout, dtype, ridge):
    """nvec is 7 ... 34 on these shapes: one to three MFMA tiles with ragged tails."""
    p, params = edge_problem(*shape)
    label = f"{shape} {layout} {np.dtype(dtype).name} ridge {ridge:g}"
    want, chisq, conds, singular = restated(p, params, dtype, ridge=ridge)
    print(f"{label}: nvec {sorted({b.shape[1] for b in p.basis})}, largest cond(N) {max(conds):.2e}")
    assert max(conds) <= COND_MAX and singular == [0] and not np.any(p.wgts[0])
    s = solver_of(p, params, dtype, layout)
    before = s.get_params()
    res = s.solve_coeffs(ridge=ridge)
    assert res == {"nsolved": p.ngrps - 1, "nsingular": 1}, res
    c_r, c_i = check_coeffs(s, want, dtype, label)
    nv0 = p.grp_coff[1]
    np.testing.assert_array_equal(c_r[:nv0], before[2][:nv0])  # the wholly flagged baseline: the bits it had
    np.testing.assert_array_equal(c_i[:nv0], before[3][:nv0])
    assert np.all(c_r[nv0:] != before[2][nv0:])
    after = s.get_params()
    np.testing.assert_array_equal(after[0], before[0])  # the gains are not touched
    np.testing.assert_array_equal(after[1], before[1])
    check_loss(s, chisq, dtype, label)
    s.close()


@pytest.mark.parametrize("layout", ["stream", "shared"])
def test_a_second_solve_at_the_same_gains_changes_nothing(layout):
    """fp64, ridge 0, damping 1: the step lands on the minimum of the quadratic."""
    p, params = edge_problem(7, 200)
    s = solver_of(p, params, np.float64, layout)
    s.solve_coeffs(ridge=0.0)
    first, chi1 = s.get_params()[2:], float(s.fit_quality()["chisq_bl"].sum())
    s.solve_coeffs(ridge=0.0)
    second, chi2 = s.get_params()[2:], float(s.fit_quality()["chisq_bl"].sum())
    moves = [plane_err(b, a) for a, b in zip(first, second)]
    print(f"{layout}: second solve moves the planes by {moves[0]:.2e}, {moves[1]:.2e}; chi-square {chi1:.12e} -> {chi2:.12e}")
    assert max(moves) < 1e-9
    assert abs(chi1 - chi2) < 1e-10 * chi1
    s.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_one_solve_on_780_groups(dtype):
    p, params = wide_problem()
    want, chisq, conds, singular = restated(p, params, dtype)
    assert max(conds) <= COND_MAX and not singular and p.ngrps == 780
    s = solver_of(p, params, dtype)
    assert s.solve_coeffs() == {"nsolved": 780, "nsingular": 0}
    check_coeffs(s, want, dtype, f"(40, 64) {np.dtype(dtype).name}")
    check_loss(s, chisq, dtype, f"(40, 64) {np.dtype(dtype).name}")
    s.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("layout", ["stream", "shared"])
def test_one_solve_on_a_fitting_group_of_several_baselines(layout, dtype):
    p0, _, start0 = synthetic.make_problem(7, 200, f0=150e6, df=400e3, seed=13)
    p, start = synthetic.add_redundant_group(p0, start0, np.random.default_rng(1), nred=3)
    assert np.diff(p.grp_bl_start).max() == 3
    params = perturbed(p, start, seed=14)
    want, chisq, conds, singular = restated(p, params, dtype)
    assert max(conds) <= COND_MAX and not singular
    s = solver_of(p, params, dtype, layout)
    assert s.solve_coeffs() == {"nsolved": p.ngrps, "nsingular": 0}
    check_coeffs(s, want, dtype, f"redundant group {layout} {np.dtype(dtype).name}")
    check_loss(s, chisq, dtype, f"redundant group {layout} {np.dtype(dtype).name}")
    s.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_an_autocorrelation_row_is_solved_like_any_row(dtype):
    p0, params0 = edge_problem(5, 48)
    rng = np.random.default_rng(9)
    nv = p0.basis[0].shape[1]
    w_auto = np.full((1, p0.nfreqs), p0.wgts.max())
    p = FitProblem(nants=p0.nants, nfreqs=p0.nfreqs, basis=p0.basis, grp_basis=np.concatenate([p0.grp_basis, [0]]).astype(np.int32),
                   grp_bl_start=np.arange(p0.nbls + 2, dtype=np.int32), bl_ant0=np.concatenate([p0.bl_ant0, [2]]).astype(np.int32),
                   bl_ant1=np.concatenate([p0.bl_ant1, [2]]).astype(np.int32), bl_rowblk=np.zeros(p0.nbls + 1, dtype=np.int32),
                   data_r=np.concatenate([p0.data_r, rng.standard_normal((1, p0.nfreqs))]),
                   data_i=np.concatenate([p0.data_i, rng.standard_normal((1, p0.nfreqs))]), wgts=np.concatenate([p0.wgts, w_auto]))
    p.validate()
    params = dict(params0, c_r=np.concatenate([params0["c_r"], rng.standard_normal(nv)]), c_i=np.concatenate([params0["c_i"], rng.standard_normal(nv)]))
    want, chisq, conds, singular = restated(p, params, dtype)
    assert max(conds) <= COND_MAX and singular == [0]
    s = solver_of(p, params, dtype)
    before = s.get_params()
    assert s.solve_coeffs() == {"nsolved": p.ngrps - 1, "nsingular": 1}
    c_r, _ = check_coeffs(s, want, dtype, f"autocorrelation {np.dtype(dtype).name}")
    assert np.all(c_r[-nv:] != before[2][-nv:])
    check_loss(s, chisq, dtype, f"autocorrelation {np.dtype(dtype).name}")
    s.close()


# ---- tile widths, folded and full tiles, slices
FOLD_CASES = {
    "512": dict(nfreqs=512, nvec=(3, 16, 9), groups=[0, 1, 2, 1, 0], nslices=1, folded={np.float32: 1}),
    "1024": dict(nfreqs=1024, nvec=(40, 100, 200), groups=[0, 1, 2] * 2, nslices=1, folded={np.float32: 1, np.float64: 1}),
    "192": dict(nfreqs=192, nvec=(17, 33, 48), groups=[0, 1, 2, 1], nslices=1, folded={np.float32: 0, np.float64: 0}),
    "256": dict(nfreqs=256, nvec=(15, 31), groups=[0, 1, 0, 1] * 2, nslices=2, folded={np.float32: 1, np.float64: 1}),
}


@functools.lru_cache(maxsize=None)
def fold_case(name):
    case = FOLD_CASES[name]
    rng = np.random.default_rng(30 + case["nfreqs"])
    blocks = [mirror_block(rng, case["nfreqs"], n) for n in case["nvec"]]
    nsl = case["nslices"]
    groups = case["groups"][: len(case["groups"]) // nsl]
    return small_problem(blocks, groups, seed=31 + case["nfreqs"], nslices=nsl)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", list(FOLD_CASES))
def test_tile_widths_folded_and_full_tiles(name, dtype):
    """"192": half the band is not a whole tile, so the tiles stay full; "1024": three tile widths; "256": two time slices, and a
    masked slice keeps its bits."""
    case = FOLD_CASES[name]
    p, start = fold_case(name)
    want, chisq, conds, singular = restated(p, start, dtype)
    print(f"{name} {np.dtype(dtype).name}: largest cond(N) {max(conds):.2e}")
    assert max(conds) <= COND_MAX and not singular
    for path in ("auto", "general_full"):
        s = solver_of(p, start, dtype, "stream", path)
        folded = s.timing_get()["basis_folded"]
        if path == "general_full":
            assert folded == 0
        elif dtype in case["folded"]:
            assert folded == case["folded"][dtype], (name, folded)
        label = f"{name} {path} (folded {folded}) {np.dtype(dtype).name}"
        if case["nslices"] == 2:
            before = s.get_params()
            half = p.ncoeffs // 2
            res = s.solve_coeffs(slice_mask=[1, 0])
            assert res == {"nsolved": p.ngrps // 2, "nsingular": 0}, res
            got = s.get_params()
            for k in (2, 3):
                np.testing.assert_array_equal(got[k][half:], before[k][half:])
            errs = (plane_err(got[2][:half], want.real[:half]), plane_err(got[3][:half], want.imag[:half]))
            print(f"{label}: slice 0 alone c_r {errs[0]:.2e}  c_i {errs[1]:.2e}")
            assert max(errs) <= TOL[np.dtype(dtype)]["plane"]
            s.set_params(c_r=start["c_r"], c_i=start["c_i"])
        assert s.solve_coeffs() == {"nsolved": p.ngrps, "nsingular": 0}
        check_coeffs(s, want, dtype, label)
        check_loss(s, chisq, dtype, label)
        s.close()


# ---- chunks, reproducibility
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_several_chunks_give_the_bits_of_one(dtype):
    """A scratch bound of one byte: every group is a chunk of its own."""
    p, start = fold_case("1024")
    got = []
    for bound in (0, 1):
        s = solver_of(p, start, dtype, "stream")
        s._set_coeff_solve_scratch(bound)
        assert s.solve_coeffs() == {"nsolved": p.ngrps, "nsingular": 0}
        got.append(s.get_params()[2:])
        s.close()
    for a, b in zip(*got):
        np.testing.assert_array_equal(a, b)
    assert not np.array_equal(got[0][0], np.asarray(start["c_r"], dtype=dtype))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_two_calls_give_the_same_bits_and_touch_nothing_else(dtype):
    p, params = edge_problem(12, 129)
    runs = []
    for _ in range(2):
        s = solver_of(p, params, dtype, "stream")
        s.set_optimizer("Adam", learning_rate=1e-2)
        s.run(3, tol=0.0, use_min=True)
        before, mom0, snap0 = s.get_params(), s.get_moments(), s.get_params(1)
        s.solve_coeffs(niters=2)
        after, mom1, snap1 = s.get_params(), s.get_moments(), s.get_params(1)
        np.testing.assert_array_equal(after[0], before[0])
        np.testing.assert_array_equal(after[1], before[1])
        for k in mom0:
            np.testing.assert_array_equal(mom1[k], mom0[k], err_msg=k)
        for a, b in zip(snap1, snap0):
            np.testing.assert_array_equal(a, b)
        runs.append(after[2:])
        s.close()
    for a, b in zip(*runs):
        np.testing.assert_array_equal(a, b)


# ---- run continuation and moments
@pytest.mark.parametrize("config", ["adam", "graph", "kernels", "gain_basis"])
def test_a_run_continued_after_an_all_zero_mask_is_bit_identical(config):
    p, params = edge_problem(12, 129)
    losses, final = {}, {}
    for with_call in (False, True):
        s = solver_of(p, params, np.float32)
        s.set_launch_mode({"graph": "graph", "kernels": "kernels"}.get(config, "auto"))
        if config == "gain_basis":
            s.set_gain_basis(np.array(modeling.gain_dpss_basis(150e6 + 400e3 * np.arange(p.nfreqs), 100.0)))
        s.set_optimizer("Adam", learning_rate=1e-2)
        first = s.run(20, tol=0.0)[0]
        if with_call:
            assert s.solve_coeffs(slice_mask=[0]) == {"nsolved": 0, "nsingular": 0}
        second = s.run(20, tol=0.0)[0]
        losses[with_call] = np.concatenate([first, second])
        final[with_call] = s.get_params()
        s.close()
    assert len(losses[True]) == 40
    np.testing.assert_array_equal(losses[True], losses[False])
    for a, b in zip(final[True], final[False]):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_with_a_gain_basis_attached(dtype):
    """The solve reads the expanded gains and writes neither them nor y."""
    p, params = edge_problem(12, 129)
    s = solver_of(p, params, dtype)
    s.set_gain_basis(np.array(modeling.gain_dpss_basis(150e6 + 400e3 * np.arange(p.nfreqs), 100.0)))
    s.set_optimizer("Adam", learning_rate=1e-2)
    s.run(3, tol=0.0)  # y != 0: the gains are g0 + B y
    before, y0 = s.get_params(), s.get_gain_coeffs()
    assert np.any(y0[0] != 0)
    cur = dict(params, c_r=before[2], c_i=before[3])
    want, chisq, conds, singular = restated(p, cur, dtype, gains=before[:2])
    assert max(conds) <= COND_MAX and singular == [0]
    assert s.solve_coeffs() == {"nsolved": p.ngrps - 1, "nsingular": 1}
    check_coeffs(s, want, dtype, f"gain basis {np.dtype(dtype).name}")
    after, y1 = s.get_params(), s.get_gain_coeffs()
    for a, b in zip(after[:2] + y1, before[:2] + y0):
        np.testing.assert_array_equal(a, b)
    check_loss(s, chisq, dtype, f"gain basis {np.dtype(dtype).name}")
    s.run(2, tol=0.0)  # and the fit goes on
    s.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("with_freq", [False, True], ids=["time", "time_x_freq"])
def test_with_a_gain_time_basis_attached(with_freq, dtype):
    """Three times of seven antennas as one fit, g = g0 + Bt (x) y or g0 + Bt (x) Bf y: the solve reads the expanded gains and writes
    neither them nor y."""
    from test_gain_time_basis_host import TIMES_60, joint_case

    ntimes = 3
    p, start = joint_case(ntimes=ntimes, nants=7, nfreqs=40)[:2]
    assert p.nants == 7 * ntimes
    label = f"gain time basis{' x frequency basis' if with_freq else ''} {np.dtype(dtype).name}"
    s = solver_of(p, start, dtype, "stream")
    if with_freq:
        s.set_gain_basis(np.array(modeling.gain_dpss_basis(150e6 + 400e3 * np.arange(p.nfreqs), 100.0)))
    s.set_gain_time_basis(np.array(modeling.gain_time_dpss_basis(TIMES_60[:ntimes], 400.0)))
    s.set_optimizer("Adam", learning_rate=1e-2)
    s.run(3, tol=0.0)  # y != 0
    before, y0 = s.get_params(), s.get_gain_coeffs()
    assert y0[0].shape[:2] == (7, 2) and np.any(y0[0] != 0) and np.any(before[0] != np.asarray(start["g_r"], dtype=dtype))
    cur = dict(start, c_r=before[2], c_i=before[3])
    want, chisq, conds, singular = restated(p, cur, dtype, gains=before[:2])
    print(f"{label}: largest cond(N) {max(conds):.2e}")
    assert max(conds) <= COND_MAX and not singular
    assert s.solve_coeffs() == {"nsolved": p.ngrps, "nsingular": 0}
    check_coeffs(s, want, dtype, label)
    after, y1 = s.get_params(), s.get_gain_coeffs()
    for a, b in zip(after[:2] + y1, before[:2] + y0):
        np.testing.assert_array_equal(a, b)
    check_loss(s, chisq, dtype, label)
    s.run(2, tol=0.0)  # and the fit goes on
    s.close()


@pytest.mark.parametrize("optimizer", ["Adam", "Adagrad"])
def test_reset_coeff_moments_restores_the_slots_of_set_optimizer(optimizer):
    """Adagrad's accumulator starts at 0.1, not 0."""
    p, params = edge_problem(7, 200)
    s = solver_of(p, params, np.float64)
    with pytest.raises(_lib.CalamityHipError) as err:  # no optimizer yet
        s.solve_coeffs(reset_coeff_moments=True)
    assert err.value.code == _lib.CAL_ERR_STATE
    s.set_optimizer(optimizer, learning_rate=1e-2)
    fresh = s.get_moments()
    s.run(5, tol=0.0)
    moved = s.get_moments()
    assert np.any(moved["cm_r"] != fresh["cm_r"]) or np.any(moved["cv_r"] != fresh["cv_r"])
    s.solve_coeffs()  # without the flag: the slots stay
    kept = s.get_moments()
    for k in fresh:
        np.testing.assert_array_equal(kept[k], moved[k], err_msg=k)
    s.solve_coeffs(reset_coeff_moments=True)
    got = s.get_moments()
    for k in ("cm_r", "cm_i", "cv_r", "cv_i"):
        np.testing.assert_array_equal(got[k], fresh[k], err_msg=k)
    for k in ("gm_r", "gm_i", "gv_r", "gv_i", "t"):
        np.testing.assert_array_equal(got[k], moved[k], err_msg=k)
    assert got["t"] == 5
    s.run(2, tol=0.0)  # and the fit goes on
    s.close()


@functools.lru_cache(maxsize=None)
def three_slices():
    """The blocks of the "256" case in three time slices of four groups each."""
    rng = np.random.default_rng(286)
    return small_problem([mirror_block(rng, 256, n) for n in FOLD_CASES["256"]["nvec"]], [0, 1, 0, 1], seed=287, nslices=3)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("mask", [[1, 0, 1], [0, 1, 1]])
@pytest.mark.parametrize("optimizer", ["Adam", "Adagrad"])
def test_a_mask_with_reset_coeff_moments_restores_the_selected_slices_only(optimizer, mask, dtype):
    """What the batched driver calls: [1, 0, 1] are two runs of one selected slice, [0, 1, 1] one run of two.  The selected slices are
    solved and their coefficient slots start over; the other slice keeps coefficients and slots to the bit; gain slots and t stay."""
    p, start = three_slices()
    label = f"{optimizer} mask {mask} {np.dtype(dtype).name}"
    s = solver_of(p, start, dtype, "stream")
    s.set_optimizer(optimizer, learning_rate=1e-2)
    fresh = s.get_moments()
    if optimizer == "Adagrad":
        assert np.all(fresh["cv_r"] == dtype(0.1)) and np.all(fresh["cv_i"] == dtype(0.1)) and not np.any(fresh["cm_r"])
    s.run_slices(4, tol=0.0)
    moved, before = s.get_moments(), s.get_params()
    per, ngrps = p.ncoeffs // 3, p.ngrps // 3
    assert p.grp_coff[ngrps] == per and p.grp_coff[2 * ngrps] == 2 * per
    parts = [slice(t * per, (t + 1) * per) for t in range(3)]
    for part in parts:
        assert np.any(moved["cv_r"][part] != fresh["cv_r"][part]) and np.any(moved["cv_i"][part] != fresh["cv_i"][part])
    want, _, conds, singular = restated(p, dict(zip(("g_r", "g_i", "c_r", "c_i"), before)), dtype)
    print(f"{label}: largest cond(N) {max(conds):.2e}")
    assert max(conds) <= COND_MAX and not singular
    res = s.solve_coeffs(slice_mask=mask, reset_coeff_moments=True)
    assert res == {"nsolved": sum(mask) * ngrps, "nsingular": 0}, res
    got, after = s.get_moments(), s.get_params()
    for t, part in enumerate(parts):
        for k in ("cm_r", "cm_i", "cv_r", "cv_i"):
            np.testing.assert_array_equal(got[k][part], (fresh if mask[t] else moved)[k][part], err_msg=f"{k} of slice {t}")
        for k, ref in ((2, want.real), (3, want.imag)):
            if mask[t]:
                err = plane_err(after[k][part], ref[part])
                print(f"{label}: slice {t} plane {k} {err:.2e}")
                assert err <= TOL[np.dtype(dtype)]["plane"] and np.all(after[k][part] != before[k][part])
            else:
                np.testing.assert_array_equal(after[k][part], before[k][part], err_msg=f"plane {k} of slice {t}")
    for k in ("gm_r", "gm_i", "gv_r", "gv_i", "t"):
        np.testing.assert_array_equal(got[k], moved[k], err_msg=k)
    assert got["t"] == 4
    np.testing.assert_array_equal(after[0], before[0])
    np.testing.assert_array_equal(after[1], before[1])
    assert len(s.run_slices(2, tol=0.0)[1][0]) == 2  # and the fit goes on
    s.close()


# ---- conditioning and convergence
@functools.lru_cache(maxsize=None)
def seed207():
    p, _, start = synthetic.make_problem(7, 200, f0=150e6, df=400e3, seed=207)
    return p, start


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_flagged_band_edge_is_solved_with_the_ridge(dtype):
    """Channels [0, 20) flagged on every baseline: cond(N) = 2e8.  The restatement with ridge 1e-6 gives 3.5204e-2 from the unity-gain
    start; an fp32 Gram with an fp64 factorisation differs from it by 1.8e-5 relative, so the bounds of 1e-3 (fp32) and 1e-6 (fp64)
    leave the device's own summation order a margin of 50."""
    p0, start = seed207()
    p = copy.copy(p0)
    p.wgts = p0.wgts.copy()
    p.wgts[:, 0:20] = 0.0
    want, chisq, conds, singular = restated(p, start, dtype)
    print(f"largest cond(N) {max(conds):.2e}; restated chi-square {chisq:.6e}")
    assert not singular
    s = solver_of(p, start, dtype)
    chi0 = float(s.fit_quality()["chisq_bl"].sum())
    assert s.solve_coeffs(ridge=1e-6) == {"nsolved": p.ngrps, "nsingular": 0}
    c_r, c_i = s.get_params()[2:]
    assert np.all(np.isfinite(c_r)) and np.all(np.isfinite(c_i))
    chi1 = float(s.fit_quality()["chisq_bl"].sum())
    dev = abs(chi1 - chisq) / chisq
    print(f"{np.dtype(dtype).name}: chi-square {chi0:.6e} -> {chi1:.6e}; restated {chisq:.6e}; deviation {dev:.2e}")
    assert chi1 < chi0
    assert dev <= (1e-3 if dtype == np.float32 else 1e-6)
    s.close()
    if dtype == np.float32:
        # without the ridge an fp32 Gram may meet non-positive pivots: every group is either solved or left alone
        s = solver_of(p, start, dtype)
        before = s.get_params()[2:]
        res = s.solve_coeffs(ridge=0.0)
        after = s.get_params()[2:]
        print(f"ridge 0, float32: {res}")
        assert res["nsolved"] + res["nsingular"] == p.ngrps
        coff = p.grp_coff
        kept = sum(all(np.array_equal(a[coff[g] : coff[g + 1]], b[coff[g] : coff[g + 1]]) for a, b in zip(after, before)) for g in range(p.ngrps))
        assert kept == res["nsingular"]
        s.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_alternating_least_squares(dtype):
    """Six rounds of (coefficient solve, five half-damped StefCal sweeps) from the start values.  The restatement falls to 1/50 of the
    start after round 1; the bound is 1/20.  Measured on an MI355X: see DESIGN.md section 3.10."""
    from test_gpu_gain_solve import restated as restated_gains

    p, start = seed207()
    cur = {k: np.asarray(v, dtype=dtype).astype(np.float64) for k, v in start.items()}
    ref = []
    for _ in range(6):
        c = restated(p, cur, dtype)[0]
        cur = dict(cur, c_r=np.ascontiguousarray(c.real), c_i=np.ascontiguousarray(c.imag))
        g, chis, _ = restated_gains(p, cur, dtype, nsweeps=5, damping=0.5)
        cur = dict(cur, g_r=np.ascontiguousarray(g.real), g_i=np.ascontiguousarray(g.imag))
        ref.append(chis[-1])
    s = solver_of(p, start, dtype)
    chi = [float(s.fit_quality()["chisq_bl"].sum())]
    for _ in range(6):
        assert s.solve_coeffs()["nsingular"] == 0
        mid = float(s.fit_quality()["chisq_bl"].sum())
        s.solve_gains(5)
        chi.append(float(s.fit_quality()["chisq_bl"].sum()))
        assert mid <= chi[-2] * (1 + TOL[np.dtype(dtype)]["loss"]) and chi[-1] <= mid * (1 + TOL[np.dtype(dtype)]["loss"])
    s.close()
    dev = abs(chi[-1] - ref[-1]) / ref[-1]
    print(f"{np.dtype(dtype).name}: chi-square " + " ".join(f"{c:.3e}" for c in chi) + f"; restated " + " ".join(f"{c:.3e}" for c in ref) +
          f"; deviation after round 6 {dev:.2e}")
    assert chi[1] < chi[0] / 20
    assert dev <= (1e-2 if dtype == np.float32 else 1e-6)


# ---- error codes
def test_wrong_arguments_and_wrong_state_are_reported():
    from calamity_amd.solver import HipFitSolver

    p, params = edge_problem(5, 48)
    s = solver_of(p, params, np.float64)
    for kw in (dict(niters=0), dict(damping=0.0), dict(damping=1.5), dict(ridge=-1e-6), dict(ridge=float("nan"))):
        with pytest.raises(_lib.CalamityHipError) as err:
            s.solve_coeffs(**kw)
        assert err.value.code == _lib.CAL_ERR_INVALID, kw
    s.solve_coeffs(damping=1.0, ridge=0.0)  # the closed ends
    with pytest.raises(ValueError):
        s.solve_coeffs(slice_mask=[1, 0])
    s.close()
    shell = copy.copy(p)
    shell.data_r = shell.data_i = shell.wgts = None
    for missing in ("gains", "coefficients"):
        s = HipFitSolver(dtype=np.float64)
        s.set_problem(shell)
        s.set_data(p.data_r, p.data_i, p.wgts)
        if missing == "gains":
            s.set_params(c_r=params["c_r"], c_i=params["c_i"])
        else:
            s.set_params(g_r=params["g_r"], g_i=params["g_i"])
        with pytest.raises(_lib.CalamityHipError) as err:
            s.solve_coeffs()
        assert err.value.code == _lib.CAL_ERR_STATE, missing
        s.close()
