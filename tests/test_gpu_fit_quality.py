"""cal_solver_fit_quality on the device against a plain NumPy restatement (include/calamity_hip.h):

    e[b][f] = w[b][f] |d[b][f] - g_i[f] conj(g_j[f]) (A c)[b][f]|^2
    chisq_bl[b] = sum_f e,  wsum_bl[b] = sum_f w,  chisq_ant[a][f] = sum_{b with a} e,  wsum_ant[a][f] = sum_{b with a} w

The restatement works in fp64 on the inputs the solver holds (cast to its dtype first).  Parameters are the start values plus a
perturbation of about 10 %, so that |residual| ~ |data|: a converged fit would make the fp32 residual a cancellation, which is not
what is tested here.  Tolerances are the project's own (tests/test_gpu_fp32_families.py): fp64 1e-10; fp32
1e-5 for sums of the loss kind, 1e-4 for every plane relative to its largest element.  The sums of weights involve no product:
1e-12."""
import copy
import functools

import numpy as np
import pytest

from calamity_amd import _lib, batched, synthetic
from calamity_amd.problem import FitProblem

pytestmark = pytest.mark.gpu

TOL = {np.dtype(np.float64): dict(loss=1e-10, plane=1e-10), np.dtype(np.float32): dict(loss=1e-5, plane=1e-4)}
PLANES = ("chisq_ant", "wsum_ant", "chisq_bl", "wsum_bl")


def solver_of(p, params, dtype, layout="shared", kernel_path="auto"):
    from calamity_amd.solver import HipFitSolver

    s = HipFitSolver(dtype=dtype)
    s.set_problem(p, layout=layout, kernel_path=kernel_path)
    s.set_params(params["g_r"], params["g_i"], params["c_r"], params["c_i"])
    return s


def perturbed(p, start, seed):
    rng = np.random.default_rng(seed)
    gs = (p.nants, p.nfreqs)
    return dict(g_r=start["g_r"] + 0.1 * rng.standard_normal(gs), g_i=start["g_i"] + 0.1 * rng.standard_normal(gs),
                c_r=start["c_r"] * (1.0 + 0.1 * rng.standard_normal(p.ncoeffs)), c_i=start["c_i"] * (1.0 + 0.1 * rng.standard_normal(p.ncoeffs)))


def restated(p, params, dtype, data=None):
    """The four arrays and e itself, fp64 arithmetic on inputs rounded to ``dtype``."""
    cast = lambda a: np.asarray(a).astype(dtype).astype(np.float64)  # noqa: E731
    d_r, d_i, w = (cast(a) for a in (data if data is not None else (p.data_r, p.data_i, p.wgts)))
    g = cast(params["g_r"]) + 1j * cast(params["g_i"])
    c = cast(params["c_r"]) + 1j * cast(params["c_i"])
    coff = p.grp_coff
    m = np.empty((p.nbls, p.nfreqs), dtype=np.complex128)
    for grp in range(p.ngrps):
        blk = cast(p.basis[p.grp_basis[grp]])
        for b in range(p.grp_bl_start[grp], p.grp_bl_start[grp + 1]):
            rows = blk[p.bl_rowblk[b] * p.nfreqs : (p.bl_rowblk[b] + 1) * p.nfreqs]
            m[b] = rows @ c[coff[grp] : coff[grp + 1]]
    e = w * np.abs((d_r + 1j * d_i) - g[p.bl_ant0] * np.conj(g[p.bl_ant1]) * m) ** 2
    out = dict(chisq_bl=e.sum(axis=1), wsum_bl=w.sum(axis=1), chisq_ant=np.zeros((p.nants, p.nfreqs)), wsum_ant=np.zeros((p.nants, p.nfreqs)), e=e)
    for b in range(p.nbls):
        for a in {int(p.bl_ant0[b]), int(p.bl_ant1[b])}:  # (a set: an autocorrelation counts once)
            out["chisq_ant"][a] += e[b]
            out["wsum_ant"][a] += w[b]
    return out


def plane_err(got, want):
    return float(np.max(np.abs(got - want)) / max(np.max(np.abs(want)), 1e-300))


def check_parity(q, ref, dtype, label):
    tol = TOL[np.dtype(dtype)]
    errs = {k: plane_err(q[k], ref[k]) for k in PLANES}
    loss_err = abs(q["chisq_bl"].sum() - ref["chisq_bl"].sum()) / ref["chisq_bl"].sum()
    print(f"{label}: sum chisq_bl {loss_err:.2e}  " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k in PLANES:
        assert q[k].dtype == np.float64 and q[k].shape == ref[k].shape and np.all(np.isfinite(q[k])), (label, k)
    assert loss_err <= tol["loss"], label
    assert errs["chisq_ant"] <= tol["plane"] and errs["chisq_bl"] <= tol["plane"], (label, errs)
    assert errs["wsum_ant"] <= 1e-12 and errs["wsum_bl"] <= 1e-12, (label, errs)
    return errs


@functools.lru_cache(maxsize=None)
def edge_problem(nants, nfreqs):
    """The last antenna has no baseline at all, the one before it a single one (fewer list entries than waves); channel 3 is flagged
    on every baseline of antenna 1 (wsum_ant == 0 there) and baseline 0 is flagged wholly (wsum_bl == 0)."""
    i_idx, j_idx = np.triu_indices(nants, k=1)
    sel = np.where((j_idx != nants - 1) & ((j_idx != nants - 2) | (i_idx == 0)))[0]
    p, _, start = synthetic.make_problem(nants, nfreqs, f0=150e6, df=400e3, seed=nants + nfreqs, bl_sel=sel)
    p.wgts = p.wgts.copy()
    p.wgts[(p.bl_ant0 == 1) | (p.bl_ant1 == 1), 3] = 0.0
    p.wgts[0, :] = 0.0
    return p, perturbed(p, start, seed=5)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("layout", ["stream", "shared"])
@pytest.mark.parametrize("shape", [(5, 48), (7, 200), (12, 129)])
def test_parity_with_the_numpy_restatement(shape, layout, dtype):
    p, params = edge_problem(*shape)
    na = p.nants
    assert not np.any((p.bl_ant0 == na - 1) | (p.bl_ant1 == na - 1)) and np.sum((p.bl_ant0 == na - 2) | (p.bl_ant1 == na - 2)) == 1
    s = solver_of(p, params, dtype, layout)
    q = s.fit_quality()
    ref = restated(p, params, dtype)
    check_parity(q, ref, dtype, f"{shape} {layout} {np.dtype(dtype).name}")
    # flagged samples give zeros, not NaN; an antenna without baselines is all zero
    assert np.all(q["wsum_ant"][1, 3] == 0) and q["chisq_ant"][1, 3] == 0 and q["wsum_bl"][0] == 0 and q["chisq_bl"][0] == 0
    assert not np.any(q["chisq_ant"][na - 1]) and not np.any(q["wsum_ant"][na - 1])
    assert np.any(q["chisq_ant"][na - 2] > 0)
    # invariants: the unregularised loss; every baseline enters two antennas; the sums of weights
    loss = s.eval_loss()
    loss_err = abs(q["chisq_bl"].sum() - loss) / loss
    twice = plane_err(q["chisq_ant"].sum(axis=0), 2.0 * ref["e"].sum(axis=0))
    print(f"  against eval_loss {loss_err:.2e}; sum_a chisq_ant against 2 sum_b e {twice:.2e}")
    assert loss_err <= TOL[np.dtype(dtype)]["loss"] and twice <= TOL[np.dtype(dtype)]["plane"]
    s.close()


@functools.lru_cache(maxsize=None)
def wide_problem():
    p, _, start = synthetic.make_problem(40, 64, f0=150e6, df=400e3, seed=3)
    return p, perturbed(p, start, seed=6)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_parity_with_more_baselines_per_antenna_than_the_unroll(dtype):
    """39 baselines on every antenna: each wave's segment of the list is longer than its unroll of eight."""
    p, params = wide_problem()
    s = solver_of(p, params, dtype)
    check_parity(s.fit_quality(), restated(p, params, dtype), dtype, f"(40, 64) {np.dtype(dtype).name}")
    s.close()


def test_an_autocorrelation_enters_its_antenna_once():
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
    for dtype in (np.float32, np.float64):
        s = solver_of(p, params, dtype)
        q, ref = s.fit_quality(), restated(p, params, dtype)
        check_parity(q, ref, dtype, f"autocorrelation {np.dtype(dtype).name}")
        # the row's power is in antenna 2 once: taken out, antenna 2 holds what its cross-correlations give
        others = (p.bl_ant0[:-1] == 2) | (p.bl_ant1[:-1] == 2)
        assert plane_err(q["chisq_ant"][2] - ref["e"][-1], ref["e"][:-1][others].sum(axis=0)) <= TOL[np.dtype(dtype)]["plane"]
        s.close()


def test_two_calls_agree_bitwise_and_nothing_else_changes():
    p, params = edge_problem(7, 200)
    for dtype in (np.float32, np.float64):
        s = solver_of(p, params, dtype, "stream")
        s.set_optimizer("Adam", learning_rate=1e-2)
        s.run(3, use_min=True)
        before = (s.get_params(0), s.get_params(1), s.eval_loss())
        q1, q2 = s.fit_quality(), s.fit_quality()
        after = (s.get_params(0), s.get_params(1), s.eval_loss())
        for k in PLANES:
            np.testing.assert_array_equal(q1[k], q2[k], err_msg=k)
        for which in (0, 1):
            for a, b in zip(before[which], after[which]):
                np.testing.assert_array_equal(a, b)
        assert before[2] == after[2]
        s.close()


@pytest.mark.parametrize("config", ["adam", "graph", "kernels", "gain_basis"])
def test_a_run_continued_after_the_call_is_bit_identical(config):
    from calamity_amd import modeling

    p, params = edge_problem(12, 129)
    losses, final = {}, {}
    for with_call in (False, True):
        s = solver_of(p, params, np.float32)
        if config == "gain_basis":
            s.set_gain_basis(np.array(modeling.gain_dpss_basis(150e6 + 400e3 * np.arange(p.nfreqs), 100.0)))
        s.set_launch_mode({"graph": "graph", "kernels": "kernels"}.get(config, "auto"))
        s.set_optimizer("Adam", learning_rate=1e-2)
        first = s.run(20, tol=0.0)[0]
        if with_call:
            q = s.fit_quality()
            assert q["chisq_bl"].sum() > 0
        second = s.run(20, tol=0.0)[0]
        losses[with_call] = np.concatenate([first, second])
        final[with_call] = s.get_params()
        s.close()
    assert len(losses[True]) == 40
    np.testing.assert_array_equal(losses[True], losses[False])
    for a, b in zip(final[True], final[False]):
        np.testing.assert_array_equal(a, b)


def test_given_gains_equal_the_same_gains_set():
    p, params = edge_problem(7, 200)
    other = perturbed(p, dict(params), seed=11)
    for dtype in (np.float32, np.float64):
        s = solver_of(p, params, dtype)
        given = s.fit_quality(other["g_r"], other["g_i"])
        held = s.get_params()
        np.testing.assert_array_equal(held[0], np.asarray(params["g_r"], dtype=dtype))  # the solver's own gains stay
        s.set_params(other["g_r"], other["g_i"])
        as_set = s.fit_quality()
        for k in PLANES:
            np.testing.assert_array_equal(given[k], as_set[k], err_msg=k)
        assert not np.array_equal(given["chisq_bl"], solver_of(p, params, dtype).fit_quality()["chisq_bl"])
        with pytest.raises(ValueError):
            s.fit_quality(other["g_r"], None)
        s.close()


@pytest.mark.parametrize("layout", ["stream", "shared"])
def test_slices_of_one_solver_equal_single_slice_solvers(layout):
    """T = 3 slices with their own data; slice 1's data are tiny, so its loss stops changing by more than the tolerance at once and
    the slice stops while the others go on.  A stopped slice is evaluated like any other."""
    from calamity_amd.solver import HipFitSolver

    T, dtype = 3, np.float64
    parts = [synthetic.make_problem(7, 200, f0=150e6, df=400e3, seed=21, data_seed=30 + t) for t in range(T)]
    p0 = parts[0][0]
    scale = [1.0, 1e-12, 1.0]
    data = (np.concatenate([parts[t][0].data_r * scale[t] for t in range(T)]), np.concatenate([parts[t][0].data_i * scale[t] for t in range(T)]),
            np.concatenate([parts[t][0].wgts for t in range(T)]))
    pars = [perturbed(parts[t][0], parts[t][2], seed=40 + t) for t in range(T)]
    for t in range(T):
        pars[t]["c_r"], pars[t]["c_i"] = pars[t]["c_r"] * scale[t], pars[t]["c_i"] * scale[t]
    sub, _, _ = batched.replicate_slices(p0, T)
    s = HipFitSolver(dtype=dtype)
    s.set_problem(sub, layout=layout)
    s.set_data(*data)
    s.set_params(*[np.concatenate([pars[t][k] for t in range(T)]) for k in ("g_r", "g_i", "c_r", "c_i")])
    s.set_optimizer("Adam", learning_rate=1e-2)
    res = s.run_slices(10, tol=1e-20)
    assert [r[1] for r in res] == [False, True, False] and len(res[1][0]) < 10
    q = s.fit_quality()
    g_r, g_i, c_r, c_i = s.get_params()
    m_all = s.model()
    na, nb, nc = p0.nants, p0.nbls, p0.ncoeffs
    for t in range(T):
        one = HipFitSolver(dtype=dtype)
        shell = copy.copy(p0)
        shell.data_r = shell.data_i = shell.wgts = None
        one.set_problem(shell, layout=layout)
        one.set_data(*[a[t * nb : (t + 1) * nb] for a in data])
        one.set_params(g_r[t * na : (t + 1) * na], g_i[t * na : (t + 1) * na], c_r[t * nc : (t + 1) * nc], c_i[t * nc : (t + 1) * nc])
        q1 = one.fit_quality()
        m1 = one.model()
        bitwise = np.array_equal(m1[0], m_all[0][t * nb : (t + 1) * nb]) and np.array_equal(m1[1], m_all[1][t * nb : (t + 1) * nb])
        for k in PLANES:
            got = q[k][t * na : (t + 1) * na] if k.endswith("_ant") else q[k][t * nb : (t + 1) * nb]
            print(f"slice {t} {layout} {k}: model pass bitwise {bitwise}, error {plane_err(got, q1[k]):.2e}")
            if bitwise:
                np.testing.assert_array_equal(got, q1[k], err_msg=f"slice {t} {k}")
            else:
                assert plane_err(got, q1[k]) <= 1e-10, (t, k)
        assert q1["chisq_bl"].sum() > 0
        one.close()
    s.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("layout", ["stream", "shared"])
def test_fitting_groups_of_several_baselines(layout, dtype):
    p0, _, start0 = synthetic.make_problem(7, 200, f0=150e6, df=400e3, seed=13)
    p, start = synthetic.add_redundant_group(p0, start0, np.random.default_rng(1), nred=3)
    assert np.diff(p.grp_bl_start).max() == 3
    params = perturbed(p, start, seed=14)
    s = solver_of(p, params, dtype, layout)
    check_parity(s.fit_quality(), restated(p, params, dtype), dtype, f"redundant group {layout} {np.dtype(dtype).name}")
    s.close()


def test_wrong_state_is_reported():
    from calamity_amd.solver import HipFitSolver

    p, params = edge_problem(5, 48)
    shell = copy.copy(p)
    shell.data_r = shell.data_i = shell.wgts = None
    s = HipFitSolver(dtype=np.float64)
    s.set_problem(shell)
    s.set_params(params["g_r"], params["g_i"], params["c_r"], params["c_i"])
    with pytest.raises(_lib.CalamityHipError) as err:  # no data
        s.fit_quality()
    assert err.value.code == _lib.CAL_ERR_STATE
    s.set_problem(shell)
    s.set_data(p.data_r, p.data_i, p.wgts)
    s.set_params(params["g_r"], params["g_i"])
    with pytest.raises(_lib.CalamityHipError) as err:  # no coefficients
        s.fit_quality()
    assert err.value.code == _lib.CAL_ERR_STATE
    s.set_problem(shell)
    s.set_data(p.data_r, p.data_i, p.wgts)
    s.set_params(c_r=params["c_r"], c_i=params["c_i"])
    with pytest.raises(_lib.CalamityHipError) as err:  # gains neither set nor given
        s.fit_quality()
    assert err.value.code == _lib.CAL_ERR_STATE
    assert s.fit_quality(params["g_r"], params["g_i"])["chisq_bl"].sum() > 0  # given: enough
    s.close()
