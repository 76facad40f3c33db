"""cal_solver_fit_errors on the device against a plain NumPy restatement (include/calamity_hip.h): the error bars of a fit.

Baseline row b of fitting group gamma has antennas (i, j) and the row block A_b [nfreqs][nvec] with rows a_{b,f}; d, w are the
solver's data and weights, g its full gains, m = A c at its coefficients:

    G = g_i conj(g_j)        q = w |G|^2        N = sum_b A_b^T diag(q_b) A_b        N_r = N + ridge (tr N / nvec) I = L L^T
    coeff_var[k] = (N_r^-1)[k][k]      model_var[b][f] = |L^-1 a_{b,f}|^2      leverage_bl[b] = sum_f q model_var      nsamp_bl[b] = #{w != 0}
    gain_var[a][f] = 1 / den_a[f],  den_a = sum_b w |m|^2 |g_other|^2 over the cross-correlations of a; 0 where den_a <= 0

The restatement works in fp64 on the inputs the solver holds (cast to its dtype first), with np.linalg.cholesky and a triangular
solve.  Tolerances are the project's own (tests/test_gpu_fit_quality.py: TOL): every plane fp64 1e-10, fp32 1e-4 of the plane's
largest element.  Every parity input is asserted to have cond(N) <= 1e4.  An fp32 Gram emulated in NumPy with an fp64 factorisation
stays within 4e-7 (lev) and 7.6e-7 (coeff_var) on the edge problems and within 3.5e-6 and 1.1e-5 on the narrow case (cond(N) = 1e3).
With ridge = 0 the leverages of a solved group add up to its nvec: relative 1e-12 in fp64, 1e-5 in fp32 (emulated: 5e-7 at worst)."""
import copy
import functools
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from calamity_amd import _lib, batched, modeling, synthetic
from test_gpu_coeff_solve import COND_MAX
from test_gpu_coeff_solve_shapes import alternating_case, boundary_case, folded_1024, narrow_case, wide_case
from test_gpu_fit_quality import TOL, edge_problem, perturbed, plane_err, solver_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
OUTPUTS = ("coeff_var", "model_var", "leverage_bl", "nsamp_bl", "gain_var")
IDENTITY = {np.dtype(np.float64): 1e-12, np.dtype(np.float32): 1e-5}


def restated(p, params, dtype, ridge=1e-6, gains=None):
    """The six outputs in fp64 arithmetic on inputs rounded to ``dtype``, plus q, cond(N) of the solved groups and the singular groups."""
    cast = lambda a: np.asarray(a).astype(dtype).astype(np.float64)  # noqa: E731
    w = cast(p.wgts)
    g_r, g_i = gains if gains is not None else (params["g_r"], params["g_i"])
    g = cast(g_r) + 1j * cast(g_i)
    c = cast(params["c_r"]) + 1j * cast(params["c_i"])
    G = g[p.bl_ant0] * np.conj(g[p.bl_ant1])
    q = w * np.abs(G) ** 2
    coff, F = p.grp_coff, p.nfreqs
    blocks = [cast(blk) for blk in p.basis]
    rows = lambda b, grp: blocks[p.grp_basis[grp]][p.bl_rowblk[b] * F : (p.bl_rowblk[b] + 1) * F]  # noqa: E731
    out = dict(coeff_var=np.zeros(p.ncoeffs), model_var=np.zeros((p.nbls, F)), leverage_bl=np.zeros(p.nbls),
               nsamp_bl=np.count_nonzero(w, axis=1).astype(np.float64), gain_var=np.zeros((p.nants, F)), q=q, conds=[], singular=[])
    m = np.empty((p.nbls, F), dtype=np.complex128)
    for grp in range(p.ngrps):
        bls = range(p.grp_bl_start[grp], p.grp_bl_start[grp + 1])
        nv = coff[grp + 1] - coff[grp]
        N = np.zeros((nv, nv))
        for b in bls:
            A = rows(b, grp)
            m[b] = A @ c[coff[grp] : coff[grp + 1]]
            N += A.T @ (q[b][:, None] * A)
        tr = np.trace(N)
        if not tr > 0:
            out["singular"].append(grp)
            continue
        out["conds"].append(np.linalg.cond(N))
        L = np.linalg.cholesky(N + ridge * tr / nv * np.eye(nv))
        W = np.linalg.solve(L, np.eye(nv))
        out["coeff_var"][coff[grp] : coff[grp + 1]] = np.sum(W * W, axis=0)
        for b in bls:
            z = np.linalg.solve(L, rows(b, grp).T)  # L z = a_f for every channel
            out["model_var"][b] = np.sum(z * z, axis=0)
    out["leverage_bl"] = np.sum(q * out["model_var"], axis=1)
    den = np.zeros((p.nants, F))
    Q = w * np.abs(m) ** 2
    for b in range(p.nbls):
        i, j = int(p.bl_ant0[b]), int(p.bl_ant1[b])
        if i != j:
            den[i] += Q[b] * np.abs(g[j]) ** 2
            den[j] += Q[b] * np.abs(g[i]) ** 2
    out["gain_var"] = np.where(den > 0, 1.0 / np.where(den > 0, den, 1.0), 0.0)
    return out


@functools.lru_cache(maxsize=None)
def edge_reference(shape, dtype, ridge):
    p, params = edge_problem(*shape)
    return p, params, restated(p, params, dtype, ridge)


@functools.lru_cache(maxsize=None)
def case_reference(builder, dtype, ridge=1e-6):
    p, start = builder()
    return p, start, restated(p, start, dtype, ridge)


def check_outputs(got, ref, dtype, label, keys=OUTPUTS):
    tol = TOL[np.dtype(dtype)]["plane"]
    errs = {k: plane_err(got[k], ref[k]) for k in keys}
    errs["lev"] = plane_err(ref["q"] * got["model_var"], ref["q"] * ref["model_var"]) if "model_var" in keys else 0.0
    print(f"{label}: " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k in keys:
        assert got[k].dtype == np.float64 and got[k].shape == ref[k].shape and np.all(np.isfinite(got[k])), (label, k)
    if "nsamp_bl" in keys:
        np.testing.assert_array_equal(got["nsamp_bl"], ref["nsamp_bl"])
    assert max(errs.values()) <= tol, (label, errs)
    if "model_var" in keys:
        lev = ref["q"] * got["model_var"]
        assert lev.min() >= 0.0 and lev.max() <= 1.0 + 1e-6, (label, lev.min(), lev.max())
    return errs


def identity_deviation(p, got, ref):
    """Largest relative deviation of sum_{b in group} leverage_bl from nvec over the solved groups."""
    worst = 0.0
    for grp in range(p.ngrps):
        if grp in ref["singular"]:
            continue
        nv = p.grp_coff[grp + 1] - p.grp_coff[grp]
        worst = max(worst, abs(got["leverage_bl"][p.grp_bl_start[grp] : p.grp_bl_start[grp + 1]].sum() - nv) / nv)
    return worst


# ---- 1. parity of all six outputs, 2. the identity
@pytest.mark.parametrize("ridge", [0.0, 1e-6])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", ["stream", "shared"])
@pytest.mark.parametrize("shape", [(5, 48), (7, 200), (12, 129), (6, 300)])
def test_parity_with_the_numpy_restatement(shape, layout, dtype, ridge):
    p, params, ref = edge_reference(shape, dtype, ridge)
    label = f"{shape} {layout} {np.dtype(dtype).name} ridge {ridge:g}"
    print(f"{label}: nvec {sorted({b.shape[1] for b in p.basis})}, largest cond(N) {max(ref['conds']):.2e}")
    assert max(ref["conds"]) <= COND_MAX and ref["singular"] == [0] and not np.any(p.wgts[0])
    s = solver_of(p, params, dtype, layout)
    got = s.fit_errors(ridge=ridge)
    s.close()
    assert (got["nsolved"], got["nsingular"]) == (p.ngrps - 1, 1), got
    check_outputs(got, ref, dtype, label)
    nv0, na = p.grp_coff[1], p.nants
    # the wholly flagged baseline is the one singular group: zeros
    assert not np.any(got["coeff_var"][:nv0]) and not np.any(got["model_var"][0]) and got["leverage_bl"][0] == 0 and got["nsamp_bl"][0] == 0
    assert np.all(got["coeff_var"][nv0:] > 0) and np.all(got["leverage_bl"][1:] > 0)
    # the antenna without baselines, and the channel flagged on every baseline of antenna 1
    assert not np.any(got["gain_var"][na - 1]) and got["gain_var"][1, 3] == 0 and np.any(got["gain_var"][1] > 0)
    np.testing.assert_array_equal(got["gain_var"] == 0, ref["gain_var"] == 0)
    if ridge == 0.0:
        dev = identity_deviation(p, got, ref)
        print(f"{label}: sum of a group's leverage_bl against nvec, worst {dev:.2e}")
        assert dev <= IDENTITY[np.dtype(dtype)], (label, dev)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("builder", [narrow_case, boundary_case, alternating_case], ids=["narrow", "boundary", "alternating"])
def test_the_leverages_of_a_group_add_up_to_its_vectors(builder, dtype):
    p, start, ref = case_reference(builder, dtype, 0.0)
    assert max(ref["conds"]) <= COND_MAX and ref["singular"] == []
    s = solver_of(p, start, dtype, "shared")
    got = s.fit_errors(ridge=0.0)
    s.close()
    dev = identity_deviation(p, got, ref)
    lev = ref["q"] * got["model_var"]
    print(f"{builder.__name__} {np.dtype(dtype).name}: largest cond(N) {max(ref['conds']):.2e}, identity worst {dev:.2e}, lev in [{lev.min():.3e}, {lev.max():.9f}]")
    assert dev <= IDENTITY[np.dtype(dtype)], dev
    assert lev.min() >= 0.0 and lev.max() <= 1.0 + 1e-6


# ---- 3. shapes the leverage kernel can go wrong at
def run_case(builder, dtype, label, layout="shared", path="auto", folded=None, scratch=None, ridge=1e-6):
    p, start, ref = case_reference(builder, dtype, ridge)
    print(f"{label}: nvec {sorted({b.shape[1] for b in p.basis})}, largest cond(N) {max(ref['conds']):.2e}")
    assert max(ref["conds"]) <= COND_MAX and ref["singular"] == []
    s = solver_of(p, start, dtype, layout, path)
    if folded is not None:
        assert s.timing_get()["basis_folded"] == folded, label
    if scratch is not None:
        s._set_coeff_solve_scratch(scratch)
    got = s.fit_errors(ridge=ridge)
    s.close()
    assert (got["nsolved"], got["nsingular"]) == (p.ngrps, 0), (label, got)
    check_outputs(got, ref, dtype, label)
    return got


@pytest.mark.parametrize("dtype", DTYPES)
def test_w_on_both_sides_of_the_lds_bound(dtype):
    """126 and 127 vectors keep the factor in LDS, 128 is the first in scratch; with a scratch bound of one byte every group is a chunk
    of its own: the same bits."""
    got = [run_case(boundary_case, dtype, f"boundary scratch {bound} {np.dtype(dtype).name}", scratch=bound) for bound in (0, 1)]
    for k in OUTPUTS:
        np.testing.assert_array_equal(got[0][k], got[1][k], err_msg=k)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", ["stream", "shared"])
def test_both_sides_of_every_tile_width_on_a_padded_band(layout, dtype):
    run_case(narrow_case, dtype, f"narrow {layout} {np.dtype(dtype).name}", layout=layout, folded=0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_runs_that_are_interrupted_and_come_back(dtype):
    """Row blocks 0 0 1 1 0 2 inside one group, a wholly flagged row inside a merged run: its model_var is the run's, its leverage 0."""
    from test_gpu_coeff_solve_shapes import FLAGGED

    got = {layout: run_case(alternating_case, dtype, f"alternating {layout} {np.dtype(dtype).name}", layout=layout) for layout in ("stream", "shared")}
    for layout in got:
        assert got[layout]["leverage_bl"][1 + FLAGGED] == 0 and got[layout]["nsamp_bl"][1 + FLAGGED] == 0
        np.testing.assert_array_equal(got[layout]["model_var"][1 + FLAGGED], got[layout]["model_var"][FLAGGED])  # rows 3 and 4: one run on row block 1
    if dtype == np.float64:
        errs = {k: plane_err(got["stream"][k], got["shared"][k]) for k in OUTPUTS}
        print("alternating float64: stream against shared " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        assert max(errs.values()) <= 1e-10


@pytest.mark.parametrize("dtype", DTYPES)
def test_folded_and_full_tiles(dtype):
    got = {}
    for path, folded in (("auto", 1), ("general_full", 0)):
        got[path] = run_case(folded_1024, dtype, f"folded_1024 {path} {np.dtype(dtype).name}", layout="stream", path=path, folded=folded)
    errs = {k: plane_err(got["auto"][k], got["general_full"][k]) for k in OUTPUTS}
    print(f"folded_1024 {np.dtype(dtype).name}: folded against full " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) <= (1e-10 if dtype == np.float64 else TOL[np.dtype(dtype)]["plane"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_wide_blocks(dtype):
    """Up to 896 vectors: 14 blocks of 64 rows of W, the factor in scratch, three baselines on three row blocks per group."""
    run_case(wide_case, dtype, f"wide shared {np.dtype(dtype).name}", layout="shared", folded=0)


# ---- 4. groups of several baselines
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", ["stream", "shared"])
def test_fitting_groups_of_several_baselines(layout, dtype):
    p0, _, start0 = synthetic.make_problem(7, 200, f0=150e6, df=400e3, seed=13)
    p, start = synthetic.add_redundant_group(p0, start0, np.random.default_rng(1), nred=3)
    assert np.diff(p.grp_bl_start).max() == 3
    params = perturbed(p, start, seed=14)
    ref = restated(p, params, dtype)
    assert max(ref["conds"]) <= COND_MAX and ref["singular"] == []
    s = solver_of(p, params, dtype, layout)
    got = s.fit_errors()
    s.close()
    check_outputs(got, ref, dtype, f"redundant group {layout} {np.dtype(dtype).name}")
    mv = got["model_var"]
    if layout == "shared":  # one run: one product, the rows share its bits
        np.testing.assert_array_equal(mv[1], mv[0])
        np.testing.assert_array_equal(mv[2], mv[0])
    else:
        assert max(plane_err(mv[1], mv[0]), plane_err(mv[2], mv[0])) <= TOL[np.dtype(dtype)]["plane"]
    lev = ref["q"][:3] * mv[:3]
    assert not np.array_equal(lev[0], lev[1]) and not np.array_equal(lev[1], lev[2])  # they differ by their q


# ---- 5. state
@pytest.mark.parametrize("dtype", DTYPES)
def test_two_calls_agree_bitwise_and_nothing_else_changes(dtype):
    p, params = edge_problem(12, 129)
    s = solver_of(p, params, dtype, "stream")
    s.set_optimizer("Adam", learning_rate=1e-2)
    s.run(3, tol=0.0, use_min=True)
    before = (s.get_params(0), s.get_params(1), s.get_moments(), s.get_weights(), s.eval_loss())
    e1, e2 = s.fit_errors(), s.fit_errors()
    after = (s.get_params(0), s.get_params(1), s.get_moments(), s.get_weights(), s.eval_loss())
    for k in OUTPUTS:
        np.testing.assert_array_equal(e1[k], e2[k], err_msg=k)
    for which in (0, 1):
        for a, b in zip(before[which], after[which]):
            np.testing.assert_array_equal(a, b)
    for k in before[2]:
        np.testing.assert_array_equal(after[2][k], before[2][k], err_msg=k)
    np.testing.assert_array_equal(after[3], before[3])
    assert before[4] == after[4]
    # subsets of the outputs: the same bits for what they keep
    for kw in (dict(model_var=False), dict(gain_var=False), dict(model_var=False, gain_var=False), dict(coeffs=False)):
        sub = s.fit_errors(**kw)
        kept = [k for k in OUTPUTS if k in sub]
        assert len(kept) == len(OUTPUTS) - {"model_var": 1, "gain_var": 1, "coeffs": 3}[next(iter(kw))] - (len(kw) - 1), (kw, kept)
        for k in kept:
            np.testing.assert_array_equal(sub[k], e1[k], err_msg=f"{kw} {k}")
    s.close()


def test_null_pointer_subsets_through_the_c_abi():
    """Every output alone gives the bits it has in the full call; counts may be NULL."""
    import ctypes as C

    p, params = edge_problem(7, 200)
    s = solver_of(p, params, np.float32, "shared")
    full = s.fit_errors()
    for k in OUTPUTS:
        out = np.full_like(full[k], -1.0)
        args = [out.ctypes.data_as(C.c_void_p) if name == k else None for name in OUTPUTS]
        _lib.check(s._lib.cal_solver_fit_errors(s._h, 1e-6, *args, None))
        np.testing.assert_array_equal(out, full[k], err_msg=k)
    s.close()


@pytest.mark.parametrize("config", ["adam", "graph", "kernels", "gain_basis"])
def test_a_run_continued_after_the_call_is_bit_identical(config):
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
            e = s.fit_errors(gain_var=config != "gain_basis")
            assert e["leverage_bl"].sum() > 0
        second = s.run(20, tol=0.0)[0]
        losses[with_call] = np.concatenate([first, second])
        final[with_call] = s.get_params()
        s.close()
    assert len(losses[True]) == 40
    np.testing.assert_array_equal(losses[True], losses[False])
    for a, b in zip(final[True], final[False]):
        np.testing.assert_array_equal(a, b)


# ---- 6. slices
@pytest.mark.parametrize("layout", ["stream", "shared"])
def test_slices_of_one_solver_equal_single_slice_solvers(layout):
    from calamity_amd.solver import HipFitSolver

    T, dtype = 3, np.float64
    parts = [synthetic.make_problem(7, 200, f0=150e6, df=400e3, seed=21, data_seed=30 + t) for t in range(T)]
    p0 = parts[0][0]
    data = tuple(np.concatenate([getattr(parts[t][0], k) for t in range(T)]) for k in ("data_r", "data_i", "wgts"))
    pars = [perturbed(parts[t][0], parts[t][2], seed=40 + t) for t in range(T)]
    sub, _, _ = batched.replicate_slices(p0, T)
    s = HipFitSolver(dtype=dtype)
    s.set_problem(sub, layout=layout)
    s.set_data(*data)
    s.set_params(*[np.concatenate([pars[t][k] for t in range(T)]) for k in ("g_r", "g_i", "c_r", "c_i")])
    e = s.fit_errors()
    m_all = s.model()
    na, nb, nc = p0.nants, p0.nbls, p0.ncoeffs
    assert (e["nsolved"], e["nsingular"]) == (T * p0.ngrps, 0)
    for t in range(T):
        one = HipFitSolver(dtype=dtype)
        shell = copy.copy(p0)
        shell.data_r = shell.data_i = shell.wgts = None
        one.set_problem(shell, layout=layout)
        one.set_data(*[a[t * nb : (t + 1) * nb] for a in data])
        one.set_params(*[pars[t][k] for k in ("g_r", "g_i", "c_r", "c_i")])
        e1 = one.fit_errors()
        m1 = one.model()
        bitwise = np.array_equal(m1[0], m_all[0][t * nb : (t + 1) * nb]) and np.array_equal(m1[1], m_all[1][t * nb : (t + 1) * nb])
        for k in OUTPUTS:
            n = {"coeff_var": nc, "gain_var": na}.get(k, nb)
            got = e[k][t * n : (t + 1) * n]
            print(f"slice {t} {layout} {k}: model pass bitwise {bitwise}, error {plane_err(got, e1[k]):.2e}")
            if bitwise or k != "gain_var":  # (only gain_var reads the model)
                np.testing.assert_array_equal(got, e1[k], err_msg=f"slice {t} {k}")
            else:
                assert plane_err(got, e1[k]) <= 1e-10, (t, k)
        one.close()
    s.close()


# ---- 7. two workers on one GPU through the exchange hook
def _free_port():
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        return sock.getsockname()[1]


def test_two_ranks_exchange_den_only(tmp_path):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import _fit_errors_rank as X
    from calamity_amd import distributed as D

    p, params = X.build_case()
    ref = X.errors_of(p, params)
    port = _free_port()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    outs = [str(tmp_path / f"errors_rank{r}.npz") for r in range(2)]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_fit_errors_rank.py"), "--rank", str(r), "--port", str(port), "--out", outs[r]],
                              cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    logs = []
    try:
        for pr in procs:
            logs.append(pr.communicate(timeout=300)[0])
    finally:  # (whatever ends this, no rank is left behind holding the GPU)
        for pr in procs:
            if pr.poll() is None:
                pr.kill()
    for r, pr in enumerate(procs):
        assert pr.returncode == 0, f"rank {r} failed:\n{logs[r][-4000:]}\nthe other rank:\n{logs[1 - r][-2000:]}"
    shares = D.partition_groups(p.grp_nvec, p.grp_basis, np.diff(p.grp_bl_start), 2)
    coff = p.grp_coff
    for r, out in enumerate(np.load(o) for o in outs):
        grps = np.asarray(shares[r])
        cidx = np.concatenate([np.arange(coff[g], coff[g + 1]) for g in grps])
        bidx = np.concatenate([np.arange(p.grp_bl_start[g], p.grp_bl_start[g + 1]) for g in grps])
        err = plane_err(out["gain_var"], ref["gain_var"])
        print(f"rank {r}: {len(grps)} groups, gain_var against one worker's {err:.2e}; exchanges {out['exchanges'].tolist()}")
        assert err <= TOL[np.dtype(np.float64)]["plane"]
        np.testing.assert_array_equal(out["coeff_var"], ref["coeff_var"][cidx])
        for k in ("model_var", "leverage_bl", "nsamp_bl"):
            np.testing.assert_array_equal(out[k], ref[k][bidx], err_msg=k)
        assert int(out["nsolved"]) == len(grps) and int(out["nsingular"]) == 0
        assert out["exchanges"].tolist() == [[8, p.nants * p.nfreqs]]        # one float64 plane: den
        assert out["exchanges_without_gain_var"].tolist() == []              # the coefficient outputs exchange nothing


# ---- 8. gain bases, wrong state
@pytest.mark.parametrize("dtype", DTYPES)
def test_with_a_gain_basis_attached(dtype):
    p, params = edge_problem(12, 129)
    s = solver_of(p, params, dtype)
    s.set_gain_basis(np.array(modeling.gain_dpss_basis(150e6 + 400e3 * np.arange(p.nfreqs), 100.0)))
    s.set_optimizer("Adam", learning_rate=1e-2)
    s.run(3, tol=0.0)  # y != 0: the gains are g0 + B y
    before, y0 = s.get_params(), s.get_gain_coeffs()
    assert np.any(y0[0] != 0)
    ref = restated(p, dict(params, c_r=before[2], c_i=before[3]), dtype, gains=before[:2])
    assert max(ref["conds"]) <= COND_MAX and ref["singular"] == [0]
    got = s.fit_errors(gain_var=False)
    assert "gain_var" not in got and (got["nsolved"], got["nsingular"]) == (p.ngrps - 1, 1)
    check_outputs(got, ref, dtype, f"gain basis {np.dtype(dtype).name}", keys=OUTPUTS[:4])
    with pytest.raises(_lib.CalamityHipError) as err:
        s.fit_errors()
    assert err.value.code == _lib.CAL_ERR_UNSUPPORTED and "gain basis" in str(err.value)
    after, y1 = s.get_params(), s.get_gain_coeffs()
    for a, b in zip(after + y1, before + y0):
        np.testing.assert_array_equal(a, b)
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
        s.fit_errors()
    assert err.value.code == _lib.CAL_ERR_STATE
    s.set_problem(shell)
    s.set_data(p.data_r, p.data_i, p.wgts)
    s.set_params(params["g_r"], params["g_i"])
    with pytest.raises(_lib.CalamityHipError) as err:  # no coefficients
        s.fit_errors()
    assert err.value.code == _lib.CAL_ERR_STATE
    s.set_problem(shell)
    s.set_data(p.data_r, p.data_i, p.wgts)
    s.set_params(c_r=params["c_r"], c_i=params["c_i"])
    with pytest.raises(_lib.CalamityHipError) as err:  # no gains
        s.fit_errors()
    assert err.value.code == _lib.CAL_ERR_STATE
    s.set_params(params["g_r"], params["g_i"])
    with pytest.raises(_lib.CalamityHipError) as err:
        s.fit_errors(ridge=-1.0)
    assert err.value.code == _lib.CAL_ERR_INVALID
    assert s.fit_errors()["nsolved"] == p.ngrps - 1
    s.close()


# ---- 9. the numbers mean what they say
def test_model_var_is_the_scatter_of_the_fitted_model():
    """Gains fixed at truth, weights 1 / sigma^2, 64 noise realisations, each solved with solve_coeffs(ridge = 0) in fp64: the sample
    variance of A c per channel, averaged over the band, against the mean model_var.  With 64 draws a per-channel variance estimate of
    complex samples has a relative standard deviation of 1 / sqrt(64) = 12.5 %; the band average is far tighter: 25 %."""
    ndraw, sigma = 64, 0.01
    p, truth, start = synthetic.make_problem(7, 200, f0=150e6, df=400e3, seed=23)
    mask = (p.wgts != 0).astype(np.float64)
    w = mask / sigma**2
    g = truth["g"]
    G = g[p.bl_ant0] * np.conj(g[p.bl_ant1])
    coff = p.grp_coff
    A = [np.asarray(p.basis[p.grp_basis[b]], dtype=np.float64) for b in range(p.nbls)]  # one baseline per group, one row block
    clean = np.stack([G[b] * (A[b] @ truth["c"][coff[b] : coff[b + 1]]) for b in range(p.nbls)])
    rng = np.random.default_rng(24)
    noise = sigma * (rng.standard_normal((ndraw,) + clean.shape) + 1j * rng.standard_normal((ndraw,) + clean.shape)) / np.sqrt(2.0)
    # NumPy first: the weighted least-squares fit per baseline and draw
    q = w * np.abs(G) ** 2
    m_np = np.empty((ndraw,) + clean.shape, dtype=np.complex128)
    mv_np = np.empty(clean.shape)
    for b in range(p.nbls):
        N = A[b].T @ (q[b][:, None] * A[b])
        P = A[b] @ np.linalg.solve(N, A[b].T * (w[b] * np.conj(G[b]))[None, :])  # m = P d
        m_np[:, b] = (clean[b] + noise[:, b]) @ P.T
        mv_np[b] = np.einsum("fk,kf->f", A[b], np.linalg.solve(N, A[b].T))
    var_np = np.var(m_np, axis=0, ddof=1)
    print(f"NumPy: sample variance of A c, band and baseline mean {var_np.mean():.4e}; mean model_var {mv_np.mean():.4e}; ratio {var_np.mean() / mv_np.mean():.3f}")
    s = solver_of(p, dict(g_r=g.real, g_i=g.imag, c_r=start["c_r"], c_i=start["c_i"]), np.float64)
    m_dev = np.empty_like(m_np)
    for k in range(ndraw):
        d = clean + noise[k]
        s.set_data(np.ascontiguousarray(d.real), np.ascontiguousarray(d.imag), w)
        assert s.solve_coeffs(ridge=0.0) == {"nsolved": p.ngrps, "nsingular": 0}
        m_r, m_i = s.model()
        m_dev[k] = m_r + 1j * m_i
    e = s.fit_errors(ridge=0.0, gain_var=False)
    s.close()
    var_dev = np.var(m_dev, axis=0, ddof=1)
    ratio_bl = var_dev.mean(axis=1) / e["model_var"].mean(axis=1)
    print(f"device: sample variance of A c {var_dev.mean():.4e}; mean model_var {e['model_var'].mean():.4e}; ratio {var_dev.mean() / e['model_var'].mean():.3f}; "
          f"per baseline {ratio_bl.min():.3f} ... {ratio_bl.max():.3f}")
    assert plane_err(e["model_var"], mv_np) <= TOL[np.dtype(np.float64)]["plane"]
    assert abs(var_np.mean() / mv_np.mean() - 1.0) <= 0.25
    assert abs(var_dev.mean() / e["model_var"].mean() - 1.0) <= 0.25
    assert np.all(np.abs(ratio_bl - 1.0) <= 0.25)
