"""cal_solver_fix_degeneracies on the device against the NumPy restatement tests/degeneracy_ref.py on identical inputs: the model rows
are the solver's own (``model()``: the same pass), the reference is that model moved by an injected (eta, Phi) plus noise, the largest
injected |Phi.d| is 1 rad.  Tolerances: fp64 1e-10, fp32 1e-4, norm-wise; the invariance of
g_i conj(g_j) m within 16 ulp of the dtype (three roundings of factors computed in double).

Shapes: 7 antennas give 21 rows (a last block of one row) and 20 channels end inside a lane vector (row padding to 32 is exercised);
25 antennas give 300 rows: two segments of 128 rows of the sum kernel and a ragged third of 44."""
import copy
import functools

import numpy as np
import pytest

import degeneracy_ref as R
from calamity_amd import _lib, batched, distributed, synthetic
from calamity_amd.problem import FitProblem

pytestmark = pytest.mark.gpu

TOL = {np.dtype(np.float64): 1e-10, np.dtype(np.float32): 1e-4}
NF = 20


def fpad_of(nfreqs):
    pw = 8
    while pw < 128 and pw < nfreqs:
        pw *= 2
    return (nfreqs + pw - 1) // pw * pw


@functools.lru_cache(maxsize=None)
def base_problem(nants, seed=0, kind="plain", nfreqs=NF):
    p, truth, start = synthetic.make_problem(nants, nfreqs, f0=150e6, df=1e6, seed=seed)
    rng = np.random.default_rng(100 + seed)
    params = dict(g_r=start["g_r"] + 0.1 * rng.standard_normal((nants, nfreqs)), g_i=start["g_i"] + 0.1 * rng.standard_normal((nants, nfreqs)),
                  c_r=start["c_r"].copy(), c_i=start["c_i"].copy())
    if kind == "group":  # a fitting group of three baselines
        p, params = synthetic.add_redundant_group(p, params, rng)
    if kind == "auto":  # one autocorrelation row of antenna 2 behind the others
        nv = p.basis[0].shape[1]
        p = FitProblem(nants=nants, nfreqs=nfreqs, basis=p.basis, grp_basis=np.concatenate([p.grp_basis, [0]]).astype(np.int32),
                       grp_bl_start=np.arange(p.nbls + 2, dtype=np.int32), bl_ant0=np.concatenate([p.bl_ant0, [2]]).astype(np.int32),
                       bl_ant1=np.concatenate([p.bl_ant1, [2]]).astype(np.int32), bl_rowblk=np.zeros(p.nbls + 1, dtype=np.int32),
                       data_r=np.concatenate([p.data_r, rng.standard_normal((1, nfreqs))]), data_i=np.concatenate([p.data_i, rng.standard_normal((1, nfreqs))]),
                       wgts=np.concatenate([p.wgts, np.full((1, nfreqs), p.wgts.max())]))
        p.validate()
        params = dict(params, c_r=np.concatenate([params["c_r"], 1.0 + rng.standard_normal(nv)]), c_i=np.concatenate([params["c_i"], rng.standard_normal(nv)]))
    return p, params, truth["freqs"], truth["antpos"][:, :2].copy()


def solver_of(p, params, dtype, layout="shared", kernel_path="auto"):
    from calamity_amd.solver import HipFitSolver

    s = HipFitSolver(dtype=dtype)
    s.set_problem(p, layout=layout, kernel_path=kernel_path)
    s.set_params(params["g_r"], params["g_i"], params["c_r"], params["c_i"])
    return s


def inject(m, ant0, ant1, antpos, freqs, seed, band=False, flag_channel=4, flag_antenna=2, direction=None):
    """The reference planes, their weights and reference gains' offsets for the model rows ``m`` of one slice.  ``direction``: the unit
    vector of a line array that does not lie along east (the tilt is injected along it: across it nothing is observable)."""
    rng = np.random.default_rng(seed)
    nbls, nf = m.shape
    d = antpos[ant0] - antpos[ant1]
    line = np.ptp(antpos[:, 1]) == 0
    if band:
        phi = (freqs / freqs.mean())[:, None] * rng.normal(size=2)[None, :]
        eta = np.full(nf, 0.15)
    else:
        phi = rng.normal(size=(nf, 2))
        eta = 0.2 * rng.normal(size=nf)
    if line:
        phi[:, 1] = 0.0
    if direction is not None:
        phi = (phi @ np.asarray(direction))[:, None] * np.asarray(direction)[None, :]
    phi = phi / np.abs(d @ phi.T).max()
    s = m * np.exp(2 * eta)[None, :] * np.exp(1j * (d @ phi.T))
    s = s + 0.02 * np.sqrt(np.mean(np.abs(m) ** 2)) * (rng.normal(size=m.shape) + 1j * rng.normal(size=m.shape))
    w = (rng.random((nbls, nf)) >= 0.05) * (0.5 + rng.random((nbls, nf)))
    if flag_channel is not None:
        w[:, flag_channel] = 0.0
    if flag_antenna is not None:
        w[(ant0 == flag_antenna) | (ant1 == flag_antenna)] = 0.0
    return s, w


def err(got, want):
    return float(np.max(np.abs(got - want)) / max(np.max(np.abs(want)), 1e-300))


def check_slice(out, t, ref, dtype, label, nants, rows):
    """Slice ``t`` of the device's ``out`` against the restatement ``ref`` of that slice."""
    tol = TOL[np.dtype(dtype)]
    a = slice(t * nants, (t + 1) * nants)
    g = out["g_r"][a].astype(np.float64) + 1j * out["g_i"][a].astype(np.float64)
    m = out["model_r"][rows].astype(np.float64) + 1j * out["model_i"][rows].astype(np.float64)
    errs = dict(eta=err(out["eta"][t], ref["eta"]), tilt=err(out["tilt"][t], ref["tilt"]),
                psi=float(np.max(np.abs(np.angle(np.exp(1j * (out["psi"][t] - ref["psi"]))))) / max(np.max(np.abs(ref["psi"])), 1e-300)),
                last_step=float(np.max(np.abs(out["last_step"][t] - ref["last_step"]))), g=err(g, ref["g"]), model=err(m, ref["model"]))
    print(f"{label} slice {t}: " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    np.testing.assert_array_equal(out["nsamples"][t], ref["nsamples"], err_msg=label)
    for k in ("eta", "tilt", "psi", "g", "model"):
        assert errs[k] <= tol, (label, k, errs)
    assert errs["last_step"] <= tol, (label, errs)
    return errs


def check_invariance(out, g, m, ant0, ant1, dtype, label):
    eps = np.finfo(dtype).eps
    g2 = out["g_r"].astype(np.float64) + 1j * out["g_i"].astype(np.float64)
    m2 = out["model_r"].astype(np.float64) + 1j * out["model_i"].astype(np.float64)
    before = g[ant0] * np.conj(g[ant1]) * m
    after = g2[ant0] * np.conj(g2[ant1]) * m2
    live = np.abs(before) > 0
    worst = float(np.max(np.abs(after - before)[live] / np.abs(before)[live]) / eps)
    print(f"{label}: invariance {worst:.2f} ulp")
    assert worst <= 16.0, (label, worst)


def cast_c(r, i, dtype):
    return np.asarray(r).astype(dtype).astype(np.float64) + 1j * np.asarray(i).astype(dtype).astype(np.float64)


def run_case(p, params, freqs, antpos, dtype, mode, seed, layout="shared", label="", direction=None):
    s = solver_of(p, params, dtype, layout)
    m_r, m_i = s.model()
    m = m_r.astype(np.float64) + 1j * m_i.astype(np.float64)
    g = cast_c(params["g_r"], params["g_i"], dtype)
    ref_s, ref_w = inject(m, p.bl_ant0, p.bl_ant1, antpos, freqs, seed, band=mode == "band", direction=direction)
    rng = np.random.default_rng(seed + 1)
    gref = g * np.exp(1j * rng.uniform(-1, 1, size=NF))[None, :] * (1 + 0.05 * rng.normal(size=g.shape))
    args = dict(ref_w=ref_w, mode=mode, iters=6, freqs=freqs, g_r=params["g_r"], g_i=params["g_i"], gref_r=gref.real, gref_i=gref.imag)
    out = s.fix_degeneracies(ref_s.real, ref_s.imag, antpos, **args)
    again = s.fix_degeneracies(ref_s.real, ref_s.imag, antpos, **args)
    for k in out:
        np.testing.assert_array_equal(out[k], again[k], err_msg=f"{label}: two calls differ in {k}")
    s.close()
    ref = R.fix_degeneracies(m, cast_c(ref_s.real, ref_s.imag, dtype), np.asarray(ref_w).astype(dtype).astype(np.float64), g, p.bl_ant0, p.bl_ant1, antpos,
                             iters=6, mode=mode, freqs=freqs, gref=cast_c(gref.real, gref.imag, dtype), dtype=dtype)
    check_slice(out, 0, ref, dtype, label, p.nants, slice(None))
    check_invariance(out, g, m, p.bl_ant0, p.bl_ant1, dtype, label)
    # the flagged channel keeps the identity bit for bit; the flagged antenna stays out of psi (the restatement leaves it out too)
    assert out["nsamples"][0, 4] == 0 and out["eta"][0, 4] == 0 and out["psi"][0, 4] == 0 and not out["tilt"][0, 4].any()
    np.testing.assert_array_equal(out["model_r"][:, 4], m_r[:, 4])
    np.testing.assert_array_equal(out["g_r"][:, 4], np.asarray(params["g_r"]).astype(dtype)[:, 4])
    assert out["last_step"].max() < 1e-3  # radians on the longest baseline: the iteration settled
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("mode", ["channel", "band"])
@pytest.mark.parametrize("shape", [(7, "plain", "stream"), (7, "group", "shared"), (7, "auto", "shared"), (25, "plain", "shared")])
def test_parity_with_the_numpy_restatement(shape, mode, dtype):
    nants, kind, layout = shape
    p, params, freqs, antpos = base_problem(nants, kind=kind)
    assert p.nbls == {7: 21, 25: 300}[nants] + (kind == "auto")
    run_case(p, params, freqs, antpos, dtype, mode, seed=nants, layout=layout, label=f"{shape} {mode} {np.dtype(dtype).name}")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_linear_array_steps_along_its_own_direction(dtype):
    p, params, freqs, _ = base_problem(7)
    out = run_case(p, params, freqs, R.line_array(7), dtype, "channel", seed=11, label=f"line {np.dtype(dtype).name}")
    assert not out["tilt"][0, :, 1].any()


@functools.lru_cache(maxsize=None)
def two_slices(per_slice):
    parts = []
    for t in range(2):
        p, params, freqs, antpos = base_problem(7, seed=t)
        parts.append((p, params))
    p2, params2 = distributed.batch_time_slices(parts, per_slice=per_slice)
    return p2, params2, parts, freqs, antpos


def slice_inputs(parts, dtype, freqs, antpos, models):
    refs = []
    for t, (p, params) in enumerate(parts):
        s, w = inject(models[t], p.bl_ant0, p.bl_ant1, antpos, freqs, seed=20 + t, flag_antenna=None if t else 3)
        refs.append((s, w))
    return refs


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_two_slices_equal_two_solvers_bit_for_bit(dtype):
    p2, params2, parts, freqs, antpos = two_slices(True)
    nb = parts[0][0].nbls
    s = solver_of(p2, params2, dtype)
    m_r, m_i = s.model()
    m = m_r.astype(np.float64) + 1j * m_i.astype(np.float64)
    refs = slice_inputs(parts, dtype, freqs, antpos, [m[:nb], m[nb:]])
    ref_s, ref_w = np.concatenate([r[0] for r in refs]), np.concatenate([r[1] for r in refs])
    g0 = cast_c(params2["g_r"], params2["g_i"], dtype)
    gref = g0 * np.exp(0.4j)
    out = s.fix_degeneracies(ref_s.real, ref_s.imag, antpos, ref_w=ref_w, gref_r=gref.real, gref_i=gref.imag)
    s.close()
    assert out["eta"].shape == (2, NF) and out["tilt"].shape == (2, NF, 2)
    assert not np.array_equal(out["eta"][0], out["eta"][1])
    for t, (p, params) in enumerate(parts):
        a, rows = slice(t * 7, (t + 1) * 7), slice(t * nb, (t + 1) * nb)
        ref = R.fix_degeneracies(m[rows], cast_c(refs[t][0].real, refs[t][0].imag, dtype), refs[t][1].astype(dtype).astype(np.float64), g0[a], p.bl_ant0,
                                 p.bl_ant1, antpos, gref=cast_c(gref.real, gref.imag, dtype)[a], dtype=dtype)
        check_slice(out, t, ref, dtype, f"two slices {np.dtype(dtype).name}", 7, rows)
        one = solver_of(p, params, dtype)
        alone = one.fix_degeneracies(refs[t][0].real, refs[t][0].imag, antpos, ref_w=refs[t][1], gref_r=gref.real[a], gref_i=gref.imag[a])
        one.close()
        for k in ("eta", "psi", "tilt", "nsamples", "last_step"):
            np.testing.assert_array_equal(out[k][t], alone[k][0], err_msg=f"slice {t}: {k} differs between the batch and the slice alone")
        np.testing.assert_array_equal(out["g_r"][a], alone["g_r"])
        np.testing.assert_array_equal(out["model_i"][rows], alone["model_i"])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_joint_time_basis_layout_has_one_slice_per_time(dtype):
    p2, params2, parts, freqs, antpos = two_slices(False)
    nb = parts[0][0].nbls
    s = solver_of(p2, params2, dtype)
    s.set_gain_time_basis(np.array([[1.0, 1.0], [1.0, -1.0]]) / np.sqrt(2.0))
    m_r, m_i = s.model()
    m = m_r.astype(np.float64) + 1j * m_i.astype(np.float64)
    refs = slice_inputs(parts, dtype, freqs, antpos, [m[:nb], m[nb:]])
    ref_s, ref_w = np.concatenate([r[0] for r in refs]), np.concatenate([r[1] for r in refs])
    g0 = cast_c(params2["g_r"], params2["g_i"], dtype)  # y = 0: the expanded gains are g0
    out = s.fix_degeneracies(ref_s.real, ref_s.imag, antpos, ref_w=ref_w, mode="band", freqs=freqs, gref_r=g0.real, gref_i=g0.imag)
    s.close()
    assert out["eta"].shape == (2, NF)
    for t, (p, params) in enumerate(parts):
        a, rows = slice(t * 7, (t + 1) * 7), slice(t * nb, (t + 1) * nb)
        ref = R.fix_degeneracies(m[rows], cast_c(refs[t][0].real, refs[t][0].imag, dtype), refs[t][1].astype(dtype).astype(np.float64), g0[a], p.bl_ant0,
                                 p.bl_ant1, antpos, mode="band", freqs=freqs, gref=g0[a], dtype=dtype)
        check_slice(out, t, ref, dtype, f"time basis {np.dtype(dtype).name}", 7, rows)
    check_invariance(out, g0, m, p2.bl_ant0, p2.bl_ant1, dtype, "time basis")


def test_without_reference_gains_and_weights_the_solver_s_own_are_used():
    p, params, freqs, antpos = base_problem(7)
    s = solver_of(p, params, np.float64)
    m_r, m_i = s.model()
    m = m_r + 1j * m_i
    ref_s, _ = inject(m, p.bl_ant0, p.bl_ant1, antpos, freqs, seed=5)
    out = s.fix_degeneracies(ref_s.real, ref_s.imag, antpos)
    s.close()
    ref = R.fix_degeneracies(m, ref_s, p.wgts, params["g_r"] + 1j * params["g_i"], p.bl_ant0, p.bl_ant1, antpos)
    check_slice(out, 0, ref, np.float64, "own weights", 7, slice(None))
    assert not out["psi"].any()


@pytest.mark.parametrize("config", ["adam", "gain_basis"])
def test_a_run_continued_after_the_call_is_bit_identical(config):
    from calamity_amd import modeling

    p, params, freqs, antpos = base_problem(7)
    losses, final = {}, {}
    for with_call in (False, True):
        s = solver_of(p, params, np.float32)
        if config == "gain_basis":
            s.set_gain_basis(np.array(modeling.gain_dpss_basis(freqs, 100.0)))
        s.set_optimizer("Adam", learning_rate=1e-2)
        first = s.run(20, tol=0.0)[0]
        if with_call:
            out = s.fix_degeneracies(p.data_r, p.data_i, antpos, mode="band", freqs=freqs, gref_r=params["g_r"], gref_i=params["g_i"])
            assert out["nsamples"].sum() > 0
        second = s.run(20, tol=0.0)[0]
        losses[with_call] = np.concatenate([first, second])
        final[with_call] = s.get_params()
        s.close()
    assert len(losses[True]) == 40
    np.testing.assert_array_equal(losses[True], losses[False])
    for a, b in zip(final[True], final[False]):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_memory_grows_by_the_documented_scratch(dtype):
    p, params, freqs, antpos = base_problem(25)
    s = solver_of(p, params, dtype)
    s.model()
    s.fit_quality(params["g_r"], params["g_i"])  # the model planes, the given gains' buffer and the staging buffer exist from here on
    before = s.memory_bytes()
    s.fix_degeneracies(p.data_r, p.data_i, antpos, ref_w=p.wgts, g_r=params["g_r"], g_i=params["g_i"], gref_r=params["g_r"], gref_i=params["g_i"])
    after = s.memory_bytes()
    s.close()
    sz, fpad, nseg, nsl = np.dtype(dtype).itemsize, fpad_of(NF), -(-p.nbls // 128), 1
    assert fpad == 32 and nseg == 3
    want = (3 * p.nbls * fpad * sz  # the reference planes (then z0) and the reference's weights
            + 8 * nseg * fpad * 8  # the segments' partial sums
            + (14 * nsl * fpad + 2 * nsl) * 8  # the channels' state
            + 2 * p.nants * fpad * 2 * sz  # g' and gref
            + (2 * p.nbls + 2 * p.nants + fpad + nsl) * 8 + (p.nbls + nsl + 1 + 4 * nseg) * 4)  # d_b, positions, ratios; row lists, segments
    assert after - before == want, (after - before, want)


def test_error_codes():
    from calamity_amd.solver import HipFitSolver

    p, params, freqs, antpos = base_problem(7)
    bare = copy.copy(p)
    bare.data_r = bare.data_i = bare.wgts = None
    s = HipFitSolver(dtype=np.float32)
    s.set_problem(bare)
    s.set_params(params["g_r"], params["g_i"], params["c_r"], params["c_i"])
    with pytest.raises(_lib.CalamityHipError) as e:
        s.fix_degeneracies(p.data_r, p.data_i, antpos)
    assert e.value.code == -4 and "no data set" in str(e.value)
    s.set_data(p.data_r, p.data_i, p.wgts)
    bad = antpos.copy()
    bad[3, 1] = np.nan
    with pytest.raises(_lib.CalamityHipError) as e:
        s.fix_degeneracies(p.data_r, p.data_i, bad)
    assert e.value.code == -1 and "not finite" in str(e.value)
    s.fix_degeneracies(p.data_r, p.data_i, antpos)  # (the same call runs while no exchange is set)
    s.set_exchange_hook(lambda arr, op: None, 0, 2)  # two ranks: refused before anything is exchanged
    with pytest.raises(_lib.CalamityHipError) as e:
        s.fix_degeneracies(p.data_r, p.data_i, antpos)
    assert e.value.code == -4 and "all-reduce" in str(e.value)
    s.close()


def test_the_batch_fitter_hands_every_slice_through():
    p2, params2, parts, freqs, antpos = two_slices(True)
    p, _ = parts[0]
    bare = copy.copy(p)
    bare.data_r = bare.data_i = bare.wgts = None
    f = batched.SliceBatchFitter(bare, 2, dtype=np.float64)
    try:
        f.set_data(p2.data_r, p2.data_i, p2.wgts)
        f.set_params(params2["g_r"], params2["g_i"], params2["c_r"], params2["c_i"])
        out = f.fix_degeneracies(p2.data_r, p2.data_i, antpos, gref_r=params2["g_r"], gref_i=params2["g_i"])
    finally:
        f.close()
    s = solver_of(f.subs[0], params2, np.float64)  # the fitter's own problem of two slices in one plain solver
    s.set_data(p2.data_r, p2.data_i, p2.wgts)
    want = s.fix_degeneracies(p2.data_r, p2.data_i, antpos, gref_r=params2["g_r"], gref_i=params2["g_i"])
    s.close()
    for k in want:
        np.testing.assert_array_equal(out[k], want[k], err_msg=k)
