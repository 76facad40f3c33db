"""The post-fit calls on the shapes at which their shared walks (csrc/row_walk.hpp, and the antenna kernels' four segments) can go
wrong, each against the NumPy restatement and at the tolerance of that call's own test file.

Seven antennas.  Antennas 0..5 carry all their cross-correlations but (0, 1): 14 rows; the autocorrelation (6, 6) makes 15, not a
multiple of the four rows of a block.  Antennas 0 and 1 have four cross entries, antennas 2..5 five, so a wave's segment of an
antenna's list holds 2, 2, 1, 0 or 1, 1, 1, 1 entries; antenna 6 has none in the sweeps' list, and the two roles of its
autocorrelation in the quality list.

nfreqs = 5: rows are padded to 8 channels only (pw = 8 in problem_plan.hpp; every kernel path shares that padding, the solver here
runs the SHARED layout's `general` kernels), so the last 16-byte vector of a row is part padding (fp32: channels 4..7; fp64: 4, 5) or
all padding (fp64: 6, 7).  nfreqs = 260: the row padding is a function of nfreqs alone and gives fpad = 384 there (not 264), so an
fp32 row needs a second trip of the wave with 32 live lanes (fp64: a second trip of 64), and the antenna kernels need a second
(fp64: a third) channel block whose channels past 260 are not stored.

Two slices in one solver; the calls that take a mask select slice 0, and slice 1 keeps its bits.  cal_solver_fix_degeneracies and
cal_solver_delay_spectrum take no mask: every slice is compared with the restatement of its own rows."""
import copy
import functools

import numpy as np
import pytest

import degeneracy_ref as R
import test_gpu_coeff_solve as CS
import test_gpu_degeneracy as DG
import test_gpu_delay_spectrum as DS
import test_gpu_fit_quality as FQ
import test_gpu_gain_solve as GS
import test_gpu_gauss_newton as GN
import test_gpu_robust_weights as RW
from calamity_amd import batched, modeling, synthetic
from calamity_amd.problem import FitProblem
from delay_spectrum_ref import NAMES, bin_rows, bound_ratio
from gauss_newton_ref import Ref

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
NFREQS = [5, 260]
NA, T = 7, 2
KEYS = ("g_r", "g_i", "c_r", "c_i")


@functools.lru_cache(maxsize=None)
def one_slice(nfreqs, t):
    """(problem, start, perturbed parameters) of slice t: the same antennas and bases, its own data."""
    i_idx, j_idx = np.triu_indices(NA, k=1)
    sel = np.where((j_idx != NA - 1) & ~((i_idx == 0) & (j_idx == 1)))[0]
    p0, _, start0 = synthetic.make_problem(NA, nfreqs, f0=150e6, df=400e3, seed=21, bl_sel=sel, data_seed=30 + t)
    rng = np.random.default_rng(9 + t)
    nv = p0.basis[0].shape[1]
    auto = NA - 1
    p = FitProblem(nants=NA, nfreqs=nfreqs, basis=p0.basis, grp_basis=np.concatenate([p0.grp_basis, [0]]).astype(np.int32),
                   grp_bl_start=np.arange(p0.nbls + 2, dtype=np.int32), bl_ant0=np.concatenate([p0.bl_ant0, [auto]]).astype(np.int32),
                   bl_ant1=np.concatenate([p0.bl_ant1, [auto]]).astype(np.int32), bl_rowblk=np.zeros(p0.nbls + 1, dtype=np.int32),
                   data_r=np.concatenate([p0.data_r, rng.standard_normal((1, nfreqs))]),
                   data_i=np.concatenate([p0.data_i, rng.standard_normal((1, nfreqs))]),
                   wgts=np.concatenate([p0.wgts, np.full((1, nfreqs), p0.wgts.max())]))
    p.validate()
    start = dict(start0, c_r=np.concatenate([start0["c_r"], rng.standard_normal(nv)]), c_i=np.concatenate([start0["c_i"], rng.standard_normal(nv)]))
    return p, start, FQ.perturbed(p, start, seed=40 + t)


@functools.lru_cache(maxsize=None)
def batch(nfreqs):
    """(the two-slice problem with its data, its parts, perturbed parameters, start parameters)."""
    parts = [one_slice(nfreqs, t) for t in range(T)]
    p0 = parts[0][0]
    assert p0.nbls == 15 and p0.nbls % 4 != 0 and p0.bl_ant0[-1] == p0.bl_ant1[-1] == NA - 1
    cross = p0.bl_ant0 != p0.bl_ant1
    counts = np.bincount(np.concatenate([p0.bl_ant0[cross], p0.bl_ant1[cross]]), minlength=NA)
    assert list(counts) == [4, 4, 5, 5, 5, 5, 0]
    sub, _, _ = batched.replicate_slices(p0, T)
    full = copy.copy(sub)
    full.data_r, full.data_i, full.wgts = (np.concatenate([getattr(parts[t][0], k) for t in range(T)]) for k in ("data_r", "data_i", "wgts"))
    pert = {k: np.concatenate([parts[t][2][k] for t in range(T)]) for k in KEYS}
    start = {k: np.concatenate([parts[t][1][k] for t in range(T)]) for k in KEYS}
    return full, [q[0] for q in parts], pert, start


def solver_of(full, params, dtype):
    from calamity_amd.solver import HipFitSolver

    s = HipFitSolver(dtype=dtype)
    s.set_problem(full, layout="shared", kernel_path="general")
    s.set_data(full.data_r, full.data_i, full.wgts)
    s.set_params(*[params[k] for k in KEYS])
    GN.assert_path(s, "general")
    return s


def sliced(params, t, p0):
    return {k: params[k][t * (p0.nants if k[0] == "g" else p0.ncoeffs):(t + 1) * (p0.nants if k[0] == "g" else p0.ncoeffs)] for k in KEYS}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nfreqs", NFREQS)
def test_fit_quality(nfreqs, dtype):
    full, parts, params, _ = batch(nfreqs)
    s = solver_of(full, params, dtype)
    q = s.fit_quality()
    ref = FQ.restated(full, params, dtype)
    FQ.check_parity(q, ref, dtype, f"fit_quality {nfreqs} {np.dtype(dtype).name}")
    # the autocorrelation enters its antenna once, and antenna 6 holds nothing else
    for t in range(T):
        a, b = t * NA + NA - 1, t * parts[0].nbls + parts[0].nbls - 1
        assert FQ.plane_err(q["chisq_ant"][a], ref["e"][b]) <= FQ.TOL[np.dtype(dtype)]["plane"]
        np.testing.assert_array_equal(q["wsum_ant"][a], full.wgts[b].astype(dtype).astype(np.float64))
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nfreqs", NFREQS)
def test_robust_weights(nfreqs, dtype):
    full, parts, params, _ = batch(nfreqs)
    s = solver_of(full, params, dtype)
    nb = parts[0].nbls
    w_in = s.get_weights(0)
    for kind in RW.R.KINDS:
        ref = RW.reference(s, full, kind)
        out = s.robust_weights(kind=kind, threshold=RW.K, slice_mask=[1, 0])
        w = s.get_weights(0)
        RW.check(out, w, ref, kind, dtype, f"robust_weights {nfreqs} {np.dtype(dtype).name}", rows=np.arange(nb))
        np.testing.assert_array_equal(w[nb:], w_in[nb:])  # the masked slice keeps its bits
        assert not np.any(out["scale_bl"][nb:]) and not np.any(out["ndown_bl"][nb:])
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nfreqs", NFREQS)
def test_solve_gains(nfreqs, dtype):
    full, parts, params, _ = batch(nfreqs)
    s = solver_of(full, params, dtype)
    before = s.get_params()
    s.solve_gains(2, damping=0.5, slice_mask=[1, 0])
    want = GS.restated(full, params, dtype, nsweeps=2, damping=0.5)[0]
    after = s.get_params()
    tol = FQ.TOL[np.dtype(dtype)]["plane"]
    errs = (FQ.plane_err(after[0][:NA], want.real[:NA]), FQ.plane_err(after[1][:NA], want.imag[:NA]))
    print(f"solve_gains {nfreqs} {np.dtype(dtype).name}: g_r {errs[0]:.2e}  g_i {errs[1]:.2e}")
    assert max(errs) <= tol, errs
    for k in (0, 1):
        np.testing.assert_array_equal(after[k][NA:], before[k][NA:])  # the masked slice
        np.testing.assert_array_equal(after[k][NA - 1], before[k][NA - 1])  # antenna 6: no cross-correlation, den = 0
        assert np.all(after[k][: NA - 1] != before[k][: NA - 1])
    for k in (2, 3):
        np.testing.assert_array_equal(after[k], before[k])
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nfreqs", NFREQS)
def test_solve_coeffs(nfreqs, dtype):
    full, parts, params, _ = batch(nfreqs)
    p0 = parts[0]
    s = solver_of(full, params, dtype)
    before = s.get_params()
    res = s.solve_coeffs(ridge=1e-6, slice_mask=[1, 0])
    want, _, conds, singular = CS.restated(p0, sliced(params, 0, p0), dtype, ridge=1e-6)
    assert max(conds) <= CS.COND_MAX and singular == [] and res == {"nsolved": p0.ngrps, "nsingular": 0}, (max(conds), singular, res)
    after = s.get_params()
    nc = p0.ncoeffs
    errs = (FQ.plane_err(after[2][:nc], want.real), FQ.plane_err(after[3][:nc], want.imag))
    print(f"solve_coeffs {nfreqs} {np.dtype(dtype).name}: c_r {errs[0]:.2e}  c_i {errs[1]:.2e}  largest cond(N) {max(conds):.2e}")
    assert max(errs) <= FQ.TOL[np.dtype(dtype)]["plane"], errs
    for k in (2, 3):
        np.testing.assert_array_equal(after[k][nc:], before[k][nc:])  # the masked slice
    for k in (0, 1):
        np.testing.assert_array_equal(after[k], before[k])
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nfreqs", NFREQS)
def test_normal_product(nfreqs, dtype):
    full, parts, params, _ = batch(nfreqs)
    s = solver_of(full, params, dtype)
    refs = GN.slice_refs(full, params, dtype, parts=parts)
    GN.check_product(s, refs, full, params, dtype, f"normal_product {nfreqs} {np.dtype(dtype).name}")
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nfreqs", NFREQS)
def test_gauss_newton_step(nfreqs, dtype):
    """ncg = 5, lambda = 1e-3 from the start values (unity gains), slice 0 alone: the short-trajectory contract of the call's own test."""
    full, parts, _, start = batch(nfreqs)
    p0 = parts[0]
    tol = GN.TOL[np.dtype(dtype)]
    s = solver_of(full, start, dtype)
    before = s.get_params()
    out = s.gauss_newton_step(ncg=5, lam=[1e-3, 1e-3], cg_tol=0.0, slice_mask=[1, 0])
    g, c = GN.cast_params(sliced(start, 0, p0), dtype)
    want = Ref(p0, dtype=dtype).step(g, c, lam=1e-3, ncg=5, cg_tol=0.0)
    got = s.get_params()
    na, nc = p0.nants, p0.ncoeffs
    errs = [GN.relnorm(got[0][:na], want["g"].real), GN.relnorm(got[1][:na], want["g"].imag), GN.relnorm(got[2][:nc], want["c"].real),
            GN.relnorm(got[3][:nc], want["c"].imag)]
    lerr = [abs(out[k][0] - want[k]) / want[k] for k in ("loss_before", "loss_after")]
    print(f"gauss_newton_step {nfreqs} {np.dtype(dtype).name}: " + "  ".join(f"{k} {e:.2e}" for k, e in zip(KEYS, errs))
          + f"  loss_before {lerr[0]:.2e}  loss_after {lerr[1]:.2e}  ({out['loss_before'][0]:.4e} -> {out['loss_after'][0]:.4e})")
    assert want["accepted"] and out["accepted"][0] and out["cg_iters"][0] == want["cg_iters"] == 5
    assert max(errs) <= tol["params"], errs
    assert max(lerr) <= tol["loss"], lerr
    # the masked slice: not accepted, no iteration, every bit kept
    assert not out["accepted"][1] and out["cg_iters"][1] == 0 and out["loss_after"][1] == out["loss_before"][1]
    for k in range(4):
        part = slice(na, None) if k < 2 else slice(nc, None)
        np.testing.assert_array_equal(got[k][part], before[k][part])
    s.close()


def fix_degeneracies_cases(s, nfreqs, dtype, label):
    """Both modes on the open solver ``s`` of ``batch(nfreqs)``: every slice against the restatement of its own rows."""
    full, parts, params, _ = batch(nfreqs)
    p0, nb = parts[0], parts[0].nbls
    assert not np.any(((p0.bl_ant0 == NA - 1) | (p0.bl_ant1 == NA - 1)) & (p0.bl_ant0 != p0.bl_ant1))  # antenna 6: its autocorrelation only
    antpos, freqs = R.hex_array(NA), 150e6 + 400e3 * np.arange(nfreqs)
    m_r, m_i = s.model()
    m = m_r.astype(np.float64) + 1j * m_i.astype(np.float64)
    g = DG.cast_c(params["g_r"], params["g_i"], dtype)
    rng = np.random.default_rng(60)
    gref = g * np.exp(1j * rng.uniform(-1, 1, size=nfreqs))[None, :] * (1 + 0.05 * rng.normal(size=g.shape))
    gref[NA - 1 :: NA] = -g[NA - 1 :: NA]  # antenna 6 of every slice: counted into psi it would turn the sum by far more than the tolerance
    gref_c = DG.cast_c(gref.real, gref.imag, dtype)
    for mode in ("channel", "band"):
        refs = [DG.inject(m[t * nb : (t + 1) * nb], p0.bl_ant0, p0.bl_ant1, antpos, freqs, seed=50 + t, band=mode == "band", flag_antenna=None if t else 2)
                for t in range(T)]
        ref_s, ref_w = np.concatenate([r[0] for r in refs]), np.concatenate([r[1] for r in refs])
        out = s.fix_degeneracies(ref_s.real, ref_s.imag, antpos, ref_w=ref_w, mode=mode, iters=6, freqs=freqs, gref_r=gref.real, gref_i=gref.imag)
        assert out["eta"].shape == (T, nfreqs)
        for t in range(T):
            a, rows = slice(t * NA, (t + 1) * NA), slice(t * nb, (t + 1) * nb)
            ref = R.fix_degeneracies(m[rows], DG.cast_c(refs[t][0].real, refs[t][0].imag, dtype), refs[t][1].astype(dtype).astype(np.float64), g[a],
                                     p0.bl_ant0, p0.bl_ant1, antpos, iters=6, mode=mode, freqs=freqs, gref=gref_c[a], dtype=dtype)
            DG.check_slice(out, t, ref, dtype, f"{label} {mode}", NA, rows)
            # antenna 6 is turned like every other antenna, from the device's own eta, tilt and psi
            k = t * NA + NA - 1
            want = g[k] * np.exp(-out["eta"][t]) * np.exp(-1j * (out["tilt"][t] @ antpos[NA - 1] + out["psi"][t]))
            got = out["g_r"][k].astype(np.float64) + 1j * out["g_i"][k].astype(np.float64)
            assert DG.err(got, want) <= DG.TOL[np.dtype(dtype)], (label, mode, t)
            assert np.count_nonzero(out["nsamples"][t]) == nfreqs - 1 and out["nsamples"][t, 4] == 0  # channel 4 is flagged (inject)
        DG.check_invariance(out, g, m, full.bl_ant0, full.bl_ant1, dtype, f"{label} {mode}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nfreqs", NFREQS)
def test_fix_degeneracies(nfreqs, dtype):
    """nfreqs = 260 (fpad 384): two channel blocks of degen_sum_kernel, the second with 4 live channels; five of degen_solve_kernel stage 0
    and of degen_phase_kernel, the last with 4; two trips of the `f += 256` loop of the band stage; two (fp32) or three (fp64) trips of a
    wave along a row in degen_rows_kernel and degen_apply_rows_kernel.  nfreqs = 5 (fpad 8): the last 16-byte vector of a row is part or
    all padding, and the flagged channel 4 is the last one before the padding.  Antenna 6 has only its autocorrelation: it stays out of psi
    (its reference gain is -g: counted, it would turn psi by up to 0.23 rad at 5 channels and 0.32 rad at 260) and is turned by eta, the tilt and psi like the others."""
    full, _, params, _ = batch(nfreqs)
    assert DG.fpad_of(nfreqs) == {5: 8, 260: 384}[nfreqs]
    s = solver_of(full, params, dtype)
    fix_degeneracies_cases(s, nfreqs, dtype, f"fix_degeneracies {nfreqs} {np.dtype(dtype).name}")
    s.close()


def test_fix_degeneracies_stream_layout():
    """The same at 260 channels in fp32 in the STREAM layout, where the replicated problem's rows share tiles through bl_alias."""
    from calamity_amd.solver import HipFitSolver

    full, _, params, _ = batch(260)
    assert full.bl_alias is not None and DG.fpad_of(260) == 384
    s = HipFitSolver(dtype=np.float32)
    s.set_problem(full, layout="stream")
    s.set_data(full.data_r, full.data_i, full.wgts)
    s.set_params(*[params[k] for k in KEYS])
    fix_degeneracies_cases(s, 260, np.float32, "fix_degeneracies 260 float32 stream")
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nfreqs", NFREQS)
def test_delay_spectrum(nfreqs, dtype):
    """All nfreqs delays.  nfreqs = 5: fpad = 8 but the masked planes' pitch is 32, so dspec_rows_kernel zeroes the channels in
    [fpad, xpitch) through its branch without loads, and the transform runs one staged step that is mostly padding.  nfreqs = 260:
    fpad = 384, a second trip of the wave along a row (fp32: 32 live lanes), twelve staged steps of the operator, and five column
    blocks of which the last holds 4 delays."""
    full, parts, params, _ = batch(nfreqs)
    p0, nb = parts[0], parts[0].nbls
    assert DG.fpad_of(nfreqs) == {5: 8, 260: 384}[nfreqs]
    op, norm_f, _ = modeling.delay_transform(150e6 + 400e3 * np.arange(nfreqs))
    assert op.shape == (nfreqs, nfreqs) and -(-nfreqs // 64) == {5: 1, 260: 5}[nfreqs] and nfreqs % 64 in (4, 5)
    local, nbins = DS.bins_of(p0)  # row 3 of a slice is in no bin, bin 3 of a slice holds no row
    bins = np.concatenate([np.where(local >= 0, local + t * nbins, -1) for t in range(T)]).astype(np.int32)
    s = solver_of(full, params, dtype)
    for calibrated in (False, True):
        label = f"delay_spectrum {nfreqs} {np.dtype(dtype).name} calibrated={calibrated}"
        out = s.delay_spectrum(op, norm_f, bin_of_bl=bins, nbins=T * nbins, per_baseline=True, calibrated=calibrated)
        for t in range(T):
            rows, mine = slice(t * nb, (t + 1) * nb), slice(t * nbins, (t + 1) * nbins)
            ref = DS.reference(parts[t], sliced(params, t, p0), dtype, op, norm_f, calibrated)
            worst = {}
            for k in NAMES:
                P = out["per_baseline"][k][rows]
                assert P.shape == (nb, nfreqs) and np.all(np.isfinite(P)), (label, k)
                worst[k] = bound_ratio(P, ref, k, dtype)
            print(f"{label} slice {t}: error / bound  " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
            assert max(worst.values()) <= 1.0, (label, t, worst)
            np.testing.assert_allclose(out["norm_bl"][rows], ref["norm_bl"], rtol=1e-13, atol=0)
            np.testing.assert_array_equal(out["count_bin"][mine], ref["count_bin"])
            assert out["count_bin"][mine].sum() == nb - 1 and out["count_bin"][mine][nbins - 1] == 0
            own = bin_rows({k: out["per_baseline"][k][rows] for k in NAMES}, out["norm_bl"][rows], local, nbins)
            for k in NAMES:  # the bins against the sequential double sum of the device's own rows, as in the call's own file
                assert np.max(np.abs(out[k][mine] - own[k])) <= nb * 2.0 ** -53 * np.max(np.abs(own[k])), (label, t, k)
    s.close()
