"""cal_solver_fix_degeneracies where its kernels branch (csrc/degeneracy_kernels.hpp), at the smallest shapes that reach each branch,
against the restatement tests/degeneracy_ref.py and with the tolerances and helpers of test_gpu_degeneracy.py (fp64 1e-10, fp32 1e-4
norm-wise, nsamples equal, the invariance of g_i conj(g_j) m within 16 ulp).  The one bound beyond those, on the tilt's component across a line, is derived at its test.

| test | the line or branch it pins | what a wrong version changes |
|---|---|---|
| test_nine_segments_* | degen_solve_kernel stage 0: `per = ceil(n / 8)`, `a0 = s0 + run * per`, `a1 = min(a0 + per, s1)` with n = 9: runs 0..3 hold two segments, run 4 one (the ragged segment of 11 rows), runs 5..7 start past s1 | a dropped or doubled segment changes `nsamples` (compared exactly) by the segment's live rows, and Q, H, q with it: eta, tilt off by far more than 1e-10 |
| test_nine_segments_two_slices_* | the clamp `a1 = s1` of slice 0's empty runs (a0 = 10, 12, 14 lie inside slice 1's segments 9..17), and `seg_ptr[t]` of slice 1 | slice 0 adds slice 1's partial sums: its nsamples grow and no output equals the slice alone bit for bit |
| test_identity_channels (channel) | `ok = live && acc[2] > 0` (sum Re z <= 0) and `dg_live`: `hee + hnn > 0` with Q > 0 | channel 3 would get `log` of a negative ratio (NaN) or a rotation; channel 7 a step `H^+ q` of a zero matrix; g', m' no longer the inputs' bits |
| test_identity_channels (band) | stage 1: `if (!dg_live(...)) continue` and the per-channel `live` of the second loop | channel 7's Q enters the band's amplitude (eta differs at 1e-3), or channel 7 gets the band's eta and tilt |
| test_identity_channels, both | degen_rows_kernel / degen_sum_kernel `live ? ... : 0` (a select, not a product with w = 0) | NaN or Inf of a flagged sample times 0 is NaN: every sum of the channel and every output of it |
| test_a_slice_that_keeps_the_identity | stage 1 `sh[2] = ok ? sre / Q : 0` and `&& amp2 > 0.0`; channel mode `acc[2] > 0`; Q = 0 everywhere; a slice's state planes `[t * fpad + f]` next to a live slice | slice 0 is scaled or rotated, reports samples, or slice 1 differs from the same slice alone |
| test_lines_not_along_east (north) | dg_step2: `if (we * we + wn * wn > ve * ve + vn * vn) ve = we, vn = wn` with (lam - c, b) = (0, 0) | n2 = 0: no step is taken, the tilt stays 0 and eta is that of Phi = 0: parity fails at 1e-1 |
| test_lines_not_along_east (oblique, 30 degrees) | dg_step2 with b != 0: `lam`, both columns, `proj = (v.q) / (n2 lam)` | a wrong sign or a swapped component of v leaves the line: the tilt's component across it is no longer 0 to rounding, and parity fails |

Measured on one MI355X, the worst case of a group, fp32 / fp64 (eta, tilt and psi of fp32 agree as closely as those of fp64 because
the restatement rounds z0 and Q to the dtype as the kernels do, and everything behind them is double on both sides):
nine segments     eta 3.0e-15 / 3.8e-15  tilt 1.0e-16 / 2.0e-16  psi 4.2e-16 / 5.3e-16  g 4.8e-8 / 1.2e-15  model 4.0e-8 / 1.0e-15  invariance 1.16 / 3.87 ulp
identity branches eta 4.6e-16 / 1.1e-15  tilt 1.4e-16 / 1.4e-16  psi 2.5e-16 / 2.5e-16  g 4.9e-8 / 3.9e-16  model 3.5e-8 / 3.6e-16  invariance 1.08 / 3.55 ulp
lines             eta 3.1e-16 / 5.5e-16  tilt 1.3e-16 / 8.8e-17  psi 1.7e-16 / 2.4e-16  g 3.9e-8 / 2.9e-16  model 3.8e-8 / 3.0e-16  invariance 1.05 / 3.45 ulp
                  the tilt across the line 1.8e-16 / 1.3e-16 of the largest tilt (north: exactly 0)"""
import functools
import warnings

import numpy as np
import pytest

import degeneracy_ref as R
from calamity_amd import distributed
from test_gpu_degeneracy import NF, TOL, base_problem, cast_c, check_invariance, check_slice, inject, run_case, solver_of, two_slices

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
MODES = ["channel", "band"]
OUTPUTS = ("eta", "psi", "tilt", "nsamples", "last_step", "g_r", "g_i", "model_r", "model_i")


def restated(m, ref_s, ref_w, g, gref, p, antpos, dtype, mode, freqs):
    s = np.empty(ref_s.shape, dtype=np.complex128)  # (part by part: 1j * inf would be nan + inf j, with a warning)
    s.real, s.imag = ref_s.real.astype(dtype), ref_s.imag.astype(dtype)
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # the restatement itself meets no NaN it does not mask
        return R.fix_degeneracies(m, s, np.asarray(ref_w).astype(dtype).astype(np.float64), g, p.bl_ant0, p.bl_ant1, antpos, iters=6, mode=mode,
                                  freqs=freqs, gref=gref, dtype=dtype)


def model_of(s):
    m_r, m_i = s.model()
    return m_r, m_i, m_r.astype(np.float64) + 1j * m_i.astype(np.float64)


def batch_and_alone(p2, params2, parts, refs, gref, antpos, dtype, mode, freqs):
    """The batch of two slices in one solver, and every slice alone in a solver of its own on the same inputs."""
    na, nb = parts[0][0].nants, parts[0][0].nbls
    ref_s, ref_w = np.concatenate([r[0] for r in refs]), np.concatenate([r[1] for r in refs])
    s = solver_of(p2, params2, dtype)
    out = s.fix_degeneracies(ref_s.real, ref_s.imag, antpos, ref_w=ref_w, mode=mode, freqs=freqs, gref_r=gref.real, gref_i=gref.imag)
    s.close()
    alone = []
    for t, (p, params) in enumerate(parts):
        a = slice(t * na, (t + 1) * na)
        one = solver_of(p, params, dtype)
        alone.append(one.fix_degeneracies(refs[t][0].real, refs[t][0].imag, antpos, ref_w=refs[t][1], mode=mode, freqs=freqs, gref_r=gref.real[a],
                                          gref_i=gref.imag[a]))
        one.close()
    assert out["eta"].shape == (2, NF) and nb * 2 == p2.nbls
    return out, alone


def assert_slice_is_the_slice_alone(out, alone, t, na, nb):
    a, rows = slice(t * na, (t + 1) * na), slice(t * nb, (t + 1) * nb)
    for k in ("eta", "psi", "tilt", "nsamples", "last_step"):
        np.testing.assert_array_equal(out[k][t], alone[k][0], err_msg=f"slice {t}: {k} differs between the batch and the slice alone")
    for k in ("g_r", "g_i"):
        np.testing.assert_array_equal(out[k][a], alone[k], err_msg=f"slice {t}: {k}")
    for k in ("model_r", "model_i"):
        np.testing.assert_array_equal(out[k][rows], alone[k], err_msg=f"slice {t}: {k}")


# ---- a. more than eight segments per slice -------------------------------------------------------------------------------------------

def assert_nine_segments(p):
    assert p.nbls == 1035 and -(-1035 // 128) == 9 and 1035 - 8 * 128 == 11  # per = 2: runs 0..3 full, run 4 the last segment, 5..7 empty


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", MODES)
def test_nine_segments_in_runs_of_two(mode, dtype):
    """46 antennas: 1035 rows = 8 segments of 128 and one of 11.  degen_solve_kernel cuts 9 segments into runs of per = 2: waves 0..3
    add two segments each, wave 4 the short last segment alone, waves 5..7 start at segments 10, 12, 14, past the slice's last, and
    must add nothing."""
    p, params, freqs, antpos = base_problem(46)
    assert_nine_segments(p)
    run_case(p, params, freqs, antpos, dtype, mode, seed=46, label=f"nine segments {mode} {np.dtype(dtype).name}")


@functools.lru_cache(maxsize=None)
def two_slices_of_46():
    parts = [base_problem(46, seed=t)[:2] for t in range(2)]
    _, _, freqs, antpos = base_problem(46)
    p2, params2 = distributed.batch_time_slices(parts, per_slice=True)
    return p2, params2, parts, freqs, antpos


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", MODES)
def test_nine_segments_two_slices_equal_two_solvers_bit_for_bit(mode, dtype):
    """2 x 1035 rows: slice 0 owns segments 0..8 and slice 1 segments 9..17, so slice 0's empty runs start at segments 10, 12 and 14 --
    slice 1's.  Only the clamp to the slice's last segment keeps them out: every output of slice t is that of the slice alone."""
    p2, params2, parts, freqs, antpos = two_slices_of_46()
    assert_nine_segments(parts[0][0])
    assert p2.nbls == 2070
    na, nb = 46, 1035
    s = solver_of(p2, params2, dtype)
    _, _, m = model_of(s)
    s.close()
    refs = [inject(m[t * nb:(t + 1) * nb], p.bl_ant0, p.bl_ant1, antpos, freqs, seed=20 + t, band=mode == "band", flag_antenna=None if t else 3)
            for t, (p, _) in enumerate(parts)]
    g0 = cast_c(params2["g_r"], params2["g_i"], dtype)
    gref = g0 * np.exp(0.4j)
    out, alone = batch_and_alone(p2, params2, parts, refs, gref, antpos, dtype, mode, freqs)
    assert not np.array_equal(out["nsamples"][0], out["nsamples"][1])
    label = f"nine segments, two slices {mode} {np.dtype(dtype).name}"
    for t, (p, _) in enumerate(parts):
        a, rows = slice(t * na, (t + 1) * na), slice(t * nb, (t + 1) * nb)
        ref = restated(m[rows], refs[t][0], refs[t][1], g0[a], cast_c(gref.real, gref.imag, dtype)[a], p, antpos, dtype, mode, freqs)
        check_slice(out, t, ref, dtype, label, na, rows)
        assert_slice_is_the_slice_alone(out, alone[t], t, na, nb)
    check_invariance(out, g0, m, p2.bl_ant0, p2.bl_ant1, dtype, label)
    assert out["last_step"].max() < 1e-3


# ---- b. the identity branches ----------------------------------------------------------------------------------------------------------

NEGATED, AUTO_ONLY = 3, 7  # channels: the reference is -m (sum Re z < 0); only the autocorrelation is live (Q > 0, tr H = 0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", MODES)
def test_identity_channels_and_non_finite_flagged_samples(mode, dtype):
    """Seven antennas, 21 cross rows and the autocorrelation of antenna 2.  Channel 3: the reference is exactly -m, so z0 = -w |m|^2,
    q = 0 and sum Re z < 0.  Channel 7: every cross row has w = 0, the autocorrelation (d_b = 0) alone is live: Q > 0, tr H = 0.
    Wherever w = 0 the reference holds NaN or Inf, as flagged samples of real data do."""
    p, params, freqs, _ = base_problem(7, kind="auto")
    antpos = R.hex_array(7)
    cross = p.bl_ant0 != p.bl_ant1
    assert p.nbls == 22 and cross.sum() == 21 and p.bl_ant0[21] == p.bl_ant1[21] == 2
    s = solver_of(p, params, dtype)
    m_r, m_i, m = model_of(s)
    g = cast_c(params["g_r"], params["g_i"], dtype)
    ref_s, ref_w = inject(m, p.bl_ant0, p.bl_ant1, antpos, freqs, 31, band=mode == "band", flag_channel=None, flag_antenna=None)
    ref_s[:, NEGATED] = -m[:, NEGATED]
    ref_w[cross, AUTO_ONLY] = 0.0
    ref_w[~cross, AUTO_ONLY] = 1.0
    dead = ref_w == 0
    assert dead[:, NEGATED].sum() < 21 and dead.sum() > 21  # flags at random too
    clean, dirty = np.where(dead, 0.0, ref_s), ref_s.copy()
    fill = np.array([complex(np.nan, 1.0), complex(np.inf, np.nan), complex(-1.0, -np.inf), complex(np.nan, np.nan)])
    dirty[dead] = fill[np.arange(dead.sum()) % 4]
    rng = np.random.default_rng(32)
    gref = g * np.exp(1j * rng.uniform(-1, 1, size=NF))[None, :] * (1 + 0.05 * rng.normal(size=g.shape))
    args = dict(ref_w=ref_w, mode=mode, iters=6, freqs=freqs, gref_r=gref.real, gref_i=gref.imag)
    out = s.fix_degeneracies(dirty.real, dirty.imag, antpos, **args)
    same = s.fix_degeneracies(clean.real, clean.imag, antpos, **args)
    s.close()
    label = f"identity channels {mode} {np.dtype(dtype).name}"
    for k in OUTPUTS:
        assert np.all(np.isfinite(out[k])), (label, k)
        np.testing.assert_array_equal(out[k], same[k], err_msg=f"{label}: {k} depends on samples with w = 0")
    ref = restated(m, dirty, ref_w, g, cast_c(gref.real, gref.imag, dtype), p, antpos, dtype, mode, freqs)
    check_slice(out, 0, ref, dtype, label, 7, slice(None))
    check_invariance(out, g, m, p.bl_ant0, p.bl_ant1, dtype, label)
    assert out["last_step"].max() < 1e-3
    identity = [NEGATED, AUTO_ONLY] if mode == "channel" else [AUTO_ONLY]
    for f in identity:
        assert out["nsamples"][0, f] == 0 and out["eta"][0, f] == 0 and out["psi"][0, f] == 0 and not out["tilt"][0, f].any(), (label, f)
        np.testing.assert_array_equal(out["g_r"][:, f], np.asarray(params["g_r"]).astype(dtype)[:, f])
        np.testing.assert_array_equal(out["g_i"][:, f], np.asarray(params["g_i"]).astype(dtype)[:, f])
        np.testing.assert_array_equal(out["model_r"][:, f], m_r[:, f])
        np.testing.assert_array_equal(out["model_i"][:, f], m_i[:, f])
    others = np.setdiff1d(np.arange(NF), identity)
    assert np.all(out["nsamples"][0, others] > 0) and np.all(out["eta"][0, others] != 0)
    if mode == "band":  # channel 3 stays in the band's sums: it carries the band's amplitude and its share of the tilt
        assert out["eta"][0, NEGATED] == out["eta"][0, 0] and out["tilt"][0, NEGATED].any()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", ["negated", "unweighted"])
def test_a_slice_that_keeps_the_identity_next_to_a_live_slice(kind, mode, dtype):
    """Two slices of 21 rows.  Slice 0 is `negated`: its reference is -e^{0.3} m, so sum Re z < 0 at every channel and over the band;
    or `unweighted`: its ref_w is 0 everywhere and its reference NaN.  It keeps every bit; slice 1 is the slice alone.

    (The negated *injection* with its tilt does not serve: the chord iteration runs away from a reference of the wrong sign, and after
    six steps the restatement finds sum Re z > 0 -- 268 samples, eta 0.42 in band mode.  Without a tilt q = 0 to rounding, Phi stays
    there and the sum stays negative.)"""
    p2, params2, parts, freqs, antpos = two_slices(True)
    na, nb = 7, parts[0][0].nbls
    s = solver_of(p2, params2, dtype)
    m_r, m_i, m = model_of(s)
    s.close()
    refs = [inject(m[t * nb:(t + 1) * nb], p.bl_ant0, p.bl_ant1, antpos, freqs, seed=40 + t, band=mode == "band", flag_antenna=None)
            for t, (p, _) in enumerate(parts)]
    if kind == "negated":
        refs[0] = (-np.exp(0.3) * m[:nb], refs[0][1])
        assert np.all((refs[0][1] > 0).sum(axis=0)[np.arange(NF) != 4] > 0)  # live samples at every channel but the flagged one
    else:
        refs[0] = (np.full((nb, NF), complex(np.nan, np.inf)), np.zeros((nb, NF)))
    g0 = cast_c(params2["g_r"], params2["g_i"], dtype)
    gref = g0 * np.exp(0.4j)
    out, alone = batch_and_alone(p2, params2, parts, refs, gref, antpos, dtype, mode, freqs)
    label = f"identity slice ({kind}) {mode} {np.dtype(dtype).name}"
    for k in OUTPUTS:
        assert np.all(np.isfinite(out[k])), (label, k)
    for k in ("nsamples", "eta", "psi", "tilt"):
        assert not out[k][0].any(), (label, k)
    for k in ("g_r", "g_i"):
        np.testing.assert_array_equal(out[k][:na], np.asarray(params2[k]).astype(dtype)[:na], err_msg=label)
    np.testing.assert_array_equal(out["model_r"][:nb], m_r[:nb], err_msg=label)
    np.testing.assert_array_equal(out["model_i"][:nb], m_i[:nb], err_msg=label)
    assert out["nsamples"][1].sum() > 0 and out["eta"][1].any()
    for t in range(2):
        assert_slice_is_the_slice_alone(out, alone[t], t, na, nb)
        rows, a = slice(t * nb, (t + 1) * nb), slice(t * na, (t + 1) * na)
        ref = restated(m[rows], refs[t][0], refs[t][1], g0[a], cast_c(gref.real, gref.imag, dtype)[a], parts[t][0], antpos, dtype, mode, freqs)
        check_slice(out, t, ref, dtype, label, na, rows)
    check_invariance(out, g0, m, p2.bl_ant0, p2.bl_ant1, dtype, label)


# ---- c. lines that are not along east --------------------------------------------------------------------------------------------------

LINES = {"north": np.array([0.0, 1.0]), "oblique": np.array([np.sqrt(3.0) / 2.0, 0.5])}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("line", list(LINES))
def test_lines_not_along_east(line, mode, dtype):
    """R.line_array(7) turned onto the unit vector u: H = S u u^T, det H = 0 to rounding (det H / (tr H / 2)^2 is -4e-16 against the
    threshold of 1e-12), so dg_step2 steps along the eigenvector.  North: a = b = 0, the column (lam - c, b) vanishes and its sibling
    (b, lam - a) is taken.  30 degrees: b != 0.  H is formed in double from exact d_b whatever the solver's dtype, so the tilt's
    component across the line is 0 to double rounding for both dtypes (the restatement gives 1.4e-16 of the largest tilt)."""
    u = LINES[line]
    antpos = R.line_array(7)[:, :1] * u[None, :]
    p, params, freqs, _ = base_problem(7)
    label = f"line {line} {mode} {np.dtype(dtype).name}"
    out = run_case(p, params, freqs, antpos, dtype, mode, seed=11, label=label, direction=u)
    tilt = out["tilt"][0]
    across = np.abs(tilt @ np.array([-u[1], u[0]])).max() / np.abs(tilt).max()
    print(f"{label}: tilt across the line / largest tilt {across:.2e}")
    assert np.abs(tilt @ u).max() > 0 and across <= TOL[np.dtype(np.float64)]
