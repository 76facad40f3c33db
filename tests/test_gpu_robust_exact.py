"""cal_solver_robust_weights on the device against a reference with the same bits (tests/test_gpu_robust_weights.py compares with a
float64 restatement at a tolerance and leaves out the samples near the threshold; a median one rank off passes there).

Construction.  The foreground coefficients are zero, so ``m = A c`` is exactly zero and, the gains being finite, so is ``g_i conj(g_j)
m``: the residual is the data, and ``e = w0 * (d_r * d_r + d_i * d_i)`` in the solver's dtype, one rounding per operation (the kernel
compiles with fp contract off).  ``robust_ref.residual_power_exact`` evaluates that line in NumPy on arrays of the dtype and has the
device's bits; every test asserts the precondition (``model()`` all zero, ``get_weights(1)`` and the data as they went in).  With ``e``
exact nothing here is a tolerance and no sample is left out:

* ``scale_bl`` is the float64 quotient ``float64(med) / ln 2`` of an element of the row: ``np.array_equal``.  The reference median is
  ``np.partition``'s, and ``robust_ref.lower_median_bits``, the kernel's bisection restated, must give the same element.
* ``ndown_bl``, the clip weights and the set of down-weighted samples of every kind are exact: ``z2``, ``k * k`` and the comparison are
  plain IEEE double operations.
* Huber and Cauchy weights take a double division, a square root and one rounding to the dtype against the NumPy float64 evaluation
  rounded once.  Every case prints how many of its weights are not bit-identical; on one MI355X that was 0 of 175 128 weights in all
  78 cases (subnormal and NaN weights included), so the assertion is equality, like the rest.

Problems are built directly: 3 antennas, the three cross-correlations and an autocorrelation (4 rows, one block of four waves), the
ties family with a second autocorrelation (5 rows: a second block with three idle waves), one random basis vector per baseline, random
finite gains.  Each row is one case (tests/robust_families.py).  Short rows run in both dtypes and both layouts, the rows at the LDS
limit (fpad = 4096 in float32, 2048 in float64: exactly 64 KB of dynamic LDS; one more channel pads to 4224 / 2176 and takes the form
with the keys in the model plane) in the SHARED layout."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import robust_families as RF  # noqa: E402
import robust_ref as R  # noqa: E402

from calamity_amd.problem import FitProblem  # noqa: E402

pytestmark = pytest.mark.gpu

K = 3.0
DTYPES = [np.float32, np.float64]
LAYOUTS = ["stream", "shared"]
PAIRS = [(0, 1), (0, 2), (1, 2), (2, 2), (0, 0)]
UINT = {4: np.uint32, 8: np.uint64}


def problem_of(d_r, d_i, w0, seed=0):
    """(problem, params): 3 antennas, the rows of ``d_r`` as baselines ``PAIRS``, a fitting group per baseline with a basis of one random
    vector, random gains of modulus about one, all coefficients zero."""
    nbls, nfreqs = d_r.shape
    assert nbls in (4, 5)
    rng = np.random.default_rng(seed)
    ant0, ant1 = (np.asarray([pq[k] for pq in PAIRS[:nbls]], dtype=np.int32) for k in (0, 1))
    p = FitProblem(nants=3, nfreqs=nfreqs, basis=[rng.standard_normal((nfreqs, 1)) for _ in range(nbls)], grp_basis=np.arange(nbls, dtype=np.int32),
                   grp_bl_start=np.arange(nbls + 1, dtype=np.int32), bl_ant0=ant0, bl_ant1=ant1, bl_rowblk=np.zeros(nbls, dtype=np.int32),
                   data_r=d_r, data_i=d_i, wgts=w0)
    p.validate()
    params = dict(g_r=1.0 + 0.2 * rng.standard_normal((3, nfreqs)), g_i=0.2 * rng.standard_normal((3, nfreqs)), c_r=np.zeros(nbls), c_i=np.zeros(nbls))
    return p, params


def solver_of(p, params, dtype, layout):
    from calamity_amd.solver import HipFitSolver

    s = HipFitSolver(dtype=dtype)
    s.set_problem(p, layout=layout, kernel_path="general")
    s.set_params(params["g_r"], params["g_i"], params["c_r"], params["c_i"])
    return s


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(UINT[a.dtype.itemsize])


def ulps_apart(a, b):
    """Distance in units of the last place between two arrays of one float dtype; two NaN count as equal, a NaN and a number as far."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    it = {4: np.int32, 8: np.int64}[a.dtype.itemsize]

    def ordered(x):  # an integer that is monotone in the value
        i = x.view(it).astype(np.int64)
        return np.where(i < 0, np.int64(np.iinfo(it).min) - i, i)

    oa, ob = ordered(a), ordered(b)
    far = np.abs(oa.astype(np.float64) - ob.astype(np.float64)) > 2.0**62  # (the int64 difference would wrap)
    d = np.where(far, np.inf, np.abs(oa - ob).astype(np.float64))
    return np.where(np.isnan(a) & np.isnan(b), 0.0, np.where(np.isnan(a) ^ np.isnan(b), np.inf, d))


def assert_precondition(s, d_r, d_i, w0, dtype):
    """m = A c is exactly zero, and the solver holds the weights and data that went in: they are of its dtype already."""
    m_r, m_i = s.model()
    assert not np.any(m_r) and not np.any(m_i)
    for a in (d_r, d_i, w0):
        assert a.dtype == np.dtype(dtype)
        np.testing.assert_array_equal(bits(s._real(a)), bits(a))
    np.testing.assert_array_equal(bits(s.get_weights(1)), bits(w0))


def exact_reference(d_r, d_i, w0, dtype, kind, k=K):
    """``robust_ref.robust_weights`` on the exact ``e``, the weights rounded once to the dtype; both selectors must name the same median."""
    e = R.residual_power_exact(d_r, d_i, w0, dtype)
    ref = R.robust_weights(e.astype(np.float64), w0.astype(np.float64), kind, k)
    for b in range(len(e)):
        sel = w0[b] > 0
        med = R.lower_median_bits(e[b][sel], dtype) if np.any(sel) else dtype(0)
        want = float(np.float64(med) / R.LN2) if med > 0 else 0.0
        assert ref["scale_bl"][b] == want, (b, ref["scale_bl"][b], want)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        ref["w"] = ref["w"].astype(dtype)
    ref["e"] = e
    return ref


def check_exact(out, w, ref, w0, kind, label):
    """Everything equal, no sample left out; prints the number of Huber and Cauchy weights that are not bit-identical."""
    assert out["scale_bl"].dtype == np.float64 and out["ndown_bl"].dtype == np.float64 and w.dtype == w0.dtype
    assert np.array_equal(out["scale_bl"], ref["scale_bl"]), (label, kind, out["scale_bl"], ref["scale_bl"])
    assert np.array_equal(out["ndown_bl"], ref["ndown_bl"]), (label, kind, out["ndown_bl"], ref["ndown_bl"])
    apart = ulps_apart(w, ref["w"])
    differ = int(np.count_nonzero(apart))
    if kind != "clip":
        print(f"{label} {kind}: {differ} of {w.size} weights not bit-identical, at most {apart.max():.0f} ulp apart")
    assert differ == 0, (label, kind, differ, float(apart.max()))
    np.testing.assert_array_equal(w < w0, ref["w"] < w0, err_msg=f"{label} {kind}: the set of down-weighted samples")
    np.testing.assert_array_equal(bits(w)[w0 <= 0], bits(w0)[w0 <= 0], err_msg=f"{label} {kind}: flagged samples keep their bits")


def run_rows(rows, dtype, layout, label, kinds=R.KINDS, k=K):
    """One solver over ``rows``; every kind in turn (each call starts from w0).  Returns {kind: (out, w, ref)}."""
    d_r, d_i, w0 = rows
    p, params = problem_of(d_r, d_i, w0)
    s = solver_of(p, params, dtype, layout)
    assert_precondition(s, d_r, d_i, w0, dtype)
    got = {}
    for kind in kinds:
        ref = exact_reference(d_r, d_i, w0, dtype, kind, k)
        out = s.robust_weights(kind=kind, threshold=k)
        w = s.get_weights()
        check_exact(out, w, ref, w0, kind, label)
        np.testing.assert_array_equal(bits(s.get_weights(1)), bits(w0))
        got[kind] = (out, w, ref)
    s.close()
    return got


def chunks_of(rows, n=4):
    return [tuple(a[i : i + n] for a in rows) for i in range(0, len(rows[0]), n)]


@functools.lru_cache(maxsize=None)
def short_families(dtype_name):
    return RF.short_families(np.dtype(dtype_name).type)


def family(name, dtype):
    return short_families(np.dtype(dtype).name)[name]


def label_of(name, dtype, layout):
    return f"{name} {np.dtype(dtype).name} {layout}"


# ---- 1. the short rows
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_ties_at_the_median(layout, dtype):
    """Five rows (a second block with one busy wave).  Row 2 holds one repeated value: z2 = ln 2 everywhere."""
    rows = family("ties", dtype)
    assert len(rows[0]) == 5
    got = run_rows(rows, dtype, layout, label_of("ties", dtype, layout))
    w0 = rows[2]
    for kind in R.KINDS:
        out, w, ref = got[kind]
        assert np.all(out["scale_bl"] > 0)
        e = ref["e"]
        assert out["scale_bl"][2] == float(e[2, 0]) / R.LN2
        # the lower of the two middle order statistics, which are one ulp apart: the 100th of 200
        assert out["scale_bl"][3] == float(np.sort(e[3])[99]) / R.LN2 != float(np.sort(e[3])[100]) / R.LN2
        # 199 good samples: the 100th is the first of a run of equal values, the 99th one ulp below it
        e4 = np.sort(e[4][w0[4] > 0])
        assert out["scale_bl"][4] == float(e4[99]) / R.LN2 != float(e4[98]) / R.LN2 and e4[99] == e4[100]
        if kind == "cauchy":
            psi = 1.0 / (1.0 + R.LN2 / (K * K))
            assert np.all(w[2] == w[2, 0]) and abs(float(w[2, 0]) - psi) <= 2 * np.finfo(dtype).eps and out["ndown_bl"][2] == w.shape[1]
        else:
            assert out["ndown_bl"][2] == 0
            np.testing.assert_array_equal(bits(w[2]), bits(w0[2]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("trips", [1, 2], ids=["W+1", "2W+3"])
def test_counts_on_both_sides_of_a_trip_of_the_wave(trips, layout, dtype):
    """n_b = 1, 2, 3, W - 1, W, W + 1 (and 2 W) good samples among W + 1 (2 W + 3) channels, the few at channel 0, at the last channel
    or in the partly filled last vector; the good samples have distinct ``e`` and the flagged ones large data."""
    v, wave = RF.lanes(dtype)
    name = "counts_W+1" if trips == 1 else "counts_2W+3"
    rows = family(name, dtype)
    assert rows[0].shape == (8, trips * wave + (1 if trips == 1 else 3))
    for i, part in enumerate(chunks_of(rows)):
        got = run_rows(part, dtype, layout, label_of(f"{name}[{4 * i}:{4 * i + 4}]", dtype, layout))
        for kind in R.KINDS:
            assert np.all(got[kind][0]["scale_bl"] > 0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_keys_over_the_whole_exponent_range_and_in_the_lowest_bits(layout, dtype):
    rows = family("whole_range", dtype)
    got = run_rows(rows, dtype, layout, label_of("whole_range", dtype, layout))
    fi = np.finfo(dtype)
    for kind in R.KINDS:
        out, w, ref = got[kind]
        e = ref["e"]
        assert np.any((e[0] > 0) & (e[0] < fi.tiny)) and np.any(np.isinf(e[0])) and np.isinf(e[0]).sum() < e.shape[1] // 2
        assert np.all(out["scale_bl"] > 0) and np.all(np.isfinite(out["scale_bl"]))
        assert np.all(w[0][np.isinf(e[0])] == 0) and out["ndown_bl"][0] >= np.isinf(e[0]).sum()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_zero_median_on_the_device(layout, dtype):
    rows = family("zero_median", dtype)
    got = run_rows(rows, dtype, layout, label_of("zero_median", dtype, layout))
    w0 = rows[2]
    for kind in R.KINDS:
        out, w, ref = got[kind]
        for b in (0, 1, 3):  # more than half, exactly half (n_b even), (n_b + 1) / 2 (n_b odd): the row keeps the bits of w0
            assert out["scale_bl"][b] == 0 and out["ndown_bl"][b] == 0
            np.testing.assert_array_equal(bits(w[b]), bits(w0[b]))
        e2 = ref["e"][2][w0[2] > 0]
        assert out["scale_bl"][2] == float(np.min(e2[e2 > 0])) / R.LN2  # half minus one: the smallest positive sample


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_nan_and_infinite_samples_with_positive_weight(layout, dtype):
    """What include/calamity_hip.h states: a NaN orders above every number, so rows 0 and 1 have a number for their median (row 1 the
    largest of the row) and rows 2 and 3 keep w0; behind a finite scale a NaN sample gets a NaN weight under Huber and Cauchy and is not
    counted, weight 0 under clip and is counted; an infinite sample gets 0 under every kind and is counted."""
    rows = family("non_finite", dtype)
    got = run_rows(rows, dtype, layout, label_of("non_finite", dtype, layout))
    w0 = rows[2]
    for kind in R.KINDS:
        out, w, ref = got[kind]
        e = ref["e"]
        for b in (2, 3):
            assert out["scale_bl"][b] == 0 and out["ndown_bl"][b] == 0
            np.testing.assert_array_equal(bits(w[b]), bits(w0[b]))
        sel1 = w0[1] > 0
        assert out["scale_bl"][1] == float(np.nanmax(e[1][sel1])) / R.LN2
        for b in (0, 1):
            sel = w0[b] > 0
            nan, inf = np.isnan(e[b]) & sel, np.isinf(e[b]) & sel
            assert nan.sum() > 0 and (b == 1 or inf.sum() == 5)
            assert np.all(w[b][inf] == 0)
            if kind == "clip":
                assert np.all(w[b][nan] == 0) and out["ndown_bl"][b] == np.sum(w[b][sel] == 0) >= nan.sum() + inf.sum()
            else:
                assert np.all(np.isnan(w[b][nan])) and np.all(np.isfinite(w[b][~nan]))
                assert out["ndown_bl"][b] == np.sum(w[b][sel & ~nan] < w0[b][sel & ~nan])


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_call_reports_nothing_left_over_from_the_call_before(dtype):
    """Huber at k = 1 fills every row's scale and count; then new data whose rows 0 and 1 have a zero median and no good sample, a
    clip call, a Cauchy call and kind "none" on the same solver: each reports its own rows alone."""
    d_r, d_i, w0 = (a[[4, 5, 6, 7]] for a in family("counts_2W+3", dtype))
    p, params = problem_of(d_r, d_i, w0)
    s = solver_of(p, params, dtype, "shared")
    assert_precondition(s, d_r, d_i, w0, dtype)
    ref = exact_reference(d_r, d_i, w0, dtype, "huber", 1.0)
    first = s.robust_weights(kind="huber", threshold=1.0)
    check_exact(first, s.get_weights(), ref, w0, "huber", f"first call {np.dtype(dtype).name}")
    assert np.all(first["scale_bl"] > 0) and np.all(first["ndown_bl"] > 0)
    d2_r, d2_i, w2 = d_r.copy(), d_i.copy(), w0.copy()
    good = np.flatnonzero(w0[0] > 0)
    d2_r[0, good[: len(good) // 2 + 1]] = 0
    d2_i[0, good[: len(good) // 2 + 1]] = 0
    w2[1] = 0
    s.set_data(d2_r, d2_i, w2)
    for kind, k in (("clip", 30.0), ("cauchy", K), ("huber", K)):
        ref = exact_reference(d2_r, d2_i, w2, dtype, kind, k)
        out = s.robust_weights(kind=kind, threshold=k)
        check_exact(out, s.get_weights(), ref, w2, kind, f"after set_data {np.dtype(dtype).name}")
        assert not np.any(out["scale_bl"][:2]) and not np.any(out["ndown_bl"][:2]) and np.all(out["scale_bl"][2:] > 0)
        if kind == "clip":  # k = 30: z2 <= 900 for every sample of these rows: nothing is left of the counts of the call before
            assert not np.any(out["ndown_bl"])
        if kind == "cauchy":
            np.testing.assert_array_equal(out["ndown_bl"][2:], np.sum(w2[2:] > 0, axis=1))
    out = s.robust_weights(kind="none")
    assert not np.any(out["scale_bl"]) and not np.any(out["ndown_bl"])
    np.testing.assert_array_equal(bits(s.get_weights()), bits(w2))
    s.close()


# ---- 2. the LDS limit
def lds_nfreqs(dtype):
    return 65536 // (4 * np.dtype(dtype).itemsize)


@functools.lru_cache(maxsize=None)
def limit_rows(dtype_name):
    dtype = np.dtype(dtype_name).type
    rows = RF.lds_limit(lds_nfreqs(dtype), dtype)
    return rows, RF.one_more_flagged_channel(rows)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_longest_row_of_the_lds_form_and_the_first_past_it(dtype):
    """The same 4096 (2048) channels in both forms -- the longer problem's extra channel is flagged -- so S_b and e are the same: each
    form equals the exact reference, and the two agree bit for bit on the shared channels."""
    n = lds_nfreqs(dtype)
    at, past = limit_rows(np.dtype(dtype).name)
    assert at[0].shape == (4, n) and past[0].shape == (4, n + 1) and not np.any(past[2][:, -1])
    got_at = run_rows(at, dtype, "shared", f"lds_limit {n} {np.dtype(dtype).name}")
    got_past = run_rows(past, dtype, "shared", f"lds_limit {n + 1} {np.dtype(dtype).name}")
    for kind in R.KINDS:
        (out_a, w_a, _), (out_p, w_p, _) = got_at[kind], got_past[kind]
        np.testing.assert_array_equal(out_a["scale_bl"], out_p["scale_bl"])
        np.testing.assert_array_equal(out_a["ndown_bl"], out_p["ndown_bl"])
        np.testing.assert_array_equal(bits(w_a), bits(w_p[:, :n]))
        assert np.all(out_a["scale_bl"] > 0) and np.all(out_a["ndown_bl"][2:] > n // 4) and not np.any(w_p[:, n])


@functools.lru_cache(maxsize=None)
def long_problem(dtype_name):
    """One channel past the LDS form, non-zero coefficients: data = the model under the gains plus noise, 2 % of the samples far off."""
    nfreqs = lds_nfreqs(np.dtype(dtype_name).type) + 1
    rng = np.random.default_rng(11)
    zero = np.zeros((4, nfreqs))
    p, params = problem_of(zero, zero, np.ones((4, nfreqs)), seed=12)
    params = dict(params, c_r=rng.standard_normal(4), c_i=rng.standard_normal(4))
    g = params["g_r"] + 1j * params["g_i"]
    m = np.stack([p.basis[b][:, 0] * (params["c_r"][b] + 1j * params["c_i"][b]) for b in range(4)])
    d = g[p.bl_ant0] * np.conj(g[p.bl_ant1]) * m + 0.3 * (rng.standard_normal(m.shape) + 1j * rng.standard_normal(m.shape))
    d = d + np.where(rng.random(m.shape) < 0.02, 10.0, 0.0)
    p.data_r, p.data_i = np.ascontiguousarray(d.real), np.ascontiguousarray(d.imag)
    p.wgts = rng.uniform(0.5, 1.5, m.shape) * (rng.random(m.shape) > 0.1)
    return p, params


def state_of(s):
    return dict(zip(("g_r", "g_i", "c_r", "c_i"), s.get_params()), **s.get_moments())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", ["graph", "kernels"])
def test_a_descent_continued_behind_the_form_that_keeps_its_keys_in_the_model_plane(mode, dtype):
    """The call overwrites the row of the model_r plane with keys.  ``model()`` returns the bits it returned before, and 20 Adam steps
    continued behind the call equal, bit for bit, those of a fresh solver given the same weights through ``set_data``."""
    p, params = long_problem(np.dtype(dtype).name)
    got, w_clip = {}, None
    for how in ("call", "upload"):
        s = solver_of(p, params, dtype, "shared")
        s.set_launch_mode(mode)
        s.set_optimizer("Adam", learning_rate=1e-2)
        first = s.run(20, tol=0.0)[0]
        if how == "call":
            before = s.model()
            out = s.robust_weights(kind="clip", threshold=2.0)
            w_clip = s.get_weights()
            assert np.all(out["scale_bl"] > 0) and np.all(out["ndown_bl"] > 0) and np.sum(w_clip == 0) > np.sum(p.wgts == 0)
            assert np.any(before[0]) and np.any(before[1])
            for a, b in zip(before, s.model()):
                np.testing.assert_array_equal(bits(a), bits(b))
        else:
            s.set_data(p.data_r, p.data_i, w_clip)
        got[how] = (np.concatenate([first, s.run(20, tol=0.0)[0]]), state_of(s))
        s.close()
    assert len(got["call"][0]) == 40 and np.all(np.isfinite(got["call"][0]))
    np.testing.assert_array_equal(got["call"][0], got["upload"][0])
    for k, v in got["upload"][1].items():
        np.testing.assert_array_equal(got["call"][1][k], v, err_msg=k)
    assert got["call"][0][20] < got["call"][0][19]  # the clipped chi-square is smaller
