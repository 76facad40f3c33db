"""The six post-fit reports behind a ``robust_weights`` call: include/calamity_hip.h promises ONE weight plane that everything reads,
tests/test_gpu_robust_consumers.py holds fit quality, the closed-form solves, ``init_coeffs`` and ``eval`` to it, and this file the
reports, which read ``wgts`` through ``coeff_planes``, ``gain_planes``, ``fit_error_rows_kernel`` (``nsamp_bl``),
``degen_rows_kernel`` (``fix_degeneracies`` with ``ref_w=None``) and ``dcross_rows_kernel`` (``delay_cross_spectrum``: the weights of BOTH rows
of a pair, as a mask -- a stale plane on one side alone changes the common mask, ``norm_pair`` and every statistic).

The scheme is that file's.  Solver A calls ``robust_weights("clip", 2.0)`` and then the report; solver B is a fresh solver given A's
weights through ``set_data``.  B has never seen ``w0``, so a report of A that took anything from the plane of ``w0`` or from a plane
cached before the reweight differs from B.  Everything is compared bit for bit, on every kernel path of tests/test_gpu_solve_paths.py
(every solver asserts the path it asked for).  The cases are those of tests/report_cases.py; Huber at k = 2 once, and once more for the cross spectrum, which
reads the weights as a mask alone: behind Huber (new values, the same zeros) it keeps every bit of a solver that never reweighted.  ``fix_degeneracies``
reads the solver's weights only with ``ref_w=None``; with ``ref_w`` given its result is bit-identical with and without the reweight.

On ``general`` and ``dense`` the reports are also held to their restatements on a copy of the problem whose weights are A's, with the
``check`` and ``TOL`` of each report's own file -- after asserting that the restatement under the new weights differs from the one
under ``w0`` by more than 100 x ``TOL`` in every plane and in the chi-square (``assert_the_weights_matter``; a condition on the inputs
that the restatement alone decides, asserted without a device in tests/test_report_paths_host.py: 11 to 19 % of the good samples
are clipped).  ``nsamp_bl`` and ``nsamples`` are integers: equal to the count of non-zero new weights, unequal to the count under
``w0``.  The outputs whose restatement cannot move that far in fp32 (``BELOW_MARGIN_FP32`` of tests/report_cases.py, with the margins
the restatement did reach: ``leverage_bl`` 3.4e-6 and 1.3e-4, ``gain_dof`` 2.7e-8 to 2.2e-7, and ``eta`` 3.7e-4, ``tilt`` 8.1e-4,
``model`` 7.0e-4 of ``fix_degeneracies`` in band mode, against 1e-2) are left out of that precondition in fp32: there the comparison
with B is what holds them.

Three slices with the middle one reweighted (``slice_mask=[0, 1, 0]``): the rows of slices 0 and 2 of ``fit_errors``,
``delay_spectrum``, ``delay_cross_spectrum`` (within-slice pairs) and ``delay_transfer`` equal a solver that never reweighted, all rows a
solver given the mixed plane; and the same-baseline pairs of the slices (0, 1), (1, 2) and (0, 2), of which the first two have ONE side
in the reweighted slice: every output the mixed-plane solver's, the (0, 2) pairs the never-reweighted solver's, ``norm_pair`` of the
others not.  A
``robust_weights("none")`` behind the reports restores ``w0``, and a report behind it equals the report of a fresh solver.

Shown once on scratch copies of the library (each inside its buffers: wrong numbers, no fault; each passes the older report files):
in each the named reader takes ``rw_w0`` (the plane of ``w0``) once a reweight has run.  (a) = ``..._equals_a_fresh_solver_given_the_same_weights``,
(b) = ``..._equals_its_restatement_under_the_new_weights``, (c) = ``test_three_slices_with_the_middle_one_reweighted``, (d) =
``..._behind_robust_weights_none_...`` (whose last line asserts that the report under the clipped weights was another one).

  * ``fit_error_rows_kernel`` (``nsamp_bl``): fails 24 -- the 12 clip cases of ``fit_errors`` in (a) (Huber leaves no zero weight:
    ``nsamp_bl`` cannot see it), its 8 in (b), the 4 of (c);
  * ``coeff_planes`` of the reports (``fit_errors``, ``delay_transfer``; ``solve_coeffs`` left right): fails 50 -- the 18
    ``fit_errors`` cases of (a) with Huber, the 12 of ``delay_transfer``, 8 + 8 in (b), the 4 of (c);
  * ``gain_planes`` of the reports (``gain_var`` of ``fit_errors``, ``gain_basis_errors``; the sweeps left right): fails 86 -- 18 + 24
    in (a), 8 + 16 in (b), the 4 of (c), the 16 ``gain_basis_errors`` cases of (d);
  * ``fix_degeneracies`` with ``ref_w`` null: fails 28 -- the 12 ``_own_w`` cases of (a), 8 in (b), 8 in (d); the control with ``ref_w``
    given passes;
  * ``dspec_rows_kernel`` of ``delay_spectrum``: fails 32 -- 12 in (a), 8 in (b), the 4 of (c), 8 in (d);
  * ``dtransfer_power_kernel``'s own weight argument in ``delay_transfer`` (``coeff_planes`` left right): fails 24 -- 12 in (a), 8 in
    (b), the 4 of (c).

  * ``dcross_rows_kernel`` given ``rw_w0`` for BOTH sides of a pair: fails 36 -- the 12 ``delay_cross`` cases of (a), 8 in (b), the 4 of
    (c) (its within-slice pairs), the 4 of ``test_pairs_with_one_side_in_the_reweighted_middle_slice``, 8 in (d);
  * ``dcross_rows_kernel`` given ``rw_w0`` for side 1 alone: fails 28 -- 12 in (a), 8 in (b), the 4 of (c), the 4 of
    ``test_pairs_with_one_side_in_the_reweighted_middle_slice``; (d) passes (side 0 makes the clipped report another one).  Neither can
    fail the Huber case, which is there for a reader of the weights' VALUES: Huber leaves the zeros of ``w0`` where they are.

The two of ``dcross_rows_kernel`` also pass tests/test_gpu_delay_cross.py, test_gpu_delay_cross_dropin.py and
test_gpu_delay_cross_ranks.py as they stood before (60 tests: none reweights).  Each fails cases of its own report alone, passes every test of tests/test_gpu_report_paths.py (which never reweights) and the 742
tests of the older files (tests/test_gpu_fit_errors.py, test_gpu_gain_basis_errors.py, test_gpu_delay_spectrum.py,
test_gpu_delay_transfer.py, test_gpu_degeneracy.py, test_gpu_robust_consumers.py, test_gpu_solve_paths.py).  The two builds that are
wrong on the dense paths only are listed in tests/test_gpu_report_paths.py."""
import numpy as np
import pytest

import report_cases as C
import test_gpu_delay_spectrum as DS
from test_gpu_report_paths import afterwards, outputs, rows_of_slice, slice_reports
from test_gpu_robust_consumers import CLIP, HUBER, assert_the_weights_matter, reweighted, slice_solver, uploaded
from test_gpu_solve_paths import PATHS, REG_PATHS, assert_path, assert_same_bits, check_loss, path_id, three_slices

pytestmark = pytest.mark.gpu

PATH_IDS = list(map(path_id, PATHS))
READERS = [(c, CLIP) for c in C.WEIGHT_READERS] + [(("fit_errors", "7x200"), HUBER)]


def reader_id(arg):
    return C.case_id(arg[0]) + ("-huber" if arg[1] is HUBER else "")


def solver_a(case, dtype, path, how=CLIP):
    return reweighted(*case, dtype, path, how, given=C.inputs(*case))


def read(s, case):
    """The report, flat, and fit quality afterwards."""
    out = C.flat(C.call(s, *case))
    out.update({f"quality_{k}": v for k, v in s.fit_quality().items()})
    return out


# ---- (a) A against B
@pytest.mark.parametrize("dtype,path", PATHS, ids=PATH_IDS)
@pytest.mark.parametrize("case,how", READERS, ids=map(reader_id, READERS))
def test_a_report_behind_the_call_equals_a_fresh_solver_given_the_same_weights(case, how, dtype, path):
    a, w, w0 = solver_a(case, dtype, path, how)
    b = uploaded(*case, dtype, path, w, given=C.inputs(*case))
    got, want = read(a, case), read(b, case)
    np.testing.assert_array_equal(a.get_weights(1), w0)
    np.testing.assert_array_equal(a.get_weights(0), w)
    for s in (a, b):
        assert_path(s, path)
        s.close()
    assert_same_bits(got, want, f"{C.case_id(case)} {path} {np.dtype(dtype).name} behind {how[0]}")


@pytest.mark.parametrize("dtype,path", PATHS, ids=PATH_IDS)
@pytest.mark.parametrize("case", C.GIVEN_REF_W, ids=map(C.case_id, C.GIVEN_REF_W))
def test_fix_degeneracies_with_ref_w_given_does_not_read_the_solver_s_weights(case, dtype, path):
    """The control: the same bits with and without the reweight (``fit_quality`` afterwards does read the plane, and differs)."""
    a, w, w0 = solver_a(case, dtype, path)
    got = C.flat(C.call(a, *case))
    assert_path(a, path)
    a.close()
    want = C.flat(outputs(case, np.dtype(dtype).name, path)[0])
    assert_same_bits(got, want, f"{C.case_id(case)} {path} {np.dtype(dtype).name}")


@pytest.mark.parametrize("dtype,path", PATHS, ids=PATH_IDS)
@pytest.mark.parametrize("variant", ["raw", "calibrated"])
def test_the_cross_spectrum_reads_the_weights_as_a_mask_huber_changes_no_bit(variant, dtype, path):
    """Huber at k = 2 changes weights and zeroes none; ``dcross_rows_kernel`` reads ``w != 0`` alone: the bits of a solver that never
    reweighted (``fit_quality`` afterwards does read the values)."""
    case = ("delay_cross", variant)
    a, w, w0 = solver_a(case, dtype, path, HUBER)
    now = a.get_weights(0)
    assert np.any(now != w0) and np.array_equal(now == 0, w0 == 0) and np.array_equal(now, w)
    got = C.flat(C.call(a, *case))
    assert_path(a, path)
    a.close()
    want = C.flat(outputs(case, np.dtype(dtype).name, path)[0])
    assert_same_bits(got, want, f"{C.case_id(case)} {path} {np.dtype(dtype).name} behind huber")


# ---- (b) A against the restatement under its weights
@pytest.mark.parametrize("dtype,path", REG_PATHS, ids=map(path_id, REG_PATHS))
@pytest.mark.parametrize("case", C.WEIGHT_READERS, ids=map(C.case_id, C.WEIGHT_READERS))
def test_a_report_behind_the_call_equals_its_restatement_under_the_new_weights(case, dtype, path):
    kind = case[0]
    p = C.inputs(*case)[0]
    label = f"{C.case_id(case)} {path} {np.dtype(dtype).name}"
    a, w, w0 = solver_a(case, dtype, path)
    model = None
    if kind == "fix_degeneracies":
        m_r, m_i = a.model()
        model = m_r.astype(np.float64) + 1j * m_i.astype(np.float64)
    moved, _, new, old = C.margins(*case, dtype, w, model)
    skip = C.below_margin(case, dtype)
    planes_new, planes_old = C.matter_planes(kind, new), C.matter_planes(kind, old)
    chisq_new, chisq_old = C.chisq_of(*case, dtype, C.with_weights(p, w)), C.chisq_of(*case, dtype)
    assert_the_weights_matter(({k: v for k, v in planes_new.items() if k not in skip}, chisq_new),
                              ({k: v for k, v in planes_old.items() if k not in skip}, chisq_old), dtype, label)
    raw = C.call(a, *case)
    quality = a.fit_quality()
    assert_path(a, path)
    a.close()
    if kind == "delay_cross":  # no integer output: norm_pair is the common mask's sum, at the tolerance of the report's own file
        pairs = C.cross_pairs(*case)[0]
        norm_f = C.delay_operator(*case)[1]
        common = lambda ww: ((ww[pairs[:, 0]] != 0) & (ww[pairs[:, 1]] != 0)).astype(np.float64) @ norm_f  # noqa: E731
        np.testing.assert_allclose(raw["norm_pair"], common(w), rtol=1e-13, atol=0, err_msg=label)
        assert not np.array_equal(raw["norm_pair"], common(w0)), label
    counts = C.sample_counts(kind, new)
    if counts is not None:
        key = "nsamp_bl" if kind == "fit_errors" else "nsamples"
        want = np.count_nonzero(w, axis=1) if kind == "fit_errors" else np.where(new["nsamples"] > 0, np.count_nonzero(w > 0, axis=0), 0)
        np.testing.assert_array_equal(np.ravel(raw[key]), want, err_msg=label)
        np.testing.assert_array_equal(counts, want, err_msg=label)
        assert np.any(counts != C.sample_counts(kind, old)), label
    C.check(*case, raw, new, dtype, label)
    check_loss(float(quality["chisq_bl"].sum()), chisq_new, dtype, label + " (fit quality afterwards)")


# ---- (c) three slices, the middle one reweighted
@pytest.mark.parametrize("dtype,path", REG_PATHS, ids=map(path_id, REG_PATHS))
def test_three_slices_with_the_middle_one_reweighted(dtype, path):
    p0 = three_slices()[0]
    nb = p0.nbls
    a = slice_solver(dtype, path)
    w_in = a.get_weights()
    down = a.robust_weights(*CLIP, slice_mask=[0, 1, 0])
    w = a.get_weights()
    mid = slice(nb, 2 * nb)
    assert down["ndown_bl"][mid].sum() > 0 and np.any((w[mid] == 0) & (w_in[mid] > 0))
    for rows in (slice(0, nb), slice(2 * nb, 3 * nb)):
        np.testing.assert_array_equal(w[rows], w_in[rows])
    b, c = slice_solver(dtype, path, wgts=w), slice_solver(dtype, path)
    results = []
    for s in (a, b, c):
        results.append(slice_reports(s, nb, 3))
        assert_path(s, path)
        s.close()
    got, mixed, never = results
    for name in got:
        assert_same_bits(got[name], mixed[name], f"{name} {path} {np.dtype(dtype).name}: against the solver given the mixed plane")
        differs = False
        for key, arr in got[name].items():
            if np.isscalar(arr):
                continue
            for t in (0, 2):
                np.testing.assert_array_equal(rows_of_slice(name, key, arr, t, p0), rows_of_slice(name, key, never[name][key], t, p0),
                                              err_msg=f"{name} {key}: slice {t} against a solver that never reweighted")
            differs |= not np.array_equal(rows_of_slice(name, key, arr, 1, p0), rows_of_slice(name, key, never[name][key], 1, p0))
        assert differs, name


def slice_pairs(nb):
    """Same-baseline pairs of the slices (0, 1), (1, 2) and (0, 2), nb each, with seeded unequal scales and one bin per slice pair."""
    pairs = np.array([(t0 * nb + b, t1 * nb + b) for t0, t1 in ((0, 1), (1, 2), (0, 2)) for b in range(nb)], dtype=np.int32)
    scale = np.random.default_rng(11).uniform(0.5, 2.0, size=(len(pairs), 2))
    return pairs, scale, np.repeat(np.arange(3), nb).astype(np.int32), 3


@pytest.mark.parametrize("dtype,path", REG_PATHS, ids=map(path_id, REG_PATHS))
def test_pairs_with_one_side_in_the_reweighted_middle_slice(dtype, path):
    """The pairs (slice 0, slice 1) and (slice 1, slice 2) have ONE side in the reweighted slice: a reader that took either side from
    the plane of ``w0`` differs from the solver given the mixed plane.  The pairs (slice 0, slice 2) touch no new weight."""
    p0 = three_slices()[0]
    nb = p0.nbls
    pairs, scale, bins, nbins = slice_pairs(nb)
    op, norm_f = DS.operator(200, 200)
    a = slice_solver(dtype, path)
    w_in = a.get_weights()
    a.robust_weights(*CLIP, slice_mask=[0, 1, 0])
    w = a.get_weights()
    assert np.any((w[nb : 2 * nb] == 0) & (w_in[nb : 2 * nb] > 0)) and np.array_equal(w[:nb], w_in[:nb]) and np.array_equal(w[2 * nb :], w_in[2 * nb :])
    results = []
    for s in (a, slice_solver(dtype, path, wgts=w), slice_solver(dtype, path)):
        results.append(C.flat(s.delay_cross_spectrum(op, norm_f, pairs, scale=scale, bin_of_pair=bins, nbins=nbins, per_pair=True)))
        assert_path(s, path)
        s.close()
    got, mixed, never = results
    label = f"{path} {np.dtype(dtype).name}"
    assert_same_bits(got, mixed, label + ": against the solver given the mixed plane")
    far, near = slice(2 * nb, 3 * nb), slice(0, 2 * nb)
    for key, arr in got.items():
        if key.startswith("per_pair_") or key == "norm_pair":
            np.testing.assert_array_equal(arr[far], never[key][far], err_msg=f"{label} {key}: the pairs (slice 0, slice 2) against a solver that never reweighted")
        else:
            np.testing.assert_array_equal(arr[2], never[key][2], err_msg=f"{label} {key}: the bin of the pairs (slice 0, slice 2)")
    changed = got["norm_pair"][near] != never["norm_pair"][near]
    print(f"{label}: norm_pair differs in {changed[:nb].sum()} of {nb} pairs (0, 1) and {changed[nb:].sum()} of {nb} pairs (1, 2)")
    assert changed[:nb].any() and changed[nb:].any(), label  # (slice 1 is side 1 of the first and side 0 of the second)


# ---- (d) back to w0
@pytest.mark.parametrize("dtype,path", REG_PATHS, ids=map(path_id, REG_PATHS))
@pytest.mark.parametrize("case", C.WEIGHT_READERS, ids=map(C.case_id, C.WEIGHT_READERS))
def test_a_report_behind_robust_weights_none_equals_the_report_of_a_fresh_solver(case, dtype, path):
    a, w, w0 = solver_a(case, dtype, path)
    first = C.flat(C.call(a, *case))
    a.robust_weights("none")
    np.testing.assert_array_equal(a.get_weights(0), w0)
    np.testing.assert_array_equal(a.get_weights(1), w0)
    got = dict(C.flat(C.call(a, *case)), **afterwards(a))
    assert_path(a, path)
    a.close()
    want = outputs(case, np.dtype(dtype).name, path)[1]
    label = f"{C.case_id(case)} {path} {np.dtype(dtype).name}"
    assert_same_bits(got, want, label + " behind robust_weights('none')")
    moved = [k for k in first if not np.isscalar(first[k]) and k not in ("m_r", "m_i") and not np.array_equal(first[k], got[k])]
    assert moved, label  # (the report under the clipped weights was another one)
