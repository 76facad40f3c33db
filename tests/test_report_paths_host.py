"""The table of cases behind tests/test_gpu_report_paths.py and tests/test_gpu_robust_reports.py (tests/report_cases.py), held to what
the two GPU files assume of it, without a device -- so a case cannot quietly stop reaching its branch:

  * every parity input has ``cond(N) <= COND_MAX``, the bound the report's own file asserts (``fit_errors``, ``delay_transfer``), under
    the problem's weights and under the clipped ones;
  * every case that reads the weight plane meets the weights-matter precondition of the robust tests with the weights of
    tests/robust_ref.py at clip k = 2, in both dtypes: every plane of the restatement and the chi-square move by more than 100 x ``TOL``
    (the outputs of ``BELOW_MARGIN_FP32`` are asserted to stay BELOW it in fp32 and above it in fp64), the integer outputs change, and
    between 5 % and 30 % of the good samples are clipped;
  * every case reaches its shape branch: more than 64 channels and one baseline per fitting group (what the dense paths need), the
    K = 65 case a ``W`` past one 64-row block, the flagged channel and the flagged antenna of the ``fix_degeneracies`` reference still
    there at 72 channels;
  * the pairs of the ``delay_cross`` cases keep what makes the common mask matter: exactly the two pairs that touch the wholly flagged
    row have ``norm_pair == 0``, under ``w0`` and under the clipped weights, and a pair's common mask differs from both rows' own."""
import numpy as np
import pytest

import report_cases as C
from test_delay_transfer_host import fe_pad
from test_gpu_coeff_solve import COND_MAX
from test_gpu_fit_quality import TOL

DTYPES = [np.float32, np.float64]
CASE_IDS = list(map(C.case_id, C.CASES))
READER_IDS = list(map(C.case_id, C.WEIGHT_READERS))


@pytest.mark.parametrize("case", C.CASES, ids=CASE_IDS)
def test_every_shape_qualifies_for_the_dense_paths(case):
    p, params, B, Bt = C.inputs(*case)
    assert p.nfreqs > 64 and np.all(np.diff(p.grp_bl_start) == 1) and p.ngrps == p.nbls
    for k in ("g_r", "g_i"):
        assert np.asarray(params[k]).shape == (p.nants, p.nfreqs)
    assert B is None or B.shape[0] == p.nfreqs
    assert Bt is None or p.nants % Bt.shape[0] == 0


def test_the_table_holds_the_shapes_it_is_meant_to():
    shapes = {C.case_id(c): (C.inputs(*c)[0].nants, C.inputs(*c)[0].nfreqs) for c in C.CASES}
    assert shapes["fit_errors-7x200"] == (7, 200) and shapes["fit_errors-12x129"] == (12, 129)
    assert shapes["gain_basis_errors-freq_K12"] == shapes["gain_basis_errors-freq_K65"] == (7, 200)
    assert shapes["gain_basis_errors-time_freq"] == shapes["gain_basis_errors-time"] == (4 * 5, 72)
    assert all(shapes[f"{kind}-{v}"] == (7, 200) for kind in ("delay_spectrum", "delay_cross", "delay_transfer") for v in ("raw", "calibrated"))
    pairs, scale, bins, nbins = C.cross_pairs()
    nb = C.inputs("delay_cross", "raw")[0].nbls
    assert nb == 22 and pairs.shape == scale.shape == (nb + 2, 2) and bins.shape == (nb + 2,) and nbins == 4 and bins.max() == 2 and bins.min() == -1
    assert [tuple(pr) for pr in pairs[:nb]] == [(b, (b + 3) % nb) for b in range(nb)] and tuple(pairs[nb]) == (2, 2) and tuple(pairs[nb + 1]) == (nb - 1, 0)
    unequal = np.delete(scale, nb, axis=0)
    assert np.all(scale[nb] == 1.0) and np.all(unequal != 1.0) and np.all(unequal[:, 0] != unequal[:, 1])
    assert C.delay_operator("delay_cross", "raw")[0].shape == (200, 200)
    assert all(v == (7, C.DEGEN_NF) for k, v in shapes.items() if k.startswith("fix_degeneracies")) and C.DEGEN_NF == 72
    K = {v: C.inputs("gain_basis_errors", v)[2].shape[1] for v in ("freq_K12", "freq_K65")}
    assert K == {"freq_K12": 12, "freq_K65": 65}
    assert fe_pad(65) > 64 >= fe_pad(12)  # W of the K = 65 case runs past one 64-row block
    _, _, B, Bt = C.inputs("gain_basis_errors", "time_freq")
    assert Bt.shape == (4, 3) and B.shape == (72, 10)  # (not three times under three time vectors: ill-conditioned)
    _, _, B, Bt = C.inputs("gain_basis_errors", "time")
    assert Bt.shape == (4, 3) and B is None
    op, norm_f = C.delay_operator("delay_spectrum", "raw")
    assert op.shape == (200, 200) and norm_f.shape == (200,)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [c for c in C.CASES if c[0] in ("fit_errors", "delay_transfer")], ids=C.case_id)
def test_every_parity_input_is_well_conditioned(case, dtype):
    ref = C.reference(*case, np.dtype(dtype).name)
    print(f"{C.case_id(case)} {np.dtype(dtype).name}: largest cond(N) {max(ref['conds']):.3e}")
    assert max(ref["conds"]) <= COND_MAX
    assert ref["singular"] == ([0] if case[0] == "fit_errors" else [1])  # the wholly flagged row is the one singular group


@pytest.mark.parametrize("mode", ["channel", "band"])
def test_the_flags_of_the_degeneracy_reference_survive_the_move_to_72_channels(mode):
    p = C.inputs("fix_degeneracies", mode)[0]
    ref_r, ref_i, antpos, kw, ref_w = C.degeneracy_args(mode)
    assert ref_r.shape == ref_w.shape == (21, 72) and antpos.shape == (7, 2) and kw["ref_w"] is ref_w and kw["iters"] == 6 and kw["mode"] == mode
    assert C.degeneracy_args(mode + "_own_w")[3]["ref_w"] is None
    on_2 = (p.bl_ant0 == 2) | (p.bl_ant1 == 2)
    assert not np.any(ref_w[:, 4]) and not np.any(ref_w[on_2]) and on_2.sum() == 6
    others = np.delete(np.arange(72), 4)
    assert np.all(np.count_nonzero(ref_w[~on_2][:, others], axis=0) > 0)
    for dtype in DTYPES:
        out = C.restatement("fix_degeneracies", mode, dtype)
        assert out["nsamples"][4] == 0 and out["eta"][4] == 0 and out["psi"][4] == 0 and not out["tilt"][4].any()
        assert np.all(out["nsamples"][others] > 0) and np.all(out["nsamples"][others] <= 15)  # antenna 2's six rows never count
        assert out["last_step"].max() < 1e-3  # the iteration settled


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", C.WEIGHT_READERS, ids=READER_IDS)
def test_every_robust_case_meets_the_weights_matter_precondition(case, dtype):
    kind = case[0]
    tol = TOL[np.dtype(dtype)]
    w, w0, frac = C.clipped_weights(*case, dtype)
    moved, loss, new, old = C.margins(*case, dtype, w)
    label = f"{C.case_id(case)} {np.dtype(dtype).name}"
    print(f"{label}: {100 * frac:.1f} % of the good samples clipped; the restatement moves by " + "  ".join(f"{k} {v:.1e}" for k, v in moved.items())
          + f"  chi-square {loss:.1e}")
    assert 0.05 <= frac <= 0.30, (label, frac)
    assert np.all((w == w0) | (w == 0)) and not np.any(w[w0 == 0])
    below = C.below_margin(case, dtype)
    assert set(below) <= set(moved), label
    for k, v in moved.items():
        if k in below:
            assert v < 100 * tol["plane"], (label, k, v)  # (the entry is needed: else take it out of BELOW_MARGIN_FP32)
        else:
            assert v > 100 * tol["plane"], (label, k, v)
    assert loss > 100 * tol["loss"], (label, loss)
    if np.dtype(dtype) == np.dtype(np.float64):
        assert not below and all(v > 100 * tol["plane"] for v in moved.values())
    counts = C.sample_counts(kind, new)
    if counts is not None:
        assert np.any(counts != C.sample_counts(kind, old)), label
    if "conds" in new:
        print(f"{label}: largest cond(N) under the clipped weights {max(new['conds']):.3e}")
        assert max(new["conds"]) <= COND_MAX and new["singular"] == old["singular"]


def test_the_margin_table_names_cases_of_the_table():
    assert set(C.BELOW_MARGIN_FP32) <= set(C.WEIGHT_READERS)
    for case, keys in C.BELOW_MARGIN_FP32.items():
        assert set(keys) <= set(C.MATTER_PLANES[case[0]])
    assert [c for c in C.CASES if c not in C.WEIGHT_READERS] == C.GIVEN_REF_W == [("fix_degeneracies", "channel"), ("fix_degeneracies", "band")]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant", ["raw", "calibrated"])
def test_the_cross_pairs_keep_two_dead_pairs_and_a_common_mask_of_their_own(variant, dtype):
    """``norm_pair == 0`` for the two pairs that touch the wholly flagged row 1 and for no other, under ``w0`` and under the clipped
    weights; some pair's common mask is neither row's own (a reader that took one side's mask for both would differ there)."""
    case = ("delay_cross", variant)
    pairs = C.cross_pairs(*case)[0]
    w, w0, _ = C.clipped_weights(*case, dtype)
    assert not np.any(w0[1]) and np.all(np.count_nonzero(np.delete(w0, 1, axis=0), axis=1) > 0)
    touches = np.flatnonzero((pairs == 1).any(axis=1))
    assert len(touches) == 2
    for weights, ref in ((w0, C.reference(*case, np.dtype(dtype).name)), (w, C.restatement(*case, dtype, C.with_weights(C.inputs(*case)[0], w)))):
        np.testing.assert_array_equal(np.flatnonzero(ref["norm_pair"] == 0), touches)
        m0, m1 = weights[pairs[:, 0]] != 0, weights[pairs[:, 1]] != 0
        common = m0 & m1
        own = np.any(common != m0, axis=1) & np.any(common != m1, axis=1)
        print(f"{C.case_id(case)} {np.dtype(dtype).name}: {own.sum()} of {len(pairs)} pairs have a common mask that is neither row's own")
        assert own.any()
