"""CPU tests of the mixed-model components' device route as restated in mixed_comps_ref.py: the restatement against
``numpy.linalg.eigh`` of the dense covariance, the certificate on indefinite covariances, and what the public functions do about
``device`` / ``use_tensorflow`` without a device."""
import ctypes

import numpy as np
import pytest

import mixed_comps_cases as K
from calamity_amd import _lib, calibration, modeling, simple_cov

EPS = np.finfo(np.float64).eps
SMALL = [n for n in K.VALID if n != "six_by_512"]  # (the n = 3072 group costs a 1.4 s eigh: the GPU tests pay for it once)


@pytest.mark.parametrize("name", SMALL)
def test_restatement_matches_dense_eigh(name):
    """Eigenvalues to Weyl's bound, the same kept count, the well-separated host eigenvectors inside the span, orthonormal vectors.
    Bounds: |lambda' - lambda| <= ||C - L L^T||_2 <= resid_fro (Weyl) plus LAPACK's n eps lambda_max on either side; for a host
    eigenvector v of eigenvalue lambda >= 100 tau, tau = cutoff lambda_max, the part of v outside the span of the kept vectors
    of L L^T obeys (lambda - tau) ||P v|| <= ||(C - L L^T) v||, so ||P v|| <= (resid_fro + 10 n eps lambda_max) / (lambda - tau)
    with the same allowance for the two eigensolvers; V^T V - I = Lambda^-1/2 U^T dG U Lambda^-1/2 for the rounding dG of L^T L and
    of its eigensolver, |dG| <= n eps lambda_max, against kept eigenvalues >= cutoff lambda_max: n eps / cutoff."""
    ref, (evals, kept, vecs) = K.restatement(name), K.host(name)
    n, lam = len(ref["cmat"]), evals[0]
    assert ref["reason"] is None and ref["status"] == 0 and ref["max_d"] < 1e-13
    assert len(set(ref["pivots"].tolist())) == ref["k"]
    assert np.min(np.abs(evals / lam - K.CUTOFF)) > 0.01 * K.CUTOFF  # no eigenvalue sits on the cut
    assert ref["kept"] == kept
    assert np.max(np.abs(ref["evals"] - evals[:kept])) <= ref["resid_fro"] + 10 * n * EPS * lam
    strong = evals[:kept] >= 100 * K.CUTOFF * lam
    defect = K.span_defect(ref["V"], vecs[:, strong])
    assert np.all(defect <= (ref["resid_fro"] + 10 * n * EPS * lam) / (evals[:kept][strong] - K.CUTOFF * lam))
    assert np.max(np.abs(ref["V"].T @ ref["V"] - np.eye(kept))) <= n * EPS / K.CUTOFF
    assert ref["resid_fro"] <= 0.1 * K.CUTOFF * lam


def test_toeplitz_case_is_the_closed_form():
    """One baseline with an offset: the sinc Toeplitz matrix of test_simple_cov_closed_form."""
    blvecs, freqs, params = K.case("toeplitz200")
    fg0, fg1 = np.meshgrid(freqs, freqs)
    assert np.allclose(K.restatement("toeplitz200")["cmat"], np.sinc(2 * (2.0 / 0.3 + 20.0) * (fg0 - fg1) / 1e9))


@pytest.mark.parametrize("name", list(K.INDEFINITE))
def test_certificate_rejects_indefinite_covariances(name):
    """offset or min_dly with several baselines: the pivoted factor stops early and the residual says so by orders of magnitude."""
    ref = K.restatement(name)
    assert ref["reason"] == "certificate" and ref["V"] is None
    assert ref["resid_fro"] >= 1e10 * 0.1 * K.CUTOFF * ref["lambda_max"]
    assert np.linalg.eigvalsh(ref["cmat"])[0] < -1e-3  # it really is indefinite


def test_rank_cap_is_a_status():
    blvecs, freqs, params = K.case("three_by_37")
    ref = K.restatement("three_by_37")
    capped = K.R.model_comps(blvecs, freqs, eigenval_cutoff=K.CUTOFF, cap=ref["k"] - 3, **params)
    assert capped["status"] == 1 and capped["reason"] == "rank cap" and capped["k"] == ref["k"] - 3 and capped["V"] is None


@pytest.mark.parametrize("params", [dict(), dict(offset=20.0), dict(horizon=0.8, offset=123.0, min_dly=200.0), dict(ant_dly=2.0 / 0.3, min_dly=50.0)])
def test_cov_column_is_the_column_of_the_dense_matrix(params):
    """``cov_column`` is the yardstick where the dense matrix is too large: every bit of the column, at n = 111 (three baselines off
    the axis) and 400, first, last and inner columns."""
    for name in ("three_by_37", "golomb2"):
        blvecs, freqs, _ = K.case(name)
        cmat = simple_cov.simple_cov_matrix(blvecs, freqs, **params)
        for p in (0, 1, len(freqs) - 1, len(freqs), len(cmat) // 2 + 3, len(cmat) - 1):
            col = K.R.cov_column(blvecs, freqs, p, **params)
            assert col.dtype == np.float64 and np.array_equal(col, cmat[:, p]), (name, p)


def test_columnwise_restatement_and_replay_are_the_restatement():
    """``pivoted_cholesky_columns`` has the bits of ``pivoted_cholesky`` (the same statements on the same columns), and ``replay`` of
    its pivots holds the restatement's own factor to what the GPU tests ask of the device's: every column within 8 times the replay's
    float64-to-longdouble noise of the longdouble replay (a BLAS product there, one column at a time here; the noise grows to 5.6e-10
    over the 46 columns), every pivot the argmax of the replayed diagonal, the stop below tol; the diagonal it returns is the one before
    every step and after the last, never negative, zero at the pivots taken."""
    blvecs, freqs, params = K.case("three_by_37")
    ref = K.restatement("three_by_37")
    cols = K.R.pivoted_cholesky_columns(lambda p: K.R.cov_column(blvecs, freqs, p, **params), len(ref["cmat"]), K.TOL)
    assert np.array_equal(cols["pivots"], ref["pivots"]) and np.array_equal(cols["L"], ref["L"]) and cols["max_d"] == ref["max_d"]
    assert cols["status"] == 0 and cols["k"] == ref["k"] and cols["last_d"] >= K.TOL
    L64, d64 = K.R.replay(ref["cmat"], ref["pivots"], np.float64)
    Lld, dld = K.R.replay(lambda p: ref["cmat"][:, p], ref["pivots"], np.longdouble, n=len(ref["cmat"]))
    assert L64.dtype == np.float64 and Lld.dtype == np.longdouble and d64.shape == (ref["k"] + 1, len(ref["cmat"]))
    assert np.all(d64[0] == 1.0) and np.all(d64 >= 0.0) and np.all(dld >= 0.0)
    for m, p in enumerate(ref["pivots"]):
        noise = max(64 * EPS, float(np.max(np.abs(L64[:, m] - Lld[:, m]))))
        assert np.max(np.abs(ref["L"][:, m] - Lld[:, m])) <= 8 * noise, m
        dn = max(64 * EPS, float(np.max(np.abs(d64[m] - dld[m]))))
        assert dld[m][p] >= dld[m].max() - 8 * dn and np.all(d64[m + 1][ref["pivots"][: m + 1]] == 0.0)
    dn = max(64 * EPS, float(np.max(np.abs(d64[-1] - dld[-1]))))
    assert abs(ref["max_d"] - float(dld[-1].max())) <= 8 * dn and float(dld[-1].max()) < K.TOL


@pytest.mark.parametrize("name", list(K.REPLAY))
def test_replay_cases_reach_their_branches(name):
    """Every figure of REPLAY_TABLE that a GPU test relies on, from the restatement: n, the rank cap of the scratch bound, k, the
    status, how many 256-row blocks hold a pivot, the block of the last pivot, the row that must be a pivot; and that the stop is no
    near-tie -- the last pivot's diagonal is >= 2 tol and the diagonal it stops on is <= tol / 2 (a capped case: >= 2 tol, it is 0.976)
    -- so the device's rank cannot differ from these for rounding.  dup3_by_200 stops on 6.7e-14, a margin of 1.5: its GPU test holds
    the device to the one-baseline group bit for bit, not to this k."""
    blvecs, freqs, _, scratch = K.REPLAY[name]
    want, ref = K.REPLAY_TABLE[name], K.replay_restatement(name)
    piv = ref["pivots"]
    assert len(blvecs) * len(freqs) == want["n"] and K.rank_cap(want["n"], scratch) == want["cap"]
    assert (ref["k"], ref["status"]) == (want["k"], want["status"]) and len(set(piv.tolist())) == ref["k"]
    assert len(set((piv // 256).tolist())) == want["pivot_blocks"] and piv[-1] // 256 == want["last_block"] and piv[0] == 0
    assert want["has_pivot"] is None or want["has_pivot"] in piv
    print(f"{name}: k {ref['k']} last pivot's d {ref['last_d']:.3e} stops on {ref['max_d']:.3e}")
    assert ref["last_d"] >= 2 * K.TOL
    if want["status"] == 0:
        assert ref["max_d"] <= K.TOL / (1.4 if name == "dup3_by_200" else 2)
    else:
        assert ref["k"] == want["cap"] and ref["max_d"] >= 2 * K.TOL


def test_replay_case_figures():
    """What the table's words say beyond its numbers."""
    assert K.TOL == simple_cov.factor_tol(K.CUTOFF)
    assert K.replay_restatement("one_by_1024_long")["k"] > 256 and K.replay_restatement("two_by_512_capped")["k"] > 256
    assert (16640 + 255) // 256 == 65  # more blocks than the 64 lanes of the partial reduction
    dup, one = K.replay_restatement("dup3_by_200"), K.R.pivoted_cholesky_columns(
        lambda p: K.R.cov_column(*K.case("toeplitz200")[:2], p, **K.case("toeplitz200")[2]), 200, K.TOL)
    assert dup["pivots"].max() < 200 and np.array_equal(dup["pivots"], one["pivots"])  # ties go to the first copy
    assert np.array_equal(dup["L"][:200], dup["L"][200:400]) and np.array_equal(dup["L"][:200], dup["L"][400:])
    assert np.array_equal(dup["L"][:200], one["L"])
    assert K.rank_cap(300) == 100 and K.rank_cap(1600, 512 << 10) == 32 and K.rank_cap(1600, 4 << 10) == 0  # (test_fallback_on_a_rank_cap)
    # the certificate's cases: n = 111 fills neither axis of its second tile, n = 1600 has more tiles than one trip of the sum kernel
    assert 111 % 64 != 0 and (1600 // 64) * (1600 // 64 + 1) // 2 == 325 > 256


@pytest.mark.parametrize("name, params, cap, k, resid", [("three_by_37", dict(offset=20.0), None, 28, 1.886), ("three_by_37", dict(min_dly=200.0), None, 51, 2.576),
                                                        ("golomb8_offset", None, None, 34, 2.09e4), ("golomb8_antdly", None, 32, 32, 0.0801)])
def test_sharp_certificate_cases_have_residuals_of_order_one(name, params, cap, k, resid):
    """The cases on which the GPU tests hold the certificate to rounding: their residual is no rounding noise (an indefinite
    covariance, or a factor stopped at 32 columns), so a tile counted once instead of twice, or not at all, shows."""
    blvecs, freqs, own = K.case(name)
    ref = K.R.model_comps(blvecs, freqs, eigenval_cutoff=K.CUTOFF, cap=cap, **(own if params is None else params))
    assert ref["k"] == k and abs(ref["resid_fro"] - resid) <= 1e-3 * resid and ref["reason"] == ("certificate" if cap is None else "rank cap")


def test_keep_and_accept():
    evals = np.array([1e-14, 1e-9, 1e-3, 2.0])
    keep, reason = simple_cov.keep_and_accept(evals, 0, 1e-12, 1e-10)
    assert reason is None and keep.tolist() == [3, 2, 1]
    assert simple_cov.keep_and_accept(evals, 0, 3e-11, 1e-10)[1] == "certificate"  # 0.1 cutoff lambda_max = 2e-11
    assert simple_cov.keep_and_accept(evals, 1, 0.0, 1e-10)[1] == "rank cap"
    assert simple_cov.keep_and_accept(evals, 2, 0.0, 1e-10)[1] == "not run"
    assert simple_cov.keep_and_accept(np.zeros(0), 0, 0.0, 1e-10)[1] == "certificate"
    assert simple_cov.factor_tol(1e-10) == 1e-13 and simple_cov.factor_tol(1e-6) == 1e-9


def test_device_keyword_checks():
    assert simple_cov.device_index(None) is None and simple_cov.device_index(None, use_tensorflow=True) == 0
    assert simple_cov.device_index(3, use_tensorflow=True) == 3 and simple_cov.device_index(np.int32(1)) == 1
    for bad in (-1, 1.0, "0", True):
        with pytest.raises(ValueError):
            simple_cov.device_index(bad)
    with pytest.raises(ValueError):
        modeling.yield_mixed_comps([], [], K.FREQS_GOLOMB, device=-2)
    assert calibration._modeling_comps_device(False, [2]) is None and calibration._modeling_comps_device(True, None) == 0
    assert calibration._modeling_comps_device(True, [2, 3]) == 2 and calibration._modeling_comps_device(True, "all") == 0


def test_default_route_is_the_host_to_the_bit():
    """Without the keywords nothing changes; return_info on the host route names the route."""
    blvecs, freqs, params = K.case("three_by_5")
    cmat = simple_cov.simple_cov_matrix(blvecs, freqs)
    evals, evecs = np.linalg.eigh(cmat)
    want = evecs[:, evals / evals[-1] >= 1e-10][:, ::-1]
    assert np.array_equal(simple_cov.yield_simple_multi_baseline_model_comps(blvecs, freqs), want)
    vecs, info = simple_cov.yield_simple_multi_baseline_model_comps(blvecs, freqs, return_info=True)
    assert np.array_equal(vecs, want) and info["route"] == "host" and info["n"] == 15
    grps = [[((0, 1),), ((0, 2),), ((0, 3),)], [((1, 2),)]]
    bls = [blvecs, np.array([[7.0, 0.0, 0.0]])]
    plain = modeling.yield_mixed_comps(grps, bls, freqs, grp_size_threshold=1)
    comps, info = modeling.yield_mixed_comps(grps, bls, freqs, grp_size_threshold=1, return_info=True)
    assert list(plain) == list(comps) and all(np.array_equal(plain[k], comps[k]) for k in plain)
    assert list(info) == [tuple(grps[0])] and info[tuple(grps[0])]["route"] == "host"


def test_device_route_fails_loudly_without_a_device():
    """No quiet fall-back to the host when the device is asked for and there is none."""
    n = ctypes.c_int(0)
    if _lib.load().cal_device_count(ctypes.byref(n)) == 0 and n.value > 0:
        pytest.skip("a GPU is present")
    blvecs, freqs, params = K.case("three_by_5")
    with pytest.raises(_lib.CalamityHipError):
        simple_cov.simple_cov_matrix(blvecs, freqs, device=0)
    with pytest.raises(_lib.CalamityHipError):
        simple_cov.yield_simple_multi_baseline_model_comps(blvecs, freqs, use_tensorflow=True)


def test_create_refuses_bad_descriptions():
    lib = _lib.load()
    starts, uvw, freqs = np.array([0, 1], dtype=np.int32), np.array([[2.0, 0.0, 0.0]]), np.array([1e8, 1.1e8])
    handle = ctypes.c_void_p()

    def desc(**kw):
        base = dict(ngroups=1, nfreqs=2, grp_bl_start=starts.ctypes.data, uvw=uvw.ctypes.data, freqs=freqs.ctypes.data, ant_dly=0.0, horizon=1.0,
                    offset=0.0, min_dly=0.0, tol=1e-13, scratch_bytes=0)
        base.update(kw)
        return _lib.MixedCompsDesc(**base)

    for kw in (dict(ngroups=0), dict(tol=0.0), dict(tol=np.nan), dict(scratch_bytes=-1), dict(horizon=np.inf), dict(uvw=None)):
        d = desc(**kw)
        assert lib.cal_mixed_comps_create(ctypes.byref(handle), 0, ctypes.byref(d)) == _lib.CAL_ERR_INVALID and handle.value is None
    assert lib.cal_mixed_comps_destroy(None) == _lib.CAL_ERR_INVALID and lib.cal_mixed_comps_info(None, None, None, None, None, None, None) == _lib.CAL_ERR_INVALID
