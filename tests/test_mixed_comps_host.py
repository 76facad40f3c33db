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
