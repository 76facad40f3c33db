"""The fitting groups the mixed-model component tests share (test_mixed_comps_host.py, test_gpu_mixed_comps.py), each computed once:
the restatement of mixed_comps_ref.py and the host route's eigenpairs are cached per case and never modified."""
import functools

import numpy as np

import mixed_comps_ref as R

FREQS_GOLOMB = 100e6 + 100e3 * np.arange(200)  # the band of tests/test_mixed_modeling.py:golomb6
BLS8 = np.array([[12.0 + 2.0 * i, 0.0, 0.0] for i in range(8)])  # its fitting group of eight redundant groups ((2, 3) ... (2, 5))
BLS2 = np.array([[32.0, 0.0, 0.0], [34.0, 0.0, 0.0]])  # its pair ((1, 5), (0, 5))
BLS3 = np.array([[14.6, 0.0, 0.0], [21.9, 2.0, 0.0], [29.2, 4.0, 0.0]])
BLS6 = np.array([[14.6 * (1.0 + 0.5 * i), 2.0 * (i % 3), 0.0] for i in range(6)])

# name -> (blvecs, freqs, parameters of simple_cov_matrix): positive semi-definite covariances, the device route is valid
VALID = {
    "golomb8_antdly": (BLS8, FREQS_GOLOMB, dict(ant_dly=2.0 / 0.3)),
    "golomb8_plain": (BLS8, FREQS_GOLOMB, dict()),
    "golomb8_horizon": (BLS8, FREQS_GOLOMB, dict(horizon=0.8)),
    "golomb2": (BLS2, FREQS_GOLOMB, dict(ant_dly=2.0 / 0.3)),
    "three_by_37": (BLS3, 100e6 + 1e6 * np.arange(37), dict()),
    "three_by_5": (BLS3, 100e6 + 1e6 * np.arange(5), dict()),
    "toeplitz200": (np.array([[2.0, 0.0, 0.0]]), FREQS_GOLOMB, dict(offset=20.0)),
    "six_by_512": (BLS6, 100e6 + 200e3 * np.arange(512), dict()),  # rank past 128 (n = 3072)
}
# indefinite covariances: the certificate must reject them
INDEFINITE = {
    "golomb8_offset": (BLS8, FREQS_GOLOMB, dict(offset=20.0)),
    "golomb8_mindly": (BLS8, FREQS_GOLOMB, dict(min_dly=200.0)),
    "golomb8_both": (BLS8, FREQS_GOLOMB, dict(offset=20.0, min_dly=200.0, horizon=0.8)),
}
CUTOFF = 1e-10


def case(name):
    return (VALID.get(name) or INDEFINITE[name])


@functools.lru_cache(maxsize=None)
def restatement(name):
    blvecs, freqs, params = case(name)
    return R.model_comps(blvecs, freqs, eigenval_cutoff=CUTOFF, **params)


@functools.lru_cache(maxsize=None)
def host(name):
    """(eigenvalues strongest first, kept count, kept vectors) of the host route."""
    return R.host_eig(restatement(name)["cmat"], CUTOFF)


def span_defect(V, vecs):
    """``||v - V V^T v||`` for every column v of ``vecs``."""
    return np.linalg.norm(vecs - V @ (V.T @ vecs), axis=0)
