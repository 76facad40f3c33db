"""The fitting groups the mixed-model component tests share (test_mixed_comps_host.py, test_gpu_mixed_comps.py,
test_gpu_mixed_comps_replay.py), each computed once: the restatement of mixed_comps_ref.py and the host route's eigenpairs are cached
per case and never modified."""
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


TOL = 1e-13  # simple_cov.factor_tol(CUTOFF)


def ramp(n, step):
    return 100e6 + step * np.arange(n)


def one_bl(length):
    return np.array([[length, 0.0, 0.0]])


# The cases of test_gpu_mixed_comps_replay.py, each chosen for a branch of mixed_comps_kernels.hpp that VALID / INDEFINITE do not
# reach: name -> (blvecs, freqs, parameters, scratch_bytes; 0 is the default bound).  REPLAY_TABLE holds what the restatement gives on
# each (test_mixed_comps_host.py asserts every figure without a GPU, so a case cannot quietly stop reaching its branch).
REPLAY = {
    # k past 256: the second trip of the step kernel's staging of row p; back-multiplication and Gram past 256 columns
    "one_by_1024_long": (one_bl(420.0), ramp(1024, 1e5), dict(), 0),
    # the rank cap past 256 (the launch `step == cap`), well conditioned
    "two_by_512_capped": (np.array([[380.0, 0.0, 0.0], [400.0, 10.0, 0.0]]), ramp(512, 2e5), dict(), 0),
    # 65 blocks of 256 rows: the second trip of the partial reduction; a certificate of 33 930 tiles (32 MiB: the cap cut to 240
    # keeps the scratch memset small)
    "one_by_16640": (one_bl(100.0), ramp(16640, 2e3), dict(), 32 << 20),
    # three copies of one baseline: every step is a three-way tie across waves and blocks, the lowest row must win
    "dup3_by_200": (np.array([[2.0, 0.0, 0.0]] * 3), FREQS_GOLOMB, dict(offset=20.0), 0),
    # a group that finishes ok in the very launch that would cap it (cap 64 = rank)
    "cap_equals_rank": (one_bl(240.0), ramp(300, 1e5), dict(), 180000),
    # the smallest sizes, the tile / pitch edge at 64 and a block of the step kernel with one live row at 257
    "edge_1": (one_bl(60.0), ramp(1, 1e6), dict(), 0),
    "edge_2": (one_bl(60.0), ramp(2, 1e6), dict(), 0),
    "edge_64": (one_bl(60.0), ramp(64, 1e6), dict(), 0),
    "edge_65": (one_bl(60.0), ramp(65, 1e6), dict(), 0),
    # (2.5e5 Hz: both stopping margins >= 2 at either size; 2e5 Hz leaves the last pivot at d = 1.01e-13)
    "edge_256": (one_bl(60.0), ramp(256, 2.5e5), dict(), 0),
    "edge_257": (one_bl(60.0), ramp(257, 2.5e5), dict(), 0),
}
# name -> n, cap, k, status (0 ok, 1 rank cap), the number of 256-row blocks that hold a pivot, the block of the last pivot, and a
# row that must be among the pivots (None: no such demand)
REPLAY_TABLE = {
    "one_by_1024_long": dict(n=1024, cap=342, k=307, status=0, pivot_blocks=4, last_block=1, has_pivot=None),
    "two_by_512_capped": dict(n=1024, cap=342, k=342, status=1, pivot_blocks=4, last_block=1, has_pivot=None),
    "one_by_16640": dict(n=16640, cap=240, k=36, status=0, pivot_blocks=33, last_block=13, has_pivot=16639),
    "dup3_by_200": dict(n=600, cap=200, k=8, status=0, pivot_blocks=1, last_block=0, has_pivot=None),
    "cap_equals_rank": dict(n=300, cap=64, k=64, status=0, pivot_blocks=2, last_block=0, has_pivot=None),
    "edge_1": dict(n=1, cap=1, k=1, status=0, pivot_blocks=1, last_block=0, has_pivot=0),
    "edge_2": dict(n=2, cap=2, k=2, status=0, pivot_blocks=1, last_block=0, has_pivot=1),
    "edge_64": dict(n=64, cap=64, k=39, status=0, pivot_blocks=1, last_block=0, has_pivot=63),
    "edge_65": dict(n=65, cap=64, k=39, status=0, pivot_blocks=1, last_block=0, has_pivot=64),
    "edge_256": dict(n=256, cap=86, k=40, status=0, pivot_blocks=1, last_block=0, has_pivot=255),
    "edge_257": dict(n=257, cap=86, k=40, status=0, pivot_blocks=2, last_block=0, has_pivot=256),
}


def rank_cap(n, scratch_bytes=0):
    """The rank cap of a group of n samples under a scratch bound (include/calamity_hip.h, cal_mixed_comps_create): a third of its
    order, at least 64, at most n and 6144; where that does not fit the bound, the columns the bound holds, in sixteens."""
    bound = scratch_bytes or 256 << 20
    ldl, nblk = (n + 63) // 64 * 64, (n + 255) // 256

    def group_bytes(cap):
        return ldl * ((cap + 15) // 16 * 16) * 8 + ldl * 8 + 2 * nblk * 16 + cap * 4

    cap = min(n, 6144, max(64, (n + 2) // 3))
    if group_bytes(cap) > bound:
        cols = (bound - group_bytes(0)) // (ldl * 8 + 4) if bound > group_bytes(0) else 0
        cap = min(cap, cols // 16 * 16)
    return cap


def replay_columns(name):
    """``columns(p)`` of a REPLAY case on the host, from the formula (mixed_comps_ref.cov_column)."""
    blvecs, freqs, params, _ = REPLAY[name]
    return lambda p: R.cov_column(blvecs, freqs, p, **params)


@functools.lru_cache(maxsize=None)
def replay_restatement(name):
    """The pivoted factor of a REPLAY case as the restatement computes it, column by column (no dense matrix: n = 16 640)."""
    blvecs, freqs, _, scratch = REPLAY[name]
    n = len(blvecs) * len(freqs)
    return R.pivoted_cholesky_columns(replay_columns(name), n, TOL, rank_cap(n, scratch))


def span_defect(V, vecs):
    """``||v - V V^T v||`` for every column v of ``vecs``."""
    return np.linalg.norm(vecs - V @ (V.T @ vecs), axis=0)
