"""GPU tests of the mixed-component kernels (csrc/mixed_comps_kernels.hpp) where they branch, at their edges and past 256 columns,
beside test_gpu_mixed_comps.py, which holds the device route to the host route through its end products.

**The factor, by pivot replay.**  Near-ties make the pivot order rounding-dependent, so no pivot list is compared with the
restatement's.  The DEVICE's pivot list is replayed in the kernel's order of operations in float64 and in longdouble
(mixed_comps_ref.replay); the columns of C are the device's dense matrix where n <= 3072 (it shares ``mixed_cov_elem`` with the step
kernel and is held here to the 64 eps max(1, max |x|) of ``test_dense_covariance``), else the host formula (``cov_column``).  With
``dn = max(64 eps, max |d_64 - d_ld|)``, the reference's own noise on that list: every pivot is the argmax of the replayed diagonal
within 8 dn and the first is row 0; the stop is where the diagonal falls below tol (within 8 dn), ``max_d`` is that diagonal; every
column of ``L`` is within 8 max(64 eps, max |L_64 - L_ld|) of the longdouble one (the 8: the device's subtraction loop is contracted
to FMAs, the replay's is not); ``G = L^T L`` within 16 n eps max |G|.  Cases and what each reaches: mixed_comps_cases.REPLAY
(test_mixed_comps_host.py asserts on the CPU that each still reaches it).

**The certificate, sharply**, on five cases whose residual is O(1) and not rounding noise: ``resid_fro`` against ``||C_host - L_dev
L_dev^T||_F`` of the downloaded factor within ``16 |r_64 - r_ld| + ||C_dev - C_host||_F``.

**The back-multiplication against a product**: ``cal_mixed_comps_vectors`` with a synthetic ``U`` and ``scale`` against ``L_dev (U
diag(scale))`` in longdouble within the dot-product bound, the groups' offsets with groups that keep nothing, a non-finite neighbour,
float32, refusals.

Measured on one MI355X with the kernels as they are (no tolerance had to exceed what is named above):
  worst ``|L_dev - L_ld|`` over the column's noise, per case (the factor 8 is the bound): one_by_1024_long 1.14 (column 304; the noise
  grows to 1.2e-9), two_by_512_capped 0.11 (noise 64 eps throughout), one_by_16640 2.39 (column 29; the only case whose columns are the
  host's sin(pi x), not the device's sinpi(x)), dup3_by_200 0.97, cap_equals_rank 1.28, edge_1 0, edge_2 0.006, edge_64 1.39, edge_65
  1.07, edge_256 1.43, edge_257 1.51;
  a pivot short of the replayed argmax: 0.04 dn at the most (one_by_16640), 0 elsewhere; ``|max_d - replayed|`` <= 0.06 dn;
  the certificate, ``|resid_fro - r_ld|`` against its tolerance, both relative to the residual: three_by_37 offset 6.6e-18 / 4.2e-15,
  min_dly 2.1e-17 / 4.4e-15, golomb8_offset 2.7e-16 / 1.2e-15, golomb8_antdly capped 9.9e-14 / 1.0e-12, two_by_512_capped 9.1e-17 /
  2.5e-15 -- eleven orders and more below the 29 % of a lost doubling;
  the back-multiplication: at most 0.052 of its elementwise bound.
Shown once on scratch copies of the library, the whole file against each: row p staged in one trip only fails 5 tests (both k > 256
cases stop at another rank); the partials reduced over the first 64 blocks only, 1 (one_by_16640: row 16639 is never a pivot); the
certificate without its doubling, and with tile (1, 0) skipped, the 5 cases of ``test_certificate_sharply`` each; ``mx_better``
preferring the higher row, 15 (ten replay cases at ``pivots[0] == 0``, the tie test, four certificate cases); the back-multiplication
without ``j < k``, the non-finite-neighbour test.  test_gpu_mixed_comps.py notices only the fifth of these, in 2 of its 36 tests.  Not
catchable by a value: the back-multiplication staging without ``c0 + c < r`` -- what it then stages for the columns c >= r feeds only
columns of the tile product that ``cc < r`` keeps from being stored; the mask guards the reads of U and scale behind their ends, and a
test of that would have to provoke a fault.  40 tests in 7.8 s.
"""
import ctypes
import concurrent.futures
import functools

import numpy as np
import pytest

import mixed_comps_cases as K
from calamity_amd import _lib, simple_cov
from calamity_amd.utils import usable_cores
from test_gpu_mixed_comps import same_bits, sinc_arguments

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
LD = np.longdouble
DENSE_MAX = 3072  # up to here the replay's columns are the device's dense matrix


@functools.lru_cache(maxsize=None)
def device(name, scratch_bytes=None):
    """The raw device route on one REPLAY (or VALID / INDEFINITE) case alone, with its factor: (vectors, info)."""
    (blvecs, freqs, params), bound = find(name), K.REPLAY[name][3] if name in K.REPLAY else 0
    bound = bound if scratch_bytes is None else scratch_bytes
    vectors, infos, _ = simple_cov.device_model_comps([blvecs], freqs, eigenval_cutoff=K.CUTOFF, device=0, return_factors=True, scratch_bytes=bound,
                                                      **params)
    return vectors[0], infos[0]


def find(name):
    return K.REPLAY[name][:3] if name in K.REPLAY else K.case(name)


def dense_pair(blvecs, freqs, params):
    """(C_device, C_host), the device's held to ``test_dense_covariance``'s bound."""
    host = simple_cov.simple_cov_matrix(blvecs, freqs, **params)
    dev = simple_cov.simple_cov_matrix(blvecs, freqs, device=0, **params)
    assert np.max(np.abs(dev - host)) <= 64 * EPS * max(1.0, sinc_arguments(blvecs, freqs, **params))
    assert np.array_equal(dev, dev.T) and np.all(np.diag(dev) == 1.0)
    return dev, host


def columns_of(name):
    blvecs, freqs, params, _ = K.REPLAY[name]
    if len(blvecs) * len(freqs) <= DENSE_MAX:
        return K.R.as_columns(dense_pair(blvecs, freqs, params)[0])
    return K.replay_columns(name)


def noise(a, b):
    return max(64 * EPS, float(np.max(np.abs(a - b))))


def check_replay(name, info, columns):
    """The replay assertions of the module's docstring on one device factor; returns the worst ratios (L, pivot, max_d)."""
    n, k, piv, L = info["n"], info["k"], info["pivots"], info["L"]
    assert L.shape == (n, k) and len(piv) == k >= 1 and piv[0] == 0 and len(set(piv.tolist())) == k and piv.min() >= 0 and piv.max() < n
    L64, d64 = K.R.replay(columns, piv, np.float64, n=n)
    Lld, dld = K.R.replay(columns, piv, LD, n=n)
    worst_p = 0.0
    for m, p in enumerate(piv):  # the pivot is the argmax
        dn = noise(d64[m], dld[m])
        worst_p = max(worst_p, float(dld[m].max() - dld[m][p]) / dn)
        assert dld[m][p] >= dld[m].max() - 8 * dn, (name, m, p)
    dn = noise(d64[k], dld[k])
    left = float(dld[k].max())
    if info["status"] == "ok":  # the stop
        assert left < K.TOL + 8 * dn and float(dld[k - 1][piv[k - 1]]) >= K.TOL - 8 * noise(d64[k - 1], dld[k - 1])
    else:
        assert info["status"] == "rank cap" and left >= K.TOL - 8 * dn
    worst_d = abs(info["max_d"] - left) / dn
    assert abs(info["max_d"] - left) <= 8 * dn
    worst_l, at = 0.0, 0
    for m in range(k):  # L, column by column
        ref = noise(L64[:, m], Lld[:, m])
        err = float(np.max(np.abs(L[:, m] - Lld[:, m])))
        if err / ref > worst_l:
            worst_l, at = err / ref, m
        assert err <= 8 * ref, (name, m, err, ref)
    G = info["G"]
    assert np.max(np.abs(G - L.T @ L)) <= 16 * n * EPS * np.max(np.abs(G)) and np.array_equal(G, G.T)
    print(f"{name}: n {n} k {k} {info['status']} max_d {info['max_d']:.3e}; worst |L_dev - L_ld| / noise {worst_l:.3f} (column {at}, noise there "
          f"{noise(L64[:, at], Lld[:, at]):.2e}, largest noise {max(noise(L64[:, m], Lld[:, m]) for m in range(k)):.2e}); "
          f"pivot short of the argmax by {worst_p:.3f} dn; |max_d - replayed| {worst_d:.3f} dn")
    return worst_l, worst_p, worst_d


@pytest.mark.parametrize("name", list(K.REPLAY))
def test_factor_by_pivot_replay(name):
    """Every REPLAY case: the branch it is there for is reached on the device too (k, cap and status of REPLAY_TABLE, which the
    stopping margins >= 2 of test_mixed_comps_host.py make safe against rounding; dup3_by_200 is held to the one-baseline group
    below instead), then the replay assertions."""
    want = K.REPLAY_TABLE[name]
    _, info = device(name)
    assert info["n"] == want["n"] and info["status"] == ("ok", "rank cap")[want["status"]] and info["chunk"] == 0
    assert info["k"] == want["k"] and (want["has_pivot"] is None or want["has_pivot"] in info["pivots"])
    assert len(set((info["pivots"] // 256).tolist())) == want["pivot_blocks"]
    check_replay(name, info, columns_of(name))


def test_ties_go_to_the_lowest_row():
    """Three copies of the one-baseline group: every diagonal is tied three ways (rows i, i + 200, i + 400: other waves, and for
    i + 400 >= 256 another block; step 0 is a tie over all 600 rows), and the lowest row wins through the wave butterflies, the four
    waves and the partials: pivots, k and the first copy's rows of L are toeplitz200's alone to the bit, the other copies' rows equal
    the first's."""
    (_, dup), (_, one) = device("dup3_by_200"), device("toeplitz200")
    assert dup["k"] == one["k"] and np.array_equal(dup["pivots"], one["pivots"]) and dup["pivots"].max() < 200
    assert np.array_equal(dup["L"][:200], one["L"])
    assert np.array_equal(dup["L"][200:400], dup["L"][:200]) and np.array_equal(dup["L"][400:], dup["L"][:200])


def test_ok_in_the_launch_that_would_cap():
    """cap = 64 = the rank: the launch `step == cap` finds the diagonal below tol and records ok, not a rank cap; the device route
    accepts the group, and the same group under the default bound (cap 100) has every bit the same."""
    blvecs, freqs, params, bound = K.REPLAY["cap_equals_rank"]
    capped, free = device("cap_equals_rank"), device("cap_equals_rank", 0)
    assert K.rank_cap(300, bound) == 64 == capped[1]["k"] and K.rank_cap(300, 0) == 100
    assert capped[1]["status"] == "ok" and capped[1]["route"] == "device" and capped[1]["reason"] is None and capped[1]["chunk"] == 0
    assert capped[0] is not None and same_bits(capped, free) and capped[1]["max_d"] == free[1]["max_d"]


def test_one_sample():
    vectors, info = device("edge_1")
    assert np.array_equal(vectors, [[1.0]]) and np.array_equal(info["G"], [[1.0]]) and np.array_equal(info["L"], [[1.0]])
    assert info["resid_fro"] == 0.0 and info["max_d"] == 0.0 and info["kept"] == 1


@pytest.mark.parametrize("name, bound, k", [("two_by_512_capped", None, 342), ("golomb8_antdly", 512 << 10, 32)])
def test_a_capped_group_reports_its_factor_and_no_vectors(name, bound, k):
    """The raw device route on a group at its rank cap: no vectors, but L, G and the certificate of the columns it has."""
    vectors, info = device(name, bound)
    assert vectors is None and info["route"] == "host" and info["reason"] == "rank cap" and info["status"] == "rank cap"
    assert info["k"] == k and info["L"].shape == (info["n"], k) and info["kept"] == 0 and info["max_d"] >= K.TOL
    L, G = info["L"], info["G"]
    assert np.max(np.abs(G - L.T @ L)) <= 16 * info["n"] * EPS * np.max(np.abs(G)) and np.array_equal(G, G.T)
    blvecs, freqs, params = find(name)
    resid = np.linalg.norm(simple_cov.simple_cov_matrix(blvecs, freqs, **params) - L @ L.T)
    print(f"{name}: k {k} resid_fro {info['resid_fro']:.6e} recomputed {resid:.6e}")
    assert resid > 1e-3 and info["resid_fro"] <= 2 * resid and resid <= 2 * info["resid_fro"]  # (sharply: test_certificate_sharply)


def lower_triangle_resid(blvecs, freqs, params, L, rows=260):
    """``||C - L L^T||_F`` over the whole matrix from its lower triangle in row blocks (C from ``cov_column``'s formula, one row
    block at a time on the usable cores), a block below the diagonal counting twice."""
    n = len(L)
    uvws = np.asarray(blvecs, dtype=np.float64).reshape(-1, 3)
    pts = (uvws[:, None, :] * (freqs[None, :, None] / 3e8)).reshape(-1, 3)
    fvals = np.tile(freqs, len(uvws))
    ant_dly, horizon, offset, min_dly = (params.get(key, default) for key, default in (("ant_dly", 0.0), ("horizon", 1.0), ("offset", 0.0), ("min_dly", 0.0)))

    def block(i0):
        i1 = min(n, i0 + rows)
        sep = np.zeros((i1 - i0, i1))
        for axis in range(3):
            sep += np.abs(pts[i0:i1, None, axis] - pts[None, :i1, axis]) ** 2.0
        sep = np.sqrt(sep) * horizon
        dfg = np.abs(fvals[i0:i1, None] - fvals[None, :i1]) / 1e9
        sep += dfg * offset
        c = np.sinc(2 * np.maximum(min_dly * dfg, sep))
        if ant_dly != 0.0:  # (sinc(0) = 1 exactly: nothing to multiply by)
            c = c * np.sinc(2 * dfg * ant_dly)
        if i0 == 0:  # the shortcut against the yardstick, on a few columns
            for p in (0, 1, i1 - 1):
                assert np.array_equal(c[:, p], K.R.cov_column(blvecs, freqs, p, **params)[:i1])
        diff = (c - L[i0:i1] @ L[:i1].T) ** 2
        return 2.0 * float(np.sum(diff[:, :i0])) + float(np.sum(np.tril(diff[:, i0:]) * 2 - np.diag(np.diag(diff[:, i0:]))))

    with concurrent.futures.ThreadPoolExecutor(max_workers=max(1, usable_cores())) as pool:
        return float(np.sqrt(sum(pool.map(block, range(0, n, rows)))))


def test_certificate_over_33930_tiles():
    """n = 16 640: 260 x 261 / 2 tiles.  The residual is rounding noise here (5e-11), so the factor 2 of ``test_factor_invariants``."""
    blvecs, freqs, params, _ = K.REPLAY["one_by_16640"]
    _, info = device("one_by_16640")
    n = info["n"]
    assert (n // 64) * (n // 64 + 1) // 2 == 33930
    resid = lower_triangle_resid(blvecs, freqs, params, info["L"])
    print(f"one_by_16640: resid_fro {info['resid_fro']:.3e} recomputed {resid:.3e}")
    assert info["resid_fro"] <= 2 * resid + n * 1e-15 and resid <= 2 * info["resid_fro"] + n * 1e-15


CERTIFICATE = {  # name -> (case, parameters, scratch bound, k and residual of the restatement)
    "three_by_37_offset": ("three_by_37", dict(offset=20.0), 0, 28, 1.886),
    "three_by_37_mindly": ("three_by_37", dict(min_dly=200.0), 0, 51, 2.576),
    "golomb8_offset": ("golomb8_offset", None, 0, None, 2.09e4),
    "golomb8_antdly_capped": ("golomb8_antdly", None, 512 << 10, 32, 0.0801),
    "two_by_512_capped": ("two_by_512_capped", None, 0, 342, None),
}


@pytest.mark.parametrize("name", list(CERTIFICATE))
def test_certificate_sharply(name):
    """Residuals that are O(1): ``resid_fro`` against the host's evaluation on the downloaded factor.  A lost doubling of the tiles
    below the diagonal, or one lost tile, moves the value by up to 29 %; the tolerance is the evaluation's own float64-to-longdouble
    discrepancy (16 times it) plus the measured ``||C_dev - C_host||_F``.  n = 111: partly filled tiles on both axes; n = 1600: 325
    tiles, more than one trip of the sum kernel."""
    case, params, bound, k, about = CERTIFICATE[name]
    blvecs, freqs, own = find(case)
    params = own if params is None else params
    _, infos, _ = simple_cov.device_model_comps([blvecs], freqs, eigenval_cutoff=K.CUTOFF, device=0, return_factors=True, scratch_bytes=bound, **params)
    info = infos[0]
    c_dev, c_host = dense_pair(blvecs, freqs, params)
    L = info["L"]
    r64 = float(np.linalg.norm(c_host - L @ L.T))
    r_ld = np.sqrt(np.sum((c_host.astype(LD) - L.astype(LD) @ L.T.astype(LD)) ** 2))
    tol = 16 * abs(float(r64 - r_ld)) + float(np.linalg.norm(c_dev - c_host))
    err = abs(float(info["resid_fro"] - r_ld))
    print(f"{name}: n {info['n']} k {info['k']} resid_fro {info['resid_fro']:.15e} host {r64:.15e}; |dev - r_ld| {err:.3e} = {err / r64:.2e} rel; "
          f"tolerance {tol:.3e} = {tol / r64:.2e} rel (|r_64 - r_ld| {abs(float(r64 - r_ld)):.2e}, ||C_dev - C_host||_F {float(np.linalg.norm(c_dev - c_host)):.2e})")
    assert info["reason"] in ("certificate", "rank cap") and (k is None or info["k"] == k) and (about is None or abs(r64 - about) <= 0.01 * about)
    assert err <= tol


# ---- the back-multiplication ----------------------------------------------------------------------------------------------------
class Factors:
    """A handle of cal_mixed_comps_create on several groups with their own bands, its ranks and downloaded factors."""

    def __init__(self, groups):
        self.lib = _lib.load()
        uvws = [np.ascontiguousarray(np.asarray(b, dtype=np.float64).reshape(-1, 3)) for b, _ in groups]
        bands = [np.ascontiguousarray(f, dtype=np.float64) for _, f in groups]
        ng = len(groups)
        starts, fstarts = np.zeros(ng + 1, dtype=np.int32), np.zeros(ng + 1, dtype=np.int32)
        starts[1:], fstarts[1:] = np.cumsum([len(u) for u in uvws]), np.cumsum([len(f) for f in bands])
        uvw, fr = np.concatenate(uvws), np.concatenate(bands)
        desc = _lib.MixedCompsDesc(ngroups=ng, nfreqs=len(fr), grp_bl_start=starts.ctypes.data, uvw=uvw.ctypes.data, freqs=fr.ctypes.data,
                                   grp_freq_start=fstarts.ctypes.data, ant_dly=0.0, horizon=1.0, offset=0.0, min_dly=0.0, tol=K.TOL, scratch_bytes=0)
        self.handle = ctypes.c_void_p()
        _lib.check(self.lib.cal_mixed_comps_create(ctypes.byref(self.handle), 0, ctypes.byref(desc)))
        rank, status = np.zeros(ng, dtype=np.int32), np.ones(ng, dtype=np.int32)
        _lib.check(self.lib.cal_mixed_comps_info(self.handle, rank.ctypes.data, status.ctypes.data, None, None, None, None))
        assert np.all(status == 0)
        self.n = [len(u) * len(f) for u, f in zip(uvws, bands)]
        self.k = [int(x) for x in rank]
        self.L = []
        for g in range(ng):
            fac = np.zeros((self.k[g], self.n[g]))
            _lib.check(self.lib.cal_mixed_comps_factor(self.handle, g, fac.ctypes.data, None))
            self.L.append(fac.T.copy())

    def close(self):
        _lib.check(self.lib.cal_mixed_comps_destroy(self.handle))

    def operands(self, g, r):
        """The synthetic U [k, r] (standard normal) and scale [r] (uniform in [0.5, 2]) of group g keeping r: seeded by (g, r)."""
        rng = np.random.default_rng([7, g, r])
        return rng.standard_normal((self.k[g], r)), rng.uniform(0.5, 2.0, r)

    def vectors(self, nkeep, dtype=np.float64, operands=None):
        """cal_mixed_comps_vectors with every group's synthetic operands (or ``operands[g]``): the list of V [n, r] per group."""
        ops = [(operands or {}).get(g) or self.operands(g, r) for g, r in enumerate(nkeep)]
        uall = np.ascontiguousarray(np.concatenate([u.ravel() for u, _ in ops] + [np.zeros(1)]))
        sall = np.ascontiguousarray(np.concatenate([s for _, s in ops] + [np.zeros(1)]))
        sizes = [n * max(r, 0) for n, r in zip(self.n, nkeep)]
        vall = np.full(max(1, sum(sizes)), np.nan, dtype=dtype)
        nk = np.asarray(nkeep, dtype=np.int32)
        _lib.check(self.lib.cal_mixed_comps_vectors(self.handle, _lib.CAL_F32 if dtype == np.float32 else _lib.CAL_F64, nk.ctypes.data, uall.ctypes.data,
                                                    sall.ctypes.data, vall.ctypes.data, None))
        off = np.concatenate([[0], np.cumsum(sizes)])
        return [vall[off[g] : off[g + 1]].reshape(self.n[g], max(nkeep[g], 0)) for g in range(len(nkeep))]


@pytest.fixture(scope="module")
def factors():
    """three_by_37 (n = 111: a partly filled row tile), one_by_1024_long (k = 307: 320 padded columns, 20 steps of the tile product)
    and three_by_5 (n = 15) in one create call."""
    groups = [K.case("three_by_37")[:2], K.REPLAY["one_by_1024_long"][:2], K.case("three_by_5")[:2]]
    f = Factors(groups)
    yield f
    f.close()


def test_back_multiplication_factors_are_the_single_groups(factors):
    """The handle's factors are those the cases have alone (so what is proven on them is proven on the factor of the replay test)."""
    assert factors.n == [111, 1024, 15] and factors.k[1] == 307 and factors.k[0] == device("three_by_37")[1]["k"]
    assert np.array_equal(factors.L[1], device("one_by_1024_long")[1]["L"]) and np.array_equal(factors.L[0], device("three_by_37")[1]["L"])


@pytest.mark.parametrize("g, r", [(1, r) for r in (1, 15, 16, 17, 63, 64, 65, "k")] + [(0, r) for r in (1, 15, 16, 17, "k")])
def test_back_multiplication_is_the_product(factors, g, r):
    """One group keeps r vectors, the others none: every element of V against ``L_dev (U diag(scale))`` in longdouble within the
    dot-product bound ``2 kpad eps (|L| |U diag(scale)|)`` (one rounding of ``u scale``, kpad fused multiply-adds).  r on both sides
    of 16 (a column quarter of the tile) and 64 (a tile), and k: 5 column tiles, the last with 51 of 64 columns."""
    r = factors.k[g] if r == "k" else r
    nkeep = [0, 0, 0]
    nkeep[g] = r
    V = factors.vectors(nkeep)[g]
    U, scale = factors.operands(g, r)
    L, kpad = factors.L[g], (factors.k[g] + 15) // 16 * 16
    B = U.astype(LD) * scale.astype(LD)
    err = np.abs(V.astype(LD) - L.astype(LD) @ B)
    bound = 2 * kpad * EPS * (np.abs(L).astype(LD) @ np.abs(B))
    print(f"group {g} r {r}: max |V - L U s| / bound {float(np.max(err / np.maximum(bound, 1e-300))):.3e}, max |V| {np.max(np.abs(V)):.3e}")
    assert V.shape == (factors.n[g], r) and np.all(np.isfinite(V)) and np.all(err <= bound)


@pytest.mark.parametrize("pick", [(0, 17, "k"), ("k", 0, 1)])
def test_back_multiplication_offsets(factors, pick):
    """Three groups of which one keeps nothing (first, then in the middle): every group's block of V has the bits of a call in which
    it is the only one that keeps any."""
    nkeep = [factors.k[g] if r == "k" else r for g, r in enumerate(pick)]
    together = factors.vectors(nkeep)
    for g, r in enumerate(nkeep):
        alone = [0, 0, 0]
        alone[g] = r
        assert together[g].shape == (factors.n[g], r) and np.array_equal(together[g], factors.vectors(alone)[g]), g


def test_back_multiplication_ignores_what_lies_behind_its_operands(factors):
    """The zero columns [k, kpad) of L meet rows of U that do not exist: what lies there in the buffer is the next group's U.  Made
    NaN, it must not reach this group's V (0 x NaN is NaN: the mask ``j < k`` has to hold), which keeps the bits it has alone; the
    group whose U is NaN gets NaN."""
    nkeep = [17, 17, factors.k[2]]  # (k = 307: 13 such rows of 17 in the middle group, fewer than the last group's U holds)
    assert 13 * 17 <= factors.k[2] ** 2
    nan_ops = (np.full((factors.k[2], factors.k[2]), np.nan), np.ones(factors.k[2]))
    together = factors.vectors(nkeep, operands={2: nan_ops})
    for g in (0, 1):
        alone = [0, 0, 0]
        alone[g] = 17
        assert np.array_equal(together[g], factors.vectors(alone)[g]), g
    assert np.all(np.isnan(together[2]))


def test_back_multiplication_in_float32_and_refusals(factors):
    nkeep = [17, factors.k[1], 1]
    v64, v32 = factors.vectors(nkeep), factors.vectors(nkeep, dtype=np.float32)
    for a, b in zip(v64, v32):
        assert b.dtype == np.float32 and np.array_equal(a.astype(np.float32), b)
    for g in range(3):
        for bad in (factors.k[g] + 1, -1):
            nkeep = [1, 1, 1]
            nkeep[g] = bad
            with pytest.raises(_lib.CalamityHipError):
                factors.vectors(nkeep, operands={g: (np.zeros((factors.k[g], factors.k[g] + 1)), np.zeros(factors.k[g] + 1))})
