"""Shape coverage of cal_solver_solve_coeffs (coeff_solve_kernels.hpp) against the NumPy restatement of tests/test_gpu_coeff_solve.py:
every tile width of both precisions (fp32 FB 128/64/32/16/8, fp64 FB 64/32/16/8/4 follow from nvec) with nvec on both sides of every
boundary, blocks of up to 896 vectors (14 blocks of 64 rows of N, 105 work items per group, four trips of the Cholesky kernel's
256-strided loops), full and folded tiles, the factor on either side of its move from LDS to scratch, fitting groups whose baselines
alternate between row blocks (merged and interrupted walks of the Gram kernel), a band that is not a multiple of any tile width,
and the bits of two fresh solvers at size.

Every parity case asserts, before it touches the device, that the restatement's largest cond(N) is at most COND_MAX and which groups
are singular; then the result dict, the coefficient planes and the chi-square within the project's TOL (tests/test_gpu_fit_quality.py:
fp32 plane 1e-4, loss 1e-5; fp64 1e-10).  cond(N) is 6 ... 63 on these inputs, and an fp32 Gram emulated in NumPy with an fp64 solve
stays within 3.2e-6 of the restatement on them: the fp32 bound leaves a factor of 30 (the single-baseline groups of the narrow case
reach cond(N) = 1.0e3 and 1.6e-5: a factor of 6).  The wide blocks keep a band at least as long as the block is wide (896 vectors on
200 channels have cond(N) = 2e18).  Measured errors: DESIGN.md section 3.10."""
import functools

import numpy as np
import pytest

from calamity_amd.problem import FitProblem
from test_gpu_coeff_solve import COND_MAX, check_coeffs, check_loss, restated
from test_gpu_fit_quality import TOL, plane_err, solver_of
from test_gpu_fold import mirror_block, small_problem
from test_gpu_shapes import random_problem

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]


@functools.lru_cache(maxsize=None)
def reference(builder, dtype):
    """(problem, start, restated coefficients, restated chi-square, largest cond(N), singular groups): once per case and dtype."""
    p, start = builder()
    want, chisq, conds, singular = restated(p, start, dtype)
    want.setflags(write=False)
    return p, start, want, chisq, max(conds), singular


def solve_and_check(builder, dtype, label, layout="shared", path="auto", folded=None, scratch=None):
    """One solve of every group against the restatement; returns the planes after the call."""
    p, start, want, chisq, cond, singular = reference(builder, dtype)
    print(f"{label}: nvec {sorted({b.shape[1] for b in p.basis})}, largest cond(N) {cond:.2e}")
    assert cond <= COND_MAX and singular == []
    s = solver_of(p, start, dtype, layout, path)
    if folded is not None:
        got = s.timing_get()["basis_folded"]
        print(f"{label}: basis_folded {got}")
        assert got == folded, (label, got)
    if scratch is not None:
        s._set_coeff_solve_scratch(scratch)
    res = s.solve_coeffs()
    assert res == {"nsolved": p.ngrps, "nsingular": 0}, (label, res)
    planes = check_coeffs(s, want, dtype, label)
    check_loss(s, chisq, dtype, label)
    s.close()
    return planes


# ---- 1. wide blocks, full tiles, three row blocks per group; 6. the bits of two solvers
@functools.lru_cache(maxsize=None)
def wide_case():
    """17 ... 896 vectors on 1024 channels: fp32 FB 128, 32, 16, 16, 8, 8 and fp64 FB 64, 8, 8, 8, 4, 4; 1 ... 14 blocks of 64 rows (up to
    105 work items a group); every group but the first has three baselines on three row blocks, hence three walks and full tiles."""
    return random_problem([17, 113, 225, 300, 449, 896], [1, 3, 3, 3, 3, 3], nfreqs=1024, seed=4, rowblocks=True)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", ["stream", "shared"])
def test_wide_blocks_on_full_tiles_with_row_blocks(layout, dtype):
    solve_and_check(wide_case, dtype, f"wide {layout} {np.dtype(dtype).name}", layout=layout, folded=0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", ["stream", "shared"])
def test_two_fresh_solvers_give_the_same_bits_at_size(layout, dtype):
    """The kernels sum in a fixed order: 105 work items of one group and four trips of the trace reduction give the same bits twice."""
    p, start = wide_case()
    runs = []
    for _ in range(2):
        s = solver_of(p, start, dtype, layout)
        assert s.solve_coeffs() == {"nsolved": p.ngrps, "nsingular": 0}
        runs.append(s.get_params()[2:])
        s.close()
    for a, b in zip(*runs):
        np.testing.assert_array_equal(a, b)
    assert np.all(runs[0][0] != np.asarray(start["c_r"], dtype=dtype))


# ---- 2. wide blocks, folded tiles
@functools.lru_cache(maxsize=None)
def _folded_cases():
    rng = np.random.default_rng(7)
    out = {}
    for nfreqs, nvecs, seed in ((2048, (257, 450, 896), 8), (1024, (225, 300, 449), 9)):  # (the blocks are drawn in this order)
        out[nfreqs] = small_problem([mirror_block(rng, nfreqs, n) for n in nvecs], [0, 1, 2, 1], seed=seed)
    return out


def folded_2048():
    return _folded_cases()[2048]


def folded_1024():
    return _folded_cases()[1024]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("builder", [folded_2048, folded_1024], ids=["2048", "1024"])
def test_wide_blocks_on_folded_tiles(builder, dtype):
    """Mirror-symmetric blocks kept as their lower half band: the mirror walk flips the sign of the odd vectors, whose parity is that of
    k0 + r in every one of the 4 ... 14 blocks of 64 rows, not of r.  "auto" folds, "general_full" does not; both equal the restatement
    and each other."""
    got = {}
    for path, folded in (("auto", 1), ("general_full", 0)):
        label = f"{builder.__name__} {path} {np.dtype(dtype).name}"
        got[path] = solve_and_check(builder, dtype, label, layout="stream", path=path, folded=folded)
    errs = [plane_err(a, np.asarray(b, np.float64)) for a, b in zip(got["auto"], got["general_full"])]
    print(f"{builder.__name__} {np.dtype(dtype).name}: folded against full c_r {errs[0]:.2e}  c_i {errs[1]:.2e}")
    assert max(errs) <= TOL[np.dtype(dtype)]["plane"]


# ---- 3. the factor in LDS and in scratch
@functools.lru_cache(maxsize=None)
def boundary_case():
    """The factor [n + 2][n | 1] stays in LDS while it has at most 16384 doubles: 126 (16256) and 127 (16383) do, 128 (16770) is the
    first in scratch."""
    return random_problem([126, 127, 128], [2, 2, 2], nfreqs=200, seed=5, rowblocks=True)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_factor_on_both_sides_of_the_lds_bound(dtype):
    """With a scratch bound of one byte every group is a chunk of its own, whose dynamic LDS is sized from that group alone: the same
    bits as the one chunk sized from the widest group."""
    assert [(n + 2) * (n | 1) <= 16384 for n in (126, 127, 128)] == [True, True, False]
    got = [solve_and_check(boundary_case, dtype, f"boundary scratch {bound} {np.dtype(dtype).name}", scratch=bound) for bound in (0, 1)]
    for a, b in zip(*got):
        np.testing.assert_array_equal(a, b)


# ---- 4. interrupted runs of row blocks in one group
ALTERNATING = [0, 0, 1, 1, 0, 2]
FLAGGED = 3  # the second baseline of group 1's second run


def alternating_problem(drop_flagged=False):
    """Group 0: one baseline, 17 vectors.  Group 1: six baselines on the row blocks 0 0 1 1 0 2 of a block of 40 vectors -- two runs of
    two, a run of one on a row block that comes back, a run of one; baseline FLAGGED of it is flagged wholly.  Group 2: two baselines on
    one row block, 33 vectors.  ``drop_flagged``: the same problem without the flagged baseline."""
    rng = np.random.default_rng(44)
    nants, nfreqs = 8, 200
    nvecs, rowblks = [17, 40, 33], [[0], ALTERNATING, [0, 0]]
    basis = [rng.standard_normal(((max(rb) + 1) * nfreqs, n)) / np.sqrt(nfreqs) for n, rb in zip(nvecs, rowblks)]
    rb = np.concatenate(rowblks)
    nbls = len(rb)
    ants = np.array([rng.choice(nants, size=2, replace=False) for _ in range(nbls)])
    w = rng.uniform(0.0, 1.0, size=(nbls, nfreqs)) * (rng.random((nbls, nfreqs)) > 0.1)
    w /= w.sum()
    w[1 + FLAGGED] = 0.0
    data_r, data_i = rng.standard_normal((nbls, nfreqs)), rng.standard_normal((nbls, nfreqs))
    keep = np.arange(nbls) != 1 + FLAGGED if drop_flagged else np.ones(nbls, bool)
    counts = [1, 6 - int(drop_flagged), 2]
    p = FitProblem(nants=nants, nfreqs=nfreqs, basis=basis, grp_basis=np.arange(3, dtype=np.int32),
                   grp_bl_start=np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), bl_ant0=ants[keep, 0].astype(np.int32),
                   bl_ant1=ants[keep, 1].astype(np.int32), bl_rowblk=rb[keep].astype(np.int32), data_r=data_r[keep], data_i=data_i[keep],
                   wgts=w[keep])
    p.validate()
    start = dict(g_r=1.0 + 0.1 * rng.standard_normal((nants, nfreqs)), g_i=0.1 * rng.standard_normal((nants, nfreqs)),
                 c_r=rng.standard_normal(p.ncoeffs), c_i=rng.standard_normal(p.ncoeffs))
    return p, start


@functools.lru_cache(maxsize=None)
def alternating_case():
    return alternating_problem()


@pytest.mark.parametrize("dtype", DTYPES)
def test_row_blocks_that_alternate_inside_a_group(dtype):
    """Consecutive baselines on one row block are one walk of the Gram kernel where they share tiles ("shared"; in "stream" every
    baseline has tiles of its own), and a new walk starts where the row block changes.  Both layouts equal the restatement, in fp64
    also each other.  The wholly flagged baseline inside a merged run has q = u = 0: it adds exact zeros, so the problem without it
    gives the same bits."""
    p, start = alternating_case()
    assert list(p.bl_rowblk[1:7]) == ALTERNATING and not np.any(p.wgts[1 + FLAGGED]) and np.all(p.wgts.sum(axis=1)[np.arange(p.nbls) != 1 + FLAGGED] > 0)
    got = {layout: solve_and_check(alternating_case, dtype, f"alternating {layout} {np.dtype(dtype).name}", layout=layout) for layout in ("stream", "shared")}
    if dtype == np.float64:
        errs = [plane_err(a, b) for a, b in zip(got["stream"], got["shared"])]
        print(f"alternating float64: stream against shared c_r {errs[0]:.2e}  c_i {errs[1]:.2e}")
        assert max(errs) <= TOL[np.dtype(dtype)]["plane"]
    q, start_q = alternating_problem(drop_flagged=True)
    for k in start:
        np.testing.assert_array_equal(start_q[k], start[k])
    for layout in ("stream", "shared"):
        s = solver_of(q, start, dtype, layout)
        assert s.solve_coeffs() == {"nsolved": 3, "nsingular": 0}
        for a, b in zip(s.get_params()[2:], got[layout]):
            np.testing.assert_array_equal(a, b, err_msg=layout)
        s.close()


# ---- 5. every tile width at the narrow end, on a band that no tile width divides
NARROW_NVECS = [1, 7, 56, 57, 112, 113, 224, 225]


@functools.lru_cache(maxsize=None)
def narrow_case():
    """300 channels are padded to 384: the channels [300, 384) of the last tiles must add nothing.  One group on each side of the
    boundaries 56 | 57, 112 | 113, 224 | 225 between the tile widths (fp32 128 | 64 | 32 | 16, fp64 64 | 32 | 16 | 8), in one launch.  One
    baseline per group: 225 vectors on 300 weighted channels have cond(N) = 1.0e3, the largest in this file (an fp32 Gram emulated in
    NumPy with an fp64 solve: 1.6e-5 of the plane)."""
    return random_problem(NARROW_NVECS, [1] * len(NARROW_NVECS), nfreqs=300, seed=6)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", ["stream", "shared"])
def test_both_sides_of_every_tile_width_on_a_padded_band(layout, dtype):
    solve_and_check(narrow_case, dtype, f"narrow {layout} {np.dtype(dtype).name}", layout=layout, folded=0)
