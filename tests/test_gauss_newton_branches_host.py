"""The host parts of tests/test_gpu_gauss_newton_branches.py (no GPU): the decisions of the restatement tests/gauss_newton_ref.py that the
device tests depend on, with their margins; the sizes the large case exists for; the layout constants those sizes are measured against."""
import os
import re

import numpy as np
import pytest

import test_gpu_gauss_newton_branches as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("dtype", B.DTYPES, ids=B.name)
@pytest.mark.parametrize("label", list(B.PLAN))
def test_the_restatement_decides_as_planned_and_not_marginally(label, dtype):
    """``planned`` asserts the margins (1.5 around cg_tol, 1e-2 of the loss around the accept test), the iteration count and the
    acceptance PLAN lists, on the inputs as a solver of ``dtype`` holds them."""
    want = B.planned(label, dtype)
    ncg, cg_tol = B.PLAN[label][2:4]
    assert want["cg_iters"] <= ncg and (want["cg_iters"] == ncg or want["cg_iters"] == 0 or want["cg_residual"] <= cg_tol)


def test_the_quoted_figures_are_the_restatements():
    """The figures the device tests' docstrings quote."""
    stop = B.planned("stop", np.float64)
    np.testing.assert_allclose(stop["residuals"][4:], [1.272e-3, 4.46e-4], rtol=2e-3)
    np.testing.assert_allclose([stop["loss_before"], stop["loss_after"]], [3.786e-2, 8.07e-3], rtol=2e-3)
    finals = [B.planned(k, np.float64)["cg_residual"] for k in B.BATCH[0]]
    np.testing.assert_allclose(finals, [4.46e-4, 2.12e-3, 9.07e-3], rtol=2e-3)
    assert [B.planned(k, np.float64)["cg_iters"] for k in B.BATCH[1]] == [10, 10, 6]
    flagged = B.planned("flagged", np.float64)
    np.testing.assert_allclose([flagged["loss_before"], flagged["loss_after"]], [3.52e-2, 3.57e-4], rtol=2e-3)
    acc, rej = B.planned("group, accepted", np.float64), B.planned("group, rejected", np.float64)
    np.testing.assert_allclose([acc["loss_before"], acc["loss_after"], rej["loss_after"]], [0.2124, 0.1353, 0.3436], rtol=2e-3)
    big = B.planned("big", np.float64)
    np.testing.assert_allclose([big["loss_before"], big["loss_after"]], [4.17e-2, 2.84e-4], rtol=2e-3)


def test_a_slice_with_nothing_to_solve_in_the_restatement():
    zero, nan = B.planned("zero_weights", np.float64), B.planned("nan", np.float64)
    assert zero["rz0"] == 0.0 and zero["loss_before"] == zero["loss_after"] == 0.0 and zero["residuals"] == ()
    assert np.isnan(nan["rz0"]) and np.isnan(nan["loss_before"]) and not nan["accepted"] and nan["cg_residual"] == 0.0
    p, _ = B.problem_of(("slice", 1, "nan"))
    good, _ = B.problem_of(("slice", 1))
    bad = np.argwhere(np.isnan(p.data_r))
    assert len(bad) == 1 and good.wgts[tuple(bad[0])] > 0 and np.all(np.isfinite(good.data_r))  # (the cached good slice is untouched)


def test_the_flagged_antenna_has_zero_diagonal_entries_before_they_are_replaced():
    """den = 0 for antenna 3 and a zero row sum for its six groups: ``Ref.precond`` hands back 1 there, and the step's direction is 0."""
    p, start = B.flagged_problem()
    rows = B.flagged_rows(p)
    assert len(rows) == 6 and np.all(np.asarray(p.wgts)[rows] == 0) and np.all(np.diff(p.grp_bl_start) == 1)
    ref = B.Ref(p)
    d_g, d_c = ref.precond(*B.cast_params(start, np.float64))
    coff = np.asarray(p.grp_coff)
    idx = np.concatenate([np.arange(coff[g], coff[g + 1]) for g in rows])
    assert np.all(d_g[B.FLAGGED_ANTENNA] == 1.0) and np.all(d_c[idx] == 1.0)
    others = np.setdiff1d(np.arange(p.nants), [B.FLAGGED_ANTENNA])
    assert np.all(d_g[others] != 1.0) and np.all(d_g[others] > 0)
    want = B.planned("flagged", np.float64)
    assert np.all(want["dg"][B.FLAGGED_ANTENNA] == 0) and np.all(want["dc"][idx] == 0) and np.all(want["dg"][others] != 0)


def test_the_large_problem_has_the_sizes_its_tests_exist_for():
    p, _ = B.big_problem()
    sizes = B.big_sizes(p)
    assert sizes == dict(nbls=276, ngrps=276, ncoeffs=9532, fpad=384, gain_reals=18432, reals=37496, rows_per_thread=2, empty_runs=118)
    assert B.big_sizes(B.big_problem(6)[0]) == sizes
    assert [B.fpad_of(n) for n in (8, 48, 64, 65, 128, 200, 260, 1024)] == [8, 64, 64, 128, 128, 256, 384, 1024]
    p3, _ = B.redundant_problem()
    assert np.diff(p3.grp_bl_start).max() == 3


def test_the_layout_constants_are_those_of_the_kernels():
    """A change of kGnBlocks, of a block size or of the row padding must fail here, not leave the large case testing one trip."""
    src = open(os.path.join(ROOT, "calamity_amd", "csrc", "gauss_newton_kernels.hpp")).read()
    assert re.search(rf"constexpr int kGnBlocks = {B.GN_BLOCKS};", src)
    for kernel in ("gn_rhs_kernel", "gn_init_kernel", "gn_diff_kernel", "gn_update1_kernel", "gn_update2_kernel", "gn_apply_kernel", "gn_scale_kernel",
                   "gn_precond_coeff_kernel"):
        assert re.search(rf"__launch_bounds__\({B.GN_THREADS}\) void {kernel}\(", src), kernel
    assert src.count(f"e += {B.GN_THREADS}ll * gridDim.x") == 6
    assert f"(r1 - r0 + {B.GN_THREADS - 1}) / {B.GN_THREADS}" in src and f"blockIdx.x * {B.GN_THREADS} + threadIdx.x;\n  if (g >= ngrps)" in src
    plan = open(os.path.join(ROOT, "calamity_amd", "csrc", "problem_plan.hpp")).read()
    assert "while (pw < 128 && pw < nfreqs) pw *= 2;" in plan and "fpad = (nfreqs + pw - 1) / pw * pw;" in plan
