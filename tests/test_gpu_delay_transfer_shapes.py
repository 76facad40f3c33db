"""cal_solver_delay_transfer on the two slices of 15 rows of test_gpu_row_walk_shapes.py (14 cross-correlations and an
autocorrelation per slice, bl_alias, the SHARED layout's `general` kernels), raw and calibrated, with all nfreqs delays:

nfreqs = 5: fpad = 8 under a row pitch of 32 -- one staged step of the power kernel, mostly padding; one column block of 5 delays.
nfreqs = 260: fpad = 384 -- twelve staged steps, five column blocks with 4 delays in the last; the basis kernel's sixth piece of 64
channels holds nothing but padding past channel 260.

Bounds as in test_gpu_delay_transfer.py."""
import numpy as np
import pytest

import test_gpu_row_walk_shapes as RS
from delay_transfer_ref import bin_rows, restated
from test_gpu_delay_spectrum import operator
from test_gpu_fit_quality import TOL, plane_err

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("calibrated", [False, True], ids=["raw", "calibrated"])
@pytest.mark.parametrize("dtype", RS.DTYPES)
@pytest.mark.parametrize("nfreqs", RS.NFREQS)
def test_two_slices_of_fifteen_rows(nfreqs, dtype, calibrated):
    full, parts, params, _ = RS.batch(nfreqs)
    nb = parts[0].nbls
    assert full.nbls == 2 * nb == 30 and full.bl_alias is not None
    op, _ = operator(nfreqs, nfreqs)
    bins = (np.repeat(np.arange(RS.T), nb) * 2 + np.tile(np.arange(nb) % 2, RS.T)).astype(np.int32)  # (slice, bin)
    ref = restated(full, params["g_r"], params["g_i"], dtype, op, calibrated=calibrated, bin_of_bl=bins, nbins=2 * RS.T)
    assert ref["singular"] == []
    s = RS.solver_of(full, params, dtype)
    out = s.delay_transfer(op, calibrated=calibrated, bin_of_bl=bins, nbins=2 * RS.T, per_baseline=True)
    again = s.delay_transfer(op, calibrated=calibrated, bin_of_bl=bins, nbins=2 * RS.T, per_baseline=True)
    s.close()
    tol = TOL[np.dtype(dtype)]["plane"]
    errs = dict(absorbed=plane_err(out["absorbed_bl"], ref["absorbed_bl"]), num=plane_err(out["absorbed_bl"] * out["noise_bl"], ref["num"]),
                noise=float(np.max(np.abs(out["noise_bl"] - ref["noise_bl"]) / ref["noise_bl"])))
    print(f"{nfreqs} channels {np.dtype(dtype).name} calibrated={calibrated}: largest cond(N) {max(ref['conds']):.2e}  " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert out["absorbed_bl"].shape == (30, nfreqs) and np.all(np.isfinite(out["absorbed_bl"])) and np.all(out["noise_bl"] > 0)
    assert (out["nsolved"], out["nsingular"]) == (full.ngrps, 0)
    assert errs["absorbed"] <= tol and errs["num"] <= tol and errs["noise"] <= 1e-12, errs
    np.testing.assert_array_equal(out["count_bin"], ref["count_bin"])
    own, _ = bin_rows(out["absorbed_bl"], ref["valid"], bins, 2 * RS.T)
    assert np.max(np.abs(out["absorbed_bin"] - own)) <= full.nbls * 2.0 ** -53 * np.max(np.abs(own))
    for k in ("absorbed_bl", "noise_bl", "absorbed_bin", "count_bin"):
        np.testing.assert_array_equal(out[k], again[k], err_msg=k)
