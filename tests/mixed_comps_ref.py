"""The device route of the mixed-model components (csrc/mixed_comps_kernels.hpp, simple_cov.device_model_comps) restated in fp64
NumPy: diagonally pivoted Cholesky of the covariance (argmax of the running diagonal, ties to the lowest index, stopped below
``tol = max(1e-13, 1e-3 eigenval_cutoff)`` or at the rank cap), the eigenpairs of ``L^T L``, ``V = L U lambda^-1/2``, the certificate
``||C - L L^T||_F`` and the acceptance ``status ok and resid_fro <= 0.1 eigenval_cutoff lambda_max``.

Near-ties make the pivot ORDER rounding-dependent (a Toeplitz group is mirror-symmetric: the two largest diagonals differ by 1.7e-13
relative and less), so a device factor is not compared with ``pivoted_cholesky`` element by element.  ``replay`` instead recomputes
the factor for a GIVEN pivot list in the kernel's order of operations, in float64 and in longdouble: the difference of the two is the
reference's own noise for that list, and what the pivot rule and the stop demand of the list is checked on the replayed diagonals."""
import numpy as np

from calamity_amd import simple_cov


def pivoted_cholesky(cmat, tol, cap=None):
    """``(L [n, k], pivots, status, max_d)``: status 0 below ``tol``, 1 at the cap."""
    n = len(cmat)
    cap = n if cap is None else min(cap, n)
    d = np.diag(cmat).astype(np.float64)
    L = np.zeros((n, cap))
    piv = []
    while True:
        p = int(np.argmax(d))  # (the first of equal maxima: the lowest index)
        if not d[p] >= tol or len(piv) >= cap:
            break
        m = len(piv)
        col = (cmat[:, p] - L[:, :m] @ L[p, :m]) / np.sqrt(d[p])
        d = np.maximum(d - col * col, 0.0)
        d[p] = 0.0
        L[:, m] = col
        piv.append(p)
    return L[:, : len(piv)], np.asarray(piv), 0 if d[p] < tol else 1, float(d[p])


def cov_column(blvecs, freqs, p, ant_dly=0.0, horizon=1.0, offset=0.0, min_dly=0.0, **_ignored):
    """Column ``p`` of ``simple_cov.simple_cov_matrix(blvecs, freqs, ...)`` in float64 from its formula, operation by operation, without
    the dense matrix (test_mixed_comps_host.py holds it to that column with ``array_equal``)."""
    uvws = np.asarray(blvecs, dtype=np.float64).reshape(-1, 3)
    freqs = np.asarray(freqs, dtype=np.float64)
    pts = (uvws[:, None, :] * (freqs[None, :, None] / 3e8)).reshape(-1, 3)
    sep = np.zeros(len(pts))
    for axis in range(3):
        sep += np.abs(pts[:, axis] - pts[p, axis]) ** 2.0
    sep = np.sqrt(sep) * horizon
    fvals = np.tile(freqs, len(uvws))
    dfg = np.abs(fvals - fvals[p]) / 1e9
    sep += dfg * offset
    col = np.sinc(2 * np.maximum(min_dly * dfg, sep))
    return col * np.sinc(2 * dfg * ant_dly)


def as_columns(cmat):
    """A dense matrix as the ``columns`` of ``replay`` and ``pivoted_cholesky_columns``."""
    return lambda p: cmat[:, p]


def pivoted_cholesky_columns(columns, n, tol, cap=None):
    """``pivoted_cholesky`` on a covariance given as ``columns(p) -> C[:, p]`` with a unit diagonal (n = 16 640 has no dense matrix
    here): the same statements, so the same bits where the columns are the same.  A dict: ``L``, ``pivots``, ``status``, ``max_d`` and
    ``last_d``, the diagonal of the last pivot when it was chosen."""
    cap = n if cap is None else min(cap, n)
    d = np.ones(n)
    L = np.zeros((n, cap))
    piv, last_d = [], np.inf
    while True:
        p = int(np.argmax(d))
        if not d[p] >= tol or len(piv) >= cap:
            break
        m = len(piv)
        last_d = float(d[p])
        col = (columns(p) - L[:, :m] @ L[p, :m]) / np.sqrt(d[p])
        d = np.maximum(d - col * col, 0.0)
        d[p] = 0.0
        L[:, m] = col
        piv.append(p)
    return dict(L=L[:, : len(piv)], pivots=np.asarray(piv), status=0 if d[p] < tol else 1, max_d=float(d[p]), last_d=last_d, k=len(piv))


def replay(columns, pivots, dtype, n=None, diag=None):
    """The factor of the GIVEN pivot list in the kernel's order of operations (mixed_step_kernel), in ``dtype`` (float64 or
    longdouble): ``(L [n, k], d [k + 1, n])``, ``d[m]`` the running diagonal before step m and ``d[k]`` after the last.  Per step:
    ``c = C[:, p]``, ``c -= L[:, j] L[p, j]`` for ascending j one column at a time (no BLAS product: its order of summation is not the
    kernel's), ``l = c / sqrt(d[p])``, ``d -= l l`` with what is not positive clamped to 0, ``d[p] = 0``.  ``columns`` is a dense
    matrix or ``columns(p) -> C[:, p]`` (then ``n``); ``diag`` defaults to the unit diagonal of a covariance."""
    if not callable(columns):
        cmat = np.asarray(columns)
        n, diag, columns = len(cmat), np.diag(cmat), as_columns(cmat)
    d = np.ones(n, dtype=dtype) if diag is None else np.array(diag, dtype=dtype)
    k = len(pivots)
    L = np.zeros((n, k), dtype=dtype, order="F")
    ds = np.zeros((k + 1, n), dtype=dtype)
    for m, p in enumerate(pivots):
        p = int(p)
        ds[m] = d
        c = np.array(columns(p), dtype=dtype)
        for j in range(m):
            c -= L[:, j] * L[p, j]
        col = c / np.sqrt(d[p])
        d = d - col * col
        d[~(d > 0)] = 0
        d[p] = 0
        L[:, m] = col
    ds[k] = d
    return L, ds


def model_comps(blvecs, freqs, eigenval_cutoff=1e-10, cap=None, **params):
    """Everything the device route reports for one group, as a dict; ``V`` is None where the group is not accepted."""
    cmat = simple_cov.simple_cov_matrix(blvecs, freqs, **params)
    L, piv, status, max_d = pivoted_cholesky(cmat, max(1e-13, 1e-3 * eigenval_cutoff), cap)
    resid = float(np.linalg.norm(cmat - L @ L.T))
    evals, U = np.linalg.eigh(L.T @ L)
    reason = None if status == 0 else "rank cap"
    if reason is None and not (evals[-1] > 0.0 and resid <= 0.1 * eigenval_cutoff * evals[-1]):
        reason = "certificate"
    keep = np.nonzero(evals / evals[-1] >= eigenval_cutoff)[0][::-1]
    V = L @ (U[:, keep] / np.sqrt(evals[keep])) if reason is None else None
    return dict(cmat=cmat, L=L, pivots=piv, status=status, max_d=max_d, resid_fro=resid, k=L.shape[1], lambda_max=float(evals[-1]),
                evals=evals[keep], kept=len(keep), reason=reason, V=V)


def host_eig(cmat, eigenval_cutoff=1e-10):
    """The host route's eigenpairs, strongest first: ``(all eigenvalues, kept count, kept vectors)``."""
    evals, evecs = np.linalg.eigh(cmat)
    keep = evals / evals[-1] >= eigenval_cutoff
    return evals[::-1], int(np.count_nonzero(keep)), evecs[:, keep][:, ::-1]
