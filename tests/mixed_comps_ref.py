"""The device route of the mixed-model components (csrc/mixed_comps_kernels.hpp, simple_cov.device_model_comps) restated in fp64
NumPy: diagonally pivoted Cholesky of the covariance (argmax of the running diagonal, ties to the lowest index, stopped below
``tol = max(1e-13, 1e-3 eigenval_cutoff)`` or at the rank cap), the eigenpairs of ``L^T L``, ``V = L U lambda^-1/2``, the certificate
``||C - L L^T||_F`` and the acceptance ``status ok and resid_fro <= 0.1 eigenval_cutoff lambda_max``."""
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
