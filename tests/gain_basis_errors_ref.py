"""fp64 NumPy restatement of cal_solver_gain_basis_errors (include/calamity_hip.h), with the dense inverse per system, and a CPU
emulation of the device's fp32 arithmetic.  No GPU; imported by tests/test_gain_basis_errors_host.py and the GPU tests.

``den[row][f]`` is the per-row sum of a per-channel sweep (autocorrelations left out), ``shift = ridge tr N / n``.  Every case is built
from the DENSE design matrix ``X`` of one system (rows: the gains it determines, columns: its unknowns), so the restatement knows
nothing of the Kronecker shortcut or of triangular factors::

    N = X^T diag(den) X      N_r = N + shift I      C = N_r^-1
    y_var = diag C           gain_var = diag(X C X^T)           gain_dof = n - shift tr C

frequency basis: X = B, one system per antenna row; time x frequency: X = kron(Bt, B), rows (t, f), one system per antenna; time basis
alone: X = Bt, one system per (antenna, channel), the dof summed over an antenna's solved channels.  A system with ``tr N <= 0`` or a
failed Cholesky factorisation leaves zeros and counts as singular."""
import numpy as np

from test_gain_time_solve_host import row_sums
from test_gpu_gain_solve import model_of


def den_of(p, params, dtype):
    """``den`` ``[nants, nfreqs]`` in fp64 from the inputs a solver of ``dtype`` holds (cast to it first)."""
    cast = lambda a: np.asarray(a).astype(dtype).astype(np.float64)  # noqa: E731
    w = cast(p.wgts)
    g = cast(params["g_r"]) + 1j * cast(params["g_i"])
    m = model_of(p, params, dtype)
    return row_sums(p.bl_ant0, p.bl_ant1, np.zeros_like(m), w * np.abs(m) ** 2, g)[1]


def system_errors(X, den, ridge):
    """One system: ``(gain_var [rows of X], y_var [n], dof)`` or ``None`` where it is singular."""
    n = X.shape[1]
    N = X.T @ (den[:, None] * X)
    tr = np.trace(N)
    if not (tr > 0 and np.isfinite(tr)):
        return None
    shift = ridge * (tr / n)
    Nr = N + shift * np.eye(n)
    try:
        np.linalg.cholesky(Nr)
    except np.linalg.LinAlgError:
        return None
    C = np.linalg.inv(Nr)
    return np.einsum("ik,kl,il->i", X, C, X), np.diag(C).copy(), n - shift * np.trace(C)


def basis_errors(den, Bt=None, B=None, ridge=1e-6):
    """``den`` ``[nants, F]`` (``[T Na, F]``, row ``t Na + a``, with ``Bt`` ``[T, L]``); ``B`` ``[F, K]`` or None.  Returns a dict like
    ``HipFitSolver.gain_basis_errors``: ``gain_var`` ``[nants, F]``, ``y_var`` ``[nants, K]`` / ``[Na, L, K]`` / ``[Na, L, F]``,
    ``gain_dof``, ``nsolved``, ``nsingular``."""
    den = np.asarray(den, dtype=np.float64)
    rows, F = den.shape
    gain_var = np.zeros((rows, F))
    nsolved = nsingular = 0
    if Bt is None:
        K = B.shape[1]
        y_var, dof = np.zeros((rows, K)), np.zeros(rows)
        for a in range(rows):
            out = system_errors(B, den[a], ridge)
            if out is None:
                nsingular += 1
                continue
            nsolved += 1
            gain_var[a], y_var[a], dof[a] = out
        return dict(gain_var=gain_var, y_var=y_var, gain_dof=dof, nsolved=nsolved, nsingular=nsingular)
    T, L = Bt.shape
    na = rows // T
    dof = np.zeros(na)
    if B is not None:
        K = B.shape[1]
        X = np.kron(Bt, B)  # [(t, f), (l, k)]
        y_var = np.zeros((na, L, K))
        for a in range(na):
            out = system_errors(X, den[a::na].reshape(-1), ridge)
            if out is None:
                nsingular += 1
                continue
            nsolved += 1
            gain_var[a::na], y_var[a], dof[a] = out[0].reshape(T, F), out[1].reshape(L, K), out[2]
        return dict(gain_var=gain_var, y_var=y_var, gain_dof=dof, nsolved=nsolved, nsingular=nsingular)
    y_var = np.zeros((na, L, F))
    for a in range(na):
        for f in range(F):
            out = system_errors(Bt, den[a::na, f], ridge)
            if out is None:
                nsingular += 1
                continue
            nsolved += 1
            gain_var[a::na, f], y_var[a, :, f] = out[0], out[1]
            dof[a] += out[2]
    return dict(gain_var=gain_var, y_var=y_var, gain_dof=dof, nsolved=nsolved, nsingular=nsingular)


def restated_errors(p, params, dtype, Bt=None, B=None, ridge=1e-6):
    """``basis_errors`` on the inputs a solver of ``dtype`` holds (planes and bases cast to it first)."""
    cast = lambda a: None if a is None else np.asarray(a).astype(dtype).astype(np.float64)  # noqa: E731
    return basis_errors(den_of(p, params, dtype), cast(Bt), cast(B), ridge)


def emulated_fp32_error(den, Bt=None, B=None, ridge=1e-6):
    """What fp32 costs on a problem with a frequency basis: the Gram matrix formed and rounded in fp32, the factor in fp64, W = L^-1
    rounded to fp32, Z = W X^T in fp32 and its squares summed in fp64 -- against ``basis_errors`` on the same fp32-rounded inputs.
    Returns ``(error of gain_var, error of y_var, largest cond(N_r))``, the errors as fractions of the plane's largest element."""
    f32 = lambda a: np.asarray(a).astype(np.float32)  # noqa: E731
    den32, B32 = f32(den), f32(B)
    want = basis_errors(den32.astype(np.float64), None if Bt is None else f32(Bt).astype(np.float64), B32.astype(np.float64), ridge)
    rows, F = den32.shape
    T = 1 if Bt is None else Bt.shape[0]
    na = rows // T
    X32 = B32 if Bt is None else f32(np.kron(f32(Bt).astype(np.float64), B32.astype(np.float64)))
    n = X32.shape[1]
    gain_var, y_var, cond = np.zeros((rows, F)), np.zeros((na, n)), 0.0
    for a in range(na):
        d = den32[a::na].reshape(-1)
        N32 = (X32.T * d[None, :]) @ X32  # fp32 throughout
        N = N32.astype(np.float64)
        tr = np.trace(N)
        if not tr > 0:
            continue
        Nr = N + ridge * (tr / n) * np.eye(n)
        try:
            Lc = np.linalg.cholesky(Nr)
        except np.linalg.LinAlgError:
            continue
        cond = max(cond, float(np.linalg.cond(Nr)))
        W = np.linalg.inv(Lc)
        y_var[a] = np.sum(W * W, axis=0)
        Z = f32(W) @ X32.T  # fp32
        gain_var[a::na] = np.sum(Z.astype(np.float64) ** 2, axis=0).reshape(T, F)
    err = lambda got, ref: float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))  # noqa: E731
    return err(gain_var, want["gain_var"]), err(y_var, want["y_var"].reshape(na, n)), cond
