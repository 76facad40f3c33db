"""NumPy restatement of cal_solver_robust_weights (include/calamity_hip.h), shared by the robust-weight tests.  Everything in float64:

    e[b][f]  = w0[b][f] |d[b][f] - g_i[f] conj(g_j[f]) m[b][f]|^2
    S_b      = { f : w0[b][f] > 0 },  n_b = |S_b|
    med_b    = the ((n_b + 1) // 2)-th smallest of e[b][S_b]            (the lower median)
    scale_b  = med_b / ln 2,  z2 = e / scale_b
    huber  : psi = 1 if z2 <= k^2 else k / sqrt(z2)
    cauchy : psi = 1 / (1 + z2 / k^2)
    clip   : psi = 1 if z2 <= k^2 else 0
    w        = w0 psi;  rows with n_b = 0 or med_b = 0 keep w = w0 and report scale 0, count 0
"""
import numpy as np

LN2 = float(np.log(2.0))
KINDS = ("huber", "cauchy", "clip")


def lower_median(x):
    """The ((n + 1) // 2)-th smallest element of ``x`` (n >= 1), by selection."""
    x = np.asarray(x, dtype=np.float64)
    k = (len(x) + 1) // 2 - 1
    return float(np.partition(x, k)[k])


def residual_power(m_r, m_i, d_r, d_i, w0, g_r, g_i, ant0, ant1):
    """``e`` from the model ``m = A c`` (``solver.model()``), the data, ``w0`` and the gains, all taken to float64 first."""
    f8 = lambda a: np.asarray(a).astype(np.float64)  # noqa: E731
    g = f8(g_r) + 1j * f8(g_i)
    r = (f8(d_r) + 1j * f8(d_i)) - g[np.asarray(ant0)] * np.conj(g[np.asarray(ant1)]) * (f8(m_r) + 1j * f8(m_i))
    return f8(w0) * (r.real**2 + r.imag**2)


def psi_of(z2, kind, k):
    z2 = np.asarray(z2, dtype=np.float64)
    if kind == "huber":
        return np.where(z2 <= k * k, 1.0, k / np.sqrt(np.where(z2 > 0, z2, 1.0)))
    if kind == "cauchy":
        return 1.0 / (1.0 + z2 / (k * k))
    if kind == "clip":
        return np.where(z2 <= k * k, 1.0, 0.0)
    raise ValueError(kind)


def robust_weights(e, w0, kind="huber", k=3.0):
    """``dict(w, scale_bl, ndown_bl, z2)``; ``z2`` is NaN outside ``S_b`` and on rows that keep ``w0``."""
    e, w0 = np.asarray(e, dtype=np.float64), np.asarray(w0, dtype=np.float64)
    w = w0.copy()
    z2 = np.full(e.shape, np.nan)
    scale, ndown = np.zeros(len(e)), np.zeros(len(e))
    for b in range(len(e)):
        sel = w0[b] > 0
        if not np.any(sel):
            continue
        med = lower_median(e[b][sel])
        if not med > 0:
            continue
        scale[b] = med / LN2
        z2[b][sel] = e[b][sel] / scale[b]
        psi = psi_of(z2[b][sel], kind, k)
        ndown[b] = np.sum(psi < 1.0)
        w[b][sel] = w0[b][sel] * psi
    return dict(w=w, scale_bl=scale, ndown_bl=ndown, z2=z2)
