"""NumPy restatement of cal_solver_robust_weights (include/calamity_hip.h), shared by the robust-weight tests.  Everything in float64:

    e[b][f]  = w0[b][f] |d[b][f] - g_i[f] conj(g_j[f]) m[b][f]|^2
    S_b      = { f : w0[b][f] > 0 },  n_b = |S_b|
    med_b    = the ((n_b + 1) // 2)-th smallest of e[b][S_b]            (the lower median)
    scale_b  = med_b / ln 2,  z2 = e / scale_b
    huber  : psi = 1 if z2 <= k^2 else k / sqrt(z2)
    cauchy : psi = 1 / (1 + z2 / k^2)
    clip   : psi = 1 if z2 <= k^2 else 0
    w        = w0 psi;  rows with n_b = 0 or med_b not > 0 keep w = w0 and report scale 0, count 0

Non-finite samples of S_b take what these lines give literally.  A NaN in ``e`` orders above every number, +inf included (``np.partition``
puts it last), so a row with fewer NaN than n_b - rank + 1 has a number for its median and a row whose median is a NaN keeps ``w0``.
Behind a finite scale a NaN sample has ``z2`` = NaN: psi is NaN under Huber and Cauchy (both comparisons with a NaN are false, the weight
becomes NaN and the sample is not counted) and 0 under clip (``z2 <= k^2`` is false: weight ``w0 * 0 = 0``, counted like every other
clipped sample).  An infinite sample has psi = 0 under all three kinds and is counted.

``residual_power_exact`` and ``lower_median_bits`` serve the tests that compare the device bit for bit (tests/test_gpu_robust_exact.py):
``e`` in the solver's dtype where ``m = A c`` is exactly zero, and the kernel's own selection, a bisection on the bit pattern.
"""
import numpy as np

LN2 = float(np.log(2.0))
KINDS = ("huber", "cauchy", "clip")


def lower_median(x):
    """The ((n + 1) // 2)-th smallest element of ``x`` (n >= 1), by selection."""
    x = np.asarray(x, dtype=np.float64)
    k = (len(x) + 1) // 2 - 1
    return float(np.partition(x, k)[k])


def residual_power_exact(d_r, d_i, w0, dtype):
    """``e`` in ``dtype`` where the model ``m = A c`` is exactly zero and the gains are finite: ``g_i conj(g_j) m`` is zero, the residual
    is the data, and ``e = w0 * (d_r * d_r + d_i * d_i)`` with one rounding per operation (the kernel compiles with fp contract off).
    NumPy arithmetic on arrays of ``dtype`` gives the device's bits, subnormals, overflow to +inf and NaN included."""
    d_r, d_i, w0 = (np.asarray(a).astype(dtype) for a in (d_r, d_i, w0))
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return w0 * (d_r * d_r + d_i * d_i)


def lower_median_bits(x, dtype):
    """The ((n + 1) // 2)-th smallest element of ``x`` (n >= 1, no negative numbers) the way robust_rows_kernel selects it: with the
    sign bit cleared the IEEE bit pattern orders like an unsigned integer (a NaN above every number); the rank-th smallest pattern is
    built from the top bit down, a bit being set when fewer than rank keys lie below the trial pattern (31 rounds in float32, 63 in
    float64).  Returns a scalar of ``dtype``: an element of ``x``, possibly a NaN."""
    dtype = np.dtype(dtype)
    ut, bits = {4: (np.uint32, 31), 8: (np.uint64, 63)}[dtype.itemsize]
    keys = np.ascontiguousarray(x, dtype=dtype).view(ut) & ut((1 << bits) - 1)
    rank = (len(keys) + 1) >> 1
    med = ut(0)
    for bit in range(bits - 1, -1, -1):
        trial = med | ut(1 << bit)
        if np.count_nonzero(keys < trial) < rank:
            med = trial
    return np.array([med], dtype=ut).view(dtype)[0]


def residual_power(m_r, m_i, d_r, d_i, w0, g_r, g_i, ant0, ant1):
    """``e`` from the model ``m = A c`` (``solver.model()``), the data, ``w0`` and the gains, all taken to float64 first."""
    f8 = lambda a: np.asarray(a).astype(np.float64)  # noqa: E731
    g = f8(g_r) + 1j * f8(g_i)
    r = (f8(d_r) + 1j * f8(d_i)) - g[np.asarray(ant0)] * np.conj(g[np.asarray(ant1)]) * (f8(m_r) + 1j * f8(m_i))
    return f8(w0) * (r.real**2 + r.imag**2)


def psi_of(z2, kind, k):
    z2 = np.asarray(z2, dtype=np.float64)
    if kind == "huber":
        with np.errstate(divide="ignore", invalid="ignore"):  # (z2 = 0 takes the first branch; a NaN takes the second and stays a NaN)
            return np.where(z2 <= k * k, 1.0, k / np.sqrt(z2))
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
        with np.errstate(invalid="ignore", over="ignore"):
            z2[b][sel] = e[b][sel] / scale[b]
            psi = psi_of(z2[b][sel], kind, k)
            ndown[b] = np.sum(psi < 1.0)
            w[b][sel] = w0[b][sel] * psi
    return dict(w=w, scale_bl=scale, ndown_bl=ndown, z2=z2)
