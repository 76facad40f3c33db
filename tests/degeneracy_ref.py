"""Double-precision NumPy restatement of cal_solver_fix_degeneracies (include/calamity_hip.h) for ONE slice, written from its formulae.

A fit constrains only ``g_i conj(g_j) m_b``.  Per channel an amplitude ``eta``, a phase ``psi`` and a tilt ``Phi`` (rad / m, east and
north) bring the fitted model ``m`` onto a reference ``s``::

    z0 = w conj(m) s   (w > 0 only; products in ``dtype``)       Q = sum_b w |m|^2        H = sum_b |z0| d d^T
    Phi = 0;  iters times:  q = sum_b Im(z0 e^{-i Phi.d}) d,  Phi += H^+ q
    e^{2 eta} = max(sum_b Re(z0 e^{-i Phi.d}), 0) / Q
    psi = arg sum_a g_a e^{-i Phi.r_a} conj(gref_a)   over the antennas with a cross-correlation row with w > 0
    m' = m e^{2 eta} e^{i Phi.d},  g' = g e^{-eta} e^{-i (Phi.r + psi)}
"""
import numpy as np


def step2(a, b, c, qe, qn):
    """H^+ q for H = [a b; b c] with tr H > 0: the inverse where det H > 1e-12 (tr H / 2)^2, else along the dominant eigenvector."""
    tr, det = a + c, a * c - b * b
    if det > 1e-12 * (0.5 * tr) ** 2:
        return (c * qe - b * qn) / det, (a * qn - b * qe) / det
    lam = 0.5 * tr + np.sqrt((0.5 * (a - c)) ** 2 + b * b)
    v = np.array([lam - c, b])
    u = np.array([b, lam - a])
    if u @ u > v @ v:
        v = u
    n2 = v @ v
    if not (n2 > 0 and lam > 0):
        return 0.0, 0.0
    proj = (v[0] * qe + v[1] * qn) / (n2 * lam)
    return v[0] * proj, v[1] * proj


def fix_degeneracies(m, s, w, g, ant0, ant1, antpos, iters=6, mode="channel", freqs=None, gref=None, dtype=np.float64):
    """``m``, ``s`` complex ``[nbls, nfreqs]``, ``w`` real, ``g`` (and ``gref``) complex ``[nants, nfreqs]``, ``antpos`` ``[nants, 2]``.
    Returns a dict: ``eta``, ``psi``, ``nsamples``, ``last_step`` ``[nfreqs]``, ``tilt`` ``[nfreqs, 2]``, ``g``, ``model`` complex128 (not
    rounded to ``dtype``)."""
    dtype = np.dtype(dtype)
    ant0, ant1 = np.asarray(ant0), np.asarray(ant1)
    antpos = np.asarray(antpos, dtype=np.float64)
    d = antpos[ant0] - antpos[ant1]  # [nbls, 2]
    nbls, nf = m.shape
    mr, mi = np.asarray(m.real, dtype=dtype), np.asarray(m.imag, dtype=dtype)
    sr, si = np.asarray(s.real, dtype=dtype), np.asarray(s.imag, dtype=dtype)
    wt = np.asarray(w, dtype=dtype)
    live = wt > 0
    with np.errstate(invalid="ignore", over="ignore"):
        z0 = np.where(live, wt * (mr * sr + mi * si), 0).astype(np.float64) + 1j * np.where(live, wt * (mr * si - mi * sr), 0).astype(np.float64)
        Q = np.where(live, wt * (mr * mr + mi * mi), 0).astype(np.float64).sum(axis=0)
    a0 = np.abs(z0)
    hee, hen, hnn = (a0 * (d[:, 0] ** 2)[:, None]).sum(0), (a0 * (d[:, 0] * d[:, 1])[:, None]).sum(0), (a0 * (d[:, 1] ** 2)[:, None]).sum(0)
    cnt = live.sum(axis=0).astype(np.float64)
    ok = (Q > 0) & (hee + hnn > 0)
    maxd = np.sqrt((d ** 2).sum(axis=1)).max()
    band = mode == "band"
    ratio = np.ones(nf) if not band else np.asarray(freqs, dtype=np.float64) / np.mean(np.asarray(freqs, dtype=np.float64))
    phi = np.zeros((nf, 2))
    phi0 = np.zeros(2)
    last = np.zeros(nf)

    def rotated(phi):
        return z0 * np.exp(-1j * (d @ phi.T))  # [nbls, nf]

    for _ in range(int(iters)):
        z = rotated(phi)
        qe, qn = (z.imag * d[:, :1]).sum(0), (z.imag * d[:, 1:]).sum(0)
        if band:
            r = ratio[ok]
            A, B, C = (r * r * hee[ok]).sum(), (r * r * hen[ok]).sum(), (r * r * hnn[ok]).sum()
            se, sn = (0.0, 0.0) if not (Q[ok].sum() > 0 and A + C > 0) else step2(A, B, C, (r * qe[ok]).sum(), (r * qn[ok]).sum())
            phi0 += (se, sn)
            phi = np.where(ok[:, None], ratio[:, None] * phi0[None, :], 0.0)
            last = np.where(ok, np.abs(ratio) * np.hypot(se, sn) * maxd, 0.0)
        else:
            for f in range(nf):
                se, sn = step2(hee[f], hen[f], hnn[f], qe[f], qn[f]) if ok[f] else (0.0, 0.0)
                phi[f] += (se, sn)
                last[f] = np.hypot(se, sn) * maxd
    sre = rotated(phi).real.sum(0)
    if band:
        tot = sre[ok].sum()
        good = ok & (tot > 0) & (Q[ok].sum() > 0)
        amp2 = np.where(good, tot / max(Q[ok].sum(), np.finfo(float).tiny), 1.0)
    else:
        good = ok & (sre > 0)
        amp2 = np.where(good, sre / np.where(Q > 0, Q, 1.0), 1.0)
    eta = 0.5 * np.log(amp2)
    phi[~good] = 0.0
    last[~good] = 0.0
    cnt[~good] = 0.0
    psi = np.zeros(nf)
    g = np.asarray(g, dtype=np.complex128)
    if gref is not None:
        cross = ant0 != ant1
        nants = g.shape[0]
        seen = np.zeros((nants, nf), dtype=bool)
        for b in np.nonzero(cross)[0]:
            seen[ant0[b]] |= live[b]
            seen[ant1[b]] |= live[b]
        rot = g * np.exp(-1j * (antpos @ phi.T)) * np.conj(np.asarray(gref, dtype=np.complex128))
        psi = np.where(good, np.angle(np.where(seen, rot, 0).sum(axis=0)), 0.0)
    g_out = g * np.exp(-eta)[None, :] * np.exp(-1j * (antpos @ phi.T + psi[None, :]))
    m_out = np.asarray(m, dtype=np.complex128) * amp2[None, :] * np.exp(1j * (d @ phi.T))
    return dict(eta=eta, psi=psi, tilt=phi, nsamples=cnt, last_step=last, g=g_out, model=m_out)


def hex_array(nants, spacing=14.6):
    """East, north positions ``[nants, 2]`` of the first ``nants`` antennas of a hexagonal grid, row by row."""
    nants = int(nants)
    pos, row = [], 0
    while len(pos) < nants:
        for k in range(int(np.ceil(np.sqrt(nants))) + 1):
            if len(pos) < nants:
                pos.append((spacing * (k + 0.5 * (row % 2)), spacing * row * np.sqrt(3.0) / 2.0))
        row += 1
    return np.asarray(pos)


def line_array(nants, spacing=14.6):
    return np.stack([spacing * np.arange(nants), np.zeros(nants)], axis=1)
