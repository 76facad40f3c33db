"""The float64 NumPy restatement of cal_solver_delay_transfer (include/calamity_hip.h), shared by the delay-transfer tests.  Row b of
fitting group gamma has antennas (i, j) and the basis rows a_{b,f}; w are the weights, g the full gains:

    G = g_i conj(g_j)      q = w |G|^2      mask = (w != 0)
    N = sum_{b in gamma} A_b^T diag(q_b) A_b      N_r = N + ridge (tr N / nvec) I = L L^T
                     raw residual  d - G m        calibrated residual  d / G - m
    s[b][f]     =    mask G                       mask                      (0 where |G|^2 == 0)
    v[b][f]     =    mask / w                     mask / q                  (0 where |G|^2 == 0)
    U[b][k]        = sum_f op[f][k] s[b][f] a_{b,f}          num[b][k] = |L^-1 U[b][k]|^2
    noise_bl[b][k] = sum_f v[b][f] |op[f][k]|^2              absorbed_bl = num / noise_bl   (0 where noise_bl == 0 or the group is singular)
    absorbed_bin[n] = the sum, taken sequentially in ascending row order, of absorbed_bl[b] over the rows with bin_of_bl[b] == n that
                      have an unflagged sample and a factored group; count_bin[n] their number

``restated`` works in float64 on the inputs the solver holds, rounded to its dtype first.  G, |G|^2 and q are formed in that dtype in
the order of the loss kernels (one rounding per operation, no fused multiply-add), as the device forms them, so that s and v are the
device's to the bit and noise_bl differs by the order of a double sum only; every product after that is in float64, with
np.linalg.cholesky and a triangular solve.  ``core`` is the same arithmetic on plain arrays, for the host tests."""
import numpy as np


def core(A_rows, q, s, v, op, ridge):
    """One fitting group: ``A_rows`` list of [F, nvec] (one per baseline), ``q``, ``s``, ``v`` [nb, F], ``op`` [F, nd] complex.
    Returns ``(num, noise, W, cond(N))``, the first two [nb, nd]; ``None`` for a singular group (tr N <= 0)."""
    nv = A_rows[0].shape[1]
    N = np.zeros((nv, nv))
    for A, qb in zip(A_rows, q):
        N += A.T @ (qb[:, None] * A)
    tr = np.trace(N)
    if not tr > 0:
        return None
    L = np.linalg.cholesky(N + ridge * tr / nv * np.eye(nv))
    W = np.linalg.solve(L, np.eye(nv))
    op2 = np.abs(op) ** 2
    num = np.empty((len(A_rows), op.shape[1]))
    for k, (A, sb) in enumerate(zip(A_rows, s)):
        U = (W @ A.T) @ (sb[:, None] * op)  # [nvec, nd] complex
        num[k] = np.sum(np.abs(U) ** 2, axis=0)
    return num, np.asarray(v) @ op2, W, float(np.linalg.cond(N))


def samples(g, ant0, ant1, w, dtype, calibrated):
    """``(q, s, v, mask)`` of every sample, ``q`` and ``s`` formed in ``dtype`` as the kernels form them, returned in float64 / complex128."""
    t = np.dtype(dtype).type
    gr, gi = np.asarray(g.real).astype(dtype), np.asarray(g.imag).astype(dtype)
    w = np.asarray(w).astype(dtype)
    ax, ay, bx, by = gr[ant0], gi[ant0], gr[ant1], gi[ant1]
    Gr = ax * bx + ay * by  # g_i conj(g_j), one rounding per operation
    Gi = ay * bx - ax * by
    den = Gr * Gr + Gi * Gi
    q = w * den
    assert Gr.dtype == np.dtype(dtype) and q.dtype == np.dtype(dtype)
    mask = w != t(0)
    q64, w64 = q.astype(np.float64), w.astype(np.float64)
    if calibrated:
        live = mask & (den != t(0))
        s = live.astype(np.complex128)
        v = np.where(live, 1.0 / np.where(live, q64, 1.0), 0.0)
    else:
        s = np.where(mask, Gr.astype(np.float64) + 1j * Gi.astype(np.float64), 0.0)
        v = np.where(mask, 1.0 / np.where(mask, w64, 1.0), 0.0)
    return q64, s, v, mask


def restated(p, g_r, g_i, dtype, op, ridge=1e-6, calibrated=False, bin_of_bl=None, nbins=0, wgts=None):
    """Everything the call returns for the problem ``p`` at the gains ``g_r + i g_i`` (``wgts``: other weights than ``p.wgts``), plus
    ``num``, ``valid``, the singular groups and cond(N) of the solved ones."""
    cast = lambda a: np.asarray(a).astype(dtype).astype(np.float64)  # noqa: E731
    g = cast(g_r) + 1j * cast(g_i)
    op = cast(np.asarray(op).real) + 1j * cast(np.asarray(op).imag)
    q, s, v, mask = samples(g, p.bl_ant0, p.bl_ant1, p.wgts if wgts is None else wgts, dtype, calibrated)
    F, nd = p.nfreqs, op.shape[1]
    blocks = [cast(blk) for blk in p.basis]
    out = dict(absorbed_bl=np.zeros((p.nbls, nd)), noise_bl=np.zeros((p.nbls, nd)), num=np.zeros((p.nbls, nd)), valid=np.zeros(p.nbls, dtype=bool),
               singular=[], conds=[], q=q)
    for grp in range(p.ngrps):
        b0, b1 = int(p.grp_bl_start[grp]), int(p.grp_bl_start[grp + 1])
        A = [blocks[p.grp_basis[grp]][p.bl_rowblk[b] * F : (p.bl_rowblk[b] + 1) * F] for b in range(b0, b1)]
        res = core(A, q[b0:b1], s[b0:b1], v[b0:b1], op, ridge)
        if res is None:
            out["singular"].append(grp)
            continue
        num, noise, _, cond = res
        out["conds"].append(cond)
        out["num"][b0:b1], out["noise_bl"][b0:b1] = num, noise
        out["absorbed_bl"][b0:b1] = np.where(noise != 0, num / np.where(noise != 0, noise, 1.0), 0.0)
        out["valid"][b0:b1] = mask[b0:b1].any(axis=1)
    out["nsolved"], out["nsingular"] = p.ngrps - len(out["singular"]), len(out["singular"])
    if nbins:
        out["absorbed_bin"], out["count_bin"] = bin_rows(out["absorbed_bl"], out["valid"], bin_of_bl, nbins)
    return out


def bin_rows(absorbed_bl, valid, bin_of_bl, nbins):
    """The bins of given per-baseline rows: sequential double sums in ascending row order; ``count_bin``."""
    out, count = np.zeros((nbins, absorbed_bl.shape[1])), np.zeros(nbins)
    for b, n in enumerate(np.asarray(bin_of_bl)):
        if n < 0 or not valid[b]:
            continue
        count[n] += 1
        out[n] = out[n] + absorbed_bl[b]
    return out, count
