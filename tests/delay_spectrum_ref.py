"""The float64 NumPy restatement of cal_solver_delay_spectrum (include/calamity_hip.h), shared by the delay-spectrum tests:

    mask = (w != 0)                     x_q = mask q,  q = d, G m, d - G m   (calibrated: d / G, m, d / G - m, zero where |G|^2 == 0)
    X_q = x_q @ op                      norm_bl = mask @ norm_f              power = |X_q|^2 / norm_bl, 0 where norm_bl == 0
    power_bin[q][n] = the sum, taken sequentially in ascending row order, of power[q][b] over the rows with bin_of_bl[b] == n, norm_bl[b] > 0

and the bound the device is held to.  With u the unit roundoff of the solver's dtype, a[b][f] the size of what is rounded per sample

    tau[b][k] = C u (nfreqs + 16) sum_f mask a[b][f] |op[f][k]|,   a = |d| + |G| |m|  (calibrated: |d / G| + |m|),   C = 8

is the forward error of a dot product of 2 nfreqs terms plus the rounding of the inputs formed in the dtype, and with X = X_ref + dX,
|dX| <= tau:  | |X|^2 - |X_ref|^2 | <= (2 |X_ref| + tau) tau.  The division by norm_bl is in double on both sides."""
import numpy as np

NAMES = ("data", "model", "resid")
UNIT = {np.dtype(np.float64): 2.0 ** -53, np.dtype(np.float32): 2.0 ** -24}
BOUND_CONSTANT = 8.0


def model_of(p, c_r, c_i, dtype):
    """m = A c of every baseline row in float64, from the basis and coefficients rounded to ``dtype``."""
    cast = lambda a: np.asarray(a).astype(dtype).astype(np.float64)  # noqa: E731
    c = cast(c_r) + 1j * cast(c_i)
    coff = p.grp_coff
    m = np.empty((p.nbls, p.nfreqs), dtype=np.complex128)
    for grp in range(p.ngrps):
        blk = cast(p.basis[p.grp_basis[grp]])
        for b in range(p.grp_bl_start[grp], p.grp_bl_start[grp + 1]):
            m[b] = blk[p.bl_rowblk[b] * p.nfreqs : (p.bl_rowblk[b] + 1) * p.nfreqs] @ c[coff[grp] : coff[grp + 1]]
    return m


def quantities(d, m, G, w, calibrated=False):
    """``({name: x_q [nbls, nfreqs] complex128}, mask, a)``: the masked quantities and the per-sample size ``a`` of the bound."""
    mask = np.asarray(w) != 0
    if calibrated:
        ok = np.abs(G) ** 2 != 0
        Gs = np.where(ok, G, 1.0)
        dq, mq = np.where(ok, d / Gs, 0.0), np.where(ok, m, 0.0)
    else:
        dq, mq = d, G * m
    q = {"data": dq, "model": mq, "resid": dq - mq}
    return {k: np.where(mask, v, 0.0) for k, v in q.items()}, mask, np.where(mask, np.abs(dq) + np.abs(mq), 0.0)


def restated(d, m, G, w, op, norm_f, calibrated=False, bin_of_bl=None, nbins=0):
    """Everything the call returns, in float64, plus ``X`` (the transforms) and ``tau`` per unit roundoff (multiply by ``UNIT[dtype]``)."""
    op = np.asarray(op, dtype=np.complex128)
    x, mask, a = quantities(d, m, G, w, calibrated)
    norm_bl = mask.astype(np.float64) @ np.asarray(norm_f, dtype=np.float64)
    out = {"norm_bl": norm_bl, "X": {}, "per_baseline": {}}
    safe = np.where(norm_bl != 0, norm_bl, 1.0)[:, None]
    for k in NAMES:
        X = x[k] @ op  # the transform as a plain matrix product
        out["X"][k] = X
        out["per_baseline"][k] = np.where(norm_bl[:, None] != 0, np.abs(X) ** 2 / safe, 0.0)
    out["tau_per_unit"] = BOUND_CONSTANT * (op.shape[0] + 16) * (a @ np.abs(op))
    if nbins:
        binned = bin_rows(out["per_baseline"], norm_bl, bin_of_bl, nbins)
        out.update(binned)
    return out


def bin_rows(per_baseline, norm_bl, bin_of_bl, nbins):
    """The bins of given per-baseline powers: sequential double sums in ascending row order; ``count_bin``."""
    out = {k: np.zeros((nbins, v.shape[1])) for k, v in per_baseline.items()}
    count = np.zeros(nbins)
    for b, n in enumerate(np.asarray(bin_of_bl)):
        if n < 0 or not norm_bl[b] > 0:
            continue
        count[n] += 1
        for k, v in per_baseline.items():
            out[k][n] = out[k][n] + v[b]
    out["count_bin"] = count
    return out


def bound_ratio(P, ref, name, dtype):
    """The largest ``|P - P_ref| norm_b / ((2 |X_ref| + tau) tau)`` over the plane (0 / 0 counts as 0)."""
    tau = UNIT[np.dtype(dtype)] * ref["tau_per_unit"]
    err = np.abs(P - ref["per_baseline"][name]) * ref["norm_bl"][:, None]
    bound = (2.0 * np.abs(ref["X"][name]) + tau) * tau
    return float(np.max(np.divide(err, bound, out=np.zeros_like(err), where=err > 0)))
