"""The float64 NumPy restatement of cal_solver_delay_coherent_spectrum (include/calamity_hip.h), shared by the coherent-average tests,
built on delay_fringe_ref and delay_spectrum_ref (imported, not copied).  Set v = g T + t holds the members k in
[set_ptr[v], set_ptr[v + 1]) with rows b_k, coefficients omega_k and conjugation flags:

    u_k = omega_k  or  omega_k w[b_k],  0 where w[b_k] == 0        den_v = sum_k u_k        xbar_q[v] = sum_k u_k c_k(q[b_k]) / den_v
    mask_v = den_v > 0        mask_g = AND over t of mask_(g, t)        x_q[g][t] = mask_g xbar_q[g T + t]

with q[b] formed under the row's own mask (delay_spectrum_ref.quantities).  From x_q on it is delay_fringe_ref.restated itself: the
averaged planes are handed to it as the data and the model of nsets rows with unit gains, and the set masks as their weights, so that
its common mask is mask_g; the residual, which the definition averages as a quantity of its own, goes through a second call as data.

The bound is delay_fringe_ref.bound_plane with the per-sample size a replaced by the u-weighted mean of the members' a,

    abar[v][f] = sum_k u_k a[b_k][f] / den_v,        |xbar_q[v][f]| <= abar[v][f]    for all three quantities,

and why that is enough: per sample, the device's averaged plane differs from the restatement's by
  * the errors of the members' q, formed in the dtype: a weighted mean of what the constant 8 (nfreqs + 16) already pays for one row,
    so no more than that with abar in the place of a;
  * the ONE rounding of the quotient to the dtype: at most u abar, one unit out of the 8 nfreqs + 128 of the constant, of which a row's
    q (at most 8 units) and a dot product of 2 nfreqs terms (2 nfreqs units) use 2 nfreqs + 8: it sits inside;
  * a one-ulp change of the weights: w is read in the dtype on both sides and omega is a double on both sides, so u differs at most by
    the rounding of the product omega w in double, relative 2^-53; a relative change delta of every u moves the quotient by at most
    2 delta abar: 2 units of 2^-53, inside the constant in either dtype;
  * the sums in double over N members and the division: at most (N + 2) 2^-53 abar.  In fp32 that is below 2 u for every N the call
    admits (2^30) and sits inside the constant; in fp64 it grows with N and does NOT sit inside a constant: it is added to tau as its
    own term, (N_v + 2) 2^-53 abar, per set -- the constant 8 (nfreqs + 16) itself stays as it is."""
import numpy as np

import delay_fringe_ref as F
from delay_spectrum_ref import BOUND_CONSTANT, NAMES, UNIT, quantities

U64 = F.U64


def averaged(d, m, G, w, set_ptr, member_row, member_wgt=None, member_conj=None, weighting=0, calibrated=False):
    """``(xbar {q: [nsets, nfreqs] complex128}, mask [nsets, nfreqs] bool, abar [nsets, nfreqs], count [nsets])``: the averaged planes
    before the common mask, the sets' masks, the u-weighted mean of the members' per-sample sizes and the members per set.  Sums are
    taken sequentially, k ascending."""
    set_ptr, member_row = np.asarray(set_ptr, dtype=np.int64), np.asarray(member_row, dtype=np.int64)
    nsets, nf = len(set_ptr) - 1, np.asarray(w).shape[1]
    omega = np.ones(len(member_row)) if member_wgt is None else np.asarray(member_wgt, dtype=np.float64)
    cj = np.zeros(len(member_row), dtype=bool) if member_conj is None else np.asarray(member_conj) != 0
    xbar = {k: np.zeros((nsets, nf), dtype=np.complex128) for k in NAMES}
    mask, abar = np.zeros((nsets, nf), dtype=bool), np.zeros((nsets, nf))
    for v in range(nsets):
        ks = np.arange(set_ptr[v], set_ptr[v + 1])
        den, asum = np.zeros(nf), np.zeros(nf)
        acc = {k: np.zeros(nf, dtype=np.complex128) for k in NAMES}
        for k in ks:
            b = member_row[k]
            x, own, a = quantities(d[b : b + 1], m[b : b + 1], G[b : b + 1], np.asarray(w)[b : b + 1], calibrated)
            u = np.where(own[0], omega[k] * (np.asarray(w, dtype=np.float64)[b] if weighting else 1.0), 0.0)
            den = den + u
            asum = asum + u * a[0]
            for q in NAMES:
                acc[q] = acc[q] + u * (np.conj(x[q][0]) if cj[k] else x[q][0])
        mask[v] = den > 0
        safe = np.where(mask[v], den, 1.0)
        abar[v] = np.where(mask[v], asum / safe, 0.0)
        for q in NAMES:
            xbar[q][v] = np.where(mask[v], acc[q] / safe, 0.0)
    return xbar, mask, abar, np.diff(set_ptr)


def restated(d, m, G, w, op, norm_f, set_ptr, member_row, opt, member_wgt=None, member_conj=None, weighting=0, scale=None, calibrated=False,
             bin_of_group=None, nbins=0):
    """Everything the call returns, in float64, in the form of ``delay_fringe_ref.restated`` (``norm_grp``, ``per_group``, the bins,
    ``Y``, ``Z``, ``opt``, ``tau_per_unit``) plus ``tau_sum`` ``[T, ngroups, ndelays]``: the term of the double sums, to be multiplied
    by 2^-53 whatever the dtype, and ``common`` ``[ngroups, nfreqs]``."""
    op = np.asarray(op, dtype=np.complex128)
    opt = np.asarray(opt, dtype=np.complex128)
    T = opt.shape[0]
    xbar, mask, abar, count = averaged(d, m, G, w, set_ptr, member_row, member_wgt, member_conj, weighting, calibrated)
    nsets = len(mask)
    rows = np.arange(nsets).reshape(-1, T)
    ones, zeros, wv = np.ones_like(xbar["data"]), np.zeros_like(xbar["data"]), mask.astype(np.float64)
    out = F.restated(xbar["data"], xbar["model"], ones, wv, op, norm_f, rows, opt, scale, False, bin_of_group, nbins)
    res = F.restated(xbar["resid"], zeros, ones, wv, op, norm_f, rows, opt, scale, False, bin_of_group, nbins)
    for key in ("Y", "Z", "per_group"):
        out[key]["resid"] = res[key]["data"]
    if nbins:
        out["resid"] = res["data"]
    common = F.common_mask(wv, rows)
    sc = np.ones(rows.shape) if scale is None else np.asarray(scale, dtype=np.float64)
    aop = np.abs(op)
    tau, tsum = np.empty((T, len(rows), op.shape[1])), np.empty((T, len(rows), op.shape[1]))
    for t in range(T):
        a = np.where(common, abar[rows[:, t]], 0.0)
        tau[t] = np.abs(sc[:, t, None]) * BOUND_CONSTANT * (op.shape[0] + 16) * (a @ aop)
        tsum[t] = np.abs(sc[:, t, None]) * (count[rows[:, t], None] + 2.0) * (a @ aop)
    out["tau_per_unit"], out["tau_sum"], out["common"] = tau, tsum, common
    return out


def bound_plane(ref, name, dtype):
    """``delay_fringe_ref.bound_plane`` with abar in the place of a, and the double sums over the members added to tau."""
    unit = UNIT[np.dtype(dtype)]
    return F.bound_plane(dict(ref, tau_per_unit=ref["tau_per_unit"] + (U64 / unit) * ref["tau_sum"]), name, dtype)


def bound_ratio(P, ref, name, dtype):
    """The largest ratio of error to bound over the plane (0 / 0 counts as 0)."""
    err = np.abs(P - ref["per_group"][name]) * ref["norm_grp"][:, None, None]
    bound = bound_plane(ref, name, dtype)
    return float(np.max(np.divide(err, bound, out=np.zeros_like(err), where=err > 0)))


def singleton_sets(rows):
    """``(set_ptr, member_row)`` of sets that hold one member each: the rows ``[ngroups, T]`` of a fringe call."""
    rows = np.asarray(rows)
    return np.arange(rows.size + 1, dtype=np.int64), rows.ravel().astype(np.int32)


def sets_of(groups):
    """``(set_ptr, member_row, ngroups, T)`` from a list of groups, each a list of T lists of rows."""
    T = len(groups[0])
    assert all(len(g) == T for g in groups)
    sizes = [len(s) for g in groups for s in g]
    member_row = np.array([r for g in groups for s in g for r in s], dtype=np.int32)
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), member_row, len(groups), T
