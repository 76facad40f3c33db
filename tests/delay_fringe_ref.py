"""The float64 NumPy restatement of cal_solver_delay_fringe_spectrum (include/calamity_hip.h), shared by the delay / fringe-rate tests,
built on delay_spectrum_ref.quantities (imported, not copied).  For group g with rows rows[g][0 .. T) and scales a[g][t]:

    mask_g = AND over t of (w[rows[g][t]] != 0)      x_q[g][t] = mask_g q[rows[g][t]]      X_q[g][t] = x_q[g][t] @ op      Y_t = a[g][t] X_q[g][t]
    Z_q[g][r] = sum_t opt[t][r] Y_t  (sequentially, t ascending)      norm_grp = mask_g @ norm_f      power = |Z|^2 / norm_grp, 0 where norm_grp == 0
    power_bin[q][n] = the sum, taken sequentially in ascending group order, over the groups of bin n with norm_grp > 0

and the bound the device is held to.  tau_t is delay_spectrum_ref's tau of row t taken under the group's common mask (its constant 8 and
its UNIT table as they stand), times |a_t|: the form of delay_cross_ref.restated.  With Y_t = Y_t_ref + dY_t, |dY_t| <= tau_t, the sum
over time in double adds at most (T + 2) 2^-53 sum_t |opt[t][r]| |Y_t| (T products and additions, two more for the complex product):

    e                      = sum_t |opt[t][r]| tau_t + (T + 2) 2^-53 sum_t |opt[t][r]| |Y_t|
    |power - ref| norm_grp <= (2 |Z_ref| + e) e + 4 * 2^-53 |Z_ref|^2

(the last term: two squares, their sum and the division, in double on both sides)."""
import numpy as np

from delay_spectrum_ref import BOUND_CONSTANT, NAMES, UNIT, quantities

U64 = 2.0 ** -53


def common_mask(w, rows):
    """``[ngroups, nfreqs]`` bool: the channels unflagged in all T rows of every group."""
    w = np.asarray(w)
    rows = np.asarray(rows)
    return np.all(w[rows] != 0, axis=1)


def restated(d, m, G, w, op, norm_f, rows, opt, scale=None, calibrated=False, bin_of_group=None, nbins=0):
    """Everything the call returns, in float64: ``norm_grp``, ``per_group[q]`` ``[ngroups, nrates, ndelays]``, with bins ``[q]``
    ``[nbins, nrates, ndelays]`` and ``count_bin``; plus ``Y[q]`` ``[T, ngroups, ndelays]`` (the scaled transforms), ``Z[q]``
    ``[ngroups, nrates, ndelays]``, ``opt`` and ``tau_per_unit`` ``[T, ngroups, ndelays]`` (multiply by ``UNIT[dtype]``)."""
    op = np.asarray(op, dtype=np.complex128)
    opt = np.asarray(opt, dtype=np.complex128)
    rows = np.asarray(rows)
    ng, T = rows.shape
    assert opt.shape[0] == T
    nr, nd = opt.shape[1], op.shape[1]
    scale = np.ones(rows.shape, dtype=np.float64) if scale is None else np.asarray(scale, dtype=np.float64)
    common = common_mask(w, rows).astype(np.float64)
    norm_grp = common @ np.asarray(norm_f, dtype=np.float64)
    Y = {k: np.empty((T, ng, nd), dtype=np.complex128) for k in NAMES}
    tau = np.empty((T, ng, nd))
    for t in range(T):
        r = rows[:, t]
        x, _, a = quantities(d[r], m[r], G[r], common, calibrated)
        for k in NAMES:
            Y[k][t] = scale[:, t, None] * (x[k] @ op)
        tau[t] = np.abs(scale[:, t, None]) * BOUND_CONSTANT * (op.shape[0] + 16) * (a @ np.abs(op))
    live = (norm_grp != 0)[:, None, None]
    safe = np.where(norm_grp != 0, norm_grp, 1.0)[:, None, None]
    out = {"norm_grp": norm_grp, "Y": Y, "Z": {}, "opt": opt, "tau_per_unit": tau, "per_group": {}}
    for k in NAMES:
        Z = np.zeros((ng, nr, nd), dtype=np.complex128)
        for t in range(T):  # sequentially, t ascending
            Z = Z + opt[t][None, :, None] * Y[k][t][:, None, :]
        out["Z"][k] = Z
        out["per_group"][k] = np.where(live, (Z.real ** 2 + Z.imag ** 2) / safe, 0.0)
    if nbins:
        out.update(bin_groups(out["per_group"], norm_grp, bin_of_group, nbins))
    return out


def bin_groups(per_group, norm_grp, bin_of_group, nbins):
    """The bins of given per-group planes ``{q: [ngroups, nrates, ndelays]}``: sequential double sums in ascending group order; ``count_bin``."""
    out = {k: np.zeros((nbins,) + v.shape[1:]) for k, v in per_group.items()}
    count = np.zeros(nbins)
    for g, n in enumerate(np.asarray(bin_of_group)):
        if n < 0 or not norm_grp[g] > 0:
            continue
        count[n] += 1
        for k, v in per_group.items():
            out[k][n] = out[k][n] + v[g]
    out["count_bin"] = count
    return out


def bound_plane(ref, name, dtype):
    """The bound on ``|power - ref| norm_grp`` ``[ngroups, nrates, ndelays]``."""
    tau = UNIT[np.dtype(dtype)] * ref["tau_per_unit"]  # [T, ng, nd]
    aopt = np.abs(ref["opt"])  # [T, nr]
    T = aopt.shape[0]
    e = np.einsum("tr,tgk->grk", aopt, tau) + (T + 2) * U64 * np.einsum("tr,tgk->grk", aopt, np.abs(ref["Y"][name]))
    aZ = np.abs(ref["Z"][name])
    return (2.0 * aZ + e) * e + 4.0 * U64 * aZ ** 2


def bound_ratio(P, ref, name, dtype):
    """The largest ratio of error to bound over the plane (0 / 0 counts as 0)."""
    err = np.abs(P - ref["per_group"][name]) * ref["norm_grp"][:, None, None]
    bound = bound_plane(ref, name, dtype)
    return float(np.max(np.divide(err, bound, out=np.zeros_like(err), where=err > 0)))
