"""The float64 NumPy restatement of cal_solver_delay_cross_spectrum (include/calamity_hip.h), shared by the cross-spectrum tests, built on
delay_spectrum_ref.quantities (imported, not copied).  For pair p = (b0, b1) with scales (a0, a1):

    mask_p = (w[b0] != 0) & (w[b1] != 0)          x_q[p][s] = mask_p q[b_s]          X_q[p][s] = x_q[p][s] @ op          Y_s = a_s X_q[p][s]
    norm_pair = mask_p @ norm_f      cross = Re(Y_0 conj(Y_1)) / norm_pair      diff = |Y_0 - Y_1|^2 / (2 norm_pair)      0 where norm_pair == 0
    cross_bin / diff_bin [q][n] = the sum, taken sequentially in ascending pair order, over the pairs of bin n with norm_pair > 0

and the bound the device is held to.  tau_s is delay_spectrum_ref's tau of side s taken under the common mask (its constant 8 and its
UNIT table as they stand), times |a_s|.  With Y_s = Y_s_ref + dY_s, |dY_s| <= tau_s:

    |cross - ref| norm  <= |Y0_ref| tau_1 + |Y1_ref| tau_0 + tau_0 tau_1
    |diff - ref| 2 norm <= (2 |Y0_ref - Y1_ref| + tau_0 + tau_1)(tau_0 + tau_1)

The scaling, the products and the division are in double on both sides."""
import numpy as np

from delay_spectrum_ref import BOUND_CONSTANT, NAMES, UNIT, quantities

STATS = ("cross", "diff")


def restated(d, m, G, w, op, norm_f, pairs, scale=None, calibrated=False, bin_of_pair=None, nbins=0):
    """Everything the call returns, in float64: ``norm_pair``, ``per_pair[stat][q]`` ``[npairs, ndelays]``, with bins ``[stat][q]``
    ``[nbins, ndelays]`` and ``count_bin``; plus ``Y[q]`` ``[2, npairs, ndelays]`` (the scaled transforms) and ``tau_per_unit``
    ``[2, npairs, ndelays]`` (multiply by ``UNIT[dtype]``)."""
    op = np.asarray(op, dtype=np.complex128)
    pairs = np.asarray(pairs).reshape(-1, 2)
    scale = np.ones(pairs.shape, dtype=np.float64) if scale is None else np.asarray(scale, dtype=np.float64)
    w = np.asarray(w)
    common = ((w[pairs[:, 0]] != 0) & (w[pairs[:, 1]] != 0)).astype(np.float64)
    norm_pair = common @ np.asarray(norm_f, dtype=np.float64)
    Y = {k: np.empty((2,) + (len(pairs), op.shape[1]), dtype=np.complex128) for k in NAMES}
    tau = np.empty((2, len(pairs), op.shape[1]))
    for s in range(2):
        rows = pairs[:, s]
        x, _, a = quantities(d[rows], m[rows], G[rows], common, calibrated)
        for k in NAMES:
            Y[k][s] = scale[:, s, None] * (x[k] @ op)
        tau[s] = np.abs(scale[:, s, None]) * BOUND_CONSTANT * (op.shape[0] + 16) * (a @ np.abs(op))
    live = norm_pair[:, None] != 0
    safe = np.where(norm_pair != 0, norm_pair, 1.0)[:, None]
    out = {"norm_pair": norm_pair, "Y": Y, "tau_per_unit": tau, "per_pair": {"cross": {}, "diff": {}}}
    for k in NAMES:
        out["per_pair"]["cross"][k] = np.where(live, (Y[k][0] * np.conj(Y[k][1])).real / safe, 0.0)
        out["per_pair"]["diff"][k] = np.where(live, np.abs(Y[k][0] - Y[k][1]) ** 2 / (2.0 * safe), 0.0)
    if nbins:
        for st in STATS:
            out[st] = bin_pairs(out["per_pair"][st], norm_pair, bin_of_pair, nbins)
        out["count_bin"] = out["cross"].pop("count_bin")
        out["diff"].pop("count_bin")
    return out


def bin_pairs(per_pair, norm_pair, bin_of_pair, nbins):
    """The bins of given per-pair planes ``{q: [npairs, ndelays]}``: sequential double sums in ascending pair order; ``count_bin``."""
    out = {k: np.zeros((nbins, v.shape[1])) for k, v in per_pair.items()}
    count = np.zeros(nbins)
    for p, n in enumerate(np.asarray(bin_of_pair)):
        if n < 0 or not norm_pair[p] > 0:
            continue
        count[n] += 1
        for k, v in per_pair.items():
            out[k][n] = out[k][n] + v[p]
    out["count_bin"] = count
    return out


def bound_ratio(P, ref, stat, name, dtype):
    """The largest ratio of error to bound over the plane (0 / 0 counts as 0)."""
    t0, t1 = UNIT[np.dtype(dtype)] * ref["tau_per_unit"]
    Y0, Y1 = ref["Y"][name]
    norm = ref["norm_pair"][:, None]
    if stat == "cross":
        err = np.abs(P - ref["per_pair"]["cross"][name]) * norm
        bound = np.abs(Y0) * t1 + np.abs(Y1) * t0 + t0 * t1
    else:
        err = np.abs(P - ref["per_pair"]["diff"][name]) * 2.0 * norm
        bound = (2.0 * np.abs(Y0 - Y1) + t0 + t1) * (t0 + t1)
    return float(np.max(np.divide(err, bound, out=np.zeros_like(err), where=err > 0)))
