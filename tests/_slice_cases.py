"""Sharded multi-slice problems whose ranks hold different kinds of share (helper of tests/test_gpu_shard_agreement.py and
tests/_exchange_rank.py).

One data-less single-slice problem of single-baseline (or, where asked, multi-baseline) fitting groups, one basis block per
group, and T slices of data, weights, gains, coefficients and sky on it.  ``distributed.partition_groups`` deals the groups in
block order round-robin, so with one block per group rank r of D holds groups r, r + D, ...: the vector counts are listed so
that the wide blocks land on the rank the case wants."""
import numpy as np

NANTS, NFREQS = 8, 200  # rows pad to 256 channels

# (nvecs, baselines per group) of every case's groups, in dealing order; per dtype where the two-pass threshold differs
# (the matrix-core multi-slice kernel takes at most 224 vectors; its one-pass regularised form 224 in fp32, 160 in fp64)
CASES = {
    # A: every block <= 160 vectors on every rank -> one regularised pass everywhere
    "uniform": {np.float32: [150, 40, 160, 100, 60, 20, 120, 80], np.float64: [150, 40, 160, 100, 60, 20, 120, 80]},
    # B: the wide blocks on rank 0 only (fp32: 230 vectors -> fused_multi_kernel; fp64: 200 and 170 -> matrix-core, two passes)
    "wide": {np.float32: [230, 40, 100, 150, 60, 20, 120, 80], np.float64: [200, 40, 170, 150, 60, 20, 120, 80]},
    # C: rank 0 the wide block, rank 1 a 3-baseline group (no alias table on that rank: no heads at all)
    "noheads": {np.float32: [230, (40, 3), 100, 150, 60, 20], np.float64: [200, (40, 3), 170, 150, 60, 20]},
    # F: three ranks, the wide blocks on rank 0 only (rank 0: groups 0, 3, 6; rank 1: 1, 4, 7; rank 2: 2, 5)
    "wide3": {np.float32: [230, 40, 100, 150, 60, 20, 120, 80], np.float64: [200, 40, 100, 150, 60, 20, 120, 80]},
    # D: dense path (SHARED layout), blocks <= 224
    "dense": {np.float32: [224, 40, 100, 150, 60, 20, 120, 80], np.float64: [224, 40, 100, 150, 60, 20, 120, 80]},
}


def build(case, dtype, nt=4, seed=0):
    """Returns dict(prob: data-less single-slice FitProblem, nt, parts: per-slice FitProblem with data, data_r / data_i / wgts:
    global [nt * nbls, nfreqs], g_r / g_i: global [nt * nants, nfreqs], c_r / c_i: global [nt * ncoeffs], prior_r / prior_i: [nt])."""
    from calamity_amd.problem import FitProblem

    spec = [g if isinstance(g, tuple) else (g, 1) for g in CASES[case][np.dtype(dtype).type]]
    rng = np.random.default_rng(seed)
    basis, a0, a1, start = [], [], [], [0]
    for nvec, nb in spec:
        basis.append(rng.standard_normal((NFREQS, nvec)) / np.sqrt(NFREQS))
        for _ in range(nb):
            i, j = rng.choice(NANTS, size=2, replace=False)
            a0.append(i)
            a1.append(j)
        start.append(start[-1] + nb)
    nbls = len(a0)
    geom = dict(nants=NANTS, nfreqs=NFREQS, basis=basis, grp_basis=np.arange(len(spec), dtype=np.int32),
                grp_bl_start=np.asarray(start, np.int32), bl_ant0=np.asarray(a0, np.int32), bl_ant1=np.asarray(a1, np.int32),
                bl_rowblk=np.zeros(nbls, np.int32))
    parts, priors = [], []
    for t in range(nt):
        w = rng.uniform(0.0, 1.0, size=(nbls, NFREQS)) * (rng.random((nbls, NFREQS)) > 0.1)
        p = FitProblem(**geom, data_r=rng.standard_normal((nbls, NFREQS)), data_i=rng.standard_normal((nbls, NFREQS)),
                       wgts=w / (w.sum() * nt))
        p.sky_r, p.sky_i = rng.standard_normal((nbls, NFREQS)), rng.standard_normal((nbls, NFREQS))
        st = dict(g_r=1.0 + 0.1 * rng.standard_normal((NANTS, NFREQS)), g_i=0.1 * rng.standard_normal((NANTS, NFREQS)),
                  c_r=rng.standard_normal(p.ncoeffs), c_i=rng.standard_normal(p.ncoeffs))
        parts.append((p, st))
        priors.append((float(np.sum(p.sky_r * p.wgts)), float(np.sum(p.sky_i * p.wgts))))
    prob = FitProblem(**geom, data_r=None, data_i=None, wgts=None)
    cat = lambda k, src: np.concatenate([getattr(p, k) if src == "p" else st[k] for p, st in parts])  # noqa: E731
    return dict(prob=prob, nt=nt, parts=parts, data_r=cat("data_r", "p"), data_i=cat("data_i", "p"), wgts=cat("wgts", "p"),
                g_r=cat("g_r", "s"), g_i=cat("g_i", "s"), c_r=cat("c_r", "s"), c_i=cat("c_i", "s"),
                prior_r=np.asarray([p[0] for p in priors]), prior_i=np.asarray([p[1] for p in priors]))


def shares(case_data, nranks):
    """The groups of every rank (SliceBatchFitter's partition)."""
    from calamity_amd import distributed

    p = case_data["prob"]
    return distributed.partition_groups(p.grp_nvec, p.grp_basis, np.diff(p.grp_bl_start), nranks)


def rank_share(case_data, rank, nranks):
    """(multi-slice FitProblem of rank's share, rows of the global per-sample arrays, indices of the global coefficients) --
    what SliceBatchFitter gives worker ``rank``."""
    from calamity_amd.batched import replicate_slices

    p, nt = case_data["prob"], case_data["nt"]
    sub, bl, cidx = replicate_slices(p, nt, shares(case_data, nranks)[rank])
    rows = np.concatenate([bl + t * p.nbls for t in range(nt)])
    cidx = np.concatenate([cidx + t * p.ncoeffs for t in range(nt)])
    return sub, rows, cidx


def per_step(pattern, nt, dtype):
    """The exchange of one train step, as (dtype str, count, op) calls: G = T * nants * 256 (row padding) gain reals per part."""
    G = nt * NANTS * 256
    gd, sd = np.dtype(dtype).str, np.dtype(np.float64).str
    return {"one_pass": [(gd, 3 * 2 * G, "sum"), (sd, 4 * nt, "sum")],
            "two_pass": [(sd, 4 * nt, "sum"), (gd, 3 * 2 * G, "sum"), (sd, 4 * nt, "sum")],
            "none": [(gd, 2 * G, "sum"), (sd, 4 * nt, "sum")],
            "dense_sum": [(sd, 4 * nt, "sum"), (gd, 2 * G, "sum"), (sd, 4 * nt, "sum")]}[pattern]
