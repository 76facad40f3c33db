#!/usr/bin/env python3
"""What cal_solver_delay_cross_spectrum costs at HERA-350 (350 antennas, 61 075 baselines x 1024 channels, fp32) with 1024 delays: two
slices in ONE solver (the second holds the first's data plus independent noise), one pair per baseline, all three quantities, both
statistics, binned -- beside cal_solver_delay_spectrum over the same 2 x npairs rows in the same process, which runs the same number
of matrix-core operations over planes of the same size and stages the operator as often.

Every call is bracketed by two HIP events (recorded on the null stream around the synchronous call; best of ``--reps`` after one
dropped round that allocates).  Timed through the C interface:
  delay_cross_spectrum   the normal call: cross_bin, diff_bin and count_bin of ``--nbins`` bins, no per-pair output
  delay_spectrum         the normal call: power_bin and count_bin of 2 x ``--nbins`` bins (a set per slice), no per-baseline output
``--host-rows N`` also runs the float64 NumPy restatement (tests/delay_cross_ref.py) for the first N pairs on ``--host-threads``
threads and scales the wall time to all pairs (labelled as scaled; ``--layouts ""`` runs it alone).  Prints one JSON object; ``--out`` also writes it to a file."""
import argparse
import concurrent.futures
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from fit_errors_time import Events  # noqa: E402


def two_slices(p, start, noise=1.0):
    """(the two-slice problem with its data, parameters of both slices): slice 1 is slice 0 plus independent noise of ``noise`` times
    the rms of the data, under the same flags."""
    from calamity_amd import batched

    rng = np.random.default_rng(2)
    sub, _, _ = batched.replicate_slices(p, 2)
    sigma = noise * float(np.sqrt(np.mean(np.square(p.data_r)) + np.mean(np.square(p.data_i)))) / np.sqrt(2.0)
    sub.data_r = np.concatenate([p.data_r, p.data_r + sigma * rng.standard_normal(p.data_r.shape)])
    sub.data_i = np.concatenate([p.data_i, p.data_i + sigma * rng.standard_normal(p.data_i.shape)])
    sub.wgts = np.concatenate([p.wgts, p.wgts])
    g_r = 1.0 + 0.05 * rng.standard_normal((2 * p.nants, p.nfreqs))
    g_i = 0.05 * rng.standard_normal((2 * p.nants, p.nfreqs))
    return sub, dict(g_r=g_r, g_i=g_i, c_r=np.tile(start["c_r"], 2), c_i=np.tile(start["c_i"], 2))


def measure(sub, params, nb, dtype, layout, reps, ev, op, norm_f, nbins):
    from calamity_amd import _lib
    from calamity_amd.solver import HipFitSolver

    s = HipFitSolver(dtype=dtype)
    s.set_problem(sub, layout=layout)
    s.set_data(sub.data_r, sub.data_i, sub.wgts)
    s.set_params(params["g_r"], params["g_i"], params["c_r"], params["c_i"])
    nd = op.shape[1]
    op_r, op_i = (np.ascontiguousarray(a, dtype=dtype) for a in (op.real, op.imag))
    pairs = np.ascontiguousarray(np.stack([np.arange(nb), nb + np.arange(nb)], axis=1), dtype=np.int32)
    pbins = (np.arange(nb) % nbins).astype(np.int32)
    rbins = np.concatenate([pbins, nbins + pbins]).astype(np.int32)
    x_bin, d_bin, c_bin = np.empty((3, nbins, nd)), np.empty((3, nbins, nd)), np.empty(nbins)
    p_bin, c2_bin, norm_bl, norm_pair = np.empty((3, 2 * nbins, nd)), np.empty(2 * nbins), np.empty(2 * nb), np.empty(nb)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    dc = _lib.DelayCrossDesc(nd, 7, 0, nb, pairs.ctypes.data, None, 3, nbins, pbins.ctypes.data, op_r.ctypes.data, op_i.ctypes.data, norm_f.ctypes.data)
    ds = _lib.DelaySpectrumDesc(nd, 7, 0, 2 * nbins, rbins.ctypes.data, op_r.ctypes.data, op_i.ctypes.data, norm_f.ctypes.data)
    forms = {"delay_cross_spectrum": lambda: _lib.check(s._lib.cal_solver_delay_cross_spectrum(s._h, C.byref(dc), None, None, None, None, ptr(norm_pair), ptr(x_bin),
                                                                                                ptr(d_bin), ptr(c_bin))),
             "delay_spectrum": lambda: _lib.check(s._lib.cal_solver_delay_spectrum(s._h, C.byref(ds), None, None, None, ptr(norm_bl), ptr(p_bin), ptr(c2_bin)))}
    ms = {k: [] for k in forms}
    for _ in range(reps + 1):  # (the first round allocates: dropped)
        for k, fn in forms.items():
            ms[k].append(ev.time_ms(fn)[0])
    best = {k: min(v[1:]) for k, v in ms.items()}
    flops = 3 * 8.0 * 2 * nb * sub.nfreqs * nd  # complex product of [2 nb, F] by [F, nd], three quantities: the same for both calls
    count = np.where(c_bin > 0, c_bin, 1.0)[None, :, None]
    auto = p_bin.reshape(3, 2, nbins, nd).sum(axis=1) / np.where(c2_bin.reshape(2, nbins).sum(axis=0) > 0, c2_bin.reshape(2, nbins).sum(axis=0), 1.0)[None, :, None]
    out = dict(layout=layout, npairs=int(nb), ms_best={k: round(v, 3) for k, v in best.items()}, ms_all={k: [round(x, 3) for x in v[1:]] for k, v in ms.items()},
               cross_over_spectrum=round(best["delay_cross_spectrum"] / best["delay_spectrum"], 3),
               tflops={k: round(flops / (v * 1e-3) / 1e12, 2) for k, v in best.items()}, pairs_counted=float(c_bin.sum()),
               # solver units, residual: the mean auto power of the two slices, the mean cross power, the mean half-difference power
               resid_mean_auto=float(auto[2].mean()), resid_mean_cross=float((x_bin / count)[2].mean()), resid_mean_noise=float((d_bin / count)[2].mean()),
               memory_bytes=int(s.memory_bytes()))
    s.close()
    return out


def host_route(sub, params, p0, nb, dtype, op, norm_f, rows, threads):
    """Wall time of the restatement for the first ``rows`` pairs on ``threads`` threads (blocks of 256 pairs), scaled to all pairs.  The
    inputs of those pairs -- data, weights, G and the model rows ``A c`` of their groups -- are formed before the clock starts: the
    device call does not form them either (it reads the solver's planes and the model pass's output)."""
    from delay_cross_ref import restated

    rows = min(rows, nb)
    sel = np.concatenate([np.arange(rows), nb + np.arange(rows)])
    cast = lambda a: np.asarray(a).astype(dtype).astype(np.float64)  # noqa: E731
    d = cast(sub.data_r[sel]) + 1j * cast(sub.data_i[sel])
    w = cast(sub.wgts[sel])
    na, nc, F = p0.nants, p0.ncoeffs, p0.nfreqs
    m = np.empty((2 * rows, F), dtype=np.complex128)
    grp_of = np.repeat(np.arange(p0.ngrps), np.diff(p0.grp_bl_start))
    for t in range(2):
        c = cast(params["c_r"][t * nc : (t + 1) * nc]) + 1j * cast(params["c_i"][t * nc : (t + 1) * nc])
        for b in range(rows):
            g = grp_of[b]
            blk = cast(p0.basis[p0.grp_basis[g]][p0.bl_rowblk[b] * F : (p0.bl_rowblk[b] + 1) * F])
            m[t * rows + b] = blk @ c[p0.grp_coff[g] : p0.grp_coff[g + 1]]
    g = cast(params["g_r"]) + 1j * cast(params["g_i"])
    G = np.concatenate([g[t * na + p0.bl_ant0[:rows]] * np.conj(g[t * na + p0.bl_ant1[:rows]]) for t in range(2)])
    op64 = op.astype(np.complex128)

    def one(lo):
        hi = min(rows, lo + 256)
        idx = np.concatenate([np.arange(lo, hi), rows + np.arange(lo, hi)])
        n = hi - lo
        ref = restated(d[idx], m[idx], G[idx], w[idx], op64, norm_f, np.stack([np.arange(n), n + np.arange(n)], axis=1))
        return float(ref["per_pair"]["cross"]["resid"].sum())

    t0 = time.perf_counter()
    with concurrent.futures.ThreadPoolExecutor(max_workers=threads) as pool:
        total = sum(pool.map(one, range(0, rows, 256)))
    wall = time.perf_counter() - t0
    return dict(pairs_run=int(rows), threads=threads, wall_s=round(wall, 3), scaled_to_all_pairs_s=round(wall * nb / rows, 1), checksum=total,
                note="scaled linearly from pairs_run to all pairs: not a measurement of the whole")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="hera350")
    ap.add_argument("--dtype", default="f32")
    ap.add_argument("--layouts", default="shared")
    ap.add_argument("--ndelays", type=int, default=1024)
    ap.add_argument("--nbins", type=int, default=64)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--host-rows", type=int, default=0)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from calamity_amd import _lib, modeling, synthetic

    _lib.load()
    dtype = np.float32 if args.dtype == "f32" else np.float64
    p, _, start = synthetic.make_config(args.config)
    full, norm_f, _ = modeling.delay_transform(150e6 + 100e3 * np.arange(p.nfreqs))
    lo = (p.nfreqs - min(args.ndelays, p.nfreqs)) // 2
    op = np.ascontiguousarray(full[:, lo : lo + min(args.ndelays, p.nfreqs)])
    norm_f = np.ascontiguousarray(norm_f, dtype=np.float64)
    sub, params = two_slices(p, start)
    ev = Events() if args.layouts else None  # (--layouts "": the host route alone)
    result = dict(workload=f"{args.config} x 2 slices, {args.dtype}, {op.shape[1]} delays", nants=p.nants, nbls=p.nbls, nfreqs=p.nfreqs, reps=args.reps,
                  runs=[measure(sub, params, p.nbls, dtype, layout, args.reps, ev, op, norm_f, args.nbins) for layout in args.layouts.split(",") if layout])
    if args.host_rows > 0:
        result["host"] = host_route(sub, params, p, p.nbls, dtype, op, norm_f, args.host_rows, args.host_threads)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
