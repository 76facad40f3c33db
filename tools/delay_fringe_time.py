#!/usr/bin/env python3
"""What cal_solver_delay_fringe_spectrum costs at HERA-350 (350 antennas, 61 075 baselines x 1024 channels, fp32) with 1024 delays:
``--slices`` slices in ONE solver (every slice holds the first's data plus independent noise), one group of ``--slices`` times per
baseline, ``--rates`` rates, all three quantities, binned only -- beside cal_solver_delay_spectrum over the same slices x nbls rows in the
same process, which runs the same matrix-core operations over planes of the same size and stages the operator as often.  What the new
call adds is the write and read of Y (the complex transform in double) and the transform along time.

Every call is bracketed by two HIP events (recorded on the null stream around the synchronous call; best of ``--reps`` after one
dropped round that allocates).  Timed through the C interface:
  delay_fringe_spectrum  the normal call: power_bin and count_bin of ``--nbins`` bins, no per-group output
  delay_spectrum         the normal call: power_bin and count_bin of slices x ``--nbins`` bins (a set per slice), no per-baseline output
``--host-rows N`` also runs the float64 NumPy restatement (tests/delay_fringe_ref.py) for the first N groups on ``--host-threads``
threads and scales the wall time to all groups (labelled as scaled; ``--layouts ""`` runs it alone).  Prints one JSON object; ``--out``
also writes it to a file."""
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


def slices_of(p, start, T, dtype, noise=1.0):
    """(the T-slice problem with its data, parameters of all slices): slice t > 0 is slice 0 plus independent noise of ``noise`` times
    the rms of the data, under the same flags.  The planes are formed in ``dtype`` (eight slices of HERA-350 in float64 are 4 GB each)."""
    from calamity_amd import batched

    rng = np.random.default_rng(2)
    sub, _, _ = batched.replicate_slices(p, T)
    sigma = noise * float(np.sqrt(np.mean(np.square(p.data_r)) + np.mean(np.square(p.data_i)))) / np.sqrt(2.0)
    d_r, d_i = np.asarray(p.data_r, dtype=dtype), np.asarray(p.data_i, dtype=dtype)
    draw = lambda: (sigma * rng.standard_normal(d_r.shape, dtype=np.float32)).astype(dtype)  # noqa: E731
    sub.data_r = np.concatenate([d_r] + [d_r + draw() for _ in range(T - 1)])
    sub.data_i = np.concatenate([d_i] + [d_i + draw() for _ in range(T - 1)])
    sub.wgts = np.tile(np.asarray(p.wgts, dtype=dtype), (T, 1))
    g_r = 1.0 + 0.05 * rng.standard_normal((T * p.nants, p.nfreqs))
    g_i = 0.05 * rng.standard_normal((T * p.nants, p.nfreqs))
    return sub, dict(g_r=g_r, g_i=g_i, c_r=np.tile(start["c_r"], T), c_i=np.tile(start["c_i"], T))


def measure(sub, params, nb, T, nrates, dtype, layout, reps, ev, op, norm_f, nbins):
    from calamity_amd import _lib, modeling
    from calamity_amd.solver import HipFitSolver

    s = HipFitSolver(dtype=dtype)
    s.set_problem(sub, layout=layout)
    s.set_data(sub.data_r, sub.data_i, sub.wgts)
    s.set_params(params["g_r"], params["g_i"], params["c_r"], params["c_i"])
    nd = op.shape[1]
    op_r, op_i = (np.ascontiguousarray(a, dtype=dtype) for a in (op.real, op.imag))
    rows = np.ascontiguousarray(np.stack([t * nb + np.arange(nb) for t in range(T)], axis=1), dtype=np.int32)
    opt = modeling.fringe_rate_transform(T, 10.7)[0][:, :nrates]
    opt_r, opt_i = np.ascontiguousarray(opt.real), np.ascontiguousarray(opt.imag)
    gbins = (np.arange(nb) % nbins).astype(np.int32)
    rbins = np.concatenate([t * nbins + gbins for t in range(T)]).astype(np.int32)
    f_bin, c_bin, norm_grp = np.empty((3, nbins, nrates, nd)), np.empty(nbins), np.empty(nb)
    p_bin, c2_bin, norm_bl = np.empty((3, T * nbins, nd)), np.empty(T * nbins), np.empty(T * nb)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    df = _lib.DelayFringeDesc(nd, 7, 0, nb, T, nrates, rows.ctypes.data, None, nbins, gbins.ctypes.data, op_r.ctypes.data, op_i.ctypes.data, norm_f.ctypes.data,
                              opt_r.ctypes.data, opt_i.ctypes.data)
    ds = _lib.DelaySpectrumDesc(nd, 7, 0, T * nbins, rbins.ctypes.data, op_r.ctypes.data, op_i.ctypes.data, norm_f.ctypes.data)
    forms = {"delay_fringe_spectrum": lambda: _lib.check(s._lib.cal_solver_delay_fringe_spectrum(s._h, C.byref(df), None, None, None, ptr(norm_grp), ptr(f_bin),
                                                                                                  ptr(c_bin))),
             "delay_spectrum": lambda: _lib.check(s._lib.cal_solver_delay_spectrum(s._h, C.byref(ds), None, None, None, ptr(norm_bl), ptr(p_bin), ptr(c2_bin)))}
    ms = {k: [] for k in forms}
    for _ in range(reps + 1):  # (the first round allocates: dropped)
        for k, fn in forms.items():
            ms[k].append(ev.time_ms(fn)[0])
    best = {k: min(v[1:]) for k, v in ms.items()}
    flops = 3 * 8.0 * T * nb * sub.nfreqs * nd  # complex product of [T nb, F] by [F, nd], three quantities: the same for both calls
    count = np.where(c_bin > 0, c_bin, 1.0)[None, :, None, None]
    out = dict(layout=layout, ngroups=int(nb), ntimes=T, nrates=nrates, ms_best={k: round(v, 3) for k, v in best.items()},
               ms_all={k: [round(x, 3) for x in v[1:]] for k, v in ms.items()},
               fringe_over_spectrum=round(best["delay_fringe_spectrum"] / best["delay_spectrum"], 3),
               tflops={k: round(flops / (v * 1e-3) / 1e12, 2) for k, v in best.items()}, groups_counted=float(c_bin.sum()),
               y_bytes=int(2 * 3 * T * nb * nd * 16), time_flops=float(3 * 8.0 * T * nrates * nb * nd),
               # solver units, residual: the mean power per rate (the first is the most negative rate of the grid)
               resid_mean_per_rate=[float(v) for v in (f_bin / count)[2].mean(axis=(0, 2))], memory_bytes=int(s.memory_bytes()))
    s.close()
    return out


def host_route(sub, params, p0, nb, T, nrates, dtype, op, norm_f, rows, threads):
    """Wall time of the restatement for the first ``rows`` groups on ``threads`` threads (blocks of 64 groups), scaled to all groups.
    The inputs of those groups -- data, weights, G and the model rows ``A c`` -- are formed before the clock starts: the device call does
    not form them either (it reads the solver's planes and the model pass's output)."""
    from calamity_amd import modeling
    from delay_fringe_ref import restated

    rows = min(rows, nb)
    sel = np.concatenate([t * nb + np.arange(rows) for t in range(T)])
    cast = lambda a: np.asarray(a).astype(dtype).astype(np.float64)  # noqa: E731
    d = cast(sub.data_r[sel]) + 1j * cast(sub.data_i[sel])
    w = cast(sub.wgts[sel])
    na, nc, F = p0.nants, p0.ncoeffs, p0.nfreqs
    m = np.empty((T * rows, F), dtype=np.complex128)
    grp_of = np.repeat(np.arange(p0.ngrps), np.diff(p0.grp_bl_start))
    for t in range(T):
        c = cast(params["c_r"][t * nc : (t + 1) * nc]) + 1j * cast(params["c_i"][t * nc : (t + 1) * nc])
        for b in range(rows):
            g = grp_of[b]
            blk = cast(p0.basis[p0.grp_basis[g]][p0.bl_rowblk[b] * F : (p0.bl_rowblk[b] + 1) * F])
            m[t * rows + b] = blk @ c[p0.grp_coff[g] : p0.grp_coff[g + 1]]
    g = cast(params["g_r"]) + 1j * cast(params["g_i"])
    G = np.concatenate([g[t * na + p0.bl_ant0[:rows]] * np.conj(g[t * na + p0.bl_ant1[:rows]]) for t in range(T)])
    op64 = op.astype(np.complex128)
    opt = modeling.fringe_rate_transform(T, 10.7)[0][:, :nrates]

    def one(lo):
        hi = min(rows, lo + 64)
        idx = np.concatenate([t * rows + np.arange(lo, hi) for t in range(T)])
        n = hi - lo
        ref = restated(d[idx], m[idx], G[idx], w[idx], op64, norm_f, np.stack([t * n + np.arange(n) for t in range(T)], axis=1), opt)
        return float(ref["per_group"]["resid"].sum())

    t0 = time.perf_counter()
    with concurrent.futures.ThreadPoolExecutor(max_workers=threads) as pool:
        total = sum(pool.map(one, range(0, rows, 64)))
    wall = time.perf_counter() - t0
    return dict(groups_run=int(rows), threads=threads, wall_s=round(wall, 3), scaled_to_all_groups_s=round(wall * nb / rows, 1), checksum=total,
                note="scaled linearly from groups_run to all groups: not a measurement of the whole")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="hera350")
    ap.add_argument("--dtype", default="f32")
    ap.add_argument("--layouts", default="shared")
    ap.add_argument("--slices", type=int, default=8)
    ap.add_argument("--rates", type=int, default=8)
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
    T, nrates = args.slices, min(args.rates, args.slices)
    sub, params = slices_of(p, start, T, dtype)
    ev = Events() if args.layouts else None  # (--layouts "": the host route alone)
    result = dict(workload=f"{args.config} x {T} slices, {args.dtype}, {op.shape[1]} delays, {nrates} rates", nants=p.nants, nbls=p.nbls, nfreqs=p.nfreqs,
                  reps=args.reps,
                  runs=[measure(sub, params, p.nbls, T, nrates, dtype, layout, args.reps, ev, op, norm_f, args.nbins) for layout in args.layouts.split(",") if layout])
    if args.host_rows > 0:
        result["host"] = host_route(sub, params, p, p.nbls, T, nrates, dtype, op, norm_f, args.host_rows, args.host_threads)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
