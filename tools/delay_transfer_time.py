#!/usr/bin/env python3
"""What cal_solver_delay_transfer costs at HERA-350 (350 antennas, 61 075 baselines x 1024 channels, fp32) with 1024 delays, SHARED and
STREAM layout in one process, beside the floor it shares with cal_solver_fit_errors.

Every call is bracketed by two HIP events (recorded on the null stream around the synchronous call; best of ``--reps`` after one
dropped round that allocates).  Timed through the C interface:
  delay_transfer    the normal call: absorbed_bin and count_bin of ``--nbins`` bins, no per-baseline output
  coeff_var         cal_solver_fit_errors with coeff_var alone: model pass, q, Gram, factorisation and W = L^-1 -- the floor both share
The difference is the share of dtransfer_basis_kernel and dtransfer_power_kernel (plus the zero fill of S and the bin sums); its rate
is quoted on the power kernel's 4 F ndelays sum(nvec) flops (real x complex) -- the basis kernel's F sum(nvec^2) come on top and are
reported beside it.  ``--host-rows N`` also runs the float64 NumPy restatement (tests/delay_transfer_ref.py) for the first N baseline
rows on ``--host-threads`` threads and scales the wall time to all rows (labelled as scaled).  Prints one JSON object; ``--out`` also
writes it to a file."""
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


def measure(p, start, dtype, layout, reps, ev, op, nbins):
    from calamity_amd import _lib
    from calamity_amd.solver import HipFitSolver

    rng = np.random.default_rng(2)
    s = HipFitSolver(dtype=dtype)
    s.set_problem(p, layout=layout)
    s.set_params(1.0 + 0.05 * rng.standard_normal((p.nants, p.nfreqs)), 0.05 * rng.standard_normal((p.nants, p.nfreqs)), start["c_r"], start["c_i"])
    nd = op.shape[1]
    op_r, op_i = (np.ascontiguousarray(a, dtype=dtype) for a in (op.real, op.imag))
    bins = (np.arange(p.nbls) % nbins).astype(np.int32)
    a_bin, c_bin, cv = np.empty((nbins, nd)), np.empty(nbins), np.empty(p.ncoeffs)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    cnt, cnt_fe = _lib.FitErrorsCounts(), _lib.FitErrorsCounts()
    d = _lib.DelayTransferDesc(nd, 0, nbins, bins.ctypes.data, op_r.ctypes.data, op_i.ctypes.data, 1e-6)
    forms = {"delay_transfer": lambda: _lib.check(s._lib.cal_solver_delay_transfer(s._h, C.byref(d), None, None, None, None, ptr(a_bin), ptr(c_bin), C.byref(cnt))),
             "coeff_var": lambda: _lib.check(s._lib.cal_solver_fit_errors(s._h, 1e-6, ptr(cv), None, None, None, None, C.byref(cnt_fe)))}
    ms = {k: [] for k in forms}
    for _ in range(reps + 1):  # (the first round allocates: dropped)
        for k, fn in forms.items():
            ms[k].append(ev.time_ms(fn)[0])
    best = {k: min(v[1:]) for k, v in ms.items()}
    nvec = np.repeat(np.asarray(p.grp_nvec, dtype=np.float64), np.diff(p.grp_bl_start))  # per baseline row
    power_flops = 4.0 * p.nfreqs * nd * float(nvec.sum())
    basis_flops = float(p.nfreqs) * float(np.sum(np.asarray(p.grp_nvec, dtype=np.float64) ** 2))
    new_ms = best["delay_transfer"] - best["coeff_var"]
    transfer = 1.0 - a_bin / np.where(c_bin > 0, c_bin, 1.0)[:, None]
    out = dict(layout=layout, basis_folded=s.timing_get()["basis_folded"], nsolved=int(cnt.nsolved), nsingular=int(cnt.nsingular),
               ms_best={k: round(v, 3) for k, v in best.items()}, ms_all={k: [round(x, 3) for x in v[1:]] for k, v in ms.items()},
               new_kernels_ms=round(new_ms, 3), power_flops=power_flops, basis_flops=basis_flops,
               new_kernels_tflops_on_power_flops=power_flops / (new_ms * 1e-3) / 1e12 if new_ms > 0 else None,
               transfer_min=float(transfer.min()), transfer_median=float(np.median(transfer)), memory_bytes=int(s.memory_bytes()))
    s.close()
    return out


def host_route(p, start, dtype, op, rows, threads):
    """Wall time of the restatement for the groups of the first ``rows`` baseline rows on ``threads`` threads, scaled to all rows."""
    from delay_transfer_ref import core, samples

    rng = np.random.default_rng(2)
    g = (1.0 + 0.05 * rng.standard_normal((p.nants, p.nfreqs))) + 1j * 0.05 * rng.standard_normal((p.nants, p.nfreqs))
    ngrps = int(np.searchsorted(p.grp_bl_start, rows, side="left"))
    nrows = int(p.grp_bl_start[ngrps])
    q, s, v, _ = samples(g, p.bl_ant0[:nrows], p.bl_ant1[:nrows], p.wgts[:nrows], dtype, False)
    F = p.nfreqs
    op64 = op.astype(np.complex128)

    def one(grp):
        b0, b1 = int(p.grp_bl_start[grp]), int(p.grp_bl_start[grp + 1])
        blk = np.asarray(p.basis[p.grp_basis[grp]], dtype=np.float64)
        A = [blk[p.bl_rowblk[b] * F : (p.bl_rowblk[b] + 1) * F] for b in range(b0, b1)]
        return core(A, q[b0:b1], s[b0:b1], v[b0:b1], op64, 1e-6) is not None

    t0 = time.perf_counter()
    with concurrent.futures.ThreadPoolExecutor(max_workers=threads) as pool:
        done = sum(pool.map(one, range(ngrps)))
    wall = time.perf_counter() - t0
    return dict(rows_run=nrows, groups_run=ngrps, groups_solved=int(done), threads=threads, wall_s=round(wall, 3),
                scaled_to_all_rows_s=round(wall * p.nbls / nrows, 1), note="scaled linearly from rows_run to all rows: not a measurement of the whole")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="hera350")
    ap.add_argument("--dtype", default="f32")
    ap.add_argument("--layouts", default="shared,stream")
    ap.add_argument("--ndelays", type=int, default=1024)
    ap.add_argument("--nbins", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-rows", type=int, default=0)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from calamity_amd import _lib, modeling, synthetic

    _lib.load()
    dtype = np.float32 if args.dtype == "f32" else np.float64
    p, _, start = synthetic.make_config(args.config)
    full, _, _ = modeling.delay_transform(150e6 + 100e3 * np.arange(p.nfreqs))
    lo = (p.nfreqs - min(args.ndelays, p.nfreqs)) // 2
    op = np.ascontiguousarray(full[:, lo : lo + min(args.ndelays, p.nfreqs)])
    ev = Events()
    result = dict(workload=f"{args.config}, {args.dtype}, {op.shape[1]} delays", nants=p.nants, nbls=p.nbls, nfreqs=p.nfreqs, reps=args.reps,
                  runs=[measure(p, start, dtype, layout, args.reps, ev, op, args.nbins) for layout in args.layouts.split(",")])
    if args.host_rows > 0:
        result["host"] = host_route(p, start, dtype, op, args.host_rows, args.host_threads)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
