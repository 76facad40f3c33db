#!/usr/bin/env python3
"""What cal_solver_robust_weights costs at HERA-350 (350 antennas, 61 075 baselines x 1024 channels, fp32, SHARED layout) beside
cal_solver_fit_quality of the same solver, which runs the same model pass and a rows kernel of the same loads, in one process.

Two kinds of numbers:
  * wall time of the two Python calls (best of ``--reps``).  Both end in small downloads (2 x 61 075 doubles against 6 MB);
  * device time of every kernel of the two calls, out of the kernel statistics of a run of this script under
    ``rocprofv3 --kernel-trace --stats --output-format csv -- python tools/robust_weights_bench.py`` (``--stats-csv`` reads them back).
Prints one JSON object; ``--out`` also writes it to a file (a measured run belongs in ``profiles/robust_weights_hera350_f32.json``)."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("fused_basis_kernel", "fused_dense", "fused_group_kernel", "robust_rows_kernel", "quality_rows_kernel", "quality_ant_kernel")


def kernel_stats(path):
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            for k in KERNELS:
                if k in name:
                    out.setdefault(k, []).append(dict(calls=int(row["Calls"]), average_us=float(row["AverageNs"]) / 1e3,
                                                      min_us=float(row["MinNs"]) / 1e3, max_us=float(row["MaxNs"]) / 1e3, name=name[:120]))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="hera350")
    ap.add_argument("--dtype", default="f32")
    ap.add_argument("--layout", default="shared")
    ap.add_argument("--kind", default="huber")
    ap.add_argument("--threshold", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stats-csv", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    result = dict(workload=f"{args.config}, {args.dtype}, layout {args.layout}, {args.kind} k = {args.threshold}")
    if args.stats_csv:
        result["kernel_stats"] = kernel_stats(args.stats_csv)
    else:
        from calamity_amd import synthetic
        from calamity_amd.solver import HipFitSolver

        dtype = np.float32 if args.dtype == "f32" else np.float64
        p, _, start = synthetic.make_config(args.config)
        rng = np.random.default_rng(2)
        g_r = 1.0 + 0.05 * rng.standard_normal((p.nants, p.nfreqs))
        g_i = 0.05 * rng.standard_normal((p.nants, p.nfreqs))
        s = HipFitSolver(dtype=dtype)
        s.set_problem(p, layout=args.layout)
        s.set_params(g_r, g_i, start["c_r"], start["c_i"])
        calls = (("robust_weights", lambda: s.robust_weights(kind=args.kind, threshold=args.threshold)), ("fit_quality", s.fit_quality))
        wall = {name: [] for name, _ in calls}
        for _ in range(args.reps + 1):  # (the first round allocates: dropped)
            for name, fn in calls:
                t0 = time.perf_counter()
                out = fn()
                wall[name].append(time.perf_counter() - t0)
        out = s.robust_weights(kind=args.kind, threshold=args.threshold)
        size = int(np.dtype(dtype).itemsize)
        result.update(nants=p.nants, nbls=p.nbls, nfreqs=p.nfreqs, kernel_path=s.timing_get()["kernel_path"],
                      wall_ms={k: dict(best=1e3 * min(v[1:]), all=[round(1e3 * x, 3) for x in v[1:]]) for k, v in wall.items()},
                      downweighted=float(out["ndown_bl"].sum()), samples=int(np.sum(s.get_weights(1) > 0)),
                      median_scale=float(np.median(out["scale_bl"])),
                      # five planes in (model_r, model_i, data_r, data_i, w0) and one out; w0 is read a second time when the weights are
                      # written (the row was loaded by the same wave a moment before: expected from the caches); the two antennas' gain
                      # rows per baseline, 3 MB of gains in all: from the caches; the median rounds run on LDS
                      bytes_moved=dict(rows_kernel=size * 6 * p.nbls * p.nfreqs, rows_kernel_w0_second_read=size * p.nbls * p.nfreqs,
                                       rows_kernel_gain_reads=size * 4 * p.nbls * p.nfreqs))
        s.close()
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
