#!/usr/bin/env python3
"""What cal_solver_solve_coeffs costs at HERA-350 (350 antennas, 61 075 baselines x 1024 channels, fp32), SHARED and STREAM layout
in one process, beside 10 descent steps of the same solver.

Two kinds of numbers:
  * wall time of one ``solve_coeffs`` call and of ``run(10, record=False)`` (best of ``--reps``; both end in a stream synchronisation
    and download nothing of size), with the chi-square (``fit_quality()["chisq_bl"].sum()``) at the start, after the solve and after
    the descent steps that follow it;
  * device time of every kernel, out of the kernel statistics of a run of this script under
    ``rocprofv3 --kernel-trace --stats --output-format csv -- python tools/coeff_solve_bench.py`` (``--stats-csv`` merges them into
    the JSON of an earlier ``--out``).
The Gram product is 2 F sum nvec^2 flops (lower triangle computed: half of it on the matrix cores); ``gram_tflops_of_full`` divides the
full count by the device time of coeff_gram_kernel.  Prints one JSON object; ``--out`` also writes it to a file."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("fused_basis_kernel", "fused_dense", "fused_group_kernel", "coeff_solve_rows_kernel", "coeff_gram_kernel", "coeff_chol_kernel")
FP32_MATRIX_PEAK_TFLOPS = 157.3


def kernel_stats(path):
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            for k in KERNELS:
                if k in name:
                    out.setdefault(k, []).append(dict(calls=int(row["Calls"]), total_ms=float(row["TotalDurationNs"]) / 1e6,
                                                      average_us=float(row["AverageNs"]) / 1e3, min_us=float(row["MinNs"]) / 1e3,
                                                      max_us=float(row["MaxNs"]) / 1e3, name=name[:120]))
    return out


def measure(p, start, dtype, layout, reps):
    from calamity_amd.solver import HipFitSolver

    rng = np.random.default_rng(2)
    g_r = 1.0 + 0.05 * rng.standard_normal((p.nants, p.nfreqs))
    g_i = 0.05 * rng.standard_normal((p.nants, p.nfreqs))
    s = HipFitSolver(dtype=dtype)
    s.set_problem(p, layout=layout)
    s.set_params(g_r, g_i, start["c_r"], start["c_i"])
    s.set_optimizer("Adamax", learning_rate=1e-3)
    chisq = dict(start=float(s.fit_quality()["chisq_bl"].sum()))
    wall = {"solve_coeffs": [], "ten_steps": []}
    counts = None
    for rep in range(reps + 1):  # (the first round allocates: dropped)
        s.set_params(c_r=start["c_r"], c_i=start["c_i"])
        t0 = time.perf_counter()
        counts = s.solve_coeffs()
        wall["solve_coeffs"].append(time.perf_counter() - t0)
        if rep == 0:
            chisq["after_one_solve"] = float(s.fit_quality()["chisq_bl"].sum())
        t0 = time.perf_counter()
        s.run(10, record=False)
        wall["ten_steps"].append(time.perf_counter() - t0)
        if rep == 0:
            chisq["after_ten_steps_more"] = float(s.fit_quality()["chisq_bl"].sum())
    nvec2 = float(np.sum(np.asarray(p.grp_nvec, dtype=np.float64) ** 2))
    out = dict(layout=layout, kernel_path=s.timing_get()["kernel_path"], basis_folded=s.timing_get()["basis_folded"], counts=counts, chisq=chisq,
               wall_ms={k: dict(best=1e3 * min(v[1:]), all=[round(1e3 * x, 3) for x in v[1:]]) for k, v in wall.items()},
               gram_flops_full=2.0 * p.nfreqs * nvec2, sum_nvec2=nvec2, max_nvec=int(np.max(p.grp_nvec)), memory_bytes=int(s.memory_bytes()))
    out["solve_over_one_step"] = out["wall_ms"]["solve_coeffs"]["best"] / (out["wall_ms"]["ten_steps"]["best"] / 10.0)
    s.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="hera350")
    ap.add_argument("--dtype", default="f32")
    ap.add_argument("--layouts", default="shared,stream")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--stats-csv", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.stats_csv:
        result = json.load(open(args.out)) if args.out and os.path.exists(args.out) else dict(workload=f"{args.config}, {args.dtype}")
        result["kernel_stats"] = kernel_stats(args.stats_csv)
        gram = result["kernel_stats"].get("coeff_gram_kernel")
        if gram and "runs" in result:
            # both layouts launch the same Gram work: flops of all timed launches over their device time
            calls = sum(g["calls"] for g in gram)
            total_s = sum(g["total_ms"] for g in gram) / 1e3
            nchunks_calls = calls  # (a call launches one Gram kernel per chunk)
            flops = sum(r["gram_flops_full"] * (args.reps + 1) for r in result["runs"])
            result["gram"] = dict(launches=nchunks_calls, device_ms_total=1e3 * total_s, tflops_of_full_count=flops / total_s / 1e12,
                                  fraction_of_fp32_matrix_peak=flops / total_s / 1e12 / FP32_MATRIX_PEAK_TFLOPS)
    else:
        from calamity_amd import synthetic

        dtype = np.float32 if args.dtype == "f32" else np.float64
        p, _, start = synthetic.make_config(args.config)
        result = dict(workload=f"{args.config}, {args.dtype}", nants=p.nants, nbls=p.nbls, nfreqs=p.nfreqs, reps=args.reps,
                      runs=[measure(p, start, dtype, layout, args.reps) for layout in args.layouts.split(",")])
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
