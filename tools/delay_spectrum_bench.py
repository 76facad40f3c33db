#!/usr/bin/env python3
"""What cal_solver_delay_spectrum costs at HERA-350 (350 antennas, 61 075 baselines x 1024 channels, fp32, one slice, data + model +
residual, binned by baseline length only) beside the HOST ROUTE on the same box: cal_solver_data_model read back, the residual,
taper, mask and numpy.fft on the CPUs the job is given, then the same bins.

Two kinds of numbers:
  * wall time of the device call and of the host route (best of ``--reps`` after a warm-up round that allocates).  The library runs on
    a stream of its own and every call ends in a stream synchronisation, so the wall time of the call brackets its device work plus
    the host side of the call (the operator image, the bins' lists, their uploads);
  * device time of every kernel of the call, out of the kernel statistics of a run of this script under
    ``rocprofv3 --kernel-trace --stats --output-format csv -- python tools/delay_spectrum_bench.py --device-only`` (``--stats-csv``
    reads them back): the transform kernel's share of the fp32 matrix peak on the useful flops 8 nwhat nbls nfreqs ndelays, and the
    model pass inside the call.
Prints one JSON object; ``--out`` also writes it to a file."""
import argparse
import concurrent.futures
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("fused_basis_kernel", "fused_dense", "fused_group_kernel", "fused_multi_mfma", "dspec_rows_kernel", "dspec_transform_kernel",
           "dspec_bin_kernel")
MFMA_F32_PEAK_TFLOPS = 157.3  # v_mfma_f32_16x16x4_f32, dense fp32 matrix peak of the MI355X


def kernel_stats(path):
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            for k in KERNELS:
                if k in name:
                    out.setdefault(k, []).append(dict(calls=int(row["Calls"]), total_ms=float(row["TotalDurationNs"]) / 1e6 if "TotalDurationNs" in row
                                                      else int(row["Calls"]) * float(row["AverageNs"]) / 1e6, average_us=float(row["AverageNs"]) / 1e3,
                                                      min_us=float(row["MinNs"]) / 1e3, max_us=float(row["MaxNs"]) / 1e3, name=name[:120]))
    return out


def host_route(s, p, taper, bins, nbins, ncpu):
    """data_model read back, then per chunk of rows: mask, the three quantities, taper, numpy.fft, |X|^2 / norm; bins summed."""
    gm_r, gm_i = s.data_model()
    mask = p.wgts != 0
    norm = mask.astype(np.float64) @ (taper * taper)
    nd = p.nfreqs
    power_bin = np.zeros((3, nbins, nd))

    def rows(lo, hi):
        d = (p.data_r[lo:hi] + 1j * p.data_i[lo:hi]).astype(np.complex64)
        gm = (gm_r[lo:hi] + 1j * gm_i[lo:hi]).astype(np.complex64)
        tm = (mask[lo:hi] * taper).astype(np.float32)
        out = np.zeros((3, nbins, nd))
        nb = np.where(norm[lo:hi] > 0, norm[lo:hi], np.inf)[:, None]
        for q, x in enumerate((d, gm, d - gm)):
            X = np.fft.fftshift(np.fft.fft(tm * x, axis=1), axes=1)
            np.add.at(out[q], bins[lo:hi], (X.real ** 2 + X.imag ** 2) / nb)
        return out

    step = max(1, -(-p.nbls // (4 * ncpu)))
    with concurrent.futures.ThreadPoolExecutor(ncpu) as pool:
        for part in pool.map(lambda lo: rows(lo, min(p.nbls, lo + step)), range(0, p.nbls, step)):
            power_bin += part
    return power_bin


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="hera350")
    ap.add_argument("--dtype", default="f32")
    ap.add_argument("--layouts", default="shared,stream")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpus", type=int, default=16)
    ap.add_argument("--device-only", action="store_true", help="skip the host route (a run under the profiler)")
    ap.add_argument("--stats-csv", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    result = dict(workload=f"{args.config}, {args.dtype}, data + model + residual, binned only")
    if args.stats_csv:
        result["kernel_stats"] = kernel_stats(args.stats_csv)
    else:
        from calamity_amd import calibration, modeling, synthetic
        from calamity_amd.solver import HipFitSolver

        dtype = np.float32 if args.dtype == "f32" else np.float64
        p, _, start = synthetic.make_config(args.config)
        nants, nfreqs, f0, df = synthetic.CONFIGS[args.config]
        rng = np.random.default_rng(2)
        g_r = 1.0 + 0.05 * rng.standard_normal((p.nants, p.nfreqs))
        g_i = 0.05 * rng.standard_normal((p.nants, p.nfreqs))
        op, norm_f, delays = modeling.delay_transform(f0 + df * np.arange(nfreqs))
        taper = modeling.delay_taper(nfreqs)
        pos = synthetic.hex_positions(nants)
        bins, bllen = calibration.baseline_length_bins(np.linalg.norm(pos[p.bl_ant0] - pos[p.bl_ant1], axis=1), 1.0)
        nbins = len(bllen)
        flops = 8.0 * 3 * p.nbls * nfreqs * op.shape[1]
        result.update(nants=p.nants, nbls=p.nbls, nfreqs=p.nfreqs, ndelays=int(op.shape[1]), nbins=int(nbins), useful_flops=flops, layouts={})
        for layout in args.layouts.split(","):
            s = HipFitSolver(dtype=dtype)
            s.set_problem(p, layout=layout)
            s.set_params(g_r, g_i, start["c_r"], start["c_i"])
            wall = {"delay_spectrum": [], "norm_only": [], "data_model": [], "host_route": [], "norm_only_after_host_route": []}
            for rep in range(args.reps + 1):  # (the first round allocates: dropped)
                t0 = time.perf_counter()
                dev = s.delay_spectrum(op, norm_f, bin_of_bl=bins, nbins=nbins)
                wall["delay_spectrum"].append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                s.delay_spectrum(op, norm_f)  # the model pass and the rows kernel alone: no transform, no bins
                wall["norm_only"].append(time.perf_counter() - t0)
                if args.device_only or rep > 2:  # (the host route takes seconds: three rounds of it)
                    continue
                t0 = time.perf_counter()
                s.data_model()
                wall["data_model"].append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                host = host_route(s, p, taper, bins, nbins, args.cpus)
                wall["host_route"].append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                s.delay_spectrum(op, norm_f)  # the first device work after the host route: what a call in that position pays beside its own work
                wall["norm_only_after_host_route"].append(time.perf_counter() - t0)
            entry = dict(kernel_path=s.timing_get()["kernel_path"],
                         wall_ms={k: dict(best=1e3 * min(v[1:]), all=[round(1e3 * x, 3) for x in v[1:]]) for k, v in wall.items() if len(v) > 1})
            if not args.device_only:
                got = np.stack([dev[k] for k in ("data", "model", "resid")])
                entry["device_against_host"] = float(np.max(np.abs(got - host)) / np.max(np.abs(host)))
                entry["host_over_device"] = entry["wall_ms"]["host_route"]["best"] / entry["wall_ms"]["delay_spectrum"]["best"]
            # what the transform alone can take at the most: the call minus the same call without transform and bins
            t_ms = entry["wall_ms"]["delay_spectrum"]["best"] - entry["wall_ms"]["norm_only"]["best"]
            entry["transform_and_bins_ms_by_difference"] = t_ms
            entry["fp32_matrix_peak_share_by_difference"] = flops / (t_ms * 1e-3) / 1e12 / MFMA_F32_PEAK_TFLOPS if t_ms > 0 else None
            result["layouts"][layout] = entry
            s.close()
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
