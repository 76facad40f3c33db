#!/usr/bin/env python3
"""What the modeling vectors of a jointly fitted group cost by the host route (dense covariance + numpy.linalg.eigh, as
simple_cov.yield_simple_multi_baseline_model_comps computes them by default) and by the device route (simple_cov.device_model_comps:
pivoted Cholesky, Gram, certificate and back-multiplication on the GPU, the k x k eigenproblems on the host), on the same inputs:

  n3072   6 baselines [14.6 (1 + 0.5 i), 2 (i mod 3), 0] x 512 channels of 200 kHz from 100 MHz
  n8192   8 such baselines x 1024 channels of 97.65625 kHz from 100 MHz (the host route is run once)
  batch8  eight groups like n8192 (baselines scaled by 1 + 0.01 g) in one device call under a 2 GiB scratch bound; the host route is
          not run for it (it is eight times n8192, one group after the other)

The host route is timed with the host clock (median of ``--host-reps`` runs for n3072).  The device route is timed with the host clock
around the whole call -- it ends in the download of V, behind a stream synchronise -- after one warm-up call per shape, median of
``--reps`` calls; its parts are the HIP events of the create call (factor: all step launches and the reads of the finished count; gram;
certificate), the host clock around the eigenproblems, and the HIP events around the back-multiplication launch.  What is left of the
call is uploads, downloads, allocation and Python.  Prints one JSON object and a table; ``--out`` also writes the JSON to a file."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PARTS = ("factor", "gram", "certificate", "eigh", "backmul")


def baselines(nbls, scale=1.0):
    return np.array([[14.6 * (1.0 + 0.5 * i) * scale, 2.0 * (i % 3), 0.0] for i in range(nbls)])


def time_host(blvecs, freqs, reps):
    from calamity_amd import simple_cov

    secs = []
    for _ in range(reps):
        t0 = time.perf_counter()
        vecs = simple_cov.yield_simple_multi_baseline_model_comps(blvecs, freqs)
        secs.append(time.perf_counter() - t0)
    return statistics.median(secs), vecs


def time_device(groups, freqs, reps, scratch_bytes):
    from calamity_amd import simple_cov

    simple_cov.device_model_comps(groups, freqs, device=0, scratch_bytes=scratch_bytes)  # warm-up: code objects, allocations
    runs = []
    for _ in range(reps):
        t0 = time.perf_counter()
        vectors, infos, times = simple_cov.device_model_comps(groups, freqs, device=0, scratch_bytes=scratch_bytes)
        times["call"] = time.perf_counter() - t0
        runs.append(times)
    med = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
    return med, vectors, infos


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--skip", default="", help="comma-separated cases to leave out (n3072, n8192, batch8)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from calamity_amd import _lib
    from calamity_amd.utils import usable_cores

    box = dict(device=_lib.device_info(0)["name"], host_cores=usable_cores())
    f512, f1024 = 100e6 + 200e3 * np.arange(512), 100e6 + 97656.25 * np.arange(1024)
    cases = {"n3072": ([baselines(6)], f512, args.host_reps, 0), "n8192": ([baselines(8)], f1024, 1, 0),
             "batch8": ([baselines(8, 1.0 + 0.01 * g) for g in range(8)], f1024, 0, 2 << 30)}
    rows = []
    for name, (groups, freqs, host_reps, bound) in cases.items():
        if name in args.skip.split(","):
            continue
        dev, vectors, infos = time_device(groups, freqs, args.reps, bound)
        row = dict(case=name, groups=len(groups), n=infos[0]["n"], k=[i["k"] for i in infos], kept=[i["kept"] for i in infos],
                   route=[i["route"] for i in infos], resid_fro=[i["resid_fro"] for i in infos], device_s={k: round(v, 5) for k, v in dev.items()},
                   eigh_share_of_call=round(dev["eigh"] / dev["call"], 3))
        if host_reps:
            host_s, host_vecs = time_host(groups[0], freqs, host_reps)
            row.update(host_s=round(host_s, 4), host_kept=host_vecs.shape[1], host_over_device=round(host_s / dev["call"], 2))
            if vectors[0] is not None:  # the same span: the largest part of a device vector outside the host's vectors
                row["defect_vs_host"] = float(np.max(np.linalg.norm(vectors[0] - host_vecs @ (host_vecs.T @ vectors[0]), axis=0)))
        rows.append(row)
    result = dict(box=box, reps=args.reps, rows=rows)
    text = json.dumps(result, indent=1)
    print(text)
    print("| case | n | k | kept | host route s | device route s | " + " | ".join(PARTS) + " | eigh share |")
    print("|---|---|---|---|---|---|" + "---|" * len(PARTS) + "---|")
    for r in rows:
        print(f"| {r['case']} | {r['groups']} x {r['n']} | {r['k'][0]} | {r['kept'][0]} | {r.get('host_s', 'not run')} | {r['device_s']['call']} | "
              + " | ".join(str(r["device_s"][p]) for p in PARTS) + f" | {r['eigh_share_of_call']} |")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
