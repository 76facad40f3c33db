#!/usr/bin/env python3
"""What cal_solver_fix_degeneracies costs at HERA-350 (350 antennas, 61 075 baselines x 1024 channels, fp32, one slice, per-channel mode,
6 iterations, reference gains given) beside the HOST ROUTE on the same box: cal_solver_model read back, then the same estimate in NumPy on
the CPUs the job is given (z0, Q, H and the iterations over chunks of rows, one thread per chunk).

Two kinds of numbers:
  * wall time (best of ``--reps`` after a warm-up round that allocates) of the device call with every output, of the call without the
    transformed model rows (the estimate and the gains: no download as large as the data), and of the host route.  The library runs on a
    stream of its own and every call ends in a stream synchronisation, so the wall time of a call brackets its device work plus its
    uploads (the two reference planes) and downloads;
  * device time of every kernel of the call, out of the kernel statistics of a run of this script under
    ``rocprofv3 --kernel-trace --stats --output-format csv -- python tools/degeneracy_bench.py`` (``--stats-csv`` reads them back), and
    the sum kernel's rate over the bytes it has to read: two planes [nbls][nfreqs] per iteration (five in the first launch).
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

KERNELS = ("fused_basis_kernel", "fused_dense", "fused_group_kernel", "fused_multi_mfma", "degen_rows_kernel", "degen_sum_kernel", "degen_solve_kernel",
           "degen_phase_kernel", "degen_apply_gains_kernel", "degen_apply_rows_kernel", "pad_rows_kernel", "unpad_rows_kernel")


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


def host_route(s, p, ref, w, d, iters, ncpu):
    """The model read back, then z0, Q, H and the iterations in NumPy; the sums over rows chunk by chunk on ``ncpu`` threads."""
    m_r, m_i = s.model()
    step = max(1, -(-p.nbls // (4 * ncpu)))
    los = list(range(0, p.nbls, step))

    def prepare(lo):
        hi = min(p.nbls, lo + step)
        m = (m_r[lo:hi] + 1j * m_i[lo:hi]).astype(np.complex64)
        z0 = (w[lo:hi] * np.conj(m) * ref[lo:hi]).astype(np.complex128)
        a = np.abs(z0)
        dd = d[lo:hi]
        return z0, (w[lo:hi] * np.abs(m) ** 2).astype(np.float64).sum(0), np.stack([(a * (dd[:, i] * dd[:, j])[:, None]).sum(0) for i, j in ((0, 0), (0, 1), (1, 1))])

    with concurrent.futures.ThreadPoolExecutor(ncpu) as pool:
        parts = list(pool.map(prepare, los))
        Q = sum(x[1] for x in parts)
        H = sum(x[2] for x in parts)
        det = H[0] * H[2] - H[1] ** 2
        phi = np.zeros((p.nfreqs, 2))

        def sums(args):
            lo, z0 = args
            dd = d[lo:lo + len(z0)]
            z = z0 * np.exp(-1j * (dd @ phi.T))
            return (z.imag * dd[:, :1]).sum(0), (z.imag * dd[:, 1:]).sum(0), z.real.sum(0)

        for it in range(iters + 1):
            got = list(pool.map(sums, zip(los, (x[0] for x in parts))))
            qe, qn, sre = (sum(g[k] for g in got) for k in range(3))
            if it < iters:
                phi = phi + np.stack([(H[2] * qe - H[1] * qn) / det, (H[0] * qn - H[1] * qe) / det], axis=1)
    return 0.5 * np.log(np.maximum(sre, 0) / Q), phi


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="hera350")
    ap.add_argument("--dtype", default="f32")
    ap.add_argument("--layout", default="shared")
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--cpus", type=int, default=16)
    ap.add_argument("--device-only", action="store_true", help="skip the host route")
    ap.add_argument("--stats-csv", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    result = dict(workload=f"{args.config}, {args.dtype}, one slice, per-channel mode, {args.iters} iterations")
    if args.stats_csv:
        result["kernel_stats"] = kernel_stats(args.stats_csv)
    else:
        from calamity_amd import synthetic
        from calamity_amd.solver import HipFitSolver

        dtype = np.float32 if args.dtype == "f32" else np.float64
        p, _, start = synthetic.make_config(args.config)
        nants = synthetic.CONFIGS[args.config][0]
        rng = np.random.default_rng(2)
        g_r = (1.0 + 0.05 * rng.standard_normal((p.nants, p.nfreqs))).astype(dtype)
        g_i = (0.05 * rng.standard_normal((p.nants, p.nfreqs))).astype(dtype)
        pos = synthetic.hex_positions(nants)[:, :2].copy()
        d = pos[p.bl_ant0] - pos[p.bl_ant1]
        s = HipFitSolver(dtype=dtype)
        s.set_problem(p, layout=args.layout)
        s.set_params(g_r, g_i, start["c_r"], start["c_i"])
        m_r, m_i = s.model()
        phi = rng.normal(size=(p.nfreqs, 2))
        phi /= np.abs(d @ phi.T).max()  # 1 rad on the longest projected baseline
        ref = ((m_r + 1j * m_i) * np.exp(0.3 + 1j * (d @ phi.T))).astype(np.complex64 if args.dtype == "f32" else np.complex128)
        ref_r, ref_i = np.ascontiguousarray(ref.real), np.ascontiguousarray(ref.imag)
        w = np.asarray(p.wgts, dtype=dtype)
        del m_r, m_i
        plane_bytes = float(p.nbls) * p.nfreqs * np.dtype(dtype).itemsize
        result.update(nants=p.nants, nbls=p.nbls, nfreqs=p.nfreqs, plane_bytes=plane_bytes, sum_bytes_per_iteration=2 * plane_bytes,
                      sum_bytes_first_launch=5 * plane_bytes, memory_bytes_before=s.memory_bytes())
        wall = {"call": [], "call_without_model_rows": [], "model_readback": [], "host_route": []}
        for rep in range(args.reps + 1):  # (the first round allocates: dropped)
            t0 = time.perf_counter()
            s.fix_degeneracies(ref_r, ref_i, pos, iters=args.iters, gref_r=g_r, gref_i=g_i)
            wall["call"].append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            dev = s.fix_degeneracies(ref_r, ref_i, pos, iters=args.iters, gref_r=g_r, gref_i=g_i, return_model=False)
            wall["call_without_model_rows"].append(time.perf_counter() - t0)
            if args.device_only or rep > 2:
                continue
            t0 = time.perf_counter()
            s.model()
            wall["model_readback"].append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            eta, tilt = host_route(s, p, ref, w, d, args.iters, args.cpus)
            wall["host_route"].append(time.perf_counter() - t0)
        result.update(memory_bytes_after=s.memory_bytes(), kernel_path=s.timing_get()["kernel_path"], last_step_max=float(dev["last_step"].max()),
                      tilt_error_rad_on_longest=float(np.abs((dev["tilt"][0] - phi) @ d.T).max()),
                      wall_ms={k: dict(best=1e3 * min(v[1:]), all=[round(1e3 * x, 3) for x in v[1:]]) for k, v in wall.items() if len(v) > 1})
        if not args.device_only:
            result["device_against_host"] = dict(eta=float(np.abs(dev["eta"][0] - eta).max()), tilt=float(np.abs(dev["tilt"][0] - tilt).max()))
            result["host_over_device"] = result["wall_ms"]["host_route"]["best"] / result["wall_ms"]["call_without_model_rows"]["best"]
        s.close()
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
