#!/usr/bin/env python3
"""What cal_solver_solve_gain_coeffs costs and buys at HERA-350 (350 antennas, 61 075 baselines x 1024 channels, fp32, SHARED layout)
with the gains in the DPSS basis of ``--gain_max_dly`` ns (100 ns: K = 30): ONE call of 10 damped sweeps projected on the basis beside
10 descent steps of the same basis solver, in one process on one box.

Both start from unity gains (y = 0) with the coefficients at the truth (the situation of a fit against a sky model), without the
regulariser.  Reported: the wall time of each call (best of ``--reps``; both calls end in a stream synchronisation and move no
arrays to the host) and the chi-square (``eval_loss``) before and after each.  The descent is the optimizer of the command line's
defaults (Adamax, learning rate 1e-2).
Prints one JSON object; ``--out`` also writes it to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="hera350")
    ap.add_argument("--dtype", default="f32")
    ap.add_argument("--layout", default="shared")
    ap.add_argument("--sweeps", type=int, default=10)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--damping", type=float, default=0.5)
    ap.add_argument("--ridge", type=float, default=1e-6)
    ap.add_argument("--gain_max_dly", type=float, default=100.0)
    ap.add_argument("--optimizer", default="Adamax")
    ap.add_argument("--learning_rate", type=float, default=1e-2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from calamity_amd import modeling, synthetic
    from calamity_amd.solver import HipFitSolver

    dtype = np.float32 if args.dtype == "f32" else np.float64
    p, truth, start = synthetic.make_config(args.config)
    c_r, c_i = np.ascontiguousarray(truth["c"].real), np.ascontiguousarray(truth["c"].imag)
    s = HipFitSolver(dtype=dtype)
    s.set_problem(p, layout=args.layout)
    s.set_regularization(None)
    B = np.array(modeling.gain_dpss_basis(np.asarray(truth["freqs"], dtype=np.float64), args.gain_max_dly))
    s.set_gain_basis(B)

    def restart():
        s.set_params(start["g_r"], start["g_i"], c_r, c_i)  # g0 = these gains, y = 0
        s.set_optimizer(args.optimizer, learning_rate=args.learning_rate)

    restart()
    chisq = dict(start=s.eval_loss())
    wall = dict(solve_gain_coeffs=[], descent=[])
    for _ in range(args.reps + 1):  # (the first round allocates and captures: dropped)
        restart()
        t0 = time.perf_counter()
        counts = s.solve_gain_coeffs(args.sweeps, damping=args.damping, ridge=args.ridge)
        wall["solve_gain_coeffs"].append(time.perf_counter() - t0)
        chisq["after_sweeps"] = s.eval_loss()
        restart()
        t0 = time.perf_counter()
        s.run(args.steps, record=False, freeze_model=True)
        s.synchronize()
        wall["descent"].append(time.perf_counter() - t0)
        chisq["after_descent"] = s.eval_loss()
    itemsize = int(np.dtype(dtype).itemsize)
    result = dict(workload=f"{args.config}, {args.dtype}, layout {args.layout}", nants=p.nants, nbls=p.nbls, nfreqs=p.nfreqs,
                  kernel_path=s.timing_get()["kernel_path"], gain_max_dly_ns=args.gain_max_dly, gain_nvec=int(B.shape[1]), sweeps=args.sweeps,
                  damping=args.damping, ridge=args.ridge, steps=args.steps, last_sweep=counts,
                  descent=f"{args.optimizer}, learning rate {args.learning_rate}, gain coefficients only",
                  wall_ms={k: dict(best=1e3 * min(v[1:]), all=[round(1e3 * x, 3) for x in v[1:]]) for k, v in wall.items()},
                  chisq=chisq, chisq_ratio={k: chisq[k] / chisq["start"] for k in ("after_sweeps", "after_descent")},
                  # rows kernel: five planes in, three out, once per call; a sweep: three planes, each row read by both of its antennas;
                  # the Gram product of a sweep: 2 nfreqs kpad^2 flops per antenna row (an estimate, not a measurement)
                  bytes_moved=dict(rows_kernel_once=itemsize * 8 * p.nbls * p.nfreqs,
                                   per_sweep=itemsize * 6 * p.nbls * p.nfreqs + 24 * p.nants * p.nfreqs),
                  gram_flops_per_sweep=2.0 * p.nfreqs * (8 * ((B.shape[1] + 7) // 8)) ** 2 * p.nants)
    s.close()
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
