#!/usr/bin/env python3
"""What cal_solver_solve_gain_time_coeffs costs and buys: ``--ntimes`` (8) times of HERA-350 (350 antennas, 61 075 baselines x 1024
channels) as ONE joint fit, fp32, SHARED layout, the gains in the DPSS basis of ``--gain_max_dly`` ns (100 ns: K = 30) and the DPSS time
basis of ``--time_scale`` seconds on times 10.7 s apart (or, with ``--time_nvec L``, the Q of a QR of a seeded [T, L] normal matrix):
ONE call of 10 damped joint sweeps beside 10 descent steps of the same joint solver, in one process on one box.

Both start from unity gains (y = 0) with the coefficients at the truth (the situation of a fit against a sky model), without the
regulariser.  Reported: the wall time of each call (best of ``--reps``; both calls end in a stream synchronisation and move no arrays to
the host) and the chi-square (``eval_loss``) before and after each.  The descent is the optimizer of the command line's defaults
(Adamax, learning rate 1e-2).  ``--no_freq_basis`` measures the per-(antenna, channel) form.  The device time per launch of the kernels
comes from a kernel trace of this program.
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
    ap.add_argument("--ntimes", type=int, default=8)
    ap.add_argument("--sweeps", type=int, default=10)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--damping", type=float, default=0.5)
    ap.add_argument("--ridge", type=float, default=1e-6)
    ap.add_argument("--gain_max_dly", type=float, default=100.0)
    ap.add_argument("--time_scale", type=float, default=600.0)
    ap.add_argument("--time_nvec", type=int, default=0)
    ap.add_argument("--no_freq_basis", action="store_true")
    ap.add_argument("--optimizer", default="Adamax")
    ap.add_argument("--learning_rate", type=float, default=1e-2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from calamity_amd import modeling, synthetic
    from calamity_amd.batched import replicate_slices
    from calamity_amd.solver import HipFitSolver

    dtype = np.float32 if args.dtype == "f32" else np.float64
    T = args.ntimes
    p, truth, start = synthetic.make_config(args.config)
    big, _, _ = replicate_slices(p, T)
    big.nslices = 1  # one fit, one loop state: distributed.batch_time_slices(per_slice=False)
    tile = lambda a: np.tile(np.asarray(a, dtype=dtype), (T,) + (1,) * (np.ndim(a) - 1))  # noqa: E731
    c_r, c_i = tile(truth["c"].real), tile(truth["c"].imag)
    g_r, g_i = tile(start["g_r"]), tile(start["g_i"])
    s = HipFitSolver(dtype=dtype)
    s.set_problem(big, layout=args.layout)
    s.set_data(tile(p.data_r), tile(p.data_i), tile(p.wgts))
    s.set_regularization(None)
    B = None if args.no_freq_basis else np.array(modeling.gain_dpss_basis(np.asarray(truth["freqs"], dtype=np.float64), args.gain_max_dly))
    if args.time_nvec > 0:
        Bt = np.ascontiguousarray(np.linalg.qr(np.random.default_rng(1).standard_normal((T, args.time_nvec)))[0])
    else:
        Bt = np.array(modeling.gain_time_dpss_basis(2458101.25 + np.arange(T) * 10.7 / 86400.0, args.time_scale))
    s.set_params(g_r, g_i, c_r, c_i)
    s.set_gain_basis(B)
    s.set_gain_time_basis(Bt)

    def restart():
        s.set_params(g_r, g_i, c_r, c_i)  # g0 = these gains, y = 0
        s.set_optimizer(args.optimizer, learning_rate=args.learning_rate)

    restart()
    chisq = dict(start=s.eval_loss())
    wall = dict(solve_gain_time_coeffs=[], descent=[])
    for _ in range(args.reps + 1):  # (the first round allocates and captures: dropped)
        restart()
        t0 = time.perf_counter()
        counts = s.solve_gain_time_coeffs(args.sweeps, damping=args.damping, ridge=args.ridge)
        wall["solve_gain_time_coeffs"].append(time.perf_counter() - t0)
        chisq["after_sweeps"] = s.eval_loss()
        restart()
        t0 = time.perf_counter()
        s.run(args.steps, record=False, freeze_model=True)
        s.synchronize()
        wall["descent"].append(time.perf_counter() - t0)
        chisq["after_descent"] = s.eval_loss()
    L, K = int(Bt.shape[1]), None if B is None else int(B.shape[1])
    result = dict(workload=f"{T} times of {args.config} as one joint fit, {args.dtype}, layout {args.layout}", nants=p.nants, nbls=p.nbls, nfreqs=p.nfreqs,
                  ntimes=T, kernel_path=s.timing_get()["kernel_path"], gain_max_dly_ns=None if B is None else args.gain_max_dly, gain_nvec=K,
                  gain_time_nvec=L, system_size=L * (K or 1), sweeps=args.sweeps, damping=args.damping, ridge=args.ridge, steps=args.steps,
                  last_sweep=counts, descent=f"{args.optimizer}, learning rate {args.learning_rate}, gain coefficients only",
                  wall_ms={k: dict(best=1e3 * min(v[1:]), all=[round(1e3 * x, 3) for x in v[1:]]) for k, v in wall.items()},
                  chisq=chisq, chisq_ratio={k: chisq[k] / chisq["start"] for k in ("after_sweeps", "after_descent")},
                  # the Kronecker assembly of a sweep: 2 T (L (L + 1) / 2) K^2 flops per antenna, against 2 T nfreqs (L K)^2 / 2 for a direct
                  # Gram over the (t, f) index (operation counts, not measurements)
                  kron_flops_per_sweep=None if B is None else float(T) * L * (L + 1) * K * K * p.nants,
                  direct_gram_flops_per_sweep=None if B is None else float(T) * p.nfreqs * (L * K) ** 2 * p.nants)
    s.close()
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
