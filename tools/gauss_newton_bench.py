#!/usr/bin/env python3
"""What a joint Gauss-Newton step costs and buys at HERA-350 x 1024 channels, fp32, both layouts, in one process on one box.

After a warm-up round of every call that is timed (code objects, first allocations), each of the three moves starts from the same
parameters (unity gains, c0) and is timed by a host clock around work that ends in a device synchronise:

    one gauss_newton_step(ncg)              (lambda 1e-3)
    one round of alternating least squares  (solve_coeffs + 5 half-damped sweeps)
    100 descent steps                       (Adam, learning rate 1e-2)

with the chi-square after each (``eval_loss``), the iterations the step ran, whether it was accepted, and the device memory before and after
the step's buffers exist.  A second step (lambda 1e-4) follows the first, as in the two-step sequence of DESIGN section 3.16.

    python tools/gauss_newton_bench.py --measure [--layouts shared,stream] [--only-step]      # one process, one JSON line
    python tools/gauss_newton_bench.py --out profiles/gauss_newton_hera350_f32.json [--stats-csv shared=a_kernel_stats.csv stream=b_kernel_stats.csv]

``--only-step``: warm-up and the one step alone, for a separate ``rocprofv3 --kernel-trace --stats`` run; ``--stats-csv``: that run's
kernel statistics, from which the times of the gn_* kernels and of the passes they sit between are taken.  The child process runs under
its own time limit."""
import argparse
import csv
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def measure(layouts, ncg, only_step, config):
    sys.path.insert(0, HERE)
    import numpy as np

    from calamity_amd import synthetic
    from calamity_amd.solver import HipFitSolver

    p, _, start = synthetic.make_config(config)
    par = [np.asarray(start[k], dtype=np.float32) for k in ("g_r", "g_i", "c_r", "c_i")]
    out = dict(config=config, nants=int(p.nants), nfreqs=int(p.nfreqs), nbls=int(p.nbls), ncoeffs=int(p.ncoeffs), ncg=ncg)

    def timed(s, fn):
        s.synchronize()
        t0 = time.perf_counter()
        ret = fn()
        s.synchronize()
        return (time.perf_counter() - t0) * 1e3, ret

    for layout in layouts:
        s = HipFitSolver(dtype=np.float32)
        s.set_problem(p, layout=layout)

        def restart():
            s.set_params(*par)
            s.set_optimizer("Adam", learning_rate=1e-2)

        restart()
        res = dict(kernel_path=s.timing_get()["kernel_path"], basis_folded=s.timing_get()["basis_folded"], memory_bytes_before=s.memory_bytes(),
                   chisq_start=s.eval_loss())
        # warm-up: every call that is timed below, once
        s.gauss_newton_step(ncg=2)
        res["memory_bytes_after"] = s.memory_bytes()
        if not only_step:
            s.solve_coeffs()
            s.solve_gains(5, damping=0.5)
            s.run(20, record=False)
        restart()
        ms, st = timed(s, lambda: s.gauss_newton_step(ncg=ncg, lam=1e-3))
        res.update(step_ms=ms, step_cg_iters=int(st["cg_iters"][0]), step_accepted=bool(st["accepted"][0]), step_cg_residual=float(st["cg_residual"][0]),
                   chisq_after_step=float(st["loss_after"][0]))
        if not only_step:
            ms, st = timed(s, lambda: s.gauss_newton_step(ncg=ncg, lam=1e-4))
            res.update(second_step_ms=ms, second_step_cg_iters=int(st["cg_iters"][0]), second_step_accepted=bool(st["accepted"][0]),
                       chisq_after_two_steps=s.eval_loss())
            restart()
            ms, _ = timed(s, lambda: (s.solve_coeffs(), s.solve_gains(5, damping=0.5)))
            res.update(als_round_ms=ms, chisq_after_als_round=s.eval_loss())
            restart()
            ms, _ = timed(s, lambda: s.solve_coeffs())
            res["solve_coeffs_ms"] = ms
            restart()
            ms, _ = timed(s, lambda: s.run(100, record=False))
            res.update(descent_100_steps_ms=ms, chisq_after_100_descent_steps=s.eval_loss())
            restart()
            ms, _ = timed(s, lambda: s.eval_grads())
            res["eval_grads_with_download_ms"] = ms
        s.close()
        out[layout] = res
        print(f"# {layout}: {res}", file=sys.stderr, flush=True)
    print(json.dumps(out), flush=True)


def kernel_stats(path):
    """Calls, average and total duration of the step's own kernels and of the passes out of rocprofv3's kernel statistics."""
    out, total = {}, 0.0
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            total += float(row["TotalDurationNs"])
            short = name.split("(")[0].replace("void ", "").replace("calk::", "").strip()  # (the template arguments tell the passes apart)
            e = out.setdefault(short, dict(calls=0, total_ms=0.0))
            e["calls"] += int(row["Calls"])
            e["total_ms"] += float(row["TotalDurationNs"]) / 1e6
    for e in out.values():
        e["average_us"] = e["total_ms"] * 1e3 / max(e["calls"], 1)
        e["percent"] = 100.0 * e["total_ms"] * 1e6 / max(total, 1.0)
    own = sum(e["total_ms"] for k, e in out.items() if k.startswith("gn_"))
    return dict(kernels=out, total_ms=total / 1e6, gn_kernels_ms=own, gn_kernels_percent=100.0 * own * 1e6 / max(total, 1.0))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--measure", action="store_true")
    ap.add_argument("--only-step", action="store_true")
    ap.add_argument("--layouts", default="shared,stream")
    ap.add_argument("--config", default="hera350")
    ap.add_argument("--ncg", type=int, default=20)
    ap.add_argument("--out")
    ap.add_argument("--stats-csv", nargs="*", default=[])
    ap.add_argument("--child-timeout", type=int, default=540)
    args = ap.parse_args()
    if args.measure:
        return measure(args.layouts.split(","), args.ncg, args.only_step, args.config)
    cmd = [sys.executable, os.path.abspath(__file__), "--measure", "--layouts", args.layouts, "--ncg", str(args.ncg), "--config", args.config]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=args.child_timeout, check=True, text=True)
    result = json.loads(r.stdout.strip().splitlines()[-1])
    result["timing"] = "host clock around calls that end in a device synchronise, after one warm-up round; one process"
    stats = [item.split("=", 1) if "=" in item else (item, item) for item in args.stats_csv]
    stats = [(label, p) for label, p in stats if os.path.exists(p)]
    # (a traced run holds the set-up, the warm-up step of two iterations and the one timed step)
    result["kernel_stats_of_only_step_runs"] = {label: kernel_stats(p) for label, p in stats} if stats else "not measured"
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
