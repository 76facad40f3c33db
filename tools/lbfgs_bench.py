#!/usr/bin/env python3
"""What L-BFGS costs and buys at HERA-350 x 1024 channels, fp32, both layouts, in one process on one box.

After a warm-up round of every call that is timed (code objects, first allocations), each move starts from the same parameters (unity
gains, c0) and is timed by a host clock around work that ends in a device synchronise:

    lbfgs(30 iterations, history 8)
    100 descent steps                       (Adam, learning rate 1e-2)
    one round of alternating least squares  (solve_coeffs + 5 half-damped sweeps)
    one gauss_newton_step(20)               (lambda 1e-3)

with the chi-square after each (``eval_loss``), the passes L-BFGS spent, the device memory before and after its vectors exist, and the
read rate ``cal_device_stream_peak`` reports in the same process.

    python tools/lbfgs_bench.py --measure [--layouts shared,stream] [--only-lbfgs]      # one process, one JSON line
    python tools/lbfgs_bench.py --out profiles/lbfgs_hera350_f32.json [--stats-csv shared=a_kernel_stats.csv stream=b_kernel_stats.csv]

``--only-lbfgs``: set-up and the one call alone (no warm-up call), for a separate ``rocprofv3 --kernel-trace --stats --output-format csv``
run; ``--stats-csv``: that run's kernel statistics, from which the split of an iteration into passes and ``lbfgs_*`` kernels and the
achieved bytes per second of ``lbfgs_pair_kernel`` and ``lbfgs_direction_kernel`` are taken.  The bytes are the algorithmic ones of the
iterations the call ran with every pair accepted: with p pairs stored the pair kernel reads 4 vectors and writes 4, then reads 3 + 2 min(4,
.) vectors per tile of four stored pairs; the direction kernel reads 2 p + 1 and writes one.  The child process runs under its own time
limit."""
import argparse
import csv
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITERS, HISTORY = 30, 8


def vector_traffic(iters, history, np_reals, itemsize):
    """Algorithmic bytes of all launches of the pair kernel and of the direction kernel over a call of ``iters`` iterations."""
    pair, direction = 4, 0  # the start: x and g read, x_k and g_k written
    for k in range(1, iters + 1):
        stored = min(k - 1, history)  # pairs held when iteration k ends / when its direction was formed
        pair += 8 + sum(3 + 2 * min(4, stored - j0) for j0 in range(0, stored, 4))
        if stored > 0:
            direction += 2 * stored + 2
    return dict(pair_bytes=pair * np_reals * itemsize, direction_bytes=direction * np_reals * itemsize, vector_bytes=np_reals * itemsize)


def measure(layouts, only_lbfgs, config):
    sys.path.insert(0, HERE)
    import numpy as np

    from calamity_amd import _lib, synthetic
    from calamity_amd.solver import HipFitSolver

    p, _, start = synthetic.make_config(config)
    par = [np.asarray(start[k], dtype=np.float32) for k in ("g_r", "g_i", "c_r", "c_i")]
    out = dict(config=config, nants=int(p.nants), nfreqs=int(p.nfreqs), nbls=int(p.nbls), ncoeffs=int(p.ncoeffs), iterations=ITERS, history=HISTORY)
    if not only_lbfgs:
        rd, cp = _lib.stream_peak(0, 1 << 30, 5)
        out.update(stream_peak_read_gbs=rd, stream_peak_copy_gbs=cp)

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
        if not only_lbfgs:  # warm-up: every call that is timed below, once
            s.lbfgs(2, history=HISTORY)
            res["memory_bytes_after"] = s.memory_bytes()  # (before the other moves allocate their own scratch)
            s.solve_coeffs()
            s.solve_gains(5, damping=0.5)
            s.gauss_newton_step(ncg=2)
            s.run(20, record=False)
            restart()
        ms, st = timed(s, lambda: s.lbfgs(ITERS, history=HISTORY))
        res.setdefault("memory_bytes_after", s.memory_bytes())
        passes = int(st["iters"][0] + st["evals"][0]) + 1
        res.update(lbfgs_ms=ms, lbfgs_iters=int(st["iters"][0]), lbfgs_evals=int(st["evals"][0]), lbfgs_passes=passes, lbfgs_status=int(st["status"][0]),
                   lbfgs_pairs_dropped=int(st["pairs_dropped"][0]), ms_per_iteration=ms / max(int(st["iters"][0]), 1),
                   chisq_after_lbfgs=float(st["loss_after"][0]), chisq_per_iteration=[float(x) for x in st["losses"][0]])
        res.update(vector_traffic(int(st["iters"][0]), HISTORY, 2 * p.nants * (-(-p.nfreqs // 8) * 8) + 2 * p.ncoeffs, 4))  # (rows are padded to a multiple of 8 channels)
        if not only_lbfgs:
            restart()
            ms, _ = timed(s, lambda: s.run(100, record=False))
            res.update(descent_100_steps_ms=ms, chisq_after_100_descent_steps=s.eval_loss())
            restart()
            ms, _ = timed(s, lambda: s.run(passes, record=False))
            res.update(descent_same_passes_ms=ms, chisq_after_descent_of_the_same_passes=s.eval_loss())
            restart()
            ms, _ = timed(s, lambda: (s.solve_coeffs(), s.solve_gains(5, damping=0.5)))
            res.update(als_round_ms=ms, chisq_after_als_round=s.eval_loss())
            restart()
            ms, gn = timed(s, lambda: s.gauss_newton_step(ncg=20, lam=1e-3))
            res.update(gauss_newton_step_ms=ms, gauss_newton_accepted=bool(gn["accepted"][0]), chisq_after_gauss_newton_step=float(gn["loss_after"][0]))
        s.close()
        out[layout] = res
        print(f"# {layout}: { {k: v for k, v in res.items() if k != 'chisq_per_iteration'} }", file=sys.stderr, flush=True)
    print(json.dumps(out), flush=True)


def kernel_stats(path):
    """Calls, average and total duration of the call's own kernels and of the passes out of rocprofv3's kernel statistics."""
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
    own = sum(e["total_ms"] for k, e in out.items() if k.startswith("lbfgs_"))
    return dict(kernels=out, total_ms=total / 1e6, lbfgs_kernels_ms=own, lbfgs_kernels_percent=100.0 * own * 1e6 / max(total, 1.0))


def achieved(stats, res):
    """GB/s of the two history kernels: the call's algorithmic bytes over the kernels' summed durations."""
    out = {}
    for key, prefix in (("pair_bytes", "lbfgs_pair_kernel"), ("direction_bytes", "lbfgs_direction_kernel")):
        ms = sum(e["total_ms"] for k, e in stats["kernels"].items() if k.startswith(prefix))
        if ms > 0:
            out[prefix + "_gbs"] = res[key] / (ms * 1e-3) / 1e9
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--measure", action="store_true")
    ap.add_argument("--only-lbfgs", action="store_true")
    ap.add_argument("--layouts", default="shared,stream")
    ap.add_argument("--config", default="hera350")
    ap.add_argument("--out")
    ap.add_argument("--stats-csv", nargs="*", default=[])
    ap.add_argument("--child-timeout", type=int, default=540)
    args = ap.parse_args()
    if args.measure:
        return measure(args.layouts.split(","), args.only_lbfgs, args.config)
    cmd = [sys.executable, os.path.abspath(__file__), "--measure", "--layouts", args.layouts, "--config", args.config]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=args.child_timeout, check=True, text=True)
    result = json.loads(r.stdout.strip().splitlines()[-1])
    result["timing"] = "host clock around calls that end in a device synchronise, after one warm-up round; one process"
    stats = [item.split("=", 1) if "=" in item else (item, item) for item in args.stats_csv]
    stats = {label: kernel_stats(p) for label, p in stats if os.path.exists(p)}
    # (a traced run holds the set-up and the one timed call)
    result["kernel_stats_of_only_lbfgs_runs"] = stats if stats else "not measured"
    for label, st in stats.items():
        if label in result:
            result[label].update(achieved(st, result[label]))
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
