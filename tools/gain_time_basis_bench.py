#!/usr/bin/env python3
"""What a gain time basis costs per train step: 8 times of HERA-350 x 1024 channels as ONE joint fit, fp32, Adam, gain_max_dly = 100 ns
(K = 30) plus the time basis of 8 integrations of 10.7 s at 400 s (L = 4), both layouts.

Yardstick: the PARENT commit running the same joint fit with the frequency basis only, from a built copy of the parent tree, in the
same call on the same box, alternated with this tree (A, A, B, A, B: the A/A pair gives the same-box spread).  Reported side by
side: the parent's frequency-basis step, this tree's frequency-basis step (must agree within the A/A spread: a fit without a time
basis pays nothing), this tree's step with both bases, its step with the time basis alone (W = fpad), and the exchange payload per
step of each form (counted through a one-rank exchange hook, not timed).  The 8 times hold the same data: a step's cost does not
depend on them.

    python tools/gain_time_basis_bench.py --ab PARENT_TREE --out profiles/gain_time_basis_hera350_f32.json [--stats-csv kernel_stats.csv]
    python tools/gain_time_basis_bench.py --measure [--tree DIR] [--time-basis] [--layouts shared,stream]   # one process, one JSON line

``--stats-csv``: the kernel statistics of a separate ``rocprofv3 --kernel-trace --stats`` run of ``--measure --time-basis``; the
durations of gain_time_project_kernel and gain_time_expand_kernel in it are the allowance for the joint step over the parent's.
Every child process runs under its own time limit and the first one that fails ends the run."""
import argparse
import csv
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NTIMES = 8


def measure(tree, time_basis, layouts, steps, warmup, dly_ns, time_scale_s):
    sys.path.insert(0, tree)
    import numpy as np

    from calamity_amd import modeling, synthetic
    from calamity_amd.batched import replicate_slices
    from calamity_amd.solver import HipFitSolver

    p, _, start = synthetic.make_config("hera350")
    big, _, _ = replicate_slices(p, NTIMES)
    big.nslices = 1  # one fit, one loop state: distributed.batch_time_slices(per_slice=False)
    tile = lambda a, dt: np.tile(np.asarray(a, dtype=dt), (NTIMES,) + (1,) * (np.ndim(a) - 1))  # noqa: E731
    data = [tile(a, np.float32) for a in (p.data_r, p.data_i, p.wgts)]
    par = [tile(start[k], np.float32) for k in ("g_r", "g_i", "c_r", "c_i")]
    B = np.array(modeling.gain_dpss_basis(100e6 + (100e6 / p.nfreqs) * np.arange(p.nfreqs), dly_ns))
    out = dict(tree=os.path.abspath(tree), ntimes=NTIMES, nants=int(p.nants), nfreqs=int(p.nfreqs), nbls=int(p.nbls), steps=steps, warmup=warmup,
               gain_nvec=int(B.shape[1]))
    Bt = None
    if time_basis:
        Bt = np.array(modeling.gain_time_dpss_basis(2458101.25 + np.arange(NTIMES) * 10.7 / 86400.0, time_scale_s))
        out["gain_time_nvec"] = int(Bt.shape[1])

    def timed(s):
        s.run(warmup, record=False)
        s.synchronize()
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            s.run(steps, record=True, tol=0.0)
            s.synchronize()
            dt = (time.perf_counter() - t0) / steps * 1e3
            best = dt if best is None else min(best, dt)
        return best

    for layout in layouts:
        s = HipFitSolver(dtype=np.float32)
        s.set_problem(big, layout=layout)
        s.set_data(*data)
        forms = [("freq", B, None)] + ([("joint", B, Bt), ("time_only", None, Bt)] if time_basis else [])
        res = dict(kernel_path=s.timing_get()["kernel_path"])
        for name, b, bt in forms:
            s.set_params(*par)
            s.set_gain_basis(b)
            if time_basis:
                s.set_gain_time_basis(bt)
            s.set_optimizer("Adam", learning_rate=1e-3)
            res[name + "_ms"] = timed(s)
        # the exchange payload of one step, counted: a one-rank hook sees what a communicator would reduce
        for name, b, bt in forms:
            calls = []
            s.set_exchange_hook(lambda arr, op: calls.append(int(arr.size)), 0, 1)
            s.set_gain_basis(b)
            if time_basis:
                s.set_gain_time_basis(bt)
            del calls[:]
            s.run(1, record=False)
            res["payload_reals_" + name] = max(calls)
            s.set_exchange_hook(None, 0, 1)
        s.close()
        out[layout] = res
        print(f"# {layout}: {res}", file=sys.stderr, flush=True)
    print(json.dumps(out), flush=True)


def child(tree, time_basis, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--measure", "--tree", tree, "--layouts", args.layouts, "--steps", str(args.steps),
           "--warmup", str(args.warmup), "--dly", str(args.dly), "--time-scale", str(args.time_scale)] + (["--time-basis"] if time_basis else [])
    r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=args.child_timeout, check=True, text=True)
    return json.loads(r.stdout.strip().splitlines()[-1])


def kernel_stats(path):
    """Average duration (us) and calls of the basis kernels and their neighbours out of rocprofv3's kernel statistics."""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            for k in ("gain_time_project_kernel", "gain_time_expand_kernel", "gain_project_kernel", "gain_expand_kernel", "gain_grad_kernel",
                      "adam2_kernel", "step_update_kernel"):
                if k in name:
                    out[k] = dict(calls=int(row["Calls"]), average_us=float(row["AverageNs"]) / 1e3, total_percent=float(row.get("Percentage", "nan")),
                                  name=name)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--measure", action="store_true")
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--time-basis", action="store_true")
    ap.add_argument("--layouts", default="shared,stream")
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=32)
    ap.add_argument("--dly", type=float, default=100.0)
    ap.add_argument("--time-scale", type=float, default=400.0)
    ap.add_argument("--ab", metavar="PARENT_TREE")
    ap.add_argument("--out")
    ap.add_argument("--stats-csv")
    ap.add_argument("--child-timeout", type=int, default=420)
    args = ap.parse_args()
    if args.measure:
        return measure(args.tree, args.time_basis, args.layouts.split(","), args.steps, args.warmup, args.dly, args.time_scale)
    if not args.ab:
        ap.error("--measure or --ab PARENT_TREE")
    runs = [("A", child(args.ab, False, args)), ("A", child(args.ab, False, args)), ("B", child(HERE, True, args)),
            ("A", child(args.ab, False, args)), ("B", child(HERE, True, args))]
    result = dict(config=f"{NTIMES} times of hera350 x 1024 channels as one joint fit, fp32, Adam, gain_max_dly {args.dly:g} ns, time scale {args.time_scale:g} s",
                  steps=args.steps, warmup=args.warmup, order="A A B A B (A: parent tree, frequency basis only; B: this tree); best of 3 timed runs per entry",
                  runs=[dict(which=w, **r) for w, r in runs])
    for layout in args.layouts.split(","):
        a = [r[layout]["freq_ms"] for w, r in runs if w == "A"]
        b = [r[layout]["freq_ms"] for w, r in runs if w == "B"]
        y = [r[layout]["joint_ms"] for w, r in runs if w == "B"]
        z = [r[layout]["time_only_ms"] for w, r in runs if w == "B"]
        b0 = runs[2][1][layout]
        result[layout] = dict(parent_freq_ms=a, aa_spread_ms=abs(a[0] - a[1]), branch_freq_ms=b, branch_joint_ms=y, branch_time_only_ms=z,
                              joint_minus_parent_ms=[min(y) - min(a), max(y) - max(a)], kernel_path=b0["kernel_path"],
                              payload_reals_freq=b0["payload_reals_freq"], payload_reals_joint=b0["payload_reals_joint"],
                              payload_reals_time_only=b0["payload_reals_time_only"])
    if args.stats_csv and os.path.exists(args.stats_csv):
        result["kernel_stats_shared_joint_run"] = kernel_stats(args.stats_csv)
    else:
        result["kernel_stats_shared_joint_run"] = "not measured"
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
