#!/usr/bin/env python3
"""What a gain basis costs per train step, HERA-350 x 1024 channels, fp32, Adam, gain_max_dly = 100 ns (K = 30), both layouts.

Yardstick: the per-channel step of the PARENT commit, from a built copy of the parent tree, in the same call on the same box,
alternated with this tree (A, A, B, A, B: the A/A pair gives the same-box spread).  Reported side by side: parent per-channel
step, this tree's per-channel step (must agree within the A/A spread: a fit without a basis pays nothing), this tree's basis
step, and the exchange payload per step with and without the basis (counted through a one-rank exchange hook, not timed).

    python tools/gain_basis_bench.py --ab PARENT_TREE --out profiles/gain_basis_hera350_f32.json [--stats-csv kernel_stats.csv]
    python tools/gain_basis_bench.py --measure [--tree DIR] [--basis] [--layouts shared,stream]   # one process, one JSON line

``--stats-csv``: the kernel statistics of a separate ``rocprofv3 --kernel-trace --stats`` run of ``--measure --basis``; the
durations of gain_project_kernel and gain_expand_kernel in it are the allowance for the basis step over the per-channel step."""
import argparse
import csv
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def measure(tree, basis, layouts, steps, warmup, dly_ns):
    sys.path.insert(0, tree)
    import numpy as np

    from calamity_amd import synthetic
    from calamity_amd.solver import HipFitSolver

    p, _, start = synthetic.make_config("hera350")
    out = dict(tree=os.path.abspath(tree), nants=int(p.nants), nfreqs=int(p.nfreqs), nbls=int(p.nbls), steps=steps, warmup=warmup)
    B = None
    if basis:
        from calamity_amd import modeling

        B = np.array(modeling.gain_dpss_basis(100e6 + (100e6 / p.nfreqs) * np.arange(p.nfreqs), dly_ns))
        out["gain_nvec"] = int(B.shape[1])

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
        s.set_problem(p, layout=layout)
        s.set_params(start["g_r"], start["g_i"], start["c_r"], start["c_i"])
        s.set_optimizer("Adam", learning_rate=1e-3)
        res = dict(kernel_path=s.timing_get()["kernel_path"], per_channel_ms=timed(s))
        if B is not None:
            s.set_params(start["g_r"], start["g_i"], start["c_r"], start["c_i"])
            s.set_gain_basis(B)
            s.set_optimizer("Adam", learning_rate=1e-3)
            res["basis_ms"] = timed(s)
            # the exchange payload of one step, counted: a one-rank hook sees what a communicator would reduce
            for name, b in (("payload_reals_basis", B), ("payload_reals_per_channel", None)):
                calls = []
                s.set_exchange_hook(lambda arr, op: calls.append(int(arr.size)), 0, 1)
                s.set_gain_basis(b)
                del calls[:]
                s.run(1, record=False)
                res[name] = max(calls)
        s.close()
        out[layout] = res
        print(f"# {layout}: {res}", file=sys.stderr, flush=True)
    print(json.dumps(out), flush=True)


def child(tree, basis, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--measure", "--tree", tree, "--layouts", args.layouts, "--steps", str(args.steps),
           "--warmup", str(args.warmup), "--dly", str(args.dly)] + (["--basis"] if basis else [])
    r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=args.child_timeout, check=True, text=True)
    return json.loads(r.stdout.strip().splitlines()[-1])


def kernel_stats(path):
    """Average duration (us) and calls of the two basis kernels out of rocprofv3's kernel statistics."""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            for k in ("gain_project_kernel", "gain_expand_kernel", "gain_grad_kernel", "adam2_kernel", "step_update_kernel"):
                if k in name:
                    out[k] = dict(calls=int(row["Calls"]), average_us=float(row["AverageNs"]) / 1e3, name=name)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--measure", action="store_true")
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--basis", action="store_true")
    ap.add_argument("--layouts", default="shared,stream")
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--dly", type=float, default=100.0)
    ap.add_argument("--ab", metavar="PARENT_TREE")
    ap.add_argument("--out")
    ap.add_argument("--stats-csv")
    ap.add_argument("--child-timeout", type=int, default=420)
    args = ap.parse_args()
    if args.measure:
        return measure(args.tree, args.basis, args.layouts.split(","), args.steps, args.warmup, args.dly)
    if not args.ab:
        ap.error("--measure or --ab PARENT_TREE")
    runs = [("A", child(args.ab, False, args)), ("A", child(args.ab, False, args)), ("B", child(HERE, True, args)),
            ("A", child(args.ab, False, args)), ("B", child(HERE, True, args))]
    result = dict(config="hera350 x 1024 channels, fp32, Adam, gain_max_dly 100 ns", steps=args.steps, warmup=args.warmup,
                  order="A A B A B (A: parent tree, B: this tree); best of 3 timed runs per entry", runs=[dict(which=w, **r) for w, r in runs])
    for layout in args.layouts.split(","):
        a = [r[layout]["per_channel_ms"] for w, r in runs if w == "A"]
        b = [r[layout]["per_channel_ms"] for w, r in runs if w == "B"]
        y = [r[layout]["basis_ms"] for w, r in runs if w == "B"]
        b0 = runs[2][1][layout]
        result[layout] = dict(parent_per_channel_ms=a, aa_spread_ms=abs(a[0] - a[1]), branch_per_channel_ms=b, branch_basis_ms=y,
                              basis_minus_parent_ms=[min(y) - min(a), max(y) - max(a)], kernel_path=b0["kernel_path"],
                              payload_reals_per_channel=b0["payload_reals_per_channel"], payload_reals_basis=b0["payload_reals_basis"])
    if args.stats_csv and os.path.exists(args.stats_csv):
        result["kernel_stats_shared_basis_run"] = kernel_stats(args.stats_csv)
    else:
        result["kernel_stats_shared_basis_run"] = "not measured"
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
