#!/usr/bin/env python3
"""Kernel experiment harness: time the fused basis kernel of several builds on the same seeded problem, alternating
between them, one fresh process per build and round.  A build is a library (.so: the child of THIS tree assigns
calamity_amd._lib.LIB_PATH before the library is loaded) or a whole source tree with its library built (a directory: its own
tools/kbench.py child runs with its own Python package -- for builds whose binding differs from this tree's).  The harness stops
at the first child that exits non-zero or exceeds --child-timeout: nothing more is started on the device after a failure.
Usage: kbench.py [--config hera350] [--max-bls N] [--rounds 5] [--kernel-path general_full] build1 build2 ..."""
import argparse
import json
import os
import subprocess
import sys

import statistics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(args):
    import numpy as np
    from calamity_amd import _lib, synthetic

    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)  # experiment build instead of the shipped one
    from calamity_amd.solver import HipFitSolver

    dtype = np.float64 if args.dtype == "f64" else np.float32
    if args.slices:
        import bench
        prob, start, _ = bench.build_sharded_job(args.config, 0, args.slices, args.slices, max_bls=args.max_bls)
    elif args.cache and os.path.exists(args.cache):
        import pickle
        prob, start = pickle.load(open(args.cache, "rb"))
    else:
        prob, truth, start = synthetic.make_config(args.config, max_bls=args.max_bls, with_sky=True)
        if args.redundant:
            prob, start = synthetic.merge_redundant_groups(prob, truth, start)
        if args.cache:
            import pickle
            pickle.dump((prob, start), open(args.cache, "wb"), protocol=4)
    s = HipFitSolver(dtype=dtype)
    if args.kernel_path:
        s.set_problem(prob, layout=args.layout, kernel_path=args.kernel_path)
    else:
        s.set_problem(prob, layout=args.layout)
    s.set_params(start["g_r"], start["g_i"], start["c_r"], start["c_i"])
    if args.reg:
        src_r, src_i = (prob.sky_r, prob.sky_i) if prob.sky_r is not None else (0.9 * prob.data_r, 1.1 * prob.data_i)  # (a sharded job carries no sky: any prior will do for timing)
        s.set_regularization("sum", float(np.sum(src_r * prob.wgts)), float(np.sum(src_i * prob.wgts)))
    s.set_optimizer("Adam", learning_rate=1e-2)
    out = {}
    s.run(3, record=False)
    s.timing_enable(True)
    import time
    s.synchronize(); t0 = time.perf_counter()
    s.run(args.steps, record=True, tol=0.0)
    s.synchronize(); dt = time.perf_counter() - t0
    t = s.timing_get()
    out["grad_ms"] = t["total_ms"] / t["launches"]
    out["step_ms"] = dt / args.steps * 1e3
    out["grad_GBs"] = t["algorithmic_bytes_per_launch"] / out["grad_ms"] / 1e6
    s.timing_enable(True)
    for _ in range(args.steps):
        s.eval_loss()
    t = s.timing_get()
    out["loss_ms"] = t["total_ms"] / t["launches"]
    out["basis_folded"] = t.get("basis_folded", 0)
    out["device_memory_GB"] = s.memory_bytes() / 1e9
    print("KBENCH " + json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="hera350")
    ap.add_argument("--max-bls", type=int, default=None)
    ap.add_argument("--dtype", default="f32")
    ap.add_argument("--layout", default="stream")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reg", action="store_true")
    ap.add_argument("--slices", type=int, default=0, help="the per-rank job of an N-GPU run: N time slices x 1/N of the baselines, sharing tiles")
    ap.add_argument("--redundant", action="store_true", help="merge redundant baselines into shared-coefficient groups")
    ap.add_argument("--cache", default="/tmp/kbench_problem.pkl")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--lib", default=None, help="(child) the library build to load")
    ap.add_argument("--rounds", type=int, default=2, help="alternations over the builds")
    ap.add_argument("--kernel-path", default=None, help="kernel_path of set_problem (e.g. general_full: the unfolded streaming kernel); only builds that know it")
    ap.add_argument("--child-timeout", type=float, default=300.0, help="seconds one child may take")
    ap.add_argument("libs", nargs="*", help="builds: .so files, or source trees with a built library; NAME@kernel_path runs a build under that kernel path")
    args = ap.parse_args()
    if args.child:
        child(args)
        sys.exit(0)
    passthrough = []
    for name in ("config", "dtype", "layout", "cache"):
        passthrough += ["--" + name, str(getattr(args, name))]
    passthrough += ["--steps", str(args.steps), "--slices", str(args.slices)]
    if args.max_bls is not None:
        passthrough += ["--max-bls", str(args.max_bls)]
    passthrough += ["--reg"] * args.reg + ["--redundant"] * args.redundant
    results = {}
    for rnd in range(args.rounds):
        for spec in args.libs:
            build, _, path = spec.partition("@")
            path = path or args.kernel_path
            if os.path.isdir(build):  # a tree: its own harness and package
                cmd = [sys.executable, os.path.join(os.path.abspath(build), "tools", "kbench.py"), "--child"] + passthrough
                cwd = os.path.abspath(build)
            else:
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--lib", os.path.abspath(build)] + passthrough
                cwd = ROOT
            if path:
                cmd += ["--kernel-path", path]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, cwd=cwd, timeout=args.child_timeout)
            except subprocess.TimeoutExpired:
                print(rnd, spec, f"TIMEOUT after {args.child_timeout:.0f} s: stopping", flush=True)
                sys.exit(124)
            line = [l for l in r.stdout.splitlines() if l.startswith("KBENCH ")]
            if r.returncode != 0 or not line:
                print(rnd, spec, f"FAILED (exit {r.returncode}): stopping\n" + r.stderr[-800:], flush=True)
                sys.exit(r.returncode or 1)
            print(rnd, spec, line[0][7:], flush=True)
            results.setdefault(spec, []).append(json.loads(line[0][7:]))
    for spec, rows in results.items():
        for key in ("step_ms", "grad_ms", "loss_ms"):
            v = [row[key] for row in rows]
            print(f"SUMMARY {spec} {key}: median {statistics.median(v):.4f} min {min(v):.4f} max {max(v):.4f} (n={len(v)})", flush=True)
