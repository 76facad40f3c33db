"""One rank of sharded cal_solver_gain_basis_errors calls whose exchange runs through cal_solver_set_exchange_hook over gloo (helper of
tests/test_gpu_gain_basis_errors_ranks.py; started as a fresh process per rank, two of them sharing the one GPU).  One solver, three
calls: under the frequency basis, under both bases, under the time basis alone; the hook's log says what each exchanged."""
import argparse
import datetime
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CONFIGS = ("freq", "both", "time")


def errors_of(sub, params, hook=None, rank=0, world=1, calls=None):
    """{config_key: array} of the three calls, and per config the slice of the hook's log that belongs to the call."""
    import _gain_time_solve_rank as X
    from calamity_amd.solver import HipFitSolver

    s = HipFitSolver(dtype=np.float64)
    if hook is not None:
        s.set_exchange_hook(hook, rank, world)  # before set_problem: the ranks agree on the kernel family there
    s.set_problem(sub, **X.OPTS)
    s.set_params(params["g_r"], params["g_i"], params["c_r"], params["c_i"])
    attach = {"freq": lambda: s.set_gain_basis(X.basis(sub.nfreqs)), "both": lambda: s.set_gain_time_basis(X.time_basis()),
              "time": lambda: s.set_gain_basis(None)}
    out = {}
    for config in CONFIGS:
        attach[config]()
        n0 = 0 if calls is None else len(calls)
        e = s.gain_basis_errors()
        for k, v in e.items():
            out[f"{config}_{k}"] = np.asarray(v)
        if calls is not None:
            out[f"{config}_sizes"] = np.asarray([c[1] for c in calls[n0:]], dtype=np.int64)
            out[f"{config}_ops"] = np.asarray([f"{c[0]} {c[2]}" for c in calls[n0:]])
    s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, required=True)
    ap.add_argument("--world", type=int, default=2)
    ap.add_argument("--port", type=int, required=True)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    import _gain_time_solve_rank as X
    from calamity_amd import _lib
    from calamity_amd import distributed as D

    _lib.load()  # our HIP runtime first, then torch (used for the gloo transport only)
    import torch
    import torch.distributed as dist

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{args.port}", rank=args.rank, world_size=args.world,
                            timeout=datetime.timedelta(seconds=60))
    calls = []

    def all_reduce(arr, op):
        calls.append((arr.dtype.str, arr.size, op))
        t = torch.from_numpy(arr)  # shares the library's staging buffer: reduced in place
        dist.all_reduce(t, op=dist.ReduceOp.MIN if op == "min" else dist.ReduceOp.SUM)

    p, params = X.build_case()
    sub, sub_params = D.shard_problem(p, params, args.rank, args.world)
    out = errors_of(sub, sub_params, hook=all_reduce, rank=args.rank, world=args.world, calls=calls)
    np.savez(args.out, **out)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
