"""One rank of a sharded cal_solver_fit_errors call under cal_solver_set_exchange_hook over gloo (helper of
tests/test_gpu_fit_errors.py; started as a fresh process per rank, two of them sharing the one GPU).  The rank reports the errors of
its own fitting groups and rows and what the call exchanged: one float64 plane (den) when gain_var is asked for, nothing otherwise."""
import argparse
import datetime
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

OPTS = dict(layout="shared", kernel_path="general")


def build_case():
    import _coeff_solve_rank

    return _coeff_solve_rank.build_case()


def errors_of(sub, params, hook=None, rank=0, world=1, calls=None):
    from calamity_amd.solver import HipFitSolver

    s = HipFitSolver(dtype=np.float64)
    if hook is not None:
        s.set_exchange_hook(hook, rank, world)  # before set_problem: the ranks agree on the kernel family there
    s.set_problem(sub, **OPTS)
    s.set_params(params["g_r"], params["g_i"], params["c_r"], params["c_i"])
    n0 = 0 if calls is None else len(calls)
    s.fit_errors(gain_var=False)
    n1 = 0 if calls is None else len(calls)
    out = s.fit_errors()
    s.close()
    if calls is not None:
        out["exchanges_without_gain_var"] = np.asarray(calls[n0:n1], dtype=np.int64).reshape(-1, 2)
        out["exchanges"] = np.asarray(calls[n1:], dtype=np.int64).reshape(-1, 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, required=True)
    ap.add_argument("--world", type=int, default=2)
    ap.add_argument("--port", type=int, required=True)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    from calamity_amd import _lib
    from calamity_amd import distributed as D

    _lib.load()  # our HIP runtime first, then torch (used for the gloo transport only)
    import torch
    import torch.distributed as dist

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{args.port}", rank=args.rank, world_size=args.world,
                            timeout=datetime.timedelta(seconds=60))
    calls = []

    def all_reduce(arr, op):
        calls.append((arr.dtype.itemsize, arr.size))
        t = torch.from_numpy(arr)  # shares the library's staging buffer: reduced in place
        dist.all_reduce(t, op=dist.ReduceOp.MIN if op == "min" else dist.ReduceOp.SUM)

    p, params = build_case()
    sub, sub_params = D.shard_problem(p, params, args.rank, args.world)
    out = errors_of(sub, sub_params, hook=all_reduce, rank=args.rank, world=args.world, calls=calls)
    np.savez(args.out, **{k: np.asarray(v) for k, v in out.items()})
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
