"""One rank of a sharded cal_solver_delay_transfer call whose exchange runs through cal_solver_set_exchange_hook over gloo (helper of
tests/test_gpu_delay_transfer_ranks.py; started as a fresh process per rank, two of them sharing the one GPU).  The case is that of
tests/_delay_spectrum_rank.py."""
import argparse
import datetime
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _delay_spectrum_rank import NBINS, NDELAYS, OPTS, build_case, rows_of_rank  # noqa: E402,F401


def transfer(sub, params, op, bins, hook=None, rank=0, world=1, per_baseline=True):
    from calamity_amd.solver import HipFitSolver

    s = HipFitSolver(dtype=np.float64)
    if hook is not None:
        s.set_exchange_hook(hook, rank, world)  # before set_problem: the ranks agree on the kernel family there
    s.set_problem(sub, **OPTS)
    s.set_params(params["g_r"], params["g_i"], params["c_r"], params["c_i"])
    out = s.delay_transfer(op, bin_of_bl=bins, nbins=NBINS, per_baseline=per_baseline)
    s.close()
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
        calls.append((arr.dtype.str, arr.size, op))
        t = torch.from_numpy(arr)  # shares the library's staging buffer: reduced in place
        dist.all_reduce(t, op=dist.ReduceOp.MIN if op == "min" else dist.ReduceOp.SUM)

    p, params, op, _, bins = build_case()
    sub, sub_params = D.shard_problem(p, params, args.rank, args.world)
    out = transfer(sub, sub_params, op, bins[rows_of_rank(p, args.rank, args.world)], hook=all_reduce, rank=args.rank, world=args.world)
    np.savez(args.out, call_sizes=np.asarray([c[1] for c in calls]), call_ops=np.asarray([c[2] for c in calls]),
             call_dtypes=np.asarray([c[0] for c in calls]), **out)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
