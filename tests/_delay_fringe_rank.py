"""One rank of a sharded cal_solver_delay_fringe_spectrum call whose exchange runs through cal_solver_set_exchange_hook over gloo (helper
of tests/test_gpu_delay_fringe_ranks.py; started as a fresh process per rank, two of them sharing the one GPU)."""
import argparse
import datetime
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _delay_spectrum_rank as S  # noqa: E402

NBINS, NDELAYS = S.NBINS, S.NDELAYS
NTIMES, NRATES = 3, 2


def build_case(world=2):
    """The spectrum's case plus (rows [ngroups, 3] of global rows, opt [3, 2], scale, bin_of_group): every rank's rows grouped among
    themselves (row i of a rank with its rows i + 1 and i + 2, cyclically), so no group joins two ranks; unequal scales; group 4 in no
    bin."""
    from calamity_amd import modeling

    p, params, op, norm_f, _ = S.build_case()
    groups = []
    for r in range(world):
        rows = S.rows_of_rank(p, r, world)
        groups += [tuple(int(rows[(i + k) % len(rows)]) for k in range(NTIMES)) for i in range(len(rows))]
    groups = np.asarray(sorted(groups), dtype=np.int32)
    opt = modeling.fringe_rate_transform(NTIMES, 10.0)[0][:, :NRATES]
    scale = np.random.default_rng(19).uniform(0.5, 2.0, size=groups.shape)
    bins = (np.arange(len(groups)) % NBINS).astype(np.int32)
    bins[4] = -1
    return p, params, op, norm_f, groups, opt, scale, bins


def fringe(sub, params, op, norm_f, rows, opt, scale, bins, hook=None, rank=0, world=1):
    from calamity_amd.solver import HipFitSolver

    s = HipFitSolver(dtype=np.float64)
    if hook is not None:
        s.set_exchange_hook(hook, rank, world)  # before set_problem: the ranks agree on the kernel family there
    s.set_problem(sub, **S.OPTS)
    s.set_params(params["g_r"], params["g_i"], params["c_r"], params["c_i"])
    out = s.delay_fringe_spectrum(op, norm_f, rows, opt, scale=scale, bin_of_group=bins, nbins=NBINS)  # binned only: the normal call
    s.close()
    return {"norm_grp": out["norm_grp"], "count_bin": out["count_bin"], **{q: out[q] for q in ("data", "model", "resid")}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, required=True)
    ap.add_argument("--world", type=int, default=2)
    ap.add_argument("--port", type=int, required=True)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    from calamity_amd import _lib, batched
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

    p, params, op, norm_f, groups, opt, scale, bins = build_case(args.world)
    sub, sub_params = D.shard_problem(p, params, args.rank, args.world)
    sel, local = batched.split_groups(groups, [S.rows_of_rank(p, r, args.world) for r in range(args.world)], p.nbls)
    mine = sel[args.rank]
    out = fringe(sub, sub_params, op, norm_f, local[args.rank], opt, scale[mine], bins[mine], hook=all_reduce, rank=args.rank, world=args.world)
    np.savez(args.out, call_sizes=np.asarray([c[1] for c in calls]), call_ops=np.asarray([c[2] for c in calls]),
             call_dtypes=np.asarray([c[0] for c in calls]), mine=mine, **out)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
