"""One rank of a sharded cal_solver_delay_coherent_spectrum call whose exchange runs through cal_solver_set_exchange_hook over gloo (helper
of tests/test_gpu_delay_coherent_ranks.py; started as a fresh process per rank, two of them sharing the one GPU)."""
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
NTIMES, NRATES = 2, 2


def build_case(world=2):
    """The spectrum's case plus ragged groups of global rows: every rank's rows grouped among themselves (group i of a rank: the sets
    {i, i + 1, i + 2} and {i + 3}, cyclically, of its rows), so no group joins two ranks; coefficients, conjugation flags, unequal
    scales; group 4 in no bin.  Returns (p, params, op, norm_f, set_ptr, member_row, member_wgt, member_conj, opt, scale, bins)."""
    from calamity_amd import modeling

    p, params, op, norm_f, _ = S.build_case()
    groups = []
    for r in range(world):
        rows = S.rows_of_rank(p, r, world)
        at = lambda i: int(rows[i % len(rows)])  # noqa: E731
        groups += [[[at(i), at(i + 1), at(i + 2)], [at(i + 3)]] for i in range(len(rows))]
    groups.sort()
    sizes = [len(s) for g in groups for s in g]
    set_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    member_row = np.asarray([b for g in groups for s in g for b in s], dtype=np.int32)
    rng = np.random.default_rng(19)
    wgt = rng.uniform(0.5, 2.0, size=len(member_row))
    cj = (rng.random(len(member_row)) < 0.3).astype(np.uint8)
    opt = modeling.fringe_rate_transform(NTIMES, 10.0)[0][:, :NRATES]
    scale = rng.uniform(0.5, 2.0, size=(len(groups), NTIMES))
    bins = (np.arange(len(groups)) % NBINS).astype(np.int32)
    bins[4] = -1
    return p, params, op, norm_f, set_ptr, member_row, wgt, cj, opt, scale, bins


def coherent(sub, params, op, norm_f, set_ptr, member_row, wgt, cj, opt, scale, bins, hook=None, rank=0, world=1):
    from calamity_amd.solver import HipFitSolver

    s = HipFitSolver(dtype=np.float64)
    if hook is not None:
        s.set_exchange_hook(hook, rank, world)  # before set_problem: the ranks agree on the kernel family there
    s.set_problem(sub, **S.OPTS)
    s.set_params(params["g_r"], params["g_i"], params["c_r"], params["c_i"])
    out = s.delay_coherent_spectrum(op, norm_f, set_ptr, member_row, opt, member_wgt=wgt, member_conj=cj, weighting="weights", scale=scale, bin_of_group=bins,
                                    nbins=NBINS)  # binned only: the normal call
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

    p, params, op, norm_f, set_ptr, member_row, wgt, cj, opt, scale, bins = build_case(args.world)
    sub, sub_params = D.shard_problem(p, params, args.rank, args.world)
    sel, parts = batched.split_member_groups(set_ptr, member_row, NTIMES, [S.rows_of_rank(p, r, args.world) for r in range(args.world)], p.nbls)
    mine, (my_ptr, my_rows, my_members) = sel[args.rank], parts[args.rank]
    out = coherent(sub, sub_params, op, norm_f, my_ptr, my_rows, wgt[my_members], cj[my_members], opt, scale[mine], bins[mine], hook=all_reduce,
                   rank=args.rank, world=args.world)
    np.savez(args.out, call_sizes=np.asarray([c[1] for c in calls]), call_ops=np.asarray([c[2] for c in calls]),
             call_dtypes=np.asarray([c[0] for c in calls]), mine=mine, **out)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
