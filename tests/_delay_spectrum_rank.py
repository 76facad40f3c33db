"""One rank of a sharded cal_solver_delay_spectrum call whose exchange runs through cal_solver_set_exchange_hook over gloo (helper of
tests/test_gpu_delay_spectrum_ranks.py; started as a fresh process per rank, two of them sharing the one GPU)."""
import argparse
import datetime
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OPTS = dict(layout="shared", kernel_path="general")
NBINS, NDELAYS = 3, 37


def build_case():
    """(problem, parameters, operator, norm_f, bin_of_bl): 7 antennas, 64 channels, the start values perturbed by about 10 %."""
    from calamity_amd import modeling, synthetic

    p, _, start = synthetic.make_problem(7, 64, f0=150e6, df=400e3, seed=17)
    rng = np.random.default_rng(18)
    gs = (p.nants, p.nfreqs)
    params = dict(g_r=start["g_r"] + 0.1 * rng.standard_normal(gs), g_i=start["g_i"] + 0.1 * rng.standard_normal(gs),
                  c_r=start["c_r"] * (1.0 + 0.1 * rng.standard_normal(p.ncoeffs)), c_i=start["c_i"] * (1.0 + 0.1 * rng.standard_normal(p.ncoeffs)))
    op, norm_f, _ = modeling.delay_transform(150e6 + 400e3 * np.arange(64))
    lo = (64 - NDELAYS) // 2
    bins = (np.arange(p.nbls) % NBINS).astype(np.int32)
    bins[4] = -1
    return p, params, np.ascontiguousarray(op[:, lo : lo + NDELAYS]), norm_f, bins


def rows_of_rank(p, rank, world):
    from calamity_amd import distributed as D

    shares = D.partition_groups(p.grp_nvec, p.grp_basis, np.diff(p.grp_bl_start), world)
    return np.concatenate([np.arange(p.grp_bl_start[g], p.grp_bl_start[g + 1]) for g in shares[rank]])


def spectrum(sub, params, op, norm_f, bins, hook=None, rank=0, world=1):
    from calamity_amd.solver import HipFitSolver

    s = HipFitSolver(dtype=np.float64)
    if hook is not None:
        s.set_exchange_hook(hook, rank, world)  # before set_problem: the ranks agree on the kernel family there
    s.set_problem(sub, **OPTS)
    s.set_params(params["g_r"], params["g_i"], params["c_r"], params["c_i"])
    out = s.delay_spectrum(op, norm_f, bin_of_bl=bins, nbins=NBINS)  # binned only: the normal call
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

    p, params, op, norm_f, bins = build_case()
    sub, sub_params = D.shard_problem(p, params, args.rank, args.world)
    out = spectrum(sub, sub_params, op, norm_f, bins[rows_of_rank(p, args.rank, args.world)], hook=all_reduce, rank=args.rank, world=args.world)
    np.savez(args.out, call_sizes=np.asarray([c[1] for c in calls]), call_ops=np.asarray([c[2] for c in calls]),
             call_dtypes=np.asarray([c[0] for c in calls]), **out)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
