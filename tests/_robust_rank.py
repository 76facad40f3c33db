"""One rank of a sharded cal_solver_robust_weights call under cal_solver_set_exchange_hook over gloo (helper of
tests/test_gpu_robust_ranks.py; started as a fresh process per rank, two of them sharing the one GPU).  The hook's call log is cut
around the call: the reweighting is local to a baseline row and must exchange nothing."""
import argparse
import datetime
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OPTS = dict(layout="shared", kernel_path="general")
KIND, THRESHOLD = "huber", 2.0


def build_case():
    """(problem, parameters): 7 antennas, 200 channels, the start values perturbed by about 10 % (|residual| ~ |data|)."""
    from calamity_amd import synthetic

    p, _, start = synthetic.make_problem(7, 200, f0=150e6, df=400e3, seed=17)
    rng = np.random.default_rng(18)
    gs = (p.nants, p.nfreqs)
    return p, dict(g_r=start["g_r"] + 0.1 * rng.standard_normal(gs), g_i=start["g_i"] + 0.1 * rng.standard_normal(gs),
                   c_r=start["c_r"] * (1.0 + 0.1 * rng.standard_normal(p.ncoeffs)), c_i=start["c_i"] * (1.0 + 0.1 * rng.standard_normal(p.ncoeffs)))


def reweight(sub, params, hook=None, rank=0, world=1, calls=None):
    """dict(w, w0, scale_bl, ndown_bl, ncalls_before, ncalls_after) of one solver."""
    from calamity_amd.solver import HipFitSolver

    s = HipFitSolver(dtype=np.float64)
    if hook is not None:
        s.set_exchange_hook(hook, rank, world)  # before set_problem: the ranks agree on the kernel family there
    s.set_problem(sub, **OPTS)
    s.set_params(params["g_r"], params["g_i"], params["c_r"], params["c_i"])
    before = 0 if calls is None else len(calls)
    out = s.robust_weights(kind=KIND, threshold=THRESHOLD)
    w, w0 = s.get_weights(0), s.get_weights(1)
    after = 0 if calls is None else len(calls)
    s.close()
    return dict(out, w=w, w0=w0, ncalls_before=before, ncalls_after=after)


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

    p, params = build_case()
    sub, sub_params = D.shard_problem(p, params, args.rank, args.world)
    r = reweight(sub, sub_params, hook=all_reduce, rank=args.rank, world=args.world, calls=calls)
    np.savez(args.out, **r)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
