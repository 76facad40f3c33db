"""One rank of a sharded cal_solver_solve_gain_time_coeffs call whose exchange runs through cal_solver_set_exchange_hook over gloo (helper
of tests/test_gpu_gain_time_solve_ranks.py; started as a fresh process per rank, two of them sharing the one GPU)."""
import argparse
import datetime
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OPTS = dict(layout="shared", kernel_path="general")
NSWEEPS = 3


NTIMES = 4


def build_case():
    """(problem, parameters): 4 times of 5 antennas x 48 channels as one fit, the start values perturbed by about 10 %."""
    from calamity_amd import distributed, synthetic

    cache, parts = {}, []
    for t in range(NTIMES):
        pt, _, st = synthetic.make_problem(5, 48, f0=150e6, df=400e3, seed=17, data_seed=40 + t, operator_cache=cache)
        parts.append((pt, st))
    p, start = distributed.batch_time_slices(parts, per_slice=False)
    rng = np.random.default_rng(18)
    gs = (p.nants, p.nfreqs)
    return p, dict(g_r=start["g_r"] + 0.1 * rng.standard_normal(gs), g_i=start["g_i"] + 0.1 * rng.standard_normal(gs),
                   c_r=start["c_r"] * (1.0 + 0.1 * rng.standard_normal(p.ncoeffs)), c_i=start["c_i"] * (1.0 + 0.1 * rng.standard_normal(p.ncoeffs)))


def basis(nfreqs):
    from calamity_amd import modeling

    return np.array(modeling.gain_dpss_basis(150e6 + 400e3 * np.arange(nfreqs), 100.0))


def time_basis():
    from calamity_amd import modeling

    return modeling.gain_time_dpss_basis(2458101.25 + 10.7 / 86400.0 * np.arange(NTIMES), 30.0)


def solved(sub, params, hook=None, rank=0, world=1, calls=None):
    """The gains and y after NSWEEPS sweeps of one call (``calls``: the hook's log; its length in front of the call is returned too)."""
    from calamity_amd.solver import HipFitSolver

    s = HipFitSolver(dtype=np.float64)
    if hook is not None:
        s.set_exchange_hook(hook, rank, world)  # before set_problem: the ranks agree on the kernel family there
    s.set_problem(sub, **OPTS)
    s.set_params(params["g_r"], params["g_i"], params["c_r"], params["c_i"])
    s.set_gain_basis(basis(sub.nfreqs))
    s.set_gain_time_basis(time_basis())
    ncalls = 0 if calls is None else len(calls)
    counts = s.solve_gain_time_coeffs(NSWEEPS)
    g_r, g_i = s.get_params()[:2]
    y_r, y_i = s.get_gain_coeffs()
    s.close()
    return dict(g_r=g_r, g_i=g_i, y_r=y_r, y_i=y_i, calls_before=ncalls, nsolved=counts["nsolved"], nsingular=counts["nsingular"])


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
    g = solved(sub, sub_params, hook=all_reduce, rank=args.rank, world=args.world, calls=calls)
    np.savez(args.out, call_sizes=np.asarray([c[1] for c in calls]), call_ops=np.asarray([c[2] for c in calls]),
             call_dtypes=np.asarray([c[0] for c in calls]), **g)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
