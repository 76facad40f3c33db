"""One rank of a sharded fit whose exchange runs through cal_solver_set_exchange_hook over gloo (helper of
tests/test_gpu_exchange_hook.py; started as a fresh process per rank, two of them sharing the one GPU)."""
import argparse
import datetime
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))  # (_slice_cases)


def build_case(name):
    """(full problem, start, per-rank group lists or None for the cost-balanced partition, solver options, run options)"""
    from calamity_amd import synthetic

    reg = name.endswith("_sum")
    if name.startswith("general_tbasis"):
        # T = 4 times of 7 antennas at 40 channels as ONE fit (antenna a at time t is row t * 7 + a), the problem of
        # tests/test_gain_time_basis_host.py: joint_case -- built here: a rank imports no test module
        from calamity_amd import distributed as D

        cache, parts = {}, []
        for t in range(len(TBASIS_TIMES)):
            p, _, start = synthetic.make_problem(7, 40, f0=150e6, df=400e3, seed=60, data_seed=61 + t, with_sky=reg, operator_cache=cache)
            parts.append((p, start))
        big, start = D.batch_time_slices(parts, per_slice=False)
        rng = np.random.default_rng(7)
        start["g_r"] = 1.0 + 0.05 * rng.standard_normal((big.nants, big.nfreqs))
        start["g_i"] = 0.05 * rng.standard_normal((big.nants, big.nfreqs))
        return big, start, None, dict(layout="stream", kernel_path="general"), dict(nsteps=12, tol=0.0), reg
    if name.startswith("fallback"):
        # 70 antennas = 2415 baselines: rank 0's share (2100) is large enough for the dense kernels, rank 1's (315) is not
        p, _, start = synthetic.make_problem(70, 128, f0=150e6, df=400e3, seed=4, with_sky=reg)
        groups = [np.arange(0, 2100), np.arange(2100, p.ngrps)]
        return p, start, groups, dict(layout="shared", kernel_path="auto"), dict(nsteps=6, tol=0.0), reg
    p, _, start = synthetic.make_problem(12, 128, f0=150e6, df=400e3, seed=6, with_sky=reg)
    rng = np.random.default_rng(8)
    start["g_r"] = 1.0 + 0.05 * rng.standard_normal((p.nants, p.nfreqs))
    start["g_i"] = 0.05 * rng.standard_normal((p.nants, p.nfreqs))
    path = "dense" if name.startswith("dense") else "general"
    run = dict(nsteps=400, tol=1e-7) if name.startswith("tolstop") else dict(nsteps=12, tol=0.0)
    return p, start, None, dict(layout="shared", kernel_path=path), run, reg


TBASIS_TIMES = 2458101.25 + np.arange(4) * 10.7 / 86400.0  # (the first four of tests/test_gain_time_basis_host.py: TIMES_60)


def case_bases(name, p):
    """(frequency basis or None, time basis or None) of a case: the 100 ns DPSS basis of its channels for "gbasis" and "tbasis", the
    400 s DPSS basis of its four times for "tbasis"."""
    from calamity_amd import modeling

    if "_gbasis" not in name and "_tbasis" not in name:
        return None, None
    Bf = np.array(modeling.gain_dpss_basis(150e6 + 400e3 * np.arange(p.nfreqs), 100.0))
    return Bf, (np.array(modeling.gain_time_dpss_basis(TBASIS_TIMES, 400.0)) if "_tbasis" in name else None)


def priors(p):
    return float(np.sum(p.sky_r * p.wgts)), float(np.sum(p.sky_i * p.wgts))


def fit(sub, start, opts, run, reg_priors, hook=None, rank=0, world=1, bases=(None, None)):
    from calamity_amd.solver import HipFitSolver

    s = HipFitSolver(dtype=np.float64)
    if hook is not None:
        s.set_exchange_hook(hook, rank, world)  # before set_problem: the ranks then agree on the kernel family there
    s.set_problem(sub, **opts)
    s.set_params(start["g_r"], start["g_i"], start["c_r"], start["c_i"])
    if reg_priors is not None:
        s.set_regularization("sum", *reg_priors)
    if bases[0] is not None:
        s.set_gain_basis(bases[0])
    if bases[1] is not None:
        s.set_gain_time_basis(bases[1])
    s.set_optimizer("Adam", learning_rate=2e-2)
    s.run(1, record=False)
    losses, stopped, nupd = s.run(run["nsteps"], record=True, tol=run["tol"])
    g_r, g_i, c_r, c_i = s.get_params()
    out = dict(losses=losses, stopped=stopped, nupd=nupd, g_r=g_r, g_i=g_i, c_r=c_r, c_i=c_i, path=s.timing_get()["kernel_path"])
    if bases[0] is not None or bases[1] is not None:
        out["y_r"], out["y_i"] = s.get_gain_coeffs()
    s.close()
    return out


def fit_slices(case_data, sub, rows, cidx, dtype, hook=None, rank=0, world=1):
    """The multi-slice cases: T slices of a share in one solver (what a rank of ``bench.py --gpus N`` holds), STREAM layout,
    the "sum" regulariser with every slice's own priors, 1 unrecorded + 12 recorded Adam steps through run_slices."""
    from calamity_amd.solver import HipFitSolver

    s = HipFitSolver(dtype=dtype)
    if hook is not None:
        s.set_exchange_hook(hook, rank, world)
    s.set_problem(sub, layout="stream", kernel_path="general")
    s.set_data(case_data["data_r"][rows], case_data["data_i"][rows], case_data["wgts"][rows])
    s.set_params(case_data["g_r"], case_data["g_i"], case_data["c_r"][cidx], case_data["c_i"][cidx])
    s.set_regularization("sum", case_data["prior_r"], case_data["prior_i"])
    s.set_optimizer("Adam", learning_rate=1e-2)
    s.run_slices(1, record=False)
    res = s.run_slices(12, record=True, tol=0.0)
    g_r, g_i, c_r, c_i = s.get_params()
    s.close()
    return dict(losses=np.stack([r[0] for r in res]), stopped=np.asarray([r[1] for r in res]), nupd=np.asarray([r[2] for r in res]),
                g_r=g_r, g_i=g_i, c_r=c_r, c_i=c_i, path="general")


SLICE_CASES = {"slices_wide32_sum": ("wide", np.float32)}  # case B of test_gpu_shard_agreement.py in fp32, one process per rank


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", required=True)
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

    # (a rank that waits for a peer that never comes fails within a minute instead of holding the test until its timeout)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{args.port}", rank=args.rank, world_size=args.world,
                            timeout=datetime.timedelta(seconds=60))
    calls = []
    dtypes = {np.dtype(np.int32).str: 0, np.dtype(np.float32).str: 1, np.dtype(np.float64).str: 2}

    def all_reduce(arr, op):
        calls.append((arr.dtype.str, arr.size, op))
        # every rank first shows what it is about to reduce: ranks that issue different exchanges all raise, naming each other's
        # calls, instead of pairing unrelated buffers in the payload reduction
        mine = torch.tensor([arr.size, dtypes[arr.dtype.str], 1 if op == "min" else 0], dtype=torch.int64)
        every = [torch.zeros_like(mine) for _ in range(args.world)]
        dist.all_gather(every, mine)
        if any(not torch.equal(e, every[0]) for e in every):
            raise RuntimeError("the ranks issued different exchanges (count, dtype code, op): "
                               + "; ".join(f"rank {r}: {tuple(e.tolist())}" for r, e in enumerate(every)))
        t = torch.from_numpy(arr)  # shares the library's staging buffer: reduced in place
        dist.all_reduce(t, op=dist.ReduceOp.MIN if op == "min" else dist.ReduceOp.SUM)

    if args.case in SLICE_CASES:
        import _slice_cases as SC

        name, dtype = SLICE_CASES[args.case]
        cd = SC.build(name, dtype)
        sub, rows, cidx = SC.rank_share(cd, args.rank, args.world)
        out = fit_slices(cd, sub, rows, cidx, dtype, hook=all_reduce, rank=args.rank, world=args.world)
    else:
        p, start, groups, opts, run, reg = build_case(args.case)
        if groups is None:
            sub, sub_start = D.shard_problem(p, start, args.rank, args.world)
        else:
            sub, sub_start = D.select_groups(p, start, groups[args.rank])
        out = fit(sub, sub_start, opts, run, priors(p) if reg else None, hook=all_reduce, rank=args.rank, world=args.world, bases=case_bases(args.case, p))
    np.savez(args.out, ncalls=len(calls), call_sizes=np.asarray([c[1] for c in calls]), call_ops=np.asarray([c[2] for c in calls]),
             call_dtypes=np.asarray([c[0] for c in calls]), **{k: np.asarray(v) for k, v in out.items()})
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
