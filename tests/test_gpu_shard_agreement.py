"""Sharded multi-slice fits whose ranks hold different kinds of share (nothing a rank decides locally may
change what it sends).

``batched.SliceBatchFitter`` with two or three workers on one GPU (``devices=[0, 0]``: exchange through host memory) against
one worker and against the C restatement fitted slice by slice.  In the STREAM layout the baselines that repeat over the slices
are fitted together as heads of the multi-slice kernels; with the "sum" regulariser a rank whose heads cannot take the
one-pass form (a block wider than 224 vectors in fp32 / 160 in fp64) runs a loss pre-pass and exchanges the slices' sums once
more per step.  The ranks agree on it in set_problem: if one needs the pre-pass, every rank runs it -- also a rank without
heads (a share that holds a multi-baseline group has no alias table).  Cases (tests/_slice_cases.py):

A  every block <= 160 vectors on every rank: one pass everywhere (the bench's own job), with and without the regulariser
B  the wide blocks on one rank only: two passes on EVERY rank; unregularised control
C  one rank without heads, the other with the wide block: two passes on both
D  the dense path (SHARED layout), several slices: the dense path's own pre-pass
E  case B with slices that stop at different steps, use_min
F  case B over three workers

Each: loss, per-slice losses and every gradient against the C oracle (fp64 1e-10; fp32 1e-5 / 1e-4), 1 + 12 Adam steps
against the oracle's trajectories and the one-worker fit, replicated gains bit-identical on every worker, and every worker's
exchange call by call.  Ranks that disagree on the problem's shape fail set_problem together."""
import os
import sys
import threading
from functools import lru_cache

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _slice_cases as SC  # noqa: E402

pytestmark = pytest.mark.gpu

AGREE = (np.dtype(np.int32).str, 4, "min")  # the set-up agreement (calamity_hip.hip: agree_problem)
NSTEPS = 12


def relnorm(a, b):
    return np.linalg.norm(np.asarray(a, dtype=np.float64) - b) / max(np.linalg.norm(b), 1e-300)


@pytest.fixture
def exchange_log(monkeypatch):
    """Every worker's exchange calls (dtype str, count, op), in order, of the fitters made while the test runs."""
    from calamity_amd import batched

    log = {}

    class Recording(batched._HostExchange):
        def hook(self, rank):
            inner = super().hook(rank)
            calls = log[rank] = []

            def all_reduce(arr, op):
                calls.append((arr.dtype.str, int(arr.size), op))
                inner(arr, op)

            return all_reduce

    monkeypatch.setattr(batched, "_HostExchange", Recording)
    return log


@lru_cache(maxsize=None)
def case_data(case, dtype):
    return SC.build(case, np.dtype(dtype).type)


@lru_cache(maxsize=None)
def oracle(case, dtype, reg):
    """The C restatement, slice by slice, stacked in the fitter's global layout: (loss, per-slice losses, gg_r, gg_i, gc_r, gc_i)
    at the start, and the 1 + NSTEPS step Adam trajectory (losses [T, NSTEPS + 1], g_r, g_i, c_r, c_i)."""
    from oracle.ref_c import CRef

    cd = case_data(case, dtype)
    ev, tr = [], []
    for t, (p, st) in enumerate(cd["parts"]):
        c = CRef(p, np.float64)
        c.set_regularization("sum" if reg else None, cd["prior_r"][t], cd["prior_i"][t])
        ev.append(c.loss_grads(st["g_r"], st["g_i"], st["c_r"], st["c_i"]))
        tr.append(c.fit(st["g_r"], st["g_i"], st["c_r"], st["c_i"], NSTEPS + 1, optimizer="Adam", learning_rate=1e-2))
    cat = lambda rows, k: np.concatenate([r[k] for r in rows])  # noqa: E731
    sl = np.asarray([e[0] for e in ev])
    return dict(loss=float(sl.sum()), slices=sl, grads=[cat(ev, k) for k in (1, 2, 3, 4)],
                losses=np.stack([r[4] for r in tr]), params=[cat(tr, k) for k in (0, 1, 2, 3)])


def make_fitter(cd, dtype, devices, reg, layout="stream", kernel_path="general"):
    from calamity_amd.batched import SliceBatchFitter

    f = SliceBatchFitter(cd["prob"], cd["nt"], dtype=dtype, layout=layout, devices=devices, kernel_path=kernel_path)
    f.set_data(cd["data_r"], cd["data_i"], cd["wgts"])
    f.set_params(cd["g_r"], cd["g_i"], cd["c_r"], cd["c_i"])
    f.set_regularization("sum" if reg else None, cd["prior_r"], cd["prior_i"])
    f.set_optimizer("Adam", learning_rate=1e-2)
    return f


def evaluate_and_fit(f, nsteps=NSTEPS, tol=0.0, use_min=False):
    ev = f.eval_grads()
    sl = f.slice_losses()
    f.run_slices(1, record=False)
    res = f.run_slices(nsteps, record=True, tol=tol, use_min=use_min)
    out = dict(ev=ev, slices=sl, res=res, params=f.get_params(), workers=[s.get_params() for s in f.solvers],
               paths=[s.timing_get()["kernel_path"] for s in f.solvers])
    if use_min:
        out["snap"] = f.get_params(1)
    return out


def solo_pattern(cd, dtype, rank, nranks):
    """Rank ``rank``'s share fitted alone under a one-rank recording hook (no peer to agree with): the exchange of one
    regularised train step as its own problem takes it."""
    from calamity_amd.solver import HipFitSolver

    sub, rows, cidx = SC.rank_share(cd, rank, nranks)
    calls = []
    s = HipFitSolver(dtype=dtype)
    s.set_exchange_hook(lambda arr, op: calls.append((arr.dtype.str, int(arr.size), op)), 0, 1)
    s.set_problem(sub, layout="stream", kernel_path="general")
    s.set_data(cd["data_r"][rows], cd["data_i"][rows], cd["wgts"][rows])
    s.set_params(cd["g_r"], cd["g_i"], cd["c_r"][cidx], cd["c_i"][cidx])
    s.set_regularization("sum", cd["prior_r"], cd["prior_i"])
    s.set_optimizer("Adam", learning_rate=1e-2)
    assert calls == [AGREE]
    del calls[:]
    s.run_slices(1, record=False)
    s.close()
    return calls


def check_exchange(log, nworkers, pattern, nt, dtype, nsteps=NSTEPS):
    """Every worker issued the identical sequence: the agreement, then the same exchange for every pass (eval_grads, 1 + nsteps
    train steps)."""
    assert sorted(log) == list(range(nworkers))
    for r in range(1, nworkers):
        assert log[r] == log[0], r
    calls = log[0]
    assert calls[0] == AGREE, calls[:2]
    step = SC.per_step(pattern, nt, dtype)
    assert calls[1:] == step * (nsteps + 2), (pattern, calls[1:1 + 2 * len(step)])


def check_against_oracle(out, cd, case, dtype, reg):
    ref = oracle(case, dtype, reg)
    f64 = np.dtype(dtype) == np.float64
    tol_l, tol_g = (1e-10, 1e-10) if f64 else (1e-5, 1e-4)
    loss, gg_r, gg_i, gc_r, gc_i = out["ev"]
    assert abs(loss - ref["loss"]) <= tol_l * abs(ref["loss"])
    np.testing.assert_allclose(out["slices"], ref["slices"], rtol=tol_l)
    errs = [relnorm(a, b) for a, b in zip((gg_r, gg_i, gc_r, gc_i), ref["grads"])]
    assert max(errs) <= tol_g, errs
    losses = np.stack([r[0] for r in out["res"]])
    if f64:
        np.testing.assert_allclose(losses, ref["losses"][:, 1:], rtol=1e-8)
    else:
        np.testing.assert_allclose(losses, ref["losses"][:, 1:], rtol=1e-4)
    perrs = [relnorm(a, b) for a, b in zip(out["params"], ref["params"])]
    assert max(perrs) <= (1e-8 if f64 else 1e-3), perrs
    return max(errs), max(perrs)


def check_against_one_worker(out, one, dtype):
    f64 = np.dtype(dtype) == np.float64
    for (la, sa, na), (lb, sb, nb) in zip(out["res"], one["res"]):
        assert len(la) == len(lb) and sa == sb and na == nb
        np.testing.assert_allclose(la, lb, rtol=1e-10 if f64 else 1e-4)
    errs = [relnorm(a, b) for a, b in zip(out["params"], one["params"])]
    assert max(errs) <= (1e-10 if f64 else 1e-3), errs
    return max(errs)


def check_replicated(out):
    """Every worker applied the same update to the same reduced gradient: bit-identical gains."""
    for w in out["workers"][1:]:
        np.testing.assert_array_equal(w[0], out["workers"][0][0])
        np.testing.assert_array_equal(w[1], out["workers"][0][1])


def run_case(exchange_log, case, dtype, reg, devices=(0, 0), layout="stream", kernel_path="general"):
    cd = case_data(case, dtype)
    f = make_fitter(cd, dtype, list(devices), reg, layout, kernel_path)
    try:
        out = evaluate_and_fit(f)
    finally:
        f.close()
    log = {r: list(c) for r, c in exchange_log.items()}
    one = make_fitter(cd, dtype, [0], reg, layout, kernel_path)
    try:
        ref1 = evaluate_and_fit(one)
    finally:
        one.close()
    check_replicated(out)
    e_or = check_against_oracle(out, cd, case, dtype, reg)
    e_one = check_against_one_worker(out, ref1, dtype)
    print(f"{case} {np.dtype(dtype).name} reg={reg}: gradients / parameters vs oracle {e_or[0]:.2e} / {e_or[1]:.2e}, "
          f"parameters vs one worker {e_one:.2e}")
    return cd, out, log


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("reg", [False, True])
def test_uniform_shares_keep_one_pass(exchange_log, dtype, reg):
    """A: every block <= 160 vectors on both ranks -- the regularised step stays ONE pass on every rank."""
    cd, out, log = run_case(exchange_log, "uniform", dtype, reg)
    for r in range(2):
        assert solo_pattern(cd, dtype, r, 2) == SC.per_step("one_pass", cd["nt"], dtype)
    check_exchange(log, 2, "one_pass" if reg else "none", cd["nt"], dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("reg", [True, False])
def test_wide_block_on_one_rank(exchange_log, dtype, reg):
    """B: the wide blocks on rank 0 only.  Alone, rank 0's share takes two passes and rank 1's one; together, with the
    regulariser, BOTH take two (rank 1's heads on the alpha form); without it, the plain exchange."""
    cd = case_data("wide", dtype)
    assert solo_pattern(cd, dtype, 0, 2) == SC.per_step("two_pass", cd["nt"], dtype)
    assert solo_pattern(cd, dtype, 1, 2) == SC.per_step("one_pass", cd["nt"], dtype)
    cd, out, log = run_case(exchange_log, "wide", dtype, reg)
    check_exchange(log, 2, "two_pass" if reg else "none", cd["nt"], dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_rank_without_heads_joins_the_pre_pass(exchange_log, dtype):
    """C: rank 1 holds a 3-baseline group (its share has no alias table: no heads, the one-pass two-adjoint-set form), rank 0
    the wide block: both run the loss pre-pass, rank 1's S partials are part of the slices' sums."""
    from calamity_amd.batched import replicate_slices

    cd = case_data("noheads", dtype)
    groups = SC.shares(cd, 2)
    assert replicate_slices(cd["prob"], cd["nt"], groups[1])[0].bl_alias is None
    assert replicate_slices(cd["prob"], cd["nt"], groups[0])[0].bl_alias is not None
    assert solo_pattern(cd, dtype, 0, 2) == SC.per_step("two_pass", cd["nt"], dtype)
    assert solo_pattern(cd, dtype, 1, 2) == SC.per_step("one_pass", cd["nt"], dtype)
    cd, out, log = run_case(exchange_log, "noheads", dtype, True)
    check_exchange(log, 2, "two_pass", cd["nt"], dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("reg", [False, True])
def test_dense_path_several_slices(exchange_log, dtype, reg):
    """D: the SHARED layout's dense kernels (split-bf16 in fp32, fp64 MFMA) over two workers with several slices: with the
    regulariser their own loss pre-pass (S, alpha) in front of the single-part gradient exchange."""
    cd, out, log = run_case(exchange_log, "dense", dtype, reg, layout="shared", kernel_path="dense")
    assert all(p.startswith("dense") for p in out["paths"]), out["paths"]
    check_exchange(log, 2, "dense_sum" if reg else "none", cd["nt"], dtype)


def test_slices_stop_at_different_steps(exchange_log):
    """E: case B in fp64 with a tolerance at which the slices stop at different steps, use_min: every slice's recorded losses,
    stop, update count and use_min snapshot equal the one-worker run's."""
    dtype, nsteps = np.float64, 80
    cd = case_data("wide", dtype)
    one = make_fitter(cd, dtype, [0], True)
    try:
        free = evaluate_and_fit(one, nsteps=nsteps)
    finally:
        one.close()
    # the tolerance: a step difference that the slices reach at different steps, well inside the run
    diffs = [np.abs(np.diff(r[0])) for r in free["res"]]
    tol = None
    for cand in np.geomspace(max(d.max() for d in diffs), min(d.min() for d in diffs), 60)[1:-1]:
        first = [int(np.argmax(d < cand)) if np.any(d < cand) else None for d in diffs]
        close = any(np.any(np.abs(d / cand - 1.0) < 1e-6) for d in diffs)
        if None not in first and max(first) < nsteps - 10 and len(set(first)) > 1 and not close:
            tol = float(cand)
            break
    assert tol is not None
    outs = []
    for devices in ([0, 0], [0]):
        f = make_fitter(cd, dtype, devices, True)
        try:
            outs.append(evaluate_and_fit(f, nsteps=nsteps, tol=tol, use_min=True))
        finally:
            f.close()
    stops = [len(r[0]) for r in outs[1]["res"]]
    assert len(set(stops)) > 1 and all(r[1] for r in outs[1]["res"]), stops
    check_against_one_worker(outs[0], outs[1], dtype)
    check_replicated(outs[0])
    for a, b in zip(outs[0]["snap"], outs[1]["snap"]):
        assert relnorm(a, b) <= 1e-10
    # (the run ended when the last slice stopped: steps are issued in chunks, so count whole steps of the two-pass exchange)
    calls = exchange_log[0]
    step = SC.per_step("two_pass", cd["nt"], dtype)
    assert exchange_log[1] == calls and calls[0] == AGREE
    assert len(calls[1:]) % len(step) == 0 and calls[1:] == step * (len(calls[1:]) // len(step))


def test_three_workers_wide_block_on_one(exchange_log):
    """F: case B over three workers (the wide blocks on rank 0 of 3): two passes on all three."""
    dtype = np.float64
    cd = case_data("wide3", dtype)
    assert solo_pattern(cd, dtype, 0, 3) == SC.per_step("two_pass", cd["nt"], dtype)
    for r in (1, 2):
        assert solo_pattern(cd, dtype, r, 3) == SC.per_step("one_pass", cd["nt"], dtype)
    cd, out, log = run_case(exchange_log, "wide3", dtype, True, devices=(0, 0, 0))
    check_exchange(log, 3, "two_pass", cd["nt"], dtype)


def test_ranks_that_disagree_on_the_slice_count_both_fail_set_problem():
    """A rank whose problem holds another number of slices (same antennas, same rows): set_problem fails with CAL_ERR_INVALID
    on BOTH ranks, naming the field, and the agreement is the only exchange."""
    from calamity_amd import _lib
    from calamity_amd.batched import _HostExchange
    from calamity_amd.solver import HipFitSolver

    cd = case_data("uniform", np.float64)
    subs = [SC.rank_share(cd, r, 2)[0] for r in range(2)]
    subs[1].nslices, subs[1].bl_alias = 2, None  # (two slices of twice the antennas)
    subs[1].validate()
    assert subs[0].nants == subs[1].nants and subs[0].nslices == 4
    ex = _HostExchange(2)
    calls, errs = {0: [], 1: []}, [None, None]
    solvers = [HipFitSolver(dtype=np.float64) for _ in range(2)]

    def hook(r):
        inner = ex.hook(r)

        def all_reduce(arr, op):
            calls[r].append((arr.dtype.str, int(arr.size), op))
            inner(arr, op)

        return all_reduce

    def work(r):
        try:
            solvers[r].set_problem(subs[r], layout="stream", kernel_path="general")
        except BaseException as e:  # noqa: BLE001 -- checked below
            errs[r] = e
            if not isinstance(e, _lib.CalamityHipError):
                ex.abort()  # (failed before the agreement: the peer must not wait for it)

    try:
        for r, s in enumerate(solvers):
            s.set_exchange_hook(hook(r), r, 2)
        threads = [threading.Thread(target=work, args=(r,)) for r in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=120)
        assert not any(t.is_alive() for t in threads)
    finally:
        for s in solvers:
            s.close()
    for r in range(2):
        assert errs[r] is not None and errs[r].code == _lib.CAL_ERR_INVALID and "nslices" in str(errs[r]), (r, errs[r])
        assert calls[r] == [AGREE], calls[r]
