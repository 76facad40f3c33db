"""cal_solver_lbfgs where its kernels branch (csrc/lbfgs_kernels.hpp), against the NumPy restatement tests/lbfgs_ref.py.
tests/test_gpu_lbfgs.py follows the run in which every slice accepts its first trial and stores every pair; here the inputs take the
device through everything else a slice can do:

    1  a pair refused by the curvature test, and a pair stored into the same free slot afterwards
    2  a search that runs out with pairs held: they are dropped and the same iteration is searched again along -g_k
    3  three slices that take different branches in one call: one starts over, one never does, one stalls after it has moved
    4  status 3 at the start for one slice of three (a NaN in its data; all its weights zero)
    5  the whole ring: history = 16, 17 slots, four tiles of stored pairs, evictions at full size
    6  more than 64 blocks a slice: the second trip of the reduce kernel's lane loop

Tolerances are those of tests/test_gpu_lbfgs.py (losses fp64 1e-10, fp32 1e-5; parameters norm-wise fp64 1e-8, fp32 1e-3; fp32 over
the first FIRST iterations), none new but the measured bound of test 5.  Every comparison first asserts the restatement's own decision
margin (fp64 >= 1e-6, fp32 >= 1e-2) and that the RESTATEMENT took the branch the test is named after: conditions on the inputs, met by
choosing them; the expected counters are never read off the device.  Every test prints the margin and the branch counters.

Left out: the cap kLbBlocks = 1024 (more than 2 M reals a slice in fp64: far beyond a few seconds); slope >= 0 out of the two-loop
recursion (it cannot happen with finite stored pairs: every stored pair has s.y > 0); a non-finite TRIAL loss (not reachable from finite
data: the first step is normalised to unit length); host-only tests (tests/test_lbfgs_host.py pins lbfgs_two_loop at every pair count)."""
import copy
import functools

import numpy as np
import pytest

from calamity_amd import synthetic
from gauss_newton_ref import Ref
from lbfgs_ref import LbfgsRef
from test_gpu_fit_quality import solver_of
from test_gpu_gauss_newton import CONFIGS, KEYS, assert_path, base_problem, cast_params, relnorm, three_slices
from test_gpu_lbfgs import COUNTERS, DTYPES, FIRST, TOL, basis_case, check_losses, check_params, heavier, name

pytestmark = pytest.mark.gpu

TWO_PATHS = [c for c in CONFIGS if (c[0], c[1]) in (("stream", "auto"), ("shared", "dense"))]
SHAPE = (7, 200)


def steps_of(dtype, full=12):
    return full if dtype == np.float64 else FIRST


def controls_key(kw):
    return tuple(sorted(kw.items()))


@functools.lru_cache(maxsize=None)
def restated(dtype_name, nsteps, weight, controls):
    """The restatement on base_problem(7, 200) with ``weight`` times the weights, from the perturbed start."""
    p, params = base_problem(*SHAPE)
    dtype = np.dtype(dtype_name).type
    g, c = cast_params(params, dtype)
    return LbfgsRef(Ref(heavier(p, weight), dtype=dtype), dtype).run(g, c, nsteps, **dict(controls))


def report(label, want, dtype):
    """Prints the restatement's margin and branch counters and asserts the margin."""
    print(f"{label}: the restatement's margin {want['margin']:.2e}, iters {want['iters']} evals {want['evals']} pairs_dropped {want['pairs_dropped']} "
          f"status {want['status']}, stored " + "".join("s" if b else "-" for b in want["stored"]))
    assert want["margin"] >= TOL[np.dtype(dtype)]["margin"], "choose a problem whose decisions are not marginal"


def check_run(s, out, want, dtype, label):
    for k in COUNTERS:
        assert out[k][0] == want[k], (label, k, out[k][0], want[k])
    check_losses(out["losses"][0], want["losses"], dtype, label, upto=want["iters"])
    assert np.all(np.isnan(out["losses"][0][want["iters"] + 1 :]))
    check_params(s, want["gains"] if "gains" in want else want["v"], want["c"], dtype, label)
    assert out["loss_before"][0] == out["losses"][0][0] and out["loss_after"][0] == out["losses"][0][want["iters"]]


def one_slice(config, dtype, weight, kw, label):
    layout, path, runs = config
    p, params = base_problem(*SHAPE)
    n = steps_of(dtype)
    want = restated(name(dtype), n, weight, controls_key(kw))
    report(label, want, dtype)
    s = solver_of(heavier(p, weight), params, dtype, layout, path)
    if runs:
        assert_path(s, runs)
    return s, want, n


# ---- 1: refused pairs
REFUSED = {np.float64: 0.6, np.float32: 0.76}  # curvature_eps at four times the weights: stored sssss-ss--s- and ss-s


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("config", TWO_PATHS, ids=lambda c: f"{c[0]}-{c[1]}")
def test_a_refused_pair_leaves_the_ring_as_it_was_and_the_next_pair_takes_its_slot(config, dtype):
    """curvature_eps = 0.6 (fp64, 12 iterations: 4 of 12 pairs refused) and 0.76 (fp32, 4 iterations: the third refused, the fourth
    stored): the refused s lies in the free slot, d is written over it and the next pair is formed into the same slot."""
    kw = dict(history=3, curvature_eps=REFUSED[dtype])
    label = f"refused pairs {config[0]}/{config[1]} {name(dtype)}"
    s, want, n = one_slice(config, dtype, 4.0, kw, label)
    stored = want["stored"]
    assert want["pairs_dropped"] > 0 and want["evals"] == want["iters"] == n and want["pairs_dropped"] == stored.count(False)
    assert any(not stored[k] and any(stored[k + 1 :]) for k in range(n)), "no pair is stored after a refusal: choose another threshold"
    check_run(s, s.lbfgs(n, **kw), want, dtype, label)
    s.close()


# ---- 2: a search that starts over along the gradient
RESTARTS = [(config, dtype, dict(max_ls=1, c1=0.5)) for config in TWO_PATHS for dtype in DTYPES] + [(TWO_PATHS[0], np.float64, dict(max_ls=3, c1=0.9))]


@pytest.mark.parametrize("config,dtype,search", RESTARTS, ids=[f"{c[0]}-{c[1]}-{name(d)}-ls{k['max_ls']}" for c, d, k in RESTARTS])
def test_a_search_that_runs_out_drops_the_pairs_and_starts_over_along_the_gradient(config, dtype, search):
    """max_ls = 1, c1 = 0.5: where the quasi-Newton step misses half its predicted fall the pairs go and the iteration's second trial
    runs along -g_k.  max_ls = 3, c1 = 0.9 (fp64): 45 trials in 12 iterations, so the second max_ls rounds of the host's loop run."""
    kw = dict(history=3, **search)
    label = f"restart {config[0]}/{config[1]} {name(dtype)} max_ls={search['max_ls']}"
    s, want, n = one_slice(config, dtype, 4.0, kw, label)
    assert want["evals"] > want["iters"] == n and want["pairs_dropped"] > 0 and want["status"] == 0 and all(want["stored"])
    if search["max_ls"] > 1:
        assert want["evals"] > n + 2 * search["max_ls"]  # (some iteration takes more than max_ls rounds)
    check_run(s, s.lbfgs(n, **kw), want, dtype, label)
    s.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_a_search_starts_over_with_a_frequency_gain_basis(dtype):
    """basis_case("freq") at 16 times the weights, max_ls = 1, c1 = 0.7: the variables are y, the expand pass sits between trial and loss,
    and -g_k is the projected gradient.  The gains after the call equal g0 + B y."""
    p, params, B, _ = basis_case("freq")
    p = heavier(p, 4.0)  # (basis_case gives four times the weights already)
    kw = dict(history=3, max_ls=1, c1=0.7)
    n = steps_of(dtype)
    s = solver_of(p, params, dtype, "shared")
    s.set_gain_basis(B)
    g0, c = cast_params(params, dtype)
    lb = LbfgsRef(Ref(p, dtype=dtype), dtype, g0=g0, B=B)
    want = lb.run(np.zeros(s.get_gain_coeffs()[0].shape, dtype=np.complex128), c, n, **kw)
    want["gains"] = lb.gains_of(want["v"])
    label = f"restart, freq basis {name(dtype)}"
    report(label, want, dtype)
    assert want["evals"] > want["iters"] == n and want["pairs_dropped"] > 0 and want["status"] == 0
    check_run(s, s.lbfgs(n, **kw), want, dtype, label)
    y_r, y_i = s.get_gain_coeffs()
    errs = [relnorm(y_r, want["v"].real), relnorm(y_i, want["v"].imag)]
    print(f"{label}: y_r {errs[0]:.2e}  y_i {errs[1]:.2e}")
    assert max(errs) <= TOL[np.dtype(dtype)]["params"]
    y = np.asarray(y_r, dtype=np.float64) + 1j * np.asarray(y_i, dtype=np.float64)
    g_r, g_i = s.get_params()[:2]
    expanded = LbfgsRef(Ref(p, dtype=dtype), np.float64, g0=g0, B=B.astype(dtype)).gains_of(y)
    assert max(relnorm(g_r, expanded.real), relnorm(g_i, expanded.imag)) <= (1e-6 if dtype == np.float32 else 1e-14)
    s.close()


# ---- 3: slices that take different branches in one call
SEARCH = dict(history=3, max_ls=1, c1=0.5)
BATCH = {np.float64: ((4.0, 32.0, 256.0), 8), np.float32: ((32.0, 4.0, 4.0), FIRST)}  # (the slices' weight factors, iterations)


def weighted_batch(dtype, layout, weights):
    s, parts, pars = three_slices(dtype, layout)
    qs = [heavier(q[0], w) for q, w in zip(parts, weights)]
    s.set_data(*[np.concatenate([np.asarray(getattr(q, k)) for q in qs]) for k in ("data_r", "data_i", "wgts")])
    return s, qs, pars


@functools.lru_cache(maxsize=None)
def batch_wants(dtype_name):
    dtype = np.dtype(dtype_name).type
    weights, n = BATCH[dtype]
    out = []
    for t, w in enumerate(weights):
        q, _, start = synthetic.make_problem(7, 200, f0=150e6, df=400e3, seed=21, data_seed=30 + t)  # (three_slices' own)
        out.append(LbfgsRef(Ref(heavier(q, w), dtype=dtype), dtype).run(*cast_params(start, dtype), n, **SEARCH))
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("layout", ["shared", "stream"])
def test_slices_that_take_different_branches_in_one_call(layout, dtype):
    """three_slices under max_ls = 1, c1 = 0.5.  fp64, weights (4, 32, 256), 8 iterations: slice 0 starts over along -g_k, slice 1 never
    does, slice 2 moves three times, drops its pairs, fails along -g_k too and stalls (status 2) while the others run five more
    iterations: its restore flag is set in one round and lbfgs_restore_kernel runs rounds later.  fp32, weights (32, 4, 4), 4 iterations:
    slice 0 never starts over, slices 1 and 2 do; the stall is not in the fp32 batch because its margin is 9.7e-3 at every weight (the
    trajectory of slice 2 does not depend on the factor from about 128 up), under the 1e-2 an fp32 decision needs.
    Every slice against the restatement of its own problem; on SHARED also bit for bit the single solver of that slice."""
    weights, n = BATCH[dtype]
    wants = batch_wants(name(dtype))
    for t, w in enumerate(wants):
        report(f"slice {t} (weights x {weights[t]:g}) {name(dtype)}", w, dtype)
    restarted = [w["evals"] > w["iters"] and w["status"] == 0 for w in wants]
    assert any(restarted) and any(w["evals"] == w["iters"] == n for w in wants)
    if dtype == np.float64:
        assert restarted[0] and [w["status"] for w in wants] == [0, 0, 2] and 0 < wants[2]["iters"] < n - 1 and wants[2]["evals"] == wants[2]["iters"] + 2
    s, qs, pars = weighted_batch(dtype, layout, weights)
    out = s.lbfgs(n, **SEARCH)
    got = s.get_params()
    na, nc = qs[0].nants, qs[0].ncoeffs
    for t, want in enumerate(wants):
        label = f"slice {t} {layout} {name(dtype)}"
        assert [out[k][t] for k in COUNTERS] == [want[k] for k in COUNTERS], (label, [out[k][t] for k in COUNTERS])
        check_losses(out["losses"][t], want["losses"], dtype, label, upto=want["iters"])
        assert np.all(np.isnan(out["losses"][t][want["iters"] + 1 :])), label
        assert out["loss_after"][t] == out["losses"][t][want["iters"]] and out["loss_before"][t] == out["losses"][t][0], label
        rows, idx = slice(t * na, (t + 1) * na), slice(t * nc, (t + 1) * nc)
        errs = [relnorm(got[0][rows], want["v"].real), relnorm(got[1][rows], want["v"].imag), relnorm(got[2][idx], want["c"].real),
                relnorm(got[3][idx], want["c"].imag)]
        print(f"{label}: " + "  ".join(f"{k} {e:.2e}" for k, e in zip(KEYS, errs)))
        assert max(errs) <= TOL[np.dtype(dtype)]["params"], (label, errs)
    s.eval_loss()
    np.testing.assert_array_equal(s.slice_losses(), out["loss_after"])
    if layout == "shared":
        for t in range(3):
            one = solver_of(qs[t], pars[t], dtype, "shared")
            o1 = one.lbfgs(n, **SEARCH)
            got1 = one.get_params()
            for i in range(4):
                part = slice(t * (na if i < 2 else nc), (t + 1) * (na if i < 2 else nc))
                np.testing.assert_array_equal(got[i][part], got1[i], err_msg=f"slice {t} {KEYS[i]}")
            np.testing.assert_array_equal(o1["losses"][0], out["losses"][t])
            assert [o1[k][0] for k in COUNTERS] == [out[k][t] for k in COUNTERS]
            one.close()
    s.close()


# ---- 4: status 3 for one slice of three
def spoiled(q, how):
    q = copy.copy(q)
    if how == "nan":
        d = np.array(q.data_r)
        b, f = np.argwhere(np.asarray(q.wgts) > 0)[5]
        d[b, f] = np.nan
        q.data_r = d
    else:
        q.wgts = np.zeros_like(np.asarray(q.wgts))
    return q


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
@pytest.mark.parametrize("layout", ["shared", "stream"])
@pytest.mark.parametrize("how", ["nan", "zero_weights"])
def test_a_slice_that_cannot_start_reports_status_3_and_the_others_run_as_if_it_were_masked(how, layout, dtype):
    """Slice 1 of three_slices holds a NaN in its data where its weight is positive (f_0 not finite), or its weights are all zero
    (f_0 = 0, g.g = 0).  Status [0, 3, 0]; slice 1: iters = evals = 0, a losses row of NaN, loss_before = loss_after = NaN (nothing
    is written for status 3), every bit of its gains and coefficients and, under reset_moments, of its moment slots kept.  Slices 0 and
    2 are bit for bit what the same call gives with slice 1 masked out instead.  The NaN is ordinary data: nothing here faults."""
    runs = {}
    for mask in (None, [1, 0, 1]):
        s, parts, pars = three_slices(dtype, layout)
        s.set_optimizer("Adam", learning_rate=1e-2)
        fresh = s.get_moments()
        s.run_slices(4, tol=0.0)  # (on the good data: the moments are no longer what set_optimizer leaves)
        qs = [parts[0][0], spoiled(parts[1][0], how), parts[2][0]]
        s.set_data(*[np.concatenate([np.asarray(getattr(q, k)) for q in qs]) for k in ("data_r", "data_i", "wgts")])
        before, moved = s.get_params(), s.get_moments()
        out = s.lbfgs(5, history=3, slice_mask=mask, reset_moments=True)
        runs[mask is None] = (out, s.get_params(), s.get_moments())
        s.close()
    na, nc = qs[0].nants, qs[0].ncoeffs
    g1 = (np.asarray(before[0], dtype=np.float64) + 1j * np.asarray(before[1], dtype=np.float64))[na : 2 * na]
    c1 = (np.asarray(before[2], dtype=np.float64) + 1j * np.asarray(before[3], dtype=np.float64))[nc : 2 * nc]
    want = LbfgsRef(Ref(qs[1], dtype=dtype), dtype).run(g1, c1, 5, history=3)
    print(f"{how} {layout} {name(dtype)}: the restatement of slice 1: status {want['status']} iters {want['iters']} evals {want['evals']} pairs_dropped {want['pairs_dropped']}")
    assert want["status"] == 3 and want["iters"] == want["evals"] == 0 and np.all(np.isnan(want["losses"]))
    (out, after, mom), (mout, mafter, mmom) = runs[True], runs[False]
    print(f"{how} {layout} {name(dtype)}: status {list(out['status'])} iters {list(out['iters'])} evals {list(out['evals'])} pairs_dropped {list(out['pairs_dropped'])}")
    assert list(out["status"]) == [0, 3, 0] and list(mout["status"]) == [0, 4, 0]
    assert out["iters"][1] == out["evals"][1] == out["pairs_dropped"][1] == 0 and np.all(np.isnan(out["losses"][1]))
    assert np.isnan(out["loss_before"][1]) and np.isnan(out["loss_after"][1])
    for i in range(4):
        n = na if i < 2 else nc
        np.testing.assert_array_equal(after[i][n : 2 * n], before[i][n : 2 * n], err_msg=f"slice 1 {KEYS[i]}")
        for t in (0, 2):
            np.testing.assert_array_equal(after[i][t * n : (t + 1) * n], mafter[i][t * n : (t + 1) * n], err_msg=f"slice {t} {KEYS[i]}")
            assert np.any(after[i][t * n : (t + 1) * n] != before[i][t * n : (t + 1) * n])
    for t in (0, 2):
        np.testing.assert_array_equal(out["losses"][t], mout["losses"][t])
        assert [out[k][t] for k in COUNTERS + ("loss_before", "loss_after")] == [mout[k][t] for k in COUNTERS + ("loss_before", "loss_after")]
        assert out["status"][t] == 0 and out["iters"][t] == 5 and out["loss_after"][t] < out["loss_before"][t]
    for k in ("gm_r", "gm_i", "gv_r", "gv_i", "cm_r", "cm_i", "cv_r", "cv_i"):
        n = na if k[0] == "g" else nc
        for t in range(3):
            part = slice(t * n, (t + 1) * n)
            np.testing.assert_array_equal(mom[k][part], (moved if t == 1 else fresh)[k][part], err_msg=f"{k} of slice {t}")
        np.testing.assert_array_equal(mom[k], mmom[k], err_msg=k)
        assert np.any(moved[k][n : 2 * n] != fresh[k][n : 2 * n]), k
    assert mom["t"] == moved["t"] == 4


# ---- 5: the whole ring
RING = dict(history=16)


@functools.lru_cache(maxsize=None)
def ring_want(dtype_name, nsteps=20, history=16):
    return restated(dtype_name, nsteps, 4.0, controls_key(dict(history=history)))


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_the_whole_ring_of_sixteen_pairs(dtype):
    """base_problem(7, 200) at four times the weights, history = 16, 20 iterations: 17 slots, four tiles of stored pairs in
    lbfgs_pair_kernel from iteration 13 on, evictions at full size from iteration 17 on.  The restatement drops no pair, its smallest
    margin is 4.4e-2 in both dtypes, and history = 16 beats history = 3 at iteration 20 (7.730e-4 against 7.873e-4), so the late slots
    matter to the answer.  fp64: counters, all 21 losses and the parameters.  fp32: counters over all 20 iterations, losses and
    parameters over the first FIRST as usual, and over the full run a bound measured on the reference: the restatement with T = float32
    against T = float64 differs by at most 2.7e-6 of the loss over the 21 values; the device may differ from the float32 restatement by
    ten times that (it adds in another order than NumPy; a wrong dot product in a late tile moves the leading digits)."""
    want = ring_want(name(dtype))
    label = f"history 16 {name(dtype)}"
    report(label, want, dtype)
    short = ring_want("float64", history=3)
    print(f"{label}: the restatement at iteration 20: history 16 {ring_want('float64')['losses'][20]:.4e}, history 3 {short['losses'][20]:.4e}")
    assert want["pairs_dropped"] == 0 and want["iters"] == want["evals"] == 20 and all(want["stored"])
    assert ring_want("float64")["losses"][20] < short["losses"][20] and short["margin"] >= 1e-6
    p, params = base_problem(*SHAPE)
    s = solver_of(heavier(p, 4.0), params, dtype, "stream")
    out = s.lbfgs(20, **RING)
    for k in COUNTERS:
        assert out[k][0] == want[k], (label, k, out[k][0], want[k])
    if dtype == np.float64:
        check_run(s, out, want, dtype, label)
        s.close()
        return
    w64 = ring_want("float64")["losses"]
    measured = float(np.max(np.abs(want["losses"] - w64) / np.abs(w64)))
    err = float(np.max(np.abs(out["losses"][0] - want["losses"]) / np.abs(want["losses"])))
    print(f"{label}: losses over 20 iterations {err:.2e}; the restatement with T = float32 against T = float64 {measured:.2e}, bound {10 * measured:.2e}")
    assert np.all(np.isfinite(out["losses"][0])) and 0.0 < measured < 1e-5 and err <= 10.0 * measured, (label, err, measured)
    check_losses(out["losses"][0], want["losses"], dtype, label, upto=FIRST)
    s.set_params(*[params[k] for k in KEYS])
    first = restated(name(dtype), FIRST, 4.0, controls_key(RING))
    assert first["margin"] >= TOL[np.dtype(dtype)]["margin"]
    check_run(s, s.lbfgs(FIRST, **RING), first, dtype, label + f" ({FIRST} iterations)")
    s.close()


# ---- 6: past 64 blocks a slice
BIG_WEIGHT = 32.0


@functools.lru_cache(maxsize=None)
def big_problem():
    p, _, start = synthetic.make_problem(64, 1024, f0=150e6, df=100e3, seed=4)
    return heavier(p, BIG_WEIGHT), start


@functools.lru_cache(maxsize=None)
def big_ref(dtype_name):
    return Ref(big_problem()[0], dtype=np.dtype(dtype_name).type)


@pytest.mark.parametrize("dtype", DTYPES, ids=name)
def test_a_slice_of_more_than_64_blocks(dtype):
    """make_problem(64, 1024): 131 072 gain reals and 99 917 complex coefficients a slice, 162 blocks in fp64 and 81 in fp32 by lb_cut's
    rule (asserted from the sizes, so a change of kLbChunksPerThread fails here instead of testing nothing): every lane of
    lbfgs_reduce_kernel makes a second trip and the partials of blocks >= 64 are read.  Three iterations at history = 2 from the
    problem's own start, 32 times the weights (the restatement's margin 1.2e-2 in both dtypes).  This is the one test of the file that
    takes seconds: the restatement's three iterations over 2016 baselines x 1024 channels cost about one second each on the CPU."""
    p, start = big_problem()
    size = np.dtype(dtype).itemsize
    V = 16 // size
    s = solver_of(p, start, dtype, "shared")
    before = s.memory_bytes()
    ngs, nco = 2 * p.nants * 1024, p.ncoeffs  # (1024 channels: rows without padding)
    chunks = -(-ngs // V) + 2 * -(-nco // V)
    nblk = -(-chunks // 1024)
    assert (ngs, nco, nblk) == (131072, 99917, 162 if dtype == np.float64 else 81) and nblk > 64
    g, c = cast_params(start, dtype)
    want = LbfgsRef(big_ref(name(dtype)), dtype).run(g, c, 3, history=2)
    label = f"64 x 1024, {nblk} blocks, {name(dtype)}"
    report(label, want, dtype)
    assert want["iters"] == 3 and want["status"] == 0
    out = s.lbfgs(3, history=2)
    assert s.memory_bytes() - before >= (2 * 2 + 4) * (ngs + 2 * nco) * size  # (the vectors are as long as the block count assumes)
    check_run(s, out, want, dtype, label)
    s.close()
