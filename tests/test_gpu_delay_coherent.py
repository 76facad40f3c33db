"""cal_solver_delay_coherent_spectrum on the device against the float64 restatement of the header text (tests/delay_coherent_ref.py),
at the smallest shapes that reach every branch, built on test_gpu_delay_cross.batch / solver_of / operator (imported): slices of
make_problem(7, 61) in ONE solver (21 rows per slice, 37 delays), of make_problem(7, 200) (200 delays; in fp64 a set goes past one
128-channel span of a wave), the two-slice problems of test_gpu_row_walk_shapes at 5 and 260 channels (past one 256-channel span in
fp32), and make_problem(13, 61) for more than 64 groups.

Every set list holds singletons, a pair, a whole slice's rows, a set of 70 members with rows repeated across slices (more members than
a wave has lanes), a set with one member flagged throughout which the others carry, an EMPTY set, a group whose sets' masks are
disjoint across t, conjugated members mixed with plain ones, unequal coefficients (one of them zero) and unequal scales; T = 1, 2, 3.

The bound is derived, not tuned (delay_coherent_ref.py).  Every case prints its largest ratio of error to bound."""
import copy
import ctypes as C

import numpy as np
import pytest

import test_gpu_delay_cross as DC
import test_gpu_delay_fringe as DF
import test_gpu_delay_spectrum as DS
import test_gpu_row_walk_shapes as RW
from calamity_amd import _lib, modeling
from delay_coherent_ref import bound_ratio, restated, sets_of, singleton_sets
from delay_fringe_ref import bin_groups
from delay_spectrum_ref import NAMES, model_of
from test_gpu_robust_consumers import CLIP
from test_gpu_solve_paths import PATHS, assert_path, path_id, path_solver

pytestmark = pytest.mark.gpu

cast = DC.cast
batch, joined, solver_of, operator = DC.batch, DC.joined, DC.solver_of, DC.operator
GENERAL, config_id = DS.GENERAL, DS.config_id
WEIGHTING = ("uniform", "weights")


def set_list(nb, S, T, singles=(0, 2, 4, 5), seed=6):
    """A description of groups of T sets on S slices of nb rows each (row 1 of slice 0 flagged wholly, row 3 of the slices 0 and 1
    with disjoint masks): ``dict(set_ptr, member_row, member_wgt, member_conj, scale, bins, nbins, pos, ngroups, T)``.  Set t of a
    group sits in slice t % S."""
    sl = [(t % S) * nb for t in range(T)]
    groups = [[[o + b] for o in sl] for b in singles]
    pos = {}

    def add(name, g):
        pos[name] = len(groups)
        groups.append(g)

    add("pair", [[o + 6, o + 7] for o in sl])
    add("slice", [[o + b for b in range(nb)] for o in sl])
    add("seventy", [[((k + t) % S) * nb + (5 * k + t) % nb for k in range(70)] for t in range(T)])
    add("carried", [[o + 8, 1, o + 9] for o in sl])  # row 1 of slice 0: flagged throughout
    add("empty", [[] if t == 0 else [o + 10] for t, o in enumerate(sl)])
    # T = 1 has no second set to be disjoint from: its one set is then the row flagged throughout
    add("disjoint", [[3] if t % 2 == 0 else [nb + 3] for t in range(T)] if T > 1 else [[1]])
    add("conj", [[o + 9, o + 10, o + 11] for o in sl])
    set_ptr, member_row, ng, _ = sets_of(groups)
    rng = np.random.default_rng(seed)
    wgt = rng.uniform(0.5, 2.0, size=len(member_row))
    cj = np.zeros(len(member_row), dtype=np.uint8)
    first = lambda name, t=0: set_ptr[pos[name] * T + t]  # noqa: E731
    cj[first("conj")], cj[first("conj") + 2] = 1, 1
    cj[first("seventy") + 3 : first("seventy") + 70 : 7] = 1
    wgt[first("slice") + 2] = 0.0  # a member that counts for nothing
    scale = rng.uniform(0.5, 2.0, size=(ng, T))
    bins = (np.arange(ng) % 3).astype(np.int32)
    bins[1] = -1
    return dict(set_ptr=set_ptr, member_row=member_row, member_wgt=wgt, member_conj=cj, scale=scale, bins=bins, nbins=4, pos=pos, ngroups=ng, T=T)


def sets_kw(L):
    return dict(member_wgt=L["member_wgt"], member_conj=L["member_conj"], scale=L["scale"], bin_of_group=L["bins"], nbins=L["nbins"])


def time_operator(T):
    return DF.time_operator(T)


def inputs(full, p0, pars, dtype, w=None):
    d = cast(full.data_r, dtype) + 1j * cast(full.data_i, dtype)
    m = np.concatenate([model_of(p0, q["c_r"], q["c_i"], dtype) for q in pars])
    gains = [cast(q["g_r"], dtype) + 1j * cast(q["g_i"], dtype) for q in pars]
    G = np.concatenate([g[p0.bl_ant0] * np.conj(g[p0.bl_ant1]) for g in gains])
    return d, m, G, cast(full.wgts if w is None else w, dtype)


def reference(full, p0, pars, dtype, op, norm_f, L, opt, weighting, calibrated=False, w=None):
    """The restatement from the inputs rounded to ``dtype``; ``pars``: the parameters of every slice (p0's shapes)."""
    d, m, G, wd = inputs(full, p0, pars, dtype, w)
    op_t = cast(op.real, dtype) + 1j * cast(op.imag, dtype)
    return restated(d, m, G, wd, op_t, norm_f, L["set_ptr"], L["member_row"], opt, L["member_wgt"], L["member_conj"], WEIGHTING.index(weighting),
                    L["scale"], calibrated, L["bins"], L["nbins"])


def assert_not_vacuous(ref, L, nfreqs):
    """A condition on the host, before the device is asked: the empty and the disjoint group have an empty common mask, every other
    group keeps at least a third of its channels."""
    kept = ref["common"].sum(axis=1)
    empty = [L["pos"]["empty"], L["pos"]["disjoint"]]
    assert not np.any(kept[empty])
    assert np.all(np.delete(kept, empty) * 3 >= nfreqs), kept


def check(out, ref, dtype, label, L, names=NAMES):
    worst = {}
    for k in names:
        P = out["per_group"][k]
        assert P.dtype == np.float64 and P.shape == ref["per_group"][k].shape and np.all(np.isfinite(P)) and np.all(P >= 0), (label, k)
        worst[k] = bound_ratio(P, ref, k, dtype)
    print(f"{label}: error / bound  " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, (label, worst)
    np.testing.assert_allclose(out["norm_grp"], ref["norm_grp"], rtol=1e-13, atol=0)
    np.testing.assert_array_equal(out["count_bin"], ref["count_bin"])
    # the bins against the sequential double sum of the device's own groups, ascending: the same additions
    own = bin_groups({k: out["per_group"][k] for k in names}, out["norm_grp"], L["bins"], L["nbins"])
    for k in names:
        np.testing.assert_array_equal(out[k], own[k], err_msg=f"{label}: bins of {k}")
        assert np.any(out[k][0]) and not np.any(out[k][L["nbins"] - 1]) and out["count_bin"][L["nbins"] - 1] == 0  # a bin without groups
    for z in ("empty", "disjoint"):
        g = L["pos"][z]
        assert out["norm_grp"][g] == 0 and not any(np.any(out["per_group"][k][g]) for k in names), (label, z)
    for z in ("pair", "slice", "seventy", "carried", "conj"):
        g = L["pos"][z]
        assert out["norm_grp"][g] > 0 and all(np.any(out["per_group"][k][g]) for k in names), (label, z)
    return worst


def run_case(s, full, p0, pars, dtype, op, norm_f, L, label, weighting, calibrated=False, w=None):
    opt = time_operator(L["T"])
    ref = reference(full, p0, pars, dtype, op, norm_f, L, opt, weighting, calibrated, w)
    assert_not_vacuous(ref, L, p0.nfreqs)
    out = s.delay_coherent_spectrum(op, norm_f, L["set_ptr"], L["member_row"], opt, weighting=weighting, calibrated=calibrated, per_group=True,
                                    **sets_kw(L))
    check(out, ref, dtype, label, L)
    return out


@pytest.mark.parametrize("config", GENERAL, ids=config_id)
@pytest.mark.parametrize("shape,S,T,ndelays", [((7, 61), 3, 3, 37), ((7, 61), 3, 1, 37), ((7, 200), 2, 2, 200)])
@pytest.mark.parametrize("calibrated", [False, True], ids=["raw", "calibrated"])
def test_parity_with_the_restatement(shape, S, T, ndelays, calibrated, config):
    dtype, layout, path = config
    full, p0, pars = batch(*shape, S)
    assert p0.nbls == 21
    op, norm_f = operator(shape[1], ndelays)
    L = set_list(p0.nbls, S, T)
    s = solver_of(full, joined(pars), dtype, layout, path)
    for weighting in WEIGHTING:
        label = f"{shape} x{S} T={T} {ndelays} {config_id(config)} calibrated={calibrated} {weighting}"
        out = run_case(s, full, p0, pars, dtype, op, norm_f, L, label, weighting, calibrated)
        assert out["per_group"]["data"].shape == (L["ngroups"], T, ndelays)
    s.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_more_than_64_groups(dtype):
    full, p0, pars = batch(13, 61, 2)
    assert p0.nbls == 78
    op, norm_f = operator(61, 37)
    L = set_list(p0.nbls, 2, 2, singles=[b for b in range(78) if b not in (1, 3)])
    assert L["ngroups"] > 64
    s = solver_of(full, joined(pars), dtype)
    run_case(s, full, p0, pars, dtype, op, norm_f, L, f"(13, 61) x2 37 {np.dtype(dtype).name}", "weights")
    s.close()


def flagged_like_the_batches(full, nb):
    """The two-slice problem of test_gpu_row_walk_shapes with the special rows of test_gpu_delay_cross.batch: row 1 of slice 0 flagged
    wholly, row 3 of the slices 0 and 1 with disjoint masks.  A copy: the cached problem stays as it is."""
    out = copy.copy(full)
    w = np.array(full.wgts, copy=True)
    w[1] = 0.0
    w[3, 1::2] = 0.0
    w[nb + 3, 0::2] = 0.0
    out.wgts = w
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("nfreqs", RW.NFREQS)
def test_row_walk_shapes(nfreqs, dtype):
    """nfreqs = 5: fpad = 8 under a pitch of 32 (the channels [fpad, xpitch) are zeroed without loads, most lanes of the one span idle);
    nfreqs = 260: fpad = 384, a second span of the set in fp32 and a third in fp64.  All nfreqs delays."""
    cached, parts, params, _ = RW.batch(nfreqs)
    p0, nb = parts[0], parts[0].nbls
    full = flagged_like_the_batches(cached, nb)
    op, norm_f, _ = modeling.delay_transform(150e6 + 400e3 * np.arange(nfreqs))
    pars = [RW.sliced(params, t, p0) for t in range(RW.T)]
    L = set_list(nb, RW.T, 2)
    s = RW.solver_of(full, params, dtype)
    for calibrated, weighting in ((False, "uniform"), (True, "weights")):
        run_case(s, full, p0, pars, dtype, op, norm_f, L, f"row walk {nfreqs} {np.dtype(dtype).name} calibrated={calibrated} {weighting}", weighting,
                 calibrated)
    s.close()


# ---- every kernel path
@pytest.mark.parametrize("dtype,path", PATHS, ids=map(path_id, PATHS))
def test_every_kernel_path(dtype, path):
    """Sets among the rows of ONE slice: what the kernel path can change is the model pass."""
    p, params = DS.problem(7, 200)
    op, norm_f = operator(200, 200)
    nb = p.nbls
    groups = [[[(b + 3 * t) % nb] for t in range(2)] for b in (0, 2, 4)] + [[[5, 6, 7], [8, 9]], [list(range(nb)), list(range(nb))[::-1]]]
    set_ptr, member_row, ng, T = sets_of(groups)
    opt = time_operator(T)
    rng = np.random.default_rng(4)
    L = dict(set_ptr=set_ptr, member_row=member_row, member_wgt=rng.uniform(0.5, 2.0, len(member_row)),
             member_conj=(rng.random(len(member_row)) < 0.3).astype(np.uint8), scale=rng.uniform(0.5, 2.0, (ng, T)),
             bins=np.array([0, 1, 0, 1, -1], dtype=np.int32), nbins=2)
    outs = {}
    for which in dict.fromkeys((path, "general")):
        s = path_solver(p, params, dtype, which)
        assert_path(s, which)
        outs[which] = s.delay_coherent_spectrum(op, norm_f, set_ptr, member_row, opt, weighting="weights", per_group=True, **sets_kw(L))
        s.close()
    ref = reference(p, p, [params], dtype, op, norm_f, L, opt, "weights")
    assert np.count_nonzero(ref["norm_grp"]) == ng
    worst = {k: bound_ratio(outs[path]["per_group"][k], ref, k, dtype) for k in NAMES}
    print(f"(7, 200) 200 {path_id((dtype, path))}: error / bound  " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst
    for k in NAMES:  # the model pass and everything behind it are those of the general path: the same bits
        np.testing.assert_array_equal(outs[path]["per_group"][k], outs["general"]["per_group"][k])
        np.testing.assert_array_equal(outs[path][k], outs["general"][k])


# ---- the properties of the header text, to the bit
def same_bits(a, b, names=NAMES, label=""):
    np.testing.assert_array_equal(a["norm_grp"], b["norm_grp"], err_msg=label)
    if "count_bin" in a:
        np.testing.assert_array_equal(a["count_bin"], b["count_bin"], err_msg=label)
    for k in names:
        np.testing.assert_array_equal(a["per_group"][k], b["per_group"][k], err_msg=f"{label} {k}")
        if k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"{label} bins of {k}")


@pytest.mark.parametrize("calibrated", [False, True], ids=["raw", "calibrated"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape,S,T", [((7, 61), 3, 3), ((7, 200), 2, 2), ((7, 61), 3, 1)])
def test_singleton_sets_are_the_fringe_spectrum_to_the_bit(shape, S, T, dtype, calibrated):
    """(a): every set one member, unit coefficient, no conjugation, uniform weighting: delay_fringe_spectrum on the same solver."""
    full, p0, pars = batch(*shape, S)
    op, norm_f = operator(shape[1], 37)
    rows, scale, pos = DF.group_list(p0.nbls, S, T)
    bins, nbins = DF.bins_of_groups(len(rows))
    opt = time_operator(T)
    set_ptr, member_row = singleton_sets(rows)
    s = solver_of(full, joined(pars), dtype)
    kw = dict(scale=scale, calibrated=calibrated, bin_of_group=bins, nbins=nbins, per_group=True)
    want = s.delay_fringe_spectrum(op, norm_f, rows, opt, **kw)
    for wgt, cj in ((None, None), (np.ones(len(member_row)), np.zeros(len(member_row), dtype=np.uint8))):
        got = s.delay_coherent_spectrum(op, norm_f, set_ptr, member_row, opt, member_wgt=wgt, member_conj=cj, **kw)
        same_bits(got, want)
    assert np.count_nonzero(want["norm_grp"]) >= len(rows) - 2 and np.any(want["per_group"]["resid"])
    s.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_row_twice_is_the_row_once(dtype):
    """(b): (q + q) / 2 is exact."""
    full, p0, pars = batch(7, 61, 3)
    op, norm_f = operator(61, 37)
    rows, scale, pos = DF.group_list(p0.nbls, 3, 3)
    opt = time_operator(3)
    set_ptr, member_row = singleton_sets(rows)
    s = solver_of(full, joined(pars), dtype)
    once = s.delay_coherent_spectrum(op, norm_f, set_ptr, member_row, opt, scale=scale, per_group=True)
    twice = s.delay_coherent_spectrum(op, norm_f, 2 * set_ptr, np.repeat(member_row, 2), opt, scale=scale, per_group=True)
    same_bits(once, twice)
    assert np.any(once["per_group"]["data"])
    s.close()


@pytest.mark.parametrize("calibrated", [False, True], ids=["raw", "calibrated"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_conjugated_sets_under_the_conjugated_operator(dtype, calibrated):
    """(c): T = 1, opt = [[1]], singleton sets all conjugated and conj(op): the bits of the plain sets with op."""
    full, p0, pars = batch(7, 61, 2)
    op, norm_f = operator(61, 37)
    member_row = np.arange(full.nbls, dtype=np.int32)
    set_ptr = np.arange(full.nbls + 1, dtype=np.int64)
    s = solver_of(full, joined(pars), dtype)
    plain = s.delay_coherent_spectrum(op, norm_f, set_ptr, member_row, np.ones((1, 1)), calibrated=calibrated, per_group=True)
    conj = s.delay_coherent_spectrum(np.conj(op), norm_f, set_ptr, member_row, np.ones((1, 1)), member_conj=np.ones(full.nbls, dtype=np.uint8),
                                     calibrated=calibrated, per_group=True)
    same_bits(plain, conj)
    other = s.delay_coherent_spectrum(op, norm_f, set_ptr, member_row, np.ones((1, 1)), member_conj=np.ones(full.nbls, dtype=np.uint8),
                                      calibrated=calibrated, per_group=True)
    assert np.any(other["per_group"]["data"] != plain["per_group"]["data"])  # (the flag does something)
    s.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape,S,T,ndelays", [((7, 61), 3, 3, 37), ((7, 200), 2, 2, 61)])
def test_chunks_and_repeated_calls_give_the_same_bits(shape, S, T, ndelays, dtype):
    """(d) and (e)."""
    full, p0, pars = batch(*shape, S)
    op, norm_f = operator(shape[1], ndelays)
    L = set_list(p0.nbls, S, T)
    opt = time_operator(T)
    s = solver_of(full, joined(pars), dtype)
    call = lambda: s.delay_coherent_spectrum(op, norm_f, L["set_ptr"], L["member_row"], opt, weighting="weights", per_group=True, **sets_kw(L))  # noqa: E731
    one = call()
    same_bits(one, call(), label="again")
    xpitch = -(-shape[1] // 32) * 32
    per_group = 3 * 2 * T * xpitch * np.dtype(dtype).itemsize + T * xpitch + 3 * 2 * T * ndelays * 8 + 3 * T * ndelays * 8
    for ngrp in (4, 1):
        s._set_delay_spectrum_scratch(ngrp * per_group + per_group // 2)
        same_bits(one, call(), label=f"{ngrp} groups per chunk")
    s._set_delay_spectrum_scratch(1)  # below one group: one group per chunk
    same_bits(one, call(), label="a bound of one byte")
    s._set_delay_spectrum_scratch(0)
    s.close()


@pytest.mark.parametrize("config", ["adam", "graph", "gain_basis"])
def test_a_run_continued_after_the_call_is_bit_identical(config):
    """(f)."""
    full, p0, pars = batch(7, 61, 2)
    op, norm_f = operator(61, 37)
    L = set_list(p0.nbls, 2, 2)
    opt = time_operator(2)
    losses, final = {}, {}
    for with_call in (False, True):
        s = solver_of(full, joined(pars), np.float32)
        if config == "gain_basis":
            s.set_gain_basis(np.array(modeling.gain_dpss_basis(DC.F0 + DC.DF * np.arange(p0.nfreqs), 100.0)))
        s.set_launch_mode("graph" if config == "graph" else "auto")
        s.set_optimizer("Adam", learning_rate=1e-2)
        first = np.array([r[0] for r in s.run_slices(20, tol=0.0)])
        if with_call:
            out = s.delay_coherent_spectrum(op, norm_f, L["set_ptr"], L["member_row"], opt, per_group=True, **sets_kw(L))
            assert out["per_group"]["resid"].sum() > 0
        second = np.array([r[0] for r in s.run_slices(20, tol=0.0)])
        losses[with_call] = np.concatenate([first, second], axis=1)
        final[with_call] = s.get_params()
        s.close()
    assert losses[True].shape == (2, 40)
    np.testing.assert_array_equal(losses[True], losses[False])
    for a, b in zip(final[True], final[False]):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_report_reads_the_rewritten_weight_plane(dtype):
    """After robust_weights("clip") the report is the restatement on the rewritten plane -- its values too, under weighting="weights"."""
    full, p0, pars = batch(7, 61, 3)
    op, norm_f = operator(61, 37)
    L = set_list(p0.nbls, 3, 3)
    opt = time_operator(3)
    s = solver_of(full, joined(pars), dtype)
    s.robust_weights(*CLIP)
    w, w0 = s.get_weights(0), s.get_weights(1)
    assert np.any((w == 0) != (w0 == 0))
    out = s.delay_coherent_spectrum(op, norm_f, L["set_ptr"], L["member_row"], opt, weighting="weights", per_group=True, **sets_kw(L))
    s.close()
    new = reference(full, p0, pars, dtype, op, norm_f, L, opt, "weights", w=w)
    old = reference(full, p0, pars, dtype, op, norm_f, L, opt, "weights", w=w0)
    check(out, new, dtype, f"behind clip {np.dtype(dtype).name}", L)
    moved = new["norm_grp"] != old["norm_grp"]
    assert np.any(moved) and np.all(out["norm_grp"][moved] != old["norm_grp"][moved])


def test_each_quantity_alone_and_each_output_alone():
    full, p0, pars = batch(7, 61, 3)
    op, norm_f = operator(61, 37)
    L = set_list(p0.nbls, 3, 3)
    opt = time_operator(3)
    s = solver_of(full, joined(pars), np.float32)
    args = (op, norm_f, L["set_ptr"], L["member_row"], opt)
    everything = s.delay_coherent_spectrum(*args, per_group=True, **sets_kw(L))
    for what in (("data",), ("model",), ("resid",), ("resid", "data")):
        one = s.delay_coherent_spectrum(*args, what=what, per_group=True, **sets_kw(L))
        assert set(one["per_group"]) == set(what) and set(one) == set(what) | {"norm_grp", "count_bin", "per_group"}
        same_bits(one, everything, names=what, label=str(what))
    only_bins = s.delay_coherent_spectrum(*args, **sets_kw(L))
    assert "per_group" not in only_bins
    for k in NAMES:
        np.testing.assert_array_equal(only_bins[k], everything[k])
    s.close()


def test_errors_are_reported():
    """Every refusal returns its code and message; nothing is launched (the outputs keep their bytes)."""
    full, p0, pars = batch(7, 61, 2)
    op, norm_f = operator(61, 37)
    params = joined(pars)
    s = solver_of(full, params, np.float64)
    op_r, op_i = np.ascontiguousarray(op.real), np.ascontiguousarray(op.imag)
    set_ptr = np.array([0, 2, 3, 3, 5], dtype=np.int64)
    rows = np.array([0, p0.nbls, 2, 4, 4], dtype=np.int32)
    wgt, cj = np.ones(5), np.zeros(5, dtype=np.uint8)
    opt_r, opt_i = np.array([[1.0, 1.0], [1.0, -1.0]]), np.zeros((2, 2))
    bins = np.zeros(2, dtype=np.int32)
    norm = np.full(2, -7.0)
    buf = np.full((3, 2, 2, 37), -7.0)
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731

    def code(ndelays=37, what=7, calibrated=0, ngroups=2, ntimes=2, nrates=2, set_ptr=set_ptr, rows=rows, wgt=None, cj=None, weighting=0, scale=None, nbins=0,
             bin_of_group=None, op_r=op_r, norm_f=norm_f, opt_r=opt_r, opt_i=opt_i, nmembers=5, power_bin=None):
        d = _lib.DelayCoherentDesc(ndelays, what, calibrated, ngroups, ntimes, nrates, ptr(set_ptr), ptr(rows), ptr(wgt), ptr(cj), weighting, ptr(scale), nbins,
                                   ptr(bin_of_group), ptr(op_r), op_i.ctypes.data, ptr(norm_f), ptr(opt_r), ptr(opt_i), nmembers)
        return s._lib.cal_solver_delay_coherent_spectrum(s._h, C.byref(d), None, None, buf.ctypes.data, norm.ctypes.data, ptr(power_bin), None)

    def refused(message, **kw):
        norm[:], buf[:] = -7.0, -7.0
        assert code(**kw) == _lib.CAL_ERR_INVALID, kw
        got = s._lib.cal_last_error().decode()
        assert got == "delay_coherent_spectrum: " + message, got
        assert np.all(norm == -7.0) and np.all(buf == -7.0)  # nothing was launched

    assert code() == 0 and code(wgt=wgt, cj=cj, weighting=1, scale=np.ones((2, 2))) == 0
    assert norm[0] > 0 and norm[1] == 0  # (group 1 holds an empty set)
    refused("what = 0: bits 0 (data), 1 (model), 2 (residual), at least one", what=0)
    refused("ndelays = 4097 lies outside [1, 4096]", ndelays=4097)
    refused("calibrated = 2 (0 or 1)", calibrated=2)
    refused("null operator or norm_f", op_r=None)
    refused("binned outputs need nbins > 0", power_bin=buf)
    refused("bin_of_group goes with nbins > 0, and only with it", nbins=2)
    refused("ngroups = 0 (at least 1)", ngroups=0)
    refused("ntimes = 65 lies outside [1, 64]", ntimes=65)
    refused("nrates = 0 lies outside [1, 64]", nrates=0)
    refused("null opt", opt_i=None)
    refused("null set_ptr", set_ptr=None)
    refused("null member_row", rows=None)
    refused("weighting = 2 (0: the coefficients, 1: coefficients times weights)", weighting=2)
    refused("nmembers = 1073741825 lies outside [0, 2^30]", nmembers=(1 << 30) + 1)
    refused("nmembers = -1 lies outside [0, 2^30]", nmembers=-1)
    refused("set_ptr[0] = 1 (it starts at 0)", set_ptr=np.array([1, 2, 3, 3, 5], dtype=np.int64))
    refused("set_ptr[2] = 1 falls below set_ptr[1] = 2", set_ptr=np.array([0, 2, 1, 3, 5], dtype=np.int64))
    refused("set_ptr ends at 4, not at nmembers = 5", set_ptr=np.array([0, 2, 3, 3, 4], dtype=np.int64))
    refused("set_ptr ends at 5, not at nmembers = 4", nmembers=4)
    refused(f"member_row[4] = {full.nbls} lies outside [0, {full.nbls})", rows=np.array([0, 1, 2, 4, full.nbls], dtype=np.int32))
    refused(f"member_row[0] = -1 lies outside [0, {full.nbls})", rows=np.array([-1, 1, 2, 4, 4], dtype=np.int32))
    for v in (-1.0, np.inf, np.nan):
        refused("member_wgt[3] is negative or not finite", wgt=np.array([1.0, 1.0, 1.0, v, 1.0]))
    refused("member_conj[1] = 2 (0 or 1)", cj=np.array([0, 2, 0, 0, 0], dtype=np.uint8))
    refused("scale[1][0] is not finite", scale=np.array([[1.0, 1.0], [np.nan, 1.0]]))
    refused("opt[1][0] is not finite", opt_r=np.array([[1.0, 1.0], [np.inf, -1.0]]))
    bins[1] = 2
    refused("bin_of_group[1] = 2 lies outside [-1, 2)", nbins=2, bin_of_group=bins)
    assert s._lib.cal_solver_delay_coherent_spectrum(s._h, None, None, None, None, None, None, None) == _lib.CAL_ERR_INVALID
    s.close()
    # state: gains neither set nor given
    from calamity_amd.solver import HipFitSolver

    s = HipFitSolver(dtype=np.float64)
    s.set_problem(full)
    s.set_data(full.data_r, full.data_i, full.wgts)
    s.set_params(c_r=params["c_r"], c_i=params["c_i"])
    with pytest.raises(_lib.CalamityHipError) as err:
        s.delay_coherent_spectrum(op, norm_f, set_ptr, rows, opt_r)
    assert err.value.code == _lib.CAL_ERR_STATE
    assert s.delay_coherent_spectrum(op, norm_f, set_ptr, rows, opt_r, g_r=params["g_r"], g_i=params["g_i"])["norm_grp"][0] > 0
    s.close()
