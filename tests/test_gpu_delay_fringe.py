"""cal_solver_delay_fringe_spectrum on the device against the float64 restatement of the header text (tests/delay_fringe_ref.py), at the
smallest shapes that reach every branch, built on test_gpu_delay_cross.batch (imported): slices of make_problem(7, 61) in ONE solver
(21 rows per slice; 37 delays: a partial column block, and 61; all rates and a subset of 2), of make_problem(7, 200) (200 delays: four
column blocks, the last ragged), of make_problem(13, 61) (78 groups: past 64), four slices of (7, 61) under T = 5, 17 and 64 (past the
16-row tile, and the limit; their groups cycle over the four slices, so the common mask stays populated), and the two-slice problems of
test_gpu_row_walk_shapes at 5 and 260 channels.

Every group list holds: the same-baseline groups, a group of one repeated row, a group in reversed order, a group with one row flagged
throughout (power 0, no bin), a group whose rows' masks are disjoint (the same), and unequal scales.

The bound is derived, not tuned (delay_fringe_ref.py).  Every case prints its largest ratio of error to bound."""
import numpy as np
import pytest

import test_gpu_delay_cross as DC
import test_gpu_delay_spectrum as DS
import test_gpu_row_walk_shapes as RW
from calamity_amd import _lib, modeling
from delay_fringe_ref import bin_groups, bound_plane, bound_ratio, common_mask, restated
from delay_spectrum_ref import NAMES, model_of
from test_gpu_robust_consumers import CLIP
from test_gpu_solve_paths import PATHS, assert_path, path_id, path_solver

pytestmark = pytest.mark.gpu

cast = DC.cast
batch, joined, solver_of, operator = DC.batch, DC.joined, DC.solver_of, DC.operator
GENERAL, config_id = DS.GENERAL, DS.config_id
U64 = 2.0 ** -53


def group_list(nb, S, T, seed=5):
    """(rows [ngroups, T], scale, named positions) on S slices of nb rows: group b of the first nb is baseline b at the slices
    t % S, t = 0 .. T - 1 (batch() flags row 1 of slice 0 wholly and gives row 3 of the slices 0 and 1 disjoint masks); "mixed" joins
    two baselines.  No group holds more than four distinct rows."""
    same = [[(t % S) * nb + b for t in range(T)] for b in range(nb)]
    extra = {"repeated": [nb + 2] * T, "reversed": same[4][::-1], "mixed": [((t + 1) % S) * nb + 5 + t % 2 for t in range(T)]}
    rows = np.array(same + list(extra.values()), dtype=np.int32)
    pos = {k: nb + i for i, k in enumerate(extra)}
    pos.update(forward=4, flagged=1, disjoint=3)
    scale = np.random.default_rng(seed).uniform(0.5, 2.0, size=rows.shape)
    scale[pos["reversed"]] = scale[pos["forward"]][::-1]
    return rows, scale, pos


def bins_of_groups(ngroups, nbins=4):
    """Groups dealt over the bins 0 .. nbins - 2 (bin nbins - 1 stays empty); group 5 is left out (-1)."""
    b = (np.arange(ngroups) % (nbins - 1)).astype(np.int32)
    b[5] = -1
    return b, nbins


def time_operator(T, rates=None, seed=9):
    """A tapered DFT along time with a seeded complex gain per time, so that no symmetry of the operator hides an error of order."""
    opt, _ = modeling.fringe_rate_transform(T, 10.0, taper="none")
    rng = np.random.default_rng(seed)
    opt = opt * (1.0 + 0.2 * rng.standard_normal((T, 1)) + 0.2j * rng.standard_normal((T, 1)))
    return np.ascontiguousarray(opt if rates is None else opt[:, rates])


def reference(full, p0, pars, dtype, op, norm_f, rows, opt, scale, calibrated=False, bins=None, nbins=0, w=None):
    """The restatement from the inputs rounded to ``dtype``; ``pars``: the parameters of every slice (p0's shapes)."""
    d = cast(full.data_r, dtype) + 1j * cast(full.data_i, dtype)
    m = np.concatenate([model_of(p0, q["c_r"], q["c_i"], dtype) for q in pars])
    gains = [cast(q["g_r"], dtype) + 1j * cast(q["g_i"], dtype) for q in pars]
    G = np.concatenate([g[p0.bl_ant0] * np.conj(g[p0.bl_ant1]) for g in gains])
    op_t = cast(op.real, dtype) + 1j * cast(op.imag, dtype)
    return restated(d, m, G, cast(full.wgts if w is None else w, dtype), op_t, norm_f, rows, opt, scale, calibrated, bins, nbins)


def assert_not_vacuous(w, rows, pos):
    """On the host, before the device is asked: the flagged and the disjoint group have an empty common mask, every other group keeps
    at least a third of its channels."""
    kept = common_mask(w, rows).sum(axis=1)
    empty = [pos["flagged"], pos["disjoint"]]
    assert not np.any(kept[empty])
    assert np.all(np.delete(kept, empty) * 3 >= np.asarray(w).shape[1]), kept


def check(out, ref, dtype, label, names=NAMES, bins=None, nbins=0):
    worst = {}
    for k in names:
        P = out["per_group"][k]
        assert P.dtype == np.float64 and P.shape == ref["per_group"][k].shape and np.all(np.isfinite(P)) and np.all(P >= 0), (label, k)
        worst[k] = bound_ratio(P, ref, k, dtype)
    print(f"{label}: error / bound  " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, (label, worst)
    np.testing.assert_allclose(out["norm_grp"], ref["norm_grp"], rtol=1e-13, atol=0)
    if nbins:
        np.testing.assert_array_equal(out["count_bin"], ref["count_bin"])
        # the bins against the sequential double sum of the device's own groups, ascending: the same additions
        own = bin_groups({k: out["per_group"][k] for k in names}, out["norm_grp"], bins, nbins)
        for k in names:
            np.testing.assert_array_equal(out[k], own[k], err_msg=f"{label}: bins of {k}")
            assert np.any(out[k][0]) and not np.any(out[k][nbins - 1]) and out["count_bin"][nbins - 1] == 0  # a bin without groups
    return worst


def check_special_groups(out, pos, names=NAMES):
    for k in names:
        for z in ("flagged", "disjoint"):
            assert not np.any(out["per_group"][k][pos[z]]), (k, z)
        for z in ("forward", "reversed", "repeated", "mixed"):
            assert np.any(out["per_group"][k][pos[z]]), (k, z)
    assert out["norm_grp"][pos["flagged"]] == 0 and out["norm_grp"][pos["disjoint"]] == 0
    assert out["norm_grp"][pos["forward"]] > 0 and out["norm_grp"][pos["forward"]] == out["norm_grp"][pos["reversed"]]


def run_case(full, p0, pars, dtype, op, norm_f, T, label, layout="shared", path="auto", calibrated=False, rates=None):
    S = len(pars)
    rows, scale, pos = group_list(p0.nbls, S, T)
    assert_not_vacuous(full.wgts, rows, pos)
    bins, nbins = bins_of_groups(len(rows))
    opt = time_operator(T, rates)
    s = solver_of(full, joined(pars), dtype, layout, path)
    out = s.delay_fringe_spectrum(op, norm_f, rows, opt, scale=scale, calibrated=calibrated, bin_of_group=bins, nbins=nbins, per_group=True)
    ref = reference(full, p0, pars, dtype, op, norm_f, rows, opt, scale, calibrated, bins, nbins)
    check(out, ref, dtype, label, bins=bins, nbins=nbins)
    check_special_groups(out, pos)
    assert out["count_bin"].sum() == len(rows) - 3  # neither the flagged nor the disjoint group is counted, nor group 5 (-1)
    return s, out, (rows, scale, pos, bins, nbins, opt)


@pytest.mark.parametrize("config", GENERAL, ids=config_id)
@pytest.mark.parametrize("shape,S,ndelays,rates", [((7, 61), 3, 37, None), ((7, 61), 3, 61, [0, 2]), ((7, 200), 2, 200, None)])
@pytest.mark.parametrize("calibrated", [False, True], ids=["raw", "calibrated"])
def test_parity_with_the_restatement(shape, S, ndelays, rates, calibrated, config):
    dtype, layout, path = config
    full, p0, pars = batch(*shape, S)
    assert p0.nbls == 21
    op, norm_f = operator(shape[1], ndelays)
    label = f"{shape} x{S} {ndelays} rates={rates} {config_id(config)} calibrated={calibrated}"
    s, out, _ = run_case(full, p0, pars, dtype, op, norm_f, S, label, layout, path, calibrated, rates)
    assert out["per_group"]["data"].shape == (24, S if rates is None else 2, ndelays)
    s.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_more_than_64_groups(dtype):
    full, p0, pars = batch(13, 61, 2)
    assert p0.nbls == 78
    op, norm_f = operator(61, 37)
    s, out, _ = run_case(full, p0, pars, dtype, op, norm_f, 2, f"(13, 61) x2 37 {np.dtype(dtype).name}")
    s.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("T", [5, 17, 64])
def test_groups_past_the_row_tile_and_at_the_limit_of_64_times(T, dtype):
    """T = 5 and 17: groups that straddle the 16-row tiles and the 128-row blocks of the transform; T = 64: the limit, the whole
    64 KiB of the time kernel's LDS, 64 rates."""
    full, p0, pars = batch(7, 61, 4)
    op, norm_f = operator(61, 37)
    s, out, _ = run_case(full, p0, pars, dtype, op, norm_f, T, f"(7, 61) x4 T={T} {np.dtype(dtype).name}")
    assert out["per_group"]["resid"].shape == (24, T, 37)
    s.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("nfreqs", RW.NFREQS)
def test_row_walk_shapes(nfreqs, dtype):
    """nfreqs = 5: fpad = 8 under a pitch of 32 (the channels [fpad, xpitch) are zeroed without loads); nfreqs = 260: fpad = 384, a
    second trip of the wave along the rows, five column blocks of which the last holds 4 delays.  All nfreqs delays."""
    full, parts, params, _ = RW.batch(nfreqs)
    p0, nb = parts[0], parts[0].nbls
    op, norm_f, _ = modeling.delay_transform(150e6 + 400e3 * np.arange(nfreqs))
    pars = [RW.sliced(params, t, p0) for t in range(RW.T)]
    rows = np.array([(b, nb + b) for b in range(nb)] + [(2, 2), (nb + 1, 0), (0, nb + 1)], dtype=np.int32)
    scale = np.random.default_rng(3).uniform(0.5, 2.0, size=rows.shape)
    bins, nbins = bins_of_groups(len(rows))
    opt = time_operator(2)
    s = RW.solver_of(full, params, dtype)
    for calibrated in (False, True):
        label = f"row walk {nfreqs} {np.dtype(dtype).name} calibrated={calibrated}"
        out = s.delay_fringe_spectrum(op, norm_f, rows, opt, scale=scale, calibrated=calibrated, bin_of_group=bins, nbins=nbins, per_group=True)
        ref = reference(full, p0, pars, dtype, op, norm_f, rows, opt, scale, calibrated, bins, nbins)
        assert np.count_nonzero(ref["norm_grp"]) * 2 >= len(rows)
        check(out, ref, dtype, label, bins=bins, nbins=nbins)
    s.close()


# ---- every kernel path, fitting groups of several baselines
def one_slice_groups(nb, T=3):
    rows = np.array([[(b + 3 * t) % nb for t in range(T)] for b in range(nb)] + [[2] * T], dtype=np.int32)
    scale = np.random.default_rng(8).uniform(0.5, 2.0, size=rows.shape)
    return (rows, scale) + bins_of_groups(len(rows))


def one_slice_case(s, p, params, dtype, op, norm_f, label):
    """Groups among the rows of ONE slice (a group is any T rows): what the kernel path and the fitting groups can change is the model
    pass."""
    rows, scale, bins, nbins = one_slice_groups(p.nbls)
    opt = time_operator(3)
    out = s.delay_fringe_spectrum(op, norm_f, rows, opt, scale=scale, bin_of_group=bins, nbins=nbins, per_group=True)
    ref = reference(p, p, [params], dtype, op, norm_f, rows, opt, scale, False, bins, nbins)
    assert np.count_nonzero(ref["norm_grp"]) * 2 >= len(rows) and np.any(ref["norm_grp"] == 0)  # (DS.problem flags row 1 wholly)
    check(out, ref, dtype, label, bins=bins, nbins=nbins)
    return out


@pytest.mark.parametrize("dtype,path", PATHS, ids=map(path_id, PATHS))
def test_every_kernel_path(dtype, path):
    p, params = DS.problem(7, 200)
    op, norm_f = operator(200, 200)
    s = path_solver(p, params, dtype, path)
    assert_path(s, path)
    out = one_slice_case(s, p, params, dtype, op, norm_f, f"(7, 200) 200 {path_id((dtype, path))}")
    s.close()
    if path != "general":  # the model pass, the rows and the transforms are those of the general path: the same bits
        g = path_solver(p, params, dtype, "general")
        want = one_slice_case(g, p, params, dtype, op, norm_f, f"(7, 200) 200 general beside {path}")
        g.close()
        for k in NAMES:
            np.testing.assert_array_equal(out["per_group"][k], want["per_group"][k])
            np.testing.assert_array_equal(out[k], want[k])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("layout", ["stream", "shared"])
def test_fitting_groups_of_several_baselines(layout, dtype):
    p, params = DS.problem(7, 61, redundant=True)
    op, norm_f = operator(61, 37)
    s = DS.solver_of(p, params, dtype, layout)
    one_slice_case(s, p, params, dtype, op, norm_f, f"redundant group {layout} {np.dtype(dtype).name}")
    s.close()


# ---- bit identities
@pytest.mark.parametrize("calibrated", [False, True], ids=["raw", "calibrated"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_one_time_is_the_delay_spectrum_to_the_bit(dtype, calibrated):
    """T = 1, opt = [[1]], unit scale: power_grp of the group (b) is delay_spectrum's power_bl[b]."""
    full, p0, pars = batch(7, 61, 3)
    op, norm_f = operator(61, 37)
    rows = np.arange(full.nbls, dtype=np.int32)[::-1].reshape(-1, 1).copy()  # every row, descending
    s = solver_of(full, joined(pars), dtype)
    spec = s.delay_spectrum(op, norm_f, per_baseline=True, calibrated=calibrated)
    for scale in (None, np.ones(rows.shape)):
        out = s.delay_fringe_spectrum(op, norm_f, rows, np.ones((1, 1)), scale=scale, calibrated=calibrated, per_group=True)
        np.testing.assert_array_equal(out["norm_grp"], spec["norm_bl"][rows[:, 0]])
        for k in NAMES:
            assert out["per_group"][k].shape == (full.nbls, 1, 37)
            np.testing.assert_array_equal(out["per_group"][k][:, 0], spec["per_baseline"][k][rows[:, 0]], err_msg=k)
    assert np.count_nonzero(out["norm_grp"]) >= full.nbls - 2
    s.close()


@pytest.mark.parametrize("calibrated", [False, True], ids=["raw", "calibrated"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_two_times_are_the_cross_spectrum_s_two_channels(dtype, calibrated):
    """T = 2, opt = [[1, 1], [1, -1]]: rate 1 is exactly 2 diff of delay_cross_spectrum on the same pairs, and (rate 0 - rate 1) / 4 is
    its cross to 8 roundings of double on rate 0 + rate 1 (counted: at most 5 in each power -- the sum or difference of the two
    sides counts twice under the square, the square, the sum, the division --, 1 for the difference of the powers, 4 in the cross
    statistic on terms no larger than a quarter of rate 0 + rate 1)."""
    full, p0, pars = batch(7, 61, 2)
    op, norm_f = operator(61, 37)
    pairs, scale, pos = DC.pair_list(p0.nbls, 2)
    opt = np.array([[1.0, 1.0], [1.0, -1.0]])
    s = solver_of(full, joined(pars), dtype)
    cross = s.delay_cross_spectrum(op, norm_f, pairs, scale=scale, calibrated=calibrated, per_pair=True)
    out = s.delay_fringe_spectrum(op, norm_f, pairs, opt, scale=scale, calibrated=calibrated, per_group=True)
    s.close()
    np.testing.assert_array_equal(out["norm_grp"], cross["norm_pair"])
    assert np.count_nonzero(out["norm_grp"]) >= len(pairs) - 2
    for k in NAMES:
        P0, P1 = out["per_group"][k][:, 0], out["per_group"][k][:, 1]
        np.testing.assert_array_equal(P1, 2.0 * cross["per_pair"]["diff"][k], err_msg=k)
        assert np.any(P1)
        err = np.abs((P0 - P1) / 4.0 - cross["per_pair"]["cross"][k])
        assert np.all(err <= 8 * U64 * (P0 + P1)), (k, float(np.max(err / np.maximum(P0 + P1, 1e-300))) / U64)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape,S,T,ndelays", [((7, 61), 3, 3, 37), ((13, 61), 2, 2, 61), ((7, 61), 4, 17, 37)])
def test_chunks_and_repeated_calls_give_the_same_bits(shape, S, T, ndelays, dtype):
    full, p0, pars = batch(*shape, S)
    op, norm_f = operator(shape[1], ndelays)
    rows, scale, pos = group_list(p0.nbls, S, T)
    bins, nbins = bins_of_groups(len(rows))
    opt = time_operator(T)
    s = solver_of(full, joined(pars), dtype)
    call = lambda: s.delay_fringe_spectrum(op, norm_f, rows, opt, scale=scale, bin_of_group=bins, nbins=nbins, per_group=True)  # noqa: E731
    one = call()
    again = call()
    xpitch = -(-shape[1] // 32) * 32
    per_group = 3 * 2 * T * xpitch * np.dtype(dtype).itemsize + 3 * 2 * T * ndelays * 8 + 3 * T * ndelays * 8
    for ngrp in (7, 1):  # seven groups per chunk, one group each
        s._set_delay_spectrum_scratch(ngrp * per_group + per_group // 2)
        cut = call()
        for a, b in ((one, again), (one, cut)):
            np.testing.assert_array_equal(a["norm_grp"], b["norm_grp"])
            np.testing.assert_array_equal(a["count_bin"], b["count_bin"])
            for k in NAMES:
                np.testing.assert_array_equal(a[k], b[k], err_msg=f"{ngrp} groups per chunk, bins of {k}")
                np.testing.assert_array_equal(a["per_group"][k], b["per_group"][k], err_msg=f"{ngrp} groups per chunk, {k}")
    s._set_delay_spectrum_scratch(1)  # below one group: one group per chunk
    cut = call()
    for k in NAMES:
        np.testing.assert_array_equal(one[k], cut[k])
        np.testing.assert_array_equal(one["per_group"][k], cut["per_group"][k])
    s._set_delay_spectrum_scratch(0)
    s.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_each_quantity_alone_and_each_output_alone(dtype):
    full, p0, pars = batch(7, 61, 3)
    op, norm_f = operator(61, 37)
    rows, scale, pos = group_list(p0.nbls, 3, 3)
    bins, nbins = bins_of_groups(len(rows))
    opt = time_operator(3)
    s = solver_of(full, joined(pars), dtype)
    kw = dict(scale=scale, bin_of_group=bins, nbins=nbins, per_group=True)
    everything = s.delay_fringe_spectrum(op, norm_f, rows, opt, **kw)
    for what in (("data",), ("model",), ("resid",), ("resid", "data")):
        one = s.delay_fringe_spectrum(op, norm_f, rows, opt, what=what, **kw)
        assert set(one["per_group"]) == set(what) and set(one) == set(what) | {"norm_grp", "count_bin", "per_group"}
        for k in what:
            np.testing.assert_array_equal(one["per_group"][k], everything["per_group"][k], err_msg=f"{what}")
            np.testing.assert_array_equal(one[k], everything[k], err_msg=f"{what}")
        np.testing.assert_array_equal(one["count_bin"], everything["count_bin"])
    only_bins = s.delay_fringe_spectrum(op, norm_f, rows, opt, scale=scale, bin_of_group=bins, nbins=nbins)
    only_groups = s.delay_fringe_spectrum(op, norm_f, rows, opt, scale=scale, per_group=True)
    neither = s.delay_fringe_spectrum(op, norm_f, rows, opt)
    assert "per_group" not in only_bins and "count_bin" not in only_groups and "data" not in only_groups
    for k in NAMES:
        np.testing.assert_array_equal(only_bins[k], everything[k])
        np.testing.assert_array_equal(only_groups["per_group"][k], everything["per_group"][k])
    np.testing.assert_array_equal(neither["norm_grp"], everything["norm_grp"])
    # no scales are unit scales
    ones = s.delay_fringe_spectrum(op, norm_f, rows, opt, scale=np.ones_like(scale), per_group=True)
    none = s.delay_fringe_spectrum(op, norm_f, rows, opt, per_group=True)
    for k in NAMES:
        np.testing.assert_array_equal(ones["per_group"][k], none["per_group"][k])
    s.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_given_gains_against_set_gains(dtype):
    full, p0, pars = batch(7, 61, 2)
    op, norm_f = operator(61, 37)
    rows, scale, pos = group_list(p0.nbls, 2, 2)
    opt = time_operator(2)
    params = joined(pars)
    og = joined([DS.perturbed(p0, dict(q), seed=11 + t) for t, q in enumerate(pars)])
    s = solver_of(full, params, dtype)
    given = s.delay_fringe_spectrum(op, norm_f, rows, opt, scale=scale, per_group=True, g_r=og["g_r"], g_i=og["g_i"])
    np.testing.assert_array_equal(s.get_params()[0], np.asarray(params["g_r"], dtype=dtype))  # the solver's own gains stay
    own = s.delay_fringe_spectrum(op, norm_f, rows, opt, scale=scale, per_group=True)
    s.set_params(og["g_r"], og["g_i"])
    as_set = s.delay_fringe_spectrum(op, norm_f, rows, opt, scale=scale, per_group=True)
    for k in NAMES:
        np.testing.assert_array_equal(given["per_group"][k], as_set["per_group"][k], err_msg=k)
    assert np.any(own["per_group"]["model"] != given["per_group"]["model"])
    with pytest.raises(ValueError):
        s.delay_fringe_spectrum(op, norm_f, rows, opt, g_r=og["g_r"])
    s.close()


@pytest.mark.parametrize("config", ["adam", "graph", "gain_basis"])
def test_a_run_continued_after_the_call_is_bit_identical(config):
    full, p0, pars = batch(7, 61, 2)
    op, norm_f = operator(61, 37)
    rows, scale, pos = group_list(p0.nbls, 2, 2)
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
            out = s.delay_fringe_spectrum(op, norm_f, rows, opt, scale=scale, per_group=True)
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
    """After robust_weights("clip") the report is the restatement on the rewritten plane, and not the one on the weights as set."""
    full, p0, pars = batch(7, 61, 3)
    op, norm_f = operator(61, 37)
    rows, scale, pos = group_list(p0.nbls, 3, 3)
    opt = time_operator(3)
    s = solver_of(full, joined(pars), dtype)
    s.robust_weights(*CLIP)
    w, w0 = s.get_weights(0), s.get_weights(1)
    assert np.any((w == 0) != (w0 == 0))
    out = s.delay_fringe_spectrum(op, norm_f, rows, opt, scale=scale, per_group=True)
    s.close()
    new = reference(full, p0, pars, dtype, op, norm_f, rows, opt, scale, w=w)
    old = reference(full, p0, pars, dtype, op, norm_f, rows, opt, scale, w=w0)
    assert np.count_nonzero(new["norm_grp"]) * 2 >= len(rows)
    check(out, new, dtype, f"behind clip {np.dtype(dtype).name}")
    moved = new["norm_grp"] != old["norm_grp"]
    assert np.any(moved) and np.all(out["norm_grp"][moved] != old["norm_grp"][moved])
    # held to the old plane's restatement the report misses the bound: it is another report, not a rounding of that one
    err = np.abs(out["per_group"]["data"] - old["per_group"]["data"]) * old["norm_grp"][:, None, None]
    assert np.any(err[moved] > bound_plane(old, "data", dtype)[moved])


def test_errors_are_reported():
    import ctypes as C

    full, p0, pars = batch(7, 61, 2)
    op, norm_f = operator(61, 37)
    params = joined(pars)
    s = solver_of(full, params, np.float64)
    op_r, op_i = np.ascontiguousarray(op.real), np.ascontiguousarray(op.imag)
    rows = np.array([[0, p0.nbls], [2, 2]], dtype=np.int32)
    scale = np.ones((2, 2))
    opt_r, opt_i = np.array([[1.0, 1.0], [1.0, -1.0]]), np.zeros((2, 2))
    bins = np.zeros(2, dtype=np.int32)
    buf = np.empty((3, 2, 2, 37))
    norm = np.empty(2)
    wide = np.zeros((2, 65), dtype=np.int32)
    wide_opt = np.ones((65, 65))

    def code(ndelays=37, what=7, calibrated=0, ngroups=2, ntimes=2, nrates=2, rows=rows, scale=None, nbins=0, bin_of_group=None, op_r=op_r.ctypes.data,
             norm_f=norm_f.ctypes.data, opt_r=opt_r, opt_i=opt_i, power_grp=None, power_bin=None):
        ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        d = _lib.DelayFringeDesc(ndelays, what, calibrated, ngroups, ntimes, nrates, ptr(rows), ptr(scale), nbins, bin_of_group, op_r, op_i.ctypes.data, norm_f,
                                 ptr(opt_r), ptr(opt_i))
        return s._lib.cal_solver_delay_fringe_spectrum(s._h, C.byref(d), None, None, ptr(power_grp), norm.ctypes.data, ptr(power_bin), None)

    INV = _lib.CAL_ERR_INVALID
    assert code() == 0 and code(scale=scale) == 0 and code(power_grp=buf) == 0
    assert code(what=0) == INV and code(what=8) == INV
    assert code(ndelays=0) == INV and code(ndelays=4097) == INV
    assert code(op_r=None) == INV and code(norm_f=None) == INV
    assert code(calibrated=2) == INV
    assert code(ngroups=0) == INV and code(rows=None) == INV
    assert code(ntimes=0) == INV and code(ntimes=65, rows=wide, opt_r=wide_opt, opt_i=wide_opt) == INV
    assert code(nrates=0) == INV and code(nrates=65, opt_r=wide_opt, opt_i=wide_opt) == INV
    assert code(opt_r=None) == INV and code(opt_i=None) == INV
    assert code(power_bin=buf) == INV  # binned outputs with nbins == 0
    assert code(nbins=2) == INV  # bins without bin_of_group
    assert code(nbins=2, bin_of_group=bins.ctypes.data) == 0
    bins[1] = 2
    assert code(nbins=2, bin_of_group=bins.ctypes.data) == INV
    bins[1] = -2
    assert code(nbins=2, bin_of_group=bins.ctypes.data) == INV
    bad = rows.copy()
    bad[1, 1] = full.nbls
    assert code(rows=bad) == INV
    bad[1, 1] = -1
    assert code(rows=bad) == INV
    for v in (np.inf, np.nan):
        sc = scale.copy()
        sc[0, 1] = v
        assert code(scale=sc) == INV
        for part in ("opt_r", "opt_i"):
            o = opt_r.copy()
            o[1, 0] = v
            assert code(**{part: o}) == INV
    assert s._lib.cal_solver_delay_fringe_spectrum(s._h, None, None, None, None, None, None, None) == INV
    s.close()
    # state: gains neither set nor given
    from calamity_amd.solver import HipFitSolver

    s = HipFitSolver(dtype=np.float64)
    s.set_problem(full)
    s.set_data(full.data_r, full.data_i, full.wgts)
    s.set_params(c_r=params["c_r"], c_i=params["c_i"])
    with pytest.raises(_lib.CalamityHipError) as err:
        s.delay_fringe_spectrum(op, norm_f, rows, opt_r)
    assert err.value.code == _lib.CAL_ERR_STATE
    assert s.delay_fringe_spectrum(op, norm_f, rows, opt_r, g_r=params["g_r"], g_i=params["g_i"])["norm_grp"][0] > 0
    s.close()
