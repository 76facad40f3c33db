"""cal_solver_delay_cross_spectrum on the device against the float64 restatement of the header text (tests/delay_cross_ref.py), at the
smallest shapes that reach every branch: slices of make_problem(7, 61) in ONE solver (21 rows per slice; 37 delays: a partial column
block, and 61), of make_problem(7, 200) (200 delays: four column blocks, the last ragged), of make_problem(13, 61) (78 same-baseline
pairs: one full block of 64 pairs and a ragged one of 14), and the two-slice problems of test_gpu_row_walk_shapes at 5 and 260 channels.

Every pair list holds: the same-baseline pairs of adjacent slices, a pair of different baselines, a pair in reversed order, (b, b)
pairs, a pair with one side wholly flagged, a pair whose masks are disjoint, and unequal scales.

The bound is derived, not tuned (delay_cross_ref.py).  Every case prints its largest ratio of error to bound."""
import copy
import functools

import numpy as np
import pytest

import test_gpu_delay_spectrum as DS
import test_gpu_row_walk_shapes as RW
from calamity_amd import _lib, batched, modeling, synthetic
from delay_cross_ref import STATS, bin_pairs, bound_ratio, restated
from delay_spectrum_ref import NAMES, model_of

pytestmark = pytest.mark.gpu

F0, DF = DS.F0, DS.DF
KEYS = ("g_r", "g_i", "c_r", "c_i")


def cast(a, dtype):
    return np.asarray(a).astype(dtype).astype(np.float64)


@functools.lru_cache(maxsize=None)
def batch(nants, nfreqs, T):
    """T slices of make_problem(nants, nfreqs) in one problem (bl_alias): (problem with data, p0, per-slice parameters).  Slice t has
    its own data and flags; row 1 of slice 0 is flagged wholly; row 3 of slice 0 keeps the even channels and row 3 of slice 1 the odd
    ones (disjoint masks)."""
    parts = [synthetic.make_problem(nants, nfreqs, f0=F0, df=DF, seed=nants + nfreqs, data_seed=30 + t, flag_frac=0.05) for t in range(T)]
    p0 = parts[0][0]
    sub, _, _ = batched.replicate_slices(p0, T)
    assert sub.bl_alias is not None
    rng = np.random.default_rng(77)
    w = np.concatenate([parts[t][0].wgts for t in range(T)])
    w = np.where(rng.random(w.shape) < 0.05, 0.0, w)  # flags that differ between the slices
    nb = p0.nbls
    w[1] = 0.0
    w[3, 1::2] = 0.0
    w[nb + 3, 0::2] = 0.0
    assert np.any((w[:nb] != 0) != (w[nb : 2 * nb] != 0))
    sub.data_r = np.concatenate([parts[t][0].data_r for t in range(T)])
    sub.data_i = np.concatenate([parts[t][0].data_i for t in range(T)])
    sub.wgts = w
    pars = [DS.perturbed(parts[t][0], parts[t][2], seed=40 + t) for t in range(T)]
    return sub, p0, pars


def joined(pars):
    return {k: np.concatenate([q[k] for q in pars]) for k in KEYS}


def pair_list(nb, T, seed=5):
    """(pairs, scale, named positions)."""
    same = [(t * nb + b, (t + 1) * nb + b) for t in range(T - 1) for b in range(nb)]
    extra = {"different": (0, nb + 2), "reversed": (nb + 4, 4), "bb0": (0, 0), "bb2": (2, 2), "bb_late": (nb + 5, nb + 5), "bb_scaled": (6, 6)}
    pairs = np.array(same + list(extra.values()), dtype=np.int32)
    pos = {k: len(same) + i for i, k in enumerate(extra)}
    pos.update(forward=4, flagged=1, disjoint=3)  # (4, nb + 4), (1, nb + 1), (3, nb + 3) among the same-baseline pairs
    scale = np.random.default_rng(seed).uniform(0.5, 2.0, size=(len(pairs), 2))
    scale[pos["reversed"]] = scale[pos["forward"]][::-1]
    for k in ("bb0", "bb2", "bb_late"):
        scale[pos[k]] = 1.0
    return pairs, scale, pos


def bins_of_pairs(npairs, nbins=4):
    """Pairs dealt over the bins 0 .. nbins - 2 (bin nbins - 1 stays empty); pair 5 is left out (-1)."""
    b = (np.arange(npairs) % (nbins - 1)).astype(np.int32)
    b[5] = -1
    return b, nbins


def solver_of(full, params, dtype, layout="shared", kernel_path="auto"):
    from calamity_amd.solver import HipFitSolver

    s = HipFitSolver(dtype=dtype)
    s.set_problem(full, layout=layout, kernel_path=kernel_path)
    s.set_data(full.data_r, full.data_i, full.wgts)
    s.set_params(*[params[k] for k in KEYS])
    return s


def reference(full, p0, pars, dtype, op, norm_f, pairs, scale, calibrated=False, bins=None, nbins=0):
    """The restatement from the inputs rounded to ``dtype``; ``pars``: the parameters of every slice (p0's shapes)."""
    d = cast(full.data_r, dtype) + 1j * cast(full.data_i, dtype)
    m = np.concatenate([model_of(p0, q["c_r"], q["c_i"], dtype) for q in pars])
    G = np.concatenate([(cast(q["g_r"], dtype) + 1j * cast(q["g_i"], dtype))[p0.bl_ant0] * np.conj((cast(q["g_r"], dtype) + 1j * cast(q["g_i"], dtype))[p0.bl_ant1])
                        for q in pars])
    op_t = cast(op.real, dtype) + 1j * cast(op.imag, dtype)
    return restated(d, m, G, cast(full.wgts, dtype), op_t, norm_f, pairs, scale, calibrated, bins, nbins)


def check(out, ref, dtype, label, names=NAMES, stats=STATS, bins=None, nbins=0):
    worst = {}
    for st in stats:
        for k in names:
            P = out["per_pair"][st][k]
            assert P.dtype == np.float64 and P.shape == ref["per_pair"][st][k].shape and np.all(np.isfinite(P)), (label, st, k)
            worst[st, k] = bound_ratio(P, ref, st, k, dtype)
            if st == "diff":
                assert np.all(P >= 0), (label, k)
    print(f"{label}: error / bound  " + "  ".join(f"{st} {k} {v:.3f}" for (st, k), v in worst.items()))
    assert max(worst.values()) <= 1.0, (label, worst)
    np.testing.assert_allclose(out["norm_pair"], ref["norm_pair"], rtol=1e-13, atol=0)
    if nbins:
        np.testing.assert_array_equal(out["count_bin"], ref["count_bin"])
        for st in stats:
            own = bin_pairs({k: out["per_pair"][st][k] for k in names}, out["norm_pair"], bins, nbins)
            for k in names:
                # the bins against the sequential double sum of the device's own pairs, ascending: the same additions
                scale = np.max(np.abs(own[k]))
                assert np.max(np.abs(out[st][k] - own[k])) <= len(bins) * 2.0 ** -53 * scale, (label, st, k)
                assert not np.any(out[st][k][nbins - 1]) and out["count_bin"][nbins - 1] == 0  # a bin without pairs
    return worst


def check_special_pairs(out, pos, names=NAMES):
    """What holds to the bit: the reversed pair, the (b, b) pairs with unit scales, the flagged and the disjoint pair."""
    pp = out["per_pair"]
    for k in names:
        np.testing.assert_array_equal(pp["diff"][k][pos["reversed"]], pp["diff"][k][pos["forward"]])  # (a - b)^2 is symmetric
        np.testing.assert_array_equal(pp["cross"][k][pos["reversed"]], pp["cross"][k][pos["forward"]])  # and so is the product
        for b in ("bb0", "bb2", "bb_late"):
            assert not np.any(pp["diff"][k][pos[b]]), (k, b)
            assert np.all(pp["cross"][k][pos[b]] >= 0)
        for z in ("flagged", "disjoint"):
            assert not np.any(pp["cross"][k][pos[z]]) and not np.any(pp["diff"][k][pos[z]]), (k, z)
    assert out["norm_pair"][pos["flagged"]] == 0 and out["norm_pair"][pos["disjoint"]] == 0
    assert out["norm_pair"][pos["forward"]] > 0


def operator(nfreqs, ndelays):
    return DS.operator(nfreqs, ndelays)


def run_case(full, p0, pars, dtype, op, norm_f, label, layout="shared", path="auto", calibrated=False):
    T = len(pars)
    pairs, scale, pos = pair_list(p0.nbls, T)
    bins, nbins = bins_of_pairs(len(pairs))
    s = solver_of(full, joined(pars), dtype, layout, path)
    out = s.delay_cross_spectrum(op, norm_f, pairs, scale=scale, calibrated=calibrated, bin_of_pair=bins, nbins=nbins, per_pair=True)
    ref = reference(full, p0, pars, dtype, op, norm_f, pairs, scale, calibrated, bins, nbins)
    check(out, ref, dtype, label, bins=bins, nbins=nbins)
    check_special_pairs(out, pos)
    # neither the flagged nor the disjoint pair is counted, nor pair 5 (-1)
    assert out["count_bin"].sum() == len(pairs) - 3
    return s, out, (pairs, scale, pos, bins, nbins)


GENERAL = DS.GENERAL
DENSE = DS.DENSE
config_id = DS.config_id


@pytest.mark.parametrize("config", GENERAL, ids=config_id)
@pytest.mark.parametrize("shape,T,ndelays", [((7, 61), 3, 37), ((7, 61), 3, 61), ((7, 200), 2, 200)])
@pytest.mark.parametrize("calibrated", [False, True], ids=["raw", "calibrated"])
def test_parity_with_the_restatement(shape, T, ndelays, calibrated, config):
    dtype, layout, path = config
    full, p0, pars = batch(*shape, T)
    assert p0.nbls == 21
    op, norm_f = operator(shape[1], ndelays)
    s, out, _ = run_case(full, p0, pars, dtype, op, norm_f, f"{shape} x{T} {ndelays} {config_id(config)} calibrated={calibrated}", layout, path, calibrated)
    s.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_full_block_of_64_pairs_and_a_ragged_one(dtype):
    full, p0, pars = batch(13, 61, 2)
    assert p0.nbls == 78
    op, norm_f = operator(61, 37)
    s, out, _ = run_case(full, p0, pars, dtype, op, norm_f, f"(13, 61) x2 37 {np.dtype(dtype).name}")
    s.close()


def single_slice_pairs(nb):
    """(pairs, scale, bins, nbins) among the rows of ONE slice: (b, (b + 3) % nb) for every row, (2, 2) with unit scales at position
    nb, (nb - 1, 0); seeded unequal scales elsewhere."""
    pairs = np.array([(b, (b + 3) % nb) for b in range(nb)] + [(2, 2), (nb - 1, 0)], dtype=np.int32)
    scale = np.random.default_rng(8).uniform(0.5, 2.0, size=(len(pairs), 2))
    scale[nb] = 1.0
    return (pairs, scale) + bins_of_pairs(len(pairs))


def single_slice_case(p, params, dtype, op, norm_f, label, layout="shared", path="auto"):
    """Pairs among the rows of ONE slice (a pair is any two rows): what the kernel path and the groups can change is the model pass."""
    nb = p.nbls
    pairs, scale, bins, nbins = single_slice_pairs(nb)
    s = DS.solver_of(p, params, dtype, layout, path)
    if path != "auto":
        assert s.timing_get()["kernel_path"] == path
    out = s.delay_cross_spectrum(op, norm_f, pairs, scale=scale, bin_of_pair=bins, nbins=nbins, per_pair=True)
    ref = reference(p, p, [params], dtype, op, norm_f, pairs, scale, False, bins, nbins)
    check(out, ref, dtype, label, bins=bins, nbins=nbins)
    # (b, b) with unit scales: diff is exactly 0 and cross is delay_spectrum's power_bl[b] to the bit (the shared loop)
    spec = s.delay_spectrum(op, norm_f, per_baseline=True)
    for k in NAMES:
        assert not np.any(out["per_pair"]["diff"][k][nb])
        np.testing.assert_array_equal(out["per_pair"]["cross"][k][nb], spec["per_baseline"][k][2])
    assert out["norm_pair"][nb] == spec["norm_bl"][2]
    s.close()


@pytest.mark.parametrize("config", DENSE, ids=config_id)
def test_parity_on_the_shared_dense_paths(config):
    dtype, layout, path = config
    p, params = DS.problem(7, 200)
    op, norm_f = operator(200, 200)
    single_slice_case(p, params, dtype, op, norm_f, f"(7, 200) 200 {config_id(config)}", layout, path)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("layout", ["stream", "shared"])
def test_fitting_groups_of_several_baselines(layout, dtype):
    p, params = DS.problem(7, 61, redundant=True)
    op, norm_f = operator(61, 37)
    single_slice_case(p, params, dtype, op, norm_f, f"redundant group {layout} {np.dtype(dtype).name}", layout)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("nfreqs", RW.NFREQS)
def test_row_walk_shapes(nfreqs, dtype):
    """nfreqs = 5: fpad = 8 under a pitch of 32 (the channels [fpad, xpitch) are zeroed without loads); nfreqs = 260: fpad = 384, a
    second trip of the wave along both rows, five column blocks of which the last holds 4 delays.  All nfreqs delays."""
    full, parts, params, _ = RW.batch(nfreqs)
    p0, nb = parts[0], parts[0].nbls
    op, norm_f, _ = modeling.delay_transform(150e6 + 400e3 * np.arange(nfreqs))
    pars = [RW.sliced(params, t, p0) for t in range(RW.T)]
    pairs = np.array([(b, nb + b) for b in range(nb)] + [(2, 2), (nb + 1, 0), (0, nb + 1)], dtype=np.int32)
    scale = np.random.default_rng(3).uniform(0.5, 2.0, size=(len(pairs), 2))
    scale[nb] = 1.0
    scale[nb + 2] = scale[nb + 1][::-1]
    bins, nbins = bins_of_pairs(len(pairs))
    s = RW.solver_of(full, params, dtype)
    for calibrated in (False, True):
        label = f"row walk {nfreqs} {np.dtype(dtype).name} calibrated={calibrated}"
        out = s.delay_cross_spectrum(op, norm_f, pairs, scale=scale, calibrated=calibrated, bin_of_pair=bins, nbins=nbins, per_pair=True)
        ref = reference(full, p0, pars, dtype, op, norm_f, pairs, scale, calibrated, bins, nbins)
        check(out, ref, dtype, label, bins=bins, nbins=nbins)
        spec = s.delay_spectrum(op, norm_f, per_baseline=True, calibrated=calibrated)
        for k in NAMES:
            assert not np.any(out["per_pair"]["diff"][k][nb])
            np.testing.assert_array_equal(out["per_pair"]["cross"][k][nb], spec["per_baseline"][k][2])
            np.testing.assert_array_equal(out["per_pair"]["diff"][k][nb + 1], out["per_pair"]["diff"][k][nb + 2])
    s.close()


# ---- two kernels, one identity
SHARED_FLAGS = (0, 1, 2, 3, 5, 20)  # rows of slice 1 given the flags of the same rows of slice 0 (row 1: all flagged; row 3: the even channels)
# 2 diff = P[b0] + P[b1] - 2 cross is exact in the reals when both sides of a pair carry one mask and unit scales: dspec_rows_kernel and
# dcross_rows_kernel then form the same planes, ds_transform_loop the same accumulators (re_s, im_s), and both epilogues work on them in
# double without contraction.  Roundings of double, counted in the two epilogues (the unit scales multiply exactly):
#   P[b]  = (re re + im im) / n                   2 products, 1 sum, 1 division: 4, all on non-negative terms: 4 u P
#   cross = (re0 re1 + im0 im1) / n               2 products (u (|re0 re1| + |im0 im1|) / n <= u (P[b0] + P[b1]) / 2), 1 sum, 1 division: 4
#   diff  = ((re0 - re1)^2 + (im0 - im1)^2) / 2n  2 differences (each counts twice under the square), 2 squares, 1 sum, 1 division: 6 operations, 5 u diff
#   the test's own P[b0] + P[b1] - 2 cross         1 sum, 1 difference: 2
# No quantity takes more than 8, so the identity is held to 16 u (P[b0] + P[b1] + 2 |cross| + 2 diff) per element, u = 2^-53: eight
# roundings for each quantity as it enters the identity (P once, cross and diff doubled).
IDENTITY_ROUNDINGS = 8


@functools.lru_cache(maxsize=None)
def shared_flag_batch():
    """``batch(7, 61, 2)`` with the rows ``SHARED_FLAGS`` of slice 1 flagged exactly as the same rows of slice 0."""
    full, p0, pars = batch(7, 61, 2)
    nb = p0.nbls
    twin = copy.copy(full)
    w = np.array(full.wgts, dtype=np.float64)
    for b in SHARED_FLAGS:
        w[nb + b] = np.where(w[b] != 0, w.max(), 0.0)
    twin.wgts = w
    return twin, p0, pars


@pytest.mark.parametrize("calibrated", [False, True], ids=["raw", "calibrated"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_cross_and_diff_of_equally_flagged_rows_add_up_to_the_spectrum_s_powers(dtype, calibrated):
    full, p0, pars = shared_flag_batch()
    nb = p0.nbls
    op, norm_f = operator(61, 37)
    pairs = np.array([(b, nb + b) for b in SHARED_FLAGS], dtype=np.int32)
    assert np.array_equal(full.wgts[pairs[:, 0]] != 0, full.wgts[pairs[:, 1]] != 0)
    assert np.any(full.wgts[pairs[:, 0]] != full.wgts[pairs[:, 1]])  # (the same flags, not the same weights)
    s = solver_of(full, joined(pars), dtype)
    out = s.delay_cross_spectrum(op, norm_f, pairs, calibrated=calibrated, per_pair=True)
    spec = s.delay_spectrum(op, norm_f, per_baseline=True, calibrated=calibrated)
    s.close()
    for side in (0, 1):
        np.testing.assert_array_equal(out["norm_pair"], spec["norm_bl"][pairs[:, side]])
    assert out["norm_pair"][1] == 0 and np.all(np.delete(out["norm_pair"], 1) > 0)
    worst = {}
    for k in NAMES:
        P0, P1 = (spec["per_baseline"][k][pairs[:, side]] for side in (0, 1))
        cross, diff = out["per_pair"]["cross"][k], out["per_pair"]["diff"][k]
        bound = 2 * IDENTITY_ROUNDINGS * 2.0 ** -53 * (P0 + P1 + 2.0 * np.abs(cross) + 2.0 * diff)
        err = np.abs(2.0 * diff - (P0 + P1 - 2.0 * cross))
        worst[k] = float(np.max(np.divide(err, bound, out=np.zeros_like(err), where=err > 0)))
        assert np.all(diff[[0, 2, 3, 4, 5]].max(axis=1) > 0) and not np.any(diff[1]) and not np.any(P0[1])  # two times differ: the identity says something
    print(f"identity {np.dtype(dtype).name} calibrated={calibrated}: error / bound  " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_each_quantity_and_each_statistic_alone(dtype):
    full, p0, pars = batch(7, 61, 3)
    op, norm_f = operator(61, 37)
    pairs, scale, pos = pair_list(p0.nbls, 3)
    bins, nbins = bins_of_pairs(len(pairs))
    s = solver_of(full, joined(pars), dtype)
    kw = dict(scale=scale, bin_of_pair=bins, nbins=nbins, per_pair=True)
    everything = s.delay_cross_spectrum(op, norm_f, pairs, **kw)
    for what in (("data",), ("model",), ("resid",), ("resid", "data")):
        for stats in (("cross",), ("diff",), ("diff", "cross")):
            one = s.delay_cross_spectrum(op, norm_f, pairs, what=what, stats=stats, **kw)
            assert set(one["per_pair"]) == set(stats)
            for st in stats:
                assert set(one["per_pair"][st]) == set(what) and set(one[st]) == set(what)
                for k in what:
                    np.testing.assert_array_equal(one["per_pair"][st][k], everything["per_pair"][st][k], err_msg=f"{what} {stats}")
                    np.testing.assert_array_equal(one[st][k], everything[st][k], err_msg=f"{what} {stats}")
            np.testing.assert_array_equal(one["count_bin"], everything["count_bin"])
    only_bins = s.delay_cross_spectrum(op, norm_f, pairs, scale=scale, bin_of_pair=bins, nbins=nbins)
    only_pairs = s.delay_cross_spectrum(op, norm_f, pairs, scale=scale, per_pair=True)
    neither = s.delay_cross_spectrum(op, norm_f, pairs)
    assert "per_pair" not in only_bins and "count_bin" not in only_pairs and "cross" not in only_pairs
    for st in STATS:
        for k in NAMES:
            np.testing.assert_array_equal(only_bins[st][k], everything[st][k])
            np.testing.assert_array_equal(only_pairs["per_pair"][st][k], everything["per_pair"][st][k])
    np.testing.assert_array_equal(neither["norm_pair"], everything["norm_pair"])
    # no scales are unit scales
    ones = s.delay_cross_spectrum(op, norm_f, pairs, scale=np.ones_like(scale), per_pair=True)
    none = s.delay_cross_spectrum(op, norm_f, pairs, per_pair=True)
    for st in STATS:
        for k in NAMES:
            np.testing.assert_array_equal(ones["per_pair"][st][k], none["per_pair"][st][k])
    s.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape,ndelays", [((7, 61), 37), ((13, 61), 61)])
def test_chunks_and_repeated_calls_give_the_same_bits(shape, ndelays, dtype):
    full, p0, pars = batch(*shape, 2)
    op, norm_f = operator(shape[1], ndelays)
    pairs, scale, pos = pair_list(p0.nbls, 2)
    bins, nbins = bins_of_pairs(len(pairs))
    s = solver_of(full, joined(pars), dtype)
    call = lambda: s.delay_cross_spectrum(op, norm_f, pairs, scale=scale, bin_of_pair=bins, nbins=nbins, per_pair=True)  # noqa: E731
    one = call()
    again = call()
    xpitch = -(-shape[1] // 32) * 32
    per_pair = 3 * 2 * 2 * xpitch * np.dtype(dtype).itemsize + 2 * 3 * ndelays * 8
    for npair in (64, 7, 1):  # 64-pair chunks (84 pairs of (13, 61): 64 + 20), seven pairs, one pair each
        s._set_delay_spectrum_scratch(npair * per_pair + per_pair // 2)
        cut = call()
        for a, b in ((one, again), (one, cut)):
            np.testing.assert_array_equal(a["norm_pair"], b["norm_pair"])
            np.testing.assert_array_equal(a["count_bin"], b["count_bin"])
            for st in STATS:
                for k in NAMES:
                    np.testing.assert_array_equal(a[st][k], b[st][k], err_msg=f"{npair} pairs per chunk, bins of {st} {k}")
                    np.testing.assert_array_equal(a["per_pair"][st][k], b["per_pair"][st][k], err_msg=f"{npair} pairs per chunk, {st} {k}")
    s._set_delay_spectrum_scratch(0)
    s.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_given_gains_and_the_expanded_gains_of_a_basis(dtype):
    full, p0, pars = batch(7, 61, 2)
    op, norm_f = operator(61, 37)
    pairs, scale, pos = pair_list(p0.nbls, 2)
    params = joined(pars)
    other = [DS.perturbed(p0, dict(q), seed=11 + t) for t, q in enumerate(pars)]
    og = joined(other)
    s = solver_of(full, params, dtype)
    given = s.delay_cross_spectrum(op, norm_f, pairs, scale=scale, per_pair=True, g_r=og["g_r"], g_i=og["g_i"])
    np.testing.assert_array_equal(s.get_params()[0], np.asarray(params["g_r"], dtype=dtype))  # the solver's own gains stay
    s.set_params(og["g_r"], og["g_i"])
    as_set = s.delay_cross_spectrum(op, norm_f, pairs, scale=scale, per_pair=True)
    for st in STATS:
        for k in NAMES:
            np.testing.assert_array_equal(given["per_pair"][st][k], as_set["per_pair"][st][k], err_msg=f"{st} {k}")
    with pytest.raises(ValueError):
        s.delay_cross_spectrum(op, norm_f, pairs, g_r=og["g_r"])
    s.close()
    # a frequency gain basis with y != 0: NULL gains are the expanded ones
    s = solver_of(full, params, dtype)
    s.set_gain_basis(np.array(modeling.gain_dpss_basis(F0 + DF * np.arange(p0.nfreqs), 100.0)))
    s.set_optimizer("Adam", learning_rate=1e-2)
    s.run_slices(3, tol=0.0)
    assert np.any(s.get_gain_coeffs()[0] != 0)
    g_r, g_i, c_r, c_i = s.get_params()
    na, nc = p0.nants, p0.ncoeffs
    now = [dict(g_r=g_r[t * na : (t + 1) * na], g_i=g_i[t * na : (t + 1) * na], c_r=c_r[t * nc : (t + 1) * nc], c_i=c_i[t * nc : (t + 1) * nc]) for t in range(2)]
    out = s.delay_cross_spectrum(op, norm_f, pairs, scale=scale, per_pair=True)
    check(out, reference(full, p0, now, dtype, op, norm_f, pairs, scale), dtype, f"gain basis {np.dtype(dtype).name}")
    s.close()


@pytest.mark.parametrize("config", ["adam", "graph", "gain_basis"])
def test_a_run_continued_after_the_call_is_bit_identical(config):
    full, p0, pars = batch(7, 61, 2)
    op, norm_f = operator(61, 37)
    pairs, scale, pos = pair_list(p0.nbls, 2)
    losses, final = {}, {}
    for with_call in (False, True):
        s = solver_of(full, joined(pars), np.float32)
        if config == "gain_basis":
            s.set_gain_basis(np.array(modeling.gain_dpss_basis(F0 + DF * np.arange(p0.nfreqs), 100.0)))
        s.set_launch_mode("graph" if config == "graph" else "auto")
        s.set_optimizer("Adam", learning_rate=1e-2)
        first = np.array([r[0] for r in s.run_slices(20, tol=0.0)])
        if with_call:
            out = s.delay_cross_spectrum(op, norm_f, pairs, scale=scale, per_pair=True)
            assert out["per_pair"]["diff"]["resid"].sum() > 0
        second = np.array([r[0] for r in s.run_slices(20, tol=0.0)])
        losses[with_call] = np.concatenate([first, second], axis=1)
        final[with_call] = s.get_params()
        s.close()
    assert losses[True].shape == (2, 40)
    np.testing.assert_array_equal(losses[True], losses[False])
    for a, b in zip(final[True], final[False]):
        np.testing.assert_array_equal(a, b)


def test_errors_are_reported():
    import ctypes as C

    full, p0, pars = batch(7, 61, 2)
    op, norm_f = operator(61, 37)
    params = joined(pars)
    s = solver_of(full, params, np.float64)
    op_r, op_i = np.ascontiguousarray(op.real), np.ascontiguousarray(op.imag)
    pairs = np.array([[0, p0.nbls], [2, 2]], dtype=np.int32)
    scale = np.ones((2, 2))
    bins = np.zeros(2, dtype=np.int32)
    buf = np.empty((3, 2, 37))
    norm = np.empty(2)

    def code(ndelays=37, what=7, calibrated=0, npairs=2, pairs=pairs, scale=None, stats=3, nbins=0, bin_of_pair=None, op_r=op_r.ctypes.data,
             norm_f=norm_f.ctypes.data, cross_pair=None, diff_pair=None, cross_bin=None, diff_bin=None):
        d = _lib.DelayCrossDesc(ndelays, what, calibrated, npairs, None if pairs is None else pairs.ctypes.data, None if scale is None else scale.ctypes.data, stats,
                                nbins, bin_of_pair, op_r, op_i.ctypes.data, norm_f)
        ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        return s._lib.cal_solver_delay_cross_spectrum(s._h, C.byref(d), None, None, ptr(cross_pair), ptr(diff_pair), norm.ctypes.data, ptr(cross_bin),
                                                      ptr(diff_bin), None)

    INV = _lib.CAL_ERR_INVALID
    assert code() == 0 and code(scale=scale) == 0 and code(cross_pair=buf, diff_pair=buf.copy()) == 0
    assert code(what=0) == INV and code(what=8) == INV
    assert code(ndelays=0) == INV and code(ndelays=4097) == INV
    assert code(op_r=None) == INV and code(norm_f=None) == INV
    assert code(calibrated=2) == INV
    assert code(npairs=0) == INV and code(pairs=None) == INV
    assert code(stats=0) == INV and code(stats=4) == INV
    assert code(stats=2, cross_pair=buf) == INV and code(stats=1, diff_pair=buf) == INV  # an output whose bit is not set
    assert code(stats=1, cross_pair=buf) == 0 and code(stats=2, diff_pair=buf) == 0
    assert code(cross_bin=buf) == INV  # binned outputs with nbins == 0
    assert code(nbins=2) == INV  # bins without bin_of_pair
    assert code(nbins=2, bin_of_pair=bins.ctypes.data) == 0
    bins[1] = 2
    assert code(nbins=2, bin_of_pair=bins.ctypes.data) == INV
    bins[1] = -2
    assert code(nbins=2, bin_of_pair=bins.ctypes.data) == INV
    bad = pairs.copy()
    bad[1, 1] = full.nbls
    assert code(pairs=bad) == INV
    bad[1, 1] = -1
    assert code(pairs=bad) == INV
    for v in (np.inf, np.nan):
        sc = scale.copy()
        sc[0, 1] = v
        assert code(scale=sc) == INV
    assert s._lib.cal_solver_delay_cross_spectrum(s._h, None, None, None, None, None, None, None, None, None) == INV
    s.close()
    # state: gains neither set nor given
    from calamity_amd.solver import HipFitSolver

    s = HipFitSolver(dtype=np.float64)
    s.set_problem(full)
    s.set_data(full.data_r, full.data_i, full.wgts)
    s.set_params(c_r=params["c_r"], c_i=params["c_i"])
    with pytest.raises(_lib.CalamityHipError) as err:
        s.delay_cross_spectrum(op, norm_f, pairs)
    assert err.value.code == _lib.CAL_ERR_STATE
    assert s.delay_cross_spectrum(op, norm_f, pairs, g_r=params["g_r"], g_i=params["g_i"])["norm_pair"][0] > 0
    s.close()
