"""Delay spectra of redundant averages without a device: the float64 restatement (tests/delay_coherent_ref.py) against the fringe
restatement it is built on and against what the average is for (noise power falls as 1 / N); the sharing of ragged groups over workers;
the host plan of cal_solver_delay_coherent_spectrum through cal_debug_delay_coherent_plan (calamity_amd/csrc/report_plan.hpp) against
its rule restated in NumPy, with every refusal's message; the surface of the call; the build guard."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import delay_fringe_ref as FR
import test_delay_fringe_host as FH
import test_report_plan_host as RP
from calamity_amd import _lib, batched, distributed, solver
from calamity_amd.solver import problem_desc
from delay_coherent_ref import averaged, restated, sets_of, singleton_sets
from delay_spectrum_ref import NAMES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
noise, unitary = FH.noise, FH.unitary


def operator(rng, nf, nd):
    return rng.standard_normal((nf, nd)) + 1j * rng.standard_normal((nf, nd)), rng.uniform(0.5, 1.5, size=nf)


# ---- the restatement against itself -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("calibrated", [False, True])
@pytest.mark.parametrize("T", [1, 3])
def test_singleton_sets_are_the_fringe_restatement(T, calibrated):
    rng = np.random.default_rng(1)
    nb, nf, nd = 6, 24, 9
    d, m, G, w, rows = FH.slices(rng, nb, nf, T, flag_frac=0.2)
    op, norm_f = operator(rng, nf, nd)
    opt = unitary(T)
    scale = rng.uniform(0.5, 2.0, size=rows.shape)
    bins = np.array([0, 1, -1, 1, 0, 2], dtype=np.int32)
    want = FR.restated(d, m, G, w, op, norm_f, rows, opt, scale, calibrated, bins, 4)
    got = restated(d, m, G, w, op, norm_f, *singleton_sets(rows), opt, scale=scale, calibrated=calibrated, bin_of_group=bins, nbins=4)
    np.testing.assert_array_equal(got["norm_grp"], want["norm_grp"])
    np.testing.assert_array_equal(got["count_bin"], want["count_bin"])
    assert np.count_nonzero(want["norm_grp"]) == nb
    for k in NAMES:
        np.testing.assert_allclose(got["per_group"][k], want["per_group"][k], rtol=1e-12, atol=0)
        np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=0)
    # with one member per set the weighted mean of the sizes is the member's size: the bound is the fringe bound
    np.testing.assert_allclose(got["tau_per_unit"], want["tau_per_unit"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(got["tau_sum"] * 8.0 * (nf + 16), 3.0 * got["tau_per_unit"], rtol=1e-12, atol=0)  # N + 2 = 3


def test_conjugated_sets_under_the_conjugated_operator_in_float64():
    """Property (c): T = 1, opt = [[1]], singleton sets all conjugated and conj(op) -- equal here to the last bit as well, since NumPy's
    complex products change sign as a whole too."""
    rng = np.random.default_rng(2)
    d, m, G, w, rows = FH.slices(rng, 7, 24, 1, flag_frac=0.2)
    op, norm_f = operator(rng, 24, 9)
    sets = singleton_sets(rows)
    plain = restated(d, m, G, w, op, norm_f, *sets, np.ones((1, 1)))
    conj = restated(d, m, G, w, np.conj(op), norm_f, *sets, np.ones((1, 1)), member_conj=np.ones(7, dtype=np.uint8))
    for k in NAMES:
        np.testing.assert_array_equal(conj["per_group"][k], plain["per_group"][k])
        np.testing.assert_array_equal(conj["Z"][k], np.conj(plain["Z"][k]))
    assert np.any(plain["per_group"]["resid"])


def test_empty_flagged_and_disjoint_sets_and_both_weightings():
    rng = np.random.default_rng(3)
    nb, nf, nd, T = 8, 24, 9, 2
    d, m, G, w, _ = FH.slices(rng, nb, nf, T, flag_frac=0.1)
    w = w * rng.uniform(0.5, 2.0, size=w.shape)  # unequal weights
    w[1] = 0.0                                   # a row flagged throughout
    w[3, 1::2] = 0.0
    w[nb + 3, 0::2] = 0.0                        # rows 3 and nb + 3: disjoint masks
    op, norm_f = operator(rng, nf, nd)
    opt = unitary(T)
    groups = [[[0, 2], [nb, nb + 2]],   # 0: a plain pair
              [[], [nb + 4]],           # 1: an empty set
              [[1], [nb + 1]],          # 2: a set flagged throughout, alone
              [[1, 5], [nb + 5]],       # 3: the same row, carried by another
              [[3], [nb + 3]],          # 4: disjoint across t
              [[3, nb + 3], [nb + 3, 3]]]  # 5: disjoint inside the sets: each channel has one member
    set_ptr, member_row, ng, _ = sets_of(groups)
    omega = rng.uniform(0.5, 2.0, size=len(member_row))
    bins = np.zeros(ng, dtype=np.int32)
    out = {k: restated(d, m, G, w, op, norm_f, set_ptr, member_row, opt, member_wgt=omega, weighting=k, bin_of_group=bins, nbins=1) for k in (0, 1)}
    for k in (0, 1):
        o = out[k]
        np.testing.assert_array_equal(o["norm_grp"] > 0, [True, False, False, True, False, True])
        assert o["count_bin"][0] == 3
        for q in NAMES:
            assert not np.any(o["per_group"][q][[1, 2, 4]]) and np.all(np.any(o["per_group"][q][[0, 3, 5]], axis=(1, 2)))
        # group 3 is row 5 and row nb + 5 alone: the flagged member adds nothing, and a mean of one member has no weights left in it
        alone = restated(d, m, G, w, op, norm_f, *sets_of([[[5], [nb + 5]]])[:2], opt)
        np.testing.assert_allclose(o["per_group"]["data"][3], alone["per_group"]["data"][0], rtol=1e-12)
    assert np.any(np.abs(out[0]["per_group"]["data"][0] - out[1]["per_group"]["data"][0]) > 1e-6 * out[0]["per_group"]["data"][0])
    # the planes themselves: the weighted mean under the members' own masks, by hand for group 0, set 0
    for weighting in (0, 1):
        xbar, mask, abar, count = averaged(d, m, G, w, set_ptr, member_row, omega, None, weighting)
        u = np.stack([omega[i] * (w[r] if weighting else 1.0) * (w[r] != 0) for i, r in enumerate((0, 2))])
        want = np.where(u.sum(0) > 0, (u * d[[0, 2]]).sum(0) / np.where(u.sum(0) > 0, u.sum(0), 1.0), 0.0)
        np.testing.assert_allclose(xbar["data"][0], want, rtol=1e-13, atol=0)
        np.testing.assert_array_equal(mask[0], (w[0] != 0) | (w[2] != 0))
        np.testing.assert_array_equal(count[:4], [2, 2, 0, 1])
        assert np.all(np.abs(xbar["data"][0]) <= abar[0] * (1 + 1e-12)) and np.all(np.abs(xbar["resid"][0]) <= abar[0] * (1 + 1e-12))


@pytest.mark.parametrize("N", [1, 4, 16])
def test_noise_power_falls_as_one_over_the_members(N):
    """N members with the same sky, independent unit noise, one mask, uniform weighting: the mean residual power over all delays and
    groups is 1 / N of a single member's, within 5 standard errors estimated from the sample itself (2560 samples of an exponential
    law: a standard error of 2 % each)."""
    rng = np.random.default_rng(10 + N)
    ng, nf = 40, 64
    op = np.exp(-2j * np.pi * np.outer(np.arange(nf), np.arange(nf)) / nf) / np.sqrt(nf)  # unitary: independent delays
    norm_f = np.full(nf, 1.0 / nf)
    sky = 3.0 * noise(rng, (ng, nf))

    def power(n):
        d = np.repeat(sky, n, axis=0) + noise(rng, (ng * n, nf))
        m, G, w = np.repeat(sky, n, axis=0), np.ones((ng * n, nf), dtype=complex), np.ones((ng * n, nf))
        groups = [[list(range(g * n, (g + 1) * n))] for g in range(ng)]
        out = restated(d, m, G, w, op, norm_f, *sets_of(groups)[:2], np.ones((1, 1)))
        np.testing.assert_allclose(out["norm_grp"], 1.0, rtol=1e-12)
        return out["per_group"]["resid"].ravel()

    single, mean = power(1), power(N)
    n = len(single)
    assert n == ng * nf
    se = np.sqrt(N * N * mean.var(ddof=1) / n + single.var(ddof=1) / n)
    assert se < 0.05 * single.mean()
    print(f"N = {N}: N mean / single = {N * mean.mean() / single.mean():.4f}, standard error {se / single.mean():.4f}")
    assert abs(N * mean.mean() - single.mean()) <= 5.0 * se


# ---- the workers ------------------------------------------------------------------------------------------------------------------------
def test_ragged_groups_are_shared_out_over_the_workers_that_hold_all_their_rows():
    rows = [np.array([4, 5, 0, 1]), np.array([2, 3, 6, 7])]  # two workers, their global rows in local order
    groups = [[[0, 4], [1]], [[2, 6, 3], []], [[], [5, 5]], [[7], [6, 2]]]
    set_ptr, member_row, ng, T = sets_of(groups)
    sel, parts = batched.split_member_groups(set_ptr, member_row, T, rows, 8)
    np.testing.assert_array_equal(sel[0], [0, 2])
    np.testing.assert_array_equal(sel[1], [1, 3])
    np.testing.assert_array_equal(parts[0][0], [0, 2, 3, 3, 5])
    np.testing.assert_array_equal(parts[0][1], [2, 0, 3, 1, 1])
    np.testing.assert_array_equal(parts[0][2], [0, 1, 2, 6, 7])
    np.testing.assert_array_equal(parts[1][0], [0, 3, 3, 4, 6])
    np.testing.assert_array_equal(parts[1][1], [0, 2, 1, 3, 2, 0])
    np.testing.assert_array_equal(parts[1][2], [3, 4, 5, 8, 9, 10])
    assert parts[0][1].dtype == np.int32 and parts[0][0].dtype == np.int64
    with pytest.raises(ValueError, match="several workers"):
        batched.split_member_groups(*sets_of([[[0, 4], [2]], [[6], [7]]])[:2], 2, rows, 8)
    with pytest.raises(ValueError, match="holds no group"):
        batched.split_member_groups(*sets_of([[[0, 4], [5]]])[:2], 2, rows, 8)


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------
PLAN = {70: ("scalars", np.int64), 71: ("bin_ent", np.int32), 72: ("chunk_ptr", np.int32), 73: ("image", None), 74: ("norm_f", np.float64),
        75: ("scale", np.float64), 76: ("opt", np.float64), 77: ("chunk_members", np.int64)}
SCALARS = "nq xpitch ndpad cgroups nchunks n_x n_ypow n_out n_mask nspans".split()


def coherent_desc(dtype, op, norm_f, set_ptr, member_row, opt, member_wgt=None, member_conj=None, weighting=0, scale=None, what=7, nbins=0, bin_of_group=None,
                  ngroups=None, ntimes=None, nrates=None, nmembers=None, opt_i=True):
    arr = lambda a, t: None if a is None else np.ascontiguousarray(a, t)  # noqa: E731
    keep = [arr(op.real, dtype), arr(op.imag, dtype), arr(norm_f, np.float64), arr(bin_of_group, np.int32), arr(set_ptr, np.int64), arr(member_row, np.int32),
            arr(member_wgt, np.float64), arr(member_conj, np.uint8), arr(scale, np.float64), None if opt is None else arr(np.asarray(opt).real, np.float64),
            None if opt is None or not opt_i else arr(np.asarray(opt).imag, np.float64)]
    nt = np.shape(opt)[0] if ntimes is None else ntimes
    nr = np.shape(opt)[1] if nrates is None else nrates
    ng = (len(set_ptr) - 1) // max(nt, 1) if ngroups is None else ngroups
    nm = len(member_row) if nmembers is None else nmembers
    p = RP.ptr
    return _lib.DelayCoherentDesc(op.shape[1], what, 0, ng, nt, nr, p(keep[4]), p(keep[5]), p(keep[6]), p(keep[7]), weighting, p(keep[8]), nbins, p(keep[3]),
                                  p(keep[0]), p(keep[1]), p(keep[2]), p(keep[9]), p(keep[10]), nm), keep


def raw_call(prob, dtype, desc, bound, what, cap=1 << 21):
    d, keep = problem_desc(prob, dtype, "stream", "auto")
    code = _lib.CAL_F32 if np.dtype(dtype) == np.float32 else _lib.CAL_F64
    buf, n = np.zeros(cap, np.uint8), C.c_int64(0)
    rc = _lib.load().cal_debug_delay_coherent_plan(code, C.byref(d), None if desc is None else C.byref(desc), bound, what, buf.ctypes.data_as(C.c_void_p), cap,
                                                   C.byref(n))
    del keep
    return rc, buf[: max(0, min(cap, n.value))]


def coherent_plan(prob, dtype, *args, bound=0, **kw):
    desc, keep = coherent_desc(dtype, *args, **kw)
    out = {}
    for what, (name, dt) in PLAN.items():
        rc, got = raw_call(prob, dtype, desc, bound, what)
        _lib.check(rc)
        out[name] = got.view(dtype if dt is None else dt).copy()
    return out


@pytest.mark.parametrize("dtype", RP.DTYPES)
@pytest.mark.parametrize("ngroups,T,bound_groups", [(300, 3, 0), (300, 3, 7), (300, 3, 1), (5, 17, -1)])
def test_the_plan_cuts_whole_groups_and_counts_the_masks(ngroups, T, bound_groups, dtype):
    """The fringe rule with T pitch bytes of set masks more per group; the member lists as given (ones and zeros for what is left out);
    every chunk's members.  Three bounds, the smallest giving one group per chunk."""
    prob = RP.rows22()
    fpad, nd, nr = RP.fpad_of(prob, dtype), 37, min(T, 5)
    rng = np.random.default_rng(3)
    op, norm_f = operator(rng, prob.nfreqs, nd)
    opt = rng.standard_normal((T, nr)) + 1j * rng.standard_normal((T, nr))
    sizes = rng.integers(0, 5, size=ngroups * T)
    set_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    member_row = rng.integers(0, prob.nbls, size=set_ptr[-1]).astype(np.int32)
    bins = (np.arange(ngroups) % 4 - (np.arange(ngroups) % 9 == 0)).astype(np.int32)  # -1 .. 3; bin 4 stays empty
    size = np.dtype(dtype).itemsize
    xpitch = -(-fpad // 32) * 32
    fringe_bytes = 3 * 2 * T * xpitch * size + 3 * 2 * T * nd * 8 + 3 * nr * nd * 8
    per_group = fringe_bytes + T * xpitch
    bound = 1 if bound_groups < 0 else bound_groups * per_group + (per_group // 2 if bound_groups else 0)
    got = coherent_plan(prob, dtype, op, norm_f, set_ptr, member_row, opt, bound=bound, nbins=5, bin_of_group=bins)
    s = dict(zip(SCALARS, got["scalars"]))
    cgroups = min(max(1, (bound or RP.DEFAULT_BOUND) // per_group), ngroups)
    assert s["cgroups"] == cgroups == {0: ngroups, 7: 7, 1: 1, -1: 1}[bound_groups]
    # everything else is the fringe rule at that many groups per chunk: ask it with a bound that gives the same cut
    want = FH.fringe_rule(ngroups, T, nr, fpad, dtype, nd, nbins=5, bin_of_group=bins, bound=cgroups * fringe_bytes)
    np.testing.assert_array_equal(got["scalars"][:8], want["scalars"])
    np.testing.assert_array_equal(got["bin_ent"], want["bin_ent"])
    np.testing.assert_array_equal(got["chunk_ptr"], want["chunk_ptr"])
    assert s["n_mask"] == cgroups * T * xpitch and s["nspans"] == -(-xpitch // (64 * 16 // size))
    nchunks = s["nchunks"]
    members = got["chunk_members"].reshape(nchunks, 2)
    g0 = np.arange(nchunks) * cgroups
    np.testing.assert_array_equal(members[:, 0], set_ptr[g0 * T])
    np.testing.assert_array_equal(members[:, 1], set_ptr[np.minimum(g0 + cgroups, ngroups) * T])
    assert members[0, 0] == 0 and members[-1, 1] == len(member_row) and np.all(members[1:, 0] == members[:-1, 1])  # whole groups tile the members
    np.testing.assert_array_equal(got["scale"], np.ones(ngroups * T))
    np.testing.assert_array_equal(got["opt"], np.concatenate([opt.real.ravel(), opt.imag.ravel()]))
    np.testing.assert_array_equal(got["norm_f"], np.concatenate([norm_f, np.zeros(xpitch - prob.nfreqs)]))
    image = got["image"].reshape(2, xpitch, s["ndpad"])
    np.testing.assert_array_equal(image[0, : prob.nfreqs, :nd], op.real.astype(dtype))


def test_the_planner_refuses_what_the_call_refuses():
    prob = RP.rows22()
    nd = 8
    op, norm_f = np.zeros((prob.nfreqs, nd), np.complex128), np.ones(prob.nfreqs)
    set_ptr = np.array([0, 2, 3, 3, 5], np.int64)
    rows = np.array([0, 1, 2, 21, 21], np.int32)
    opt = np.array([[1.0, 1.0], [1.0, -1.0]], np.complex128)

    def refused(selector=70, bound=0, **kw):
        desc, keep = coherent_desc(np.float32, op, norm_f, **{"set_ptr": set_ptr, "member_row": rows, "opt": opt, **kw})
        rc, _ = raw_call(prob, np.float32, desc, bound, selector)
        return rc, _lib.load().cal_last_error().decode()

    assert refused()[0] == 0 and refused(member_wgt=np.ones(5), member_conj=[0, 1, 0, 1, 1], weighting=1, selector=77)[0] == 0
    INV = _lib.CAL_ERR_INVALID
    bad_opt = opt.copy()
    bad_opt[1, 0] = np.nan
    who = "delay_coherent_spectrum: "
    for kw, text in ((dict(ngroups=0), "ngroups = 0 (at least 1)"),
                     (dict(ntimes=0), "ntimes = 0 lies outside [1, 64]"),
                     (dict(ntimes=65, ngroups=1), "ntimes = 65 lies outside [1, 64]"),
                     (dict(nrates=0), "nrates = 0 lies outside [1, 64]"),
                     (dict(nrates=65), "nrates = 65 lies outside [1, 64]"),
                     (dict(weighting=2), "weighting = 2 (0: the coefficients, 1: coefficients times weights)"),
                     (dict(weighting=-1), "weighting = -1 (0: the coefficients, 1: coefficients times weights)"),
                     (dict(nmembers=(1 << 30) + 1), "nmembers = 1073741825 lies outside [0, 2^30]"),
                     (dict(nmembers=-1), "nmembers = -1 lies outside [0, 2^30]"),
                     (dict(set_ptr=None, ngroups=2), "null set_ptr"),
                     (dict(member_row=None, nmembers=5), "null member_row"),
                     (dict(opt=None, ntimes=2, nrates=2), "null opt"), (dict(opt_i=False), "null opt"),
                     (dict(set_ptr=[1, 2, 3, 3, 5]), "set_ptr[0] = 1 (it starts at 0)"),
                     (dict(set_ptr=[0, 2, 1, 3, 5]), "set_ptr[2] = 1 falls below set_ptr[1] = 2"),
                     (dict(set_ptr=[0, 2, 3, 3, 4]), "set_ptr ends at 4, not at nmembers = 5"),
                     (dict(nmembers=6, member_row=[0, 1, 2, 21, 21, 0]), "set_ptr ends at 5, not at nmembers = 6"),
                     (dict(member_row=[0, 1, 2, 21, 22]), "member_row[4] = 22 lies outside [0, 22)"),
                     (dict(member_row=[-1, 1, 2, 21, 21]), "member_row[0] = -1 lies outside [0, 22)"),
                     (dict(member_wgt=[1.0, -0.5, 1.0, 1.0, 1.0]), "member_wgt[1] is negative or not finite"),
                     (dict(member_wgt=[1.0, 1.0, np.inf, 1.0, 1.0]), "member_wgt[2] is negative or not finite"),
                     (dict(member_wgt=[1.0, 1.0, 1.0, 1.0, np.nan]), "member_wgt[4] is negative or not finite"),
                     (dict(member_conj=[0, 0, 2, 0, 0]), "member_conj[2] = 2 (0 or 1)"),
                     (dict(scale=np.array([[1.0, 1.0], [np.inf, 1.0]])), "scale[1][0] is not finite"),
                     (dict(opt=bad_opt), "opt[1][0] is not finite"),
                     (dict(nbins=2, bin_of_group=[0, 2]), "bin_of_group[1] = 2 lies outside [-1, 2)"),
                     (dict(nbins=2, bin_of_group=[-2, 0]), "bin_of_group[0] = -2 lies outside [-1, 2)")):
        rc, msg = refused(**kw)
        assert rc == INV and msg == who + text, (kw, msg)
    assert refused(member_wgt=[1.0, 0.0, 1.0, 1.0, 1.0])[0] == 0  # a coefficient of zero is a coefficient
    for kw in (dict(what=0), dict(what=8), dict(nbins=-1), dict(nbins=2), dict(bin_of_group=[0, 0])):
        rc, msg = refused(**kw)
        assert rc == INV and "takes a description cal_solver_delay_coherent_spectrum would plan for" in msg, (kw, msg)
    assert refused(bound=-1)[0] == INV
    assert raw_call(prob, np.float32, None, 0, 70)[0] == INV  # no description
    assert refused(selector=78)[0] == INV and refused(selector=69)[0] == INV  # the range is 70 .. 77


# ---- the surface ------------------------------------------------------------------------------------------------------------------------
def test_the_methods_and_the_binding():
    for cls in (solver.HipFitSolver, batched.SliceBatchFitter):
        params = inspect.signature(cls.delay_coherent_spectrum).parameters
        assert list(params)[1:] == ["op", "norm_f", "set_ptr", "member_row", "opt", "member_wgt", "member_conj", "weighting", "scale", "what", "calibrated",
                                    "bin_of_group", "nbins", "per_group", "g_r", "g_i"]
        assert params["member_wgt"].default is None and params["member_conj"].default is None and params["weighting"].default == "uniform"
        assert params["scale"].default is None and params["what"].default == ("data", "model", "resid") and params["calibrated"].default is False
        assert params["nbins"].default == 0 and params["per_group"].default is False and params["bin_of_group"].default is None
    names = [f[0] for f in _lib.DelayCoherentDesc._fields_]
    fringe = [f[0] for f in _lib.DelayFringeDesc._fields_]
    at = fringe.index("rows")
    assert names == fringe[:at] + ["set_ptr", "member_row", "member_wgt", "member_conj", "weighting"] + fringe[at + 1 :] + ["nmembers"]
    text = open(os.path.join(ROOT, "include", "calamity_hip.h")).read()
    fields = text.split("typedef struct cal_delay_coherent_desc {")[1].split("}")[0]
    assert re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", fields)) == names
    for word in ("cal_solver_delay_coherent_spectrum(", "cal_debug_delay_coherent_plan(", "then rounded ONCE to the solver's dtype",
                 "mask_g[f]   = AND over t of mask_(g,t)[f]", "acc += u * (double) q with contraction off", "ONE all-reduce of\n * nwhat nbins nrates ndelays + nbins doubles",
                 "An empty set gives its group norm_grp == 0"):
        assert word in text, word
    lib = _lib.load()
    assert hasattr(lib, "cal_solver_delay_coherent_spectrum") and hasattr(lib, "cal_debug_delay_coherent_plan")
    spec = distributed.exchange_spec(7, 64, delay_coherent=(3, 5, 8, 37))
    assert spec["delay_coherent_f64"] == 3 * 5 * 8 * 37 + 5
    assert {k: v for k, v in spec.items() if k != "delay_coherent_f64"} == distributed.exchange_spec(7, 64)
    assert "delay_coherent_f64" not in distributed.exchange_spec(7, 64, delay_fringe=(3, 5, 8, 37))


def test_the_python_checks_come_before_the_library():
    s = object.__new__(solver.HipFitSolver)  # no device: the checks below never reach it
    s.nfreqs, s.nants, s.dtype = 8, 3, np.float32
    op, norm_f, opt = np.zeros((8, 4), complex), np.ones(8), np.ones((2, 2))
    call = lambda **kw: s.delay_coherent_spectrum(**{**dict(op=op, norm_f=norm_f, set_ptr=[0, 1, 2], member_row=[0, 1], opt=opt), **kw})  # noqa: E731
    for kw, text in ((dict(weighting="both"), "weighting"), (dict(set_ptr=[0, 1, 2, 3]), "set_ptr"), (dict(member_wgt=[1.0]), "member_wgt"),
                     (dict(member_conj=[0]), "member_conj"), (dict(scale=np.ones((2, 2))), "scale"), (dict(nbins=2), "bin_of_group"),
                     (dict(what=("noise",)), "what"), (dict(g_r=np.ones((3, 8))), "g_r"), (dict(opt=np.ones(2)), "opt")):
        with pytest.raises(ValueError, match=text):
            call(**kw)


# ---- the build guard --------------------------------------------------------------------------------------------------------------------
def test_the_build_guard_refuses_a_spilling_coherent_kernel():
    script = os.path.join(ROOT, "calamity_amd", "csrc", "check_resources.py")

    def remarks(name, scratch, vspill, occ=1):  # (no occupancy rule for the two: 1 passes)
        return (f"./x.hpp:1:1: remark: Function Name: {name} [-Rpass-analysis=kernel-resource-usage]\n"
                f"./x.hpp:1:1: remark:     ScratchSize [bytes/lane]: {scratch} [-Rpass-analysis=kernel-resource-usage]\n"
                f"./x.hpp:1:1: remark:     Occupancy [waves/SIMD]: {occ} [-Rpass-analysis=kernel-resource-usage]\n"
                f"./x.hpp:1:1: remark:     VGPRs Spill: {vspill} [-Rpass-analysis=kernel-resource-usage]\n")

    def run(text):
        return subprocess.run([sys.executable, script], input=text, capture_output=True, text=True)

    dense = remarks("_ZN4calk18fused_dense_kernelILb1EEEvNS_8MfmaArgsE", 0, 0, occ=2)
    names = {f"{k}<{t}>": f"_ZN4calk21{k}I{t}EEvPKT_" for k in ("dcoherent_rows_kernel", "dcoherent_mask_kernel") for t in "fd"}
    assert run(dense + "".join(remarks(n, 0, 0) for n in names.values())).returncode == 0
    for k, n in names.items():
        for scratch, vspill in ((16, 0), (0, 4)):
            bad = run(dense + remarks(n, scratch, vspill))
            assert bad.returncode != 0 and k.split("<")[0] in bad.stdout + bad.stderr, (k, scratch, vspill)
    log = os.path.join(ROOT, "calamity_amd", "csrc", "resources.log")
    if os.path.exists(log):  # the build's own remarks name all four
        text = open(log).read()
        assert all(f"{k}I{t}E" in text for k in ("dcoherent_rows_kernel", "dcoherent_mask_kernel") for t in "fd")


# ---- the drop-in ------------------------------------------------------------------------------------------------------------------------
CALLS = ["calibrate_and_model_tensor", "calibrate_and_model_mixed", "calibrate_and_model_dpss", "read_calibrate_and_model_dpss"]
ON = dict(delay_redundant_spectrum=True, delay_spectrum=True, delay_spectrum_calibrated=True)


@pytest.mark.parametrize("bad", [dict(delay_redundant_spectrum=True), dict(delay_redundant_spectrum=True, delay_spectrum=True),
                                 dict(ON, delay_spectrum_calibrated=False), dict(ON, batch_slices=False), dict(ON, batch_slices=1),
                                 dict(ON, delay_redundant_times=3, batch_slices=2), dict(ON, init_guesses_from_previous_time_step=True),
                                 dict(ON, delay_redundant_times=0), dict(ON, delay_redundant_times=65), dict(ON, delay_redundant_times=2.5),
                                 dict(ON, delay_redundant_times=True), dict(ON, delay_redundant_taper="hann"), dict(ON, delay_redundant_weighting="both"),
                                 dict(ON, delay_redundant_weighting=1), dict(ON, device_split="groups"),
                                 dict(delay_redundant_spectrum="yes", delay_spectrum=True, delay_spectrum_calibrated=True)])
@pytest.mark.parametrize("name", CALLS)
def test_bad_keywords_are_refused_before_anything_is_touched(name, bad):
    from calamity_amd import calibration

    call = getattr(calibration, name)
    with pytest.raises(ValueError, match="delay_redundant_spectrum"):
        call(None, {}, **bad) if name == "calibrate_and_model_tensor" else call(None, **bad)  # (no data, no device: the check comes first)


@pytest.mark.parametrize("name", CALLS)
def test_the_keywords_are_off_by_default_in_their_place_and_python_keywords_only(name):
    from calamity_amd import calibration
    from calamity_amd.fit_loop import FitControls

    params = inspect.signature(getattr(calibration, name)).parameters
    assert params["delay_redundant_spectrum"].default is False and params["delay_redundant_times"].default == 2
    assert params["delay_redundant_taper"].default == "none" and params["delay_redundant_weighting"].default == "weights"
    names = list(params)
    at = names.index("delay_fringe_spectrum")
    assert names[at - 4 : at] == ["delay_redundant_spectrum", "delay_redundant_times", "delay_redundant_taper", "delay_redundant_weighting"]
    assert not any(n.startswith("delay_spectrum") and "redundant" in n for n in names)
    assert not any("redundant" in f for f in FitControls().keywords())
    assert not any("delay_redundant" in a.dest for a in calibration.dpss_fit_argparser()._actions)


def line_array(flip=()):
    """Seven antennas on a line, 10 m apart: 21 pairs in six groups of 6, 5, 4, 3, 2, 1 members at 10 .. 60 m.  ``flip``: pairs the data
    object holds the other way round."""
    from calamity_amd import uvcompat

    antpos = np.stack([10.0 * np.arange(7), np.zeros(7), np.zeros(7)], axis=1)
    pairs = [(j, i) if (i, j) in flip else (i, j) for i in range(7) for j in range(i + 1, 7)]
    return uvcompat.SimpleUVData(antpos, pairs, 150e6 + 1e5 * np.arange(16), 2458000.0 + 1e-4 * np.arange(4), pols=(-5, -6))


def test_the_groups_of_a_line_of_seven():
    import types

    from calamity_amd import calibration

    flip = {(0, 1), (2, 5), (3, 6)}
    uvd = line_array(flip)
    # the fit's rows: the pairs in ascending order, four of them held the other way round (two of those the data hold reversed as well)
    held = [(i, j) for i in range(7) for j in range(i + 1, 7)]
    reversed_rows = {(0, 1), (1, 3), (2, 5), (4, 6)}
    a0 = np.array([j if (i, j) in reversed_rows else i for i, j in held], dtype=np.int32)
    a1 = np.array([i if (i, j) in reversed_rows else j for i, j in held], dtype=np.int32)
    prob = types.SimpleNamespace(bl_ant0=a0, bl_ant1=a1, nbls=21)
    red = calibration.delay_redundant_setup(uvd, np.arange(7), prob, 2, taper="none", weighting="uniform", per_group=True, bllen_bin=25.0)
    assert red["ntimes"] == 2 and red["weighting"] == "uniform" and red["per_group"] is True and red["opt"].shape == (2, 2)
    # every row in exactly one set; groups by separation
    np.testing.assert_array_equal(np.sort(np.concatenate(red["rows"])), np.arange(21))
    assert sorted(len(r) for r in red["rows"]) == [1, 2, 3, 4, 5, 6]
    for rows, conj, pairs, length in zip(red["rows"], red["conj"], red["pairs"], red["lengths"]):
        sep = {abs(held[b][1] - held[b][0]) for b in rows}
        assert len(sep) == 1 and abs(length - 10.0 * sep.pop()) < 1e-9 and len(pairs) == len(rows)
        for b, c, ap in zip(rows, conj, pairs):
            assert {int(a0[b]), int(a1[b])} == set(ap)
            assert c == int((int(a0[b]), int(a1[b])) != ap)  # conjugated where the row holds the group's pair reversed
        # the group's pairs all point one way
        assert len({np.sign(ap[1] - ap[0]) for ap in pairs}) == 1
    flipped = {frozenset((int(a0[b]), int(a1[b]))) for rows, conj in zip(red["rows"], red["conj"]) for b, c in zip(rows, conj) if c}
    assert flipped in ({frozenset(p) for p in reversed_rows}, {frozenset(p) for p in held} - {frozenset(p) for p in reversed_rows})
    assert 0 < sum(int(c.sum()) for c in red["conj"]) < 21
    # the bins of the groups' lengths at 25 m: 10, 20 | 30, 40 | 50, 60
    order = np.argsort(red["lengths"])
    np.testing.assert_array_equal(np.asarray(red["bin_of_group"])[order], [0, 0, 1, 1, 2, 2])
    np.testing.assert_allclose(red["bllen_m"], [15.0, 35.0, 55.0])
    # flipping pairs in the data object changes nothing: the groups come from the positions, the orientation from the fit's rows
    again = calibration.delay_redundant_setup(line_array(), np.arange(7), prob, 2, taper="none", weighting="uniform", per_group=True, bllen_bin=25.0)
    for k in ("rows", "conj"):
        for x, y in zip(red[k], again[k]):
            np.testing.assert_array_equal(x, y)
    # pairs without a row are dropped, and so are groups without rows
    few = types.SimpleNamespace(bl_ant0=a0[:6], bl_ant1=a1[:6], nbls=6)  # the rows of antenna 0 alone: one per separation
    part = calibration.delay_redundant_setup(uvd, np.arange(7), few, 1, bllen_bin=25.0)
    assert [len(r) for r in part["rows"]] == [1] * 6 and part["per_group"] is False and part["opt"].shape == (1, 1)

    # the windows across two polarizations, and the sets of a batch: four times of two polarizations, slice-major
    polnums, tidx = [0, 0, 0, 0, 1, 1, 1, 1], [0, 1, 2, 3, 0, 1, 2, 3]
    windows = calibration.delay_fringe_windows(polnums, tidx, 2, red["times"], red["dt"])
    assert windows == [(0, 1), (2, 3), (4, 5), (6, 7)]
    assert calibration.delay_fringe_windows([0, 0, 0, 1, 1, 1], [0, 1, 2, 0, 1, 2], 2) == [(0, 1), (3, 4)]  # none spans the polarizations
    rms = np.arange(1.0, 9.0)
    set_ptr, member_row, member_conj, scale, bins = calibration.delay_redundant_sets(windows, red, rms, 21)
    ng = len(red["rows"])
    assert len(set_ptr) == 4 * ng * 2 + 1 and set_ptr[0] == 0 and set_ptr[-1] == len(member_row) == 8 * 21 and scale.shape == (4 * ng, 2)
    assert set_ptr.dtype == np.int64 and member_row.dtype == np.int32 and member_conj.dtype == np.uint8 and bins.dtype == np.int32
    np.testing.assert_array_equal(np.sort(member_row), np.arange(8 * 21))  # every row of the batch in exactly one set
    for k, win in enumerate(windows):
        for g in range(ng):
            for i, t in enumerate(win):
                v = (k * ng + g) * 2 + i
                np.testing.assert_array_equal(member_row[set_ptr[v] : set_ptr[v + 1]], t * 21 + red["rows"][g])
                np.testing.assert_array_equal(member_conj[set_ptr[v] : set_ptr[v + 1]], red["conj"][g])
            np.testing.assert_array_equal(scale[k * ng + g], [rms[t] for t in win])
            assert bins[k * ng + g] == k * red["nbins"] + red["bin_of_group"][g]
    one = calibration.delay_redundant_sets([(0,), (1,)], dict(part, ntimes=1), rms, 6)
    np.testing.assert_array_equal(one[3], np.ones((12, 1)))  # windows of one time: unit scales, rms^2 behind the square


def test_the_entry_of_a_window():
    from calamity_amd import calibration

    red = dict(rows=[np.array([0, 1]), np.array([2]), np.array([3, 4, 5])], pairs=[[(0, 1), (1, 2)], [(0, 2)], [(3, 4), (4, 5), (5, 6)]], nbins=2,
               bin_of_group=np.array([0, 1, 0]), bllen_m=np.array([10.0, 20.0]), rates_hz=np.array([-0.1, 0.0]), ntimes=2)
    rng = np.random.default_rng(5)
    out = {q: rng.uniform(size=(4, 2, 3)) for q in NAMES}
    out["count_bin"] = np.array([2.0, 1.0, 1.0, 0.0])
    out["per_group"] = {q: rng.uniform(size=(6, 2, 3)) for q in NAMES}
    e = calibration.delay_redundant_entry(out, red, 1, [4, 5], rms=3.0)
    assert e["time_indices"] == [4, 5] and list(e["ngroups"]) == [1, 0] and list(e["nmembers"]) == [2, 1, 3]
    np.testing.assert_array_equal(e["bllen_m"], [10.0, 20.0])
    np.testing.assert_array_equal(e["fringe_rates"], [-0.1, 0.0])
    for q in NAMES:
        np.testing.assert_array_equal(e[q][0], out[q][2])
        assert not np.any(e[q][1])  # a bin without a counted group
        assert list(e["groups"]) == [(0, 1), (0, 2), (3, 4)] and e["groups"][(3, 4)]["antpairs"] == [(3, 4), (4, 5), (5, 6)]
        np.testing.assert_array_equal(e["groups"][(0, 2)][q], out["per_group"][q][4])
    one = calibration.delay_redundant_entry(out, dict(red, ntimes=1), 0, [7], rms=3.0)  # one time: rms^2 sum / count, delay_spectrum_entry's order
    np.testing.assert_array_equal(one["data"][0], (3.0 ** 2 * (1.0 / 2.0)) * out["data"][0])
    np.testing.assert_array_equal(one["groups"][(0, 1)]["data"], 9.0 * out["per_group"]["data"][0])
    tables = calibration.delay_spectrum_tables({0: {4: {"delay_spectrum": dict(delays_ns=np.arange(3.0), bllen_m=np.ones(1), nbls=np.ones(1), data=np.ones((1, 3)),
                                                                                model=np.ones((1, 3)), resid=np.ones((1, 3)), redundant=e)}}})
    assert tables["redundant_data"].shape == (1, 5, 2, 2, 3) and np.all(np.isnan(tables["redundant_data"][0, :4]))
    np.testing.assert_array_equal(tables["redundant_data"][0, 4], e["data"])
    np.testing.assert_array_equal(tables["redundant_window"][0, 4], [4, 5])
    np.testing.assert_array_equal(tables["redundant_antpairs"], [[0, 1], [0, 2], [3, 4]])
    np.testing.assert_array_equal(tables["redundant_resid_grp"][0, 4, 2], e["groups"][(3, 4)]["resid"])
