"""The host side of the delay transfer (cal_solver_delay_transfer): the restatement tests/delay_transfer_ref.py against a Monte Carlo of
what it claims to predict and against two identities, the plan of csrc/report_plan.hpp through cal_debug_report_plan, the keyword surface
of the four drop-in calls, the binding, the header text, the exchange spec and the build guard.  No device.

Monte Carlo: a group of three baselines, 61 channels, 9 vectors, random complex gains, random weights with 7 flagged channels per row,
one row with uniform weights, a Blackman-tapered shifted DFT; noise of variance 1 / w on the unflagged samples, the coefficients at
their weighted least-squares optimum.  The mean delay power of the masked data must be noise_bl and that of the masked residual
noise_bl - num.  One delay's power is exponentially distributed, so a mean over D draws scatters by noise_bl / sqrt(D): the bound is
5 / sqrt(D) of noise_bl over all rows and delays (measured 3.0 / sqrt(D) at 20 000 draws)."""
import ctypes as C
import hashlib
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

import _plan_cases as pc
from calamity_amd import _lib, batched, calibration, distributed, solver
from calamity_amd.solver import problem_desc
from delay_transfer_ref import bin_rows, core

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRAWS = 20000
F, NV, NB = 61, 9, 3


def shifted_dft(n, taper=None):
    k = np.fft.fftshift(np.arange(n))
    op = np.exp(-2j * np.pi * np.outer(np.arange(n), k) / n)
    return op if taper is None else taper[:, None] * op


def monte_carlo_case(seed=0):
    rng = np.random.default_rng(seed)
    A = [np.linalg.qr(rng.standard_normal((F, NV)))[0] * np.sqrt(F / NV) for _ in range(NB)]
    G = (1.0 + 0.3 * rng.standard_normal((NB, F))) * np.exp(2j * np.pi * rng.uniform(size=(NB, F)))
    w = rng.uniform(0.5, 2.0, size=(NB, F))
    w[1] = 1.3  # one row with uniform weights
    for b in range(NB):
        w[b, rng.choice(F, 7, replace=False)] = 0.0
    return A, G, w, shifted_dft(F, np.blackman(F))


def sample_terms(G, w, calibrated):
    mask = w != 0
    q = w * np.abs(G) ** 2
    if calibrated:
        live = mask & (np.abs(G) ** 2 != 0)
        return q, live.astype(np.complex128), np.where(live, 1.0 / np.where(live, q, 1.0), 0.0), mask
    return q, np.where(mask, G, 0.0), np.where(mask, 1.0 / np.where(mask, w, 1.0), 0.0), mask


@pytest.mark.parametrize("calibrated", [False, True], ids=["raw", "calibrated"])
def test_monte_carlo_of_the_absorbed_noise_power(calibrated):
    A, G, w, op = monte_carlo_case()
    q, s, v, mask = sample_terms(G, w, calibrated)
    num, noise, W, _ = core(A, q, s, v, op, 0.0)
    assert np.all(num >= 0) and np.all(num <= noise * (1 + 1e-12)) and np.all(noise > 0)  # 0 <= absorbed_bl <= 1
    rng = np.random.default_rng(1)
    sigma = np.where(mask, 1.0 / np.sqrt(np.where(mask, w, 1.0)), 0.0)
    d = sigma * (rng.standard_normal((DRAWS, NB, F)) + 1j * rng.standard_normal((DRAWS, NB, F))) / np.sqrt(2.0)
    # the weighted least-squares optimum of sum w |d - G (A c)|^2 over the group's nine complex coefficients
    N = sum(A[b].T @ (q[b][:, None] * A[b]) for b in range(NB))
    rhs = sum((d[:, b] * (w[b] * np.conj(G[b]))) @ A[b] for b in range(NB))  # [draws, nvec]
    c = np.linalg.solve(N, rhs.T).T
    worst = {}
    for name in ("data", "resid"):
        dev = 0.0
        for b in range(NB):
            m = c @ A[b].T  # [draws, F]
            if calibrated:
                ok = np.abs(G[b]) ** 2 != 0
                x = np.where(ok, d[:, b] / np.where(ok, G[b], 1.0), 0.0) - (np.where(ok, m, 0.0) if name == "resid" else 0.0)
            else:
                x = d[:, b] - (G[b] * m if name == "resid" else 0.0)
            power = np.mean(np.abs(np.where(mask[b], x, 0.0) @ op) ** 2, axis=0)
            want = noise[b] - (num[b] if name == "resid" else 0.0)
            dev = max(dev, float(np.max(np.abs(power - want) / noise[b])))
        worst[name] = dev
    print(f"calibrated={calibrated}: {DRAWS} draws, largest deviation / noise_bl  " + "  ".join(f"{k} {v * np.sqrt(DRAWS):.2f} / sqrt(draws)" for k, v in worst.items()))
    assert max(worst.values()) <= 5.0 / np.sqrt(DRAWS), worst


def test_the_identity_with_model_var():
    """With the unshifted rectangular DFT of all F delays, sum_k num[b][k] = F sum_f mask |G|^2 model_var[b][f]."""
    A, G, w, _ = monte_carlo_case(seed=3)
    op = np.exp(-2j * np.pi * np.outer(np.arange(F), np.arange(F)) / F)
    for ridge in (0.0, 1e-6):
        q, s, v, mask = sample_terms(G, w, False)
        num, noise, W, _ = core(A, q, s, v, op, ridge)
        for b in range(NB):
            model_var = np.sum((W @ A[b].T) ** 2, axis=0)
            want = F * np.sum(mask[b] * np.abs(G[b]) ** 2 * model_var)
            assert abs(num[b].sum() - want) <= 1e-12 * want, (ridge, b)


def test_one_clean_baseline_absorbs_as_many_delays_as_it_has_vectors():
    rng = np.random.default_rng(4)
    A = [np.linalg.qr(rng.standard_normal((F, NV)))[0]]
    G = np.exp(2j * np.pi * rng.uniform(size=(1, F)))  # |G| = 1
    w = np.full((1, F), 0.7)
    op = np.exp(-2j * np.pi * np.outer(np.arange(F), np.arange(F)) / F)
    for calibrated in (False, True):
        q, s, v, _ = sample_terms(G, w, calibrated)
        num, noise, _, _ = core(A, q, s, v, op, 0.0)
        absorbed = num / noise
        assert abs(absorbed.sum() - NV) <= 1e-12 * NV
        assert absorbed.min() >= 0.0 and absorbed.max() <= 1.0 + 1e-12


def test_the_restatement_bins_sequentially_and_leaves_dead_rows_out():
    rows = np.arange(12.0).reshape(4, 3)
    out, count = bin_rows(rows, np.asarray([True, True, False, True]), [0, 1, 0, 0], 3)
    np.testing.assert_array_equal(out, [rows[0] + rows[3], rows[1], np.zeros(3)])
    np.testing.assert_array_equal(count, [2, 1, 0])
    assert core([np.ones((4, 2))], np.zeros((1, 4)), np.zeros((1, 4), complex), np.zeros((1, 4)), np.ones((4, 3), complex), 1e-6) is None  # tr N == 0


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------
FE_PIECE, DS_STEP, DS_COLS = 64, 32, 64  # kFePiece, kDsStep, kDsCols
DEFAULT_BOUND = 256 << 20
GROUP = np.dtype([("b0", "<i4"), ("b1", "<i4"), ("nvec", "<i4"), ("coff", "<i4"), ("fb_log2", "<i4"), ("slice", "<i4"), ("noff", "<i8"), ("doff", "<i8")])
CHUNK = np.dtype([(k, "<i4") for k in ("g0", "g1", "w0", "w1", "r0", "r1", "q0", "q1")] + [("lds", "<i8")])
RUN = np.dtype([("soff", "<i8"), ("grp", "<i4"), ("b0", "<i4"), ("b1", "<i4"), ("pad", "<i4")])
ROW = np.dtype([("soff", "<i8"), ("b", "<i4"), ("grp", "<i4")])
TRANSFER = {40: ("scalars", np.int64), 41: ("grp", GROUP), 42: ("order", np.int32), 43: ("chunks", CHUNK), 44: ("woff", np.int64), 45: ("runs", RUN),
            46: ("rows", ROW), 47: ("bin_ent", np.int32), 48: ("bin_ptr", np.int32)}
SCALARS = "xpitch ndpad npieces n_max d_max x_max nchunks nruns nrows n_rows_out n_out".split()


def raw_call(prob, dtype, layout, report, what, cap=1 << 21):
    d, keep = problem_desc(prob, dtype, layout, "auto")
    code = _lib.CAL_F32 if np.dtype(dtype) == np.float32 else _lib.CAL_F64
    buf, n = np.zeros(cap, np.uint8), C.c_int64(0)
    rc = _lib.load().cal_debug_report_plan(code, C.byref(d), C.byref(report), what, buf.ctypes.data_as(C.c_void_p), cap, C.byref(n))
    del keep
    return rc, buf[: max(0, min(cap, n.value))].copy()


def transfer_plan(prob, dtype, layout, ndelays, bound=0, nbins=0, bin_of_bl=None):
    op = np.zeros((prob.nfreqs, ndelays), dtype)
    bins = None if bin_of_bl is None else np.ascontiguousarray(bin_of_bl, np.int32)
    desc = _lib.DelayTransferDesc(ndelays, 0, nbins, None if bins is None else bins.ctypes.data, op.ctypes.data, op.ctypes.data, 1e-6)
    report = _lib.ReportPlanDesc(transfer=C.pointer(desc), scratch_bytes=bound)
    out = {}
    for what, (name, dt) in TRANSFER.items():
        rc, got = raw_call(prob, dtype, layout, report, what)
        _lib.check(rc)
        out[name] = got.view(dt)
    out.update(zip(SCALARS, (int(x) for x in out["scalars"])))
    return out


def fe_pad(n):
    return (n + 15) & ~15


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("layout", ["shared", "stream"])
@pytest.mark.parametrize("bound", [0, 1, 200_000, 1_000_000])
def test_the_plan_cuts_groups_by_the_rule_of_the_closed_form_solves(bound, layout, dtype):
    prob = pc.groups()
    nbls, size = prob.nbls, np.dtype(dtype).itemsize
    bins = (np.arange(nbls) % 3 - (np.arange(nbls) % 7 == 0)).astype(np.int32)  # -1, 0, 1, 2
    P = transfer_plan(prob, dtype, layout, 37, bound=bound, nbins=4, bin_of_bl=bins)
    grp, order, chunks, runs, rows = P["grp"], P["order"], P["chunks"], P["runs"], P["rows"]
    nvec = grp["nvec"].astype(np.int64)
    assert P["ndpad"] == 64 and P["xpitch"] % DS_STEP == 0 and P["xpitch"] >= prob.nfreqs and P["npieces"] == -(-96 // FE_PIECE)
    assert P["n_rows_out"] == nbls * 37 and P["n_out"] == nbls + 4 * 37 + 4
    np.testing.assert_array_equal(order, np.argsort(-nvec, kind="stable"))  # heaviest first
    # the runs: every group's baselines in order, cut where the row block (the tiles) changes
    want_runs = []
    for g in order:
        b0, b1 = int(grp["b0"][g]), int(grp["b1"][g])
        cuts = [b0] + [b for b in range(b0 + 1, b1) if prob.bl_rowblk[b] != prob.bl_rowblk[b - 1]] + [b1]
        want_runs += [(g, a, b) for a, b in zip(cuts[:-1], cuts[1:])]
    assert [(int(r["grp"]), int(r["b0"]), int(r["b1"])) for r in runs] == want_runs
    assert P["nruns"] == len(runs) and P["nrows"] == len(rows) == nbls
    np.testing.assert_array_equal(rows["b"], np.concatenate([np.arange(a, b) for _, a, b in want_runs]))
    nruns_of = np.bincount(runs["grp"], minlength=len(grp))
    npad = np.asarray([fe_pad(int(n)) for n in nvec], dtype=np.int64)
    extra = npad * npad + nruns_of * npad * P["xpitch"]
    limit = bound or DEFAULT_BOUND
    assert chunks["g0"][0] == 0 and chunks["g1"][-1] == len(grp) and np.all(chunks["g0"][1:] == chunks["g1"][:-1]) and P["nchunks"] == len(chunks)
    n_max = d_max = x_max = 0
    for i, ch in enumerate(chunks):
        gs = order[ch["g0"] : ch["g1"]]
        assert len(gs) >= 1  # never less than one group
        nbytes = int((nvec[gs] ** 2).sum() + extra[gs].sum()) * size + int(((nvec[gs] + 2) * nvec[gs]).sum()) * 8
        assert len(gs) == 1 or nbytes <= limit  # under the bound, but for a group that alone needs more
        if ch["g1"] < len(grp):  # the next group would not have fitted
            nxt = order[ch["g1"]]
            assert nbytes + int(nvec[nxt] ** 2 + extra[nxt]) * size + int((nvec[nxt] + 2) * nvec[nxt]) * 8 > limit
        # the offsets restart in every chunk: N, the factor, W then S of the group's runs
        noff = doff = xoff = 0
        for g in gs:
            assert (grp["noff"][g], grp["doff"][g], P["woff"][g]) == (noff, doff, xoff)
            mine = runs[(runs["grp"] == g)]
            np.testing.assert_array_equal(mine["soff"], xoff + npad[g] ** 2 + np.arange(len(mine)) * npad[g] * P["xpitch"])
            noff, doff, xoff = noff + nvec[g] ** 2, doff + (nvec[g] + 2) * nvec[g], xoff + extra[g]
        n_max, d_max, x_max = max(n_max, noff), max(d_max, doff), max(x_max, xoff)
        assert set(runs["grp"][ch["r0"] : ch["r1"]]) == set(gs) and set(rows["grp"][ch["q0"] : ch["q1"]]) == set(gs)
        assert ch["lds"] == min(int((nvec[gs].max() + 2) * (nvec[gs].max() | 1)), 16384) * 8
    assert (P["n_max"], P["d_max"], P["x_max"]) == (n_max, d_max, x_max)
    for r in rows:
        assert r["soff"] == runs["soff"][(runs["b0"] <= r["b"]) & (r["b"] < runs["b1"])][0]
    if bound == 1:
        assert len(chunks) == len(grp) and np.all(chunks["g1"] - chunks["g0"] == 1)  # one group per chunk
    if bound == 0:
        assert len(chunks) == 1
    # the bins: the sorted row list of every bin, one after the other
    np.testing.assert_array_equal(P["bin_ent"], np.concatenate([np.flatnonzero(bins == n) for n in range(4)]))
    ptr = P["bin_ptr"].reshape(4, 2)
    counts = np.bincount(bins[bins >= 0], minlength=4)
    np.testing.assert_array_equal(ptr[:, 1] - ptr[:, 0], counts)
    np.testing.assert_array_equal(ptr[:, 0], np.concatenate([[0], np.cumsum(counts)[:-1]]))


def test_the_planner_refuses_what_the_call_refuses():
    prob = pc.groups()
    op = np.zeros((prob.nfreqs, 8), np.float32)
    bins = np.zeros(prob.nbls, np.int32)
    bins[5] = 3

    def rc(**kw):
        f = dict(ndelays=8, calibrated=0, nbins=0, bin_of_bl=None, op_r=op.ctypes.data, op_i=op.ctypes.data, ridge=0.0)
        f.update(kw)
        desc = _lib.DelayTransferDesc(*f.values())
        return raw_call(prob, np.float32, "shared", _lib.ReportPlanDesc(transfer=C.pointer(desc)), 40)[0]

    assert rc() == 0
    assert rc(nbins=3, bin_of_bl=bins.ctypes.data) == _lib.CAL_ERR_INVALID and "bin_of_bl[5] = 3" in _lib.load().cal_last_error().decode()
    assert rc(nbins=2) == _lib.CAL_ERR_INVALID and rc(op_r=None) == _lib.CAL_ERR_INVALID and rc(ndelays=0) == _lib.CAL_ERR_INVALID
    assert raw_call(prob, np.float32, "shared", _lib.ReportPlanDesc(), 40)[0] == _lib.CAL_ERR_INVALID  # no description
    assert raw_call(prob, np.float32, "shared", _lib.ReportPlanDesc(), 49)[0] == _lib.CAL_ERR_INVALID


# sha256 of what cal_debug_report_plan returned for the selectors it had before the transfer's, recorded from the library before this call
# existed: (dtype, selector) -> digest.  Problem, operator and descriptions: existing_selector_bytes below.
EXISTING = {
    ("float32", 0): "d8a1311d656407d36329fe1f4dba24ce00095550c5911c6ebcf29d05a5ef5ed9",
    ("float32", 1): "c7f07b44b08cff915e94deac094090271bd6704e9b41e957a54979ed4e45978a",
    ("float32", 2): "ea40e48abf21cc279233c24f5a35fb91d91dac4524cf342be2df58e9d427f48e",
    ("float32", 3): "756f2eae9c1b0fc5570d20da377ec3d89c9c2ea99791d42f027f98bc67717b85",
    ("float32", 4): "0281e15b9e5627e9fe44dfca31617155382aad9c834c5650570c82bc0ab5310f",
    ("float32", 10): "58ec869b52b1afa4b51dbac4aeec775a3c0e1eeee62dbee1dfb613debed4b58e",
    ("float32", 11): "b28898bd153f1378281e2cd565cbc9efe7164355705e25420227b7c509ac621c",
    ("float32", 12): "298dcc99f0a07e64a9f0128b0f7acb2b068ba97a828636f92e410273319ea1d8",
    ("float32", 13): "2d153ec6c4d34d46cbae7f81a06ecc5b57ffaf438b8024747f01c9bf5ff0c82b",
    ("float32", 14): "ddf95c4c75dd3f8a07e8d77a6eb78ba9181518b9b4505cacf811eb4089c9ed10",
    ("float32", 15): "d38dacbf5cf5e2079b702319fb27fee0cdf9fe4c8ed423e071f2142f5522492c",
    ("float32", 16): "1b03ab083d0fb41e44d480f48d5bba181c623c0594bda1aa8ea71a3b67dbf3b1",
    ("float32", 17): "86a56b06597d49c261a9800d66300763324765d3f4f1ebccd0d1d7b8a2fe4323",
    ("float32", 18): "c1ea9998a08f1fbd839fdb923984fb0b2718636b2facf7293120f7340cb8c6cd",
    ("float32", 19): "800c32b0fe73226215181e416343d8802a787b429de4dbbbf04471a37363f4a0",
    ("float64", 0): "6a2e9c47f70293554b1884677e100dc14559d9235a71e19229eb185b0d695e06",
    ("float64", 1): "c7f07b44b08cff915e94deac094090271bd6704e9b41e957a54979ed4e45978a",
    ("float64", 2): "22cbdab8641720fb146e6677bfee1c2191e46fd6ea22ffb432b350fd612a6b16",
    ("float64", 3): "3c3a065d308b0ff32f59ef9017f171eb0129101827466eba410c1a23c25208ac",
    ("float64", 4): "0281e15b9e5627e9fe44dfca31617155382aad9c834c5650570c82bc0ab5310f",
    ("float64", 10): "58ec869b52b1afa4b51dbac4aeec775a3c0e1eeee62dbee1dfb613debed4b58e",
    ("float64", 11): "b28898bd153f1378281e2cd565cbc9efe7164355705e25420227b7c509ac621c",
    ("float64", 12): "298dcc99f0a07e64a9f0128b0f7acb2b068ba97a828636f92e410273319ea1d8",
    ("float64", 13): "2d153ec6c4d34d46cbae7f81a06ecc5b57ffaf438b8024747f01c9bf5ff0c82b",
    ("float64", 14): "ddf95c4c75dd3f8a07e8d77a6eb78ba9181518b9b4505cacf811eb4089c9ed10",
    ("float64", 15): "d38dacbf5cf5e2079b702319fb27fee0cdf9fe4c8ed423e071f2142f5522492c",
    ("float64", 16): "1b03ab083d0fb41e44d480f48d5bba181c623c0594bda1aa8ea71a3b67dbf3b1",
    ("float64", 17): "86a56b06597d49c261a9800d66300763324765d3f4f1ebccd0d1d7b8a2fe4323",
    ("float64", 18): "c1ea9998a08f1fbd839fdb923984fb0b2718636b2facf7293120f7340cb8c6cd",
    ("float64", 19): "800c32b0fe73226215181e416343d8802a787b429de4dbbbf04471a37363f4a0",
}


def existing_selector_bytes(dtype):
    """{selector: bytes} of the spectrum's (0 .. 4) and the degeneracy fix's (10 .. 19) plans of a fixed case."""
    prob = pc.groups()
    rng = np.random.default_rng(11)
    op_r, op_i = (np.ascontiguousarray(rng.standard_normal((prob.nfreqs, 37)), dtype) for _ in range(2))
    norm_f = rng.uniform(size=prob.nfreqs)
    bins = (np.arange(prob.nbls) % 5 - 1).astype(np.int32)
    sd = _lib.DelaySpectrumDesc(37, 5, 0, 4, bins.ctypes.data, op_r.ctypes.data, op_i.ctypes.data, norm_f.ctypes.data)
    antpos = np.ascontiguousarray(rng.standard_normal((prob.nants, 2)))
    freqs = 150e6 + 400e3 * np.arange(prob.nfreqs)
    dd = _lib.DegeneracyDesc(_lib.DEGENERACY_MODES["band"], 1, None, None, None, antpos.ctypes.data, freqs.ctypes.data, None, None, None, None)
    report = _lib.ReportPlanDesc(spectrum=C.pointer(sd), degeneracy=C.pointer(dd), scratch_bytes=100_000, with_power_bl=1, nslices=0)
    out = {}
    for what in list(range(5)) + list(range(10, 20)):
        rc, got = raw_call(prob, dtype, "shared", report, what)
        assert rc == 0, what
        out[what] = got.tobytes()
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_existing_selectors_return_the_bytes_they_returned(dtype):
    got = existing_selector_bytes(dtype)
    for what, data in got.items():
        assert len(data) > 0 and hashlib.sha256(data).hexdigest() == EXISTING[(np.dtype(dtype).name, what)], what


# ---- the surface ------------------------------------------------------------------------------------------------------------------------
CALLS = ["calibrate_and_model_tensor", "calibrate_and_model_mixed", "calibrate_and_model_dpss", "read_calibrate_and_model_dpss"]


@pytest.mark.parametrize("name", CALLS)
def test_the_keywords_sit_directly_in_front_of_the_spectrum_keywords(name):
    params = inspect.signature(getattr(calibration, name)).parameters
    names = list(params)
    i = names.index("delay_spectrum")
    assert names[i - 2 : i] == ["delay_transfer", "delay_transfer_ridge"]
    assert params["delay_transfer"].default is False and params["delay_transfer_ridge"].default == 1e-6
    assert not any(k.startswith("delay_spectrum") for k in names[:i])
    # Python keywords only: no fit-loop control, no command-line flag
    from calamity_amd.fit_loop import FitControls

    assert len(FitControls().keywords()) == 27 and not any("delay_transfer" in f for f in FitControls().keywords())
    actions = calibration.dpss_fit_argparser()._actions
    assert len(actions) == 70 and not any("delay_transfer" in a.dest for a in actions)


@pytest.mark.parametrize("bad", [dict(delay_transfer=True), dict(delay_transfer=True, delay_spectrum=True, freeze_model=True),
                                 dict(delay_transfer=True, delay_spectrum=True, delay_transfer_ridge=-1.0),
                                 dict(delay_transfer=True, delay_spectrum=True, delay_transfer_ridge=np.inf), dict(delay_transfer="yes", delay_spectrum=True)])
def test_bad_keywords_are_refused_before_anything_is_touched(bad):
    with pytest.raises(ValueError, match="delay_transfer"):
        calibration.calibrate_and_model_tensor(None, {}, **bad)  # (no data, no device: the check comes first)
    with pytest.raises(ValueError, match="delay_transfer"):
        calibration.calibrate_and_model_dpss(None, **bad)
    with pytest.raises(ValueError, match="delay_transfer"):
        calibration.calibrate_and_model_mixed(None, **bad)
    with pytest.raises(ValueError, match="delay_transfer"):
        calibration.read_calibrate_and_model_dpss(None, **bad)


def test_the_methods_and_the_binding():
    for cls in (solver.HipFitSolver, batched.SliceBatchFitter):
        params = inspect.signature(cls.delay_transfer).parameters
        assert list(params)[1:] == ["op", "ridge", "calibrated", "bin_of_bl", "nbins", "per_baseline", "g_r", "g_i"]
        assert params["ridge"].default == 1e-6 and params["calibrated"].default is False and params["nbins"].default == 0
        assert params["per_baseline"].default is False and params["bin_of_bl"].default is None
        assert hasattr(cls, "_set_delay_transfer_scratch")
    assert [f[0] for f in _lib.DelayTransferDesc._fields_] == ["ndelays", "calibrated", "nbins", "bin_of_bl", "op_r", "op_i", "ridge"]
    assert [f[1] for f in _lib.DelayTransferDesc._fields_] == [C.c_int32] * 3 + [C.c_void_p] * 3 + [C.c_double] and C.sizeof(_lib.DelayTransferDesc) == 48
    assert [f[0] for f in _lib.ReportPlanDesc._fields_] == ["spectrum", "degeneracy", "scratch_bytes", "with_power_bl", "nslices", "transfer"]
    lib = _lib.load()
    assert hasattr(lib, "cal_solver_delay_transfer") and hasattr(lib, "cal_solver_set_delay_transfer_scratch")
    spec = distributed.exchange_spec(7, 64, delay_transfer=(5, 37))
    assert spec["delay_transfer_f64"] == 5 * 37 + 5
    assert "delay_transfer_f64" not in distributed.exchange_spec(7, 64)  # every existing key keeps its value, and no new one appears
    assert {k: v for k, v in spec.items() if k != "delay_transfer_f64"} == distributed.exchange_spec(7, 64)
    both = distributed.exchange_spec(7, 64, reg_sum=True, delay_spectrum=(3, 5, 37), delay_transfer=(5, 37))
    assert {k: v for k, v in both.items() if k != "delay_transfer_f64"} == distributed.exchange_spec(7, 64, reg_sum=True, delay_spectrum=(3, 5, 37))


def test_the_header_documents_the_call():
    text = open(os.path.join(ROOT, "include", "calamity_hip.h")).read()
    for word in ("cal_solver_delay_transfer(", "cal_solver_set_delay_transfer_scratch(", "typedef struct cal_delay_transfer_desc", "absorbed_bl[b][k]",
                 "noise_bl[b][k]", "absorbed_bin[n][k]", "count_bin[n]", "num[b][k]", "ONE all-reduce of nbins ndelays + nbins", "in ascending b",
                 "bit-identical to one without it", "two calls give the same bits", "CAL_ERR_STATE", "CAL_ERR_INVALID", "|G|^2 == 0", "lower bound",
                 "const struct cal_delay_transfer_desc* transfer", "what = 40 .. 48"):
        assert word in text, word
    fields = text.split("typedef struct cal_delay_transfer_desc {")[1].split("}")[0]
    import re

    assert re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", fields)) == [f[0] for f in _lib.DelayTransferDesc._fields_]


def test_the_build_guard_refuses_a_spilling_transfer_kernel():
    script = os.path.join(ROOT, "calamity_amd", "csrc", "check_resources.py")

    def remarks(name, scratch, vspill, occ=2):
        return (f"./x.hpp:1:1: remark: Function Name: {name} [-Rpass-analysis=kernel-resource-usage]\n"
                f"./x.hpp:1:1: remark:     VGPRs: 250 [-Rpass-analysis=kernel-resource-usage]\n"
                f"./x.hpp:1:1: remark:     ScratchSize [bytes/lane]: {scratch} [-Rpass-analysis=kernel-resource-usage]\n"
                f"./x.hpp:1:1: remark:     Occupancy [waves/SIMD]: {occ} [-Rpass-analysis=kernel-resource-usage]\n"
                f"./x.hpp:1:1: remark:     SGPRs Spill: 0 [-Rpass-analysis=kernel-resource-usage]\n"
                f"./x.hpp:1:1: remark:     VGPRs Spill: {vspill} [-Rpass-analysis=kernel-resource-usage]\n")

    def run(text):
        return subprocess.run([sys.executable, script], input=text, capture_output=True, text=True)

    dense = remarks("_ZN4calk18fused_dense_kernelILb1EEEvNS_8MfmaArgsE", 0, 0)
    names = {k: f"_ZN4calk{len(k)}{k}I{t}EEvPKT_" for k in ("dtransfer_basis_kernel", "dtransfer_power_kernel") for t in "fd"}
    names = {f"{k}<{t}>": f"_ZN4calk{len(k)}{k}I{t}EEvPKT_" for k in ("dtransfer_basis_kernel", "dtransfer_power_kernel") for t in "fd"}
    assert run(dense + "".join(remarks(n, 0, 0) for n in names.values())).returncode == 0
    for k, n in names.items():
        for scratch, vspill in ((16, 0), (0, 4)):
            bad = run(dense + remarks(n, scratch, vspill))
            assert bad.returncode != 0 and k.split("<")[0] in bad.stdout + bad.stderr, (k, scratch, vspill)
    for t in "fd":
        low = run(dense + remarks(names[f"dtransfer_power_kernel<{t}>"], 0, 0, occ=1))
        assert low.returncode != 0 and "occupancy" in low.stdout + low.stderr
        assert run(dense + remarks(names[f"dtransfer_basis_kernel<{t}>"], 0, 0, occ=1)).returncode == 0  # no occupancy rule for the basis kernel
    # the leverage kernel, whose loop the basis kernel copies, stays in its own no-scratch, no-spill group
    lev = "_ZN4calk25fit_error_leverage_kernelIfEEvPKT_"
    assert run(dense + remarks(lev, 0, 4)).returncode != 0 and run(dense + remarks(lev, 0, 0)).returncode == 0
