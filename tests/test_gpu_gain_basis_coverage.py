"""The gain-basis kernels where tests/test_gpu_gain_basis.py and tests/test_gpu_gain_time_basis.py do not go: every optimizer on the
basis coefficients ``y`` (enqueue_update_y: both launch forms, the accumulator fill of Adagrad / Ftrl on either order of the setters),
and shapes past the first tile of gain_project_kernel (``kpad / V > 256``), the first LDS batch and the first channel block of
gain_expand_kernel (``kpad > 256``, ``fpad > 256 V``) and the first block in x of the two time kernels (V = 16 / sizeof(T)).

Yardstick: the fp64 NumPy restatements ``gamma_fit`` (tests/test_gain_basis_host.py) and ``gamma2_fit``
(tests/test_gain_time_basis_host.py), which CPU tests pin to the oracle and which take any ``oracle.ref_numpy.OPTIMIZERS`` entry, run
on the bases rounded to the device dtype; ``oracle.ref_numpy.loss_and_grads`` for the projected gradient.  Tolerances are the
project's (tests/test_gpu_parity.py: TOL; 1e-12 for the fp64 span checks); two device runs that must be the same numbers are compared
bit for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from calamity_amd import modeling, problem  # noqa: E402
from oracle import ref_numpy as R  # noqa: E402
from test_gain_basis_host import gamma_fit, small_case  # noqa: E402
from test_gain_time_basis_host import gamma2_fit, joint_case  # noqa: E402
from test_gpu_gain_time_basis import expand, outside_span, time_basis  # noqa: E402
from test_gpu_launch_modes import OPT_CASES  # noqa: E402
from test_gpu_parity import TOL, make_solver, oracle_inputs, relnorm  # noqa: E402,F401

pytestmark = pytest.mark.gpu

OPTS = [(n, k) for n, k in OPT_CASES if n != "LAMB"]  # (LAMB is refused while a basis is set: tests/test_gpu_gain_basis.py)
assert len(OPTS) == 11


def opt_id(entry):
    return f"{entry[0]}-{'-'.join(sorted(entry[1]))}"


ACC_OPTS = [e for e in OPTS if e[0] in ("Adagrad", "Ftrl")]  # default initial_accumulator_value 0.1, and 0.0 / 0.2
assert [e[1].get("initial_accumulator_value", 0.1) for e in ACC_OPTS] == [0.1, 0.0, 0.1, 0.2]
# SGD + Nesterov, Adagrad (default accumulator), Adadelta, Nadam, RMSprop with momentum, the first Ftrl entry
TIME_OPTS = [OPTS[2], OPTS[5], OPTS[7], OPTS[8], OPTS[4], OPTS[9]]
assert [e[0] for e in TIME_OPTS] == ["SGD", "Adagrad", "Adadelta", "Nadam", "RMSprop", "Ftrl"] and TIME_OPTS[0][1]["nesterov"] and TIME_OPTS[4][1]["momentum"]


def cplx(a_r, a_i):
    return np.asarray(a_r, dtype=np.float64) + 1j * np.asarray(a_i, dtype=np.float64)


def rounded(B, dtype):
    """The basis the device holds, as float64."""
    return np.asarray(B).astype(dtype).astype(np.float64)


def freq_basis_100ns(nfreqs):
    return np.array(modeling.gain_dpss_basis(150e6 + 400e3 * np.arange(nfreqs), 100.0))


def gpu_fit(p, start, dtype, Bf, Bt, optimizer, kw, reg, nsteps, launch, optimizer_first=False):
    """1 unrecorded + ``nsteps`` recorded steps (tol = 0) of the STREAM layout's general kernels.  ``optimizer_first``: set_optimizer before
    the bases (reshape_gain_coeffs then re-applies it) instead of after them."""
    s = make_solver(p, start, dtype, "stream", reg, kernel_path="auto")
    s.set_launch_mode(launch)
    if optimizer_first:
        s.set_optimizer(optimizer, **kw)
    if Bf is not None:
        s.set_gain_basis(Bf)
    if Bt is not None:
        s.set_gain_time_basis(Bt)
    if not optimizer_first:
        s.set_optimizer(optimizer, **kw)
    s.run(1, record=False)
    losses, stopped, nupd = s.run(nsteps, record=True, tol=0.0)
    assert len(losses) == nsteps == nupd and not stopped
    g_r, g_i, c_r, c_i = s.get_params()
    y_r, y_i = s.get_gain_coeffs()
    s.close()
    return dict(loss=losses, g=cplx(g_r, g_i), c_r=c_r, c_i=c_i, y=cplx(y_r, y_i), y_r=y_r)


def check_trajectory(out, ref, p, tol, what):
    """Losses, y, gains and both coefficient planes against a restatement's result, all at ``tol``; the figures are printed first."""
    ref_g, ref_y = cplx(ref["g_r"], ref["g_i"]), cplx(ref["y_r"], ref["y_i"])
    ref_c_r, ref_c_i = problem.coeffs_from_chunks(p, ref["fg_r"]), problem.coeffs_from_chunks(p, ref["fg_i"])
    assert np.all(np.isfinite(ref["loss"])) and len(out["loss"]) == len(ref["loss"])
    assert out["y"].shape == ref_y.shape
    print(f"{what}: loss {np.max(np.abs(out['loss'] - ref['loss']) / np.abs(ref['loss'])):.2e}  g {relnorm(out['g'], ref_g):.2e}  y {relnorm(out['y'], ref_y):.2e}  "
          f"c {relnorm(out['c_r'], ref_c_r):.2e} {relnorm(out['c_i'], ref_c_i):.2e}  |y| {np.linalg.norm(ref_y):.2e}")
    np.testing.assert_allclose(out["loss"], ref["loss"], rtol=tol)
    assert relnorm(out["y"], ref_y) <= tol
    assert relnorm(out["g"], ref_g) <= tol
    assert relnorm(out["c_r"], ref_c_r) <= tol and relnorm(out["c_i"], ref_c_i) <= tol
    assert np.linalg.norm(out["y"]) > 0


def check_span(out, start, dtype, Bt, Bf, na, tol):
    """The gains the solver returns are ``g0 + Bt (x) Bf y`` of the coefficients it returns; in fp64 nothing of ``g - g0`` lies outside the
    span.  ``Bt = None``: one time."""
    g0 = cplx(np.asarray(start["g_r"], dtype=dtype), np.asarray(start["g_i"], dtype=dtype))
    if Bt is None:
        y3, bt = out["y"][:, None, :], np.ones((1, 1))
    else:
        y3, bt = out["y"], Bt
    assert relnorm(out["g"], g0 + expand(bt, y3, Bf)) <= tol
    if dtype == np.float64:
        outside = outside_span(bt, Bf, out["g"] - g0, na)
        print(f"outside the span: {outside / np.linalg.norm(out['g']):.2e}")
        assert outside <= 1e-12 * np.linalg.norm(out["g"])
    return g0


def assert_same_bits(a, b):
    for k in ("loss", "g", "y", "c_r", "c_i"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


# ---- A. every optimizer on y --------------------------------------------------------------------------------------------------
_opt_case = {}


def opt_case(reg):
    if reg not in _opt_case:
        p, start, ch, fg_r, fg_i = small_case(nants=9, nfreqs=40, seed=5, with_sky=reg)
        rng = np.random.default_rng(3)
        start["g_r"] = 1.0 + 0.05 * rng.standard_normal((p.nants, p.nfreqs))
        start["g_i"] = 0.05 * rng.standard_normal((p.nants, p.nfreqs))
        B = freq_basis_100ns(40)
        assert B.shape == (40, 9)
        _opt_case[reg] = (p, start, ch, fg_r, fg_i, B)
    return _opt_case[reg]


# reg selects the launch form of the update (enqueue_update_y): without the regulariser the one-launch tail (step_update_kernel), with
# "sum" on this single-slice general-kernel solver (Rk) finalize_kernel + adam2_kernel -- both with y_row() as the row length
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("reg", [False, True])
@pytest.mark.parametrize("entry", OPTS, ids=opt_id)
def test_every_optimizer_on_the_frequency_coefficients(entry, reg, dtype):
    optimizer, kw = entry
    p, start, ch, fg_r, fg_i, B = opt_case(reg)
    B = rounded(B, dtype)
    ref = gamma_fit(B, start["g_r"], start["g_i"], fg_r, fg_i, ch, 25, optimizer, tol=0.0, reg=reg, **kw)
    out = gpu_fit(p, start, dtype, B, None, optimizer, kw, reg, 25, "kernels")
    tol = TOL[dtype]["traj"]
    assert out["y_r"].shape == (p.nants, B.shape[1]) and out["y_r"].dtype == np.dtype(dtype)
    check_trajectory(out, ref, p, tol, f"A.1 {np.dtype(dtype).name}")
    check_span(out, start, dtype, None, B, p.nants, tol)
    assert_same_bits(gpu_fit(p, start, dtype, B, None, optimizer, kw, reg, 25, "graph"), out)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("reg", [False, True])
@pytest.mark.parametrize("entry", ACC_OPTS, ids=opt_id)
def test_accumulator_fill_on_either_order_of_the_setters(entry, reg, dtype):
    """Adagrad's and Ftrl's accumulators of y start at initial_accumulator_value whether set_optimizer fills them (the basis set first:
    the order of the test above, which the restatement pins) or set_gain_basis re-applies the optimizer (the optimizer set first)."""
    optimizer, kw = entry
    p, start, _, _, _, B = opt_case(reg)
    basis_first = gpu_fit(p, start, dtype, B, None, optimizer, kw, reg, 25, "kernels")
    optimizer_first = gpu_fit(p, start, dtype, B, None, optimizer, kw, reg, 25, "kernels", optimizer_first=True)
    assert np.linalg.norm(basis_first["y"]) > 0
    assert_same_bits(optimizer_first, basis_first)


_time_case = {}


def time_case():
    if not _time_case:
        big, start, ch, fg_r, fg_i = joint_case(ntimes=3, nants=7, nfreqs=40, with_sky=True)
        _time_case["c"] = (big, start, ch, fg_r, fg_i, time_basis(3), freq_basis_100ns(40))
    return _time_case["c"]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("entry", TIME_OPTS, ids=opt_id)
def test_optimizers_on_the_time_and_frequency_coefficients(entry, dtype):
    optimizer, kw = entry
    big, start, ch, fg_r, fg_i, Bt, Bf = time_case()
    Bt, Bf = rounded(Bt, dtype), rounded(Bf, dtype)
    ref = gamma2_fit(Bt, Bf, start["g_r"], start["g_i"], fg_r, fg_i, ch, 25, optimizer, tol=0.0, reg=True, **kw)
    out = gpu_fit(big, start, dtype, Bf, Bt, optimizer, kw, True, 25, "kernels")
    tol = TOL[dtype]["traj"]
    assert out["y_r"].shape == (7, Bt.shape[1], Bf.shape[1])
    check_trajectory(out, ref, big, tol, f"A.3 {np.dtype(dtype).name}")
    check_span(out, start, dtype, Bt, Bf, 7, tol)
    assert_same_bits(gpu_fit(big, start, dtype, Bf, Bt, optimizer, kw, True, 25, "graph"), out)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("entry", [OPTS[5], OPTS[9]], ids=opt_id)
def test_accumulator_optimizers_on_time_coefficients_of_padded_rows(entry, dtype):
    """No frequency basis: W = fpad = 64 for 40 channels, so the accumulator fill covers 24 padded channels of every row of y."""
    optimizer, kw = entry
    assert optimizer in ("Adagrad", "Ftrl") and "initial_accumulator_value" not in kw
    big, start, ch, fg_r, fg_i, Bt, _ = time_case()
    Bt = rounded(Bt, dtype)
    ref = gamma2_fit(Bt, np.eye(big.nfreqs), start["g_r"], start["g_i"], fg_r, fg_i, ch, 25, optimizer, tol=0.0, reg=True, **kw)
    out = gpu_fit(big, start, dtype, None, Bt, optimizer, kw, True, 25, "kernels")
    tol = TOL[dtype]["traj"]
    assert out["y_r"].shape == (7, Bt.shape[1], big.nfreqs)
    check_trajectory(out, ref, big, tol, f"A.3 no frequency basis {np.dtype(dtype).name}")
    check_span(out, start, dtype, Bt, None, 7, tol)
    assert_same_bits(gpu_fit(big, start, dtype, None, Bt, optimizer, kw, True, 25, "graph"), out)


# ---- B. shapes past the first tile --------------------------------------------------------------------------------------------
# 1064 channels: fpad = 1152, two channel blocks of gain_expand_kernel in fp32 (256 * 4 channels each) and three in fp64, the last one
# partly filled.  K (kpad):  1 (8): nq = 2 / 4 vector groups, 128 / 64 segments;  260 (264): a second LDS batch of 8 coefficients in the
# expansion;  512 (512): fp64 nq = 256, one segment, exactly one full tile of the projection;  1030 (1032): two projection tiles in fp32
# (256 + 2 groups), three in fp64 (256 + 256 + 4), five LDS batches in the expansion.
WIDE_F = 1064
WIDE_K = [1, 260, 512, 1030]
_wide = {}


def wide_case():
    if not _wide:
        p, start, ch, fg_r, fg_i = small_case(nants=4, nfreqs=WIDE_F, seed=11, with_sky=True)
        assert p.nbls == 6
        rng = np.random.default_rng(12)
        start["g_r"] = 1.0 + 0.05 * rng.standard_normal((p.nants, p.nfreqs))
        start["g_i"] = 0.05 * rng.standard_normal((p.nants, p.nfreqs))
        _wide["c"] = (p, start, ch, fg_r, fg_i)
    return _wide["c"]


def random_basis(nfreqs, K, dtype):
    """Not orthogonal; rounded to the device dtype."""
    return rounded(np.random.default_rng(K).standard_normal((nfreqs, K)) / np.sqrt(nfreqs), dtype)


def blocks(n, dtype):
    """The column ranges of 256 V: what one tile of gain_project_kernel or one channel block of gain_expand_kernel covers."""
    per = 256 * (16 // np.dtype(dtype).itemsize)
    return [slice(c, min(c + per, n)) for c in range(0, n, per)]


_wide_grads = {}


def wide_grads(reg):
    """(loss, gg_r, gg_i) of the oracle at the start of the wide case: computed once per reg, never changed."""
    if reg not in _wide_grads:
        p, start, ch, fg_r, fg_i = wide_case()
        a0, a1 = R.ant_inds_from_corr_inds(ch["corr_inds"])
        priors = R.prior_sums(ch["sky_model_r"], ch["sky_model_i"], ch["wgts"]) if reg else (None, None)
        loss, gg_r, gg_i, _, _ = R.loss_and_grads(start["g_r"], start["g_i"], fg_r, fg_i, ch["fg_comps"], ch["data_r"], ch["data_i"], ch["wgts"],
                                                  a0, a1, *priors)
        for a in (gg_r, gg_i):
            a.setflags(write=False)
        _wide_grads[reg] = (loss, gg_r, gg_i)
    return _wide_grads[reg]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("reg", [False, True])
@pytest.mark.parametrize("K", WIDE_K)
def test_projected_gradient_past_the_first_tile(K, reg, dtype):
    p, start, _, _, _ = wide_case()
    loss, gg_r, gg_i = wide_grads(reg)
    B = random_basis(WIDE_F, K, dtype)
    s = make_solver(p, start, dtype, "stream", reg)
    s.set_gain_basis(B)
    l2, gy_r, gy_i = s.eval_gain_coeff_grads()
    s.close()
    tol = TOL[dtype]
    want_r, want_i = gg_r @ B, gg_i @ B
    assert gy_r.shape == gy_i.shape == (p.nants, K)
    tiles = blocks(K, dtype)
    per_tile = [max(relnorm(gy_r[:, c], want_r[:, c]), relnorm(gy_i[:, c], want_i[:, c])) for c in tiles]
    print(f"B.1 {np.dtype(dtype).name}: loss rel {abs(l2 - loss) / abs(loss):.2e}  grad y rel {relnorm(gy_r, want_r):.2e} {relnorm(gy_i, want_i):.2e}  "
          f"per tile {' '.join(f'{e:.2e}' for e in per_tile)}")
    assert abs(l2 - loss) <= tol["loss"] * abs(loss)
    assert relnorm(gy_r, want_r) <= tol["grad"] and relnorm(gy_i, want_i) <= tol["grad"]
    # every tile of 256 V vectors on its own: a wrong last tile of two vector groups cannot hide in the norm of the whole
    assert len(tiles) == {1: 1, 260: 1, 512: 1, 1030: 2 if dtype == np.float32 else 3}[K]
    assert max(per_tile) <= tol["grad"], per_tile
    for gy in (gy_r, gy_i):
        assert np.all(np.linalg.norm(gy, axis=1) > 0)
        if K >= 260:  # every vector got its own sum: no vector's column and no antenna's row repeats another
            assert len(np.unique(gy, axis=0)) == p.nants and len(np.unique(gy.T, axis=0)) == K


_wide_refs = {}


def wide_ref(K, dtype):
    key = (K, np.dtype(dtype).name)
    if key not in _wide_refs:
        p, start, ch, fg_r, fg_i = wide_case()
        _wide_refs[key] = gamma_fit(random_basis(WIDE_F, K, dtype), start["g_r"], start["g_i"], fg_r, fg_i, ch, 12, "Adam", tol=0.0, reg=True,
                                    learning_rate=1e-2)
    return _wide_refs[key]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("K", WIDE_K)
def test_trajectory_past_the_first_tile(K, dtype):
    p, start, _, _, _ = wide_case()
    B = random_basis(WIDE_F, K, dtype)
    ref = wide_ref(K, dtype)
    out = gpu_fit(p, start, dtype, B, None, "Adam", dict(learning_rate=1e-2), True, 12, "kernels")
    tol = TOL[dtype]["traj"]
    check_trajectory(out, ref, p, tol, f"B.2 {np.dtype(dtype).name}")
    g0 = check_span(out, start, dtype, None, B, p.nants, tol)
    # the correction of every channel block of 256 V on its own: a block gain_expand_kernel never wrote is g0 there and fails alone
    moved = cplx(ref["y_r"], ref["y_i"]) @ B.T
    chans = blocks(WIDE_F, dtype)
    assert len(chans) == (2 if dtype == np.float32 else 3)
    per_block = [relnorm((out["g"] - g0)[:, c], moved[:, c]) for c in chans]
    print(f"B.2 {np.dtype(dtype).name}: g - g0 per channel block {' '.join(f'{e:.2e}' for e in per_block)}")
    assert max(per_block) <= tol, per_block
    assert_same_bits(gpu_fit(p, start, dtype, B, None, "Adam", dict(learning_rate=1e-2), True, 12, "graph"), out)


# T = L = 9: one full tile of kTimeTile = 8 plus one row in both time kernels.  K = 150: kpad = 152, a row of y is 304 reals, and the
# 7 antennas' rows are 532 threads in fp32 (3 blocks in x) and 1064 in fp64 (5 blocks), the last block partly filled.
TIMES_T, TIMES_NA, TIMES_F, TIMES_K = 9, 7, 200, 150
_times = {}


def times_case():
    if not _times:
        big, start, ch, fg_r, fg_i = joint_case(ntimes=TIMES_T, nants=TIMES_NA, nfreqs=TIMES_F, with_sky=True, seed=80)
        Bt = np.random.default_rng(9).standard_normal((TIMES_T, TIMES_T)) / 3.0
        Bf = np.random.default_rng(TIMES_K).standard_normal((TIMES_F, TIMES_K)) / np.sqrt(TIMES_F)
        _times["c"] = (big, start, ch, fg_r, fg_i, Bt, Bf)
    return _times["c"]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("reg", [False, True])
def test_time_projected_gradient_over_several_blocks(reg, dtype):
    big, start, ch, fg_r, fg_i, Bt, Bf = times_case()
    T, na, K = TIMES_T, TIMES_NA, TIMES_K
    a0, a1 = R.ant_inds_from_corr_inds(ch["corr_inds"])
    priors = R.prior_sums(ch["sky_model_r"], ch["sky_model_i"], ch["wgts"]) if reg else (None, None)
    loss, gg_r, gg_i, _, _ = R.loss_and_grads(start["g_r"], start["g_i"], fg_r, fg_i, ch["fg_comps"], ch["data_r"], ch["data_i"], ch["wgts"],
                                              a0, a1, *priors)
    Bt, Bf = rounded(Bt, dtype), rounded(Bf, dtype)
    s = make_solver(big, start, dtype, "stream", reg)
    s.set_gain_basis(Bf)
    s.set_gain_time_basis(Bt)
    l2, gy_r, gy_i = s.eval_gain_coeff_grads()
    s.close()
    contract = lambda gg: np.einsum("tl,taf,fk->alk", Bt, gg.reshape(T, na, TIMES_F), Bf)  # noqa: E731
    want_r, want_i = contract(gg_r), contract(gg_i)
    tol = TOL[dtype]
    assert gy_r.shape == gy_i.shape == (na, T, K)
    # the blocks in x run through the antennas' rows: every antenna on its own, and every vector l of the second tile
    per_ant = [max(relnorm(gy_r[a], want_r[a]), relnorm(gy_i[a], want_i[a])) for a in range(na)]
    per_vec = [max(relnorm(gy_r[:, l], want_r[:, l]), relnorm(gy_i[:, l], want_i[:, l])) for l in range(T)]
    print(f"B.3 {np.dtype(dtype).name}: loss rel {abs(l2 - loss) / abs(loss):.2e}  grad y rel {relnorm(gy_r, want_r):.2e} {relnorm(gy_i, want_i):.2e}  "
          f"per antenna {max(per_ant):.2e}  per time vector {max(per_vec):.2e}")
    assert abs(l2 - loss) <= tol["loss"] * abs(loss)
    assert relnorm(gy_r, want_r) <= tol["grad"] and relnorm(gy_i, want_i) <= tol["grad"]
    assert max(per_ant) <= tol["grad"] and max(per_vec) <= tol["grad"], (per_ant, per_vec)
    for gy in (gy_r, gy_i):
        flat = gy.reshape(na * T, K)
        assert np.all(np.linalg.norm(flat, axis=1) > 0) and len(np.unique(flat, axis=0)) == na * T


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_time_trajectory_over_several_blocks(dtype):
    big, start, ch, fg_r, fg_i, Bt, Bf = times_case()
    T, na = TIMES_T, TIMES_NA
    Bt, Bf = rounded(Bt, dtype), rounded(Bf, dtype)
    ref = gamma2_fit(Bt, Bf, start["g_r"], start["g_i"], fg_r, fg_i, ch, 12, "Adam", tol=0.0, reg=True, learning_rate=1e-2)
    out = gpu_fit(big, start, dtype, Bf, Bt, "Adam", dict(learning_rate=1e-2), True, 12, "kernels")
    tol = TOL[dtype]["traj"]
    assert out["y_r"].shape == (na, T, TIMES_K)
    check_trajectory(out, ref, big, tol, f"B.3 {np.dtype(dtype).name}")
    g0 = check_span(out, start, dtype, Bt, Bf, na, tol)
    # the correction of every time's and every antenna's rows on its own: rows a block never wrote are g0 and fail alone
    moved = expand(Bt, cplx(ref["y_r"], ref["y_i"]), Bf).reshape(T, na, TIMES_F)
    got = (out["g"] - g0).reshape(T, na, TIMES_F)
    per_time = [relnorm(got[t], moved[t]) for t in range(T)]
    per_ant = [relnorm(got[:, a], moved[:, a]) for a in range(na)]
    print(f"B.3 {np.dtype(dtype).name}: g - g0 per time {max(per_time):.2e}  per antenna {max(per_ant):.2e}")
    assert max(per_time) <= tol and max(per_ant) <= tol, (per_time, per_ant)
    assert_same_bits(gpu_fit(big, start, dtype, Bf, Bt, "Adam", dict(learning_rate=1e-2), True, 12, "graph"), out)
