"""Gains fitted in a smooth frequency basis, host side: the DPSS gain basis, the command-line argument, and the NumPy
restatement of the basis fit that the GPU tests (tests/test_gpu_gain_basis.py) are measured against.

Parameterisation: ``g = g0 + B y`` with ``B`` real ``[F, K]`` shared by every antenna, ``g0`` the gains the fit starts from and
``y`` (complex, zero at the start) the optimizer's variables in place of the per-channel gains; chain rule ``grad y = grad g @ B``.
``gamma_fit`` below is that, built from the oracle's public pieces (``oracle.ref_numpy.loss_and_grads`` and its optimizer
classes) with the oracle's loop semantics (one unrecorded step, recorded loss k before update k, use_min, tolerance stop,
freeze_model).  With ``B = I`` it must BE the oracle's per-channel fit: that is the anchor that keeps the yardstick honest."""
import sys

import numpy as np
import pytest

from calamity_amd import calibration, modeling, problem, synthetic
from oracle import ref_numpy as R


def gamma_fit(B, g0_r, g0_i, fg_r, fg_i, ch, maxsteps, optimizer, tol=1e-14, use_min=False, freeze_model=False, reg=False, **opt_kwargs):
    """The basis fit in NumPy (float64).  Returns dict(loss, g_r, g_i, y_r, y_i, fg_r, fg_i): the parameters after the last
    update or, with ``use_min``, those held right after the update of the lowest-loss step."""
    a0, a1 = R.ant_inds_from_corr_inds(ch["corr_inds"])
    B = np.asarray(B, dtype=np.float64)
    g0_r, g0_i = np.array(g0_r, dtype=np.float64), np.array(g0_i, dtype=np.float64)
    y_r = np.zeros((g0_r.shape[0], B.shape[1]))
    y_i = np.zeros_like(y_r)
    fg_r = [np.array(a, dtype=np.float64) for a in fg_r]
    fg_i = [np.array(a, dtype=np.float64) for a in fg_i]
    priors = R.prior_sums(ch["sky_model_r"], ch["sky_model_i"], ch["wgts"]) if reg else (None, None)
    opt = R.OPTIMIZERS[optimizer](**opt_kwargs)

    def step():
        loss, gg_r, gg_i, gf_r, gf_i = R.loss_and_grads(g0_r + y_r @ B.T, g0_i + y_i @ B.T, fg_r, fg_i, ch["fg_comps"], ch["data_r"],
                                                        ch["data_i"], ch["wgts"], a0, a1, *priors)
        grads = [(gg_r @ B, y_r), (gg_i @ B, y_i)]
        if not freeze_model:
            grads += list(zip(gf_r, fg_r)) + list(zip(gf_i, fg_i))
        opt.apply_gradients(grads)
        return loss

    def snapshot():
        return dict(y_r=y_r.copy(), y_i=y_i.copy(), fg_r=[a.copy() for a in fg_r], fg_i=[a.copy() for a in fg_i])

    step()  # the unrecorded step
    losses, min_loss, best = [], 9e99, None
    for k in range(maxsteps):
        losses.append(step())
        if use_min and losses[-1] < min_loss:
            min_loss, best = losses[-1], snapshot()
        if k >= 1 and abs(losses[-1] - losses[-2]) < tol:
            break
    out = best if use_min else snapshot()
    out.update(loss=np.asarray(losses), g_r=g0_r + out["y_r"] @ B.T, g_i=g0_i + out["y_i"] @ B.T)
    return out


def small_case(nants=9, nfreqs=40, seed=5, with_sky=False):
    p, _, start = synthetic.make_problem(nants, nfreqs, f0=150e6, df=400e3, seed=seed, with_sky=with_sky)
    ch = problem.chunks_from_problem(p)
    fg_r = problem.coeffs_to_chunks(p, start["c_r"], np.float64)
    fg_i = problem.coeffs_to_chunks(p, start["c_i"], np.float64)
    return p, start, ch, fg_r, fg_i


HERA_FREQS = np.linspace(100e6, 200e6, 1024, endpoint=False)


def test_gain_dpss_basis():
    counts = []
    for dly in (50.0, 100.0, 200.0):
        B = modeling.gain_dpss_basis(HERA_FREQS, dly)
        amat, nterms = modeling.dpss_operator(HERA_FREQS, [0.0], [dly * 1e-9], [1e-10])
        assert B.dtype == np.float64 and not np.iscomplexobj(B)
        assert B.shape == (1024, nterms[0]) == amat.shape
        assert np.abs(B.T @ B - np.eye(B.shape[1])).max() <= 1e-10
        assert np.abs(B - amat.real).max() <= 1e-12 and np.abs(amat.imag).max() == 0.0
        counts.append(B.shape[1])
    assert counts == [18, 30, 51]
    # a tighter eigenvalue cut keeps fewer vectors; the basis is cached (the same read-only array comes back)
    assert modeling.gain_dpss_basis(HERA_FREQS, 100.0, eigenval_cutoff=1e-4).shape[1] < 30
    assert modeling.gain_dpss_basis(HERA_FREQS, 100.0) is modeling.gain_dpss_basis(HERA_FREQS, 100.0)
    with pytest.raises(ValueError):
        modeling.gain_dpss_basis(HERA_FREQS, 0.0)


@pytest.mark.parametrize("optimizer", ["Adam", "Adamax"])
def test_identity_basis_restates_the_oracle(optimizer):
    """B = I: the restatement IS the per-channel fit of the oracle (float64, 1e-12; about 1e-15 measured)."""
    p, start, ch, fg_r, fg_i = small_case()
    ref = R.fit_gains_and_foregrounds(start["g_r"], start["g_i"], fg_r, fg_i, ch["data_r"], ch["data_i"], ch["wgts"], ch["fg_comps"],
                                      ch["corr_inds"], maxsteps=30, optimizer=optimizer, learning_rate=1e-2)
    out = gamma_fit(np.eye(p.nfreqs), start["g_r"], start["g_i"], fg_r, fg_i, ch, 30, optimizer, learning_rate=1e-2)
    ref_loss = np.asarray(ref[4]["loss"], dtype=np.float64)
    assert len(out["loss"]) == 30
    assert np.max(np.abs(out["loss"] - ref_loss) / ref_loss) <= 1e-12
    g, g_ref = out["g_r"] + 1j * out["g_i"], ref[0] + 1j * ref[1]
    assert np.linalg.norm(g - g_ref) <= 1e-12 * np.linalg.norm(g_ref)
    for a, b in zip(out["fg_r"] + out["fg_i"], list(ref[2]) + list(ref[3])):
        assert np.linalg.norm(a - b) <= 1e-12 * max(np.linalg.norm(b), 1e-300)


def test_argparser_and_argument_checks(monkeypatch):
    monkeypatch.setattr(sys, "argv", [sys.argv[0], "--input_data_files", "input.uvh5"])
    assert calibration.dpss_fit_argparser().parse_args().gain_max_dly is None
    monkeypatch.setattr(sys, "argv", [sys.argv[0], "--input_data_files", "input.uvh5", "--gain_max_dly", "100"])
    args = calibration.dpss_fit_argparser().parse_args()
    assert args.gain_max_dly == 100.0 and isinstance(args.gain_max_dly, float)
    import inspect

    for fn in (calibration.calibrate_and_model_tensor,):
        params = inspect.signature(fn).parameters
        assert params["gain_basis"].default is None and params["gain_max_dly"].default is None
    assert inspect.signature(calibration.fit_gains_and_foregrounds).parameters["gain_basis"].default is None
    # both given: refused before anything is touched (no device, not even a look at the data)
    with pytest.raises(ValueError, match="not both"):
        calibration.calibrate_and_model_tensor(None, {}, gain_basis=np.eye(4), gain_max_dly=100.0)
    uvd, _, _ = synthetic.make_uvdata(nants=4, nfreqs=32, ntimes=1, seed=0)
    with pytest.raises(ValueError, match="shape"):
        calibration.calibrate_and_model_tensor(uvd, {}, gain_basis=np.eye(31))
    with pytest.raises(ValueError, match="real"):
        calibration.calibrate_and_model_tensor(uvd, {}, gain_basis=np.eye(32) * 1j)
