"""Host-only checks of the degeneracy fix: the NumPy restatement (tests/degeneracy_ref.py) recovers what was injected, and the drop-in
calls refuse bad keywords before any solver exists."""
import numpy as np
import pytest

import degeneracy_ref as R


def degenerate_case(antpos, nfreqs=20, seed=0, flag_frac=0.05, band=False, autos=False, phase=True):
    """A sky model ``s``, true gains, and a fitted ``(g, m)`` that differs from them by an injected ``(eta, psi, Phi)`` exactly."""
    rng = np.random.default_rng(seed)
    na = len(antpos)
    pairs = [(i, j) for i in range(na) for j in range(i + (0 if autos else 1), na)]
    ant0, ant1 = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    nbls = len(pairs)
    d = antpos[ant0] - antpos[ant1]
    freqs = 150e6 + 1e6 * np.arange(nfreqs)
    s = rng.normal(size=(nbls, nfreqs)) + 1j * rng.normal(size=(nbls, nfreqs))
    s[ant0 == ant1] = np.abs(s[ant0 == ant1]) + 1.0
    g_true = (1 + 0.1 * rng.normal(size=(na, nfreqs))) * np.exp(1j * 0.3 * rng.normal(size=(na, nfreqs)))
    w = (rng.random((nbls, nfreqs)) >= flag_frac) * (0.5 + rng.random((nbls, nfreqs)))
    if band:
        ratio = freqs / freqs.mean()
        phi = ratio[:, None] * rng.normal(size=2)[None, :]
        eta = np.full(nfreqs, 0.2)
    else:
        phi = rng.normal(size=(nfreqs, 2))
        eta = 0.3 * rng.normal(size=nfreqs)
    if np.ptp(antpos[:, 1]) == 0:
        phi[:, 1] = 0.0  # a line sees the tilt along itself only
    phi = phi / np.abs(d @ phi.T).max()  # the largest |Phi.d| is 1 rad
    psi = rng.uniform(-1, 1, size=nfreqs) if phase else np.zeros(nfreqs)
    m = s * np.exp(-2 * eta)[None, :] * np.exp(-1j * (d @ phi.T))
    g = g_true * np.exp(eta)[None, :] * np.exp(1j * (antpos @ phi.T + psi[None, :]))
    return dict(ant0=ant0, ant1=ant1, antpos=antpos, freqs=freqs, s=s, g_true=g_true, w=w, m=m, g=g, eta=eta, psi=psi, phi=phi)


ARRAYS = {"hex": R.hex_array(7), "line": R.line_array(7)}


@pytest.mark.parametrize("array", sorted(ARRAYS))
def test_recovery(array):
    c = degenerate_case(ARRAYS[array], seed=1)
    out = R.fix_degeneracies(c["m"], c["s"], c["w"], c["g"], c["ant0"], c["ant1"], c["antpos"], iters=6, gref=c["g_true"])
    assert np.abs(out["eta"] - c["eta"]).max() < 1e-12
    assert np.abs(out["tilt"] - c["phi"]).max() * np.abs(c["antpos"]).max() < 1e-12
    assert np.abs(np.angle(np.exp(1j * (out["psi"] - c["psi"])))).max() < 1e-12
    assert np.abs(out["g"] - c["g_true"]).max() < 1e-12
    assert np.abs(out["model"] - c["s"]).max() < 1e-12 * np.abs(c["s"]).max()
    assert out["last_step"].max() < 1e-12
    assert np.array_equal(out["nsamples"], (c["w"] > 0).sum(axis=0))


def test_band_mode_recovers_one_shift_and_one_amplitude():
    c = degenerate_case(ARRAYS["hex"], seed=2, band=True)
    out = R.fix_degeneracies(c["m"], c["s"], c["w"], c["g"], c["ant0"], c["ant1"], c["antpos"], iters=6, mode="band", freqs=c["freqs"], gref=c["g_true"])
    assert np.abs(out["eta"] - 0.2).max() < 1e-12
    assert np.ptp(out["eta"]) == 0.0
    ratio = c["freqs"] / c["freqs"].mean()
    assert np.abs(out["tilt"] / ratio[:, None] - out["tilt"][0] / ratio[0]).max() < 1e-15
    assert np.abs(out["tilt"] - c["phi"]).max() * np.abs(c["antpos"]).max() < 1e-12
    assert np.abs(out["g"] - c["g_true"]).max() < 1e-12


def test_empty_channel_keeps_the_identity():
    c = degenerate_case(ARRAYS["hex"], seed=3)
    c["w"][:, 4] = 0.0
    out = R.fix_degeneracies(c["m"], c["s"], c["w"], c["g"], c["ant0"], c["ant1"], c["antpos"], gref=c["g_true"])
    assert out["nsamples"][4] == 0 and out["eta"][4] == 0 and out["psi"][4] == 0 and not out["tilt"][4].any() and out["last_step"][4] == 0
    assert np.array_equal(out["g"][:, 4], c["g"][:, 4]) and np.array_equal(out["model"][:, 4], c["m"][:, 4])
    assert np.abs(out["g"][:, 5] - c["g_true"][:, 5]).max() < 1e-12


@pytest.mark.parametrize("mode", ["channel", "band"])
def test_invariance(mode):
    """The product the fit constrains is unchanged, whatever the reference is (here: unrelated noise)."""
    c = degenerate_case(ARRAYS["hex"], seed=4, autos=True)
    rng = np.random.default_rng(5)
    s = c["s"] + 0.3 * (rng.normal(size=c["s"].shape) + 1j * rng.normal(size=c["s"].shape))
    out = R.fix_degeneracies(c["m"], s, c["w"], c["g"], c["ant0"], c["ant1"], c["antpos"], mode=mode, freqs=c["freqs"], gref=c["g_true"])
    before = c["g"][c["ant0"]] * np.conj(c["g"][c["ant1"]]) * c["m"]
    after = out["g"][c["ant0"]] * np.conj(out["g"][c["ant1"]]) * out["model"]
    assert np.abs(after - before).max() < 1e-13 * np.abs(before).max()


BAD_KEYWORDS = [
    (dict(fix_degeneracies="both"), "fix_degeneracies"),
    (dict(fix_degeneracies=True, degeneracy_iters=0), "degeneracy_iters"),
    (dict(fix_degeneracies=True, sky_model=None), "sky_model"),
    (dict(fix_degeneracies=True, freeze_model=True), "freeze_model"),
    (dict(fix_degeneracies=True, model_regularization="post_hoc"), "post_hoc"),
    (dict(fix_degeneracies=True, devices=(0, 1), device_split="groups"), "devices"),
]


@pytest.mark.parametrize("kw,word", BAD_KEYWORDS, ids=[b[1] for b in BAD_KEYWORDS])
def test_bad_keywords_raise_before_a_solver_exists(kw, word, monkeypatch):
    from calamity_amd import batched, calibration, solver

    def no_solver(*a, **k):
        raise AssertionError("a solver was created before the keywords were checked")

    monkeypatch.setattr(solver.HipFitSolver, "__init__", no_solver)
    monkeypatch.setattr(batched.SliceBatchFitter, "__init__", no_solver)
    sentinel = object()
    args = dict(sky_model=sentinel, model_regularization=None)
    args.update(kw)
    with pytest.raises(ValueError, match=word):
        calibration.check_degeneracy_keywords(**{k: args.get(k, d) for k, d in (
            ("fix_degeneracies", False), ("degeneracy_iters", 6), ("sky_model", sentinel), ("freeze_model", False),
            ("model_regularization", None), ("devices", None), ("device_split", "slices"))})
    with pytest.raises(ValueError, match=word):
        calibration.calibrate_and_model_tensor(uvdata=None, fg_model_comps_dict={}, **args)
