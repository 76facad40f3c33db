"""The host loop of a fit (calamity_amd/fit_loop.py: drive) against a scripted fitter that records every call (no GPU, no library):
the order of the calls and their arguments are the contract, DESIGN.md "The host loop"."""
import glob
import json

import numpy as np

from calamity_amd.fit_loop import FitControls, FitOptions, FitResult, drive, history_entry
from fit_loop_cases import TOL, UNRECORDED, Fake, going, recorded


def run(fake, opts, nl, maxsteps, rows=0, **kw):
    """The four fields of the result that the closed-form solves and the reweighting fill."""
    r = drive(fake, FitControls(opts), nl, rows // nl, maxsteps, TOL, False, False, **kw)
    assert r.newton is None and r.lbfgs is None
    return r.loops, r.nsingular, r.sweep_singular, r.robust


def test_plain_fit_is_one_unrecorded_step_and_one_call():
    script = going(7, 3)
    fake = Fake([script], nl=3)
    results, nsingular, sweep_singular, robust = run(fake, FitOptions(), 3, 7)
    assert fake.log == [UNRECORDED, recorded(7)]
    assert results is script and nsingular is None and sweep_singular is None and robust is None


def test_start_up_rounds():
    coeffs = ("solve_coeffs", (), dict(ridge=1e-4))
    sweeps = ("solve_gains", (3,), dict(damping=0.25))
    for rounds, nsweeps, want in ((2, 3, [coeffs, sweeps, coeffs, sweeps]), (0, 3, [sweeps]), (2, 0, [coeffs, coeffs])):
        fake = Fake([going(4, 1)])
        opts = FitOptions(coeff_solve_rounds=rounds, coeff_solve_ridge=1e-4, gain_solve_sweeps=nsweeps, gain_solve_damping=0.25)
        _, nsingular, sweep_singular, _ = run(fake, opts, 1, 4)
        assert fake.log == want + [UNRECORDED, recorded(4)], (rounds, nsweeps)
        # the count of the LAST coefficient solve (the fake numbers its calls); per-channel sweeps have none
        assert nsingular == (None if rounds == 0 else len(want) - (nsweeps > 0)) and sweep_singular is None


def test_chunks_gaps_masks_and_what_a_stopped_loop_returns():
    second = going(5, 3)
    second[1] = (np.arange(3, dtype=np.float64), True, 3)  # loop 1 meets the tolerance inside the second chunk
    third = going(2, 3)
    third[1] = (np.zeros(0), True, 0)  # (held: the library reports it as stopped, with nothing recorded)
    fake = Fake([going(5, 3), second, third], nl=3)
    opts = FitOptions(gain_solve_every=5, coeff_solve_rounds=1)
    results, nsingular, sweep_singular, robust = run(fake, opts, 3, 12)

    def gap(over):
        mask = [1 - o for o in over]
        return [("hold_slices", (over,), {}), ("solve_coeffs", (), dict(ridge=1e-6, slice_mask=mask, reset_coeff_moments=True)),
                ("solve_gains", (1,), dict(damping=0.5, slice_mask=mask, reset_gain_moments=True))]  # max(1, 0) sweeps

    assert fake.log == ([("solve_coeffs", (), dict(ridge=1e-6)), UNRECORDED, recorded(5)] + gap([0, 0, 0]) + [recorded(5)] + gap([0, 1, 0])
                        + [recorded(2), ("hold_slices", (None,), {})])
    assert [len(r[0]) for r in results] == [12, 8, 12]
    np.testing.assert_array_equal(results[1][0], np.concatenate([np.arange(5.0), np.arange(3.0)]))
    assert [r[1] for r in results] == [False, True, False]
    assert [r[2] for r in results] == [12, 8, 12]  # summed over the chunks in which the loop was running
    assert nsingular == 9 and sweep_singular is None and robust is None  # (the second gap's coefficient solve is log entry 9)


def test_the_loop_ends_when_every_loop_is_over():
    second = [(np.arange(5, dtype=np.float64), True, 5), (np.arange(2, dtype=np.float64), False, 2)]  # stopped; a short chunk
    fake = Fake([going(5, 2), second], nl=2)
    results, _, _, _ = run(fake, FitOptions(gain_solve_every=5), 2, 40)
    assert fake.log == [UNRECORDED, recorded(5), ("hold_slices", ([0, 0],), {}),
                        ("solve_gains", (1,), dict(damping=0.5, slice_mask=[1, 1], reset_gain_moments=True)), recorded(5),
                        ("hold_slices", (None,), {})]
    assert [(len(r[0]), r[1], r[2]) for r in results] == [(10, True, 10), (7, True, 7)]


def test_robust_rounds_and_rows_of_loops_left_alone():
    second = going(4, 2)
    second[1] = (np.arange(1, dtype=np.float64), True, 1)
    held = [(np.arange(4, dtype=np.float64), False, 4), (np.zeros(0), True, 0)]
    fake = Fake([going(4, 2), second, held, held], nl=2, rows=6)
    opts = FitOptions(robust_every=4, robust_rounds=2, robust_kind="cauchy", robust_threshold=2.5)
    results, nsingular, sweep_singular, robust = run(fake, opts, 2, 16, rows=6)

    def reweight(mask):
        return ("robust_weights", (), dict(kind="cauchy", threshold=2.5, slice_mask=mask))

    assert fake.log == [UNRECORDED, recorded(4), ("hold_slices", ([0, 0],), {}), reweight([1, 1]), recorded(4),
                        ("hold_slices", ([0, 1],), {}), reweight([1, 0]), recorded(4),
                        ("hold_slices", ([0, 1],), {}), recorded(4), ("hold_slices", (None,), {})]  # no third reweight of loop 0
    assert robust["rounds"].tolist() == [2, 1]
    # loop 0: the second reweight's rows; loop 1 took no part in it and keeps the first one's
    assert robust["ndown_bl"].tolist() == [200.0, 201.0, 202.0, 103.0, 104.0, 105.0]
    assert robust["scale_bl"].tolist() == [200.5, 201.5, 202.5, 103.5, 104.5, 105.5]
    assert [len(r[0]) for r in results] == [16, 5] and nsingular is None and sweep_singular is None
    # robust_rounds = 0: a reweight in every gap
    fake = Fake([going(4, 2) for _ in range(4)], nl=2, rows=6)
    _, _, _, robust = run(fake, FitOptions(robust_every=4), 2, 16, rows=6)
    assert [e[0] for e in fake.log].count("robust_weights") == 3 and robust["rounds"].tolist() == [3, 3]
    assert robust["ndown_bl"].tolist() == [300.0 + r for r in range(6)]


def test_a_gap_is_reweight_then_coefficients_then_sweeps():
    fake = Fake([going(5, 2), going(5, 2)], nl=2, rows=4)
    opts = FitOptions(robust_every=5, gain_solve_every=5, gain_solve_sweeps=2, coeff_solve_rounds=1)
    run(fake, opts, 2, 10, rows=4)
    assert fake.log[4:-2] == [("hold_slices", ([0, 0],), {}), ("robust_weights", (), dict(kind="huber", threshold=3.0, slice_mask=[1, 1])),
                              ("solve_coeffs", (), dict(ridge=1e-6, slice_mask=[1, 1], reset_coeff_moments=True)),
                              ("solve_gains", (2,), dict(damping=0.5, slice_mask=[1, 1], reset_gain_moments=True))]
    assert fake.log[:4] == [("solve_coeffs", (), dict(ridge=1e-6)), ("solve_gains", (2,), dict(damping=0.5)), UNRECORDED, recorded(5)]
    assert fake.log[-2:] == [recorded(5), ("hold_slices", (None,), {})]
    # sweeps before the loop only (no chunk length of their own) leave the gaps of the reweighting alone
    fake = Fake([going(5, 1), going(5, 1)], rows=2)
    run(fake, FitOptions(robust_every=5, gain_solve_sweeps=2), 1, 10, rows=2)
    assert [e[0] for e in fake.log] == ["solve_gains", "run_slices", "run_slices", "hold_slices", "robust_weights", "run_slices", "hold_slices"]


def test_the_basis_family_calls_its_own_solve():
    fake = Fake([going(5, 2), going(5, 2)], nl=2)
    opts = FitOptions(gain_basis_solve_sweeps=2, gain_basis_solve_every=5, gain_basis_solve_damping=0.75, gain_basis_solve_ridge=1e-3)
    _, nsingular, sweep_singular, _ = run(fake, opts, 2, 10)
    assert fake.log == [("solve_gain_coeffs", (2,), dict(damping=0.75, ridge=1e-3)), UNRECORDED, recorded(5), ("hold_slices", ([0, 0],), {}),
                        ("solve_gain_coeffs", (2,), dict(damping=0.75, ridge=1e-3, slice_mask=[1, 1], reset_gain_moments=True)), recorded(5),
                        ("hold_slices", (None,), {})]
    assert nsingular is None and sweep_singular == 5  # the last sweep's count
    # switched on, but no sweep came to run: the count is 0, not None
    fake = Fake([going(5, 2)], nl=2)
    assert run(fake, FitOptions(gain_basis_solve_every=5), 2, 5)[2] == 0


def test_the_time_family_has_no_mask_and_one_loop_over_all_rows():
    fake = Fake([going(5, 1), going(5, 1)], nl=1, rows=6)  # a joint fit of 2 times x 3 baselines
    opts = FitOptions(gain_time_solve_sweeps=2, gain_time_solve_every=5, gain_time_solve_damping=0.75, gain_time_solve_ridge=1e-3,
                      robust_every=5, coeff_solve_rounds=1)
    _, nsingular, sweep_singular, robust = run(fake, opts, 1, 10, rows=6)
    assert fake.log == [("solve_coeffs", (), dict(ridge=1e-6)), ("solve_gain_time_coeffs", (2,), dict(damping=0.75, ridge=1e-3)), UNRECORDED,
                        recorded(5), ("hold_slices", ([0],), {}), ("robust_weights", (), dict(kind="huber", threshold=3.0, slice_mask=[1])),
                        ("solve_coeffs", (), dict(ridge=1e-6, slice_mask=[1], reset_coeff_moments=True)),
                        ("solve_gain_time_coeffs", (2,), dict(damping=0.75, ridge=1e-3, reset_gain_moments=True)), recorded(5),
                        ("hold_slices", (None,), {})]
    assert (nsingular, sweep_singular) == (7, 8)
    assert robust["rounds"].tolist() == [1] and robust["ndown_bl"].tolist() == [100.0 + r for r in range(6)]


def test_profiled_steps_sit_between_the_solves_and_the_unrecorded_step(tmp_path):
    fake = Fake([going(4, 2)], nl=2)
    run(fake, FitOptions(coeff_solve_rounds=1), 2, 4, n_profile_steps=3, profile_log_dir=str(tmp_path / "log"), profile_extra=dict(slices=2))
    assert fake.log == [("solve_coeffs", (), dict(ridge=1e-6)), ("timing_enable", (True,), {}),
                        ("run_slices", (3,), dict(record=False, freeze_model=False)), ("timing_get", (), {}), ("timing_enable", (False,), {}),
                        UNRECORDED, recorded(4)]
    (path,) = glob.glob(str(tmp_path / "log" / "calamity_amd_profile_*.json"))
    with open(path) as f:
        assert json.load(f) == {"n_profile_steps": 3, "slices": 2, "fused_basis_kernel": {"mean_ms": 1.5}}
    # no extra keys: the file of a single solver
    fake = Fake([going(4, 1)])
    run(fake, FitOptions(), 1, 4, n_profile_steps=1, profile_log_dir=str(tmp_path / "one"))
    (path,) = glob.glob(str(tmp_path / "one" / "*.json"))
    with open(path) as f:
        assert json.load(f) == {"n_profile_steps": 1, "fused_basis_kernel": {"mean_ms": 1.5}}


def test_use_min_freeze_model_and_tol_reach_every_step():
    fake = Fake([going(3, 1)])
    drive(fake, FitControls(), 1, 0, 3, 1e-3, True, True)
    assert fake.log == [("run_slices", (1,), dict(record=False, freeze_model=True)),
                        ("run_slices", (3,), dict(record=True, tol=1e-3, use_min=True, freeze_model=True))]


def test_history_entry_keys_follow_the_configuration():
    f32 = np.dtype(np.float32)

    def entry(opts, losses, nsingular, sweep_singular, robust, as_reported=None):
        return history_entry(FitControls(opts), FitResult([(losses, False, 0)], nsingular, sweep_singular, robust), 0, f32, robust=as_reported)

    plain = entry(FitOptions(), np.arange(3.0), None, None, None)
    assert list(plain) == ["loss"] and plain["loss"] == [0.0, 1.0, 2.0] and all(type(l) is np.float32 for l in plain["loss"])
    reweights = dict(rounds=np.array([1]), ndown_bl=np.zeros(2), scale_bl=np.ones(2))
    basis = entry(FitOptions(gain_basis_solve_every=5), [], 2, 0, reweights, as_reported={"rounds": 1})
    assert basis == {"loss": [], "coeff_solve_singular": 2, "gain_basis_solve_singular": 0, "robust": {"rounds": 1}}
    assert list(basis) == ["loss", "coeff_solve_singular", "gain_basis_solve_singular", "robust"]
    # without the caller's own: the loop's reweights in solver units and row order
    own = entry(FitOptions(robust_every=5), [], None, None, reweights)["robust"]
    assert own["rounds"] == 1 and own["ndown_bl"].tolist() == [0.0, 0.0] and own["scale_bl"].tolist() == [1.0, 1.0]
    assert list(entry(FitOptions(gain_time_solve_sweeps=1), [], None, 4, None)) == ["loss", "gain_time_solve_singular"]
    assert list(entry(FitOptions(gain_solve_sweeps=1), [], None, None, None)) == ["loss"]
