"""``fit_loop.FitOptions`` (no GPU): its fields are the public keywords with their public defaults, and what it derives from them
-- the sweep family, its numbers, the chunk length of the recorded loop."""
import dataclasses
import inspect

import pytest

from calamity_amd import calibration
from calamity_amd.fit_loop import FitOptions

BASE = ["--input_data_files", "x.uvh5"]


def test_fields_are_the_public_keywords_with_their_defaults():
    fields = dataclasses.fields(FitOptions)
    assert len(fields) == 17
    signatures = [inspect.signature(fn).parameters for fn in (calibration.calibrate_and_model_tensor, calibration.fit_gains_and_foregrounds)]
    parsed = [ap.parse_args(BASE) for ap in (calibration.fitting_argparser(), calibration.dpss_fit_argparser())]
    for f in fields:
        for params in signatures:
            assert params[f.name].default == f.default and type(params[f.name].default) is type(f.default), f.name
        for args in parsed:
            assert getattr(args, f.name) == f.default and type(getattr(args, f.name)) is type(f.default), f.name
    assert FitOptions.pick(dict({f.name: f.default for f in fields}, dtype="other keywords are left alone")) == FitOptions()


@pytest.mark.parametrize("robust", [0, 5])
def test_family_sweep_and_chunk(robust):
    cases = [(dict(), None, (0, 0, None, None)),
             (dict(gain_solve_sweeps=3, gain_solve_every=5, gain_solve_damping=0.25), "gain", (3, 5, 0.25, None)),
             (dict(gain_basis_solve_every=5, gain_basis_solve_damping=0.25, gain_basis_solve_ridge=1e-3), "basis", (0, 5, 0.25, 1e-3)),
             (dict(gain_time_solve_sweeps=2, gain_time_solve_every=5, gain_time_solve_ridge=0.0), "time", (2, 5, 0.5, 0.0))]
    for kw, family, sweep in cases:
        opts = FitOptions(robust_every=robust, **kw)
        assert opts.family == family and opts.sweep == sweep
        assert opts.chunk == (5 if family or robust else 0) and opts.chunked == bool(family or robust)
        opts.check(family == "basis", family == "time", False, False)
        opts.check(family == "basis", family == "time", False, False, robust_first=True)
    # sweeps before the loop only: the recorded loop is one call, or the reweighting's chunks
    opts = FitOptions(gain_solve_sweeps=3, robust_every=robust)
    assert opts.family == "gain" and opts.chunk == robust and opts.chunked == bool(robust)


def test_the_two_orders_of_check():
    opts = FitOptions(robust_kind="tukey", gain_solve_damping=2.0)
    with pytest.raises(ValueError, match="gain_solve_damping"):
        opts.check(False, False, False, False)
    with pytest.raises(ValueError, match="robust_kind"):
        opts.check(False, False, False, False, robust_first=True)
    FitOptions(gain_solve_sweeps=True).check(False, False, False, False)  # accepted, as ever
    with pytest.raises(ValueError, match="gain_basis_solve_sweeps and gain_basis_solve_every must be non-negative integers"):
        FitOptions(gain_basis_solve_sweeps=True).check(True, False, False, False)
