"""Today's calamity_amd/fit_loop.py against tests/golden/fit_loop/table.npz (no GPU, no library): the checks, the calls of ``drive`` and
the command line as the commit named in the table had them (tests/golden/make_fit_loop_table.py recorded it; its ``--show N`` prints
fit case N as that commit ran it).  Also: the keywords of the three sections are those of both public signatures."""
import dataclasses
import inspect
import json
import os

import numpy as np

import fit_loop_cases as cases
from calamity_amd import calibration
from calamity_amd.fit_loop import FitControls, FitOptions, GaussNewtonOptions, LbfgsOptions

TABLE = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fit_loop", "table.npz"))


def test_every_check_gives_the_recorded_outcome():
    messages, index = [str(m) for m in TABLE["check_messages"]], TABLE["check_index"]
    todo = cases.check_cases()
    assert len(todo) == len(index) == 64 * (384 + 2 * 27) and np.sum(index < 0) > 500 and len(messages) > 40
    controls = {}
    for (kw, flags), want in zip(todo, index):
        key = tuple(kw.items())
        if key not in controls:
            controls[key] = cases.new_controls(kw)
        assert cases.check_outcome(controls[key].check, flags) == (None if want < 0 else messages[want]), (kw, flags)


def test_every_fit_makes_the_recorded_calls_and_reports_the_recorded_history():
    digests = TABLE["log_digests"]
    fits = cases.fit_cases(lambda kw, flags: cases.check_outcome(cases.new_controls(kw).check, flags) is None)
    assert len(fits) == len(digests) > 1500
    for n, case in enumerate(fits):
        assert cases.digest(cases.new_record(case)) == digests[n].tobytes(), (n, case)


def test_the_scripts_reject_a_step_and_end_lbfgs_differently():
    """What the table is worth: the scripted fitter of its cases does reject Gauss-Newton steps and does end L-BFGS with status 2 on
    one loop and 0 on another."""
    case = dict(keywords=dict(gauss_newton_rounds=2, lbfgs_steps=3, lbfgs_every=4, gauss_newton_every=4), freeze_model=False, nl=3, maxsteps=12,
                script="apart", chunk=4)
    rec = cases.new_record(case)
    assert [c[0] for c in rec["calls"]].count("gauss_newton_step") == 4 and rec["newton"]["steps"] == [3, 4, 4] and rec["newton"]["accepted"] == [2, 3, 3]
    assert {0, 2} <= set(rec["lbfgs"]["status"]) and rec["lbfgs"]["calls"] == [2, 3, 3]
    assert [k for k, _ in rec["history"][0]] == ["loss", "gauss_newton", "lbfgs"]


def test_the_command_line_is_the_recorded_one():
    want = json.loads(str(TABLE["parser"]))
    assert json.loads(json.dumps(cases.parser_record(calibration), sort_keys=True)) == want
    assert len(want["actions"]) == 70 and want["namespace"]["lbfgs_history"] == 8


def test_the_sections_are_the_public_keywords_with_their_defaults():
    fields = FitControls.keyword_fields()
    assert [f.name for f in fields] == [f.name for cls in (FitOptions, GaussNewtonOptions, LbfgsOptions) for f in dataclasses.fields(cls)] and len(fields) == 27
    for fn in (calibration.fit_gains_and_foregrounds, calibration.calibrate_and_model_tensor):
        params = inspect.signature(fn).parameters
        names = [k for k in params if k in {f.name for f in fields}]
        assert names == [f.name for f in fields], fn.__name__  # every keyword, in the order of the sections
        for f in fields:
            assert params[f.name].default == f.default and type(params[f.name].default) is type(f.default) is f.type, (fn.__name__, f.name)
    assert FitControls.pick(dict({f.name: f.default for f in fields}, dtype="other keywords are left alone")) == FitControls()
    assert FitControls().keywords() == {f.name: f.default for f in fields} and list(FitControls().keywords()) == [f.name for f in fields]
