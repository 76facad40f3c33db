#!/usr/bin/env python3
"""Generates tests/golden/fit_loop/table.npz: what the host loop did at commit ``COMMIT``, before its three option classes became one
controls object, its gap an action list and its return value one result (tests/test_fit_loop_table.py replays it on today's code).

The package's Python files of that commit are read out of git into a temporary directory and imported from there -- this program
never imports the working tree's package.  Recorded, over the cases of tests/fit_loop_cases.py:

* ``check_index`` / ``check_messages``: per check case ``-1`` (accepted) or the index of ``"<exception type>: <text>"``, from the three
  ``check`` methods chained as every caller chained them (``FitOptions``, then Gauss-Newton, then L-BFGS);
* ``log_digests``: per fit case the BLAKE2b-128 digest of the canonical JSON of its record -- every call ``drive`` made on the scripted
  fitter with its arguments, what it returned, every loop's ``history_entry`` (the plain logs are megabytes);
* ``parser``: every action of ``dpss_fit_argparser()`` and the namespace of a minimal command line, as JSON.

``--show N`` prints fit case N with its record at ``COMMIT`` instead, to compare against ``fit_loop_cases.new_record`` after a mismatch.
"""
import argparse
import io
import json
import os
import subprocess
import sys
import tarfile
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
COMMIT = "c07a13cd3f5e38bdb398e416524b6634cec0d0a4"
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fit_loop_cases as cases  # noqa: E402


def import_parent(tmp):
    """``(fit_loop, calibration)`` of ``COMMIT``."""
    tar = subprocess.run(["git", "-C", ROOT, "archive", COMMIT, "--", "calamity_amd"], check=True, capture_output=True).stdout
    with tarfile.open(fileobj=io.BytesIO(tar)) as f:
        f.extractall(tmp, members=[m for m in f.getmembers() if m.name.endswith(".py")])
    sys.path.insert(0, tmp)
    from calamity_amd import calibration, fit_loop

    assert os.path.dirname(fit_loop.__file__).startswith(tmp)
    return fit_loop, calibration


def sections(pl, keywords):
    return [cls(**{k: v for k, v in keywords.items() if k in cls.__dataclass_fields__}) for cls in (pl.FitOptions, pl.GaussNewtonOptions, pl.LbfgsOptions)]


def parent_check(pl, keywords):
    opts, newton, lbfgs = sections(pl, keywords)

    def check(freq_basis_given, time_basis_given, freeze_model, use_min, robust_first=False, groups_split=False):
        opts.check(freq_basis_given, time_basis_given, freeze_model, use_min, robust_first=robust_first)
        newton.check(opts, freq_basis_given, time_basis_given, freeze_model, groups_split=groups_split)
        lbfgs.check(opts, newton, groups_split=groups_split)

    return check


def parent_record(pl, case, rows=2):
    opts, newton, lbfgs = sections(pl, case["keywords"])
    fitter = cases.scripted_fitter(case, rows)
    loops, nsingular, sweep_singular, robust, gn, lb = pl.drive(fitter, opts, case["nl"], rows, case["maxsteps"], cases.TOL, False, case["freeze_model"],
                                                                newton=newton, lbfgs=lbfgs)
    history = []
    for t in range(case["nl"]):  # (the reweighting in solver units and row order, as fit_gains_and_foregrounds files its one loop)
        rb = robust and {"rounds": int(robust["rounds"][t]), "ndown_bl": robust["ndown_bl"][t * rows : (t + 1) * rows],
                         "scale_bl": robust["scale_bl"][t * rows : (t + 1) * rows]}
        history.append(pl.history_entry(opts, loops[t][0], np.dtype(np.float64), nsingular, sweep_singular, rb, pl.newton_history(gn, t),
                                        pl.lbfgs_history(lb, t)))
    return cases.record(fitter.log, loops, nsingular, sweep_singular, robust, gn, lb, history)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--show", type=int, default=None, help="print this fit case and its record at COMMIT, write nothing")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        pl, calibration = import_parent(tmp)
        fits = cases.fit_cases(lambda kw, flags: cases.check_outcome(parent_check(pl, kw), flags) is None)
        if args.show is not None:
            print(json.dumps(dict(case=fits[args.show], record=parent_record(pl, fits[args.show])), indent=1))
            return
        outcomes = [cases.check_outcome(parent_check(pl, kw), flags) for kw, flags in cases.check_cases()]
        messages = sorted({o for o in outcomes if o is not None})
        index = np.asarray([-1 if o is None else messages.index(o) for o in outcomes], dtype=np.int16)
        records = [parent_record(pl, case) for case in fits]
        # the scripts do what the table is for: wherever Gauss-Newton steps were taken one of them was rejected, and some L-BFGS call
        # left one loop with status 2 and another with 0
        assert all(sum(r["newton"]["accepted"]) < sum(r["newton"]["steps"]) for r in records if r["newton"] and sum(r["newton"]["steps"]))
        assert any({0, 2} <= set(r["lbfgs"]["status"]) for r in records if r["lbfgs"])
        digests = np.frombuffer(b"".join(cases.digest(r) for r in records), dtype=np.uint8).reshape(len(records), 16)
        parser = json.dumps(cases.parser_record(calibration), sort_keys=True)
    out = os.path.join(HERE, "fit_loop", "table.npz")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    np.savez_compressed(out, commit=COMMIT, check_messages=np.asarray(messages), check_index=index, log_digests=digests, parser=parser)
    print(f"{out}: {len(outcomes)} checks ({len(messages)} messages, {int(np.sum(index < 0))} accepted), {len(records)} fits, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
