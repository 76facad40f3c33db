"""Shared by the host tests of calamity_amd/fit_loop.py (no GPU, no library): the scripted fitters that record every call ``drive`` makes, and
the cases of tests/golden/fit_loop/table.npz -- the grid of options whose checks, and the fits whose call logs, were recorded from the
version of fit_loop.py before its controls became one object (tests/golden/make_fit_loop_table.py) and are replayed by
tests/test_fit_loop_table.py."""
import hashlib
import itertools
import json

import numpy as np

TOL = 1e-9
UNRECORDED = ("run_slices", (1,), dict(record=False, freeze_model=False))


def recorded(n):
    return ("run_slices", (n,), dict(record=True, tol=TOL, use_min=False, freeze_model=False))


def going(n, nl):
    """A chunk of ``n`` steps that every one of ``nl`` loops ran to its end."""
    return [(np.arange(n, dtype=np.float64), False, n) for _ in range(nl)]


class Fake:
    """Every method ``drive`` may call; ``chunks``: what the recorded ``run_slices`` calls return, in order; ``rows``: the baseline
    rows a reweight reports (call k: ``100 k + row`` for the rows of the selected loops, 0 for the others, like the library)."""

    def __init__(self, chunks=(), nl=1, rows=0):
        self.log, self.chunks, self.nl, self.rows, self.nrobust = [], list(chunks), nl, rows, 0

    def _put(self, name, args, kw):
        kw = {k: [int(x) for x in v] if k == "slice_mask" else v for k, v in kw.items()}
        self.log.append((name, args, kw))

    def run_slices(self, n, **kw):
        self._put("run_slices", (n,), kw)
        return self.chunks.pop(0) if kw["record"] else None

    def hold_slices(self, mask=None):
        self._put("hold_slices", (None if mask is None else [int(x) for x in mask],), {})

    def robust_weights(self, **kw):
        self._put("robust_weights", (), kw)
        self.nrobust += 1
        sel = np.repeat(np.asarray(kw["slice_mask"], dtype=bool), self.rows // self.nl)
        vals = np.where(sel, 100.0 * self.nrobust + np.arange(self.rows), 0.0)
        return dict(ndown_bl=vals, scale_bl=vals + 0.5)

    def solve_gains(self, n, **kw):
        self._put("solve_gains", (n,), kw)

    def solve_coeffs(self, **kw):
        self._put("solve_coeffs", (), kw)
        return dict(nsolved=9, nsingular=len(self.log))

    def solve_gain_coeffs(self, n, **kw):
        self._put("solve_gain_coeffs", (n,), kw)
        return dict(nsolved=9, nsingular=len(self.log))

    def solve_gain_time_coeffs(self, n, **kw):
        self._put("solve_gain_time_coeffs", (n,), kw)
        return dict(nsolved=9, nsingular=len(self.log))

    def timing_enable(self, on):
        self._put("timing_enable", (on,), {})

    def timing_get(self):
        self._put("timing_get", (), {})
        return {"mean_ms": 1.5}


class NewtonFake(Fake):
    """``accept``: per call the slices whose step is accepted."""

    def __init__(self, chunks=(), nl=1, rows=0, accept=()):
        super().__init__(chunks, nl, rows)
        self.accept = list(accept)

    def gauss_newton_step(self, **kw):
        lam = [float(x) for x in kw.pop("lam")]
        self._put("gauss_newton_step", (), dict(kw, lam=lam))
        ok = np.asarray(self.accept.pop(0), dtype=bool)
        k = len(self.log)
        return dict(loss_before=np.full(self.nl, 10.0 * k), loss_after=np.full(self.nl, 10.0 * k - 1.0), cg_residual=np.zeros(self.nl),
                    cg_iters=np.full(self.nl, k), accepted=ok)


class LbfgsFake(NewtonFake):
    """Every slice that takes part reports all the iterations asked for."""

    def lbfgs(self, nsteps, **kw):
        self._put("lbfgs", (nsteps,), kw)
        k = len(self.log)
        mask = np.asarray(kw.get("slice_mask", np.ones(self.nl)), dtype=bool)
        return dict(loss_before=np.full(self.nl, 10.0 * k), loss_after=np.full(self.nl, 10.0 * k - 1.0), iters=np.where(mask, nsteps, 0),
                    evals=np.where(mask, nsteps + 1, 0), pairs_dropped=np.zeros(self.nl, dtype=np.int64), status=np.where(mask, 0, 4),
                    losses=np.zeros((self.nl, nsteps + 1)))


# ---- the recorded table: the grid
FAMILIES = {None: {}, "gain": dict(gain_solve_sweeps=2, gain_solve_every=4), "basis": dict(gain_basis_solve_sweeps=2, gain_basis_solve_every=4),
            "time": dict(gain_time_solve_sweeps=2, gain_time_solve_every=4)}
COEFF_ROUNDS = (0, 2)
ROBUST_EVERY = (0, 4, 5)
GAUSS_NEWTON = ((0, 0), (2, 0), (0, 4), (0, 5))  # (gauss_newton_rounds, gauss_newton_every)
LBFGS = ((0, 0), (3, 0), (3, 4), (0, 4))  # (lbfgs_steps, lbfgs_every)
# one value out of range for every field that is validated
BAD_VALUES = dict(gain_solve_sweeps=-1, gain_solve_every=1.5, gain_solve_damping=0.0, coeff_solve_rounds=True, coeff_solve_ridge=-1.0,
                  gain_basis_solve_sweeps=True, gain_basis_solve_every=-2, gain_basis_solve_damping=1.5, gain_basis_solve_ridge=float("inf"),
                  gain_time_solve_sweeps=2.5, gain_time_solve_every=True, gain_time_solve_damping=-0.5, gain_time_solve_ridge=float("nan"),
                  robust_every=-1, robust_rounds=0.5, robust_kind="tukey", robust_threshold=0.0,
                  gauss_newton_rounds=True, gauss_newton_every=-3, gauss_newton_cg_iters=0, gauss_newton_lambda=-1e-3, gauss_newton_cg_tol=float("nan"),
                  lbfgs_steps=1.5, lbfgs_every=True, lbfgs_history=17, lbfgs_max_ls=0, lbfgs_ftol=float("inf"))
# (freq_basis_given, time_basis_given, freeze_model, use_min, robust_first, groups_split)
FLAGS = list(itertools.product((False, True), repeat=6))


def grid_keywords():
    """The keyword sets of the grid: family x coeff_solve_rounds x robust_every x Gauss-Newton x L-BFGS."""
    out = []
    for fam, coeff, robust, (gn_rounds, gn_every), (lb_steps, lb_every) in itertools.product(FAMILIES, COEFF_ROUNDS, ROBUST_EVERY, GAUSS_NEWTON, LBFGS):
        out.append(dict(FAMILIES[fam], coeff_solve_rounds=coeff, robust_every=robust, gauss_newton_rounds=gn_rounds, gauss_newton_every=gn_every,
                        lbfgs_steps=lb_steps, lbfgs_every=lb_every))
    return out


def check_cases():
    """``(keywords, flags)`` of every recorded check: the whole grid under every combination of the flags, then every bad value on the
    defaults and on a set of keywords that clash among themselves, so that the order of the messages across the sections shows."""
    clashing = dict(gain_solve_every=4, coeff_solve_rounds=2, robust_every=5, gauss_newton_every=5, lbfgs_steps=3, lbfgs_every=4)
    keywords = grid_keywords() + [dict(base, **{name: bad}) for name, bad in BAD_VALUES.items() for base in ({}, clashing)]
    return [(kw, flags) for kw in keywords for flags in FLAGS]


def check_outcome(check, flags):
    """``None`` or ``"<exception type>: <text>"`` of ``check(freq_basis_given, time_basis_given, freeze_model, use_min, robust_first=,
    groups_split=)``."""
    try:
        check(*flags[:4], robust_first=flags[4], groups_split=flags[5])
    except Exception as err:  # noqa: BLE001
        return f"{type(err).__name__}: {err}"
    return None


def new_controls(keywords):
    """Today's ``FitControls`` with ``keywords`` on top of the defaults."""
    from calamity_amd.fit_loop import FitControls

    return FitControls.pick({**{f.name: f.default for f in FitControls.keyword_fields()}, **keywords})


# ---- the recorded table: the fits
def fit_cases(valid):
    """Every fit whose calls are recorded.  ``valid(keywords, flags)``: whether the check accepts them.  Every keyword set of the grid
    that some fit may have (the flags: the gain bases its family needs, ``freeze_model`` both ways) x the loops x ``maxsteps`` a multiple
    of the chunk length or not x the script of the loops' ends."""
    out = []
    for kw in grid_keywords():
        fam = next((f for f in FAMILIES if f and FAMILIES[f].items() <= kw.items()), None)
        chunk = max(4 if fam else 0, kw["robust_every"], kw["gauss_newton_every"], kw["lbfgs_every"])
        for freeze_model in (False, True):
            if not valid(kw, (fam == "basis", fam == "time", freeze_model, False, False, False)):
                continue
            for nl, multiple, script in itertools.product((1, 3), (True, False), ("apart", "first", "none")):
                out.append(dict(keywords=kw, freeze_model=freeze_model, nl=nl, maxsteps=3 * (chunk or 4) - (0 if multiple else 2), script=script,
                                chunk=chunk))
    return out


class ScriptedFitter:
    """A fitter whose every answer follows from the calls made so far.  ``ends``: per loop the recorded step at which it meets the
    tolerance (``None``: never).  Of Gauss-Newton call ``k`` (from 0) loop ``t`` rejects the step where ``(k + t) % 3 == 0``; of L-BFGS
    call ``k`` a loop that takes part ends with status 2 where ``(k + t) % 3 == 0``, else 0, and the others report 4."""

    def __init__(self, nl, rows_per_loop, ends):
        self.log, self.nl, self.rows, self.ends = [], nl, rows_per_loop, ends
        self.done, self.held, self.count = np.zeros(nl, dtype=int), np.zeros(nl, dtype=bool), {}

    def _put(self, name, args, kw):
        self.log.append([name, plain(list(args)), plain(kw)])
        self.count[name] = self.count.get(name, 0) + 1
        return self.count[name] - 1

    def run_slices(self, n, **kw):
        self._put("run_slices", (n,), kw)
        if not kw["record"]:
            return None
        out = []
        for t in range(self.nl):
            if self.held[t]:
                out.append((np.zeros(0), True, 0))
                continue
            stop = self.ends[t] is not None and self.done[t] + n >= self.ends[t]
            m = self.ends[t] - self.done[t] if stop else n
            out.append((100.0 * t + 0.5 * (self.done[t] + np.arange(m, dtype=np.float64)), bool(stop), int(m)))
            self.done[t] += m
        return out

    def hold_slices(self, mask=None):
        self._put("hold_slices", (mask,), {})
        self.held = np.zeros(self.nl, dtype=bool) if mask is None else np.array(mask, dtype=bool)

    def robust_weights(self, **kw):
        k = self._put("robust_weights", (), kw)
        sel = np.repeat(np.asarray(kw["slice_mask"], dtype=bool), self.rows)
        vals = np.where(sel, 100.0 * (k + 1) + np.arange(self.nl * self.rows), 0.0)
        return dict(ndown_bl=vals, scale_bl=vals + 0.5)

    def solve_gains(self, n, **kw):
        self._put("solve_gains", (n,), kw)

    def solve_coeffs(self, **kw):
        return dict(nsolved=9, nsingular=self._put("solve_coeffs", (), kw))

    def solve_gain_coeffs(self, n, **kw):
        return dict(nsolved=9, nsingular=self._put("solve_gain_coeffs", (n,), kw) % 2)

    def solve_gain_time_coeffs(self, n, **kw):
        return dict(nsolved=9, nsingular=self._put("solve_gain_time_coeffs", (n,), kw) % 2)

    def gauss_newton_step(self, **kw):
        k = self._put("gauss_newton_step", (), kw)
        t = np.arange(self.nl)
        return dict(loss_before=50.0 - k + t, loss_after=49.5 - k + t, cg_residual=np.zeros(self.nl), cg_iters=3 + (k + t) % 4, accepted=(k + t) % 3 != 0)

    def lbfgs(self, nsteps, **kw):
        k = self._put("lbfgs", (nsteps,), kw)
        t = np.arange(self.nl)
        mask = np.asarray(kw.get("slice_mask", np.ones(self.nl)), dtype=bool)
        short = (k + t) % 3 == 0
        return dict(loss_before=30.0 - k + t, loss_after=29.25 - k + t, iters=np.where(mask, nsteps - short, 0), evals=np.where(mask, nsteps + 1 + t, 0),
                    pairs_dropped=np.zeros(self.nl, dtype=np.int64), status=np.where(mask, np.where(short, 2, 0), 4), losses=np.zeros((self.nl, nsteps + 1)))


def plain(v):
    """Arrays as lists, NumPy scalars as Python's, for JSON."""
    if isinstance(v, dict):
        return {k: plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [plain(x) for x in v]
    if isinstance(v, np.ndarray):
        return plain(v.tolist())
    if isinstance(v, np.generic):
        return v.item()
    return v


def scripted_fitter(case, rows_per_loop=2):
    nl, chunk, maxsteps = case["nl"], case["chunk"] or 4, case["maxsteps"]
    ends = {"none": [None] * nl, "first": [None] * (nl - 1) + [chunk - 1], "apart": [chunk + 2, None, 2 * chunk + 1][:nl]}[case["script"]]
    assert all(e is None or e < maxsteps for e in ends)
    return ScriptedFitter(nl, rows_per_loop, ends)


def record(calls, loops, nsingular, sweep_singular, robust, newton, lbfgs, history):
    """One fit as the table holds it; ``history``: every loop's ``history_entry``, its keys in their order."""
    return dict(calls=calls, loops=plain(loops), nsingular=plain(nsingular), sweep_singular=plain(sweep_singular), robust=plain(robust), newton=plain(newton),
                lbfgs=plain(lbfgs), history=[[[k, plain(v)] for k, v in entry.items()] for entry in history])


def canonical(rec):
    return json.dumps(rec, sort_keys=True, allow_nan=True)


def digest(rec):
    return hashlib.blake2b(canonical(rec).encode(), digest_size=16).digest()


def new_record(case, rows_per_loop=2):
    """The fit of ``case`` through today's ``drive`` and ``history_entry``."""
    from calamity_amd.fit_loop import drive, history_entry

    controls = new_controls(case["keywords"])
    fitter = scripted_fitter(case, rows_per_loop)
    r = drive(fitter, controls, case["nl"], rows_per_loop, case["maxsteps"], TOL, False, case["freeze_model"])
    history = [history_entry(controls, r, t, np.dtype(np.float64)) for t in range(case["nl"])]
    return record(fitter.log, r.loops, r.nsingular, r.sweep_singular, r.robust, r.newton, r.lbfgs, history)


def parser_record(calibration):
    """Every action of ``dpss_fit_argparser()`` and the namespace of a minimal command line."""
    ap = calibration.dpss_fit_argparser()
    actions = [[a.option_strings, a.dest, getattr(a.type, "__name__", None), a.default, a.nargs, a.help] for a in ap._actions]
    return dict(actions=actions, namespace=vars(ap.parse_args(["--input_data_files", "x"])))
