"""The host loop of a fit, stated once: ``FitControls`` holds the keywords that steer it in three sections (``FitOptions``: the
closed-form solves and the robust reweighting, ``GaussNewtonOptions``: the joint Gauss-Newton steps, ``LbfgsOptions``: the L-BFGS
iterations), ``drive`` issues everything between ``set_optimizer`` and reading the parameters back and returns one ``FitResult``,
``history_entry`` files a loop of it.  Host only: NumPy, never the library ("The host loop")."""
import dataclasses
import datetime
import json
import os

import numpy as np

# sweep family -> (prefix of its keywords, the fitter's call); the first family that is switched on is the fit's
_FAMILIES = {"time": ("gain_time_solve", "solve_gain_time_coeffs"), "basis": ("gain_basis_solve", "solve_gain_coeffs"),
             "gain": ("gain_solve", "solve_gains")}


def _count(v, allow_bool=False):
    """A non-negative integer (a ``bool`` only where it always was one)."""
    return (allow_bool or not isinstance(v, bool)) and int(v) == v and v >= 0


def _unit(v):
    return 0.0 < float(v) <= 1.0


def _finite_nonneg(v):
    return bool(np.isfinite(float(v)) and float(v) >= 0.0)


def _one_chunk_length(name, every, others, other_named):
    """The rule of the chunked loop: every ``*_every`` that is set names the same length.  ``others``: the lengths ``every`` (the
    keyword ``name``) has to agree with, ``other_named``: how the message names the one that differs (``{}``: its value)."""
    for other in others:
        if every and other and other != every:
            raise ValueError(f"{name}={every} and {other_named.format(other)} share the gaps of one chunked loop: give them the same value")


class _Section:
    """A group of public keywords as a frozen dataclass: the fields are the keywords, under their public names and defaults."""

    @classmethod
    def pick(cls, keywords):
        """The options out of a mapping that holds them among others (a public function's ``locals()``)."""
        return cls(**{f.name: keywords[f.name] for f in dataclasses.fields(cls)})


@dataclasses.dataclass(frozen=True)
class FitOptions(_Section):
    """The closed-form and robust keywords of ``calibrate_and_model_tensor`` / ``fit_gains_and_foregrounds`` (documented there),
    under their public names and defaults."""
    gain_solve_sweeps: int = 0
    gain_solve_every: int = 0
    gain_solve_damping: float = 0.5
    coeff_solve_rounds: int = 0
    coeff_solve_ridge: float = 1e-6
    gain_basis_solve_sweeps: int = 0
    gain_basis_solve_every: int = 0
    gain_basis_solve_damping: float = 0.5
    gain_basis_solve_ridge: float = 1e-6
    gain_time_solve_sweeps: int = 0
    gain_time_solve_every: int = 0
    gain_time_solve_damping: float = 0.5
    gain_time_solve_ridge: float = 1e-6
    robust_every: int = 0
    robust_rounds: int = 0
    robust_kind: str = "huber"
    robust_threshold: float = 3.0

    def _on(self, family):
        prefix = _FAMILIES[family][0]
        return bool(getattr(self, prefix + "_sweeps") or getattr(self, prefix + "_every"))

    @property
    def family(self):
        """Whose sweeps the fit runs: "time", "basis", "gain" or ``None``."""
        return next((fam for fam in _FAMILIES if self._on(fam)), None)

    @property
    def sweep(self):
        """``(sweeps, every, damping, ridge)`` of the family (ridge ``None`` for per-channel gains; no family: no sweeps)."""
        if self.family is None:
            return 0, 0, None, None
        prefix = _FAMILIES[self.family][0]
        return tuple(getattr(self, f"{prefix}_{k}", None) for k in ("sweeps", "every", "damping", "ridge"))

    @property
    def chunk(self):
        """Steps per chunk of the recorded loop (``check``: the sweeps and the reweighting share one length); 0: one call."""
        return self.sweep[1] or self.robust_every

    @property
    def chunked(self):
        return self.chunk > 0

    def _check_sweeps(self, family):
        prefix = _FAMILIES[family][0]
        sweeps, every, damping = (getattr(self, f"{prefix}_{k}") for k in ("sweeps", "every", "damping"))
        if not (_count(sweeps, family == "gain") and _count(every, family == "gain")):
            raise ValueError(f"{prefix}_sweeps and {prefix}_every must be non-negative integers, got {sweeps!r} and {every!r}")
        if not _unit(damping):
            raise ValueError(f"{prefix}_damping must lie in (0, 1], got {damping!r}")
        if family != "gain" and not _finite_nonneg(getattr(self, prefix + "_ridge")):
            raise ValueError(f"{prefix}_ridge must be finite and >= 0, got {getattr(self, prefix + '_ridge')!r}")
        return self._on(family)

    def _check_robust(self, use_min):
        every, rounds = self.robust_every, self.robust_rounds
        if not (_count(every) and _count(rounds)):
            raise ValueError(f"robust_every and robust_rounds must be non-negative integers, got {every!r} and {rounds!r}")
        if self.robust_kind not in ("huber", "cauchy", "clip"):
            raise ValueError(f"robust_kind must be 'huber', 'cauchy' or 'clip', got {self.robust_kind!r}")
        if not (np.isfinite(float(self.robust_threshold)) and float(self.robust_threshold) > 0.0):
            raise ValueError(f"robust_threshold must be finite and > 0 (it is in sigma), got {self.robust_threshold!r}")
        if not every:
            return
        if use_min:
            raise ValueError("robust_every rewrites the weights between chunks of the loop: losses under different weights are not comparable, so "
                             "use_min (the minimum over them) cannot be combined with it")
        _one_chunk_length("robust_every", every, (self.gain_solve_every, self.gain_basis_solve_every, self.gain_time_solve_every),
                          "the closed-form sweeps' chunk length {} (gain_solve_every / gain_basis_solve_every / gain_time_solve_every)")

    def check(self, freq_basis_given, time_basis_given, freeze_model, use_min, robust_first=False):
        """``ValueError`` before any device work.  The families in the order gain, coefficients, basis, time; the robust keywords
        after them (``calibrate_and_model_tensor``) or, ``robust_first``, in front (``fit_gains_and_foregrounds``)."""
        if robust_first:
            self._check_robust(use_min)
        gain_on = self._check_sweeps("gain")
        if gain_on and (freq_basis_given or time_basis_given):
            raise ValueError("gain_solve_sweeps / gain_solve_every solve free per-channel gains in closed form: they cannot be combined with "
                             "gain_basis / gain_max_dly / gain_time_basis / gain_time_scale (projecting the solved gains onto a basis is not implemented); a fit with a frequency gain basis has "
                             "gain_basis_solve_sweeps / gain_basis_solve_every")
        if not _count(self.coeff_solve_rounds):
            raise ValueError(f"coeff_solve_rounds must be a non-negative integer, got {self.coeff_solve_rounds!r}")
        if not _finite_nonneg(self.coeff_solve_ridge):
            raise ValueError(f"coeff_solve_ridge must be finite and >= 0, got {self.coeff_solve_ridge!r}")
        if self.coeff_solve_rounds and freeze_model:
            raise ValueError("coeff_solve_rounds solves the foreground coefficients in closed form: it cannot be combined with freeze_model, "
                             "which keeps them as given")
        basis_on = self._check_sweeps("basis")
        if basis_on and time_basis_given:
            raise ValueError("gain_basis_solve_sweeps / gain_basis_solve_every solve the coefficients of a frequency gain basis antenna by antenna: they "
                             "cannot be combined with gain_time_basis / gain_time_scale, whose variables couple the times (a joint system that is not implemented)")
        if basis_on and not freq_basis_given:
            raise ValueError("gain_basis_solve_sweeps / gain_basis_solve_every solve the coefficients of a frequency gain basis: give gain_basis or "
                             "gain_max_dly (free per-channel gains have gain_solve_sweeps / gain_solve_every)")
        time_on = self._check_sweeps("time")
        if time_on and not time_basis_given:
            raise ValueError("gain_time_solve_sweeps / gain_time_solve_every solve the coefficients of a joint fit over the times: give gain_time_basis "
                             "or gain_time_scale (a frequency gain basis alone has gain_basis_solve_sweeps / gain_basis_solve_every, free per-channel "
                             "gains have gain_solve_sweeps / gain_solve_every)")
        if time_on and (basis_on or gain_on):
            raise ValueError("gain_time_solve_sweeps / gain_time_solve_every are the sweeps of a fit with a gain time basis: they cannot be combined "
                             "with gain_basis_solve_sweeps / gain_basis_solve_every or gain_solve_sweeps / gain_solve_every")
        if not robust_first:
            self._check_robust(use_min)


@dataclasses.dataclass(frozen=True)
class GaussNewtonOptions(_Section):
    """The keywords of the joint Gauss-Newton steps of ``calibrate_and_model_tensor`` / ``fit_gains_and_foregrounds`` (documented
    there), under their public names and defaults."""
    gauss_newton_rounds: int = 0
    gauss_newton_every: int = 0
    gauss_newton_cg_iters: int = 20
    gauss_newton_lambda: float = 1e-3
    gauss_newton_cg_tol: float = 1e-3

    @property
    def on(self):
        return bool(self.gauss_newton_rounds or self.gauss_newton_every)

    def check(self, opts, freq_basis_given, time_basis_given, freeze_model, groups_split=False):
        """``ValueError`` before any device work.  ``opts``: the call's ``FitOptions`` (one chunk length for every ``*_every``);
        ``groups_split``: several devices share out the fitting groups of a slice."""
        rounds, every, iters = self.gauss_newton_rounds, self.gauss_newton_every, self.gauss_newton_cg_iters
        if not (_count(rounds) and _count(every)):
            raise ValueError(f"gauss_newton_rounds and gauss_newton_every must be non-negative integers, got {rounds!r} and {every!r}")
        if not (_count(iters) and iters >= 1):
            raise ValueError(f"gauss_newton_cg_iters must be a positive integer, got {iters!r}")
        if not _finite_nonneg(self.gauss_newton_lambda):
            raise ValueError(f"gauss_newton_lambda must be finite and >= 0, got {self.gauss_newton_lambda!r}")
        if not _finite_nonneg(self.gauss_newton_cg_tol):
            raise ValueError(f"gauss_newton_cg_tol must be finite and >= 0, got {self.gauss_newton_cg_tol!r}")
        if not self.on:
            return
        if freq_basis_given:
            raise ValueError("gauss_newton_rounds / gauss_newton_every step the free per-channel gains and the coefficients together: they cannot be "
                             "combined with gain_basis / gain_max_dly (the step projected on the basis coefficients is not implemented)")
        if time_basis_given:
            raise ValueError("gauss_newton_rounds / gauss_newton_every step the free per-channel gains and the coefficients together: they cannot be "
                             "combined with gain_time_basis / gain_time_scale (the step projected on the basis coefficients is not implemented)")
        if freeze_model:
            raise ValueError("gauss_newton_rounds / gauss_newton_every move the foreground coefficients: they cannot be combined with freeze_model, "
                             "which keeps them as given (gain_solve_sweeps is the exact answer for the gains alone)")
        if groups_split:
            raise ValueError("gauss_newton_rounds / gauss_newton_every need every slice whole on one device: several devices that share out the "
                             "fitting groups (device_split='groups', or too few batches for the devices) would have to exchange the per-slice scalars of "
                             "conjugate gradients, which is not implemented; device_split='slices' works")
        _one_chunk_length("gauss_newton_every", every, (opts.chunk,),
                          "the chunk length {} of gain_solve_every / gain_basis_solve_every / gain_time_solve_every / robust_every")


@dataclasses.dataclass(frozen=True)
class LbfgsOptions(_Section):
    """The keywords of the L-BFGS iterations of ``calibrate_and_model_tensor`` / ``fit_gains_and_foregrounds`` (documented there),
    under their public names and defaults."""
    lbfgs_steps: int = 0
    lbfgs_every: int = 0
    lbfgs_history: int = 8
    lbfgs_max_ls: int = 20
    lbfgs_ftol: float = 0.0

    @property
    def on(self):
        return bool(self.lbfgs_steps or self.lbfgs_every)

    def check(self, opts, newton=None, groups_split=False):
        """``ValueError`` before any device work.  ``opts``: the call's ``FitOptions``, ``newton``: its ``GaussNewtonOptions`` (one chunk
        length for every ``*_every``); ``groups_split``: several devices share out the fitting groups of a slice.  Gain bases and
        ``freeze_model`` need no check: the iterations run on the optimizer's own variables."""
        steps, every, history, max_ls = self.lbfgs_steps, self.lbfgs_every, self.lbfgs_history, self.lbfgs_max_ls
        if not (_count(steps) and _count(every)):
            raise ValueError(f"lbfgs_steps and lbfgs_every must be non-negative integers, got {steps!r} and {every!r}")
        if not (_count(history) and 1 <= history <= 16):
            raise ValueError(f"lbfgs_history must be an integer in [1, 16], got {history!r}")
        if not (_count(max_ls) and max_ls >= 1):
            raise ValueError(f"lbfgs_max_ls must be a positive integer, got {max_ls!r}")
        if not _finite_nonneg(self.lbfgs_ftol):
            raise ValueError(f"lbfgs_ftol must be finite and >= 0, got {self.lbfgs_ftol!r}")
        if not self.on:
            return
        if every and not steps:
            raise ValueError(f"lbfgs_every={every} says where the iterations run, lbfgs_steps how many: give lbfgs_steps >= 1 with it")
        if groups_split:
            raise ValueError("lbfgs_steps / lbfgs_every need every slice whole on one device: several devices that share out the fitting groups "
                             "(device_split='groups', or too few batches for the devices) would have to exchange the dot products of the history, "
                             "which is not implemented; device_split='slices' works")
        _one_chunk_length("lbfgs_every", every, (opts.chunk, newton.gauss_newton_every if newton is not None else 0),
                          "the chunk length {} of gain_solve_every / gain_basis_solve_every / gain_time_solve_every / robust_every / gauss_newton_every")


@dataclasses.dataclass(frozen=True)
class FitControls:
    """Everything that steers the host loop of one call: the three sections of keywords."""
    fit: FitOptions = FitOptions()
    newton: GaussNewtonOptions = GaussNewtonOptions()
    lbfgs: LbfgsOptions = LbfgsOptions()

    @classmethod
    def pick(cls, keywords):
        """The controls out of a mapping that holds their keywords among others (a public function's ``locals()``)."""
        return cls(*(f.type.pick(keywords) for f in dataclasses.fields(cls)))

    @classmethod
    def keyword_fields(cls):
        """The dataclass fields of every keyword, in the order of the public signatures."""
        return [k for f in dataclasses.fields(cls) for k in dataclasses.fields(f.type)]

    def keywords(self):
        """The keywords as one mapping, to pass on to a public function."""
        return {f.name: getattr(section, f.name) for section in (self.fit, self.newton, self.lbfgs) for f in dataclasses.fields(section)}

    @property
    def chunk(self):
        """Steps per chunk of the recorded loop, the one length of every ``*_every`` that is set (``check``); 0: one call."""
        return self.fit.chunk or self.newton.gauss_newton_every or self.lbfgs.lbfgs_every

    def check(self, freq_basis_given, time_basis_given, freeze_model, use_min, robust_first=False, groups_split=False):
        """``ValueError`` before any device work: the sections' checks in the order ``FitOptions`` (``robust_first``: see there),
        Gauss-Newton, L-BFGS.  ``groups_split``: several devices share out the fitting groups of a slice."""
        self.fit.check(freq_basis_given, time_basis_given, freeze_model, use_min, robust_first=robust_first)
        self.newton.check(self.fit, freq_basis_given, time_basis_given, freeze_model, groups_split=groups_split)
        self.lbfgs.check(self.fit, self.newton, groups_split=groups_split)


# keyword -> its help text on the command line (``calibration.fitting_argparser`` makes one argument of every field above)
KEYWORD_HELP = {
    "gain_solve_sweeps": "solve the gains in closed form (damped StefCal sweeps) this many times before the first descent step; default 0: descent only",
    "gain_solve_every": "run gain sweeps (--gain_solve_sweeps of them, at least one) after every this many recorded descent steps; default 0: never",
    "gain_solve_damping": "damping of a gain sweep, in (0, 1]: g <- (1 - damping) g + damping x the closed-form minimiser; default 0.5",
    "coeff_solve_rounds": "before the first descent step, this many rounds of [the foreground coefficients in closed form, then "
                          "--gain_solve_sweeps gain sweeps]; with --gain_solve_every one coefficient solve in front of every later group of sweeps; "
                          "default 0: descent only",
    "coeff_solve_ridge": "ridge of a coefficient solve, as a fraction of the mean diagonal of a group's normal matrix; default 1e-6",
    "gain_basis_solve_sweeps": "with --gain_max_dly: solve the gain-basis coefficients in closed form (damped StefCal sweeps projected on the basis) this "
                               "many times before the first descent step; default 0: descent only",
    "gain_basis_solve_every": "with --gain_max_dly: run basis sweeps (--gain_basis_solve_sweeps of them, at least one) after every this many recorded "
                              "descent steps; default 0: never",
    "gain_basis_solve_damping": "damping of a basis sweep, in (0, 1]: y <- y + damping x the closed-form step; default 0.5",
    "gain_basis_solve_ridge": "ridge of a basis sweep, as a fraction of the mean diagonal of an antenna's normal matrix; default 1e-6",
    "gain_time_solve_sweeps": "with --gain_time_scale: solve the coefficients of the joint fit over the times in closed form (damped StefCal sweeps "
                              "taken jointly over the times) this many times before the first descent step; default 0: descent only",
    "gain_time_solve_every": "with --gain_time_scale: run joint sweeps (--gain_time_solve_sweeps of them, at least one) after every this many "
                             "recorded descent steps; default 0: never",
    "gain_time_solve_damping": "damping of a joint sweep, in (0, 1]: y <- y + damping x the closed-form step; default 0.5",
    "gain_time_solve_ridge": "ridge of a joint sweep, as a fraction of the mean diagonal of a system's normal matrix; default 1e-6",
    "robust_every": "downweight outliers: recompute the weights from the residual (iteratively reweighted least squares, scale from each "
                    "baseline's median) after every this many recorded descent steps; with a --gain*_solve_every flag both must be equal; "
                    "default 0: never",
    "robust_rounds": "with --robust_every: reweight at most this many times; default 0: after every chunk",
    "robust_kind": "weight function of --robust_every: huber, cauchy or clip; default huber",
    "robust_threshold": "threshold of the weight function in sigma; default 3",
    "gauss_newton_rounds": "joint Gauss-Newton steps over gains and coefficients (conjugate gradients on the joint normal matrix) before the first "
                           "descent step, after the --coeff_solve_rounds rounds and the start-up sweeps; default 0: none",
    "gauss_newton_every": "one joint Gauss-Newton step after every this many recorded descent steps, behind the reweighting, the coefficient solve "
                          "and the sweeps of the gap; with another --*_every flag both must be equal; default 0: never",
    "gauss_newton_cg_iters": "conjugate-gradient iterations of a Gauss-Newton step; default 20",
    "gauss_newton_lambda": "initial Levenberg damping of a Gauss-Newton step (a tenth after an accepted step, ten times after a rejected one); default 1e-3",
    "gauss_newton_cg_tol": "relative preconditioned residual at which the conjugate gradients of a step stop early; default 1e-3",
    "lbfgs_steps": "iterations of L-BFGS over the optimizer's own variables (gains or gain-basis coefficients, and the foreground "
                   "coefficients unless the model is frozen) before the first descent step, after the start-up rounds and the "
                   "Gauss-Newton rounds; works with --gain_max_dly, --gain_time_scale and a frozen model; default 0: none",
    "lbfgs_every": "with --lbfgs_steps: that many iterations again after every this many recorded descent steps, last in the gap; with "
                   "another --*_every flag both must be equal; default 0: never",
    "lbfgs_history": "stored pairs of L-BFGS, 1 to 16; default 8",
    "lbfgs_max_ls": "trials of a backtracking line search of L-BFGS; default 20",
    "lbfgs_ftol": "a slice's L-BFGS iterations stop once the loss falls by no more than this fraction; default 0: never",
}


def next_lambda(lam, accepted):
    """The damping after a step: a tenth where the step was accepted, ten times ``max(lambda, 1e-6)`` where it was rejected."""
    lam = np.asarray(lam, dtype=np.float64)
    return np.where(np.asarray(accepted, dtype=bool), lam / 10.0, 10.0 * np.maximum(lam, 1e-6))


def newton_history(gn, t):
    """Loop ``t``'s ``fit_history[...]["gauss_newton"]`` from ``FitResult.newton`` (``None`` while the steps are off)."""
    if gn is None:
        return None
    return {"steps": int(gn["steps"][t]), "accepted": int(gn["accepted"][t]), "lambda": float(gn["lambda"][t]), "loss": list(gn["loss"][t]),
            "cg_iters": list(gn["cg_iters"][t])}


def lbfgs_history(lb, t):
    """Loop ``t``'s ``fit_history[...]["lbfgs"]`` from ``FitResult.lbfgs`` (``None`` while the iterations are off)."""
    if lb is None:
        return None
    return {"calls": int(lb["calls"][t]), "iters": int(lb["iters"][t]), "evals": int(lb["evals"][t]), "loss": list(lb["loss"][t]),
            "status": int(lb["status"][t])}


class _Action:
    """One thing a fit does besides descent steps.  ``start()``: its work before the first descent step; ``gap(running)``: its work between
    two chunks of the recorded loop, on the mask of the loops not yet over; ``fields()``: what it adds to the ``FitResult``, unless it says
    otherwise its per-loop ``record`` as the field ``name``; ``entry(record, t)``: loop ``t`` of that record as ``fit_history`` reports it.
    ``drive`` runs its list of actions front to back both times."""

    def start(self):
        pass

    def gap(self, running):
        pass

    def fields(self):
        return {self.name: self.record}


class _Reweight(_Action):
    """``robust_every``: per loop the reweights it took part in, per baseline row what its last one reported."""
    name = "robust"

    def __init__(self, fitter, o, nl, rows_per_loop):
        self.fitter, self.o, self.rows_per_loop = fitter, o, rows_per_loop
        self.record = dict(rounds=np.zeros(nl, dtype=np.int64), ndown_bl=np.zeros(nl * rows_per_loop), scale_bl=np.zeros(nl * rows_per_loop))

    def gap(self, running):
        o, rec = self.o, self.record
        todo = running if o.robust_rounds == 0 else running & (rec["rounds"] < o.robust_rounds)
        if np.any(todo):
            rw = self.fitter.robust_weights(kind=o.robust_kind, threshold=o.robust_threshold, slice_mask=todo)
            rows = np.repeat(todo, self.rows_per_loop)
            rec["ndown_bl"][rows] = rw["ndown_bl"][rows]
            rec["scale_bl"][rows] = rw["scale_bl"][rows]
            rec["rounds"] += todo

    @staticmethod
    def entry(rec, t):
        """Solver units and row order; a caller that reports other units hands ``history_entry`` its own."""
        n = len(rec["ndown_bl"]) // len(rec["rounds"])
        rows = slice(t * n, (t + 1) * n)
        return {"rounds": int(rec["rounds"][t]), "ndown_bl": rec["ndown_bl"][rows], "scale_bl": rec["scale_bl"][rows]}


class _ClosedForm(_Action):
    """``coeff_solve_rounds`` and the sweeps of the fit's family: the singular counts of the last coefficient solve and the last sweep."""

    def __init__(self, fitter, o):
        self.fitter, self.o, self.family = fitter, o, o.family
        self.sweeps, self.every, self.damping, self.ridge = o.sweep
        self.nsingular = self.last = None

    def _coeffs(self, **kw):
        self.nsingular = self.fitter.solve_coeffs(ridge=self.o.coeff_solve_ridge, **kw)["nsingular"]

    def _sweep(self, n, **kw):
        if self.family == "time":  # one system over the times: no slice mask
            kw.pop("slice_mask", None)
        if self.family != "gain":
            kw["ridge"] = self.ridge
        out = getattr(self.fitter, _FAMILIES[self.family][1])(n, damping=self.damping, **kw)
        self.last = None if self.family == "gain" else out["nsingular"]

    def start(self):
        if self.o.coeff_solve_rounds > 0:  # alternating least squares: rounds of (the coefficients in closed form, then the gain sweeps)
            for _ in range(self.o.coeff_solve_rounds):
                self._coeffs()
                if self.sweeps > 0:
                    self._sweep(self.sweeps)
        elif self.sweeps > 0:  # the coefficients are initialised: the gains in closed form before any descent step
            self._sweep(self.sweeps)

    def gap(self, running):
        if self.every > 0:
            if self.o.coeff_solve_rounds > 0:
                self._coeffs(slice_mask=running, reset_coeff_moments=True)
            self._sweep(max(1, self.sweeps), slice_mask=running, reset_gain_moments=True)

    def fields(self):
        return dict(nsingular=self.nsingular, sweep_singular=int(self.last or 0) if self.family in ("basis", "time") else None)


class _GaussNewton(_Action):
    """``gauss_newton_rounds`` / ``gauss_newton_every``: the damping is kept per loop (``next_lambda``); a rejected step is simply
    followed by the next one."""
    name = "newton"

    def __init__(self, fitter, o, nl):
        self.fitter, self.o, self.nl = fitter, o, nl
        self.record = dict(steps=np.zeros(nl, dtype=np.int64), accepted=np.zeros(nl, dtype=np.int64), loss=[[] for _ in range(nl)],
                           cg_iters=[[] for _ in range(nl)])
        self.record["lambda"] = np.full(nl, float(o.gauss_newton_lambda))

    def _step(self, todo, **kw):
        o, gn = self.o, self.record
        out = self.fitter.gauss_newton_step(ncg=o.gauss_newton_cg_iters, lam=gn["lambda"], cg_tol=o.gauss_newton_cg_tol, **kw)
        ok = np.asarray(out["accepted"], dtype=bool)
        gn["lambda"] = np.where(todo, next_lambda(gn["lambda"], ok), gn["lambda"])
        gn["steps"] += todo
        gn["accepted"] += ok & todo
        for t in np.where(todo)[0]:
            gn["loss"][t].append(float(out["loss_after"][t] if ok[t] else out["loss_before"][t]))
            gn["cg_iters"][t].append(int(out["cg_iters"][t]))

    def start(self):
        for _ in range(self.o.gauss_newton_rounds):
            self._step(np.ones(self.nl, dtype=bool))

    def gap(self, running):
        if self.o.gauss_newton_every > 0:
            self._step(running, slice_mask=running, reset_moments=True)

    entry = staticmethod(newton_history)


class _Lbfgs(_Action):
    """``lbfgs_steps`` / ``lbfgs_every``: per loop the calls, iterations and evaluations, the loss after every call, its last status."""
    name = "lbfgs"

    def __init__(self, fitter, o, nl, freeze_model):
        self.fitter, self.o, self.nl, self.freeze_model = fitter, o, nl, freeze_model
        self.record = dict(calls=np.zeros(nl, dtype=np.int64), iters=np.zeros(nl, dtype=np.int64), evals=np.zeros(nl, dtype=np.int64),
                           loss=[[] for _ in range(nl)], status=np.full(nl, 4, dtype=np.int64))

    def _call(self, todo, **kw):
        o, lb = self.o, self.record
        out = self.fitter.lbfgs(o.lbfgs_steps, history=o.lbfgs_history, max_ls=o.lbfgs_max_ls, ftol=o.lbfgs_ftol, freeze_model=self.freeze_model, **kw)
        lb["calls"] += todo
        lb["iters"] += np.where(todo, out["iters"], 0)
        lb["evals"] += np.where(todo, out["evals"], 0)
        lb["status"] = np.where(todo, out["status"], lb["status"])
        for t in np.where(todo)[0]:
            lb["loss"][t].append(float(out["loss_after"][t]))

    def start(self):
        if self.o.lbfgs_steps > 0:
            self._call(np.ones(self.nl, dtype=bool))

    def gap(self, running):
        if self.o.lbfgs_every > 0:
            self._call(running, slice_mask=running, reset_moments=True)

    entry = staticmethod(lbfgs_history)


@dataclasses.dataclass
class FitResult:
    """What ``drive`` returns.  ``loops``: per loop ``(losses, stopped, nupdates)``; ``nsingular``, ``sweep_singular``: the singular count
    of the last coefficient solve and of the last sweep of a basis or time family; ``robust``: what the last reweight of every loop
    reported, ``{"rounds": [nl], "ndown_bl", "scale_bl": [nl * rows_per_loop]}``; ``newton``: ``{"steps", "accepted": [nl], "lambda": [nl]
    (the damping a next step would use), "loss", "cg_iters": per loop the loss after and the iterations of every step it took part in}``;
    ``lbfgs``: ``{"calls", "iters", "evals": [nl], "loss": per loop the loss after every call it took part in, "status": [nl] of its last
    call}``.  ``None`` where the fit has no such thing."""
    loops: list
    nsingular: object = None
    sweep_singular: object = None
    robust: object = None
    newton: object = None
    lbfgs: object = None


def drive(fitter, controls, nl, rows_per_loop, maxsteps, tol, use_min, freeze_model, n_profile_steps=0, profile_log_dir="./logdir",
          profile_extra=None):
    """Everything between ``set_optimizer`` and reading the parameters back, on a ``SliceBatchFitter`` or a one-slice
    ``HipFitSolver``, as ``controls`` (``FitControls``) say: the start-up work of the actions (the rounds of closed-form solves, the
    Gauss-Newton rounds, the L-BFGS iterations), ``n_profile_steps`` profiled steps (their timings, with the keys of ``profile_extra``,
    as JSON into ``profile_log_dir``), the unrecorded step, the recorded loop -- with a chunk length (``controls.chunk``) in chunks,
    with the actions' gap work between them (the reweighting, the coefficient solve and the sweeps, one Gauss-Newton step, the L-BFGS
    iterations) on the loops not yet over and with the optimizer's slots of the loops that moved started over.  ``nl``: the loops of
    the fitter (1 for a single solver and for a joint fit, else the slices of the batch), ``rows_per_loop``: the baseline rows of each.
    An action that is switched off is not in the list and makes no call.  Returns a ``FitResult``."""
    o = controls.fit
    actions = [_Reweight(fitter, o, nl, rows_per_loop) if o.robust_every > 0 else None,
               _ClosedForm(fitter, o) if o.coeff_solve_rounds > 0 or o.family is not None else None,
               _GaussNewton(fitter, controls.newton, nl) if controls.newton.on else None,
               _Lbfgs(fitter, controls.lbfgs, nl, freeze_model) if controls.lbfgs.on else None]
    actions = [a for a in actions if a is not None]
    for action in actions:
        action.start()
    if n_profile_steps > 0:
        fitter.timing_enable(True)
        fitter.run_slices(n_profile_steps, record=False, freeze_model=freeze_model)
        os.makedirs(profile_log_dir, exist_ok=True)
        with open(os.path.join(profile_log_dir, f"calamity_amd_profile_{datetime.datetime.now():%Y%m%d_%H%M%S_%f}.json"), "w") as f:
            json.dump(dict(n_profile_steps=n_profile_steps, **(profile_extra or {}), fused_basis_kernel=fitter.timing_get()), f)
        fitter.timing_enable(False)
    fitter.run_slices(1, record=False, freeze_model=freeze_model)  # the unrecorded step of calibration.py:693
    run = dict(record=True, tol=tol, use_min=use_min, freeze_model=freeze_model)
    chunk = controls.chunk
    if chunk > 0:
        # the recorded loop in chunks (every loop's state -- step count, previous and lowest loss -- persists from run to run); a loop
        # that has ended is held in the chunks that follow, as one call would leave it, and takes no part in the gaps between them
        parts, over, nupd, issued = [[] for _ in range(nl)], np.zeros(nl, dtype=bool), np.zeros(nl, dtype=np.int64), 0
        while issued < maxsteps and not np.all(over):
            n = min(chunk, maxsteps - issued)
            for t, (part, stopped, nu) in enumerate(fitter.run_slices(n, **run)):
                if not over[t]:
                    parts[t].append(part)
                    nupd[t] += nu
                    over[t] = stopped or len(part) < n
            issued += n
            if issued < maxsteps and not np.all(over):
                fitter.hold_slices(over)
                for action in actions:
                    action.gap(~over)
        fitter.hold_slices(None)
        loops = [(np.concatenate([np.zeros(0)] + parts[t]), bool(over[t]), int(nupd[t])) for t in range(nl)]
    else:
        loops = fitter.run_slices(maxsteps, **run)
    return FitResult(loops, **{k: v for action in actions for k, v in action.fields().items()})


def history_entry(controls, result, t, dtype, robust=None):
    """Loop ``t`` of a ``FitResult`` as one slice's ``fit_history`` entry.  ``robust``: the reweighting as the caller reports it, where
    that is not loop ``t`` in solver units and row order."""
    hist = {"loss": [dtype.type(l) for l in result.loops[t][0]]}
    if result.nsingular is not None:
        hist["coeff_solve_singular"] = int(result.nsingular)
    if result.sweep_singular is not None:
        hist[_FAMILIES[controls.fit.family][0] + "_singular"] = int(result.sweep_singular)
    if result.robust is not None:
        hist["robust"] = _Reweight.entry(result.robust, t) if robust is None else robust
    if result.newton is not None:
        hist["gauss_newton"] = _GaussNewton.entry(result.newton, t)
    if result.lbfgs is not None:
        hist["lbfgs"] = _Lbfgs.entry(result.lbfgs, t)
    return hist
