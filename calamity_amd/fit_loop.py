"""The host loop of a fit, stated once: ``FitOptions`` holds the keywords of the closed-form solves and of the robust reweighting,
``GaussNewtonOptions`` those of the joint Gauss-Newton steps, ``LbfgsOptions`` those of the L-BFGS iterations, ``drive`` issues everything between ``set_optimizer`` and reading the parameters back, ``history_entry`` files what it returns.
Host only: NumPy, never the library ("The host loop")."""
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


@dataclasses.dataclass(frozen=True)
class FitOptions:
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

    @classmethod
    def pick(cls, keywords):
        """The options out of a mapping that holds them among others (a public function's ``locals()``)."""
        return cls(**{f.name: keywords[f.name] for f in dataclasses.fields(cls)})

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
        for other in (self.gain_solve_every, self.gain_basis_solve_every, self.gain_time_solve_every):
            if other and other != every:
                raise ValueError(f"robust_every={every} and the closed-form sweeps' chunk length {other} (gain_solve_every / gain_basis_solve_every / "
                                 "gain_time_solve_every) share the gaps of one chunked loop: give them the same value")

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
class GaussNewtonOptions:
    """The keywords of the joint Gauss-Newton steps of ``calibrate_and_model_tensor`` / ``fit_gains_and_foregrounds`` (documented
    there), under their public names and defaults."""
    gauss_newton_rounds: int = 0
    gauss_newton_every: int = 0
    gauss_newton_cg_iters: int = 20
    gauss_newton_lambda: float = 1e-3
    gauss_newton_cg_tol: float = 1e-3

    @classmethod
    def pick(cls, keywords):
        """The options out of a mapping that holds them among others (a public function's ``locals()``)."""
        return cls(**{f.name: keywords[f.name] for f in dataclasses.fields(cls)})

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
        if every and opts.chunk and opts.chunk != every:
            raise ValueError(f"gauss_newton_every={every} and the chunk length {opts.chunk} of gain_solve_every / gain_basis_solve_every / "
                             "gain_time_solve_every / robust_every share the gaps of one chunked loop: give them the same value")


@dataclasses.dataclass(frozen=True)
class LbfgsOptions:
    """The keywords of the L-BFGS iterations of ``calibrate_and_model_tensor`` / ``fit_gains_and_foregrounds`` (documented there),
    under their public names and defaults."""
    lbfgs_steps: int = 0
    lbfgs_every: int = 0
    lbfgs_history: int = 8
    lbfgs_max_ls: int = 20
    lbfgs_ftol: float = 0.0

    @classmethod
    def pick(cls, keywords):
        """The options out of a mapping that holds them among others (a public function's ``locals()``)."""
        return cls(**{f.name: keywords[f.name] for f in dataclasses.fields(cls)})

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
        others = [opts.chunk] + ([newton.gauss_newton_every] if newton is not None and newton.on else [])
        for other in others:
            if every and other and other != every:
                raise ValueError(f"lbfgs_every={every} and the chunk length {other} of gain_solve_every / gain_basis_solve_every / "
                                 "gain_time_solve_every / robust_every / gauss_newton_every share the gaps of one chunked loop: give them the same value")


def next_lambda(lam, accepted):
    """The damping after a step: a tenth where the step was accepted, ten times ``max(lambda, 1e-6)`` where it was rejected."""
    lam = np.asarray(lam, dtype=np.float64)
    return np.where(np.asarray(accepted, dtype=bool), lam / 10.0, 10.0 * np.maximum(lam, 1e-6))


def drive(fitter, opts, nl, rows_per_loop, maxsteps, tol, use_min, freeze_model, n_profile_steps=0, profile_log_dir="./logdir",
          profile_extra=None, newton=None, lbfgs=None):
    """Everything between ``set_optimizer`` and reading the parameters back, on a ``SliceBatchFitter`` or a one-slice
    ``HipFitSolver``: the start-up rounds of closed-form solves, ``n_profile_steps`` profiled steps (their timings, with the keys of
    ``profile_extra``, as JSON into ``profile_log_dir``), the unrecorded step, the recorded loop.  ``nl``: the loops of the fitter (1 for
    a single solver and for a joint fit, else the slices of the batch), ``rows_per_loop``: the baseline rows of each.  Returns
    ``(results, nsingular, sweep_singular, robust)``: per loop ``(losses, stopped, nupdates)``; the singular count of the last
    coefficient solve and of the last sweep of a basis or time family (``None`` where there is none); with ``robust_every`` what the
    last reweight of every loop reported, ``{"rounds": [nl], "ndown_bl", "scale_bl": [nl * rows_per_loop]}``, else ``None``.
    ``newton`` (``GaussNewtonOptions``): ``gauss_newton_rounds`` joint steps after the start-up rounds and sweeps, and with
    ``gauss_newton_every`` one step in every gap of the chunked loop behind the reweighting, the coefficient solve and the sweeps, on the
    loops not yet over and with the optimizer's slots of the accepted ones started over.  The damping is kept per loop (``next_lambda``);
    a rejected step is simply followed by the next one.  With ``newton`` given a fifth value is returned: ``None`` while it is off,
    else ``{"steps", "accepted": [nl], "lambda": [nl] (the damping a next step would use), "loss", "cg_iters": per loop the loss after and the
    iterations of every step it took part in}``.
    ``lbfgs`` (``LbfgsOptions``): ``lbfgs_steps`` iterations of L-BFGS after the start-up rounds and the Gauss-Newton rounds, before the
    profiled and unrecorded steps, and with ``lbfgs_every`` as many again last in every gap of the chunked loop, on the loops not yet
    over and with the optimizer's slots of the loops that moved started over.  With ``lbfgs`` given one more value is appended: ``None``
    while it is off, else ``{"calls", "iters", "evals": [nl], "loss": per loop the loss after every call it took part in, "status":
    [nl] of its last call}``."""
    family = opts.family
    sweeps, every, damping, ridge = opts.sweep

    def sweep(n, **kw):
        if family == "time":  # one system over the times: no slice mask
            kw.pop("slice_mask", None)
        if family != "gain":
            kw["ridge"] = ridge
        out = getattr(fitter, _FAMILIES[family][1])(n, damping=damping, **kw)
        return None if family == "gain" else out["nsingular"]

    nsingular = last = None
    if opts.coeff_solve_rounds > 0:  # alternating least squares: rounds of (the coefficients in closed form, then the gain sweeps)
        for _ in range(opts.coeff_solve_rounds):
            nsingular = fitter.solve_coeffs(ridge=opts.coeff_solve_ridge)["nsingular"]
            if sweeps > 0:
                last = sweep(sweeps)
    elif sweeps > 0:  # the coefficients are initialised: the gains in closed form before any descent step
        last = sweep(sweeps)
    gn = None
    if newton is not None and newton.on:
        gn = dict(steps=np.zeros(nl, dtype=np.int64), accepted=np.zeros(nl, dtype=np.int64), loss=[[] for _ in range(nl)],
                  cg_iters=[[] for _ in range(nl)])
        gn["lambda"] = np.full(nl, float(newton.gauss_newton_lambda))

    def newton_step(todo, **kw):
        out = fitter.gauss_newton_step(ncg=newton.gauss_newton_cg_iters, lam=gn["lambda"], cg_tol=newton.gauss_newton_cg_tol, **kw)
        ok = np.asarray(out["accepted"], dtype=bool)
        gn["lambda"] = np.where(todo, next_lambda(gn["lambda"], ok), gn["lambda"])
        gn["steps"] += todo
        gn["accepted"] += ok & todo
        for t in np.where(todo)[0]:
            gn["loss"][t].append(float(out["loss_after"][t] if ok[t] else out["loss_before"][t]))
            gn["cg_iters"][t].append(int(out["cg_iters"][t]))

    if gn is not None:
        for _ in range(newton.gauss_newton_rounds):
            newton_step(np.ones(nl, dtype=bool))
    lb = None
    if lbfgs is not None and lbfgs.on:
        lb = dict(calls=np.zeros(nl, dtype=np.int64), iters=np.zeros(nl, dtype=np.int64), evals=np.zeros(nl, dtype=np.int64),
                  loss=[[] for _ in range(nl)], status=np.full(nl, 4, dtype=np.int64))

    def lbfgs_call(todo, **kw):
        out = fitter.lbfgs(lbfgs.lbfgs_steps, history=lbfgs.lbfgs_history, max_ls=lbfgs.lbfgs_max_ls, ftol=lbfgs.lbfgs_ftol,
                           freeze_model=freeze_model, **kw)
        lb["calls"] += todo
        lb["iters"] += np.where(todo, out["iters"], 0)
        lb["evals"] += np.where(todo, out["evals"], 0)
        lb["status"] = np.where(todo, out["status"], lb["status"])
        for t in np.where(todo)[0]:
            lb["loss"][t].append(float(out["loss_after"][t]))

    if lb is not None and lbfgs.lbfgs_steps > 0:
        lbfgs_call(np.ones(nl, dtype=bool))
    if n_profile_steps > 0:
        fitter.timing_enable(True)
        fitter.run_slices(n_profile_steps, record=False, freeze_model=freeze_model)
        os.makedirs(profile_log_dir, exist_ok=True)
        with open(os.path.join(profile_log_dir, f"calamity_amd_profile_{datetime.datetime.now():%Y%m%d_%H%M%S_%f}.json"), "w") as f:
            json.dump(dict(n_profile_steps=n_profile_steps, **(profile_extra or {}), fused_basis_kernel=fitter.timing_get()), f)
        fitter.timing_enable(False)
    fitter.run_slices(1, record=False, freeze_model=freeze_model)  # the unrecorded step of calibration.py:693
    run = dict(record=True, tol=tol, use_min=use_min, freeze_model=freeze_model)
    robust = None
    if opts.robust_every > 0:  # per loop the reweights it took part in; per baseline row what its last one reported
        robust = dict(rounds=np.zeros(nl, dtype=np.int64), ndown_bl=np.zeros(nl * rows_per_loop), scale_bl=np.zeros(nl * rows_per_loop))
    chunk = opts.chunk or (newton.gauss_newton_every if gn is not None else 0) or (lbfgs.lbfgs_every if lb is not None else 0)
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
                if robust is not None:
                    todo = ~over if opts.robust_rounds == 0 else ~over & (robust["rounds"] < opts.robust_rounds)
                    if np.any(todo):
                        rw = fitter.robust_weights(kind=opts.robust_kind, threshold=opts.robust_threshold, slice_mask=todo)
                        rows = np.repeat(todo, rows_per_loop)
                        robust["ndown_bl"][rows] = rw["ndown_bl"][rows]
                        robust["scale_bl"][rows] = rw["scale_bl"][rows]
                        robust["rounds"] += todo
                if every > 0:
                    if opts.coeff_solve_rounds > 0:
                        nsingular = fitter.solve_coeffs(ridge=opts.coeff_solve_ridge, slice_mask=~over, reset_coeff_moments=True)["nsingular"]
                    last = sweep(max(1, sweeps), slice_mask=~over, reset_gain_moments=True)
                if gn is not None and newton.gauss_newton_every > 0:
                    newton_step(~over, slice_mask=~over, reset_moments=True)
                if lb is not None and lbfgs.lbfgs_every > 0:
                    lbfgs_call(~over, slice_mask=~over, reset_moments=True)
        fitter.hold_slices(None)
        results = [(np.concatenate([np.zeros(0)] + parts[t]), bool(over[t]), int(nupd[t])) for t in range(nl)]
    else:
        results = fitter.run_slices(maxsteps, **run)
    out = (results, nsingular, (int(last or 0) if family in ("basis", "time") else None), robust)
    if newton is not None:
        out = out + (gn,)
    return out if lbfgs is None else out + (lb,)


def newton_history(gn, t):
    """Loop ``t``'s ``fit_history[...]["gauss_newton"]`` from the fifth value of ``drive`` (``None`` while the steps are off)."""
    if gn is None:
        return None
    return {"steps": int(gn["steps"][t]), "accepted": int(gn["accepted"][t]), "lambda": float(gn["lambda"][t]), "loss": list(gn["loss"][t]),
            "cg_iters": list(gn["cg_iters"][t])}


def lbfgs_history(lb, t):
    """Loop ``t``'s ``fit_history[...]["lbfgs"]`` from the value ``drive`` appends for ``lbfgs=`` (``None`` while the iterations are off)."""
    if lb is None:
        return None
    return {"calls": int(lb["calls"][t]), "iters": int(lb["iters"][t]), "evals": int(lb["evals"][t]), "loss": list(lb["loss"][t]),
            "status": int(lb["status"][t])}


def history_entry(opts, losses, dtype, nsingular, sweep_singular, robust, newton=None, lbfgs=None):
    """One slice's ``fit_history`` entry from what ``drive`` returned for it (``robust``, ``newton``, ``lbfgs``: the entries as the caller
    reports them, ``newton_history`` and ``lbfgs_history`` for the latter two)."""
    hist = {"loss": [dtype.type(l) for l in losses]}
    if nsingular is not None:
        hist["coeff_solve_singular"] = int(nsingular)
    if sweep_singular is not None:
        hist[_FAMILIES[opts.family][0] + "_singular"] = int(sweep_singular)
    if robust is not None:
        hist["robust"] = robust
    if newton is not None:
        hist["gauss_newton"] = newton
    if lbfgs is not None:
        hist["lbfgs"] = lbfgs
    return hist
