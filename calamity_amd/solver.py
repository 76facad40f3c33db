"""Thin object wrapper over the C-ABI handle (include/calamity_hip.h).  NumPy in, NumPy out."""
import ctypes as C

import numpy as np

from . import _lib
from .problem import FitProblem

# OPTIMIZERS of /root/reference/calamity/calibration.py:17-27 -- the whole table, "LAMB" being tensorflow_addons.optimizers.LAMB;
# any other name raises KeyError exactly like ``OPTIMIZERS[optimizer]`` at
# calibration.py:571.  Constructor arguments and defaults are those of tf.keras.optimizers.* (OptimizerV2, TF 2.4 - 2.10);
# an argument the optimizer does not take raises TypeError, as the Keras constructor would.
OPTIMIZERS = {"Adam": _lib.CAL_OPT_ADAM, "Adamax": _lib.CAL_OPT_ADAMAX, "SGD": _lib.CAL_OPT_SGD, "RMSprop": _lib.CAL_OPT_RMSPROP,
              "Adagrad": _lib.CAL_OPT_ADAGRAD, "Nadam": _lib.CAL_OPT_NADAM, "Adadelta": _lib.CAL_OPT_ADADELTA, "Ftrl": _lib.CAL_OPT_FTRL, "LAMB": _lib.CAL_OPT_LAMB}
_MOMENTS = dict(learning_rate=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7)
_OPT_DEFAULTS = {
    "Adam": _MOMENTS,
    "Adamax": _MOMENTS,
    "Nadam": _MOMENTS,
    "SGD": dict(learning_rate=1e-2, momentum=0.0, nesterov=False),
    "RMSprop": dict(learning_rate=1e-3, rho=0.9, momentum=0.0, epsilon=1e-7),
    "Adagrad": dict(learning_rate=1e-3, initial_accumulator_value=0.1, epsilon=1e-7),
    "Adadelta": dict(learning_rate=1e-3, rho=0.95, epsilon=1e-7),
    "Ftrl": dict(learning_rate=1e-3, learning_rate_power=-0.5, initial_accumulator_value=0.1, l1_regularization_strength=0.0,
                 l2_regularization_strength=0.0, l2_shrinkage_regularization_strength=0.0, beta=0.0),
    "LAMB": dict(learning_rate=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-6, weight_decay_rate=0.0),
}


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def problem_desc(prob, dtype, layout="stream", kernel_path="auto"):
    """``(_lib.ProblemDesc, arrays)`` of ``prob`` for a solver of ``dtype``: what ``cal_solver_set_problem`` and the host-only
    ``cal_debug_plan`` take.  The descriptor points into ``arrays``: keep them alive while it is in use."""
    dtype = np.dtype(dtype)
    basis = [np.ascontiguousarray(b, dtype=dtype) for b in prob.basis]
    sizes = np.asarray([b.size for b in basis], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    flat = np.concatenate([b.ravel() for b in basis]) if len(basis) > 1 else basis[0].ravel()
    nvec = np.asarray([b.shape[1] for b in basis], dtype=np.int32)
    nrb = np.asarray([b.shape[0] // prob.nfreqs for b in basis], dtype=np.int32)
    keep = [
        flat, offs, nvec, nrb,
        np.ascontiguousarray(prob.grp_basis, dtype=np.int32),
        np.ascontiguousarray(prob.grp_bl_start, dtype=np.int32),
        np.ascontiguousarray(prob.bl_ant0, dtype=np.int32),
        np.ascontiguousarray(prob.bl_ant1, dtype=np.int32),
        np.ascontiguousarray(prob.bl_rowblk, dtype=np.int32),
        None if getattr(prob, "bl_alias", None) is None else np.ascontiguousarray(prob.bl_alias, dtype=np.int32),
        # the reference's variables fg_r[chunk] / fg_i[chunk] (a layer-wise optimizer -- LAMB -- takes one trust ratio per variable)
        None if getattr(prob, "chunk_of_grp", None) is None else np.ascontiguousarray(prob.chunk_of_grp, dtype=np.int32),
    ]
    d = _lib.ProblemDesc(
        nants=prob.nants, nfreqs=prob.nfreqs, ngrps=prob.ngrps, nbls=prob.nbls, nbasis=len(basis),
        basis_offset=_ptr(offs), basis_nvec=_ptr(nvec), basis_nrowblk=_ptr(nrb), basis_data=_ptr(flat),
        grp_basis=_ptr(keep[4]), grp_bl_start=_ptr(keep[5]), bl_ant0=_ptr(keep[6]), bl_ant1=_ptr(keep[7]),
        bl_rowblk=_ptr(keep[8]), bl_alias=_ptr(keep[9]), nslices=int(getattr(prob, "nslices", 1) or 1), grp_var=_ptr(keep[10]),
        layout={"stream": _lib.CAL_LAYOUT_STREAM, "shared": _lib.CAL_LAYOUT_SHARED}[layout],
        kernel_path={"auto": _lib.CAL_PATH_AUTO, "general": _lib.CAL_PATH_GENERAL, "dense": _lib.CAL_PATH_DENSE,
                     "dense_f32": _lib.CAL_PATH_DENSE_F32, "dense_split1": _lib.CAL_PATH_DENSE_SPLIT1,
                     "general_full": _lib.CAL_PATH_GENERAL_FULL}[kernel_path],
    )
    return d, keep


class HipFitSolver:
    """One gain + foreground fit resident on one MI355X."""

    def __init__(self, dtype=np.float32, device=0):
        self._lib = _lib.load()
        self.dtype = np.dtype(dtype)
        if self.dtype == np.float32:
            code = _lib.CAL_F32
        elif self.dtype == np.float64:
            code = _lib.CAL_F64
        else:
            raise ValueError(f"dtype must be float32 or float64, got {dtype}")
        self._h = C.c_void_p()
        _lib.check(self._lib.cal_solver_create(C.byref(self._h), int(device), code))
        self.problem = None

    def close(self):
        if getattr(self, "_h", None):
            self._lib.cal_solver_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _real(self, a, shape=None):
        a = np.ascontiguousarray(a, dtype=self.dtype)
        if shape is not None and a.shape != tuple(shape):
            raise ValueError(f"expected shape {tuple(shape)}, got {a.shape}")
        return a

    # ---- problem -------------------------------------------------------------------------------------------
    def set_problem(self, prob: FitProblem, layout="stream", kernel_path="auto"):
        """``kernel_path``: "auto" (dense matrix-core kernel when eligible and large enough), "general", "dense", or
        "dense_f32" (fp32: the v_mfma_f32_32x32x2_f32 kernel the split-bf16 one replaced).  In the "stream" layout "auto" and
        "general" keep only the lower half band of a mirror-symmetric basis (``timing_get()["basis_folded"]``);
        "general_full" is "general" with the full band kept whatever the basis looks like."""
        prob.validate()
        d, _keep = problem_desc(prob, self.dtype, layout, kernel_path)
        _lib.check(self._lib.cal_solver_set_problem(self._h, C.byref(d)))
        self.problem = prob
        self.nants, self.nfreqs, self.nbls, self.ncoeffs = prob.nants, prob.nfreqs, prob.nbls, prob.ncoeffs
        self.nslices = int(getattr(prob, "nslices", 1) or 1)
        self.gain_nvec = 0  # a new problem fits per channel until set_gain_basis
        self.gain_time_shape = None  # ... and per time until set_gain_time_basis: (ntimes, nvec_t)
        if prob.data_r is not None:
            self.set_data(prob.data_r, prob.data_i, prob.wgts)
        return self

    def set_data(self, data_r, data_i, wgts):
        shp = (self.nbls, self.nfreqs)
        a, b, c = self._real(data_r, shp), self._real(data_i, shp), self._real(wgts, shp)
        _lib.check(self._lib.cal_solver_set_data(self._h, _ptr(a), _ptr(b), _ptr(c)))

    def set_regularization(self, mode=None, prior_r_sum=0.0, prior_i_sum=0.0):
        """``prior_*_sum``: one number, or one per time slice of the solver (cal_solver_set_regularization_slices)."""
        code = _lib.CAL_REG_SUM if mode == "sum" else _lib.CAL_REG_NONE
        if np.ndim(prior_r_sum) == 0:
            _lib.check(self._lib.cal_solver_set_regularization(self._h, code, float(prior_r_sum), float(prior_i_sum)))
            return
        pr = np.ascontiguousarray(prior_r_sum, dtype=np.float64)
        pi = np.ascontiguousarray(prior_i_sum, dtype=np.float64)
        if pr.shape != (self.nslices,) or pi.shape != (self.nslices,):
            raise ValueError(f"expected {self.nslices} priors per component")
        _lib.check(self._lib.cal_solver_set_regularization_slices(self._h, code, _ptr(pr), _ptr(pi)))

    def set_optimizer(self, optimizer="Adamax", **opt_kwargs):
        opt_id = OPTIMIZERS[optimizer]  # KeyError for anything else, like calibration.py:571
        defaults = _OPT_DEFAULTS[optimizer]
        unknown = set(opt_kwargs) - set(defaults)
        if unknown:
            raise TypeError(f"Unexpected keyword argument(s) passed to optimizer: {sorted(unknown)}")
        kw = dict(defaults, **opt_kwargs)
        d = _lib.OptimizerDesc(opt_id, kw["learning_rate"], kw.get("beta_1", 0.9), kw.get("beta_2", 0.999), kw.get("epsilon", 1e-7),
                               kw.get("rho", 0.9), kw.get("momentum", 0.0), kw.get("initial_accumulator_value", 0.1),
                               int(bool(kw.get("nesterov", False))), 0, kw.get("learning_rate_power", -0.5),
                               kw.get("l1_regularization_strength", 0.0), kw.get("l2_regularization_strength", 0.0),
                               kw.get("l2_shrinkage_regularization_strength", 0.0), kw.get("beta", 0.0), kw.get("weight_decay_rate", 0.0))
        if optimizer == "Ftrl" and (kw["learning_rate_power"] > 0.0 or kw["initial_accumulator_value"] < 0.0):
            raise ValueError("Ftrl: learning_rate_power must be <= 0 and initial_accumulator_value >= 0 (as the Keras constructor checks)")
        _lib.check(self._lib.cal_solver_set_optimizer(self._h, C.byref(d)))

    # ---- parameters ----------------------------------------------------------------------------------------
    def set_params(self, g_r=None, g_i=None, c_r=None, c_i=None):
        gs, cs = (self.nants, self.nfreqs), (self.ncoeffs,)
        arrs = [None if a is None else self._real(a, s) for a, s in ((g_r, gs), (g_i, gs), (c_r, cs), (c_i, cs))]
        _lib.check(self._lib.cal_solver_set_params(self._h, *[_ptr(a) for a in arrs]))

    def get_params(self, which=0):
        g_r = np.empty((self.nants, self.nfreqs), dtype=self.dtype)
        g_i = np.empty_like(g_r)
        c_r = np.empty(self.ncoeffs, dtype=self.dtype)
        c_i = np.empty_like(c_r)
        _lib.check(self._lib.cal_solver_get_params(self._h, int(which), _ptr(g_r), _ptr(g_i), _ptr(c_r), _ptr(c_i)))
        return g_r, g_i, c_r, c_i

    # ---- gain basis ----------------------------------------------------------------------------------------
    def set_gain_basis(self, basis):
        """Confine the fit's correction to the gains to span(B): ``g = g0 + B y`` with ``basis`` real ``[nfreqs, K]`` shared by
        every antenna (and time slice), ``g0`` the gains the solver holds at this call (or is given later by ``set_params``),
        ``y`` the optimizer's variables (zero at the start).  Call after ``set_problem``; moments and iteration count start
        over as after ``set_optimizer``.  ``None`` detaches the basis: the fit is per channel again."""
        if basis is None:
            _lib.check(self._lib.cal_solver_set_gain_basis(self._h, None, 0))
            self.gain_nvec = 0
            return
        b = np.asarray(basis)
        if np.iscomplexobj(b):
            raise ValueError("the gain basis must be real")
        if b.ndim != 2 or b.shape[0] != self.nfreqs or b.shape[1] < 1:
            raise ValueError(f"expected a gain basis of shape ({self.nfreqs}, K >= 1), got {b.shape}")
        b = np.ascontiguousarray(b, dtype=self.dtype)
        _lib.check(self._lib.cal_solver_set_gain_basis(self._h, _ptr(b), int(b.shape[1])))
        self.gain_nvec = int(b.shape[1])

    def set_gain_time_basis(self, basis_t):
        """Fit gains that are smooth in time.  The solver holds ``T`` times as one fit (``distributed.batch_time_slices(parts,
        per_slice=False)``: ``nants = T * Na``, antenna ``a`` at time ``t`` is row ``t * Na + a``) and
        ``g[t * Na + a] = g0[t * Na + a] + sum_l Bt[t, l] z[a, l]`` with ``basis_t`` real ``[T, L]``, ``1 <= L <= T``; ``z[a, l]`` is
        ``B y[a, l]`` when a frequency basis is set as well (``set_gain_basis``, in either order) and ``y[a, l]`` itself without
        one.  ``g0`` are the gains the solver holds at this call (or is given later by ``set_params``), ``y`` starts at zero, moments
        and iteration count start over.  ``None`` detaches the time basis alone."""
        if basis_t is None:
            _lib.check(self._lib.cal_solver_set_gain_time_basis(self._h, None, 0, 0))
            self.gain_time_shape = None
            return
        b = np.asarray(basis_t)
        if np.iscomplexobj(b):
            raise ValueError("the gain time basis must be real")
        if b.ndim != 2 or b.shape[0] < 1 or b.shape[1] < 1:
            raise ValueError(f"expected a gain time basis of shape (T >= 1, 1 <= L <= T), got {b.shape}")
        b = np.ascontiguousarray(b, dtype=self.dtype)
        _lib.check(self._lib.cal_solver_set_gain_time_basis(self._h, _ptr(b), int(b.shape[0]), int(b.shape[1])))
        self.gain_time_shape = (int(b.shape[0]), int(b.shape[1]))

    def _gain_coeff_shape(self):
        k = int(getattr(self, "gain_nvec", 0))
        tshape = getattr(self, "gain_time_shape", None)
        if tshape is None:
            return (self.nants, k)
        return (self.nants // tshape[0], tshape[1], k if k else self.nfreqs)

    def get_gain_coeffs(self, which=0):
        """The coefficients ``y`` of the gain basis, ``(y_r, y_i)`` of shape ``[nants, K]`` (``which`` as in ``get_params``); while a
        time basis is set ``[Na, L, K]``, or ``[Na, L, nfreqs]`` without a frequency basis."""
        y_r = np.empty(self._gain_coeff_shape(), dtype=self.dtype)
        y_i = np.empty_like(y_r)
        _lib.check(self._lib.cal_solver_get_gain_coeffs(self._h, int(which), _ptr(y_r), _ptr(y_i)))
        return y_r, y_i

    def get_gain_coeff_moments(self):
        """The optimizer's slots of a fit with a gain basis, read only (``get_moments`` / ``set_moments`` stay refused there):
        ``ym_*``, ``yv_*`` in the shape of ``get_gain_coeffs``, ``cm_*``, ``cv_*`` ``[ncoeffs]`` and ``t`` ``[nslices]``, every slice's own
        count of applied updates."""
        y = [np.empty(self._gain_coeff_shape(), dtype=self.dtype) for _ in range(4)]
        c = [np.empty(self.ncoeffs, dtype=self.dtype) for _ in range(4)]
        t = np.zeros(self.nslices, dtype=np.int64)
        _lib.check(self._lib.cal_solver_get_gain_coeff_moments(self._h, *[_ptr(a) for a in y + c], t.ctypes.data_as(C.POINTER(C.c_int64))))
        return dict(ym_r=y[0], ym_i=y[1], yv_r=y[2], yv_i=y[3], cm_r=c[0], cm_i=c[1], cv_r=c[2], cv_i=c[3], t=t)

    def eval_gain_coeff_grads(self):
        """Loss and its gradient with respect to ``y``: ``grad g @ B`` (contracted with ``Bt`` over the times while a time basis is
        set), ``(loss, gy_r, gy_i)`` in the shape of ``get_gain_coeffs``."""
        gy_r = np.empty(self._gain_coeff_shape(), dtype=self.dtype)
        gy_i = np.empty_like(gy_r)
        loss = C.c_double(0)
        _lib.check(self._lib.cal_solver_eval_gain_coeff_grads(self._h, C.byref(loss), _ptr(gy_r), _ptr(gy_i)))
        return loss.value, gy_r, gy_i

    def get_moments(self):
        g = [np.empty((self.nants, self.nfreqs), dtype=self.dtype) for _ in range(4)]
        c = [np.empty(self.ncoeffs, dtype=self.dtype) for _ in range(4)]
        t = C.c_int64(0)
        _lib.check(self._lib.cal_solver_get_moments(self._h, *[_ptr(a) for a in g + c], C.byref(t)))
        return dict(gm_r=g[0], gm_i=g[1], gv_r=g[2], gv_i=g[3], cm_r=c[0], cm_i=c[1], cv_r=c[2], cv_i=c[3], t=t.value)

    def set_moments(self, gm_r, gm_i, gv_r, gv_i, cm_r, cm_i, cv_r, cv_i, t):
        gs, cs = (self.nants, self.nfreqs), (self.ncoeffs,)
        arrs = [self._real(a, gs) for a in (gm_r, gm_i, gv_r, gv_i)] + [self._real(a, cs) for a in (cm_r, cm_i, cv_r, cv_i)]
        _lib.check(self._lib.cal_solver_set_moments(self._h, *[_ptr(a) for a in arrs], int(t)))

    # ---- compute -------------------------------------------------------------------------------------------
    def eval_loss(self):
        loss = C.c_double(0)
        _lib.check(self._lib.cal_solver_eval_loss(self._h, C.byref(loss)))
        return loss.value

    def slice_losses(self):
        """The loss of every time slice as of the last eval_loss / eval_grads."""
        out = np.zeros(self.nslices, dtype=np.float64)
        _lib.check(self._lib.cal_solver_get_slice_losses(self._h, _ptr(out)))
        return out

    def eval_grads(self):
        gg_r = np.empty((self.nants, self.nfreqs), dtype=self.dtype)
        gg_i = np.empty_like(gg_r)
        gc_r = np.empty(self.ncoeffs, dtype=self.dtype)
        gc_i = np.empty_like(gc_r)
        loss = C.c_double(0)
        _lib.check(self._lib.cal_solver_eval_grads(self._h, C.byref(loss), _ptr(gg_r), _ptr(gg_i), _ptr(gc_r), _ptr(gc_i)))
        return loss.value, gg_r, gg_i, gc_r, gc_i

    def run(self, nsteps, record=True, tol=1e-14, use_min=False, freeze_model=False):
        """``nsteps`` train steps at most.  Returns (recorded losses, stopped, nupdates)."""
        d = _lib.RunDesc(int(nsteps), int(bool(record)), int(bool(use_min)), int(bool(freeze_model)), float(tol))
        losses = np.zeros(max(int(nsteps), 1), dtype=np.float64)
        res = _lib.RunResult()
        _lib.check(self._lib.cal_solver_run(self._h, C.byref(d), _ptr(losses), C.byref(res)))
        return losses[: res.nrecorded], bool(res.stopped), res.nupdates

    def run_slices(self, nsteps, record=True, tol=1e-14, use_min=False, freeze_model=False):
        """The same loop for every time slice of the solver at once (cal_solver_run_slices): each slice records its own
        losses, applies the tolerance test and the use_min bookkeeping to its own loss and stops on its own.  Returns a
        list with one (recorded losses, stopped, nupdates) per slice.  A non-finite loss in any slice raises (code
        CAL_ERR_NONFINITE) after the others have finished."""
        d = _lib.RunDesc(int(nsteps), int(bool(record)), int(bool(use_min)), int(bool(freeze_model)), float(tol))
        losses = np.zeros((self.nslices, max(int(nsteps), 1)), dtype=np.float64)
        res = (_lib.RunResult * self.nslices)()
        _lib.check(self._lib.cal_solver_run_slices(self._h, C.byref(d), _ptr(losses), res))
        return [(losses[t, : res[t].nrecorded].copy(), bool(res[t].stopped), res[t].nupdates) for t in range(self.nslices)]

    def model(self):
        m_r = np.empty((self.nbls, self.nfreqs), dtype=self.dtype)
        m_i = np.empty_like(m_r)
        _lib.check(self._lib.cal_solver_model(self._h, _ptr(m_r), _ptr(m_i)))
        return m_r, m_i

    def data_model(self):
        """data_model (calibration.py:1593-1605): ``g_ant0 conj(g_ant1) (A c)`` of every baseline, ``[nbls, nfreqs]``."""
        m_r = np.empty((self.nbls, self.nfreqs), dtype=self.dtype)
        m_i = np.empty_like(m_r)
        _lib.check(self._lib.cal_solver_data_model(self._h, _ptr(m_r), _ptr(m_i)))
        return m_r, m_i

    def fit_quality(self, g_r=None, g_i=None):
        """Where the residual power sits (cal_solver_fit_quality), in solver units: with ``e = w |d - g_i conj(g_j) (A c)|^2``,
        ``chisq_bl``, ``wsum_bl`` ``[nbls]`` (sums of ``e`` and ``w`` over the channels) and ``chisq_ant``, ``wsum_ant``
        ``[nants, nfreqs]`` (sums over the baselines of each antenna), all float64.  ``g_r``, ``g_i`` ``[nants, nfreqs]``: gains to
        evaluate at for this call only; ``None``: the solver's current gains.  Under an exchange the antenna planes are summed over
        the ranks; the baseline arrays stay this rank's own."""
        if (g_r is None) != (g_i is None):
            raise ValueError("give both g_r and g_i, or neither")
        gs = (self.nants, self.nfreqs)
        a = None if g_r is None else self._real(g_r, gs)
        b = None if g_i is None else self._real(g_i, gs)
        out = dict(chisq_ant=np.empty(gs, dtype=np.float64), wsum_ant=np.empty(gs, dtype=np.float64),
                   chisq_bl=np.empty(self.nbls, dtype=np.float64), wsum_bl=np.empty(self.nbls, dtype=np.float64))
        _lib.check(self._lib.cal_solver_fit_quality(self._h, _ptr(a), _ptr(b), _ptr(out["chisq_ant"]), _ptr(out["wsum_ant"]),
                                                    _ptr(out["chisq_bl"]), _ptr(out["wsum_bl"])))
        return out

    def delay_spectrum(self, op, norm_f, what=("data", "model", "resid"), calibrated=False, bin_of_bl=None, nbins=0, per_baseline=False,
                       g_r=None, g_i=None):
        """Where the power of data, model and residual sits in delay (cal_solver_delay_spectrum), in solver units.  ``op``
        ``[nfreqs, ndelays]`` complex: the transform along frequency with the taper folded in (``modeling.delay_transform``, or any
        other linear spectral estimator); ``norm_f`` ``[nfreqs]``: what an unflagged channel adds to a row's normalisation (the
        taper squared).  With ``G = g_i conj(g_j)``, ``m = A c`` and ``mask = (w != 0)`` for the weights the solver holds now::

            x_q[b][f]  = mask q[b][f],   q = d, G m, d - G m        (calibrated: d / G, m, d / G - m, zero where |G|^2 == 0)
            X_q[b][k]  = sum_f x_q[b][f] op[f][k]                   (products in the solver's dtype, on the matrix cores)
            norm_bl[b] = sum_f mask norm_f[f]
            power      = |X_q[b][k]|^2 / norm_bl[b]                 0 where norm_bl[b] == 0

        ``what``: which of ``"data"``, ``"model"``, ``"resid"`` to form.  ``bin_of_bl`` ``[nbls]`` integers in ``[-1, nbins)`` (-1: the
        row is left out): the returned entry of each quantity asked for is then ``[nbins, ndelays]``, the SUM of the power over the
        bin's rows with ``norm_bl > 0`` in ascending row order, and ``"count_bin"`` ``[nbins]`` their number.  ``per_baseline=True``
        adds ``"per_baseline": {quantity: [nbls, ndelays]}`` (as large as the data: off by default).  ``"norm_bl"`` is always
        returned.  ``g_r``, ``g_i``: gains for this call only, as in ``fit_quality``.  All float64; sums in a fixed order: two calls
        give the same bits.  The parameters, moments, weights and loop state are untouched.  Under an exchange the binned arrays are
        summed over the ranks (one all-reduce); ``norm_bl`` and ``per_baseline`` stay this rank's own rows."""
        if (g_r is None) != (g_i is None):
            raise ValueError("give both g_r and g_i, or neither")
        what = (what,) if isinstance(what, str) else tuple(what)
        if not what or any(q not in _lib.DELAY_SPECTRUM_WHAT for q in what) or len(set(what)) != len(what):
            raise ValueError(f"what must name one or more of {sorted(_lib.DELAY_SPECTRUM_WHAT)} once each, got {what!r}")
        names = [q for q in ("data", "model", "resid") if q in what]  # the library's order
        op = np.asarray(op)
        if op.ndim != 2 or op.shape[0] != self.nfreqs:
            raise ValueError(f"op must be [nfreqs = {self.nfreqs}, ndelays], got shape {op.shape}")
        nd = op.shape[1]
        op_r, op_i = self._real(op.real), self._real(op.imag)
        norm_f = np.ascontiguousarray(norm_f, dtype=np.float64)
        if norm_f.shape != (self.nfreqs,):
            raise ValueError(f"norm_f must be [nfreqs = {self.nfreqs}], got shape {norm_f.shape}")
        nbins = int(nbins)
        if (bin_of_bl is None) != (nbins == 0):
            raise ValueError("give bin_of_bl and nbins > 0 together, or neither")
        bins = None
        if bin_of_bl is not None:
            bins = np.ascontiguousarray(bin_of_bl, dtype=np.int32)
            if bins.shape != (self.nbls,):
                raise ValueError(f"bin_of_bl must be [nbls = {self.nbls}], got shape {bins.shape}")
        gs = (self.nants, self.nfreqs)
        a = None if g_r is None else self._real(g_r, gs)
        b = None if g_i is None else self._real(g_i, gs)
        d = _lib.DelaySpectrumDesc(nd, sum(_lib.DELAY_SPECTRUM_WHAT[q] for q in names), int(bool(calibrated)), nbins,
                                   None if bins is None else bins.ctypes.data, op_r.ctypes.data, op_i.ctypes.data, norm_f.ctypes.data)
        norm_bl = np.empty(self.nbls, dtype=np.float64)
        p_bl = np.empty((len(names), self.nbls, nd), dtype=np.float64) if per_baseline else None
        p_bin = np.empty((len(names), nbins, nd), dtype=np.float64) if nbins else None
        c_bin = np.empty(nbins, dtype=np.float64) if nbins else None
        _lib.check(self._lib.cal_solver_delay_spectrum(self._h, C.byref(d), _ptr(a), _ptr(b), _ptr(p_bl), _ptr(norm_bl), _ptr(p_bin), _ptr(c_bin)))
        out = {"norm_bl": norm_bl}
        if nbins:
            out.update({q: p_bin[i] for i, q in enumerate(names)}, count_bin=c_bin)
        if per_baseline:
            out["per_baseline"] = {q: p_bl[i] for i, q in enumerate(names)}
        return out

    def fix_degeneracies(self, ref_r, ref_i, antpos, ref_w=None, mode="channel", iters=6, freqs=None, g_r=None, g_i=None, gref_r=None,
                         gref_i=None, return_gains=True, return_model=True):
        """Refer the fitted solution to a reference (sky) model (cal_solver_fix_degeneracies), in solver units.  The fit constrains
        only ``g_i conj(g_j) m_b``; per slice and channel an amplitude ``eta``, a phase ``psi`` and a tilt ``Phi`` (rad / m, east and
        north) are free.  ``ref_r``, ``ref_i`` ``[nbls, nfreqs]``: the reference visibilities ``s`` in the solver's row order;
        ``ref_w``: their weights (``None``: the weights the solver reads now); ``antpos`` ``[nants per slice, 2]``: east, north in
        metres, ``d_b = r_i - r_j``.  With ``m = A c`` and ``z0 = w conj(m) s`` (only ``w > 0`` counts)::

            Q = sum_b w |m|^2        H = sum_b |z0| d d^T        Phi = 0
            iters times:  q = sum_b Im(z0 e^{-i Phi.d}) d,   Phi += H^+ q         (a linear array: along H's dominant eigenvector)
            e^{2 eta} = max(sum_b Re(z0 e^{-i Phi.d}), 0) / Q
            psi = arg sum_a g_a e^{-i Phi.r_a} conj(gref_a)      over the antennas with an unflagged cross-correlation; 0 without gref
            model' = m e^{2 eta} e^{i Phi.d}        g' = g e^{-eta} e^{-i (Phi.r + psi)}

        so ``g'_i conj(g'_j) model'`` is what it was.  ``mode="band"``: one amplitude and one sky shift per slice,
        ``Phi(f) = (freqs[f] / mean(freqs)) Phi_0``.  ``g_r``, ``g_i``: gains for this call only, as in ``fit_quality``.  A channel
        without samples keeps the identity and reports 0 samples.  Returns ``eta``, ``psi``, ``nsamples``, ``last_step``
        ``[nslices, nfreqs]`` and ``tilt`` ``[nslices, nfreqs, 2]`` (float64; with a time basis the slices are its times),
        ``g_r``, ``g_i`` ``[nants, nfreqs]`` and ``model_r``, ``model_i`` ``[nbls, nfreqs]`` in the solver's dtype.  ``last_step``: the
        last update of ``Phi`` times the longest baseline, in radians: a value that is not tiny tells a tilt outside the basin (about
        pi / 2 on the longest baseline).  ``return_gains=False`` / ``return_model=False`` leave the transformed arrays out (the model rows
        are as large as the data).  Sums in double in a fixed order: two calls give the same bits.  Nothing the fit reads changes."""
        if mode not in _lib.DEGENERACY_MODES:
            raise ValueError(f"mode must be one of {sorted(_lib.DEGENERACY_MODES)}, got {mode!r}")
        if int(iters) < 1:
            raise ValueError(f"iters must be at least 1, got {iters!r}")
        if (g_r is None) != (g_i is None) or (gref_r is None) != (gref_i is None):
            raise ValueError("give both parts of g and of gref, or neither")
        if mode == "band" and freqs is None:
            raise ValueError("mode='band' needs freqs")
        nsl = self.gain_time_shape[0] if self.gain_time_shape is not None else self.nslices
        rs, gs = (self.nbls, self.nfreqs), (self.nants, self.nfreqs)
        keep = [self._real(ref_r, rs), self._real(ref_i, rs), None if ref_w is None else self._real(ref_w, rs),
                np.ascontiguousarray(antpos, dtype=np.float64), None if freqs is None else np.ascontiguousarray(freqs, dtype=np.float64)]
        keep += [None if a is None else self._real(a, gs) for a in (g_r, g_i, gref_r, gref_i)]
        if keep[3].shape != (self.nants // nsl, 2):
            raise ValueError(f"antpos must be [{self.nants // nsl}, 2], got shape {keep[3].shape}")
        if keep[4] is not None and keep[4].shape != (self.nfreqs,):
            raise ValueError(f"freqs must be [nfreqs = {self.nfreqs}], got shape {keep[4].shape}")
        d = _lib.DegeneracyDesc(_lib.DEGENERACY_MODES[mode], int(iters), *(None if a is None else a.ctypes.data for a in keep))
        params = np.empty((nsl, self.nfreqs, 4), dtype=np.float64)
        nsamp, step = np.empty((nsl, self.nfreqs), dtype=np.float64), np.empty((nsl, self.nfreqs), dtype=np.float64)
        o_gr, o_gi = (np.empty(gs, dtype=self.dtype), np.empty(gs, dtype=self.dtype)) if return_gains else (None, None)
        o_mr, o_mi = (np.empty(rs, dtype=self.dtype), np.empty(rs, dtype=self.dtype)) if return_model else (None, None)
        _lib.check(self._lib.cal_solver_fix_degeneracies(self._h, C.byref(d), _ptr(params), _ptr(nsamp), _ptr(step), _ptr(o_gr), _ptr(o_gi),
                                                         _ptr(o_mr), _ptr(o_mi)))
        out = dict(eta=params[..., 0].copy(), psi=params[..., 1].copy(), tilt=params[..., 2:].copy(), nsamples=nsamp, last_step=step)
        if return_gains:
            out.update(g_r=o_gr, g_i=o_gi)
        if return_model:
            out.update(model_r=o_mr, model_i=o_mi)
        return out

    def _set_delay_spectrum_scratch(self, nbytes):
        """Scratch bound of ``delay_spectrum`` in bytes (0: the default); the results do not depend on it (tests)."""
        _lib.check(self._lib.cal_solver_set_delay_spectrum_scratch(self._h, int(nbytes)))

    def delay_cross_spectrum(self, op, norm_f, pairs, scale=None, what=("data", "model", "resid"), stats=("cross", "diff"), calibrated=False,
                             bin_of_pair=None, nbins=0, per_pair=False, g_r=None, g_i=None):
        """Delay power that noise does not bias (cal_solver_delay_cross_spectrum), for pairs of rows that see the same sky with
        independent noise -- two adjacent integrations of one baseline, held as rows of this solver.  ``op``, ``norm_f``, ``what``,
        ``calibrated``, ``g_r``, ``g_i``: as in ``delay_spectrum``.  ``pairs`` ``[npairs, 2]`` row indices; ``scale`` ``[npairs, 2]``
        (``None``: ones) puts both sides into common units before they are combined.  For pair ``p = (b0, b1)``, scales ``(a0, a1)``::

            mask_p     = (w[b0] != 0) & (w[b1] != 0)                  the COMMON mask
            X_q[p][s]  = (mask_p q[b_s]) @ op                          s = 0, 1; products in the solver's dtype, on the matrix cores
            norm_pair  = sum_f mask_p norm_f
            Y_s        = a_s X_q[p][s]                                 in float64
            cross      = Re(Y_0 conj(Y_1)) / norm_pair                 signed; 0 where norm_pair == 0
            diff       = |Y_0 - Y_1|^2 / (2 norm_pair)                 >= 0

        With independent noise of equal variance on both sides ``cross`` expects the power of the common signal alone and ``diff`` the
        noise power of one side.  ``stats``: which of ``"cross"``, ``"diff"`` to form.  ``bin_of_pair`` ``[npairs]`` integers in
        ``[-1, nbins)``: the entry ``out[stat][quantity]`` is then ``[nbins, ndelays]``, the SUM over the bin's pairs with
        ``norm_pair > 0`` in ascending order, and ``"count_bin"`` their number.  ``per_pair=True`` adds
        ``"per_pair": {stat: {quantity: [npairs, ndelays]}}``.  ``"norm_pair"`` is always returned.  All float64; sums in a fixed
        order: two calls give the same bits.  Nothing the fit reads changes.  Under an exchange the binned arrays are summed over the
        ranks (one all-reduce); the per-pair arrays stay this rank's own."""
        if (g_r is None) != (g_i is None):
            raise ValueError("give both g_r and g_i, or neither")
        what = (what,) if isinstance(what, str) else tuple(what)
        if not what or any(q not in _lib.DELAY_SPECTRUM_WHAT for q in what) or len(set(what)) != len(what):
            raise ValueError(f"what must name one or more of {sorted(_lib.DELAY_SPECTRUM_WHAT)} once each, got {what!r}")
        stats = (stats,) if isinstance(stats, str) else tuple(stats)
        if not stats or any(k not in _lib.DELAY_CROSS_STATS for k in stats) or len(set(stats)) != len(stats):
            raise ValueError(f"stats must name one or more of {sorted(_lib.DELAY_CROSS_STATS)} once each, got {stats!r}")
        names = [q for q in ("data", "model", "resid") if q in what]  # the library's order
        snames = [k for k in ("cross", "diff") if k in stats]
        op = np.asarray(op)
        if op.ndim != 2 or op.shape[0] != self.nfreqs:
            raise ValueError(f"op must be [nfreqs = {self.nfreqs}, ndelays], got shape {op.shape}")
        nd = op.shape[1]
        op_r, op_i = self._real(op.real), self._real(op.imag)
        norm_f = np.ascontiguousarray(norm_f, dtype=np.float64)
        if norm_f.shape != (self.nfreqs,):
            raise ValueError(f"norm_f must be [nfreqs = {self.nfreqs}], got shape {norm_f.shape}")
        pairs = np.ascontiguousarray(pairs, dtype=np.int32)
        if pairs.ndim != 2 or pairs.shape[1] != 2 or pairs.shape[0] < 1:
            raise ValueError(f"pairs must be [npairs >= 1, 2], got shape {pairs.shape}")
        npairs = pairs.shape[0]
        if scale is not None:
            scale = np.ascontiguousarray(scale, dtype=np.float64)
            if scale.shape != (npairs, 2):
                raise ValueError(f"scale must be [npairs = {npairs}, 2], got shape {scale.shape}")
        nbins = int(nbins)
        if (bin_of_pair is None) != (nbins == 0):
            raise ValueError("give bin_of_pair and nbins > 0 together, or neither")
        bins = None
        if bin_of_pair is not None:
            bins = np.ascontiguousarray(bin_of_pair, dtype=np.int32)
            if bins.shape != (npairs,):
                raise ValueError(f"bin_of_pair must be [npairs = {npairs}], got shape {bins.shape}")
        gs = (self.nants, self.nfreqs)
        a = None if g_r is None else self._real(g_r, gs)
        b = None if g_i is None else self._real(g_i, gs)
        d = _lib.DelayCrossDesc(nd, sum(_lib.DELAY_SPECTRUM_WHAT[q] for q in names), int(bool(calibrated)), npairs, pairs.ctypes.data,
                                None if scale is None else scale.ctypes.data, sum(_lib.DELAY_CROSS_STATS[k] for k in snames), nbins,
                                None if bins is None else bins.ctypes.data, op_r.ctypes.data, op_i.ctypes.data, norm_f.ctypes.data)
        norm_pair = np.empty(npairs, dtype=np.float64)
        pp = {k: np.empty((len(names), npairs, nd), dtype=np.float64) if per_pair and k in snames else None for k in ("cross", "diff")}
        pb = {k: np.empty((len(names), nbins, nd), dtype=np.float64) if nbins and k in snames else None for k in ("cross", "diff")}
        c_bin = np.empty(nbins, dtype=np.float64) if nbins else None
        _lib.check(self._lib.cal_solver_delay_cross_spectrum(self._h, C.byref(d), _ptr(a), _ptr(b), _ptr(pp["cross"]), _ptr(pp["diff"]), _ptr(norm_pair),
                                                             _ptr(pb["cross"]), _ptr(pb["diff"]), _ptr(c_bin)))
        out = {"norm_pair": norm_pair}
        if nbins:
            out.update({k: {q: pb[k][i] for i, q in enumerate(names)} for k in snames}, count_bin=c_bin)
        if per_pair:
            out["per_pair"] = {k: {q: pp[k][i] for i, q in enumerate(names)} for k in snames}
        return out

    def delay_fringe_spectrum(self, op, norm_f, rows, opt, scale=None, what=("data", "model", "resid"), calibrated=False,
                              bin_of_group=None, nbins=0, per_group=False, g_r=None, g_i=None):
        """The delay / fringe-rate plane (cal_solver_delay_fringe_spectrum): the delay transform of groups of ``T`` rows -- one
        baseline at ``T`` integrations, held as rows of this solver -- and then a transform along time.  Instrument-locked residuals
        sit at fringe rate 0, the sky at the rate its baseline gives it, noise is white in fringe rate.  ``op``, ``norm_f``, ``what``,
        ``calibrated``, ``g_r``, ``g_i``: as in ``delay_spectrum``.  ``rows`` ``[ngroups, T]`` row indices (repeats allowed), ``T`` in
        ``[1, 64]``; ``opt`` ``[T, nrates]`` complex, ``nrates`` in ``[1, 64]``: the transform along time with its taper and
        normalisation folded in (``modeling.fringe_rate_transform``); ``scale`` ``[ngroups, T]`` (``None``: ones) puts the rows into
        common units before they are combined.  For group ``g``::

            mask_g     = AND over t of (w[rows[g][t]] != 0)            the COMMON mask of all T rows
            X_q[g][t]  = (mask_g q[rows[g][t]]) @ op                   products in the solver's dtype, on the matrix cores
            Y_t        = scale[g][t] X_q[g][t]                         in float64
            Z_q[g][r]  = sum_t opt[t][r] Y_t                           in float64, t ascending
            norm_grp   = sum_f mask_g norm_f
            power      = |Z|^2 / norm_grp                              0 where norm_grp == 0

        A group with one row flagged throughout has ``norm_grp == 0``, power 0, and enters no bin.  ``bin_of_group`` ``[ngroups]``
        integers in ``[-1, nbins)``: the entry ``out[quantity]`` is then ``[nbins, nrates, ndelays]``, the SUM over the bin's groups
        with ``norm_grp > 0`` in ascending order, and ``"count_bin"`` their number.  ``per_group=True`` adds
        ``"per_group": {quantity: [ngroups, nrates, ndelays]}``.  ``"norm_grp"`` is always returned.  All float64; sums in a fixed
        order: two calls give the same bits.  Nothing the fit reads changes.  Under an exchange the binned arrays are summed over the
        ranks (one all-reduce); the per-group arrays stay this rank's own."""
        if (g_r is None) != (g_i is None):
            raise ValueError("give both g_r and g_i, or neither")
        what = (what,) if isinstance(what, str) else tuple(what)
        if not what or any(q not in _lib.DELAY_SPECTRUM_WHAT for q in what) or len(set(what)) != len(what):
            raise ValueError(f"what must name one or more of {sorted(_lib.DELAY_SPECTRUM_WHAT)} once each, got {what!r}")
        names = [q for q in ("data", "model", "resid") if q in what]  # the library's order
        op = np.asarray(op)
        if op.ndim != 2 or op.shape[0] != self.nfreqs:
            raise ValueError(f"op must be [nfreqs = {self.nfreqs}, ndelays], got shape {op.shape}")
        nd = op.shape[1]
        op_r, op_i = self._real(op.real), self._real(op.imag)
        norm_f = np.ascontiguousarray(norm_f, dtype=np.float64)
        if norm_f.shape != (self.nfreqs,):
            raise ValueError(f"norm_f must be [nfreqs = {self.nfreqs}], got shape {norm_f.shape}")
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        if rows.ndim != 2 or rows.shape[0] < 1 or rows.shape[1] < 1:
            raise ValueError(f"rows must be [ngroups >= 1, ntimes >= 1], got shape {rows.shape}")
        ngroups, ntimes = rows.shape
        opt = np.asarray(opt, dtype=np.complex128)
        if opt.ndim != 2 or opt.shape[0] != ntimes or opt.shape[1] < 1:
            raise ValueError(f"opt must be [ntimes = {ntimes}, nrates >= 1], got shape {opt.shape}")
        nrates = opt.shape[1]
        opt_r, opt_i = np.ascontiguousarray(opt.real), np.ascontiguousarray(opt.imag)
        if scale is not None:
            scale = np.ascontiguousarray(scale, dtype=np.float64)
            if scale.shape != (ngroups, ntimes):
                raise ValueError(f"scale must be [ngroups = {ngroups}, ntimes = {ntimes}], got shape {scale.shape}")
        nbins = int(nbins)
        if (bin_of_group is None) != (nbins == 0):
            raise ValueError("give bin_of_group and nbins > 0 together, or neither")
        bins = None
        if bin_of_group is not None:
            bins = np.ascontiguousarray(bin_of_group, dtype=np.int32)
            if bins.shape != (ngroups,):
                raise ValueError(f"bin_of_group must be [ngroups = {ngroups}], got shape {bins.shape}")
        gs = (self.nants, self.nfreqs)
        a = None if g_r is None else self._real(g_r, gs)
        b = None if g_i is None else self._real(g_i, gs)
        d = _lib.DelayFringeDesc(nd, sum(_lib.DELAY_SPECTRUM_WHAT[q] for q in names), int(bool(calibrated)), ngroups, ntimes, nrates, rows.ctypes.data,
                                 None if scale is None else scale.ctypes.data, nbins, None if bins is None else bins.ctypes.data, op_r.ctypes.data,
                                 op_i.ctypes.data, norm_f.ctypes.data, opt_r.ctypes.data, opt_i.ctypes.data)
        norm_grp = np.empty(ngroups, dtype=np.float64)
        p_grp = np.empty((len(names), ngroups, nrates, nd), dtype=np.float64) if per_group else None
        p_bin = np.empty((len(names), nbins, nrates, nd), dtype=np.float64) if nbins else None
        c_bin = np.empty(nbins, dtype=np.float64) if nbins else None
        _lib.check(self._lib.cal_solver_delay_fringe_spectrum(self._h, C.byref(d), _ptr(a), _ptr(b), _ptr(p_grp), _ptr(norm_grp), _ptr(p_bin), _ptr(c_bin)))
        out = {"norm_grp": norm_grp}
        if nbins:
            out.update({q: p_bin[i] for i, q in enumerate(names)}, count_bin=c_bin)
        if per_group:
            out["per_group"] = {q: p_grp[i] for i, q in enumerate(names)}
        return out

    def delay_coherent_spectrum(self, op, norm_f, set_ptr, member_row, opt, member_wgt=None, member_conj=None, weighting="uniform", scale=None,
                                what=("data", "model", "resid"), calibrated=False, bin_of_group=None, nbins=0, per_group=False, g_r=None, g_i=None):
        """Delay / fringe-rate power of redundant averages (cal_solver_delay_coherent_spectrum): the rows of a redundant group are
        averaged BEFORE they are transformed and squared, so that noise power falls as 1 / N in the group size, where the mean of
        ``delay_fringe_spectrum``'s powers cannot.  ``op``, ``norm_f``, ``opt``, ``scale``, ``what``, ``calibrated``, the bins, ``g_r``,
        ``g_i`` and the returned dictionary are ``delay_fringe_spectrum``'s.  A group has ``T = opt.shape[0]`` SETS of rows; set
        ``v = g T + t`` holds the members ``set_ptr[v] .. set_ptr[v + 1]`` (``set_ptr`` ``[ngroups T + 1]``, from 0, never falling) of
        ``member_row`` (rows of this solver, repeats allowed), with coefficients ``member_wgt`` (finite, ``>= 0``; ``None``: ones) and
        flags ``member_conj`` (0 / 1: the row holds the pair reversed; ``None``: none)::

            u_k      = member_wgt[k]                          weighting="uniform"
                     = member_wgt[k] w[row_k]                 weighting="weights"      both 0 where w[row_k] == 0
            xbar_q[v]= sum_k u_k c_k(q[row_k]) / sum_k u_k    in float64, k ascending, rounded once to the dtype; 0 where the sum of u is 0
            mask_g   = AND over t of (sum_k u_k > 0)
            x_q[g][t]= mask_g xbar_q[g T + t]

        and from ``x_q`` on everything is ``delay_fringe_spectrum``'s.  An empty set gives its group ``norm_grp == 0``, power 0 and no
        bin.  Sets of one member with unit coefficient give ``delay_fringe_spectrum`` of those rows to the bit."""
        if (g_r is None) != (g_i is None):
            raise ValueError("give both g_r and g_i, or neither")
        if weighting not in ("uniform", "weights"):
            raise ValueError(f"weighting must be 'uniform' or 'weights', got {weighting!r}")
        what = (what,) if isinstance(what, str) else tuple(what)
        if not what or any(q not in _lib.DELAY_SPECTRUM_WHAT for q in what) or len(set(what)) != len(what):
            raise ValueError(f"what must name one or more of {sorted(_lib.DELAY_SPECTRUM_WHAT)} once each, got {what!r}")
        names = [q for q in ("data", "model", "resid") if q in what]  # the library's order
        op = np.asarray(op)
        if op.ndim != 2 or op.shape[0] != self.nfreqs:
            raise ValueError(f"op must be [nfreqs = {self.nfreqs}, ndelays], got shape {op.shape}")
        nd = op.shape[1]
        op_r, op_i = self._real(op.real), self._real(op.imag)
        norm_f = np.ascontiguousarray(norm_f, dtype=np.float64)
        if norm_f.shape != (self.nfreqs,):
            raise ValueError(f"norm_f must be [nfreqs = {self.nfreqs}], got shape {norm_f.shape}")
        opt = np.asarray(opt, dtype=np.complex128)
        if opt.ndim != 2 or opt.shape[0] < 1 or opt.shape[1] < 1:
            raise ValueError(f"opt must be [ntimes >= 1, nrates >= 1], got shape {opt.shape}")
        ntimes, nrates = opt.shape
        opt_r, opt_i = np.ascontiguousarray(opt.real), np.ascontiguousarray(opt.imag)
        set_ptr = np.ascontiguousarray(set_ptr, dtype=np.int64)
        if set_ptr.ndim != 1 or len(set_ptr) < ntimes + 1 or (len(set_ptr) - 1) % ntimes:
            raise ValueError(f"set_ptr must be [ngroups ntimes + 1] with ntimes = {ntimes} and ngroups >= 1, got shape {set_ptr.shape}")
        ngroups = (len(set_ptr) - 1) // ntimes
        member_row = np.ascontiguousarray(member_row, dtype=np.int32)
        if member_row.ndim != 1:
            raise ValueError(f"member_row must be [nmembers], got shape {member_row.shape}")
        nmembers = len(member_row)
        if member_wgt is not None:
            member_wgt = np.ascontiguousarray(member_wgt, dtype=np.float64)
            if member_wgt.shape != (nmembers,):
                raise ValueError(f"member_wgt must be [nmembers = {nmembers}], got shape {member_wgt.shape}")
        if member_conj is not None:
            member_conj = np.ascontiguousarray(member_conj, dtype=np.uint8)  # (the library refuses anything but 0 and 1)
            if member_conj.shape != (nmembers,):
                raise ValueError(f"member_conj must be [nmembers = {nmembers}], got shape {member_conj.shape}")
        if scale is not None:
            scale = np.ascontiguousarray(scale, dtype=np.float64)
            if scale.shape != (ngroups, ntimes):
                raise ValueError(f"scale must be [ngroups = {ngroups}, ntimes = {ntimes}], got shape {scale.shape}")
        nbins = int(nbins)
        if (bin_of_group is None) != (nbins == 0):
            raise ValueError("give bin_of_group and nbins > 0 together, or neither")
        bins = None
        if bin_of_group is not None:
            bins = np.ascontiguousarray(bin_of_group, dtype=np.int32)
            if bins.shape != (ngroups,):
                raise ValueError(f"bin_of_group must be [ngroups = {ngroups}], got shape {bins.shape}")
        gs = (self.nants, self.nfreqs)
        a = None if g_r is None else self._real(g_r, gs)
        b = None if g_i is None else self._real(g_i, gs)
        d = _lib.DelayCoherentDesc(nd, sum(_lib.DELAY_SPECTRUM_WHAT[q] for q in names), int(bool(calibrated)), ngroups, ntimes, nrates, set_ptr.ctypes.data,
                                   member_row.ctypes.data if nmembers else None, None if member_wgt is None else member_wgt.ctypes.data,
                                   None if member_conj is None else member_conj.ctypes.data, int(weighting == "weights"),
                                   None if scale is None else scale.ctypes.data, nbins, None if bins is None else bins.ctypes.data, op_r.ctypes.data,
                                   op_i.ctypes.data, norm_f.ctypes.data, opt_r.ctypes.data, opt_i.ctypes.data, nmembers)
        norm_grp = np.empty(ngroups, dtype=np.float64)
        p_grp = np.empty((len(names), ngroups, nrates, nd), dtype=np.float64) if per_group else None
        p_bin = np.empty((len(names), nbins, nrates, nd), dtype=np.float64) if nbins else None
        c_bin = np.empty(nbins, dtype=np.float64) if nbins else None
        _lib.check(self._lib.cal_solver_delay_coherent_spectrum(self._h, C.byref(d), _ptr(a), _ptr(b), _ptr(p_grp), _ptr(norm_grp), _ptr(p_bin), _ptr(c_bin)))
        out = {"norm_grp": norm_grp}
        if nbins:
            out.update({q: p_bin[i] for i, q in enumerate(names)}, count_bin=c_bin)
        if per_group:
            out["per_group"] = {q: p_grp[i] for i, q in enumerate(names)}
        return out

    def delay_transfer(self, op, ridge=1e-6, calibrated=False, bin_of_bl=None, nbins=0, per_baseline=False, g_r=None, g_i=None):
        """The signal loss of the fit in delay space (cal_solver_delay_transfer): the share of the power at every delay that the
        coefficient fit itself removes.  ``op`` ``[nfreqs, ndelays]`` complex: the operator of ``delay_spectrum``.  With
        ``G = g_i conj(g_j)``, ``q = w |G|^2``, ``mask = (w != 0)``, ``a_{b,f}`` row ``f`` of the basis of row ``b`` and ``L`` the
        Cholesky factor of the group's ridged normal matrix (``fit_errors``')::

                             calibrated=False (d - G m)     calibrated=True (d / G - m)
            s[b][f]     =    mask G                         mask                    (0 where |G|^2 == 0)
            v[b][f]     =    mask / w                       mask / q                (0 where |G|^2 == 0)
            num[b][k]      = |L^-1 sum_f op[f][k] s[b][f] a_{b,f}|^2
            noise_bl[b][k] = sum_f v[b][f] |op[f][k]|^2
            absorbed_bl    = num / noise_bl                 0 where noise_bl == 0 or the group is singular; in [0, 1]

        For noise of variance ``1 / w`` on the unflagged samples, the gains held fixed (the conditional view of ``fit_errors``: a lower
        bound on the loss) and the coefficients at their weighted least-squares optimum, ``noise_bl`` is the expected delay power of
        the masked data and ``noise_bl - num`` that of the masked residual; exact at ``ridge = 0``.  ``bin_of_bl`` ``[nbls]`` integers
        in ``[-1, nbins)``: ``"absorbed_bin"`` ``[nbins, ndelays]`` is the SUM of ``absorbed_bl`` over the bin's rows that have an
        unflagged sample and a factored group, in ascending row order, and ``"count_bin"`` ``[nbins]`` their number, so that
        ``1 - absorbed_bin / count_bin`` is the transfer of a signal that is white in delay.  ``per_baseline=True`` adds
        ``"absorbed_bl"`` and ``"noise_bl"`` ``[nbls, ndelays]`` (as large as the data: off by default).  ``g_r``, ``g_i``: gains for
        this call only, as in ``fit_quality``.  All float64; sums in a fixed order: two calls give the same bits.  The parameters,
        moments, weights and loop state are untouched.  Under an exchange the binned arrays are summed over the ranks (one
        all-reduce); the per-baseline arrays stay this rank's own rows.  Returns a dict with ``nsolved`` and ``nsingular`` (groups)
        beside the arrays."""
        if (g_r is None) != (g_i is None):
            raise ValueError("give both g_r and g_i, or neither")
        op = np.asarray(op)
        if op.ndim != 2 or op.shape[0] != self.nfreqs:
            raise ValueError(f"op must be [nfreqs = {self.nfreqs}, ndelays], got shape {op.shape}")
        nd = op.shape[1]
        op_r, op_i = self._real(op.real), self._real(op.imag)
        nbins = int(nbins)
        if (bin_of_bl is None) != (nbins == 0):
            raise ValueError("give bin_of_bl and nbins > 0 together, or neither")
        bins = None
        if bin_of_bl is not None:
            bins = np.ascontiguousarray(bin_of_bl, dtype=np.int32)
            if bins.shape != (self.nbls,):
                raise ValueError(f"bin_of_bl must be [nbls = {self.nbls}], got shape {bins.shape}")
        gs = (self.nants, self.nfreqs)
        a = None if g_r is None else self._real(g_r, gs)
        b = None if g_i is None else self._real(g_i, gs)
        d = _lib.DelayTransferDesc(nd, int(bool(calibrated)), nbins, None if bins is None else bins.ctypes.data, op_r.ctypes.data, op_i.ctypes.data,
                                   float(ridge))
        a_bl = np.empty((self.nbls, nd), dtype=np.float64) if per_baseline else None
        n_bl = np.empty((self.nbls, nd), dtype=np.float64) if per_baseline else None
        a_bin = np.empty((nbins, nd), dtype=np.float64) if nbins else None
        c_bin = np.empty(nbins, dtype=np.float64) if nbins else None
        cnt = _lib.FitErrorsCounts()
        _lib.check(self._lib.cal_solver_delay_transfer(self._h, C.byref(d), _ptr(a), _ptr(b), _ptr(a_bl), _ptr(n_bl), _ptr(a_bin), _ptr(c_bin),
                                                       C.byref(cnt)))
        out = {"nsolved": int(cnt.nsolved), "nsingular": int(cnt.nsingular)}
        if nbins:
            out.update(absorbed_bin=a_bin, count_bin=c_bin)
        if per_baseline:
            out.update(absorbed_bl=a_bl, noise_bl=n_bl)
        return out

    def _set_delay_transfer_scratch(self, nbytes):
        """Scratch bound of ``delay_transfer`` in bytes (0: the default); the results do not depend on it (tests)."""
        _lib.check(self._lib.cal_solver_set_delay_transfer_scratch(self._h, int(nbytes)))

    def fit_errors(self, ridge=1e-6, model_var=True, gain_var=True, coeffs=True):
        """The errors of the fit at the solver's current parameters (cal_solver_fit_errors): the inverses of the curvature matrices
        of ``solve_coeffs`` and ``solve_gains``.  With ``G = g_i conj(g_j)`` from the full (expanded) gains, ``q = w |G|^2``, ``A_b``
        the row block of baseline row ``b`` in fitting group ``gamma`` and ``a_{b,f}`` its row ``f``::

            N_gamma = sum_{b in gamma} A_b^T diag(q_b) A_b      N_r = N_gamma + ridge (tr N_gamma / nvec) I      L L^T = N_r
            coeff_var[k]    = (N_r^-1)[k][k]                                [ncoef]         (re and im of c_k: this variance / 2 each)
            model_var[b][f] = a_{b,f}^T N_r^-1 a_{b,f} = |L^-1 a_{b,f}|^2   [nbls, nfreqs]  (variance of m = A c, before the gains)
            leverage_bl[b]  = sum_f q[b][f] model_var[b][f]                 [nbls]          (q model_var lies in [0, 1])
            nsamp_bl[b]     = #{f : w[b][f] != 0}                           [nbls]
            gain_var[a][f]  = 1 / den_a[f], den_a = sum_b w |m|^2 |g_other|^2 of ``solve_gains``; 0 where den_a <= 0   [nants, nfreqs]

        All float64, variances for unit noise scale: exact where the weights are inverse noise variances.  These are CONDITIONAL
        errors -- the gains are held fixed for the coefficients and the model, the model and the other gains for a gain: the block
        diagonal of the Gauss-Newton matrix.  The gain-foreground covariance and with it the degeneracies are ignored, so they are
        lower bounds.  With ``ridge = 0`` and ``N`` of full rank the ``leverage_bl`` of a group add up to its ``nvec``.  A singular
        group (wholly flagged, or a non-positive pivot) keeps zeros and counts in ``nsingular``.

        ``model_var=False`` leaves the ``[nbls, nfreqs]`` plane out (it is as large as the data); ``gain_var=False`` skips the antenna
        part; ``coeffs=False`` skips the coefficient part (``coeff_var``, ``model_var``, ``leverage_bl``).  With a gain basis attached
        ``gain_var=True`` raises: the variance of a basis gain is ``b_f^T N_a^-1 b_f`` with the projected ``N_a``, which is not
        computed here but by ``gain_basis_errors``.  The parameters, the optimizer's slots, the weights and the loop state are untouched.  Under an exchange only
        ``den`` is summed over the ranks (one ``[nants, nfreqs]`` float64 plane); every other output is this rank's own rows and groups.
        Returns a dict of the arrays asked for plus ``nsolved`` and ``nsingular``."""
        out = {}
        if coeffs:
            out["coeff_var"] = np.empty(self.ncoeffs, dtype=np.float64)
            if model_var:
                out["model_var"] = np.empty((self.nbls, self.nfreqs), dtype=np.float64)
            out["leverage_bl"] = np.empty(self.nbls, dtype=np.float64)
        out["nsamp_bl"] = np.empty(self.nbls, dtype=np.float64)
        if gain_var:
            out["gain_var"] = np.empty((self.nants, self.nfreqs), dtype=np.float64)
        cnt = _lib.FitErrorsCounts()
        _lib.check(self._lib.cal_solver_fit_errors(self._h, float(ridge), *(_ptr(out.get(k)) for k in ("coeff_var", "model_var", "leverage_bl",
                                                                                                      "nsamp_bl", "gain_var")), C.byref(cnt)))
        out["nsolved"], out["nsingular"] = int(cnt.nsolved), int(cnt.nsingular)
        return out

    def gain_basis_errors(self, ridge=1e-6, y_var=True):
        """The error bars of gains confined to a basis at the solver's current parameters (cal_solver_gain_basis_errors): the inverse
        of the projected curvature matrix of ``solve_gain_coeffs`` / ``solve_gain_time_coeffs``.  ``den[row][f]`` is ``solve_gains``'
        per-row sum (autocorrelations left out), ``shift = ridge tr N / n``.  With a frequency basis ``B [nfreqs, K]``, per antenna
        row ``a`` (``n = K``)::

            N_a = B^T diag(den_a) B     N_r = N_a + shift I     L L^T = N_r     W = L^-1
            y_var[a][k]    = sum_i W[i][k]^2                        (variance of the complex y_k)
            gain_var[a][f] = |W b_f|^2 = b_f^T N_r^-1 b_f           (b_f: row f of B), flagged channels included: the basis interpolates
            gain_dof[a]    = n - shift sum_k y_var[a][k]            (= tr(N_a N_r^-1): complex parameters spent)

        with a time basis ``Bt [T, L]`` on top, per antenna ``a``, ``n = L K``, index ``l K + k``, ``N_a`` as
        ``solve_gain_time_coeffs`` forms it::

            gain_var[t Na + a][f] = |W (Bt[t,:] (x) b_f)|^2         y_var[a][l][k] = sum_i W[i][l K + k]^2

        and with a time basis alone, per (antenna, channel), ``L x L``, in float64 throughout::

            N_{a,f}[l,l'] = sum_t Bt[t,l] Bt[t,l'] den[t,a,f]       y_var[a][l][f] = (N_r^-1)[l][l]
            gain_var[t Na + a][f] = Bt[t,:] N_r^-1 Bt[t,:]^T        gain_dof[a] = sum over the solved f of (L - shift_f sum_l y_var[a][l][f])

        All float64, variances for unit noise scale, CONDITIONAL on the other antennas and the model like ``fit_errors``'
        ``gain_var``, which ``B = I`` reproduces.  A singular system (an antenna row, an antenna, or an (antenna, channel) pair
        under a time basis alone: no unflagged cross-correlation, or a non-positive pivot) keeps zeros in all outputs and counts in
        ``nsingular``.  ``y_var=False`` leaves ``y_var`` out.  Needs a gain basis (``set_gain_basis``, ``set_gain_time_basis``).
        The parameters, ``y``, the optimizer's slots and the loop state are untouched; sums run in a fixed order, so two calls give
        the same bits.  Under an exchange only ``den`` is summed over the ranks (one ``[nants, nfreqs]`` float64 plane) and every
        rank computes the same planes.  Returns a dict: ``gain_var`` ``[nants, nfreqs]``, ``y_var`` in the shape of
        ``get_gain_coeffs``, ``gain_dof`` (one per row of ``y``), ``nsolved``, ``nsingular``."""
        shape = self._gain_coeff_shape()
        out = dict(gain_var=np.empty((self.nants, self.nfreqs), dtype=np.float64))
        if y_var:
            out["y_var"] = np.empty(shape, dtype=np.float64)
        out["gain_dof"] = np.empty(shape[0], dtype=np.float64)
        cnt = _lib.FitErrorsCounts()
        _lib.check(self._lib.cal_solver_gain_basis_errors(self._h, float(ridge), _ptr(out["gain_var"]), _ptr(out.get("y_var")), _ptr(out["gain_dof"]),
                                                          C.byref(cnt)))
        out["nsolved"], out["nsingular"] = int(cnt.nsolved), int(cnt.nsingular)
        return out

    def _slice_mask(self, mask):
        if mask is None:
            return None
        m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        if m.shape != (self.nslices,):
            raise ValueError(f"expected one mask entry per time slice ({self.nslices}), got shape {m.shape}")
        return m

    def robust_weights(self, kind="huber", threshold=3.0, slice_mask=None):
        """One round of iteratively reweighted least squares (cal_solver_robust_weights): the weight plane every kernel path reads is
        rewritten in place from the residual at the solver's current parameters.  ``fit_quality``, the closed-form solves and the five
        post-fit reports read that one plane too: ``fit_errors``, ``gain_basis_errors``, ``delay_spectrum``, ``delay_transfer``, and
        ``fix_degeneracies`` where its ``ref_w`` is ``None`` (given reference weights replace it).  With ``w0`` the weights as ``set_data`` gave them,
        ``(i, j)`` the antennas of baseline row ``b``, ``m = A c``, ``g`` the solver's gains and ``k = threshold`` (in sigma)::

            e[b][f]  = w0[b][f] |d[b][f] - g_i[f] conj(g_j[f]) m[b][f]|^2     (products in the solver's dtype)
            S_b      = { f < nfreqs : w0[b][f] > 0 },  n_b = |S_b|
            med_b    = the ((n_b + 1) // 2)-th smallest of e[b][S_b]          (the lower median: an element of the row)
            scale_b  = med_b / ln 2
            z2       = e / scale_b
            huber  : psi = 1 if z2 <= k^2 else k / sqrt(z2)
            cauchy : psi = 1 / (1 + z2 / k^2)
            clip   : psi = 1 if z2 <= k^2 else 0
            w[b][f]  = w0[b][f] * psi

        ``scale_b = med_b / ln 2`` because ``w |r|^2`` of complex Gaussian residuals is exponentially distributed (median = ``ln 2`` x
        mean).  Rows with ``n_b = 0`` or ``med_b = 0`` keep ``w = w0``.  Every call starts from ``w0``, never from the previous ``w``;
        the weights are not renormalised, so losses before and after a call are not comparable.  ``kind="none"`` puts ``w0`` back.
        ``slice_mask``: ``[nslices]``, the slices to reweight (``None``: all); the rows of the others keep their bits.  The call is
        local to a baseline row: no exchange under a communicator.  Returns ``{"scale_bl", "ndown_bl"}``, ``[nbls]`` float64:
        ``scale_b`` and the number of samples with ``psi < 1`` (both 0 for rows of unselected slices)."""
        if kind not in _lib.ROBUST_KINDS:
            raise ValueError(f"unknown robust kind {kind!r}: one of {sorted(_lib.ROBUST_KINDS)}")
        m = self._slice_mask(slice_mask)
        d = _lib.RobustDesc(_lib.ROBUST_KINDS[kind], float(threshold), None if m is None else m.ctypes.data)
        out = dict(scale_bl=np.empty(self.nbls, dtype=np.float64), ndown_bl=np.empty(self.nbls, dtype=np.float64))
        _lib.check(self._lib.cal_solver_robust_weights(self._h, C.byref(d), _ptr(out["scale_bl"]), _ptr(out["ndown_bl"])))
        return out

    def get_weights(self, which=0):
        """The weight plane ``[nbls, nfreqs]``: ``which=0`` the weights the kernels read now, ``which=1`` ``w0``, the weights as
        ``set_data`` gave them (the same until ``robust_weights`` has run)."""
        out = np.empty((self.nbls, self.nfreqs), dtype=self.dtype)
        _lib.check(self._lib.cal_solver_get_weights(self._h, _ptr(out), int(which)))
        return out

    def solve_gains(self, nsweeps, damping=0.5, slice_mask=None, reset_gain_moments=False):
        """``nsweeps`` damped StefCal sweeps over the gains with the foreground model ``m = A c`` held fixed at the solver's
        coefficients (cal_solver_solve_gains): per antenna ``a`` and channel, with the other antennas at their OLD gains,
        ``g_a <- (1 - damping) g_a + damping num_a / den_a``, ``num_a = sum_b w d conj(m) g_other`` (conjugated where ``a`` is the
        baseline's second antenna), ``den_a = sum_b w |m|^2 |g_other|^2`` over the cross-correlation baselines of ``a``; unchanged
        where ``den_a`` is 0.  The sweeps minimise the chi-square term only (not the "sum" regulariser).  ``slice_mask``:
        ``[nslices]``, the slices to solve (``None``: all); the others keep their gains bit for bit.  ``reset_gain_moments``: the
        optimizer's gain slots of the solved slices start over as after ``set_optimizer`` (iteration counts and coefficient slots
        stay).  Not available while a gain basis is set.  Under an exchange every sweep sums three ``[nants, nfreqs]`` float64 planes
        over the ranks, and every rank applies the same update."""
        m = self._slice_mask(slice_mask)
        d = _lib.GainSolveDesc(int(nsweeps), int(bool(reset_gain_moments)), float(damping), None if m is None else m.ctypes.data)
        _lib.check(self._lib.cal_solver_solve_gains(self._h, C.byref(d)))

    def solve_coeffs(self, niters=1, damping=1.0, ridge=1e-6, slice_mask=None, reset_coeff_moments=False):
        """The foreground coefficients in closed form with the gains held fixed (cal_solver_solve_coeffs): per fitting group the
        normal equations ``(N + ridge tr(N)/nvec I) delta = rhs`` with ``N = sum_b A_b^T diag(w |G|^2) A_b`` and
        ``rhs = sum_b A_b^T (w conj(G) (d - G A c))``, ``G = g_i conj(g_j)`` from the solver's full gains, then
        ``c <- c + damping delta``.  ``N`` and ``rhs`` are formed in the solver's dtype on the matrix cores, the Cholesky solve runs in
        float64.  ``niters`` repeats the whole sequence (in float32 a second iteration is iterative refinement).  ``slice_mask``:
        ``[nslices]``, the slices to solve (``None``: all); the others keep their coefficients bit for bit.
        ``reset_coeff_moments``: the optimizer's coefficient slots of the solved slices start over as after ``set_optimizer``.  Works
        with a gain basis attached (the gains are only read) and issues no exchange.  Returns ``{"nsolved", "nsingular"}`` of the last
        iteration: a singular group (wholly flagged, or a non-positive pivot) keeps its coefficients."""
        m = self._slice_mask(slice_mask)
        d = _lib.CoeffSolveDesc(int(niters), int(bool(reset_coeff_moments)), float(damping), float(ridge), None if m is None else m.ctypes.data)
        r = _lib.CoeffSolveResult()
        _lib.check(self._lib.cal_solver_solve_coeffs(self._h, C.byref(d), C.byref(r)))
        return {"nsolved": int(r.nsolved), "nsingular": int(r.nsingular)}

    def normal_product(self, p_g_r, p_g_i, p_c_r, p_c_i):
        """``N p`` for the joint Gauss-Newton matrix ``N = J^H W J`` over gains and coefficients at the solver's current parameters
        (cal_solver_normal_product).  With ``m = A c``, ``G = g_i conj(g_j)`` and the direction ``p = (dg [nants, nfreqs], dc [ncoeffs])``
        complex, held as (re, im) like the parameters::

            (J p)[b][f] = (dg_i conj(g_j) + g_i conj(dg_j)) m + G (A dc)
            N p = -1/2 (grad(G m + J p) - grad(G m))

        where ``grad(d')`` is what ``eval_grads`` returns when the data are ``d'``: the product runs the solver's own model and gradient
        passes on substituted operands and puts everything back (data, weights, loss and loop state keep their bits).  ``N`` is that of
        the chi-square term alone, regulariser on or off.  Returns ``(out_g_r, out_g_i, out_c_r, out_c_i)``, laid out like the gradient.
        Not available with a gain basis or under an exchange."""
        gs, cs = (self.nants, self.nfreqs), (self.ncoeffs,)
        arrs = [self._real(a, shp) for a, shp in ((p_g_r, gs), (p_g_i, gs), (p_c_r, cs), (p_c_i, cs))]
        out = [np.empty(gs, dtype=self.dtype), np.empty(gs, dtype=self.dtype), np.empty(cs, dtype=self.dtype), np.empty(cs, dtype=self.dtype)]
        _lib.check(self._lib.cal_solver_normal_product(self._h, *[_ptr(a) for a in arrs + out]))
        return tuple(out)

    def gauss_newton_step(self, ncg=20, lam=1e-3, cg_tol=1e-3, slice_mask=None, reset_moments=False):
        """One Levenberg-damped Gauss-Newton step over gains and coefficients together (cal_solver_gauss_newton_step): per slice
        ``(N + lam D) p = rhs`` with ``N = J^H W J`` (``normal_product``), ``rhs = J^H W (d - G m)`` (minus half the chi-square gradient)
        and the diagonal ``D`` (for a gain ``den`` of ``solve_gains``, for a coefficient of group ``gamma`` ``sum_b mean_f w |G|^2``), solved
        by at most ``ncg`` iterations of conjugate gradients preconditioned with ``D`` from ``p = 0``; a slice stops once
        ``sqrt(rz / rz0) <= cg_tol``.  The trial parameters ``g + dg``, ``c + dc`` are kept iff their loss (as ``eval_loss``, regulariser
        included) is finite and strictly below the loss before; a rejected slice and a slice whose ``slice_mask`` entry is 0 keep the
        bits of their parameters.  ``lam``: one number or one per slice.  ``reset_moments``: the optimizer's gain and coefficient slots
        of the accepted slices start over as after ``set_optimizer`` (iteration counts stay).  Nothing else the fit reads changes.
        Not available with a gain basis or under an exchange.  Returns a dict of per-slice arrays: ``loss_before``, ``loss_after``,
        ``cg_residual`` (float64), ``cg_iters`` (int) and ``accepted`` (bool)."""
        m = self._slice_mask(slice_mask)
        lam = np.ascontiguousarray(np.broadcast_to(np.asarray(lam, dtype=np.float64), (self.nslices,)))
        d = _lib.GaussNewtonDesc(int(ncg), int(bool(reset_moments)), float(cg_tol), lam.ctypes.data, None if m is None else m.ctypes.data)
        res = (_lib.GaussNewtonResult * self.nslices)()
        _lib.check(self._lib.cal_solver_gauss_newton_step(self._h, C.byref(d), res))
        return dict(loss_before=np.asarray([r.loss_before for r in res]), loss_after=np.asarray([r.loss_after for r in res]),
                    cg_residual=np.asarray([r.cg_residual for r in res]), cg_iters=np.asarray([r.cg_iters for r in res], dtype=np.int64),
                    accepted=np.asarray([bool(r.accepted) for r in res]))

    LBFGS_STATUS = {0: "nsteps", 1: "ftol", 2: "stalled", 3: "bad start", 4: "masked"}

    def lbfgs(self, nsteps, history=8, max_ls=20, c1=1e-4, shrink=0.5, ftol=0.0, curvature_eps=1e-8, slice_mask=None, freeze_model=False,
              reset_moments=False):
        """``nsteps`` iterations of L-BFGS with a backtracking Armijo line search (cal_solver_lbfgs), every slice on its own, over the
        optimizer's own variables: the gains -- with a frequency or time gain basis the coefficients ``y`` -- and the foreground
        coefficients (``freeze_model``: the gains alone, the coefficients keep their bits).  It needs only the loss and its gradient,
        so it runs where ``gauss_newton_step`` refuses: with gain bases and with a frozen model.  ``history`` in [1, 16] pairs; a trial
        is accepted iff its loss (as ``eval_loss``, regulariser included) is finite and ``<= f + c1 t slope``, else ``t *= shrink``, at
        most ``max_ls`` times; a pair enters the history iff ``s.y > curvature_eps sqrt(s.s y.y)``; a slice stops early once
        ``ftol > 0`` and ``f_k - f_{k+1} <= ftol |f_k|``.  ``reset_moments``: the optimizer's slots of the variables of the slices
        that moved start over as after ``set_optimizer``.  Nothing else the fit reads changes.  Not available under an exchange.
        Returns a dict of per-slice arrays ``loss_before``, ``loss_after``, ``iters``, ``evals`` (trial losses), ``pairs_dropped``,
        ``status`` (0 all iterations, 1 ``ftol``, 2 stalled: no trial accepted and the variables as they were, 3 the start's loss or
        gradient not usable, 4 masked) and ``losses`` ``[nslices, nsteps + 1]``, NaN past ``iters``."""
        m = self._slice_mask(slice_mask)
        d = _lib.LbfgsDesc(int(nsteps), int(history), int(max_ls), int(bool(freeze_model)), int(bool(reset_moments)), 0, float(c1), float(shrink),
                           float(ftol), float(curvature_eps), None if m is None else m.ctypes.data)
        res = (_lib.LbfgsResult * self.nslices)()
        losses = np.full((self.nslices, max(int(nsteps), 0) + 1), np.nan)
        _lib.check(self._lib.cal_solver_lbfgs(self._h, C.byref(d), losses.ctypes.data, res))
        return dict(loss_before=np.asarray([r.loss_before for r in res]), loss_after=np.asarray([r.loss_after for r in res]),
                    iters=np.asarray([r.iters for r in res], dtype=np.int64), evals=np.asarray([r.evals for r in res], dtype=np.int64),
                    pairs_dropped=np.asarray([r.pairs_dropped for r in res], dtype=np.int64),
                    status=np.asarray([r.status for r in res], dtype=np.int64), losses=losses)

    def _set_coeff_solve_scratch(self, nbytes):
        """Scratch bound of ``solve_coeffs`` in bytes (0: the default); the results do not depend on it (tests)."""
        _lib.check(self._lib.cal_solver_set_coeff_solve_scratch(self._h, int(nbytes)))

    def solve_gain_coeffs(self, nsweeps, damping=0.5, ridge=1e-6, slice_mask=None, reset_gain_moments=False):
        """``nsweeps`` damped StefCal sweeps projected on the frequency gain basis ``g = g0 + B y`` (cal_solver_solve_gain_coeffs),
        with the foreground model held fixed.  ``num``, ``den`` are ``solve_gains``' per-antenna sums from the OLD gains; for antenna
        row ``a`` (one antenna of one slice), ``g_a`` the current expanded gains and ``B [nfreqs, K]`` the attached basis::

            r_a[f]  = num_a[f] - den_a[f] g_a[f]                 (complex; minus half the chi-square gradient w.r.t. g_a)
            N_a     = B^T diag(den_a) B                          [K][K], real symmetric
            rhs_a   = B^T r_a                                    [K], complex
            (N_a + ridge (tr N_a / K) I) delta_a = rhs_a         (one factorisation, two right-hand sides: re, im)
            y_a    <- y_a + damping delta_a                      then gains = g0 + B y for the whole array

        ``N_a`` and ``rhs_a`` are formed in the solver's dtype on the matrix cores, the Cholesky solve and the update run in float64.
        ``B = I``, ``ridge = 0`` is ``solve_gains``' update; a channel with ``den = 0`` of a non-singular antenna does move (the basis
        interpolates across it).  The sweeps minimise the chi-square term only (not the "sum" regulariser).  ``slice_mask``:
        ``[nslices]``, the slices to solve (``None``: all); the others keep ``y`` and gains bit for bit.  ``reset_gain_moments``: the
        optimizer's ``y`` slots of the solved slices start over as after ``set_optimizer``.  Needs a frequency gain basis
        (``set_gain_basis``) and refuses a time gain basis.  Under an exchange every sweep sums three ``[nants, nfreqs]`` float64
        planes over the ranks, and every rank applies the same update.  Returns ``{"nsolved", "nsingular"}``, the antenna rows of the
        last sweep: a singular row (no unflagged cross-correlation, or a non-positive pivot) keeps its ``y``."""
        m = self._slice_mask(slice_mask)
        d = _lib.GainCoeffSolveDesc(int(nsweeps), int(bool(reset_gain_moments)), float(damping), float(ridge), None if m is None else m.ctypes.data)
        r = _lib.GainCoeffSolveResult()
        _lib.check(self._lib.cal_solver_solve_gain_coeffs(self._h, C.byref(d), C.byref(r)))
        return {"nsolved": int(r.nsolved), "nsingular": int(r.nsingular)}

    def solve_gain_time_coeffs(self, nsweeps, damping=0.5, ridge=1e-6, reset_gain_moments=False):
        """``nsweeps`` damped StefCal sweeps taken jointly over the times of a fit with a gain time basis
        (cal_solver_solve_gain_time_coeffs), ``g[t] = g0[t] + sum_l Bt[t,l] z_l`` with ``z_l = B y_l`` under a frequency basis and
        ``y_l`` without one, the foreground model held fixed.  The solver holds ``T`` times of ``Na`` antennas as one fit (row
        ``t Na + a``); ``y`` is ``[Na, L, W]``.  ``num``, ``den`` are ``solve_gains``' per-row sums from the OLD gains,
        ``r[row][f] = num - den g`` in float64.  With a frequency basis (``n = L K``, index ``l K + k``),
        ``M_{t,a} = B^T diag(den_{t,a}) B`` as ``solve_gain_coeffs`` forms it::

            N_a[(l,k),(l',k')] = sum_t Bt[t,l] Bt[t,l'] M_{t,a}[k,k']          rhs_a[(l,k)] = sum_t Bt[t,l] (B^T r_{t,a})[k]
            (N_a + ridge (tr N_a / n) I) delta_a = rhs_a                        y_a <- y_a + damping delta_a

        Without one the system decouples per (antenna, channel), ``L x L`` each, everything in float64::

            N_{a,f}[l,l'] = sum_t Bt[t,l] Bt[t,l'] den[t,a,f]                   rhs_{a,f}[l] = sum_t Bt[t,l] r[t,a,f]
            (N_{a,f} + ridge (tr N_{a,f} / L) I) delta = rhs                    y[a][:][f] <- y[a][:][f] + damping delta

        Every system is solved from the old gains (a Jacobi sweep) and the gains are rebuilt once per sweep.  A system with
        ``tr <= 0`` (no unflagged cross-correlation at any time) or a bad pivot keeps the bits of its ``y`` and gains; an antenna
        flagged at some times only IS solved and its gains there move (the time basis interpolates), like a flagged channel under a
        frequency basis.  ``T = 1, Bt = [[1]]`` gives the bits of ``solve_gain_coeffs``; ``Bt = I, ridge = 0`` is its sweep per time;
        ``damping = 1, ridge = 0`` lands on the exact per-antenna minimiser.  The sweeps minimise the chi-square term only (not the
        "sum" regulariser).  ``M_{t,a}`` and ``B^T r`` are in the solver's dtype, the sums over ``t`` run in float64 in ascending
        ``t`` and are rounded once, the Cholesky solve and the update run in float64; two calls give the same bits.
        ``reset_gain_moments``: the optimizer's ``y`` slots start over as after ``set_optimizer``.  Needs a gain time basis
        (``set_gain_time_basis``).  Returns ``{"nsolved", "nsingular"}``, the systems of the last sweep: antennas with a frequency
        basis, (antenna, channel) pairs without one."""
        d = _lib.GainTimeSolveDesc(int(nsweeps), int(bool(reset_gain_moments)), float(damping), float(ridge))
        r = _lib.GainTimeSolveResult()
        _lib.check(self._lib.cal_solver_solve_gain_time_coeffs(self._h, C.byref(d), C.byref(r)))
        return {"nsolved": int(r.nsolved), "nsingular": int(r.nsingular)}

    def hold_slices(self, mask=None):
        """Slices that enter every later ``run`` / ``run_slices`` as already stopped (``[nslices]``, nonzero = held; ``None``: no
        slice): a loop issued in several calls keeps the slices that met the tolerance earlier as they are.  ``set_optimizer``
        clears it.  (cal_solver_hold_slices)"""
        m = self._slice_mask(mask)
        _lib.check(self._lib.cal_solver_hold_slices(self._h, _ptr(m)))

    def init_coeffs(self, src_r, src_i):
        shp = (self.nbls, self.nfreqs)
        a, b = self._real(src_r, shp), self._real(src_i, shp)
        _lib.check(self._lib.cal_solver_init_coeffs(self._h, _ptr(a), _ptr(b)))

    def synchronize(self):
        _lib.check(self._lib.cal_solver_synchronize(self._h))

    def set_launch_mode(self, mode="auto"):
        """How a train step is issued: "auto", "kernels" (every kernel its own launch), "one_tail" (two launches per step),
        "graph" (two-launch steps replayed from a hipGraph).  Same numbers in every mode."""
        ids = {"auto": _lib.CAL_LAUNCH_AUTO, "kernels": _lib.CAL_LAUNCH_KERNELS, "one_tail": _lib.CAL_LAUNCH_ONE_TAIL, "graph": _lib.CAL_LAUNCH_GRAPH}
        _lib.check(self._lib.cal_solver_set_launch_mode(self._h, ids[mode]))

    def timing_enable(self, enable=True):
        _lib.check(self._lib.cal_solver_timing_enable(self._h, int(bool(enable))))

    def timing_get(self):
        t = _lib.KernelTiming()
        _lib.check(self._lib.cal_solver_timing_get(self._h, C.byref(t)))
        return dict(launches=t.launches, total_ms=t.total_ms, algorithmic_bytes_per_launch=t.algorithmic_bytes_per_launch,
                    basis_bytes_per_launch=t.basis_bytes_per_launch, flops_per_launch=t.flops_per_launch,
                    kernel_path={_lib.CAL_PATH_GENERAL: "general", _lib.CAL_PATH_DENSE: "dense", _lib.CAL_PATH_DENSE_F32: "dense_f32", _lib.CAL_PATH_DENSE_SPLIT1: "dense_split1"}[t.kernel_path],
                    dense_wg_per_cu=t.dense_wg_per_cu, basis_folded=int(t.basis_folded))

    def memory_bytes(self):
        n = C.c_int64(0)
        _lib.check(self._lib.cal_solver_memory_bytes(self._h, C.byref(n)))
        return n.value

    def set_exchange_hook(self, all_reduce, rank: int, nranks: int):
        """Run the per-step exchange through ``all_reduce(array, op)`` instead of RCCL: ``array`` is a NumPy view (float32,
        float64 or int32) of the library's staging buffer, to be reduced IN PLACE over the ``nranks`` callers; ``op`` is
        "sum" or "min".  ``None`` detaches.  (cal_solver_set_exchange_hook)"""
        if all_reduce is None:
            self._hook = None
            _lib.check(self._lib.cal_solver_set_exchange_hook(self._h, None, None, 0, 1))
            return
        dtypes = {_lib.CAL_XCHG_F32: np.float32, _lib.CAL_XCHG_F64: np.float64, _lib.CAL_XCHG_I32: np.int32}

        def trampoline(ctx, buf, count, dtype, op):
            try:
                dt = np.dtype(dtypes[dtype])
                arr = np.frombuffer((C.c_char * (count * dt.itemsize)).from_address(buf), dtype=dt)
                all_reduce(arr, "min" if op == _lib.CAL_XCHG_MIN else "sum")
                return 0
            except Exception:  # noqa: BLE001 -- never unwind through the C frames: report failure to the library
                import traceback

                traceback.print_exc()
                return 1

        self._hook = _lib.EXCHANGE_FN(trampoline)  # keep the callback alive as long as the solver uses it
        _lib.check(self._lib.cal_solver_set_exchange_hook(self._h, C.cast(self._hook, C.c_void_p), None, int(rank), int(nranks)))

    def comm_size(self):
        """Ranks that take part in the exchange, counted by an all-reduce of ones over it (cal_solver_comm_size)."""
        n = C.c_int(0)
        _lib.check(self._lib.cal_solver_comm_size(self._h, C.byref(n)))
        return n.value

    def comm_init(self, unique_id: bytes, rank: int, nranks: int):
        buf = C.create_string_buffer(bytes(unique_id), _lib.CAL_COMM_ID_BYTES)
        _lib.check(self._lib.cal_solver_comm_init(self._h, buf, int(rank), int(nranks)))


def comm_unique_id() -> bytes:
    buf = C.create_string_buffer(_lib.CAL_COMM_ID_BYTES)
    _lib.check(_lib.load().cal_comm_unique_id(buf))
    return buf.raw
