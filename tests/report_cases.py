"""The table of cases behind tests/test_gpu_report_paths.py and tests/test_gpu_robust_reports.py: the six post-fit reports
(``fit_errors``, ``gain_basis_errors``, ``delay_spectrum``, ``delay_cross_spectrum``, ``delay_transfer``, ``fix_degeneracies``) on the smallest shapes that
qualify for the dense kernel paths (SHARED layout, one baseline per fitting group, more than 64 channels).  No GPU here: the inputs
of every case, the one call per case on a solver it is handed, the restatement of that call (the one of the report's own test file,
on the problem's weights or on others) and its ``check`` (the one of the report's own test file).  tests/test_report_paths_host.py
holds the table to its preconditions without a device.

The ``fix_degeneracies`` problem is ``base_problem(7)`` of tests/test_gpu_degeneracy.py at 72 channels; its reference is ``inject`` on
the fp64 NumPy model of the start parameters (an input like any other: the restatement is evaluated on the device's own model rows,
as in that file), modes ``channel`` and ``band``, 6 iterations, with ``gref``; ``_own_w``: ``ref_w=None``, the solver's weights.

The ``delay_cross`` cases are the spectrum's problem and operator with the pairs of ``single_slice_case`` of tests/test_gpu_delay_cross.py
(any two rows of ONE slice make a pair: (b, (b + 3) % nb) for every row, (2, 2) with unit scales, (nb - 1, 0), unequal scales elsewhere),
four bins, both statistics of all three quantities per pair; ``reference``, ``check`` and the bound are that file's."""
import copy
import functools

import numpy as np

import degeneracy_ref as R
import delay_spectrum_ref as DSR
import robust_ref
import test_gpu_degeneracy as DG
import test_gpu_delay_cross as DC
import test_gpu_delay_spectrum as DS
import test_gpu_delay_transfer as DT
import test_gpu_fit_errors as FE
import test_gpu_gain_basis_errors as GBE
from gain_basis_errors_ref import restated_errors
from test_gain_basis_errors_host import freq_case
from test_gain_time_solve_host import bases_of, flagged_case, rand_basis
from test_gpu_coeff_solve import COND_MAX
from test_gpu_fit_quality import edge_problem, plane_err
from test_gpu_fit_quality import restated as restated_quality

RIDGE = 1e-6
DEGEN_NF = 72
TIME_SHAPE = (4, 5, 72)
CASES = [("fit_errors", "7x200"), ("fit_errors", "12x129"), ("gain_basis_errors", "freq_K12"), ("gain_basis_errors", "freq_K65"),
         ("gain_basis_errors", "time_freq"), ("gain_basis_errors", "time"), ("delay_spectrum", "raw"), ("delay_spectrum", "calibrated"),
         ("delay_cross", "raw"), ("delay_cross", "calibrated"), ("delay_transfer", "raw"), ("delay_transfer", "calibrated"), ("fix_degeneracies", "channel"), ("fix_degeneracies", "band"),
         ("fix_degeneracies", "channel_own_w"), ("fix_degeneracies", "band_own_w")]
# the cases whose call reads the solver's weight plane (fix_degeneracies with ref_w given must not)
WEIGHT_READERS = [c for c in CASES if c[0] != "fix_degeneracies" or c[1].endswith("_own_w")]
GIVEN_REF_W = [c for c in CASES if c[0] == "fix_degeneracies" and not c[1].endswith("_own_w")]


def case_id(case):
    return "-".join(case)


@functools.lru_cache(maxsize=None)
def inputs(kind, variant):
    """(problem, params, frequency basis or None, time basis or None)."""
    if kind == "fit_errors":
        return edge_problem(*map(int, variant.split("x"))) + (None, None)
    if kind == "gain_basis_errors":
        if variant.startswith("freq_K"):
            return freq_case((7, 200)) + (rand_basis(200, int(variant[len("freq_K"):]), 2), None)
        Bt, B = bases_of(TIME_SHAPE, ("rand",), (3, 10 if variant == "time_freq" else None))
        return flagged_case(*TIME_SHAPE) + (B, Bt)
    if kind in ("delay_spectrum", "delay_cross", "delay_transfer"):
        return DS.problem(7, 200) + (None, None)
    return DG.base_problem(7, nfreqs=DEGEN_NF)[:2] + (None, None)


@functools.lru_cache(maxsize=None)
def degeneracy_args(variant):
    """(ref_r, ref_i, antpos, keywords) of the ``fix_degeneracies`` call, and the complex planes the restatement takes."""
    p, params, freqs, antpos = DG.base_problem(7, nfreqs=DEGEN_NF)
    mode = variant.split("_")[0]
    m = DSR.model_of(p, params["c_r"], params["c_i"], np.float64)
    ref_s, ref_w = DG.inject(m, p.bl_ant0, p.bl_ant1, antpos, freqs, seed=7, band=mode == "band")
    rng = np.random.default_rng(8)
    g = params["g_r"] + 1j * params["g_i"]
    gref = g * np.exp(1j * rng.uniform(-1, 1, size=DEGEN_NF))[None, :] * (1 + 0.05 * rng.normal(size=g.shape))
    kw = dict(ref_w=None if variant.endswith("_own_w") else ref_w, mode=mode, iters=6, freqs=freqs, gref_r=np.ascontiguousarray(gref.real),
              gref_i=np.ascontiguousarray(gref.imag))
    return np.ascontiguousarray(ref_s.real), np.ascontiguousarray(ref_s.imag), antpos, kw, ref_w


def delay_operator(kind, variant):
    return DS.operator(200, 200)


def cross_pairs(kind="delay_cross", variant="raw"):
    """(pairs, scale, bins, nbins) of the ``delay_cross`` cases."""
    return DC.single_slice_pairs(inputs(kind, variant)[0].nbls)


def call(s, kind, variant):
    """The one call of the case on the solver ``s``: what it returns (``fix_degeneracies``: with the solver's model rows beside it)."""
    p = inputs(kind, variant)[0]
    if kind == "fit_errors":
        return s.fit_errors(ridge=RIDGE)
    if kind == "gain_basis_errors":
        return s.gain_basis_errors(ridge=RIDGE)
    if kind == "delay_spectrum":
        op, norm_f = delay_operator(kind, variant)
        return DS.call(s, p, op, norm_f, calibrated=variant == "calibrated")
    if kind == "delay_cross":
        op, norm_f = delay_operator(kind, variant)
        pairs, scale, bins, nbins = cross_pairs(kind, variant)
        return s.delay_cross_spectrum(op, norm_f, pairs, scale=scale, calibrated=variant == "calibrated", bin_of_pair=bins, nbins=nbins, per_pair=True)
    if kind == "delay_transfer":
        return DT.call(s, p, delay_operator(kind, variant)[0], ridge=RIDGE, calibrated=variant == "calibrated")
    ref_r, ref_i, antpos, kw, _ = degeneracy_args(variant)
    out = s.fix_degeneracies(ref_r, ref_i, antpos, **kw)
    out["m_r"], out["m_i"] = s.model()
    return out


def flat(out):
    """Nested dicts of arrays (``per_baseline`` of ``delay_spectrum``; ``per_pair[stat][quantity]`` of ``delay_cross_spectrum``, two levels)
    as keys of their own, for a bit-for-bit comparison."""
    res = {}
    for k, v in out.items():
        if isinstance(v, dict):
            res.update({f"{k}_{kk}": vv for kk, vv in flat(v).items()})
        else:
            res[k] = v
    return res


def with_weights(p, w):
    """A copy of the problem ``p`` whose weights are ``w``."""
    q = copy.copy(p)
    q.wgts = np.asarray(w).astype(np.float64)
    return q


def host_model(kind, variant, dtype):
    p, params = inputs(kind, variant)[:2]
    return DSR.model_of(p, params["c_r"], params["c_i"], dtype)


def restatement(kind, variant, dtype, p=None, model=None):
    """The restatement of the case's call in fp64 NumPy on the inputs a solver of ``dtype`` holds.  ``p``: a copy of the problem with
    other weights (``with_weights``); ``model``: the model rows ``fix_degeneracies`` is restated on (the device's own), None: A c."""
    p0, params, B, Bt = inputs(kind, variant)
    p = p0 if p is None else p
    if kind == "fit_errors":
        return FE.restated(p, params, dtype, RIDGE)
    if kind == "gain_basis_errors":
        return restated_errors(p, params, dtype, Bt, B, RIDGE)
    if kind == "delay_spectrum":
        op, norm_f = delay_operator(kind, variant)
        return DS.reference(p, params, dtype, op, norm_f, variant == "calibrated")
    if kind == "delay_cross":
        op, norm_f = delay_operator(kind, variant)
        pairs, scale, bins, nbins = cross_pairs(kind, variant)
        return DC.reference(p, p, [params], dtype, op, norm_f, pairs, scale, variant == "calibrated", bins, nbins)
    if kind == "delay_transfer":
        return DT.reference(p, params, dtype, delay_operator(kind, variant)[0], ridge=RIDGE, calibrated=variant == "calibrated")
    ref_r, ref_i, antpos, kw, _ = degeneracy_args(variant)
    m = host_model(kind, variant, dtype) if model is None else model
    w = p.wgts if kw["ref_w"] is None else kw["ref_w"]
    return R.fix_degeneracies(m, DG.cast_c(ref_r, ref_i, dtype), np.asarray(w).astype(dtype).astype(np.float64), DG.cast_c(params["g_r"], params["g_i"], dtype),
                              p.bl_ant0, p.bl_ant1, antpos, iters=kw["iters"], mode=kw["mode"], freqs=kw["freqs"],
                              gref=DG.cast_c(kw["gref_r"], kw["gref_i"], dtype), dtype=dtype)


@functools.lru_cache(maxsize=None)
def reference(kind, variant, dtype_name):
    """``restatement`` on the problem's own weights (not for ``fix_degeneracies``, which is restated on the device's model rows)."""
    assert kind != "fix_degeneracies"
    return restatement(kind, variant, np.dtype(dtype_name).type)


def device_model(out):
    return out["m_r"].astype(np.float64) + 1j * out["m_i"].astype(np.float64)


def check(kind, variant, out, ref, dtype, label):
    """``out`` (as ``call`` returned it) against the restatement ``ref`` with the ``check`` and ``TOL`` of the report's own test file."""
    p = inputs(kind, variant)[0]
    if kind == "fit_errors":
        assert max(ref["conds"]) <= COND_MAX, label
        assert (out["nsolved"], out["nsingular"]) == (p.ngrps - len(ref["singular"]), len(ref["singular"])), (label, out["nsolved"], out["nsingular"])
        return FE.check_outputs(out, ref, dtype, label)
    if kind == "gain_basis_errors":
        return GBE.check(out, ref, dtype, label)
    if kind == "delay_spectrum":
        return DS.check(out, ref, p, dtype, label)
    if kind == "delay_cross":
        bins, nbins = cross_pairs(kind, variant)[2:]
        return DC.check(out, ref, dtype, label, bins=bins, nbins=nbins)
    if kind == "delay_transfer":
        assert max(ref["conds"]) <= COND_MAX, label
        return DT.check(out, ref, p, dtype, label)
    return DG.check_slice(out, 0, ref, dtype, label, p.nants, slice(None))


# ---- what the weights-matter precondition of the robust tests compares (planes of the restatement; the integers apart)
MATTER_PLANES = {"fit_errors": ("coeff_var", "model_var", "leverage_bl", "gain_var"), "gain_basis_errors": ("gain_var", "y_var", "gain_dof"),
                 "delay_spectrum": ("data", "model", "resid", "norm_bl"),
                 "delay_cross": tuple(f"{st}_{k}" for st in DC.STATS for k in DSR.NAMES) + ("norm_pair",), "delay_transfer": ("absorbed_bl", "noise_bl"),
                 "fix_degeneracies": ("eta", "tilt", "psi", "g", "model")}
# Outputs whose restatement does NOT move by 100 x TOL in fp32 under clip at k = 2 (it does in fp64, where TOL is 1e-10): a reader of w0
# could pass their comparison with the restatement, so in fp32 they are held to solver B alone (bit for bit).  Two are identities that
# hold whatever the weights are: the leverages of a fitting group of ONE baseline add up to tr(N N_r^-1) = nvec - O(ridge), and
# gain_dof = n - shift tr(N_r^-1) likewise (under the time basis alone the set of solved channels changes, and gain_dof with it).  The
# third is the band mode of fix_degeneracies: its reference is the model moved by (eta, Phi) plus 2 % noise, so one amplitude and one
# shift over 21 x 72 samples barely depend on which 18 % of them are clipped.  tests/test_report_paths_host.py asserts every entry
# (below the margin in fp32, above it in fp64) and that every other plane of every case is above it in both dtypes; measured there:
# leverage_bl 3.4e-6 (7x200) and 1.3e-4 (12x129), gain_dof 2.7e-8 / 2.2e-7 / 1.1e-7, band eta 3.7e-4, tilt 8.1e-4, model 7.0e-4,
# against a margin of 1e-2.
BELOW_MARGIN_FP32 = {("fit_errors", "7x200"): ("leverage_bl",), ("fit_errors", "12x129"): ("leverage_bl",), ("gain_basis_errors", "freq_K12"): ("gain_dof",),
                     ("gain_basis_errors", "freq_K65"): ("gain_dof",), ("gain_basis_errors", "time_freq"): ("gain_dof",),
                     ("fix_degeneracies", "band_own_w"): ("eta", "tilt", "model")}


def below_margin(case, dtype):
    return BELOW_MARGIN_FP32.get(tuple(case), ()) if np.dtype(dtype) == np.dtype(np.float32) else ()


def matter_planes(kind, ref):
    if kind == "delay_spectrum":
        return dict({k: ref["per_baseline"][k] for k in DSR.NAMES}, norm_bl=ref["norm_bl"])
    if kind == "delay_cross":
        return dict({f"{st}_{k}": ref["per_pair"][st][k] for st in DC.STATS for k in DSR.NAMES}, norm_pair=ref["norm_pair"])
    return {k: np.asarray(ref[k]) for k in MATTER_PLANES[kind]}


def chisq_of(kind, variant, dtype, p=None):
    p0, params = inputs(kind, variant)[:2]
    return float(restated_quality(p0 if p is None else p, params, dtype)["chisq_bl"].sum())


def sample_counts(kind, ref):
    """The integer output of the reports that have one: the number of samples with a non-zero (``fix_degeneracies``: positive) weight."""
    return {"fit_errors": lambda: ref["nsamp_bl"], "fix_degeneracies": lambda: ref["nsamples"]}.get(kind, lambda: None)()


def clipped_weights(kind, variant, dtype, how=("clip", 2.0)):
    """The weights of ``robust_ref`` for the case's problem at its start parameters, on the inputs a solver of ``dtype`` holds:
    (w, w0, fraction of the good samples with a smaller weight)."""
    p, params = inputs(kind, variant)[:2]
    cast = lambda a: np.asarray(a).astype(dtype).astype(np.float64)  # noqa: E731
    m = host_model(kind, variant, dtype)
    w0 = cast(p.wgts)
    e = robust_ref.residual_power(m.real, m.imag, cast(p.data_r), cast(p.data_i), w0, cast(params["g_r"]), cast(params["g_i"]), p.bl_ant0, p.bl_ant1)
    out = robust_ref.robust_weights(e, w0, *how)
    return out["w"], w0, float(out["ndown_bl"].sum() / np.count_nonzero(w0 > 0))


def margins(kind, variant, dtype, w, model=None):
    """How far the restatement under the weights ``w`` lies from the one under the problem's own: (planes' ``plane_err``, the
    chi-square's relative difference, new and old restatement)."""
    p = inputs(kind, variant)[0]
    new, old = restatement(kind, variant, dtype, with_weights(p, w), model), restatement(kind, variant, dtype, None, model)
    a, b = matter_planes(kind, new), matter_planes(kind, old)
    moved = {k: plane_err(a[k], b[k]) for k in a}
    c_new, c_old = chisq_of(kind, variant, dtype, with_weights(p, w)), chisq_of(kind, variant, dtype)
    return moved, abs(c_new - c_old) / c_old, new, old
