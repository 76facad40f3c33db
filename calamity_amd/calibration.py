"""Drop-in counterparts of the fit path of /root/reference/calamity/calibration.py, running on the MI355X HIP
library (include/calamity_hip.h) instead of TensorFlow.

Same function names, argument meaning and error behaviour as the reference for the gain + foreground
gradient-descent fitter: ``calibrate_and_model_dpss`` (:1503-1584) -> ``calibrate_and_model_tensor`` (:963-1331)
-> ``fit_gains_and_foregrounds`` (:447-738).  Differences a user can observe:

* tensors are NumPy arrays, and the foreground components are kept ragged (``problem.FitProblem``: true vector counts,
  identical basis blocks stored once) instead of one zero-padded ``(nvecs, ngrps, nbls, nfreqs)`` tensor per chunk
  (:140-146, :167); ``fg_comps`` arguments accept either form;
* ``graph_mode`` / ``graph_args_dict`` are accepted and ignored (there is no tracing compiler on this path);
* ``n_profile_steps`` writes HIP-event kernel timings as JSON into ``profile_log_dir`` instead of a TF profile;
* optimizers: the whole ``OPTIMIZERS`` table (:17-27) -- "Adamax", "Adam", "SGD", "RMSprop", "Adagrad", "Adadelta", "Nadam", "Ftrl" with
  the Keras (OptimizerV2) semantics, defaults and constructor arguments, "LAMB" with those of tensorflow-addons; every other name
  raises ``KeyError`` like ``OPTIMIZERS[...]`` (:571).

There is no CPU fallback: without the HIP library / a GPU these functions raise.
"""
import argparse
import collections
import concurrent.futures
import copy
import datetime
import os
import threading
import types

import numpy as np

from . import cal_utils, modeling, slice_pipeline, utils
from .fit_loop import KEYWORD_HELP, FitControls, drive, history_entry
from .slice_pipeline import init_coeffs as _init_coeffs, slice_stats as _slice_stats  # noqa: F401 -- (names kept here for tools and tests)
from .problem import FitProblem, coeffs_from_chunks, coeffs_to_chunks, problem_from_chunks
from .solver import OPTIMIZERS, HipFitSolver
from .utils import PBARS, echo
from .uvcompat import gain4, is_uvcal, is_uvdata, polstr2num, vis3


# ------------------------------------------------------------------------------------------------------------------
# layout: calibration.py:30-190
# ------------------------------------------------------------------------------------------------------------------
def chunk_fg_comp_dict_by_nbls(fg_model_comps_dict, use_redundancy=False, grp_size_threshold=5):
    """Group fitting groups into chunks keyed ``(nbl, maxvecs)`` -- behaviour of calibration.py:30-101.

    Without ``use_redundancy`` a fitting group whose redundant groups all have the same length (and that has fewer
    than ``grp_size_threshold`` of them) is split into one fitting group per redundant copy, all sharing the same
    modeling vectors (:69-81).
    """
    comps = dict(fg_model_comps_dict)
    if not use_redundancy:
        # The reference pops every group it splits and appends the pieces (:73-81) -- a single baseline is "split" into itself, i.e. moved
        # to the end.  Same order here (it fixes the layout of fg_model_comps, corr_inds and the coefficient arrays): the groups that stay
        # whole first, then the pieces in the order of their groups; without 61 075 pops and re-inserts for HERA-350's single baselines.
        kept, moved = {}, {}
        for fit_grp, vectors in comps.items():
            if len(fit_grp) == 1 and len(fit_grp[0]) == 1:
                moved[fit_grp] = vectors  # one baseline: its only piece is itself
                continue
            rlens = np.asarray([len(red_grp) for red_grp in fit_grp])
            if np.allclose(rlens, np.mean(rlens)) and len(rlens) < grp_size_threshold:
                for rednum in range(int(rlens[0])):
                    moved[tuple((red_grp[rednum],) for red_grp in fit_grp)] = vectors
            else:
                kept[fit_grp] = vectors
        comps = {**kept, **moved}
    by_nbl, maxvecs = {}, {}
    for fit_grp, vectors in comps.items():
        nbl = sum(len(red_grp) for red_grp in fit_grp)
        by_nbl.setdefault(nbl, []).append(fit_grp)
        maxvecs[nbl] = max(maxvecs.get(nbl, 0), vectors.shape[1])
    return {(nbl, maxvecs[nbl]): {k: comps[k] for k in grps} for nbl, grps in by_nbl.items()}


def tensorize_fg_model_comps_dict(
    fg_model_comps_dict,
    ants_map,
    nfreqs,
    use_redundancy=False,
    dtype=np.float32,
    notebook_progressbar=False,
    verbose=False,
    grp_size_threshold=5,
):
    """Modeling-component dictionary -> (ragged ``FitProblem`` without data, ``corr_inds``).

    Counterpart of calibration.py:104-190.  ``corr_inds[chunk][group][baseline] = (i, j)`` is built exactly like the
    reference (:169-188); the components are NOT expanded into the zero-padded ``(nvecs, ngrps, nbls, nfreqs)``
    tensor (:167): each group keeps its own vector count and arrays that are the same object in the dictionary
    (the operator cache of modeling.py:291-301) are stored once.
    """
    echo(f"{datetime.datetime.now()} Computing foreground components matrices...\n", verbose=verbose)
    chunked = chunk_fg_comp_dict_by_nbls(fg_model_comps_dict, use_redundancy=use_redundancy, grp_size_threshold=grp_size_threshold)
    basis, basis_id = [], {}
    grp_basis, grp_bl_start = [], [0]
    bl_ant0, bl_ant1, bl_rowblk = [], [], []
    corr_inds, chunk_of_grp, pos_in_chunk, chunk_shapes = [], [], [], []
    for cnum, (nbls, nvecs) in enumerate(chunked):
        corr_inds_chunk = []
        for grpnum, (modeling_grp, vectors) in enumerate(chunked[(nbls, nvecs)].items()):
            if vectors.shape[0] != len(modeling_grp) * nfreqs:
                raise ValueError(
                    f"modeling vectors of a fitting group with {len(modeling_grp)} redundant groups must have "
                    f"{len(modeling_grp) * nfreqs} rows, got {vectors.shape[0]}"
                )
            if id(vectors) not in basis_id:
                basis_id[id(vectors)] = len(basis)
                basis.append(np.ascontiguousarray(vectors, dtype=np.float64))
            grp_basis.append(basis_id[id(vectors)])
            corr_inds_grp = []
            for rgrpnum, red_grp in enumerate(modeling_grp):
                for ap in red_grp:
                    i, j = ants_map[ap[0]], ants_map[ap[1]]
                    corr_inds_grp.append((i, j))
                    bl_ant0.append(i)
                    bl_ant1.append(j)
                    bl_rowblk.append(rgrpnum)
            grp_bl_start.append(grp_bl_start[-1] + len(corr_inds_grp))
            corr_inds_chunk.append(corr_inds_grp)
            chunk_of_grp.append(cnum)
            pos_in_chunk.append(grpnum)
        corr_inds.append(corr_inds_chunk)
        chunk_shapes.append((nvecs, len(corr_inds_chunk), nbls))
    nbl_total = len(bl_ant0)
    fg_model_comps = FitProblem(
        nants=len(ants_map),
        nfreqs=int(nfreqs),
        basis=basis,
        grp_basis=np.asarray(grp_basis, dtype=np.int32),
        grp_bl_start=np.asarray(grp_bl_start, dtype=np.int32),
        bl_ant0=np.asarray(bl_ant0, dtype=np.int32),
        bl_ant1=np.asarray(bl_ant1, dtype=np.int32),
        bl_rowblk=np.asarray(bl_rowblk, dtype=np.int32),
        data_r=None,
        data_i=None,
        wgts=None,
        chunk_of_grp=np.asarray(chunk_of_grp, dtype=np.int32),
        pos_in_chunk=np.asarray(pos_in_chunk, dtype=np.int32),
        chunk_shapes=chunk_shapes,
    )
    assert nbl_total == fg_model_comps.nbls
    return fg_model_comps, corr_inds


# ------------------------------------------------------------------------------------------------------------------
# data / gains <-> arrays: calibration.py:193-399
# ------------------------------------------------------------------------------------------------------------------
def _baseline_rows(uvdata, prob, ants_map, time):
    """Row of every baseline of ``prob`` in the blt axis of ``uvdata`` at ``time``, and whether the data hold the pair in the
    reversed order (then the conjugate is wanted, calibration.py:263-278) -- by one (antenna, antenna) -> row table instead of a
    dictionary lookup per baseline.  KeyError if a pair is in the data in neither order, like ``_key2inds``."""
    cache = prob.__dict__.setdefault("_row_cache", {})
    key = (id(uvdata), float(time), int(getattr(uvdata, "Nblts", 0)))
    hit = cache.get(key)
    if hit is not None and hit[0] is uvdata:
        return hit[1], hit[2]
    tsel = np.where(np.isclose(np.asarray(uvdata.time_array), time, rtol=0.0, atol=1e-7))[0]
    nants = len(ants_map)
    lut_keys = np.fromiter(ants_map.keys(), dtype=np.int64, count=nants)
    lut_vals = np.fromiter(ants_map.values(), dtype=np.int64, count=nants)
    order = np.argsort(lut_keys)
    a1 = np.asarray(uvdata.ant_1_array)[tsel].astype(np.int64)
    a2 = np.asarray(uvdata.ant_2_array)[tsel].astype(np.int64)

    def to_index(a):  # antenna number -> index of ants_map (-1: not a gain antenna)
        pos = np.clip(np.searchsorted(lut_keys[order], a), 0, nants - 1)
        ok = lut_keys[order][pos] == a
        return np.where(ok, lut_vals[order][pos], -1)

    i1, i2 = to_index(a1), to_index(a2)
    ok = (i1 >= 0) & (i2 >= 0)
    table = np.full((nants, nants), -1, dtype=np.int64)
    table[i1[ok], i2[ok]] = tsel[ok]
    b0, b1 = np.asarray(prob.bl_ant0, dtype=np.int64), np.asarray(prob.bl_ant1, dtype=np.int64)
    rows = table[b0, b1]
    conj = rows < 0
    if conj.any():
        rows = np.where(conj, table[b1, b0], rows)
        if (rows < 0).any():
            n = int(np.where(rows < 0)[0][0])
            inv = {v: k for k, v in ants_map.items()}
            raise KeyError((inv[int(b0[n])], inv[int(b1[n])]))
    if len(cache) > 64:
        cache.clear()
    cache[key] = (uvdata, rows, conj)
    return rows, conj


def _time_ind(times, inds, time):
    return inds[np.where(np.isclose(np.asarray(times)[inds], time, rtol=0.0, atol=1e-7))[0][0]]


class _Baselines:
    """The antenna index pairs of ``corr_inds`` as flat arrays, in chunk -> group -> baseline order (= the ragged baseline order
    of the FitProblem built from the same dictionary)."""

    def __init__(self, corr_inds):
        pairs = [np.asarray(chunk, dtype=np.int64).reshape(-1, 2) for chunk in corr_inds]
        flat = np.concatenate(pairs) if len(pairs) else np.zeros((0, 2), dtype=np.int64)
        self.bl_ant0, self.bl_ant1 = flat[:, 0], flat[:, 1]
        self.shapes = [(len(chunk), len(chunk[0])) for chunk in corr_inds]


def _baselines_of(corr_inds):
    hit = _baselines_of.cache.get(id(corr_inds))
    if hit is None or hit[0] is not corr_inds:
        if len(_baselines_of.cache) > 16:
            _baselines_of.cache.clear()
        hit = (corr_inds, _Baselines(corr_inds))
        _baselines_of.cache[id(corr_inds)] = hit
    return hit[1]


_baselines_of.cache = {}


def _tensorize_flat(uvdata, bls, ants_map, polarization, time, data_scale_factor=1.0, weights=None, nsamples_in_weights=False,
                    dtype=np.float32, want_weights=True):
    """The arithmetic of tensorize_data (calibration.py:193-310) on flat ``(nbls, nfreqs)`` arrays in the baseline order of
    ``bls`` (a FitProblem or _Baselines): data of a pair that only exists in reversed order are conjugated (:263-278); weights
    are ``~flags`` (``* nsamples`` / ``* UVFlag.weights``) divided by their sum over ALL baselines and channels (:282-303).
    Returns (data_r, data_i, wgts or None)."""
    rows, conj = _baseline_rows(uvdata, bls, ants_map, time)
    pols = np.asarray(uvdata.polarization_array)
    polnum = polstr2num(polarization, x_orientation=uvdata.x_orientation)
    swap = {-7: -8, -8: -7, -3: -4, -4: -3}  # conjugating swaps the feeds of cross-hand products
    pind = int(np.where(pols == polnum)[0][0])
    pind_conj = np.where(pols == swap.get(polnum, polnum))[0]
    any_conj = bool(conj.any())
    if any_conj and len(pind_conj) == 0:
        raise KeyError(f"polarization {polarization}: the conjugate product is not in the data")
    if weights is not None and want_weights:
        wrows, _ = _baseline_rows(weights, bls, ants_map, time)
        wpol = int(np.where(np.asarray(weights.polarization_array) == polstr2num(polarization, x_orientation=weights.x_orientation))[0][0])
    nb, nf = len(rows), uvdata.Nfreqs
    d_r = np.empty((nb, nf), dtype=dtype)
    d_i = np.empty((nb, nf), dtype=dtype)
    w = np.empty((nb, nf), dtype=dtype) if want_weights else None
    vis, flg = vis3(np.asarray(uvdata.data_array)), vis3(np.asarray(uvdata.flag_array))
    nsm = vis3(np.asarray(uvdata.nsample_array)) if (nsamples_in_weights and want_weights) else None
    wts = vis3(np.asarray(weights.weights_array)) if (weights is not None and want_weights) else None
    row_sums = np.zeros(nb, dtype=np.float64)  # per baseline: the total below does not depend on how the rows are chunked

    def rows_chunk(lo, hi):
        # gather + scale + split of a run of baselines (memory-bound NumPy passes: one thread per run, utils.for_row_chunks)
        r, cj = rows[lo:hi], conj[lo:hi]
        # (row gathers with np.take from the polarization's plane: NumPy's fancy indexing with two index arrays around a
        # slice is an order of magnitude slower on complex data)
        data = np.take(vis[:, :, pind], r, axis=0)
        if any_conj and cj.any():  # pairs held in the reversed order: the conjugate product's column, conjugated
            pc = int(pind_conj[0])
            data[cj] = np.take(vis[:, :, pc], r[cj], axis=0)
        data /= data_scale_factor
        d_r[lo:hi] = data.real
        d_i[lo:hi] = data.imag
        if any_conj:
            d_i[lo:hi][cj] *= -1
        if not want_weights:
            return
        keep = ~np.take(flg[:, :, pind], r, axis=0)
        ns = np.take(nsm[:, :, pind], r, axis=0) if nsm is not None else None
        if any_conj and cj.any():
            pc = int(pind_conj[0])
            keep[cj] = ~np.take(flg[:, :, pc], r[cj], axis=0)
            if ns is not None:
                ns[cj] = np.take(nsm[:, :, pc], r[cj], axis=0)
        ww = keep.astype(dtype) if wts is None else np.take(wts[:, :, wpol], wrows[lo:hi], axis=0).astype(dtype) * keep
        if ns is not None:
            ww = ww * ns
        w[lo:hi] = ww
        row_sums[lo:hi] = np.sum(w[lo:hi], axis=1, dtype=np.float64)

    utils.for_row_chunks(rows_chunk, nb)
    if want_weights:
        wgtsum = float(np.sum(row_sums))
        w = (w / wgtsum).astype(dtype)
    return d_r, d_i, w


def tensorize_data(
    uvdata,
    corr_inds,
    ants_map,
    polarization,
    time,
    data_scale_factor=1.0,
    weights=None,
    nsamples_in_weights=False,
    dtype=np.float32,
):
    """UVData -> per-chunk ``(ngrps, nbls, nfreqs)`` arrays ``data_r, data_i, wgts`` -- calibration.py:193-310.

    Data of a pair that only exists in reversed order are conjugated (:263-278); weights are ``~flags``
    (``* nsamples`` / ``* UVFlag.weights``) divided by their sum over ALL baselines and channels (:282-303).
    """
    bls = _baselines_of(corr_inds)
    d_r, d_i, w = _tensorize_flat(uvdata, bls, ants_map, polarization, time, data_scale_factor=data_scale_factor, weights=weights,
                                  nsamples_in_weights=nsamples_in_weights, dtype=dtype)
    data_r, data_i, wgts, lo = [], [], [], 0
    nf = uvdata.Nfreqs
    for ngrps, nbls in bls.shapes:
        hi = lo + ngrps * nbls
        data_r.append(d_r[lo:hi].reshape(ngrps, nbls, nf))
        data_i.append(d_i[lo:hi].reshape(ngrps, nbls, nf))
        wgts.append(w[lo:hi].reshape(ngrps, nbls, nf))
        lo = hi
    return data_r, data_i, wgts


def tensorize_gains(uvcal, polarization, time, dtype=np.float32):
    """UVCal -> ``(Nants, Nfreqs)`` real and imaginary gain arrays -- calibration.py:369-399."""
    polnum = np.where(np.asarray(uvcal.jones_array) == polstr2num(polarization, x_orientation=uvcal.x_orientation))[0][0]
    gindt = np.where(np.isclose(uvcal.time_array, time, atol=1e-7, rtol=0.0))[0][0]
    g = gain4(uvcal.gain_array)[:, :, gindt, polnum]
    return np.ascontiguousarray(g.real, dtype=dtype), np.ascontiguousarray(g.imag, dtype=dtype)


def renormalize(uvdata_reference_model, uvdata_deconv, gains, polarization, time, additional_flags=None):
    """Remove the arbitrary amplitude of the deconvolved model and gains -- calibration.py:313-366 (the phase factor is
    computed by the reference but deliberately not applied, :359).  Modifies ``uvdata_deconv`` and ``gains``.
    ``scale = sqrt(nanmean |reference / deconvolved|^2)`` over the samples no flag array marks, non-finite ratios left out
    (:355-358) -- accumulated baseline by baseline on the host's cores instead of through three boolean-indexed copies of the slice."""
    polnum_data = np.where(uvdata_deconv.polarization_array == polstr2num(polarization, x_orientation=uvdata_deconv.x_orientation))[0][0]
    rows = np.where(np.isclose(uvdata_deconv.time_array, time, atol=1e-7, rtol=0.0))[0]
    dec, dflag = vis3(uvdata_deconv.data_array), vis3(uvdata_deconv.flag_array)
    ref, rflag = vis3(np.asarray(uvdata_reference_model.data_array)), vis3(np.asarray(uvdata_reference_model.flag_array))
    aflag = vis3(np.asarray(additional_flags)) if additional_flags is not None else None
    ssq = np.zeros(len(rows), dtype=np.float64)
    cnt = np.zeros(len(rows), dtype=np.int64)

    def chunk(lo, hi):
        r = rows[lo:hi]
        sel = ~(np.take(dflag[:, :, polnum_data], r, axis=0) | np.take(rflag[:, :, polnum_data], r, axis=0))
        if aflag is not None:
            sel &= ~np.take(aflag[:, :, polnum_data], r, axis=0)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.take(ref[:, :, polnum_data], r, axis=0) / np.take(dec[:, :, polnum_data], r, axis=0)
            p = ratio.real * ratio.real + ratio.imag * ratio.imag
        sel &= np.isfinite(ratio.real) & np.isfinite(ratio.imag)  # data_ratio[~isfinite] = nan, then nanmean (:355-358)
        ssq[lo:hi] = np.sum(np.where(sel, p, 0.0), axis=1)
        cnt[lo:hi] = np.count_nonzero(sel, axis=1)

    utils.for_row_chunks(chunk, len(rows))
    n = int(cnt.sum())
    with np.errstate(divide="ignore", invalid="ignore"):
        scale_factor = np.sqrt(np.float64(ssq.sum()) / n) if n else np.float64("nan")

    def scale(lo, hi):
        dec[rows[lo:hi], :, polnum_data] *= scale_factor

    utils.for_row_chunks(scale, len(rows))
    polnum_gains = np.where(np.asarray(gains.jones_array) == polstr2num(polarization, x_orientation=uvdata_deconv.x_orientation))[0][0]
    gindt = np.where(np.isclose(gains.time_array, time, atol=1e-7, rtol=0.0))[0][0]
    gains.gain_array[..., gindt, polnum_gains] *= (scale_factor) ** -0.5


# ------------------------------------------------------------------------------------------------------------------
# the solver behind a set of components
# ------------------------------------------------------------------------------------------------------------------
def _as_problem(fg_comps, corr_inds, nants):
    """Accept the ragged FitProblem or the reference's list of zero-padded chunk tensors."""
    if isinstance(fg_comps, FitProblem):
        return fg_comps
    if corr_inds is None:  # antenna indices are irrelevant to the caller (coefficient initialisation)
        corr_inds = [[[(0, 0)] * np.asarray(c).shape[2] for _ in range(np.asarray(c).shape[1])] for c in fg_comps]
        nants = 1
    dummy = [np.zeros(np.asarray(c).shape[1:]) for c in fg_comps]
    prob = problem_from_chunks(nants, fg_comps, corr_inds, dummy, dummy, dummy)
    prob.data_r = prob.data_i = prob.wgts = None
    return prob


def _flatten(chunks, prob):
    """Per-chunk ``(ngrps, nbls, nfreqs)`` arrays -> ``(nbls_total, nfreqs)`` in the ragged baseline order."""
    return np.concatenate([np.asarray(c).reshape(-1, prob.nfreqs) for c in chunks])


# device selection of the file driver (calibration.py:1741-1753): which GPU the solvers are created on, and a cap on
# the device memory one fit may take
_DEVICE = {"index": None, "memory_limit_gib": None}


def _wake_device(devices=None):
    """Start the HIP runtime on the devices a fit is going to use, on a thread of its own: the first HIP call of a process costs
    0.2 s (runtime start-up, device properties), and the entry points have half a second of host work -- the modeling components
    -- in front of their first solver.  Nothing depends on the thread: the fit creates its solvers as ever (and fails there,
    loudly, when there is no usable device).  Returns the thread; the entry points join it before they return or raise (it has
    long finished by then), so that it never outlives their call."""
    from . import _lib

    def wake():
        try:
            for d in (range(_lib.device_count()) if devices == "all" else devices) or [_DEVICE["index"] or 0]:
                _lib.device_info(int(d))
                HipFitSolver(dtype=np.float32, device=int(d)).close()  # (a stream on the device: its queues exist afterwards)
        except Exception:  # noqa: BLE001 -- reported by the solver that needs the device
            pass

    t = threading.Thread(target=wake, daemon=True)
    t.start()
    return t


def get_solver(fg_model_comps, dtype=np.float32, layout=None, device=None):
    """The HipFitSolver that holds these components on the GPU (created once per component set and dtype)."""
    dtype = np.dtype(dtype)
    cache = fg_model_comps.__dict__.setdefault("_solvers", {})
    # (a caller's explicit choice -- calibrate_and_model_tensor(layout=..., devices=[...]) -- travels with the components)
    layout = layout or fg_model_comps.__dict__.get("_layout") or "shared"
    if device is None:
        device = fg_model_comps.__dict__.get("_device")
    if device is None:
        device = _DEVICE["index"] if _DEVICE["index"] is not None else 0
    # one solver per calling thread: a handle is not re-entrant, and concurrent fits of different (pol, time) slices
    # (calibrate_and_model_tensor, parallel_fits > 1) each need their own device buffers and stream
    key = (dtype.str, layout, device, threading.get_ident())
    if key not in cache:
        shell = copy.copy(fg_model_comps)
        shell.data_r = shell.data_i = shell.wgts = None
        solver = HipFitSolver(dtype=dtype, device=device)
        solver.set_problem(shell, layout=layout)
        limit = _DEVICE["memory_limit_gib"]
        if limit is not None and solver.memory_bytes() > limit * 2.0**30:
            used = solver.memory_bytes() / 2.0**30
            solver.close()
            raise MemoryError(f"the fit needs {used:.2f} GiB of device memory, gpu_memory_limit is {limit} GiB")
        cache[key] = solver
    return cache[key]


def tensorize_fg_coeffs(data, wgts, fg_model_comps, notebook_progressbar=False, verbose=False, dtype=None):
    """Initial foreground coefficients of ONE real component by per-group linear least squares on ``data`` with
    zero-weight samples zeroed -- calibration.py:828-913.  Returns the reference's list of ``(nvecs, ngrps, 1, 1)``
    zero-padded arrays."""
    echo(f"{datetime.datetime.now()} Computing initial foreground coefficient guesses using linear-leastsq...\n", verbose=verbose)
    dtype = np.dtype(dtype or np.asarray(data[0]).dtype)
    prob = _as_problem(fg_model_comps, None, None)
    solver = get_solver(prob, dtype)
    src = _flatten(data, prob)
    zeros = np.zeros_like(src)
    solver.set_data(zeros, zeros, _flatten(wgts, prob))
    c_r, _ = _init_coeffs(solver, prob, src, zeros)
    echo(f"{datetime.datetime.now()} Finished initial foreground coefficient guesses...\n", verbose=verbose)
    return coeffs_to_chunks(prob, c_r, dtype)


def yield_fg_model_array(nants, nfreqs, fg_model_comps, fg_coeffs, corr_inds, dtype=np.float32):
    """Foreground model ``sum_k c_k A_k`` of ONE real component as a ``(nants, nants, nfreqs)`` float64 cube --
    calibration.py:402-444 (the A c product runs on the GPU)."""
    prob = _as_problem(fg_model_comps, corr_inds, nants)
    solver = get_solver(prob, dtype)
    c = coeffs_from_chunks(prob, fg_coeffs)
    solver.set_params(c_r=c, c_i=np.zeros_like(c))
    m_r, _ = solver.model()
    model = np.zeros((nants, nants, nfreqs))
    model[prob.bl_ant0, prob.bl_ant1] = m_r
    return model


# ------------------------------------------------------------------------------------------------------------------
# the fit loop: calibration.py:447-738
# ------------------------------------------------------------------------------------------------------------------
# ------------------------------------------------------------------------------------------------------------------
# The reference's graph functions under their own names and signatures (calibration.py:1587-1656), on NumPy arrays in the
# reference's zero-padded chunk layout -- fg_comps[chunk]: (nvecs, ngrps, nbls, nfreqs); fg_r / fg_i[chunk]: (nvecs, ngrps, 1, 1);
# data / weights[chunk]: (ngrps, nbls, nfreqs); ant0_inds / ant1_inds[chunk]: (ngrps, nbls).  Every one of them is evaluated by the
# HIP library (the fused kernels of the fit in their loss-only / model form); the fit itself never calls them -- it runs forward,
# adjoints and update without materialising a model.
_GRAPH_SOLVERS = []  # [(key, arrays kept alive, FitProblem)]: the last few chunk sets seen, so that repeated calls reuse the uploaded basis


def _fingerprint(a):
    """Shape, dtype and a strided checksum (at most ~4096 samples): enough to notice a component tensor that was modified in place
    between two calls, cheap beside the upload it guards."""
    a = np.asarray(a)
    flat = a.reshape(-1)
    step = max(1, flat.size // 4096)
    return (a.shape, a.dtype.str, float(np.sum(flat[::step], dtype=np.float64)), float(flat[-1]) if flat.size else 0.0)


def _graph_problem(fg_comps, ant0_inds, ant1_inds, nants):
    # (the component tensors by identity AND a content fingerprint -- they are kept alive below, but a caller may write into them --,
    # the small index arrays by content)
    key = (tuple((id(c), _fingerprint(c)) for c in fg_comps), tuple(np.asarray(a, dtype=np.int64).tobytes() for a in ant0_inds),
           tuple(np.asarray(a, dtype=np.int64).tobytes() for a in ant1_inds), int(nants))
    for k, _, prob in _GRAPH_SOLVERS:
        if k == key:
            return prob
    corr_inds = [[[(int(i), int(j)) for i, j in zip(r0, r1)] for r0, r1 in zip(np.asarray(a0), np.asarray(a1))] for a0, a1 in zip(ant0_inds, ant1_inds)]
    prob = _as_problem(list(fg_comps), corr_inds, int(nants))
    _GRAPH_SOLVERS.append((key, list(fg_comps), prob))
    while len(_GRAPH_SOLVERS) > 4:
        _, _, old = _GRAPH_SOLVERS.pop(0)
        for sv in old.__dict__.get("_solvers", {}).values():
            sv.close()
    return prob


def _graph_dtype(*arrays):
    return np.dtype(np.float64) if any(np.asarray(a).dtype == np.float64 for a in arrays) else np.dtype(np.float32)


def fg_model(fg_r, fg_i, fg_comps):
    """Foreground model of ONE chunk, ``v = sum_vec fg * fg_comps`` separately for re and im (calibration.py:1587-1590):
    ``(vr, vi)``, each ``(ngrps, nbls, nfreqs)``."""
    fg_comps = np.asarray(fg_comps)
    _, ngrps, nbls, nfreqs = fg_comps.shape
    zeros = np.zeros((ngrps, nbls), dtype=np.int64)
    prob = _graph_problem([fg_comps], [zeros], [zeros], 1)
    solver = get_solver(prob, _graph_dtype(fg_comps, fg_r))
    solver.set_params(None, None, coeffs_from_chunks(prob, [np.asarray(fg_r)]), coeffs_from_chunks(prob, [np.asarray(fg_i)]))
    vr, vi = solver.model()
    return vr.reshape(ngrps, nbls, nfreqs), vi.reshape(ngrps, nbls, nfreqs)


def data_model(g_r, g_i, fg_r, fg_i, fg_comps, ant0_inds, ant1_inds):
    """Model visibilities of ONE chunk: the foreground model times ``g_ant0 conj(g_ant1)`` (calibration.py:1593-1605):
    ``(model_r, model_i)``, each ``(ngrps, nbls, nfreqs)``."""
    fg_comps, g_r, g_i = np.asarray(fg_comps), np.asarray(g_r), np.asarray(g_i)
    _, ngrps, nbls, nfreqs = fg_comps.shape
    prob = _graph_problem([fg_comps], [ant0_inds], [ant1_inds], g_r.shape[0])
    solver = get_solver(prob, _graph_dtype(fg_comps, g_r))
    solver.set_params(g_r, g_i, coeffs_from_chunks(prob, [np.asarray(fg_r)]), coeffs_from_chunks(prob, [np.asarray(fg_i)]))
    m_r, m_i = solver.data_model()
    return m_r.reshape(ngrps, nbls, nfreqs), m_i.reshape(ngrps, nbls, nfreqs)


def mse(model_r, model_i, data_r, data_i, wgts):
    """``sum(w ((d_r - m_r)^2 + (d_i - m_i)^2))`` (calibration.py:1608-1609) -- cal_weighted_square_error on the device."""
    import ctypes as C

    from . import _lib

    dtype = _graph_dtype(model_r, data_r, wgts)
    arrs = [np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=dtype), np.shape(data_r))).ravel() for a in (model_r, model_i, data_r, data_i, wgts)]
    out = C.c_double(0.0)
    device = _DEVICE["index"] if _DEVICE["index"] is not None else 0
    _lib.check(_lib.load().cal_weighted_square_error(int(device), _lib.CAL_F64 if dtype == np.float64 else _lib.CAL_F32, arrs[0].size,
                                                     *[a.ctypes.data_as(C.c_void_p) for a in arrs], C.byref(out)))
    return dtype.type(out.value)


def _graph_loss(g_r, g_i, fg_r, fg_i, fg_comps, nchunks, data_r, data_i, wgts, ant0_inds, ant1_inds, dtype, priors=None):
    g_r = np.asarray(g_r)
    dtype = np.dtype(dtype)
    prob = _graph_problem(list(fg_comps)[:nchunks], list(ant0_inds)[:nchunks], list(ant1_inds)[:nchunks], g_r.shape[0])
    solver = get_solver(prob, dtype)
    solver.set_data(_flatten(list(data_r)[:nchunks], prob), _flatten(list(data_i)[:nchunks], prob), _flatten(list(wgts)[:nchunks], prob))
    solver.set_params(g_r, np.asarray(g_i), coeffs_from_chunks(prob, list(fg_r)[:nchunks]), coeffs_from_chunks(prob, list(fg_i)[:nchunks]))
    if priors is None:
        solver.set_regularization(None)
    else:
        solver.set_regularization("sum", float(priors[0]), float(priors[1]))
    return dtype.type(solver.eval_loss())


def mse_chunked(g_r, g_i, fg_r, fg_i, fg_comps, nchunks, data_r, data_i, wgts, ant0_inds, ant1_inds, dtype=np.float32):
    """The loss of the fit: ``sum_chunks mse(data_model(...))`` (calibration.py:1612-1620) -- one loss-only pass of the fused kernel."""
    return _graph_loss(g_r, g_i, fg_r, fg_i, fg_comps, nchunks, data_r, data_i, wgts, ant0_inds, ant1_inds, dtype)


def mse_chunked_sum_regularized(
    g_r,
    g_i,
    fg_r,
    fg_i,
    fg_comps,
    nchunks,
    data_r,
    data_i,
    wgts,
    ant0_inds,
    ant1_inds,
    prior_r_sum,
    prior_i_sum,
    dtype=np.float32,
):
    """``mse_chunked + (sum w m_r - prior_r_sum)^2 + (sum w m_i - prior_i_sum)^2`` (calibration.py:1623-1656)."""
    return _graph_loss(g_r, g_i, fg_r, fg_i, fg_comps, nchunks, data_r, data_i, wgts, ant0_inds, ant1_inds, dtype, priors=(prior_r_sum, prior_i_sum))


def fit_gains_and_foregrounds(
    g_r,
    g_i,
    fg_r,
    fg_i,
    data_r,
    data_i,
    wgts,
    fg_comps,
    corr_inds,
    use_min=False,
    tol=1e-14,
    maxsteps=10000,
    optimizer="Adamax",
    freeze_model=False,
    verbose=False,
    notebook_progressbar=False,
    dtype=np.float32,
    graph_mode=False,
    n_profile_steps=0,
    profile_log_dir="./logdir",
    sky_model_r=None,
    sky_model_i=None,
    model_regularization=None,
    graph_args_dict=None,
    gain_basis=None,
    gain_solve_sweeps=0,
    gain_solve_every=0,
    gain_solve_damping=0.5,
    coeff_solve_rounds=0,
    coeff_solve_ridge=1e-6,
    gain_basis_solve_sweeps=0,
    gain_basis_solve_every=0,
    gain_basis_solve_damping=0.5,
    gain_basis_solve_ridge=1e-6,
    gain_time_solve_sweeps=0,
    gain_time_solve_every=0,
    gain_time_solve_damping=0.5,
    gain_time_solve_ridge=1e-6,
    robust_every=0,
    robust_rounds=0,
    robust_kind="huber",
    robust_threshold=3.0,
    gauss_newton_rounds=0,
    gauss_newton_every=0,
    gauss_newton_cg_iters=20,
    gauss_newton_lambda=1e-3,
    gauss_newton_cg_tol=1e-3,
    lbfgs_steps=0,
    lbfgs_every=0,
    lbfgs_history=8,
    lbfgs_max_ls=20,
    lbfgs_ftol=0.0,
    **opt_kwargs,
):
    """Run the optimization loop that fits gains and foreground coefficients -- calibration.py:447-738.

    Same arguments and returns as the reference (arrays are NumPy).  Loop semantics kept: ``n_profile_steps``
    profiled steps and one more step are real, unrecorded updates (:681-693); recorded loss k is evaluated before
    update k (:700-701); ``use_min`` returns the parameters held right after the update of the lowest-loss step
    (:702-710); the loop ends when ``step >= 1 and |l_k - l_{k-1}| < tol`` (:712-717); ``freeze_model`` optimises
    gains only and returns ``fg_r, fg_i`` untouched (:598-603, :730-732).  The whole loop runs on the GPU; losses come
    back once at the end instead of once per step (:701).

    Not in the reference: ``gain_basis`` (real ``[Nfreqs, K]``, e.g. ``modeling.gain_dpss_basis``) confines the CORRECTION to the
    gains to its span, ``g = g_in + B y`` with the coefficients ``y`` (zero at the start) as the optimizer's variables in place of
    the per-channel gains; everything else -- loss, loop semantics, returns (full gains) -- is unchanged.  Default ``None``: free
    per-channel gains.  ``gain_solve_sweeps`` / ``gain_solve_every`` / ``gain_solve_damping``: closed-form gain sweeps before and
    between the descent steps, and ``coeff_solve_rounds`` / ``coeff_solve_ridge``: closed-form coefficient solves in front of them,
    and ``gain_basis_solve_sweeps`` / ``gain_basis_solve_every`` / ``gain_basis_solve_damping`` / ``gain_basis_solve_ridge``: the sweeps
    of a fit with a ``gain_basis``, see ``calibrate_and_model_tensor``.  ``gain_time_solve_sweeps`` / ``gain_time_solve_every`` /
    ``gain_time_solve_damping`` / ``gain_time_solve_ridge`` are checked like theirs, but belong to the joint fit over the times of
    ``calibrate_and_model_tensor(gain_time_basis=... / gain_time_scale=...)``: this function fits one time, so switching them on raises
    ``ValueError``.  ``robust_every`` / ``robust_rounds`` / ``robust_kind`` / ``robust_threshold``: iteratively reweighted least squares
    between chunks of the recorded loop, see ``calibrate_and_model_tensor``; here ``fit_history["robust"]`` holds the last reweight in
    solver units and row order, ``{"rounds": n, "ndown_bl": [nbls], "scale_bl": [nbls]}`` (``HipFitSolver.robust_weights``).
    ``gauss_newton_rounds`` / ``gauss_newton_every`` / ``gauss_newton_cg_iters`` / ``gauss_newton_lambda`` / ``gauss_newton_cg_tol``: joint
    Gauss-Newton steps over gains and coefficients, see ``calibrate_and_model_tensor``.  ``lbfgs_steps`` / ``lbfgs_every`` /
    ``lbfgs_history`` / ``lbfgs_max_ls`` / ``lbfgs_ftol``: L-BFGS iterations over the optimizer's own variables (with a ``gain_basis``
    its coefficients, with ``freeze_model`` the gains alone), see ``calibrate_and_model_tensor``; ``fit_history["lbfgs"]`` as there.
    """
    controls = FitControls.pick(locals())
    controls.check(gain_basis is not None, False, freeze_model, use_min, robust_first=True)
    if gain_basis is not None:
        gain_basis = _check_gain_basis(gain_basis, np.asarray(g_r).shape[-1])
    echo(f"Using {str(dtype)} precision.")
    echo(f"{datetime.datetime.now()} Provided the following opt_kwargs")
    for k in opt_kwargs:
        echo(f"{k}: {opt_kwargs[k]}")
    OPTIMIZERS[optimizer]  # unknown optimizer -> KeyError, like calibration.py:571
    dtype = np.dtype(dtype)
    g_r = np.asarray(g_r)
    nants = g_r.shape[0]
    prob = _as_problem(fg_comps, corr_inds, nants)
    solver = get_solver(prob, dtype)
    w_flat = _flatten(wgts, prob)
    solver.set_data(_flatten(data_r, prob), _flatten(data_i, prob), w_flat)
    solver.set_params(g_r, np.asarray(g_i), coeffs_from_chunks(prob, fg_r), coeffs_from_chunks(prob, fg_i))
    echo(f"{datetime.datetime.now()} Performing gradient descent on {np.prod(g_r.shape)} complex gain parameters...", verbose=verbose)
    if not freeze_model:
        echo(f"Performing gradient descent on total of {prob.ncoeffs} complex foreground parameters", verbose=verbose)
    # priors of calibration.py:619-625 (accumulated in float64 on the host); the gain basis: g0 = the gains just set, y = 0
    priors = slice_pipeline.prior_sums(_flatten(sky_model_r, prob), _flatten(sky_model_i, prob), w_flat) if model_regularization == "sum" else None
    slice_pipeline.configure(solver, gain_basis, priors, optimizer, opt_kwargs)
    if n_profile_steps > 0:
        echo(f"{datetime.datetime.now()} Profiling with {n_profile_steps}. And writing output to {profile_log_dir}...")
    echo(f"{datetime.datetime.now()} Building Computational Graph...\n", verbose=verbose)
    echo(f"{datetime.datetime.now()} Performing Gradient Descent...\n", verbose=verbose)
    result = drive(solver, controls, 1, prob.nbls, maxsteps, tol, use_min, freeze_model, n_profile_steps, profile_log_dir)
    ((losses, stopped, _),) = result.loops
    fit_history = history_entry(controls, result, 0, dtype)  # (the reweighting in solver units and row order: the documented shape of this function)
    if stopped:
        echo(f"Tolerance thresshold met with delta of {np.abs(losses[-1] - losses[-2]):.2e}. Terminating...\n ", verbose=verbose)
    g_r_opt, g_i_opt, c_r, c_i = solver.get_params(which=1 if (use_min and len(losses) > 0) else 0)
    if freeze_model:
        fg_r_opt, fg_i_opt = fg_r, fg_i
    else:
        fg_r_opt = coeffs_to_chunks(prob, c_r, dtype)
        fg_i_opt = coeffs_to_chunks(prob, c_i, dtype)
    min_loss = np.min(losses) if (use_min and len(losses)) else (losses[-1] if len(losses) else np.nan)
    echo(f"{datetime.datetime.now()} Finished Gradient Descent. MSE of {min_loss:.2e}...\n", verbose=verbose)
    return g_r_opt, g_i_opt, fg_r_opt, fg_i_opt, fit_history


# ------------------------------------------------------------------------------------------------------------------
# write-back: calibration.py:741-825, :1334-1350
# ------------------------------------------------------------------------------------------------------------------
def _check_gain_basis(basis, nfreqs):
    """A gain basis as the solver takes it: real, finite, ``[nfreqs, K >= 1]`` (ValueError otherwise, before any device work)."""
    basis = np.asarray(basis)
    if np.iscomplexobj(basis):
        raise ValueError("gain_basis must be real")
    if basis.ndim != 2 or basis.shape[0] != nfreqs or not 1 <= basis.shape[1] <= nfreqs:
        raise ValueError(f"gain_basis must have shape (Nfreqs = {nfreqs}, 1 <= K <= Nfreqs), got {basis.shape}")
    if not np.all(np.isfinite(basis)):
        raise ValueError("gain_basis has non-finite elements")
    return np.ascontiguousarray(basis, dtype=np.float64)


def robust_history(rounds, ndown_bl, scale_bl, rms, prob, ant_numbers):
    """One slice's ``fit_history[...]["robust"]``: ``{"rounds": n, "downweighted": {(ant0, ant1): count}, "scale": {(ant0, ant1):
    rms^2 scale_b}}`` with antenna NUMBERS, one entry per baseline row of ``prob``, from the last reweight of the slice
    (``HipFitSolver.robust_weights``; the scale in the data's units)."""
    ants = np.asarray(ant_numbers)
    keys = [(int(ants[i]), int(ants[j])) for i, j in zip(prob.bl_ant0, prob.bl_ant1)]
    return {"rounds": int(rounds), "downweighted": {k: int(v) for k, v in zip(keys, ndown_bl)},
            "scale": {k: float(rms) ** 2 * float(v) for k, v in zip(keys, scale_bl)}}


def _check_gain_time_basis(basis, ntimes):
    """``gain_time_basis`` as a real float64 ``[Ntimes, L]`` array, 1 <= L <= Ntimes (ValueError otherwise)."""
    basis = np.asarray(basis)
    if np.iscomplexobj(basis):
        raise ValueError("gain_time_basis must be real")
    if basis.ndim != 2 or basis.shape[0] != ntimes or not 1 <= basis.shape[1] <= ntimes:
        raise ValueError(f"gain_time_basis must have shape (Ntimes = {ntimes}, 1 <= L <= Ntimes), got {basis.shape}")
    if not np.all(np.isfinite(basis)):
        raise ValueError("gain_time_basis has non-finite elements")
    return np.ascontiguousarray(basis, dtype=np.float64)


def insert_model_into_uvdata_tensor(uvdata, time, polarization, ants_map, red_grps, model_r, model_i, scale_factor=1.0):
    """Insert ``(Nants, Nants, Nfreqs)`` model cubes back into a UVData object, conjugating pairs stored in reversed
    order and multiplying by ``scale_factor`` -- calibration.py:741-795.  Modifies ``uvdata``."""
    antpairs_data = set(uvdata.get_antpairs())
    polnum = np.where(uvdata.polarization_array == polstr2num(polarization, x_orientation=uvdata.x_orientation))[0][0]
    for red_grp in red_grps:
        for ap in red_grp:
            i, j = ants_map[ap[0]], ants_map[ap[1]]
            if ap in antpairs_data:
                dind = _time_ind(uvdata.time_array, uvdata.antpair2ind(ap), time)
                model = model_r[i, j] + 1j * model_i[i, j]
            else:
                dind = _time_ind(uvdata.time_array, uvdata.antpair2ind(ap[::-1]), time)
                model = model_r[i, j] - 1j * model_i[i, j]
            vis3(uvdata.data_array)[dind, :, polnum] = model * scale_factor


def insert_gains_into_uvcal(uvcal, time, polarization, gains_re, gains_im):
    """Insert ``(Nants, Nfreqs)`` gain arrays back into a UVCal object -- calibration.py:798-825."""
    polnum = np.where(np.asarray(uvcal.jones_array) == polstr2num(polarization, x_orientation=uvcal.x_orientation))[0][0]
    gindt = np.where(np.isclose(uvcal.time_array, time, atol=1e-7, rtol=0.0))[0][0]
    gain4(uvcal.gain_array)[:, :, gindt, polnum] = np.asarray(gains_re) + 1j * np.asarray(gains_im)


def flag_poltime(data_object, time, polarization):
    """Flag (and zero / set to unity) one polarization-time of a UVData or UVCal -- calibration.py:1334-1350."""
    if is_uvdata(data_object):
        bltsel = np.isclose(data_object.time_array, time, atol=1e-7, rtol=0.0)
        polnum = np.where(data_object.polarization_array == polstr2num(polarization, x_orientation=data_object.x_orientation))[0][0]
        data_object.flag_array[bltsel, ..., polnum] = True
        data_object.data_array[bltsel, ..., polnum] = 0.0
    elif is_uvcal(data_object):
        polnum = np.where(np.asarray(data_object.jones_array) == polstr2num(polarization, x_orientation=data_object.x_orientation))[0][0]
        gindt = np.where(np.isclose(data_object.time_array, time, atol=1e-7, rtol=0.0))[0][0]
        gain4(data_object.gain_array)[:, :, gindt, polnum] = 1.0
        gain4(data_object.flag_array)[:, :, gindt, polnum] = True
    else:
        raise ValueError("only supports data_object that is UVCal or UVData.")


def fit_quality_arrays(q, rms=1.0):
    """The sums of ``HipFitSolver.fit_quality`` (solver units: the data divided by ``rms``, the slice's ``data_scale_factor``) as
    weighted mean squared residuals in the data's units: ``(per_antenna [nants, nfreqs], total [nfreqs], per_baseline [nbls])``,
    ``rms^2 chisq / wsum`` each (the total: both sums taken over the antennas first), 0 where the sum of weights is 0."""
    def ratio(c, w):
        c, w = np.asarray(c, dtype=np.float64), np.asarray(w, dtype=np.float64)
        return float(rms) ** 2 * np.divide(c, w, out=np.zeros_like(c), where=w != 0)

    return (ratio(q["chisq_ant"], q["wsum_ant"]), ratio(np.sum(q["chisq_ant"], axis=0), np.sum(q["wsum_ant"], axis=0)),
            ratio(q["chisq_bl"], q["wsum_bl"]))


def fit_errors_arrays(e, chisq_bl, rms=1.0, gain_dof=None, ntimes=1):
    """The outputs of ``HipFitSolver.fit_errors`` of ONE slice (solver units; any of ``leverage_bl``, ``gain_var``, ``model_var`` may be
    missing) and the slice's ``chisq_bl`` (``fit_quality``) as what ``fit_history`` reports.  With ``n`` the samples with ``w != 0``
    and ``p = sum leverage_bl + #{(a, f): gain_var > 0}`` the parameters the fit spent on them::

        chisq_red_bl = chisq_bl / (nsamp_bl - leverage_bl)        nan where the denominator is <= 0
        noise_scale  = sum chisq_bl / (n - p)                     1.0 with underdetermined = True where n - p < 1
        gain_std     = sqrt(noise_scale gain_var)                 [nants, nfreqs], dimensionless
        model_std    = rms sqrt(noise_scale model_var)            [nbls, nfreqs] float32, the data's units (``rms``: the slice's
                                                                  ``data_scale_factor``, as in ``fit_quality_arrays``)

    ``gain_dof`` (``HipFitSolver.gain_basis_errors``; ``gain_var`` is then its ``gain_var`` of the slice): the complex parameters the
    basis gains of the slice's antennas spent, one number per antenna; they replace the count in ``p``: ``p = sum leverage_bl +
    sum gain_dof / ntimes``.  In a joint fit over ``ntimes`` times (a gain time basis) an antenna's coefficients are shared by the
    times, and so is their cost: every time is charged ``1 / ntimes`` of the antenna's ``gain_dof``, so that the times' ``p`` add up
    to what the joint fit spent.

    Returns a dict with ``noise_scale``, ``underdetermined``, ``n``, ``p`` and, where their inputs are given, ``leverage_bl``,
    ``chisq_red_bl``, ``gain_std``, ``model_std``."""
    chisq_bl = np.asarray(chisq_bl, dtype=np.float64)
    nsamp = np.asarray(e["nsamp_bl"], dtype=np.float64)
    out = {}
    n, p = float(np.sum(nsamp)), 0.0
    if "leverage_bl" in e:
        lev = np.asarray(e["leverage_bl"], dtype=np.float64)
        dof = nsamp - lev
        out["leverage_bl"] = lev
        out["chisq_red_bl"] = np.divide(chisq_bl, dof, out=np.full_like(chisq_bl, np.nan), where=dof > 0)
        p += float(np.sum(lev))
    if gain_dof is not None:
        p += float(np.sum(np.asarray(gain_dof, dtype=np.float64))) / float(ntimes)
    elif "gain_var" in e:
        p += float(np.count_nonzero(np.asarray(e["gain_var"]) > 0))
    under = n - p < 1.0
    scale = 1.0 if under else float(np.sum(chisq_bl)) / (n - p)
    out.update(noise_scale=scale, underdetermined=bool(under), n=n, p=p)
    if "gain_var" in e:
        out["gain_std"] = np.sqrt(scale * np.asarray(e["gain_var"], dtype=np.float64))
    if "model_var" in e:
        out["model_std"] = (float(rms) * np.sqrt(scale * np.asarray(e["model_var"], dtype=np.float64))).astype(np.float32)
    return out


def insert_fit_errors(gain_std, uvcal, hist, time, polarization, e, chisq_bl, rms, prob, nsingular=None, gain_dof=None, ntimes=1):
    """File one (polarization, time) slice's fit errors (``fit_errors_arrays``): ``hist["errors"]`` with ``noise_scale``,
    ``underdetermined``, ``nsingular`` and, unless the model was frozen, ``leverage_per_baseline`` and ``chisq_red_per_baseline`` (dicts
    ``{(ant0, ant1): value}`` with antenna NUMBERS like ``chisq_per_baseline``) and, where ``model_var`` was asked for, ``model_std``
    ``[rows, nfreqs]`` with its ``antpairs``; the slice's plane of ``gain_std`` (``[Nants, Nfreqs, Ntimes, Njones]`` or ``None``).
    ``gain_dof``, ``ntimes``: ``fit_errors_arrays``' (basis gains)."""
    a = fit_errors_arrays(e, chisq_bl, rms, gain_dof=gain_dof, ntimes=ntimes)
    ants = np.asarray(uvcal.ant_array)
    keys = [(int(ants[i]), int(ants[j])) for i, j in zip(prob.bl_ant0, prob.bl_ant1)]
    entry = {"noise_scale": a["noise_scale"], "underdetermined": a["underdetermined"], "nsingular": int(e.get("nsingular", 0) if nsingular is None else nsingular)}
    if "leverage_bl" in a:
        entry["leverage_per_baseline"] = {k: float(v) for k, v in zip(keys, a["leverage_bl"])}
        entry["chisq_red_per_baseline"] = {k: float(v) for k, v in zip(keys, a["chisq_red_bl"])}
    if "model_std" in a:
        entry["model_std"], entry["antpairs"] = a["model_std"], keys
    hist["errors"] = entry
    if gain_std is not None and "gain_std" in a:
        polnum = np.where(np.asarray(uvcal.jones_array) == polstr2num(polarization, x_orientation=uvcal.x_orientation))[0][0]
        gindt = np.where(np.isclose(uvcal.time_array, time, atol=1e-7, rtol=0.0))[0][0]
        gain_std[:, :, gindt, polnum] = a["gain_std"]


def _fit_errors_mode(fit_errors):
    if fit_errors not in (False, True, "samples"):
        raise ValueError(f"fit_errors must be False, True or 'samples', got {fit_errors!r}")
    return fit_errors


def insert_fit_quality(uvcal, hist, time, polarization, q, rms, prob):
    """Write one (polarization, time) slice's fit quality (``fit_quality_arrays``) into ``uvcal.quality_array[a, f, t, pol]`` and
    ``uvcal.total_quality_array[f, t, pol]`` (``(Nfreqs, Ntimes, Njones)``, created when ``None``) and, as
    ``hist["chisq_per_baseline"]``, a dict ``{(ant0, ant1): value}`` with antenna NUMBERS, one entry per baseline row of ``prob``."""
    per_ant, total, per_bl = fit_quality_arrays(q, rms)
    polnum = np.where(np.asarray(uvcal.jones_array) == polstr2num(polarization, x_orientation=uvcal.x_orientation))[0][0]
    gindt = np.where(np.isclose(uvcal.time_array, time, atol=1e-7, rtol=0.0))[0][0]
    gain4(uvcal.quality_array)[:, :, gindt, polnum] = per_ant
    if getattr(uvcal, "total_quality_array", None) is None:
        shape = gain4(uvcal.quality_array).shape
        uvcal.total_quality_array = np.zeros(shape[1:], dtype=np.float64)
    tot = uvcal.total_quality_array
    (tot[0] if np.ndim(tot) == 4 else tot)[:, gindt, polnum] = total
    ants = np.asarray(uvcal.ant_array)
    hist["chisq_per_baseline"] = {(int(ants[i]), int(ants[j])): float(v) for i, j, v in zip(prob.bl_ant0, prob.bl_ant1, per_bl)}


def _check_delay_spectrum(delay_spectrum, taper, max_dly, bllen_bin):
    """The delay-spectrum keywords of ``calibrate_and_model_tensor``, checked before anything is touched (``ValueError``)."""
    if not any(delay_spectrum is v for v in (False, True)) and delay_spectrum != "baselines":
        raise ValueError(f"delay_spectrum must be False, True or 'baselines', got {delay_spectrum!r}")
    if isinstance(taper, str) and taper not in ("bh4", "none"):
        raise ValueError(f"delay_spectrum_taper must be 'bh4', 'none' or an array of Nfreqs values, got {taper!r}")
    if not (np.isfinite(float(bllen_bin)) and float(bllen_bin) > 0.0):
        raise ValueError(f"delay_spectrum_bllen_bin must be a positive length in metres, got {bllen_bin!r}")
    if max_dly is not None and not (np.isfinite(float(max_dly)) and float(max_dly) >= 0.0):
        raise ValueError(f"delay_spectrum_max_dly must be a delay >= 0 in ns, got {max_dly!r}")


def _check_delay_transfer(delay_transfer, ridge, delay_spectrum, freeze_model):
    """The delay-transfer keywords of ``calibrate_and_model_tensor``, checked before anything is touched (``ValueError``)."""
    if not any(delay_transfer is v for v in (False, True)):
        raise ValueError(f"delay_transfer must be False or True, got {delay_transfer!r}")
    if not delay_transfer:
        return
    if not delay_spectrum:
        raise ValueError("delay_transfer needs delay_spectrum=True or 'baselines': it reports the signal loss of that spectrum, with its operator and bins")
    if freeze_model:
        raise ValueError("delay_transfer with freeze_model: no foreground coefficients are fitted, so the fit absorbs nothing")
    if not (np.isfinite(float(ridge)) and float(ridge) >= 0.0):
        raise ValueError(f"delay_transfer_ridge must be finite and >= 0, got {ridge!r}")


def _check_delay_cross(delay_cross_spectrum, delay_spectrum, batch_slices, init_guesses_from_previous_time_step):
    """The ``delay_cross_spectrum`` keyword of ``calibrate_and_model_tensor``, checked before anything is touched (``ValueError``)."""
    if not any(delay_cross_spectrum is v for v in (False, True)) and delay_cross_spectrum != "baselines":
        raise ValueError(f"delay_cross_spectrum must be False, True or 'baselines', got {delay_cross_spectrum!r}")
    if not delay_cross_spectrum:
        return
    if not delay_spectrum:
        raise ValueError("delay_cross_spectrum needs delay_spectrum=True or 'baselines': it uses that spectrum's operator, taper, bins and calibrated switch")
    if init_guesses_from_previous_time_step:
        raise ValueError("delay_cross_spectrum pairs the times of a batch: init_guesses_from_previous_time_step (a chain of single times) contradicts it")
    if batch_slices is not None and batch_slices is not True and int(batch_slices) < 2:
        raise ValueError(f"delay_cross_spectrum pairs the times of a batch: batch_slices={batch_slices!r} leaves nothing to pair (True or at least 2)")


def delay_cross_pairing(polnums, time_indices):
    """The pairs of a batch's unskipped slices, given in order by their polarization numbers and time indices: slices ``i`` and
    ``i + 1`` pair when they share the polarization and their time indices differ by exactly 1, and the walk then moves on by two;
    otherwise it moves on by one and slice ``i`` stays unpaired.  Returns the list of ``(i, i + 1)``."""
    pairs, i = [], 0
    while i + 1 < len(polnums):
        if polnums[i] == polnums[i + 1] and abs(int(time_indices[i + 1]) - int(time_indices[i])) == 1:
            pairs.append((i, i + 1))
            i += 2
        else:
            i += 1
    return pairs


def delay_cross_rows(pairing, dspec, rms, nbls):
    """What ``SliceBatchFitter.delay_cross_spectrum`` takes for the slice pairs ``pairing`` of a batch: pair ``p`` of baseline row ``b``
    is rows ``(t nbls + b, t' nbls + b)`` with scales ``(rms_t, rms_t')`` and bin ``pairindex nbins + bin_of_bl[b]``.  Returns
    ``(pairs [npairs, 2] int32, scale [npairs, 2], bin_of_pair [npairs] int32)``, slice pair by slice pair."""
    b = np.arange(nbls, dtype=np.int64)
    pairs = np.concatenate([np.stack([t0 * nbls + b, t1 * nbls + b], axis=1) for t0, t1 in pairing]).astype(np.int32)
    scale = np.concatenate([np.tile([float(rms[t0]), float(rms[t1])], (nbls, 1)) for t0, t1 in pairing])
    bins = np.concatenate([k * dspec["nbins"] + np.asarray(dspec["bin_of_bl"], dtype=np.int64) for k in range(len(pairing))]).astype(np.int32)
    return pairs, scale, bins


def delay_cross_entry(cross, dspec, k, partner_time_index, prob, ant_array):
    """Slice pair ``k`` of a ``delay_cross_spectrum`` over ``delay_cross_rows`` as what both of its members report under
    ``fit_history[...]["delay_spectrum"]["cross"]``: ``data``, ``model``, ``resid`` ``[nbins, ndelays]``, the MEAN cross power per
    baseline-length bin in the data's units squared (the scales were the slices' ``rms``; 0 for a bin without a counted pair),
    ``noise`` with the mean half-difference power of the same three, ``nbls`` the counted pairs per bin, the partner's time index, and
    with per-pair rows ``per_baseline`` keyed by antenna numbers."""
    nb, nbins = prob.nbls, dspec["nbins"]
    bins, rows = slice(k * nbins, (k + 1) * nbins), slice(k * nb, (k + 1) * nb)
    count = np.asarray(cross["count_bin"][bins], dtype=np.float64)
    mean = np.divide(1.0, count, out=np.zeros_like(count), where=count > 0)[:, None]
    entry = {"partner_time_index": int(partner_time_index), "nbls": count.astype(np.int64), "noise": {}}
    for q in ("data", "model", "resid"):
        entry[q] = mean * np.asarray(cross["cross"][q][bins])
        entry["noise"][q] = mean * np.asarray(cross["diff"][q][bins])
    if "per_pair" in cross:
        ants = np.asarray(ant_array)
        pp = cross["per_pair"]
        entry["per_baseline"] = {(int(ants[i]), int(ants[j])): dict({q: pp["cross"][q][rows][b] for q in ("data", "model", "resid")},
                                                                     noise={q: pp["diff"][q][rows][b] for q in ("data", "model", "resid")})
                                 for b, (i, j) in enumerate(zip(prob.bl_ant0, prob.bl_ant1))}
    return entry


def _check_delay_fringe(delay_fringe_spectrum, delay_fringe_times, delay_fringe_taper, delay_spectrum, batch_slices, init_guesses_from_previous_time_step):
    """The ``delay_fringe_spectrum`` keywords of ``calibrate_and_model_tensor``, checked before anything is touched (``ValueError``)."""
    if not any(delay_fringe_spectrum is v for v in (False, True)) and delay_fringe_spectrum != "baselines":
        raise ValueError(f"delay_fringe_spectrum must be False, True or 'baselines', got {delay_fringe_spectrum!r}")
    if not delay_fringe_spectrum:
        return
    if not delay_spectrum:
        raise ValueError("delay_fringe_spectrum needs delay_spectrum=True or 'baselines': it uses that spectrum's operator, taper, bins and calibrated switch")
    if isinstance(delay_fringe_times, bool) or not isinstance(delay_fringe_times, (int, np.integer)) or not 2 <= int(delay_fringe_times) <= 64:
        raise ValueError(f"delay_fringe_spectrum: delay_fringe_times must be an integer in [2, 64], got {delay_fringe_times!r}")
    try:
        modeling.delay_taper(int(delay_fringe_times), delay_fringe_taper)
    except ValueError:
        raise ValueError(f"delay_fringe_spectrum: delay_fringe_taper must be 'bh4', 'none' or an array of delay_fringe_times values, got {delay_fringe_taper!r}") from None
    if init_guesses_from_previous_time_step:
        raise ValueError("delay_fringe_spectrum transforms along the times of a batch: init_guesses_from_previous_time_step (a chain of single times) contradicts it")
    if batch_slices is not None and batch_slices is not True and int(batch_slices) < int(delay_fringe_times):
        raise ValueError(f"delay_fringe_spectrum transforms along the times of a batch: batch_slices={batch_slices!r} holds no window of "
                         f"delay_fringe_times={int(delay_fringe_times)} (True or at least that many)")


def delay_fringe_windows(polnums, time_indices, ntimes, times=None, dt=None):
    """The windows of a batch's unskipped slices, given in order by their polarization numbers and time indices: every run of ``ntimes``
    slices of one polarization whose time indices rise by exactly 1; the walk then moves on behind the run (windows do not overlap),
    otherwise by one, and a slice left over belongs to no window.  Returns the list of tuples of ``ntimes`` positions.  With ``times``
    (the data's distinct times, indexed by the time indices) and ``dt`` (their median spacing) a window whose spacings differ from
    ``dt`` by more than 1 % raises ``ValueError`` naming the times: the transform along time takes evenly spaced integrations."""
    n = int(ntimes)
    windows, i = [], 0
    while i + n <= len(polnums):
        run = all(polnums[i + k] == polnums[i] and int(time_indices[i + k]) - int(time_indices[i]) == k for k in range(1, n))
        if run:
            windows.append(tuple(range(i, i + n)))
            i += n
        else:
            i += 1
    if times is not None:
        for win in windows:
            at = np.asarray([times[int(time_indices[k])] for k in win], dtype=np.float64)
            if np.any(np.abs(np.diff(at) - dt) > 0.01 * abs(dt)):
                raise ValueError(f"delay_fringe_spectrum: the times {at.tolist()} are not evenly spaced by the data's median spacing {dt!r}")
    return windows


def delay_fringe_setup(times, ntimes, taper="bh4", per_baseline=False):
    """What the fringe-rate pass of every batch of a call shares: the data's distinct ``times`` (Julian days), their median spacing ``dt``
    (the same unit), the transform along time (``modeling.fringe_rate_transform`` on ``ntimes`` integrations ``dt`` apart, all rates) and
    its fringe rates in Hz."""
    times = np.asarray(times, dtype=np.float64)
    dt = float(np.median(np.diff(times))) if len(times) > 1 else 1.0
    opt, rates_hz = modeling.fringe_rate_transform(int(ntimes), dt * 86400.0, taper=taper)
    return dict(ntimes=int(ntimes), times=times, dt=dt, opt=opt, rates_hz=rates_hz, per_group=bool(per_baseline))


def delay_fringe_rows(windows, dspec, rms, nbls):
    """What ``SliceBatchFitter.delay_fringe_spectrum`` takes for the slice windows ``windows`` of a batch: group ``g`` of baseline row
    ``b`` in window ``k`` is the rows ``t nbls + b`` of the window's slices ``t`` with their ``rms`` as scales and bin
    ``k nbins + bin_of_bl[b]``.  Returns ``(rows [ngroups, ntimes] int32, scale [ngroups, ntimes], bin_of_group [ngroups] int32)``,
    window by window."""
    b = np.arange(nbls, dtype=np.int64)
    rows = np.concatenate([np.stack([t * nbls + b for t in win], axis=1) for win in windows]).astype(np.int32)
    scale = np.concatenate([np.tile([float(rms[t]) for t in win], (nbls, 1)) for win in windows])
    bins = np.concatenate([k * dspec["nbins"] + np.asarray(dspec["bin_of_bl"], dtype=np.int64) for k in range(len(windows))]).astype(np.int32)
    return rows, scale, bins


def delay_fringe_entry(fringe, dspec, k, time_indices, prob, ant_array):
    """Window ``k`` of a ``delay_fringe_spectrum`` over ``delay_fringe_rows`` as what every member of it reports under
    ``fit_history[...]["delay_spectrum"]["fringe"]``: ``time_indices`` of the window, ``fringe_rates`` in Hz, ``data``, ``model``,
    ``resid`` ``[nbins, nrates, ndelays]``, the MEAN power per baseline-length bin in the data's units squared (the scales were the
    slices' ``rms``; 0 for a bin without a counted group), ``nbls`` the counted groups per bin, and with per-group rows
    ``per_baseline`` keyed by antenna numbers."""
    nb, nbins = prob.nbls, dspec["nbins"]
    bins, rows = slice(k * nbins, (k + 1) * nbins), slice(k * nb, (k + 1) * nb)
    count = np.asarray(fringe["count_bin"][bins], dtype=np.float64)
    mean = np.divide(1.0, count, out=np.zeros_like(count), where=count > 0)[:, None, None]
    entry = {"time_indices": [int(t) for t in time_indices], "fringe_rates": np.array(dspec["fringe"]["rates_hz"]), "nbls": count.astype(np.int64)}
    for q in ("data", "model", "resid"):
        entry[q] = mean * np.asarray(fringe[q][bins])
    if "per_group" in fringe:
        ants = np.asarray(ant_array)
        entry["per_baseline"] = {(int(ants[i]), int(ants[j])): {q: fringe["per_group"][q][rows][b] for q in ("data", "model", "resid")}
                                 for b, (i, j) in enumerate(zip(prob.bl_ant0, prob.bl_ant1))}
    return entry


def _check_delay_redundant(delay_redundant_spectrum, delay_redundant_times, delay_redundant_taper, delay_redundant_weighting, delay_spectrum,
                           delay_spectrum_calibrated, batch_slices, init_guesses_from_previous_time_step, device_split):
    """The ``delay_redundant_spectrum`` keywords of ``calibrate_and_model_tensor``, checked before anything is touched (``ValueError``)."""
    if not any(delay_redundant_spectrum is v for v in (False, True)) and delay_redundant_spectrum != "groups":
        raise ValueError(f"delay_redundant_spectrum must be False, True or 'groups', got {delay_redundant_spectrum!r}")
    if not delay_redundant_spectrum:
        return
    if not delay_spectrum:
        raise ValueError("delay_redundant_spectrum needs delay_spectrum=True or 'baselines': it uses that spectrum's operator, taper and bin width")
    if not delay_spectrum_calibrated:
        raise ValueError("delay_redundant_spectrum needs delay_spectrum_calibrated=True: an average of uncalibrated rows of different antennas decoheres")
    if isinstance(delay_redundant_times, bool) or not isinstance(delay_redundant_times, (int, np.integer)) or not 1 <= int(delay_redundant_times) <= 64:
        raise ValueError(f"delay_redundant_spectrum: delay_redundant_times must be an integer in [1, 64], got {delay_redundant_times!r}")
    try:
        modeling.delay_taper(int(delay_redundant_times), delay_redundant_taper)
    except ValueError:
        raise ValueError(f"delay_redundant_spectrum: delay_redundant_taper must be 'bh4', 'none' or an array of delay_redundant_times values, "
                         f"got {delay_redundant_taper!r}") from None
    if not isinstance(delay_redundant_weighting, str) or delay_redundant_weighting not in ("weights", "uniform"):
        raise ValueError(f"delay_redundant_spectrum: delay_redundant_weighting must be 'weights' or 'uniform', got {delay_redundant_weighting!r}")
    if init_guesses_from_previous_time_step:
        raise ValueError("delay_redundant_spectrum transforms along the times of a batch: init_guesses_from_previous_time_step (a chain of single times) contradicts it")
    if batch_slices is not None and batch_slices is not True and int(batch_slices) < int(delay_redundant_times):
        raise ValueError(f"delay_redundant_spectrum transforms along the times of a batch: batch_slices={batch_slices!r} holds no window of "
                         f"delay_redundant_times={int(delay_redundant_times)} (True or at least that many)")
    if device_split == "groups":
        raise ValueError("delay_redundant_spectrum averages the rows of a redundant group: device_split='groups' would put them on several devices "
                         "(use one device or device_split='slices')")


def delay_redundant_setup(uvdata, ant_array, prob, ntimes, taper="none", weighting="weights", per_group=False, bllen_bin=1.0, red_tol=1.0,
                          include_autos=False):
    """What the redundant-average pass of every batch of a call shares.  The groups are those of
    ``modeling.get_redundant_grps_data(uvdata, tol=red_tol, include_autos=include_autos)``: every pair of a group maps to its baseline row
    of ``prob`` (``ant_array``: the antenna numbers ``prob``'s antenna indices count through), with ``conj = 1`` where the row holds the
    pair reversed -- the average is taken in the group's orientation; a pair without a row is dropped, and so is a group without rows; no
    row enters two sets.  ``rows``, ``conj`` and ``pairs`` list the kept members group by group, the groups in the order of their first rows; ``bin_of_group`` and ``bllen_m`` come from
    ``baseline_length_bins`` on the GROUPS' lengths at ``bllen_bin``; the transform along time, its rates, ``times`` and ``dt`` are
    ``delay_fringe_setup``'s."""
    out = delay_fringe_setup(np.unique(uvdata.time_array), ntimes, taper, per_group)
    _, grps, _, lengths = modeling.get_redundant_grps_data(uvdata, tol=red_tol, include_autos=include_autos)
    ants = np.asarray(ant_array)
    row_of = {}
    for b, (i, j) in enumerate(zip(prob.bl_ant0, prob.bl_ant1)):
        row_of.setdefault((int(ants[i]), int(ants[j])), b)
    rows, conj, pairs, kept, used = [], [], [], [], set()
    for grp, length in zip(grps, lengths):
        r, c, p = [], [], []
        for i, j in grp:
            i, j = int(i), int(j)
            b, flip = (row_of[(i, j)], 0) if (i, j) in row_of else (row_of.get((j, i)), 1)
            if b is None or b in used:
                continue
            used.add(b)
            r.append(b), c.append(flip), p.append((i, j))
        if r:
            rows.append(np.asarray(r, dtype=np.int32)), conj.append(np.asarray(c, dtype=np.uint8)), pairs.append(p), kept.append(float(length))
    if not rows:
        raise ValueError("delay_redundant_spectrum: no redundant group holds a baseline of the fit")
    # the groups in the order of their first rows: a bin then adds its groups as delay_spectrum adds its rows
    order = sorted(range(len(rows)), key=lambda g: int(rows[g][0]))
    rows, conj, pairs, kept = ([x[g] for g in order] for x in (rows, conj, pairs, kept))
    bin_of_group, bllen_m = baseline_length_bins(kept, bllen_bin)
    out.update(weighting=weighting, rows=rows, conj=conj, pairs=pairs, lengths=np.asarray(kept), bin_of_group=bin_of_group, nbins=len(bllen_m), bllen_m=bllen_m)
    return out


def delay_redundant_sets(windows, red, rms, nbls):
    """What ``SliceBatchFitter.delay_coherent_spectrum`` takes for the slice windows ``windows`` of a batch: group ``g`` of window ``k`` has
    the sets ``t nbls + red["rows"][g]`` of the window's slices ``t`` with their ``rms`` as scales (ones for windows of one time:
    ``delay_redundant_entry`` then multiplies by ``rms^2`` as ``delay_spectrum_entry`` does) and bin ``k nbins + bin_of_group[g]``.
    Returns ``(set_ptr int64, member_row int32, member_conj uint8, scale [ngroups, ntimes], bin_of_group int32)``, window by window."""
    sizes, members, conj, scale, bins = [], [], [], [], []
    for k, win in enumerate(windows):
        for g, r in enumerate(red["rows"]):
            for t in win:
                sizes.append(len(r)), members.append(t * nbls + r.astype(np.int64)), conj.append(red["conj"][g])
            scale.append([float(rms[t]) if len(win) > 1 else 1.0 for t in win])  # (one time: the entry applies rms^2 behind the square)
            bins.append(k * red["nbins"] + int(red["bin_of_group"][g]))
    return (np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), np.concatenate(members).astype(np.int32), np.concatenate(conj).astype(np.uint8),
            np.asarray(scale, dtype=np.float64), np.asarray(bins, dtype=np.int32))


def delay_redundant_entry(out, red, k, time_indices, rms=1.0):
    """Window ``k`` of a ``delay_coherent_spectrum`` over ``delay_redundant_sets`` as what every member of it reports under
    ``fit_history[...]["delay_spectrum"]["redundant"]``: ``time_indices`` of the window, ``fringe_rates`` in Hz, ``bllen_m`` of the GROUPS'
    length bins, ``ngroups`` the counted groups per bin, ``nmembers`` the rows per group, ``data``, ``model``, ``resid``
    ``[nbins, nrates, ndelays]``, the MEAN over the bin's groups of the power of the group's average in the data's units squared (the
    scales were the slices' ``rms``; with windows of one time ``rms`` is the reporting slice's, applied here as ``rms^2 sum / count``
    in ``delay_spectrum_entry``'s order of operations; 0 for a bin without a counted group), and with per-group planes ``groups`` keyed by
    the group's first antenna pair: ``{"antpairs": its member pairs, "data", "model", "resid"}``."""
    ng, nbins = len(red["rows"]), red["nbins"]
    bins, grp = slice(k * nbins, (k + 1) * nbins), slice(k * ng, (k + 1) * ng)
    count = np.asarray(out["count_bin"][bins], dtype=np.float64)
    unit = float(rms) ** 2 if red["ntimes"] == 1 else 1.0
    mean = (unit * np.divide(1.0, count, out=np.zeros_like(count), where=count > 0))[:, None, None]
    entry = {"time_indices": [int(t) for t in time_indices], "fringe_rates": np.array(red["rates_hz"]), "bllen_m": np.array(red["bllen_m"]),
             "ngroups": count.astype(np.int64), "nmembers": np.asarray([len(r) for r in red["rows"]], dtype=np.int64)}
    for q in ("data", "model", "resid"):
        entry[q] = mean * np.asarray(out[q][bins])
    if "per_group" in out:
        entry["groups"] = {p[0]: dict({q: unit * out["per_group"][q][grp][g] for q in ("data", "model", "resid")}, antpairs=list(p))
                           for g, p in enumerate(red["pairs"])}
    return entry


def baseline_length_bins(lengths, width):
    """Baseline rows into bins of ``width`` metres, bin ``floor(length / width)``, only the bins that hold a row, in ascending order:
    ``(bin_of_bl [nbls] int32, bllen_m [nbins])`` with ``bllen_m`` the mean length of each bin's rows."""
    lengths = np.asarray(lengths, dtype=np.float64)
    idx = np.floor(lengths / float(width)).astype(np.int64)
    used, bin_of_bl = np.unique(idx, return_inverse=True)
    bin_of_bl = bin_of_bl.reshape(-1)
    bllen = np.bincount(bin_of_bl, weights=lengths, minlength=len(used)) / np.bincount(bin_of_bl, minlength=len(used))
    return bin_of_bl.astype(np.int32), bllen


def delay_spectrum_setup(uvdata, ant_array, prob, taper="bh4", max_dly=None, bllen_bin=1.0, calibrated=False, per_baseline=False):
    """What the delay-spectrum pass of every slice of a call shares: the operator, ``norm_f`` and delays (``modeling.delay_transform``
    on the data's frequencies), the length bin of every baseline row of ``prob`` (``baseline_length_bins`` on the antenna positions of
    ``uvdata``; ``ant_array``: the antenna numbers ``prob``'s antenna indices count through) and the two switches.  ``transfer_ridge``
    stays ``None`` unless the call also asks for the delay transfer (``delay_transfer``: its ridge then), ``cross`` unless it asks for the
    cross spectrum of paired times (``delay_cross_spectrum``: ``"bins"`` or ``"baselines"`` then), ``fringe`` unless it asks for the delay /
    fringe-rate plane (``delay_fringe_spectrum``: ``delay_fringe_setup``'s dictionary then)."""
    op, norm_f, delays_ns = modeling.delay_transform(np.asarray(uvdata.freq_array, dtype=np.float64).ravel(), taper=taper, max_delay_ns=max_dly)
    if op.shape[1] < 1 or op.shape[1] > 4096:
        raise ValueError(f"the delay spectrum has {op.shape[1]} delays: between 1 and 4096 (delay_spectrum_max_dly)")
    pos = {int(a): np.asarray(x, dtype=np.float64) for a, x in zip(np.asarray(uvdata.antenna_numbers), np.asarray(uvdata.antenna_positions))}
    ants = np.asarray(ant_array)
    lengths = np.asarray([np.linalg.norm(pos[int(ants[i])] - pos[int(ants[j])]) for i, j in zip(prob.bl_ant0, prob.bl_ant1)])
    bin_of_bl, bllen_m = baseline_length_bins(lengths, bllen_bin)
    return dict(op=op, norm_f=norm_f, delays_ns=delays_ns, bin_of_bl=bin_of_bl, nbins=len(bllen_m), bllen_m=bllen_m, calibrated=bool(calibrated),
                per_baseline=bool(per_baseline), transfer_ridge=None, cross=None, fringe=None)


def delay_spectrum_slice_bins(dspec, nt):
    """``bin_of_bl`` of ``nt`` slices in slice-major row order: row ``b`` of slice ``t`` goes to bin ``t nbins + bin_of_bl[b]``."""
    return (np.repeat(np.arange(nt, dtype=np.int32) * dspec["nbins"], len(dspec["bin_of_bl"])) + np.tile(dspec["bin_of_bl"], nt)).astype(np.int32)


def delay_spectrum_of_slice(spectra, dspec, t, nbls):
    """Slice ``t``'s part of a ``SliceBatchFitter.delay_spectrum`` whose bins are those of ``delay_spectrum_slice_bins``."""
    bins, rows = slice(t * dspec["nbins"], (t + 1) * dspec["nbins"]), slice(t * nbls, (t + 1) * nbls)
    out = {k: spectra[k][bins] for k in ("data", "model", "resid", "count_bin")}
    if "per_baseline" in spectra:
        out["per_baseline"] = {k: v[rows] for k, v in spectra["per_baseline"].items()}
    return out


def delay_transfer_of_slice(transfer, dspec, t, nbls):
    """Slice ``t``'s part of a ``SliceBatchFitter.delay_transfer`` whose bins are those of ``delay_spectrum_slice_bins``; the counts of
    groups are those of the whole call."""
    bins, rows = slice(t * dspec["nbins"], (t + 1) * dspec["nbins"]), slice(t * nbls, (t + 1) * nbls)
    out = {k: transfer[k][bins] for k in ("absorbed_bin", "count_bin")}
    out.update({k: transfer[k][rows] for k in ("absorbed_bl", "noise_bl") if k in transfer}, nsingular=transfer["nsingular"])
    return out


def delay_transfer_entry(tr, prob, ant_array):
    """One slice's ``HipFitSolver.delay_transfer`` as what ``fit_history`` reports beside the spectrum: ``transfer`` ``[nbins, ndelays]``,
    ``1 - absorbed_bin / count_bin`` -- the share of the power of a signal that is white in delay which survives the fit, per
    baseline-length bin; dimensionless (0 for a bin without a counted row) --, ``transfer_nsingular``, the singular groups of the call
    that held the slice, and with per-baseline rows ``transfer_per_baseline`` keyed by antenna numbers (``1 - absorbed_bl``; 0 for a
    row that is flagged throughout or belongs to a singular group)."""
    count = np.asarray(tr["count_bin"], dtype=np.float64)
    mean = np.asarray(tr["absorbed_bin"]) * np.divide(1.0, count, out=np.zeros_like(count), where=count > 0)[:, None]
    entry = {"transfer": np.where(count[:, None] > 0, 1.0 - mean, 0.0), "transfer_nsingular": int(tr["nsingular"])}
    if "absorbed_bl" in tr:
        ants = np.asarray(ant_array)
        live = np.any(np.asarray(tr["noise_bl"]) != 0, axis=1)
        rows = np.where(live[:, None], 1.0 - np.asarray(tr["absorbed_bl"]), 0.0)
        entry["transfer_per_baseline"] = {(int(ants[i]), int(ants[j])): rows[b] for b, (i, j) in enumerate(zip(prob.bl_ant0, prob.bl_ant1))}
    return entry


def delay_spectrum_entry(ds, dspec, rms, prob, ant_array):
    """One slice's ``HipFitSolver.delay_spectrum`` (solver units: the data divided by ``rms``; sums over the bins' rows) as what
    ``fit_history`` reports: the MEAN power per baseline-length bin in the data's units squared, ``rms^2 sum / count`` (0 for a bin
    whose rows are all flagged), and with ``per_baseline`` every row's own spectrum keyed by antenna numbers."""
    count = np.asarray(ds["count_bin"], dtype=np.float64)
    scale = float(rms) ** 2 * np.divide(1.0, count, out=np.zeros_like(count), where=count > 0)
    entry = {"delays_ns": dspec["delays_ns"], "bllen_m": dspec["bllen_m"], "nbls": count.astype(np.int64)}
    for k in ("data", "model", "resid"):
        entry[k] = scale[:, None] * np.asarray(ds[k])
    if "per_baseline" in ds:
        ants = np.asarray(ant_array)
        pb = {k: float(rms) ** 2 * np.asarray(v) for k, v in ds["per_baseline"].items()}
        entry["per_baseline"] = {(int(ants[i]), int(ants[j])): {k: pb[k][b] for k in pb} for b, (i, j) in enumerate(zip(prob.bl_ant0, prob.bl_ant1))}
    return entry


DEGENERACY_MODES = {False: None, True: "channel", "channel": "channel", "band": "band"}


def check_degeneracy_keywords(fix_degeneracies, degeneracy_iters, sky_model, freeze_model, model_regularization, devices=None, device_split=None):
    """The degeneracy keywords of ``calibrate_and_model_tensor``, checked before anything is touched (``ValueError``).  Returns the mode,
    ``None`` | ``"channel"`` | ``"band"``."""
    if not any(fix_degeneracies is v for v in (False, True)) and fix_degeneracies not in ("channel", "band"):
        raise ValueError(f"fix_degeneracies must be False, True, 'channel' or 'band', got {fix_degeneracies!r}")
    mode = DEGENERACY_MODES[fix_degeneracies]
    if mode is None:
        return None
    if isinstance(degeneracy_iters, bool) or int(degeneracy_iters) != degeneracy_iters or int(degeneracy_iters) < 1:
        raise ValueError(f"degeneracy_iters must be an integer >= 1, got {degeneracy_iters!r}")
    if sky_model is None:
        raise ValueError("fix_degeneracies needs a sky_model: a reference made from the data themselves fixes nothing")
    if freeze_model:
        raise ValueError("fix_degeneracies with freeze_model: the model is the sky model already, nothing is degenerate")
    if model_regularization == "post_hoc":
        raise ValueError("fix_degeneracies and model_regularization='post_hoc' both set the amplitude: choose one")
    if device_split == "groups" and devices is not None and (isinstance(devices, str) or len(list(devices)) > 1):
        raise ValueError("fix_degeneracies with several devices that share out the fitting groups of a slice is not implemented (the channel sums "
                         "would need an exchange per iteration): use one device or device_split='slices'")
    return mode


def _check_degeneracy_call(fix_degeneracies, degeneracy_iters, fitting_kwargs):
    """``check_degeneracy_keywords`` for an entry point that hands ``fitting_kwargs`` on to ``calibrate_and_model_tensor``."""
    return check_degeneracy_keywords(fix_degeneracies, degeneracy_iters, fitting_kwargs.get("sky_model"), fitting_kwargs.get("freeze_model", False),
                                     fitting_kwargs.get("model_regularization", "sum"), fitting_kwargs.get("devices"), fitting_kwargs.get("device_split"))


def degeneracy_setup(uvdata, ant_array, mode, iters, phase_ref):
    """What the degeneracy fix of every slice of a call shares: the mode and iterations, the data's frequencies and the east, north
    positions ``[Nants, 2]`` of the antennas in the order of ``ant_array`` (the positions ``delay_spectrum_setup`` takes its baseline
    lengths from)."""
    pos = {int(a): np.asarray(x, dtype=np.float64) for a, x in zip(np.asarray(uvdata.antenna_numbers), np.asarray(uvdata.antenna_positions))}
    antpos = np.ascontiguousarray([pos[int(a)][:2] for a in np.asarray(ant_array)], dtype=np.float64)
    return dict(mode=mode, iters=int(iters), phase_ref=bool(phase_ref), antpos=antpos, freqs=np.asarray(uvdata.freq_array, dtype=np.float64).ravel().copy())


def degeneracy_entry(out, t, degen):
    """Slice ``t`` of a ``fix_degeneracies`` result as what ``fit_history`` reports, per channel."""
    return {"mode": degen["mode"], "amplitude": np.exp(out["eta"][t]), "phase": out["psi"][t].copy(), "tilt": out["tilt"][t].copy(),
            "nsamples": out["nsamples"][t].astype(np.int64), "iters": degen["iters"], "last_step": out["last_step"][t].copy()}


# ------------------------------------------------------------------------------------------------------------------
# orchestration: calibration.py:963-1331, :1503-1584
# ------------------------------------------------------------------------------------------------------------------
def calibrate_and_model_tensor(
    uvdata,
    fg_model_comps_dict,
    gains=None,
    freeze_model=False,
    optimizer="Adamax",
    tol=1e-14,
    maxsteps=10000,
    include_autos=False,
    verbose=False,
    sky_model=None,
    dtype=np.float32,
    use_min=False,
    use_redundancy=False,
    notebook_progressbar=False,
    correct_resid=False,
    correct_model=True,
    weights=None,
    nsamples_in_weights=True,
    graph_mode=False,
    grp_size_threshold=5,
    n_profile_steps=0,
    profile_log_dir="./logdir",
    model_regularization="sum",
    init_guesses_from_previous_time_step=False,
    skip_threshold=0.5,
    use_model_snr_weights=False,
    parallel_fits=None,
    batch_slices=None,
    devices=None,
    layout=None,
    device_split=None,
    gain_basis=None,
    gain_max_dly=None,
    gain_time_basis=None,
    gain_time_scale=None,
    fit_quality=False,
    gain_solve_sweeps=0,
    gain_solve_every=0,
    gain_solve_damping=0.5,
    coeff_solve_rounds=0,
    coeff_solve_ridge=1e-6,
    gain_basis_solve_sweeps=0,
    gain_basis_solve_every=0,
    gain_basis_solve_damping=0.5,
    gain_basis_solve_ridge=1e-6,
    gain_time_solve_sweeps=0,
    gain_time_solve_every=0,
    gain_time_solve_damping=0.5,
    gain_time_solve_ridge=1e-6,
    robust_every=0,
    robust_rounds=0,
    robust_kind="huber",
    robust_threshold=3.0,
    gauss_newton_rounds=0,
    gauss_newton_every=0,
    gauss_newton_cg_iters=20,
    gauss_newton_lambda=1e-3,
    gauss_newton_cg_tol=1e-3,
    lbfgs_steps=0,
    lbfgs_every=0,
    lbfgs_history=8,
    lbfgs_max_ls=20,
    lbfgs_ftol=0.0,
    fit_errors=False,
    fit_errors_ridge=1e-6,
    gain_basis_errors=False,
    fix_degeneracies=False,
    degeneracy_iters=6,
    degeneracy_phase_ref=True,
    delay_redundant_spectrum=False,
    delay_redundant_times=2,
    delay_redundant_taper="none",
    delay_redundant_weighting="weights",
    delay_fringe_spectrum=False,
    delay_fringe_times=8,
    delay_fringe_taper="bh4",
    delay_cross_spectrum=False,
    delay_transfer=False,
    delay_transfer_ridge=1e-6,
    delay_spectrum=False,
    delay_spectrum_taper="bh4",
    delay_spectrum_max_dly=None,
    delay_spectrum_bllen_bin=1.0,
    delay_spectrum_calibrated=False,
    **opt_kwargs,
):
    """Simultaneous calibration and foreground fitting -- calibration.py:963-1331, same arguments, defaults and
    returns ``(model, resid, gains, fit_history)``.  See SURVEY.md Appendix A for the behaviours kept (the input
    ``uvdata`` is not modified; a supplied ``gains`` object IS modified in place and returned).

    Not in the reference (which loops over polarizations and times, one fit after the other on one device, :1160-1167):

    * ``batch_slices`` (default: on whenever the slices are independent, i.e. unless ``init_guesses_from_previous_time_step``):
      all unskipped (polarization, time) slices of the call -- ``batch_slices=N``: at most N at a time -- are fitted TOGETHER
      in one solver per device: one pass over the modeling components serves every slice, while each slice keeps its own
      rms scale, weight normalisation, priors, loss history, tolerance stop and use_min snapshot, exactly as in the loop
      (``batched.SliceBatchFitter``).  ``fit_history`` and every output equal those of the sequential loop (to rounding:
      the same kernels in the same order).  ``batch_slices=False`` keeps the loop.
    * ``devices``: GPUs to fit on: a list of device indices, or "all" for every visible GPU (a set-up that fails on "all" continues on one
      device with a RuntimeWarning).  Default ``None``: the ONE device of the process (``gpu_index`` of the file driver, else 0) -- a run
      spreads over several GPUs only when the caller says so.
    * ``device_split``: what several devices share out.  "slices": whole batches of slices go to different devices -- no exchange
      between them, every slice is fitted exactly as on one device (bit for bit); "groups": each device takes a share of the
      fitting groups of every slice, with one exchange of the gain gradients per step.  Default: "slices" when the call has at
      least as many batches as devices, else "groups".
    * ``gain_basis`` / ``gain_max_dly`` (give one, default neither: free per-channel gains): fit the gains in a smooth frequency
      basis.  ``gain_basis``: real ``[Nfreqs, K]``; ``gain_max_dly``: a delay in ns, the basis is then
      ``modeling.gain_dpss_basis(freqs, gain_max_dly)``.  Every (polarization, time) slice is fitted as ``g = g_in + B y`` with
      ``g_in`` the gains it starts from (unity, the ``gains`` object's, or the previous time's with
      ``init_guesses_from_previous_time_step``): output gains minus input gains lie in span(B).  Works in the loop, in batches and
      on several devices (``device_split="groups"`` then exchanges the projected gradient, K instead of Nfreqs numbers per antenna).
    * ``gain_time_basis`` / ``gain_time_scale`` (give one, default neither: every time fits its own gains): fit gains that are smooth
      in time.  ``gain_time_basis``: real ``[Ntimes, L]`` on the times of ``uvdata``; ``gain_time_scale``: a time in seconds, the basis
      is then ``modeling.gain_time_dpss_basis(times, gain_time_scale)``.  It stands alone (gains free per channel, smooth in time) or
      combines with ``gain_basis`` / ``gain_max_dly``.  All unskipped times of a polarization are then ONE joint fit on one device,
      ``g[t] = g_in[t] + sum_l Bt[t, l] (B) y[l]`` with ``y`` shared by the times (``HipFitSolver.set_gain_time_basis``); the
      per-slice host work (skip test, rms scale, weights, initial coefficients, write-back, post-hoc renormalisation, residual) is
      that of the batched path.  A skipped time is flagged as always; ``Bt`` is evaluated on all times and the rows of the fitted
      ones are used (its first columns, should fewer times be fitted than it has columns).  The joint fit has ONE loss, the sum over
      its times: ``tol`` acts on that sum, and ``fit_history[pol][t]["loss"]`` is that same list for every fitted ``t``.
      ``model_regularization="sum"`` uses one pair of sums for the joint fit, ``S = sum_t S_t`` and ``P = sum_t P_t`` with every
      time's weights normalised as before: the per-slice regulariser exactly only for one time.  Refused with ``ValueError``:
      ``init_guesses_from_previous_time_step`` (a chain is not a joint fit), ``batch_slices=False``, ``batch_slices=N`` below the number
      of times (the times share variables: one batch, whose device memory is that of the same times batched -- ``_auto_batch``'s
      sizing does not apply, ``gpu_memory_limit`` does), ``parallel_fits > 1``, more than one device or a ``device_split``, and a basis
      that is complex, non-finite or of another shape.
    * ``fit_quality`` (default off: ``quality_array`` stays zero as in the reference, cal_utils.py:48): report where the residual power
      of every fitted slice sits.  With ``e = w |d - g_i conj(g_j) m|^2`` in the fit's own units (``w`` the weights the fit used,
      ``m`` the returned model before gains, ``g`` the returned gains, evaluated before any post-hoc renormalisation, which leaves the
      product unchanged) and ``rms`` the slice's data scale: ``gains.quality_array[a, f, t, pol] = rms^2 sum_{b with a} e / sum_{b with a} w``,
      the weighted mean squared residual of antenna ``a``'s baselines in the data's units; ``gains.total_quality_array[f, t, pol]``
      (``(Nfreqs, Ntimes, Njones)``, created if ``None``) the same with both sums taken over all antennas;
      ``fit_history[polnum][time_index]["chisq_per_baseline"]`` a dict ``{(ant0, ant1): rms^2 sum_f e / sum_f w}`` with antenna
      numbers, one entry per baseline of the fit.  0 where the weights sum to 0.  A skipped slice keeps zeros and has no dict.  One
      device pass after the fit (``HipFitSolver.fit_quality``); no step of the fit changes.
    * ``fit_errors`` / ``fit_errors_ridge`` (default off: no call changes by a bit): report how well the fit is determined
      (``HipFitSolver.fit_errors``: one device pass after the fit, at the reported parameters, on the data and weights the fit used).
      ``fit_history[polnum][time_index]["errors"]`` holds ``leverage_per_baseline`` (the parameters the model spent on each baseline)
      and ``chisq_red_per_baseline = chisq_bl / (nsamp_bl - leverage_bl)`` (``nan`` where the denominator is <= 0), dicts keyed by
      antenna numbers like ``chisq_per_baseline``; ``noise_scale = chisq / (n - p)`` with ``n`` the samples of non-zero weight and
      ``p = sum leverage + #{(a, f): den > 0}`` (1.0 with ``underdetermined = True`` where ``n - p < 1``); ``nsingular``.
      ``fit_errors="samples"`` adds ``model_std`` ``[rows, nfreqs]`` float32, the standard deviation of the model before the gains in the
      data's units, with ``antpairs`` (as large as the data, hence on request).  ``fit_history["gain_std"]``
      ``[Nants, Nfreqs, Ntimes, Njones]`` is ``sqrt(noise_scale gain_var)``, dimensionless, zero where the gain is flagged.  These are
      CONDITIONAL errors -- the gains held fixed for the model, the model and the other gains for a gain: the block diagonal of the
      Gauss-Newton matrix, which ignores the gain-foreground covariance and the degeneracies, so they are lower bounds.  With a gain
      basis (frequency or time) ``gain_std`` is absent: the variance of a basis gain is ``b_f^T N_a^-1 b_f`` with the projected normal
      matrix, which is not computed (``p`` then counts no gain parameters) unless ``gain_basis_errors`` is on.  With ``freeze_model``
      only the gain part runs (no leverage tables).
    * ``gain_basis_errors`` (default off: no call changes by a bit; a Python keyword only, a report and no fit-loop control; needs
      ``fit_errors`` and a gain basis -- ``gain_basis`` / ``gain_max_dly`` or ``gain_time_basis`` / ``gain_time_scale`` -- else
      ``ValueError``): the error bars of basis gains (``HipFitSolver.gain_basis_errors``, one more device pass where ``fit_errors`` runs,
      at the reported gains, with ``fit_errors_ridge``).  ``fit_history["gain_std"]`` is then ``sqrt(noise_scale gain_var)`` with
      ``gain_var = b_f^T N_r^-1 b_f`` of the projected normal matrix (positive at flagged channels of an unflagged antenna: the basis
      interpolates), and ``p`` of ``noise_scale`` counts ``sum_a gain_dof[a]``, the parameters the basis gains spent; in a joint fit
      over ``T`` times every time is charged ``1 / T`` of an antenna's ``gain_dof``.  Model, residual, gains and every other history
      number keep their bits; ``noise_scale`` (and with it ``model_std``) grows with ``p``.  With ``freeze_model`` ``gain_std`` is the
      only error output.  The variances of the coefficients ``y`` stay at solver level.
    * ``gain_solve_sweeps`` / ``gain_solve_every`` / ``gain_solve_damping`` (defaults 0, 0, 0.5: descent only, no call changes by a bit):
      solve the gains in closed form.  With the foreground model held fixed the chi-square is linear least squares in one antenna's
      gain while the others are held fixed; a damped StefCal sweep (``HipFitSolver.solve_gains``) sets every antenna's gain to
      ``(1 - damping) g + damping num / den`` from the old gains of the others.  ``gain_solve_sweeps=N``: N sweeps on every fitted
      slice after its coefficients are initialised and before the first (unrecorded) descent step -- what a fit against a
      ``sky_model`` (with or without ``freeze_model``) otherwise spends hundreds of descent steps on.  ``gain_solve_every=K``: the
      recorded loop is issued in chunks of K steps, and between two chunks ``gain_solve_sweeps`` sweeps (1 if that is 0) run on the
      slices whose loop has not ended, with the optimizer's gain moments started over (stale momentum after a jump in the gains is
      harmful); no sweeps follow the last chunk, so the returned parameters are those of the last step (or of the lowest loss with
      ``use_min``) as always.  ``fit_history`` keeps one loss per recorded step.  The sweeps minimise the chi-square term only:
      the ``"sum"`` regulariser depends on the gains and is NOT part of the closed form; it is allowed, and the descent steps that
      follow see it as before.  Works in the loop, in batches and on several devices (``device_split="groups"`` sums the three planes
      of a sweep over the devices in one exchange).  ``ValueError`` when combined with ``gain_basis`` / ``gain_max_dly`` /
      ``gain_time_basis`` / ``gain_time_scale``.
    * ``coeff_solve_rounds`` / ``coeff_solve_ridge`` (defaults 0, 1e-6: off, no call changes by a bit): solve the foreground
      coefficients in closed form.  With the gains held fixed the chi-square is linear least squares in the coefficients of every
      fitting group; ``HipFitSolver.solve_coeffs`` solves ``(N + ridge tr(N) / nvec I) delta = rhs`` per group and adds ``delta``.
      ``coeff_solve_rounds=R``: at the point where the gain sweeps run (after the initial coefficients and the optimizer are set,
      before the first unrecorded descent step) R rounds of [one coefficient solve, then ``gain_solve_sweeps`` sweeps if that is
      > 0] -- alternating least squares.  Under ``gain_solve_every=K`` every between-chunk point runs one coefficient solve, with the
      optimizer's coefficient moments started over, in front of its sweeps, on the slices whose loop has not ended.  Allowed with
      ``gain_basis`` / ``gain_max_dly`` / ``gain_time_basis`` / ``gain_time_scale`` (the solve only reads the gains; the sweeps remain
      refused there).  ``ValueError`` with ``freeze_model``.  Like the sweeps it minimises the chi-square term only.
      ``fit_history[polnum][time_index]["coeff_solve_singular"]`` (present only with the feature on): the groups the last solve left
      alone because their normal matrix was singular (wholly flagged); in a batch the count is over the slices fitted together.
    * ``gain_basis_solve_sweeps`` / ``gain_basis_solve_every`` / ``gain_basis_solve_damping`` / ``gain_basis_solve_ridge`` (defaults 0, 0,
      0.5, 1e-6: off, no call changes by a bit): the closed-form sweeps for fits with ``gain_basis`` / ``gain_max_dly``
      (``HipFitSolver.solve_gain_coeffs``): the StefCal sweep projected on the basis ``g = g0 + B y``.  With ``num``, ``den`` the
      per-antenna sums of a per-channel sweep from the OLD gains, for antenna ``a``::

          r_a[f]  = num_a[f] - den_a[f] g_a[f]                 (complex; minus half the chi-square gradient w.r.t. g_a)
          N_a     = B^T diag(den_a) B                          [K][K], real symmetric
          rhs_a   = B^T r_a                                    [K], complex
          (N_a + ridge (tr N_a / K) I) delta_a = rhs_a         (one factorisation, two right-hand sides: re, im)
          y_a    <- y_a + damping delta_a                      then gains = g0 + B y for the whole array

      They act where ``gain_solve_sweeps`` / ``gain_solve_every`` act on per-channel fits, in the loop, in batches and on several
      devices: ``gain_basis_solve_sweeps=N`` sweeps after the optimizer is set and before the first unrecorded step; with
      ``coeff_solve_rounds=R``, R rounds of [coefficient solve, N sweeps]; ``gain_basis_solve_every=K``: the recorded loop in chunks of
      K steps, between two chunks one coefficient solve (if ``coeff_solve_rounds > 0``) and ``max(1, N)`` sweeps with the optimizer's
      ``y`` moments started over, on the slices whose loop has not ended.  A flagged channel of an antenna that has data elsewhere
      moves (the basis interpolates across it).  ``ValueError`` without ``gain_basis`` / ``gain_max_dly`` and with ``gain_time_basis`` /
      ``gain_time_scale`` (the joint system across times is a different solve).  The sweeps minimise the chi-square term only.
      ``fit_history[polnum][time_index]["gain_basis_solve_singular"]`` (present only with the feature on): the antenna rows the last
      sweep left alone (no unflagged cross-correlation, or a non-positive pivot); in a batch the count is over the slices fitted together.
    * ``gain_time_solve_sweeps`` / ``gain_time_solve_every`` / ``gain_time_solve_damping`` / ``gain_time_solve_ridge`` (defaults 0, 0,
      0.5, 1e-6: off, no call changes by a bit): the closed-form sweeps for the joint fit of ``gain_time_basis`` / ``gain_time_scale``
      (``HipFitSolver.solve_gain_time_coeffs``), with or without ``gain_basis`` / ``gain_max_dly``.  ``num``, ``den`` are the per-row sums
      of a per-channel sweep from the OLD gains, ``r = num - den g``; with a frequency basis (``n = L K``, index ``l K + k``),
      ``M_{t,a} = B^T diag(den_{t,a}) B``::

          N_a[(l,k),(l',k')] = sum_t Bt[t,l] Bt[t,l'] M_{t,a}[k,k']          rhs_a[(l,k)] = sum_t Bt[t,l] (B^T r_{t,a})[k]
          (N_a + ridge (tr N_a / n) I) delta_a = rhs_a                        y_a <- y_a + damping delta_a

      and without one, per (antenna, channel), ``N_{a,f}[l,l'] = sum_t Bt[t,l] Bt[t,l'] den[t,a,f]``,
      ``rhs_{a,f}[l] = sum_t Bt[t,l] r[t,a,f]``, ridge ``ridge tr N_{a,f} / L``.  They act where ``gain_basis_solve_sweeps`` /
      ``gain_basis_solve_every`` act: ``gain_time_solve_sweeps=N`` sweeps after the optimizer is set; with ``coeff_solve_rounds=R``, R
      rounds of [coefficient solve, N sweeps]; ``gain_time_solve_every=K``: the recorded loop in chunks of K steps, between two chunks
      one coefficient solve (if ``coeff_solve_rounds > 0``) and ``max(1, N)`` sweeps with the optimizer's ``y`` moments started over.
      An antenna flagged at some times only is solved and its gains there move (the time basis interpolates).  ``ValueError`` without
      ``gain_time_basis`` / ``gain_time_scale`` and together with ``gain_basis_solve_*`` or ``gain_solve_*``.  The sweeps minimise the
      chi-square term only.  ``fit_history[polnum][time_index]["gain_time_solve_singular"]`` (present only with the feature on): the
      systems the last sweep left alone (antennas with a frequency basis, (antenna, channel) pairs without one).
    * ``layout``: "shared" (default; baselines alias the distinct basis blocks) or "stream" (every baseline owns its tiles).
    * ``robust_every`` / ``robust_rounds`` / ``robust_kind`` / ``robust_threshold`` (defaults 0, 0, ``"huber"``, 3.0: a plain weighted
      chi-square, no call changes by a bit and no new kernel is launched): iteratively reweighted least squares against outliers that
      escaped the flags.  ``robust_every=K``: the recorded loop is issued in chunks of K steps (the machinery of ``gain_solve_every``,
      held slices included); between two chunks the weights of the slices whose loop has not ended are recomputed from the residual at
      the current parameters (``HipFitSolver.robust_weights``), at most ``robust_rounds`` times (0: after every chunk).  With ``w0`` the
      slice's weights as tensorized, ``e = w0 |d - g_i conj(g_j) (A c)|^2``, ``med_b`` the lower median of ``e`` over the unflagged
      channels of baseline ``b``, ``scale_b = med_b / ln 2``, ``z2 = e / scale_b`` and ``k = robust_threshold`` (in sigma):
      ``huber: psi = 1 if z2 <= k^2 else k / sqrt(z2)``, ``cauchy: psi = 1 / (1 + z2 / k^2)``, ``clip: psi = 1 if z2 <= k^2 else 0``,
      ``w = w0 psi``.  Every reweight starts from ``w0``; the weights are not renormalised, so the losses of different chunks are
      under different weights -- ``use_min`` together with ``robust_every`` raises ``ValueError``.  Together with ``gain_solve_every`` /
      ``gain_basis_solve_every`` / ``gain_time_solve_every`` both use ONE chunk length (``ValueError`` if they differ), and in the gap
      the reweight comes first, then the coefficient solve and the sweeps.  A baseline that is bad at every channel is not caught (its
      own median scales it): that is what ``fit_quality`` reports.  ``fit_history[pol][t]["robust"] = {"rounds": n, "downweighted":
      {(ant0, ant1): count}, "scale": {(ant0, ant1): rms^2 scale_b}}`` from the slice's last reweight.  ``fit_quality=True`` then
      reports under the robust weights.  The model, residual and flag outputs are computed as always: no sample is flagged.
    * ``gauss_newton_rounds`` / ``gauss_newton_every`` / ``gauss_newton_cg_iters`` / ``gauss_newton_lambda`` / ``gauss_newton_cg_tol``
      (defaults 0, 0, 20, 1e-3, 1e-3: off, no call changes by a bit and no new kernel is launched): Levenberg-damped Gauss-Newton steps over
      gains and coefficients TOGETHER (``HipFitSolver.gauss_newton_step``).  The descent loop is first-order and the closed forms above
      are block-wise: alternated they stall in the valley where gains and foregrounds trade against each other.  A step solves
      ``(N + lambda D) p = rhs`` with the joint ``N = J^H W J``, ``rhs`` minus half the chi-square gradient and ``D`` a diagonal estimate of
      ``N``, by ``gauss_newton_cg_iters`` iterations of preconditioned conjugate gradients (stopped early at a relative residual of
      ``gauss_newton_cg_tol``), and keeps the trial parameters iff the slice's loss (regulariser included) is finite and strictly lower.
      ``gauss_newton_rounds=R``: R steps after the rounds of ``coeff_solve_rounds`` and the start-up sweeps, before the first unrecorded
      descent step.  ``gauss_newton_every=K``: the recorded loop in chunks of K steps (one chunk length for every ``*_every``,
      ``ValueError`` if they differ); in every gap, after the reweighting, the coefficient solve and the sweeps, one step on the slices
      whose loop has not ended, with the optimizer's slots of the accepted slices started over.  The damping is kept per slice:
      ``gauss_newton_lambda`` at first, a tenth after an accepted step, ten times ``max(lambda, 1e-6)`` after a rejected one; a rejected
      start-up round is simply followed by the next.  ``ValueError`` with ``gain_basis`` / ``gain_max_dly``, ``gain_time_basis`` /
      ``gain_time_scale``, ``freeze_model`` (the sweeps are the exact answer for gains alone) and with several devices that share out the
      fitting groups (``device_split="groups"`` or the automatic choice of it; ``device_split="slices"`` works).
      ``fit_history[polnum][time_index]["gauss_newton"] = {"steps", "accepted", "lambda", "loss", "cg_iters"}`` (present only with the
      feature on): the steps the slice took part in, how many were accepted, the damping a next step would use, and per step the
      loss after it and the iterations it ran.
    * ``lbfgs_steps`` / ``lbfgs_every`` / ``lbfgs_history`` / ``lbfgs_max_ls`` / ``lbfgs_ftol`` (no counterpart in the reference): L-BFGS with
      a backtracking Armijo line search over the optimizer's own variables (``HipFitSolver.lbfgs``): the gains -- with ``gain_basis`` /
      ``gain_max_dly`` / ``gain_time_basis`` / ``gain_time_scale`` the basis coefficients -- and the foreground coefficients, or with
      ``freeze_model`` the gains alone.  It needs only the loss and its gradient, so it is the curvature-aware move of the fits the
      Gauss-Newton step refuses.  ``lbfgs_steps=N``: N iterations after the start-up rounds and the Gauss-Newton rounds, before the first
      unrecorded descent step.  ``lbfgs_every=K`` (needs ``lbfgs_steps``): the recorded loop in chunks of K steps (one chunk length for every
      ``*_every``) and N iterations last in every gap, on the slices still running, whose optimizer slots start over where they moved.
      ``lbfgs_history`` stored pairs (1 .. 16), ``lbfgs_max_ls`` trials per line search, ``lbfgs_ftol``: a slice's iterations stop once
      the loss falls by no more than this fraction (0: never).  Refused with several devices that share out the fitting groups
      (``device_split="groups"`` or the automatic choice of it; ``device_split="slices"`` works).
      ``fit_history[polnum][time_index]["lbfgs"] = {"calls", "iters", "evals", "loss", "status"}`` (present only with the feature on): the
      calls the slice took part in, its iterations and trial losses over all of them, the loss after every call, the status of the last.
    * ``delay_spectrum`` (``False`` | ``True`` | ``"baselines"``; default off: no call changes by a bit and no new kernel is launched),
      ``delay_spectrum_taper`` (``"bh4"`` | ``"none"`` | an array ``[Nfreqs]``), ``delay_spectrum_max_dly`` (ns; ``None``: all delays),
      ``delay_spectrum_bllen_bin`` (metres), ``delay_spectrum_calibrated``: report where the power of data, model and residual of every
      fitted slice sits in delay (``HipFitSolver.delay_spectrum``: one device pass after the fit, at the reported parameters, on the data
      and flags the fit used; the operator is ``modeling.delay_transform``).  ``fit_history[polnum][time_index]["delay_spectrum"]`` holds
      ``delays_ns`` ``[Ndelays]``, ``bllen_m`` ``[nbins]`` (the mean length of each bin's baselines; bin ``floor(length / width)``, only the
      bins that hold a baseline), ``nbls`` ``[nbins]`` (the baselines of the bin with an unflagged channel) and ``data``, ``model``,
      ``resid`` ``[nbins, Ndelays]``: the mean over the bin's baselines of ``|sum_f mask t_f x_f exp(-2 pi i f k / Nfreqs)|^2 / sum_f mask t_f^2``
      in the data's units squared, with ``x`` = data, gains x model, data - gains x model (``delay_spectrum_calibrated``: data / gains,
      model, their difference) and ``mask`` the samples of non-zero weight.  ``"baselines"`` adds ``per_baseline``: ``{(ant0, ant1):
      {"data", "model", "resid"}}`` with antenna numbers, ``[Ndelays]`` each.  A baseline is transformed the way round the fit holds it
      (the antenna pairs of ``fg_model_comps_dict``, the keys of ``per_baseline``): held as ``(j, i)`` its spectrum is the mirror image
      in delay of ``(i, j)``'s.  A joint time-basis fit reports every time on its own.
      ``ValueError`` before any device work for an unknown taper, a bin width that is not positive, a negative ``delay_spectrum_max_dly``.
    * ``delay_redundant_spectrum`` (``False`` | ``True`` | ``"groups"``), ``delay_redundant_times`` (1 .. 64), ``delay_redundant_taper``,
      ``delay_redundant_weighting`` (``"weights"`` | ``"uniform"``) (Python keywords only; default off: no call changes by a bit and no new
      kernel is launched; needs ``delay_spectrum`` on, ``delay_spectrum_calibrated=True`` -- an average of uncalibrated rows of different
      antennas decoheres -- and batches that hold a window, under the rules of ``delay_fringe_spectrum`` for ``batch_slices`` and
      ``init_guesses_from_previous_time_step``; ``device_split="groups"`` is refused; else ``ValueError`` before anything is touched): delay /
      fringe-rate power of the redundant groups' AVERAGES (``HipFitSolver.delay_coherent_spectrum``: one more device pass, at the reported
      gains).  The calibrated rows of every group of ``modeling.get_redundant_grps_data`` (tolerance 1 m, this call's ``include_autos``) are
      averaged per channel over the unflagged members -- weighted by the fit's weights, or uniformly --, a row that holds a pair reversed
      conjugated; the averages of ``delay_redundant_times`` consecutive slices (the windows of ``delay_fringe_windows``) are then transformed
      and squared as the delay / fringe-rate plane is: noise power falls as 1 / N in the group size, where the mean of the baselines'
      powers cannot.  Every member of a window gets ``["delay_spectrum"]["redundant"]``: ``time_indices``, ``fringe_rates`` (Hz),
      ``bllen_m`` (``baseline_length_bins`` on the GROUPS' lengths at ``delay_spectrum_bllen_bin``), ``ngroups`` the counted groups per
      bin, ``nmembers`` the rows per group, ``data``, ``model``, ``resid`` ``[nbins, Nrates, Ndelays]`` -- the MEAN over the bin's groups,
      data's units squared; ``"groups"`` adds ``groups``, every group's own plane keyed by its first antenna pair, with its member pairs.
    * ``delay_fringe_spectrum`` (``False`` | ``True`` | ``"baselines"``), ``delay_fringe_times`` (2 .. 64), ``delay_fringe_taper`` (Python
      keywords only; default off: no call changes by a bit and no new kernel is launched; needs ``delay_spectrum`` on and batches that
      hold a window, else ``ValueError`` before anything is touched -- ``batch_slices`` ``False`` or below ``delay_fringe_times`` and
      ``init_guesses_from_previous_time_step`` are refused; an automatic batch size becomes a multiple of ``delay_fringe_times``): the
      delay / fringe-rate plane (``HipFitSolver.delay_fringe_spectrum``: one more device pass beside the spectrum's, at the reported
      gains, with the spectrum's operator, taper along frequency, bins and ``delay_spectrum_calibrated``; along time the tapered DFT of
      ``modeling.fringe_rate_transform`` at the data's median spacing).  Inside a batch the unskipped slices are cut into windows in
      order (``delay_fringe_windows``): every run of ``delay_fringe_times`` slices of one polarization whose time indices rise by
      exactly 1; windows do not overlap and do not span batches; slices left over belong to no window; a window that is not evenly
      spaced to 1 % is a ``ValueError``.  A joint time-basis fit is cut the same way.  Every member of a window gets
      ``["delay_spectrum"]["fringe"]``: ``time_indices``, ``fringe_rates`` (Hz, ascending), ``data``, ``model``, ``resid``
      ``[nbins, Nrates, Ndelays]`` -- the MEAN over the bin's baselines of ``|Z|^2 / norm`` under the COMMON mask of the window's times,
      data's units squared --, and ``nbls``; ``"baselines"`` adds ``per_baseline`` keyed by antenna numbers.  A slice outside every
      window has no ``"fringe"`` key.  Several devices are refused with ``ValueError`` where a window's rows would lie on two of them.
    * ``delay_cross_spectrum`` (``False`` | ``True`` | ``"baselines"``; a Python keyword only; default off: no call changes by a bit and no
      new kernel is launched; needs ``delay_spectrum`` on and batching, else ``ValueError`` before anything is touched -- ``batch_slices``
      ``False`` or 1 and ``init_guesses_from_previous_time_step`` are refused; an automatic batch size becomes even): delay power that
      the noise does not bias (``HipFitSolver.delay_cross_spectrum``: one more device pass beside the spectrum's, at the reported gains,
      with the spectrum's operator, taper, bins and ``delay_spectrum_calibrated``).  Inside a batch the unskipped slices are paired in
      order (``delay_cross_pairing``): slices ``i`` and ``i + 1`` pair when they share the polarization and their time indices differ by
      exactly 1, and the walk moves on by two; otherwise slice ``i`` stays unpaired.  A joint time-basis fit pairs the same way.  Both
      members of a pair get ``["delay_spectrum"]["cross"]``: ``partner_time_index``, ``data``, ``model``, ``resid`` ``[nbins, Ndelays]`` -- the
      MEAN over the bin's baselines of ``Re(X_t conj(X_t')) / norm`` under the COMMON mask of the two times, data's units squared, signed --,
      ``noise`` with the same three for the mean half-difference power ``|X_t - X_t'|^2 / (2 norm)``, the noise spectrum measured from the
      data, and ``nbls``; ``"baselines"`` adds ``per_baseline`` keyed by antenna numbers.  An unpaired slice has no ``"cross"`` key.
    * ``delay_transfer`` / ``delay_transfer_ridge`` (default off: no call changes by a bit and no new kernel is launched; needs
      ``delay_spectrum`` on and a fitted model, else ``ValueError`` before anything is touched -- ``freeze_model=True`` is refused): the
      signal loss of the fit in delay space (``HipFitSolver.delay_transfer``: one more device pass beside the spectrum's, at the reported
      gains, with the spectrum's operator, bins and ``delay_spectrum_calibrated``).  The foreground basis absorbs every component of the
      data in its span, so a residual spectrum is biased low near the edge of the basis.  The ``"delay_spectrum"`` entry gains
      ``"transfer"`` ``[bins, Ndelays]`` = ``1 - absorbed_bin / count_bin``, the share of the power of a signal that is white in delay
      which survives the fit (dimensionless: no ``rms`` factor; the gains held fixed: an upper bound on the transfer; 0 for a bin without
      a counted row), ``"transfer_nsingular"`` (singular groups of the device call that held the slice) and, with
      ``delay_spectrum="baselines"``, ``"transfer_per_baseline"`` keyed like ``"per_baseline"``.  ``delay_transfer_ridge`` is the ridge of
      the factorisation, as ``fit_errors_ridge``.
    * ``fix_degeneracies`` (``False`` | ``True`` = ``"channel"`` | ``"band"``; default off: no call changes by a bit and no new kernel is
      launched), ``degeneracy_iters`` (6), ``degeneracy_phase_ref`` (``True``): refer every fitted slice to ``sky_model`` before it is
      written (``HipFitSolver.fix_degeneracies``: one device pass after the fit).  The fit constrains only ``g_i conj(g_j) m``; an overall
      amplitude, an overall phase and a phase gradient across the array are free per channel because the model absorbs them.  The call
      estimates the amplitude ``e^{eta}`` and tilt ``Phi`` (rad / m, east and north) that bring the fitted model onto the sky model (the
      slice's ``tensorize_data`` rows of it; weights: the sky model's own times ``data weights > 0``; positions: the antenna positions of
      ``uvdata``) and, with ``degeneracy_phase_ref``, the phase against the gains the fit started from, and writes
      ``g e^{-eta} e^{-i (Phi.r + psi)}`` and ``m e^{2 eta} e^{i Phi.d}`` instead of ``g`` and ``m``: gains of different times, nights
      and runs then refer to the same sky.  ``"band"``: one amplitude and one sky shift ``Phi(f) = (nu_f / mean nu) Phi_0`` per slice.
      ``resid`` does not change (to rounding), nor do quality, errors and delay spectra, which are taken before the transformation; the
      values handed to the next time (``init_guesses_from_previous_time_step``) stay the raw fitted ones; the slice's plane of
      ``fit_history["gain_std"]`` is multiplied by ``e^{-eta}``.  ``fit_history[polnum][time_index]["degeneracies"]`` holds ``mode``,
      ``amplitude``, ``phase``, ``nsamples``, ``last_step`` ``[Nfreqs]``, ``tilt`` ``[Nfreqs, 2]`` and ``iters``; ``last_step`` (radians on
      the longest baseline) tells a tilt outside the basin of about pi / 2.  ``ValueError`` before any device work for an unknown value,
      ``degeneracy_iters < 1``, ``sky_model=None``, ``freeze_model``, ``model_regularization="post_hoc"`` (both set the amplitude) and
      several devices that share out the fitting groups of a slice (``device_split="slices"`` works).
    * ``parallel_fits`` (default 1): with ``batch_slices=False``, fits that many slices concurrently, each on its own
      solver and HIP stream.
    (Nothing here is steered by environment variables: layout, devices and concurrency are arguments.)"""
    degen_mode = check_degeneracy_keywords(fix_degeneracies, degeneracy_iters, sky_model, freeze_model, model_regularization, devices, device_split)
    if gain_basis is not None and gain_max_dly is not None:
        raise ValueError("give gain_basis or gain_max_dly, not both")
    _check_delay_spectrum(delay_spectrum, delay_spectrum_taper, delay_spectrum_max_dly, delay_spectrum_bllen_bin)
    _check_delay_transfer(delay_transfer, delay_transfer_ridge, delay_spectrum, freeze_model)
    _check_delay_cross(delay_cross_spectrum, delay_spectrum, batch_slices, init_guesses_from_previous_time_step)
    _check_delay_fringe(delay_fringe_spectrum, delay_fringe_times, delay_fringe_taper, delay_spectrum, batch_slices, init_guesses_from_previous_time_step)
    _check_delay_redundant(delay_redundant_spectrum, delay_redundant_times, delay_redundant_taper, delay_redundant_weighting, delay_spectrum,
                           delay_spectrum_calibrated, batch_slices, init_guesses_from_previous_time_step, device_split)
    controls = FitControls.pick(locals())
    controls.check(gain_basis is not None or gain_max_dly is not None, gain_time_basis is not None or gain_time_scale is not None, freeze_model, use_min)
    if gain_max_dly is not None:
        gain_basis = modeling.gain_dpss_basis(np.asarray(uvdata.freq_array, dtype=np.float64).ravel(), gain_max_dly)
    if gain_time_basis is not None and gain_time_scale is not None:
        raise ValueError("give gain_time_basis or gain_time_scale, not both")
    if gain_time_basis is not None or gain_time_scale is not None:
        if init_guesses_from_previous_time_step:
            raise ValueError("a gain time basis fits all times jointly: init_guesses_from_previous_time_step (a chain over the times) contradicts it")
        if batch_slices is not None and not batch_slices:
            raise ValueError("a gain time basis fits all times jointly: batch_slices=False (the loop over the times) contradicts it")
        if parallel_fits is not None and parallel_fits > 1:
            raise ValueError("a gain time basis fits all times jointly: parallel_fits > 1 (concurrent fits of single times) contradicts it")
        if device_split is not None or isinstance(devices, str) or (devices is not None and len(list(devices)) > 1):
            raise ValueError("a gain time basis fits on one device: give devices=None or one device index, and no device_split")
    if gain_basis is not None:
        gain_basis = _check_gain_basis(gain_basis, uvdata.Nfreqs)
    if gain_time_scale is not None:
        gain_time_basis = modeling.gain_time_dpss_basis(np.unique(uvdata.time_array), gain_time_scale)
    if gain_time_basis is not None:
        ntimes_all = len(np.unique(uvdata.time_array))
        gain_time_basis = _check_gain_time_basis(gain_time_basis, ntimes_all)
        if batch_slices is not None and batch_slices is not True and int(batch_slices) < ntimes_all:
            raise ValueError(f"a gain time basis fits all {ntimes_all} times of a polarization as ONE fit, which batch_slices={batch_slices} cannot "
                             "hold: the times share their variables and cannot be split into smaller batches")
    antpairs_data = uvdata.get_antpairs()
    if not include_autos:
        antpairs_data = set([ap for ap in antpairs_data if ap[0] != ap[1]])
    if len(antpairs_data) != len(uvdata.get_antpairs()):
        uvdata = uvdata.select(inplace=False, bls=[ap for ap in antpairs_data])
    # (with nothing to drop the input object itself is used: it is only read from here on, and the reference's
    # select(inplace=False) copy of a gigabyte of visibilities bought nothing but that guarantee)
    resid = _blank_copy(uvdata, keep_flags=True)  # its visibilities are written slice by slice (_output_finisher): data - gains x model
    model = _blank_copy(uvdata)
    unity_gains = gains is None
    if gains is None:
        echo(f"{datetime.datetime.now()} Gains are None. Initializing gains starting with unity...\n", verbose=verbose)
        gains = cal_utils.blank_uvcal_from_uvdata(uvdata)
    if fit_quality and getattr(gains, "total_quality_array", None) is None:
        # (here, once, not by whichever slice is written first: with parallel_fits the slices are written from several threads)
        gains.total_quality_array = np.zeros(gain4(gains.quality_array).shape[1:], dtype=np.float64)
    errs = None
    if _fit_errors_mode(fit_errors):
        if not (np.isfinite(float(fit_errors_ridge)) and float(fit_errors_ridge) >= 0.0):
            raise ValueError(f"fit_errors_ridge must be finite and >= 0, got {fit_errors_ridge!r}")
        with_gains = gain_basis is None and gain_time_basis is None
        if gain_basis_errors and with_gains:
            raise ValueError("gain_basis_errors needs a gain basis (gain_basis / gain_max_dly or gain_time_basis / gain_time_scale): fit_errors alone "
                             "reports gain_std of free per-channel gains")
        errs = dict(samples=fit_errors == "samples", ridge=float(fit_errors_ridge), with_gains=with_gains, basis_gains=bool(gain_basis_errors),
                    gain_std=np.zeros(gain4(gains.gain_array).shape, dtype=np.float64) if with_gains or gain_basis_errors else None)
    elif gain_basis_errors:
        raise ValueError("gain_basis_errors needs fit_errors=True or 'samples': it adds the basis gains' error bars to that report")
    if sky_model is None and model_regularization is not None:
        echo(f"{datetime.datetime.now()} Sky model is None. Initializing from data...\n", verbose=verbose)
        # data / (g_i conj(g_j)) with the initial gains (:1131-1136).  With the unity, unflagged gains built just above that is
        # the data themselves: the sky model is only read from here on, so the input object stands in for the gigabyte copy
        sky_model = uvdata if unity_gains else cal_utils.apply_gains(uvdata, gains)
    else:
        # the reference dereferences sky_model here even when it is None (calibration.py:1137-1138)
        sky_model = sky_model.select(inplace=False, bls=[ap for ap in antpairs_data])
    fit_history = {}
    ants_map = {ant: i for i, ant in enumerate(np.asarray(gains.ant_array).tolist())}
    prob, _ = tensorize_fg_model_comps_dict(
        fg_model_comps_dict=fg_model_comps_dict,
        ants_map=ants_map,
        dtype=dtype,
        nfreqs=sky_model.Nfreqs,
        verbose=verbose,
        notebook_progressbar=notebook_progressbar,
        use_redundancy=use_redundancy,
        grp_size_threshold=grp_size_threshold,
    )
    echo(f"{datetime.datetime.now()}Finished Converting Foreground Modeling Components to Tensors...\n", verbose=verbose)
    del fg_model_comps_dict
    dspec = None
    if delay_spectrum:
        dspec = delay_spectrum_setup(uvdata, gains.ant_array, prob, taper=delay_spectrum_taper, max_dly=delay_spectrum_max_dly,
                                     bllen_bin=delay_spectrum_bllen_bin, calibrated=delay_spectrum_calibrated,
                                     per_baseline=delay_spectrum == "baselines")
        if delay_transfer:
            dspec["transfer_ridge"] = float(delay_transfer_ridge)
        dspec["cross"] = {False: None, True: "bins", "baselines": "baselines"}[delay_cross_spectrum]
        if delay_fringe_spectrum:
            dspec["fringe"] = delay_fringe_setup(np.unique(uvdata.time_array), delay_fringe_times, delay_fringe_taper, delay_fringe_spectrum == "baselines")
        if delay_redundant_spectrum:
            dspec["redundant"] = delay_redundant_setup(uvdata, gains.ant_array, prob, delay_redundant_times, delay_redundant_taper, delay_redundant_weighting,
                                                       delay_redundant_spectrum == "groups", delay_spectrum_bllen_bin, include_autos=include_autos)
    degen = degeneracy_setup(uvdata, gains.ant_array, degen_mode, degeneracy_iters, degeneracy_phase_ref) if degen_mode is not None else None
    if parallel_fits is None:
        parallel_fits = 1
    if init_guesses_from_previous_time_step:
        parallel_fits = 1
    times = np.unique(uvdata.time_array)
    if batch_slices is None:
        batch_slices = (parallel_fits <= 1 or gain_time_basis is not None or bool(delay_cross_spectrum) or bool(delay_fringe_spectrum)
                        or bool(delay_redundant_spectrum))
    if init_guesses_from_previous_time_step:
        batch_slices = False  # every time starts from the previous one's result: a chain, not a batch
    # the call's settings, once, for the loop and the batches alike (slice_pipeline's stages read them)
    cfg = types.SimpleNamespace(
        uvdata=uvdata, sky_model=sky_model, gains=gains, resid=resid, model=model, prob=prob, ants_map=ants_map, times=times, weights=weights,
        nsamples_in_weights=nsamples_in_weights, dtype=np.dtype(dtype), skip_threshold=skip_threshold, use_model_snr_weights=use_model_snr_weights,
        optimizer=optimizer, opt_kwargs=opt_kwargs, use_min=use_min, freeze_model=freeze_model, tol=tol, maxsteps=maxsteps,
        n_profile_steps=n_profile_steps, profile_log_dir=profile_log_dir, model_regularization=model_regularization, verbose=verbose,
        devices=devices, layout=layout, device_split=device_split, gain_basis=gain_basis, gain_time_basis=gain_time_basis, fit_quality=fit_quality,
        controls=controls, errs=errs, dspec=dspec, degen=degen,
        finish=_output_finisher(uvdata, model, resid, gains, correct_model, correct_resid))
    if batch_slices:
        if gain_time_basis is not None:
            # the joint fit of a polarization holds all of its times, whatever _auto_batch would make of them: its device memory is
            # about that of the same times as one batch (gpu_memory_limit raises MemoryError as for any batch)
            max_batch = len(times)
        else:
            max_batch = _auto_batch(prob, dtype, layout) if batch_slices is True else max(1, min(int(batch_slices), _lib_max_slices()))
            if delay_cross_spectrum and batch_slices is True:
                max_batch = max(2, max_batch) // 2 * 2  # the times are paired inside a batch: an even number of them
            if delay_fringe_spectrum and batch_slices is True:
                n = int(delay_fringe_times) * (2 if delay_cross_spectrum and int(delay_fringe_times) % 2 else 1)
                max_batch = max(n, max_batch) // n * n  # whole windows inside a batch (and whole pairs, where both are asked for)
            if delay_redundant_spectrum and batch_slices is True:
                n = int(np.lcm.reduce([int(delay_redundant_times), 2 if delay_cross_spectrum else 1, int(delay_fringe_times) if delay_fringe_spectrum else 1]))
                max_batch = max(n, max_batch) // n * n  # whole windows of the redundant averages too
        fit_history = _fit_slices_batched(cfg, max_batch)
        _file_gain_std(fit_history, errs, gains)
        return model, resid, gains, fit_history  # (every fitted slice left its write-back in its final state)
    assert gain_time_basis is None, "a gain time basis must not reach the loop over single times"
    if layout is not None:
        prob.__dict__["_layout"] = layout
    if devices is not None:
        prob.__dict__["_device"] = 0 if isinstance(devices, str) else int(list(devices)[0])  # the loop fits on one device

    def fit_slice(polnum, pol, time_index, time, carry):
        """One (polarization, time) slice: calibration.py:1167-1330, a batch of one on this thread's solver.  ``carry`` holds the
        parameters handed from one time to the next when init_guesses_from_previous_time_step is set."""
        echo(f"{datetime.datetime.now()} Working on time {time_index + 1} of {uvdata.Ntimes}...\n", verbose=verbose)
        sl = slice_pipeline.tensorize(cfg, dict(polnum=polnum, pol=pol, time_index=time_index, time=time))
        if sl is None:
            return None  # (the reference's fit_history[polnum] = "skipped!" (:1309) is overwritten at the end of the pol loop (:1321))
        arrs = slice_pipeline.gather([sl])
        solver = get_solver(prob, dtype)
        echo(f"Using {str(dtype)} precision.")  # (the lines of fit_gains_and_foregrounds, :447-738, which every fit of the loop prints)
        echo(f"{datetime.datetime.now()} Provided the following opt_kwargs")
        for k in opt_kwargs:
            echo(f"{k}: {opt_kwargs[k]}")
        OPTIMIZERS[optimizer]  # unknown optimizer -> KeyError, like calibration.py:571
        slice_pipeline.start(solver, 1, arrs, cfg, handed=carry.get("fitted") if init_guesses_from_previous_time_step else None)
        echo(f"{datetime.datetime.now()} Performing Gradient Descent...\n", verbose=verbose)
        result = drive(solver, controls, 1, prob.nbls, maxsteps, tol, use_min, freeze_model, n_profile_steps, profile_log_dir)
        out = slice_pipeline.report(solver, 1, arrs, cfg, result)
        carry["fitted"] = out["fitted"]  # (the raw fitted values, whatever fix_degeneracies writes)
        return slice_pipeline.write(cfg, sl, 0, out)

    # one pool for the whole call: its threads (and with them their solvers, get_solver) serve every polarization
    pool = concurrent.futures.ThreadPoolExecutor(max_workers=parallel_fits) if parallel_fits > 1 and len(times) > 1 else None
    for polnum, pol in enumerate(uvdata.get_pols()):
        echo(f"{datetime.datetime.now()} Working on pol {pol}, {polnum + 1} of {uvdata.Npols}...\n", verbose=verbose)
        if pool is not None:
            futures = [pool.submit(fit_slice, polnum, pol, ti, t, {}) for ti, t in enumerate(times)]
            hists = [fut.result() for fut in futures]
        else:
            carry = {}
            hists = [fit_slice(polnum, pol, ti, t, carry) for ti, t in enumerate(times)]
        fit_history[polnum] = {ti: hist for ti, hist in enumerate(hists) if hist is not None}
    if pool is not None:
        pool.shutdown()
    _file_gain_std(fit_history, errs, gains)
    return model, resid, gains, fit_history  # (every fitted slice left its write-back in its final state; a skipped one is flagged)


def _file_gain_std(fit_history, errs, gains):
    """``fit_history["gain_std"]`` of a call with ``fit_errors`` and free per-channel gains: zero where the gain is flagged."""
    if errs is not None and errs["gain_std"] is not None:
        fit_history["gain_std"] = np.where(gain4(gains.flag_array), 0.0, errs["gain_std"])


def _output_finisher(uvdata, model, resid, gains, correct_model, correct_resid):
    """``finish(pnum, time)``: residual and model of ONE (polarization, time) in the requested calibration state --
    calibration.py:1322-1331: ``model_with_gains = apply_gains(model, gains, inverse=True)``; ``resid = data - model_with_gains``,
    zero where the model (with gains) or the data are flagged; ``correct_resid``: ``resid / (g_i conj(g_j))``, flags or-ed with
    the gain flags; ``correct_model=False`` returns the model with gains.  The same arithmetic in the same order as those calls, in
    ONE pass over the slice's baseline-times (row chunks on the host's cores) instead of four passes and three container copies."""
    ants = np.asarray(gains.ant_array).astype(np.int64)
    order = np.argsort(ants)

    def ant_rows(a):
        a = np.asarray(a).astype(np.int64)
        pos = np.clip(np.searchsorted(ants[order], a), 0, len(ants) - 1)
        if not np.all(ants[order][pos] == a):
            raise KeyError(int(a[np.where(ants[order][pos] != a)[0][0]]))
        return order[pos]

    a0, a1 = ant_rows(uvdata.ant_1_array), ant_rows(uvdata.ant_2_array)
    gtimes = np.asarray(gains.time_array)
    utimes = np.unique(uvdata.time_array)
    tind = np.asarray([np.where(np.isclose(gtimes, t, rtol=0.0, atol=1e-7))[0][0] for t in utimes])
    gt = tind[np.searchsorted(utimes, np.asarray(uvdata.time_array))]
    udata, uflag = vis3(np.asarray(uvdata.data_array)), vis3(np.asarray(uvdata.flag_array))
    pols = list(uvdata.get_pols())

    def finish(pnum, time):
        # (the containers' arrays as they are NOW: the write-backs before this call may have attached new ones)
        mdata, mflag = vis3(model.data_array), vis3(model.flag_array)
        rdata, rflag = vis3(resid.data_array), vis3(resid.flag_array)
        garr, gflags = gain4(gains.gain_array), gain4(gains.flag_array)
        gindp = np.where(np.asarray(gains.jones_array) == polstr2num(pols[pnum], x_orientation=gains.x_orientation))[0][0]
        t = tind[np.where(np.isclose(utimes, time, rtol=0.0, atol=1e-7))[0][0]]
        gplane = np.ascontiguousarray(garr[:, :, t, gindp])
        fplane = np.ascontiguousarray(gflags[:, :, t, gindp])
        sel = np.where(gt == t)[0]
        contiguous = len(sel) == sel[-1] - sel[0] + 1

        def rows(lo, hi):
            r = slice(sel[0] + lo, sel[0] + hi) if contiguous else sel[lo:hi]
            gg = np.take(gplane, a0[r], axis=0)
            gg *= np.conj(np.take(gplane, a1[r], axis=0))
            gf = np.take(fplane, a0[r], axis=0) | np.take(fplane, a1[r], axis=0)
            mwg = mdata[r, :, pnum] * gg  # apply_gains(model, gains, inverse=True)
            mwf = mflag[r, :, pnum] | gf
            d = udata[r, :, pnum] - mwg
            d[mwf | uflag[r, :, pnum]] = 0.0
            if correct_resid:  # apply_gains(resid, gains)
                d /= gg
                rflag[r, :, pnum] |= gf
            rdata[r, :, pnum] = d
            if not correct_model:
                mdata[r, :, pnum] = mwg
                mflag[r, :, pnum] = mwf

        utils.for_row_chunks(rows, len(sel))

    finish.times, finish.npols = utimes, len(pols)
    return finish


def _finish_outputs(uvdata, model, resid, gains, fit_history, correct_model, correct_resid):
    """Every (polarization, time) through _output_finisher in one go (calibrate_and_model_tensor itself finishes every fitted slice
    as it is written, ``slice_pipeline.write``; a skipped slice is all flags and zeros, which finishing leaves as they are)."""
    finish = _output_finisher(uvdata, model, resid, gains, correct_model, correct_resid)
    for pnum in range(finish.npols):
        for time in finish.times:
            finish(pnum, time)
    return model, resid, gains, fit_history


def _lib_max_slices():
    from . import _lib

    return _lib.CAL_MAX_SLICES


def _auto_batch(prob, dtype, layout=None):
    """How many slices one batch may hold when the caller does not say: what fits a quarter of the host memory now available (five
    per-sample arrays per slice and their concatenation) and half a device's memory (about eight per-sample arrays per slice), at
    most the library's CAL_MAX_SLICES.  Tutorial-scale arrays batch hundreds of slices.  In the SHARED layout a slice of 10^7 samples
    or more goes alone: its step is bound by arithmetic, not by launches (HERA-350: 1.29 s per 1 000 steps and slice whether four
    slices are fitted together or one by one), and batches of one let the host work of neighbouring slices run under the fits
    (_fit_slices_batched).  The STREAM layout keeps batching at every size: its slices share the basis tiles they stream."""
    from . import _lib

    if (layout or "shared") == "shared" and float(prob.nbls) * prob.nfreqs >= 1.0e7:
        return 1
    per_array = float(prob.nbls) * prob.nfreqs * np.dtype(dtype).itemsize
    host_avail = 8.0e9
    try:
        with open("/proc/meminfo") as meminfo:
            for line in meminfo:
                if line.startswith("MemAvailable:"):
                    host_avail = float(line.split()[1]) * 1024.0
                    break
    except OSError:
        pass
    try:
        dev_total = float(_lib.device_info(_DEVICE["index"] or 0)["total_mem_bytes"])
    except Exception:  # noqa: BLE001 -- sizing only
        dev_total = 64.0e9
    n = min(0.25 * host_avail / (10.0 * per_array), 0.5 * dev_total / (8.0 * per_array))
    return int(max(1, min(n, _lib_max_slices())))


def _default_devices(nsamples_per_step=None):
    """Devices of a batched fit when the caller names none: the ONE device selected for the process (read_calibrate_and_model_dpss:
    calibration.py:1741-1753; device 0 otherwise).  Several devices are an explicit request -- ``devices=[0, 1, ...]`` or
    ``devices="all"`` -- because that path sets up an RCCL communicator between threads of this process (or none, with whole batches
    per device) that no default should stake a caller's run on before it has been exercised on multi-GPU hardware."""
    return [_DEVICE["index"] if _DEVICE["index"] is not None else 0]


def _resolve_devices(devices):
    """``devices`` keyword of the batched entry points: None (the process's device), "all" (every visible GPU) or a list of indices."""
    from . import _lib

    if devices is None:
        return _default_devices(), True
    if isinstance(devices, str):
        if devices != "all":
            raise ValueError(f"devices={devices!r}: None, 'all' or a list of device indices")
        return list(range(max(1, _lib.device_count()))), True  # ("all" is a wish, not a list: set-up failure falls back to one device, aloud)
    return [int(d) for d in devices], False


def _batch_fitter(prob, nt, dtype, layout, devices, joint=False):
    """The SliceBatchFitter of ``nt`` slices of these components (kept with them: a second call re-uses the device copy);
    ``joint``: the slices are one fit with one loop state (a gain time basis)."""
    from .batched import SliceBatchFitter

    cache = prob.__dict__.setdefault("_batch_fitters", {})
    key = (np.dtype(dtype).str, layout, tuple(devices), int(nt) if not joint else -int(nt), threading.get_ident())
    if key not in cache:
        for k in [k for k in cache if k[:3] == key[:3] and k[4] == key[4]]:  # another batch size of the same call: free it first
            cache.pop(k).close()
        fitter = SliceBatchFitter(prob, nt, dtype=dtype, layout=layout, devices=devices, joint=joint)
        limit = _DEVICE["memory_limit_gib"]
        if limit is not None and fitter.memory_bytes() > limit * 2.0**30:
            used = fitter.memory_bytes() / 2.0**30
            fitter.close()
            raise MemoryError(f"the fit needs {used:.2f} GiB of device memory, gpu_memory_limit is {limit} GiB")
        cache[key] = fitter
    return cache[key]


def _fit_slices_batched(cfg, max_batch):
    """The pol x time loop of calibration.py:1160-1331 with the fits of all unskipped slices issued as batches: per slice
    exactly the host-side steps of the loop body (``slice_pipeline``: skip test :1173-1177, rms scale :1178-1182, tensorize :1184-1233,
    write-back :1271-1300, post-hoc renormalisation :1311-1319, residual and calibration state of the outputs :1322-1331), the gradient
    descent of :1244-1269 for up to ``max_batch`` slices at once with per-slice loop control.  ``cfg``: the settings object of
    ``calibrate_and_model_tensor``.  Returns ``fit_history``; model, resid and gains are complete when it returns.
    ``cfg.gain_time_basis`` (``[len(times), L]``): the unskipped times of a polarization are one batch and one JOINT fit (one loop state,
    loss = the sum over the times; calibrate_and_model_tensor's docstring).  ``cfg.controls``: the closed-form, robust, Gauss-Newton and
    L-BFGS keywords of calibrate_and_model_tensor (``fit_loop.FitControls``)."""
    OPTIMIZERS[cfg.optimizer]  # unknown optimizer -> KeyError, like calibration.py:571
    prob, dtype, controls, degen, verbose = cfg.prob, cfg.dtype, cfg.controls, cfg.degen, cfg.verbose
    gain_basis, freeze_model, use_min, device_split = cfg.gain_basis, cfg.freeze_model, cfg.use_min, cfg.device_split
    layout = cfg.layout or "shared"
    pols = list(cfg.uvdata.get_pols())
    fit_history = {polnum: {} for polnum in range(len(pols))}
    todo = [dict(polnum=polnum, pol=pol, time_index=time_index, time=time) for polnum, pol in enumerate(pols) for time_index, time in enumerate(cfg.times)]
    devices, chose_devices = _resolve_devices(cfg.devices)
    joint = cfg.gain_time_basis is not None

    # One batch goes through three stages: prep (host: the slices' rows out of the containers), fit (device), post (host: the model
    # rows and gains back into the containers).  The stages of neighbouring batches overlap -- while the device fits batch k, one
    # host thread prepares batch k + 1 and another writes batch k - 1 back (NumPy and the library both release the GIL): with several
    # batches the host work of all but the first and the last disappears behind the fits.  The (polarization, time) slices of
    # different batches are disjoint parts of the containers, so the stages never touch the same rows.
    def prep(candidates):
        batch = [sl for sl in (slice_pipeline.tensorize(cfg, c) for c in candidates) if sl is not None]
        echo(f"{datetime.datetime.now()} {len(batch)} of {len(candidates)} (polarization, time) slices tensorized.\n", verbose=verbose)
        arrs = slice_pipeline.gather(batch) if batch else {}
        # (the slices keep their scalars only: the arrays live on in the batch's, which die with the fit)
        return dict(arrs, batch=[{k: v for k, v in sl.items() if not isinstance(v, np.ndarray)} for sl in batch])

    def fit(batch, arrs, on=None):
        nonlocal devices
        nt = len(batch)
        echo(f"{datetime.datetime.now()} Working on {nt} (polarization, time) slices together...\n", verbose=verbose)
        try:
            fitter = _batch_fitter(prob, nt, dtype, layout, devices if on is None else on, joint=joint)
        except Exception as err:  # noqa: BLE001
            if on is not None:
                raise
            # several devices were this function's own choice, not the caller's: when they cannot be set up together (communicator,
            # memory of a peer) the fit runs on the one selected device instead -- said aloud, never silently; an explicit devices=[...]
            # or a single device fails as it stands
            if not (chose_devices and len(devices) > 1):
                raise
            import warnings

            warnings.warn(f"calamity_amd: the fit could not be set up on devices {devices} ({type(err).__name__}: {err}); continuing on device {devices[0]}",
                          RuntimeWarning, stacklevel=2)
            devices = devices[:1]
            fitter = _batch_fitter(prob, nt, dtype, layout, devices, joint=joint)
        slice_pipeline.start(fitter, nt, arrs, cfg)
        result = drive(fitter, controls, 1 if joint else nt, nt * prob.nbls if joint else prob.nbls, cfg.maxsteps, cfg.tol, use_min, freeze_model,
                       cfg.n_profile_steps, cfg.profile_log_dir, dict(slices=nt))
        out = slice_pipeline.report(fitter, nt, arrs, cfg, result)
        echo(f"{datetime.datetime.now()} ... fitted.\n", verbose=verbose)
        return out

    def post(batch, out):
        for t, sl in enumerate(batch):
            fit_history[sl["polnum"]][sl["time_index"]] = slice_pipeline.write(cfg, sl, t, out)
        echo(f"{datetime.datetime.now()} {len(batch)} (polarization, time) slices written back.\n", verbose=verbose)

    batches = [todo[lo : lo + max_batch] for lo in range(0, len(todo), max_batch)]
    if joint:
        batches = [[sl for sl in todo if sl["polnum"] == polnum] for polnum in range(len(pols))]
    if device_split not in (None, "slices", "groups"):
        raise ValueError(f"device_split={device_split!r}: 'slices', 'groups' or None")
    D = len(devices)
    whole_slices = D > 1 and (device_split == "slices" or (device_split is None and len(batches) >= D))
    # (the caller's check over again, now that it is known whether the devices share out the groups of a slice)
    controls.check(gain_basis is not None, joint, freeze_model, use_min, groups_split=D > 1 and not whole_slices)
    if degen is not None and D > 1 and not whole_slices:
        raise ValueError(f"fix_degeneracies on devices {devices} that share out the fitting groups of a slice is not implemented (the channel sums would "
                         "need an exchange per iteration): use one device or device_split='slices'")
    if whole_slices:
        # Whole batches on different devices: device d fits batches d, d + D, ... on a thread of its own (its solvers live on that
        # thread), nothing is exchanged between devices, and every slice is fitted exactly as it would be on one device.  One prep
        # thread runs at most D + 1 batches ahead of the fits (a batch of HERA-350 rows is 1.3 GB); one thread writes back in order.
        permits, failed = threading.Semaphore(D + 1), threading.Event()

        def prep_when_allowed(candidates):
            permits.acquire()
            return dict(batch=[]) if failed.is_set() else prep(candidates)

        fit_threads = set()

        def fit_on(batch, holder, dev):
            fit_threads.add(threading.get_ident())
            try:
                if failed.is_set():  # (another batch has failed: the call is on its way out, no more maxsteps-long fits)
                    raise RuntimeError("an earlier batch of this call failed")
                return fit(batch, holder.pop(), on=[dev])  # the arrays (1.1-1.3 GB per HERA-350 slice) die with this frame
            except BaseException:
                failed.set()
                raise
            finally:
                permits.release()

        def post_of(batch, fitted):
            try:
                post(batch, fitted.result())
            except BaseException:
                failed.set()
                raise

        pools = [concurrent.futures.ThreadPoolExecutor(1) for _ in range(D + 2)]
        prep_pool, post_pool, fit_pools = pools[0], pools[1], pools[2:]
        try:
            # The prep futures are consumed front to back and dropped as they go: a Future keeps its result alive, and a list of
            # all of them held every batch's arrays until the call returned (60 times x 4 polarizations: ~240 GB of host memory).
            ahead = collections.deque(prep_pool.submit(prep_when_allowed, c) for c in batches)
            written, nfit = collections.deque(), 0
            while ahead:
                arrs = ahead.popleft().result()
                batch = arrs["batch"]
                if not batch:
                    permits.release()
                    continue
                fitted = fit_pools[nfit % D].submit(fit_on, batch, [arrs], devices[nfit % D])
                nfit += 1
                del arrs
                written.append(post_pool.submit(post_of, batch, fitted))
                while written and written[0].done():  # (a failed fit or write-back surfaces here, not after every other batch has been fitted)
                    written.popleft().result()
            while written:
                written.popleft().result()
        except BaseException:
            failed.set()
            for _ in range(len(batches) + D + 2):  # (nobody stays blocked behind the throttle)
                permits.release()
            raise
        finally:
            for pl in pools:
                pl.shutdown(wait=True)
            # the fitters of this call's fit threads (kept with the components, keyed by thread): their threads are gone, nobody
            # could reuse them -- their device memory goes back now
            cache = prob.__dict__.get("_batch_fitters", {})
            for key in [k for k in cache if k[4] in fit_threads]:
                cache.pop(key).close()
    elif len(batches) <= 1:
        for candidates in batches:
            arrs = prep(candidates)
            if arrs["batch"]:
                post(arrs["batch"], fit(arrs["batch"], arrs))
    else:
        with concurrent.futures.ThreadPoolExecutor(1) as prep_pool, concurrent.futures.ThreadPoolExecutor(1) as post_pool:
            ahead, written = prep_pool.submit(prep, batches[0]), []
            for k in range(len(batches)):
                arrs = ahead.result()
                if k + 1 < len(batches):
                    ahead = prep_pool.submit(prep, batches[k + 1])
                batch = arrs["batch"]
                if not batch:  # (every slice of it was skipped)
                    continue
                out = fit(batch, arrs)
                del arrs
                written.append(post_pool.submit(post, batch, out))
                for f in written[:-2]:  # (an exception of a write-back surfaces here, not at the end of the whole job)
                    f.result()
                written = written[-2:]
            for f in written:
                f.result()
    return fit_history


def _blank_copy(uvdata, keep_flags=False):
    """A copy of ``uvdata`` with all-zero visibilities and no flags (the reference deep-copies, then clears, :1113-1116;
    ``keep_flags``: the flags are copied), without copying the arrays that are about to be overwritten -- and without touching
    the input, which other holders of the object may be reading: the deep copy is told that the two big arrays are already
    copied (the memo maps them to placeholders), then fresh arrays are attached."""
    data, flags = uvdata.data_array, uvdata.flag_array
    hold_d, hold_f = np.zeros(0, dtype=np.asarray(data).dtype), np.zeros(0, dtype=bool)
    out = copy.deepcopy(uvdata, {id(data): hold_d, id(flags): hold_f})
    # (np.zeros: fresh zero pages from the operating system, touched when they are first written -- the write-back of a slice, which
    # runs beside the fits; zeros_like fills the gigabytes here and now)
    out.data_array = np.zeros(np.shape(data), dtype=np.asarray(data).dtype)
    out.flag_array = np.array(flags, copy=True) if keep_flags else np.zeros(np.shape(flags), dtype=bool)
    return out


def _insert_model_rows(uvdata, time, polarization, ants_map, prob, m_r, m_i, scale_factor):
    """insert_model_into_uvdata_tensor (calibration.py:741-795) from per-baseline rows instead of cubes: the row table of the
    time slice (``_baseline_rows``), then a single scatter; pairs the container holds in the reversed order get the conjugate."""
    polnum = np.where(uvdata.polarization_array == polstr2num(polarization, x_orientation=uvdata.x_orientation))[0][0]
    rows, conj = _baseline_rows(uvdata, prob, ants_map, time)
    out = vis3(uvdata.data_array)
    m_r, m_i = np.asarray(m_r), np.asarray(m_i)
    sign = np.where(conj, -1.0, 1.0)

    def chunk(lo, hi):
        out[rows[lo:hi], :, polnum] = (m_r[lo:hi] + 1j * sign[lo:hi, None] * m_i[lo:hi]) * scale_factor

    utils.for_row_chunks(chunk, len(rows))


def calibrate_and_model_dpss(
    uvdata,
    horizon=1.0,
    min_dly=0.0,
    offset=0.0,
    include_autos=False,
    verbose=False,
    red_tol=1.0,
    notebook_progressbar=False,
    fg_model_comps_dict=None,
    fix_degeneracies=False,
    degeneracy_iters=6,
    degeneracy_phase_ref=True,
    delay_redundant_spectrum=False,
    delay_redundant_times=2,
    delay_redundant_taper="none",
    delay_redundant_weighting="weights",
    delay_fringe_spectrum=False,
    delay_fringe_times=8,
    delay_fringe_taper="bh4",
    delay_cross_spectrum=False,
    delay_transfer=False,
    delay_transfer_ridge=1e-6,
    delay_spectrum=False,
    delay_spectrum_taper="bh4",
    delay_spectrum_max_dly=None,
    delay_spectrum_bllen_bin=1.0,
    delay_spectrum_calibrated=False,
    **fitting_kwargs,
):
    """Simultaneously solve for gains and model foregrounds with per-baseline DPSS vectors -- the kept entry point,
    calibration.py:1503-1584.  ``fg_model_comps_dict`` is accepted and ignored, as in the reference (:1564).  The ``delay_spectrum``
    and ``fix_degeneracies`` / ``degeneracy_*`` keywords are ``calibrate_and_model_tensor``'s, and so are ``fit_errors`` and
    ``gain_basis_errors`` among ``fitting_kwargs``."""
    _check_delay_spectrum(delay_spectrum, delay_spectrum_taper, delay_spectrum_max_dly, delay_spectrum_bllen_bin)
    _check_delay_transfer(delay_transfer, delay_transfer_ridge, delay_spectrum, fitting_kwargs.get("freeze_model", False))
    _check_delay_cross(delay_cross_spectrum, delay_spectrum, fitting_kwargs.get("batch_slices"), fitting_kwargs.get("init_guesses_from_previous_time_step", False))
    _check_delay_fringe(delay_fringe_spectrum, delay_fringe_times, delay_fringe_taper, delay_spectrum, fitting_kwargs.get("batch_slices"),
                        fitting_kwargs.get("init_guesses_from_previous_time_step", False))
    _check_delay_redundant(delay_redundant_spectrum, delay_redundant_times, delay_redundant_taper, delay_redundant_weighting, delay_spectrum,
                           delay_spectrum_calibrated, fitting_kwargs.get("batch_slices"), fitting_kwargs.get("init_guesses_from_previous_time_step", False),
                           fitting_kwargs.get("device_split"))
    _check_degeneracy_call(fix_degeneracies, degeneracy_iters, fitting_kwargs)
    waker = _wake_device(fitting_kwargs.get("devices"))
    try:
        dpss_model_comps_dict = modeling.yield_pbl_dpss_model_comps(
            uvdata, horizon=horizon, min_dly=min_dly, offset=offset, include_autos=include_autos, red_tol=red_tol,
            notebook_progressbar=notebook_progressbar, verbose=verbose,
        )
        (model, resid, gains, fitted_info) = calibrate_and_model_tensor(
            uvdata=uvdata, fg_model_comps_dict=dpss_model_comps_dict, include_autos=include_autos, verbose=verbose,
            notebook_progressbar=notebook_progressbar, delay_spectrum=delay_spectrum, delay_spectrum_taper=delay_spectrum_taper,
            delay_spectrum_max_dly=delay_spectrum_max_dly, delay_spectrum_bllen_bin=delay_spectrum_bllen_bin,
            delay_spectrum_calibrated=delay_spectrum_calibrated, delay_transfer=delay_transfer, delay_transfer_ridge=delay_transfer_ridge, delay_cross_spectrum=delay_cross_spectrum,
            delay_fringe_spectrum=delay_fringe_spectrum, delay_fringe_times=delay_fringe_times, delay_fringe_taper=delay_fringe_taper, delay_redundant_spectrum=delay_redundant_spectrum,
            delay_redundant_times=delay_redundant_times, delay_redundant_taper=delay_redundant_taper, delay_redundant_weighting=delay_redundant_weighting,
            fix_degeneracies=fix_degeneracies, degeneracy_iters=degeneracy_iters,
            degeneracy_phase_ref=degeneracy_phase_ref, **fitting_kwargs,
        )
    finally:
        waker.join()
    return model, resid, gains, fitted_info


def _modeling_comps_device(use_device, devices):
    """The ``device`` of ``modeling.yield_mixed_comps`` for ``use_tensorflow_to_derive_modeling_comps``: None (the host) when the flag is
    off; else the first entry of ``devices`` when there is one, else 0."""
    if not use_device:
        return None
    if devices is None or isinstance(devices, str):  # ("all": every visible GPU, the first of which is 0)
        return 0
    if isinstance(devices, (int, np.integer)):
        return int(devices)
    return int(devices[0]) if len(devices) else 0


def calibrate_and_model_mixed(
    uvdata,
    horizon=1.0,
    min_dly=0.0,
    offset=0.0,
    ant_dly=0.0,
    include_autos=False,
    verbose=False,
    red_tol=1.0,
    red_tol_freq=0.5,
    n_angle_bins=200,
    notebook_progressbar=False,
    use_redundancy=False,
    use_tensorflow_to_derive_modeling_comps=False,
    eigenval_cutoff=1e-10,
    dtype_matinv=np.float64,
    require_exact_angle_match=True,
    angle_match_tol=1e-3,
    grp_size_threshold=5,
    model_comps_dict=None,
    save_dict_to=None,
    fix_degeneracies=False,
    degeneracy_iters=6,
    degeneracy_phase_ref=True,
    delay_redundant_spectrum=False,
    delay_redundant_times=2,
    delay_redundant_taper="none",
    delay_redundant_weighting="weights",
    delay_fringe_spectrum=False,
    delay_fringe_times=8,
    delay_fringe_taper="bh4",
    delay_cross_spectrum=False,
    delay_transfer=False,
    delay_transfer_ridge=1e-6,
    delay_spectrum=False,
    delay_spectrum_taper="bh4",
    delay_spectrum_max_dly=None,
    delay_spectrum_bllen_bin=1.0,
    delay_spectrum_calibrated=False,
    **fitting_kwargs,
):
    """Gains + foregrounds with DPSS vectors for baselines without frequency redundancy and joint covariance
    eigenvectors for groups of baselines whose uv tracks overlap -- calibration.py:1353-1500 (same signature and
    returns).  ``use_tensorflow_to_derive_modeling_comps=True`` derives the joint groups' modeling vectors on the GPU
    (``modeling.yield_mixed_comps(device=...)``: the first entry of ``devices`` when one is given, else device 0); the default derives
    them on the host.  The ``delay_spectrum`` and ``fix_degeneracies`` / ``degeneracy_*`` keywords are ``calibrate_and_model_tensor``'s,
    and so are ``fit_errors`` and ``gain_basis_errors`` among ``fitting_kwargs``."""
    _check_delay_spectrum(delay_spectrum, delay_spectrum_taper, delay_spectrum_max_dly, delay_spectrum_bllen_bin)
    _check_delay_transfer(delay_transfer, delay_transfer_ridge, delay_spectrum, fitting_kwargs.get("freeze_model", False))
    _check_delay_cross(delay_cross_spectrum, delay_spectrum, fitting_kwargs.get("batch_slices"), fitting_kwargs.get("init_guesses_from_previous_time_step", False))
    _check_delay_fringe(delay_fringe_spectrum, delay_fringe_times, delay_fringe_taper, delay_spectrum, fitting_kwargs.get("batch_slices"),
                        fitting_kwargs.get("init_guesses_from_previous_time_step", False))
    _check_delay_redundant(delay_redundant_spectrum, delay_redundant_times, delay_redundant_taper, delay_redundant_weighting, delay_spectrum,
                           delay_spectrum_calibrated, fitting_kwargs.get("batch_slices"), fitting_kwargs.get("init_guesses_from_previous_time_step", False),
                           fitting_kwargs.get("device_split"))
    _check_degeneracy_call(fix_degeneracies, degeneracy_iters, fitting_kwargs)
    fitting_grps, blvecs, _, _ = modeling.get_uv_overlapping_grps_conjugated(
        uvdata, red_tol=red_tol, include_autos=include_autos, red_tol_freq=red_tol_freq, n_angle_bins=n_angle_bins,
        notebook_progressbar=notebook_progressbar, require_exact_angle_match=require_exact_angle_match,
        angle_match_tol=angle_match_tol,
    )
    if model_comps_dict is None:
        waker = _wake_device(fitting_kwargs.get("devices"))
        try:
            freqs = uvdata.freq_array[0] if np.ndim(uvdata.freq_array) == 2 else uvdata.freq_array
            model_comps_dict = modeling.yield_mixed_comps(
                fitting_grps, blvecs, freqs, eigenval_cutoff=eigenval_cutoff, ant_dly=ant_dly, horizon=horizon, offset=offset,
                min_dly=min_dly, verbose=verbose, dtype=dtype_matinv, notebook_progressbar=notebook_progressbar,
                grp_size_threshold=grp_size_threshold, device=_modeling_comps_device(use_tensorflow_to_derive_modeling_comps, fitting_kwargs.get("devices")),
            )
        finally:
            waker.join()
    if save_dict_to is not None:
        np.save(save_dict_to, model_comps_dict)
    (model, resid, gains, fitted_info) = calibrate_and_model_tensor(
        uvdata=uvdata, fg_model_comps_dict=model_comps_dict, include_autos=include_autos, verbose=verbose,
        notebook_progressbar=notebook_progressbar, use_redundancy=use_redundancy, delay_spectrum=delay_spectrum, delay_spectrum_taper=delay_spectrum_taper,
        delay_spectrum_max_dly=delay_spectrum_max_dly, delay_spectrum_bllen_bin=delay_spectrum_bllen_bin,
        delay_spectrum_calibrated=delay_spectrum_calibrated, delay_transfer=delay_transfer, delay_transfer_ridge=delay_transfer_ridge, delay_cross_spectrum=delay_cross_spectrum,
            delay_fringe_spectrum=delay_fringe_spectrum, delay_fringe_times=delay_fringe_times, delay_fringe_taper=delay_fringe_taper, delay_redundant_spectrum=delay_redundant_spectrum,
            delay_redundant_times=delay_redundant_times, delay_redundant_taper=delay_redundant_taper, delay_redundant_weighting=delay_redundant_weighting,
            fix_degeneracies=fix_degeneracies, degeneracy_iters=degeneracy_iters,
        degeneracy_phase_ref=degeneracy_phase_ref, **fitting_kwargs,
    )
    return model, resid, gains, fitted_info


# ------------------------------------------------------------------------------------------------------------------
# weights from autocorrelations, file / command-line driver: calibration.py:916-960, :1659-1942
# ------------------------------------------------------------------------------------------------------------------
def get_auto_weights(uvdata, delay_extent=25.0):
    """Inverse-variance weights from DPSS-smoothed autocorrelations -- calibration.py:916-960.

    Every autocorrelation spectrum is fitted (least squares on its unflagged channels) with the DPSS modes of a
    zero-length baseline widened by ``delay_extent`` ns; the weight of baseline (i, j) is ``1 / (auto_i auto_j)`` on its
    unflagged samples.  Returns a UVFlag-like object in flag mode whose ``weights_array`` holds the weights.
    """
    freqs = uvdata.freq_array[0] if np.ndim(uvdata.freq_array) == 2 else uvdata.freq_array
    dpss_components = modeling.yield_dpss_model_comps_bl_grp(0.0, freqs, offset=delay_extent)
    if type(uvdata).__module__.startswith("pyuvdata"):
        from pyuvdata import UVFlag

        data_weights = UVFlag(uvdata, mode="flag")
    else:
        from .uvcompat import SimpleUVFlag

        data_weights = SimpleUVFlag(uvdata, mode="flag")
    data_weights.weights_array = np.zeros(uvdata.data_array.shape)
    auto_fit = {}
    bls = uvdata.get_antpairpols()
    for bl in bls:
        if bl[0] == bl[1]:
            rows = []
            for ds, fs in zip(np.atleast_2d(uvdata.get_data(bl)), ~np.atleast_2d(uvdata.get_flags(bl))):
                coeffs = np.linalg.lstsq(dpss_components[fs], ds[fs].real, rcond=None)[0]
                rows.append(dpss_components @ coeffs)
            auto_fit[bl] = np.atleast_2d(np.asarray(rows))
    for bl in bls:
        smooth_weights = 1.0 / (auto_fit[bl[0], bl[0], bl[-1]] * auto_fit[bl[1], bl[1], bl[-1]])
        smooth_weights = smooth_weights * ~np.atleast_2d(uvdata.get_flags(bl))
        dinds = data_weights.antpair2ind(*bl[:2])
        polnum = np.where(data_weights.polarization_array == polstr2num(bl[-1], x_orientation=data_weights.x_orientation))[0][0]
        vis3(data_weights.weights_array)[dinds, :, polnum] = smooth_weights
    return data_weights


def _read_uvdata(files):
    from .uvcompat import read_container

    if is_uvdata(files):
        return files
    files = [files] if isinstance(files, str) else list(files)
    try:
        from pyuvdata import UVData
    except ImportError:  # uvh5 files (or archives of this package) read natively; several files are concatenated
        uvd = read_container(files[0])
        for fn in files[1:]:
            more = read_container(fn)
            rows = set(zip(uvd.ant_1_array.tolist(), uvd.ant_2_array.tolist(), uvd.time_array.tolist()))
            if not rows.isdisjoint(zip(more.ant_1_array.tolist(), more.ant_2_array.tolist(), more.time_array.tolist())):
                raise ValueError(f"{fn} holds (baseline, time) rows that an earlier input file already holds")
            uvd = uvd + more
        return uvd
    uvd = UVData()
    uvd.read(files)
    return uvd


def _read_uvcal(files):
    from .uvcompat import read_container

    if is_uvcal(files):
        return files
    files = [files] if isinstance(files, str) else list(files)
    try:
        from pyuvdata import UVCal
    except ImportError:  # calfits files (or archives of this package) read natively; several files are concatenated in time
        from .calfits import concat_times

        objs = [read_container(fn) for fn in files]
        for fn, obj in zip(files, objs):
            if not is_uvcal(obj):
                raise ValueError(f"{fn} holds visibilities, not gains")
        return concat_times(objs, files)
    uvc = UVCal()
    uvc.read_calfits(files)
    return uvc


def read_calibrate_and_model_dpss(
    input_data_files,
    input_model_files=None,
    input_gain_files=None,
    resid_outfilename=None,
    gain_outfilename=None,
    model_outfilename=None,
    fitted_info_outfilename=None,
    x_orientation="east",
    clobber=False,
    bllen_min=0.0,
    bllen_max=np.inf,
    bl_ew_min=0.0,
    ex_ants=None,
    select_ants=None,
    gpu_index=None,
    gpu_memory_limit=None,
    precision=32,
    use_autocorrs_in_weights=False,
    fit_errors=False,
    fit_errors_samples=False,
    fit_errors_ridge=1e-6,
    gain_basis_errors=False,
    fix_degeneracies=False,
    degeneracy_iters=6,
    degeneracy_phase_ref=True,
    delay_redundant_spectrum=False,
    delay_redundant_times=2,
    delay_redundant_taper="none",
    delay_redundant_weighting="weights",
    delay_fringe_spectrum=False,
    delay_fringe_times=8,
    delay_fringe_taper="bh4",
    delay_cross_spectrum=False,
    delay_transfer=False,
    delay_transfer_ridge=1e-6,
    delay_spectrum=False,
    delay_spectrum_taper="bh4",
    delay_spectrum_max_dly=None,
    delay_spectrum_bllen_bin=1.0,
    delay_spectrum_calibrated=False,
    delay_spectrum_outfile=None,
    **calibration_kwargs,
):
    """File driver of the DPSS fit -- calibration.py:1659-1817 (same arguments, returns and output files).

    Inputs are paths or the objects themselves.  Paths are read with pyuvdata when it is installed; without it, uvh5
    data files (one or several, concatenated) are read by this package's own uvh5 reader (``uvh5.py``, the HDF5 subset
    pyuvdata writes) and gain files (one or several, concatenated in time) by its calfits reader (``calfits.py``, the
    FITS subset of ``fits.py``).  Visibility outputs are written as uvh5 files and gain outputs as calfits files, which
    pyuvdata, HDF5 tools and FITS readers open.  ``gpu_index`` picks the MI355X the solvers are created on (default: device 0, all of them are
    visible); ``gpu_memory_limit`` [GiB] makes a fit that needs more device memory raise ``MemoryError`` instead of
    configuring an allocator pool.  As in the reference the baseline cuts are applied to the data only (:1767-1783
    select on ``uvd`` twice and never on the model) and ``fitted_info_outfilename`` is accepted but nothing is written --
    unless ``fit_errors`` (``fit_errors_samples``: with ``model_std``; ``fit_errors_ridge``: see ``calibrate_and_model_tensor``) is on:
    then ``gain_std`` (where the gains are free per channel, or with ``gain_basis_errors``, ``calibrate_and_model_tensor``'s, a Python
    keyword only) and the per-baseline tables go there as an ``.npz`` archive: ``antpairs``
    ``[rows, 2]`` and, ``[Npols, Ntimes, rows]`` each with ``nan`` for a skipped slice, ``leverage_per_baseline``,
    ``chisq_red_per_baseline``; ``noise_scale`` ``[Npols, Ntimes]``.
    The ``delay_spectrum`` keywords are ``calibrate_and_model_tensor``'s (Python keywords only: there is no command-line flag yet);
    ``delay_spectrum_outfile`` writes the entries as one ``.npz`` archive (``delay_spectrum_tables``): ``delays_ns``, ``bllen_m`` and,
    ``[Npols, Ntimes, nbins, Ndelays]`` each with ``nan`` for a skipped slice, ``data``, ``model``, ``resid``; ``nbls``
    ``[Npols, Ntimes, nbins]``; with ``"baselines"`` also ``antpairs`` ``[rows, 2]`` and ``data_bl``, ``model_bl``, ``resid_bl``
    ``[Npols, Ntimes, rows, Ndelays]``.
    ``delay_transfer`` / ``delay_transfer_ridge`` are ``calibrate_and_model_tensor``'s (Python keywords only); the archive then also holds
    ``transfer`` ``[Npols, Ntimes, nbins, Ndelays]``, ``transfer_nsingular`` ``[Npols, Ntimes]`` (-1 for a skipped slice) and, with
    ``"baselines"``, ``transfer_bl`` ``[Npols, Ntimes, rows, Ndelays]``.
    ``delay_cross_spectrum`` is ``calibrate_and_model_tensor``'s (a Python keyword only); the archive then also holds ``cross_partner``
    ``[Npols, Ntimes]`` (the partner's time index; -1 for a slice without one), ``cross_nbls`` ``[Npols, Ntimes, nbins]``, ``cross_data``,
    ``cross_model``, ``cross_resid`` and ``cross_noise_data``, ``cross_noise_model``, ``cross_noise_resid`` ``[Npols, Ntimes, nbins, Ndelays]``
    (``nan`` for a slice without a partner) and, with ``"baselines"``, ``cross_antpairs`` and the same six with ``_bl`` ``[Npols, Ntimes, rows, Ndelays]``.
    ``delay_fringe_spectrum``, ``delay_fringe_times``, ``delay_fringe_taper`` are ``calibrate_and_model_tensor``'s (Python keywords only);
    the archive then also holds ``fringe_rates`` ``[Nrates]`` (Hz), ``fringe_window`` ``[Npols, Ntimes, delay_fringe_times]`` (the time
    indices of the slice's window; -1 for a slice outside every window), ``fringe_nbls`` ``[Npols, Ntimes, nbins]``, ``fringe_data``,
    ``fringe_model``, ``fringe_resid`` ``[Npols, Ntimes, nbins, Nrates, Ndelays]`` (``nan`` for a slice outside every window) and, with
    ``"baselines"``, ``fringe_antpairs`` and the same three with ``_bl`` ``[Npols, Ntimes, rows, Nrates, Ndelays]``.
    ``delay_redundant_spectrum``, ``delay_redundant_times``, ``delay_redundant_taper``, ``delay_redundant_weighting`` are
    ``calibrate_and_model_tensor``'s (Python keywords only); the archive then also holds ``redundant_rates`` ``[Nrates]`` (Hz),
    ``redundant_bllen_m``, ``redundant_nmembers`` ``[ngroups]``, ``redundant_window`` ``[Npols, Ntimes, delay_redundant_times]`` (-1 for a
    slice outside every window), ``redundant_ngroups`` ``[Npols, Ntimes, nbins]``, ``redundant_data``, ``redundant_model``,
    ``redundant_resid`` ``[Npols, Ntimes, nbins, Nrates, Ndelays]`` (``nan`` outside every window) and, with ``"groups"``,
    ``redundant_antpairs`` (every group's first pair) and the same three with ``_grp`` ``[Npols, Ntimes, ngroups, Nrates, Ndelays]``.
    ``fix_degeneracies``, ``degeneracy_iters``, ``degeneracy_phase_ref`` are ``calibrate_and_model_tensor``'s too (Python keywords only);
    the sky model is ``input_model_files`` and the written gains and model are the fixed ones.
    """
    _check_delay_spectrum(delay_spectrum, delay_spectrum_taper, delay_spectrum_max_dly, delay_spectrum_bllen_bin)
    _check_delay_transfer(delay_transfer, delay_transfer_ridge, delay_spectrum, calibration_kwargs.get("freeze_model", False))
    _check_delay_cross(delay_cross_spectrum, delay_spectrum, calibration_kwargs.get("batch_slices"), calibration_kwargs.get("init_guesses_from_previous_time_step", False))
    _check_delay_fringe(delay_fringe_spectrum, delay_fringe_times, delay_fringe_taper, delay_spectrum, calibration_kwargs.get("batch_slices"),
                        calibration_kwargs.get("init_guesses_from_previous_time_step", False))
    _check_delay_redundant(delay_redundant_spectrum, delay_redundant_times, delay_redundant_taper, delay_redundant_weighting, delay_spectrum,
                           delay_spectrum_calibrated, calibration_kwargs.get("batch_slices"), calibration_kwargs.get("init_guesses_from_previous_time_step", False),
                           calibration_kwargs.get("device_split"))
    _check_degeneracy_call(fix_degeneracies, degeneracy_iters, dict(calibration_kwargs, sky_model=input_model_files))
    if delay_spectrum_outfile is not None and not delay_spectrum:
        raise ValueError("delay_spectrum_outfile needs delay_spectrum=True or 'baselines'")
    uvd = _read_uvdata(input_data_files)
    weights = get_auto_weights(uvd) if use_autocorrs_in_weights else None
    utils.select_baselines(uvd, bllen_min=bllen_min, bllen_max=bllen_max, bl_ew_min=bl_ew_min, ex_ants=ex_ants, select_ants=select_ants)
    uvd_model = _read_uvdata(input_model_files) if input_model_files is not None else None
    if uvd_model is not None:
        utils.select_baselines(uvd, bllen_min=bllen_min, bllen_max=bllen_max, bl_ew_min=bl_ew_min)
    uvc = _read_uvcal(input_gain_files) if input_gain_files is not None else None
    dtype = {32: np.float32, 64: np.float64}[precision]
    saved = dict(_DEVICE)
    _DEVICE["index"] = gpu_index
    _DEVICE["memory_limit_gib"] = gpu_memory_limit
    try:
        model_fit, resid_fit, gains_fit, fit_info = calibrate_and_model_dpss(
            uvdata=uvd, sky_model=uvd_model, gains=uvc, dtype=dtype, weights=weights, **calibration_kwargs,
            **(dict(fit_errors="samples" if fit_errors_samples else True, fit_errors_ridge=fit_errors_ridge) if fit_errors or fit_errors_samples else {}),
            **(dict(delay_spectrum=delay_spectrum, delay_spectrum_taper=delay_spectrum_taper, delay_spectrum_max_dly=delay_spectrum_max_dly,
                    delay_spectrum_bllen_bin=delay_spectrum_bllen_bin, delay_spectrum_calibrated=delay_spectrum_calibrated) if delay_spectrum else {}),
            **(dict(delay_transfer=True, delay_transfer_ridge=delay_transfer_ridge) if delay_transfer else {}),
            **(dict(delay_cross_spectrum=delay_cross_spectrum) if delay_cross_spectrum else {}),
            **(dict(delay_fringe_spectrum=delay_fringe_spectrum, delay_fringe_times=delay_fringe_times, delay_fringe_taper=delay_fringe_taper)
               if delay_fringe_spectrum else {}),
            **(dict(delay_redundant_spectrum=delay_redundant_spectrum, delay_redundant_times=delay_redundant_times, delay_redundant_taper=delay_redundant_taper,
                    delay_redundant_weighting=delay_redundant_weighting) if delay_redundant_spectrum else {}),
            **(dict(fix_degeneracies=fix_degeneracies, degeneracy_iters=degeneracy_iters, degeneracy_phase_ref=degeneracy_phase_ref)
               if fix_degeneracies else {}),
            **(dict(gain_basis_errors=True) if gain_basis_errors else {}),
        )
    finally:
        _DEVICE.update(saved)
    if resid_outfilename is not None:
        resid_fit.write_uvh5(resid_outfilename, clobber=clobber)
    if gain_outfilename is not None:
        gains_fit.x_orientation = x_orientation
        gains_fit.write_calfits(gain_outfilename, clobber=clobber)
    if model_outfilename is not None:
        model_fit.write_uvh5(model_outfilename, clobber=clobber)
    if (fit_errors or fit_errors_samples) and fitted_info_outfilename is not None:
        _write_fit_errors(fitted_info_outfilename, fit_info, clobber)
    if delay_spectrum_outfile is not None:
        if os.path.exists(delay_spectrum_outfile) and not clobber:
            raise IOError(f"{delay_spectrum_outfile} exists; use clobber=True to overwrite")
        with open(delay_spectrum_outfile, "wb") as f:  # (a file object: np.savez appends no suffix to the name the caller gave)
            np.savez(f, **delay_spectrum_tables(fit_info))
    fit_info["calibration_kwargs"] = calibration_kwargs
    fit_info["calibration_kwargs"]["dtype"] = dtype
    return model_fit, resid_fit, gains_fit, fit_info


def fit_errors_tables(fit_info):
    """The arrays the file driver writes from a ``fit_history`` with ``errors`` entries (``read_calibrate_and_model_dpss``)."""
    pols = sorted(k for k in fit_info if isinstance(k, int))
    ntimes = 1 + max([t for p in pols for t in fit_info[p]], default=-1)
    entries = [h["errors"] for p in pols for h in fit_info[p].values() if "errors" in h]
    out = {"noise_scale": np.full((len(pols), ntimes), np.nan)}
    pairs = next((list(h["leverage_per_baseline"]) for h in entries if "leverage_per_baseline" in h), None)
    if pairs is not None:
        out["antpairs"] = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        for k in ("leverage_per_baseline", "chisq_red_per_baseline"):
            out[k] = np.full((len(pols), ntimes, len(pairs)), np.nan)
    for i, p in enumerate(pols):
        for t, h in fit_info[p].items():
            if "errors" not in h:
                continue
            out["noise_scale"][i, t] = h["errors"]["noise_scale"]
            for k in ("leverage_per_baseline", "chisq_red_per_baseline"):
                if k in h["errors"]:
                    out[k][i, t] = [h["errors"][k][ap] for ap in pairs]
    if "gain_std" in fit_info:
        out["gain_std"] = np.asarray(fit_info["gain_std"])
    return out


def delay_spectrum_tables(fit_info):
    """The arrays the file driver writes from a ``fit_history`` with ``delay_spectrum`` entries (``read_calibrate_and_model_dpss``)."""
    pols = sorted(k for k in fit_info if isinstance(k, int))
    ntimes = 1 + max([t for p in pols for t in fit_info[p]], default=-1)
    entries = [h["delay_spectrum"] for p in pols for h in fit_info[p].values() if "delay_spectrum" in h]
    if not entries:
        return {}
    first = entries[0]
    nbins, nd = first["data"].shape
    out = {"delays_ns": np.asarray(first["delays_ns"]), "bllen_m": np.asarray(first["bllen_m"]), "nbls": np.zeros((len(pols), ntimes, nbins), dtype=np.int64)}
    for k in ("data", "model", "resid"):
        out[k] = np.full((len(pols), ntimes, nbins, nd), np.nan)
    pairs = list(first["per_baseline"]) if "per_baseline" in first else None
    if pairs is not None:
        out["antpairs"] = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        for k in ("data", "model", "resid"):
            out[k + "_bl"] = np.full((len(pols), ntimes, len(pairs), nd), np.nan)
    if "transfer" in first:
        out["transfer"] = np.full((len(pols), ntimes, nbins, nd), np.nan)
        out["transfer_nsingular"] = np.full((len(pols), ntimes), -1, dtype=np.int64)
        if "transfer_per_baseline" in first:
            out["transfer_bl"] = np.full((len(pols), ntimes, len(pairs), nd), np.nan)
    crossed = [e["cross"] for e in entries if "cross" in e]
    if crossed:  # (nan, -1 and 0 pairs for a slice without a partner)
        out["cross_partner"] = np.full((len(pols), ntimes), -1, dtype=np.int64)
        out["cross_nbls"] = np.zeros((len(pols), ntimes, nbins), dtype=np.int64)
        for k in ("data", "model", "resid"):
            out["cross_" + k] = np.full((len(pols), ntimes, nbins, nd), np.nan)
            out["cross_noise_" + k] = np.full((len(pols), ntimes, nbins, nd), np.nan)
        cpairs = list(crossed[0]["per_baseline"]) if "per_baseline" in crossed[0] else None
        if cpairs is not None:
            out["cross_antpairs"] = np.asarray(cpairs, dtype=np.int64).reshape(-1, 2)
            for k in ("data", "model", "resid"):
                out["cross_" + k + "_bl"] = np.full((len(pols), ntimes, len(cpairs), nd), np.nan)
                out["cross_noise_" + k + "_bl"] = np.full((len(pols), ntimes, len(cpairs), nd), np.nan)
    fringed = [e["fringe"] for e in entries if "fringe" in e]
    if fringed:  # (nan, -1 and 0 groups for a slice outside every window)
        nwin, nr = len(fringed[0]["time_indices"]), len(fringed[0]["fringe_rates"])
        out["fringe_rates"] = np.array(fringed[0]["fringe_rates"], dtype=np.float64)
        out["fringe_window"] = np.full((len(pols), ntimes, nwin), -1, dtype=np.int64)
        out["fringe_nbls"] = np.zeros((len(pols), ntimes, nbins), dtype=np.int64)
        for k in ("data", "model", "resid"):
            out["fringe_" + k] = np.full((len(pols), ntimes, nbins, nr, nd), np.nan)
        fpairs = list(fringed[0]["per_baseline"]) if "per_baseline" in fringed[0] else None
        if fpairs is not None:
            out["fringe_antpairs"] = np.asarray(fpairs, dtype=np.int64).reshape(-1, 2)
            for k in ("data", "model", "resid"):
                out["fringe_" + k + "_bl"] = np.full((len(pols), ntimes, len(fpairs), nr, nd), np.nan)
    averaged = [e["redundant"] for e in entries if "redundant" in e]
    if averaged:  # (nan, -1 and 0 groups for a slice outside every window)
        nwin, nr, nrb = len(averaged[0]["time_indices"]), len(averaged[0]["fringe_rates"]), len(averaged[0]["bllen_m"])
        out["redundant_rates"] = np.array(averaged[0]["fringe_rates"], dtype=np.float64)
        out["redundant_bllen_m"] = np.array(averaged[0]["bllen_m"], dtype=np.float64)
        out["redundant_nmembers"] = np.array(averaged[0]["nmembers"], dtype=np.int64)
        out["redundant_window"] = np.full((len(pols), ntimes, nwin), -1, dtype=np.int64)
        out["redundant_ngroups"] = np.zeros((len(pols), ntimes, nrb), dtype=np.int64)
        for k in ("data", "model", "resid"):
            out["redundant_" + k] = np.full((len(pols), ntimes, nrb, nr, nd), np.nan)
        rkeys = list(averaged[0]["groups"]) if "groups" in averaged[0] else None
        if rkeys is not None:
            out["redundant_antpairs"] = np.asarray(rkeys, dtype=np.int64).reshape(-1, 2)  # every group's first pair
            for k in ("data", "model", "resid"):
                out["redundant_" + k + "_grp"] = np.full((len(pols), ntimes, len(rkeys), nr, nd), np.nan)
    for i, p in enumerate(pols):
        for t, h in fit_info[p].items():
            if "delay_spectrum" not in h:
                continue
            e = h["delay_spectrum"]
            out["nbls"][i, t] = e["nbls"]
            if "redundant" in e:
                x = e["redundant"]
                out["redundant_window"][i, t], out["redundant_ngroups"][i, t] = x["time_indices"], x["ngroups"]
                for k in ("data", "model", "resid"):
                    out["redundant_" + k][i, t] = x[k]
                    if "groups" in x:
                        out["redundant_" + k + "_grp"][i, t] = [x["groups"][ap][k] for ap in rkeys]
            if "fringe" in e:
                x = e["fringe"]
                out["fringe_window"][i, t], out["fringe_nbls"][i, t] = x["time_indices"], x["nbls"]
                for k in ("data", "model", "resid"):
                    out["fringe_" + k][i, t] = x[k]
                    if "per_baseline" in x:
                        out["fringe_" + k + "_bl"][i, t] = [x["per_baseline"][ap][k] for ap in fpairs]
            if "cross" in e:
                x = e["cross"]
                out["cross_partner"][i, t], out["cross_nbls"][i, t] = x["partner_time_index"], x["nbls"]
                for k in ("data", "model", "resid"):
                    out["cross_" + k][i, t], out["cross_noise_" + k][i, t] = x[k], x["noise"][k]
                    if "per_baseline" in x:
                        out["cross_" + k + "_bl"][i, t] = [x["per_baseline"][ap][k] for ap in cpairs]
                        out["cross_noise_" + k + "_bl"][i, t] = [x["per_baseline"][ap]["noise"][k] for ap in cpairs]
            if "transfer" in e:
                out["transfer"][i, t], out["transfer_nsingular"][i, t] = e["transfer"], e["transfer_nsingular"]
                if "transfer_bl" in out:
                    out["transfer_bl"][i, t] = [e["transfer_per_baseline"][ap] for ap in pairs]
            for k in ("data", "model", "resid"):
                out[k][i, t] = e[k]
                if pairs is not None:
                    out[k + "_bl"][i, t] = [e["per_baseline"][ap][k] for ap in pairs]
    return out


def _write_fit_errors(filename, fit_info, clobber):
    if os.path.exists(filename) and not clobber:
        raise IOError(f"{filename} exists; use clobber=True to overwrite")
    with open(filename, "wb") as f:  # (a file object: np.savez appends no suffix to the name the caller gave)
        np.savez(f, **fit_errors_tables(fit_info))


def input_output_parser():
    """Input / output / selection / device arguments (names, types and defaults of calibration.py:1820-1858)."""
    ap = argparse.ArgumentParser()
    sp = ap.add_argument_group("Input and Output Arguments.")
    sp.add_argument("--input_data_files", type=str, nargs="+", required=True, help="visibility files to fit")
    sp.add_argument("--input_model_files", type=str, nargs="+", help="sky-model files that fix the overall amplitude and phase")
    sp.add_argument("--input_gain_files", type=str, nargs="+", help="gain files to start from")
    sp.add_argument("--resid_outfilename", type=str, default=None, help="where to write the residual visibilities")
    sp.add_argument("--model_outfilename", type=str, default=None, help="where to write the foreground model")
    sp.add_argument("--gain_outfilename", type=str, default=None, help="where to write the fitted gains")
    # (the reference's default is the STRING "False", which is truthy, so its CLI always overwrites, :1831; here the flag
    # means what it says)
    sp.add_argument("--clobber", action="store_true", default=False, help="replace existing output files")
    sp.add_argument("--x_orientation", default="east", type=str, help="x_orientation recorded in the output gains")
    sp.add_argument("--bllen_min", default=0.0, type=float, help="shortest baseline kept [m]")
    sp.add_argument("--bllen_max", default=np.inf, type=float, help="longest baseline kept [m]")
    sp.add_argument("--bl_ew_min", default=0.0, type=float, help="baselines need an east-west extent above this [m]")
    sp.add_argument("--ex_ants", default=None, type=int, nargs="+", help="antennas to leave out")
    sp.add_argument("--select_ants", default=None, type=int, nargs="+", help="use only these antennas")
    sp.add_argument("--gpu_index", default=None, type=int, help="which GPU of the node to run on")
    sp.add_argument("--gpu_memory_limit", default=None, type=int, help="refuse fits that need more device memory than this [GiB]")
    sp.add_argument("--precision", default=32, type=int, help="32 or 64 bit arithmetic")
    return ap


def fitting_argparser():
    """General fitting arguments (names, types and defaults of calibration.py:1861-1930)."""
    ap = input_output_parser()
    sp = ap.add_argument_group("General Fitting Arguments.")
    sp.add_argument("--tol", type=float, default=1e-14, help="stop when the loss changes by less than this between steps")
    sp.add_argument("--optimizer", type=str, default="Adamax", help="Adam or Adamax")
    sp.add_argument("--maxsteps", type=int, default=10000, help="upper bound on recorded descent steps")
    sp.add_argument("--verbose", default=False, action="store_true", help="print progress")
    sp.add_argument("--use_min", default=False, action="store_true", help="return the parameters of the lowest loss seen instead of the last ones")
    sp.add_argument("--use_redundancy", default=False, action="store_true", help="one set of foreground coefficients per redundant group")
    sp.add_argument("--correct_model", default=True, action="store_true", help="divide the fitted gains out of the model")
    sp.add_argument("--correct_resid", default=False, action="store_true", help="calibrate the residuals with the fitted gains")
    sp.add_argument("--graph_mode", default=False, action="store_true", help="accepted for compatibility; nothing is traced on this path")
    sp.add_argument("--init_guesses_from_previous_time_step", default=False, action="store_true", help="warm-start each time from the previous one")
    sp.add_argument("--learning_rate", type=float, default=1e-2, help="optimizer step size")
    sp.add_argument("--red_tol", type=float, default=1.0, help="baselines closer than this are redundant [m]")
    sp.add_argument("--skip_threshold", type=float, default=0.5, help="flag a (time, polarization) whose unflagged fraction is below this")
    sp.add_argument("--model_regularization", type=str, default="post_hoc", help="sum, post_hoc or None")
    sp.add_argument("--nsamples_in_weights", default=False, action="store_true", help="multiply the weights by nsamples")
    sp.add_argument("--use_model_snr_weights", default=False, action="store_true", help="weight samples by the model's signal to noise")
    sp.add_argument("--use_autocorrs_in_weights", default=False, action="store_true", help="inverse-variance weights from the autocorrelations")
    sp.add_argument("--gain_max_dly", type=float, default=None,
                    help="fit the gains in a DPSS basis that is smooth up to this delay [ns]; default: free per-channel gains")
    sp.add_argument("--gain_time_scale", type=float, default=None,
                    help="fit the times of a polarization jointly, with gains in a DPSS basis that drifts no faster than this [s]; "
                         "default: every time fits its own gains")
    sp.add_argument("--fit_quality", default=False, action="store_true",
                    help="write the weighted mean squared residual per antenna and channel into the gains' quality column and the total "
                         "over antennas into TOTQLTY; default: zeros")
    sp.add_argument("--fit_errors", default=False, action="store_true",
                    help="report the errors of the fit: a standard deviation per gain, the leverage and the reduced chi-square per baseline "
                         "(conditional errors: lower bounds); the file driver writes them to fitted_info_outfilename as an .npz archive; default: off")
    sp.add_argument("--fit_errors_samples", default=False, action="store_true",
                    help="--fit_errors plus the standard deviation of the fitted model at every sample (as large as the data)")
    sp.add_argument("--fit_errors_ridge", type=float, default=1e-6,
                    help="ridge of the factorisation behind --fit_errors, as a fraction of the mean diagonal of a group's normal matrix; default 1e-6")
    for f in FitControls.keyword_fields():  # the closed-form, robust, Gauss-Newton and L-BFGS keywords: name, type and default of the field
        sp.add_argument("--" + f.name, type=f.type, default=f.default, help=KEYWORD_HELP[f.name])
    return ap


def dpss_fit_argparser():
    """DPSS-specific arguments on top of the general ones (calibration.py:1933-1942)."""
    ap = fitting_argparser()
    sp = ap.add_argument_group("DPSS Specific Fitting Arguments.")
    sp.add_argument("--horizon", default=1.0, type=float, help="fraction of the horizon delay covered by the basis")
    sp.add_argument("--min_dly", default=0.0, type=float, help="smallest delay half-width of a basis [ns]")
    sp.add_argument("--offset", default=0.0, type=float, help="delay added beyond the horizon [ns]")
    return ap
