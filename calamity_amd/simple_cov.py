"""Analytic multi-baseline foreground covariance and its leading eigenvectors (setup time).

Counterpart of /root/reference/calamity/simple_cov.py:7-189.  The covariance between sample (baseline a, channel i) and
(baseline b, channel j) is ``sinc(2 max(min_dly * dnu, horizon * |u_a(nu_i) - u_b(nu_j)| + offset * dnu)) *
sinc(2 ant_dly * dnu)`` with ``u = b nu / c`` in wavelengths and ``dnu = |nu_i - nu_j|`` in GHz (delays in ns); the
modeling vectors of a fitting group are the eigenvectors whose eigenvalue is at least ``eigenval_cutoff`` times the
largest, strongest first.

Two routes.  The host route (the default) is a dense symmetric eigenproblem of size (Nbls * Nfreqs).  The device route
(``device=`` an index, or the reference's ``use_tensorflow=True``, which means device 0) is the low-rank one of
csrc/mixed_comps_kernels.hpp: a pivoted Cholesky factor ``L`` of the covariance, the eigenpairs of the small ``L^T L`` from
the host's LAPACK, ``V = L U lambda^-1/2``, and ``||C - L L^T||_F`` as the certificate.  A group whose certificate fails
(the covariance is indefinite for ``offset`` or ``min_dly`` != 0 with several baselines) or whose factor hit its rank cap is
computed by the host route instead: the device route never raises for such a group and never returns uncertified vectors.
"""
import concurrent.futures
import ctypes as C
import time

import numpy as np

from .utils import echo, usable_cores


def device_index(device, use_tensorflow=False):
    """The device of the device route, or None for the host route: ``device`` when given (an int >= 0), else 0 with the
    reference's ``use_tensorflow=True``."""
    if device is None:
        return 0 if use_tensorflow else None
    if isinstance(device, (bool, np.bool_)) or not isinstance(device, (int, np.integer)) or int(device) < 0:
        raise ValueError(f"device must be None or a device index >= 0, got {device!r}")
    return int(device)


def factor_tol(eigenval_cutoff):
    """Where the pivoted Cholesky stops: the largest remaining diagonal below ``max(1e-13, 1e-3 eigenval_cutoff)`` (1e-13 is the
    rounding of the running diagonal)."""
    return max(1e-13, 1e-3 * float(eigenval_cutoff))


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _bands(freqs, ngroups):
    """``(bands, shared)``: the band of each of ``ngroups`` groups, from one band for all of them (``shared``) or a list with a 1-D
    band per group."""
    if isinstance(freqs, (list, tuple)) and len(freqs) and np.ndim(freqs[0]) == 1:
        if len(freqs) != ngroups:
            raise ValueError(f"{len(freqs)} bands for {ngroups} groups")
        return [_f64(f) for f in freqs], False
    return [_f64(freqs).ravel()] * ngroups, True


def simple_cov_matrix(blvecs, freqs, ant_dly=0.0, horizon=1.0, offset=0.0, min_dly=0.0, dtype=np.float64, device=None, **_ignored):
    """(Nbls * Nfreqs) square covariance, baseline-major rows -- simple_cov.py:7-107.  ``device``: an index computes it on that
    device in double (cal_simple_cov_matrix) and casts to ``dtype``; None is the host."""
    if device_index(device) is not None:
        from . import _lib

        uvws, fr = _f64(np.asarray(blvecs, dtype=np.float64).reshape(-1, 3)), _f64(freqs).ravel()
        n = len(uvws) * len(fr)
        cmat = np.empty((n, n), dtype=np.float64)
        _lib.check(_lib.load().cal_simple_cov_matrix(device_index(device), len(uvws), uvws.ctypes.data, len(fr), fr.ctypes.data, float(ant_dly),
                                                     float(horizon), float(offset), float(min_dly), cmat.ctypes.data))
        return cmat.astype(dtype, copy=False)
    uvws = np.asarray(blvecs, dtype=dtype).reshape(-1, 3)
    freqs = np.asarray(freqs, dtype=dtype)
    # position of every (baseline, channel) sample in the uvw space, in wavelengths
    pts = (uvws[:, None, :] * (freqs[None, :, None] / 3e8)).reshape(-1, 3)
    sep = np.zeros((len(pts), len(pts)), dtype=dtype)
    for axis in range(3):
        sep += np.abs(pts[:, None, axis] - pts[None, :, axis]) ** 2.0
    sep = np.sqrt(sep) * horizon
    fvals = np.tile(freqs, len(uvws))
    dfg = np.abs(fvals[:, None] - fvals[None, :]) / 1e9
    sep += dfg * offset
    cmat = np.sinc(2 * np.maximum(min_dly * dfg, sep))
    cmat = cmat * np.sinc(2 * dfg * ant_dly)
    return cmat


def _host_model_comps(blvecs, freqs, ant_dly, horizon, offset, min_dly, dtype, eigenval_cutoff):
    cmat = simple_cov_matrix(blvecs, freqs, ant_dly=ant_dly, horizon=horizon, offset=offset, min_dly=min_dly, dtype=dtype)
    evals, evecs = np.linalg.eigh(cmat)
    keep = evals / evals[-1] >= eigenval_cutoff
    return evecs[:, keep][:, ::-1]


def keep_and_accept(evals, status, resid_fro, eigenval_cutoff):
    """What the device route decides from the ascending eigenvalues of ``L^T L``: the indices it keeps (``lambda / lambda_max >=
    eigenval_cutoff``, strongest first) and why the group goes to the host route (None: it does not) -- the group is accepted iff the
    factor finished below its tolerance (status 0) and ``resid_fro <= 0.1 eigenval_cutoff lambda_max``."""
    if status != 0:
        return np.zeros(0, dtype=np.int64), ("rank cap" if status == 1 else "not run")
    lam_max = evals[-1] if len(evals) else 0.0
    if not (lam_max > 0.0) or not (resid_fro <= 0.1 * eigenval_cutoff * lam_max):
        return np.zeros(0, dtype=np.int64), "certificate"
    return np.nonzero(evals / lam_max >= eigenval_cutoff)[0][::-1], None


def device_model_comps(blvecs_list, freqs, ant_dly=0.0, horizon=1.0, offset=0.0, min_dly=0.0, dtype=np.float64, eigenval_cutoff=1e-10,
                       device=0, scratch_bytes=0, return_factors=False):
    """The device route for several groups in one call: ``(vectors, infos, times)``.  ``freqs`` is the band of all groups, or a list
    with one band per group.  ``vectors[g]`` is ``(n_g, kept_g)`` in ``dtype``,
    or None where the group is not accepted; ``infos[g]`` holds route, reason, n, k, kept, resid_fro, lambda_max, max_d, the chunk the group was factored in and the kept
    eigenvalues ``evals`` (with ``return_factors`` also ``L`` [n, k], ``pivots`` and ``G``); ``times`` the seconds of the create call
    and, inside it, of factor, gram and certificate, of the host eigenproblems and of the back-multiplication call and its launch."""
    from . import _lib

    lib = _lib.load()
    uvws = [_f64(np.asarray(b, dtype=np.float64).reshape(-1, 3)) for b in blvecs_list]
    ng = len(uvws)
    starts = np.zeros(ng + 1, dtype=np.int32)
    starts[1:] = np.cumsum([len(u) for u in uvws])
    uvw = _f64(np.concatenate(uvws, axis=0))
    bands, shared = _bands(freqs, ng)
    nchan = [len(f) for f in bands]
    if shared:
        fr, fptr = bands[0], None
    else:
        fstarts = np.zeros(ng + 1, dtype=np.int32)
        fstarts[1:] = np.cumsum(nchan)
        fr, fptr = _f64(np.concatenate(bands)), fstarts.ctypes.data
    desc = _lib.MixedCompsDesc(ngroups=ng, nfreqs=len(fr), grp_bl_start=starts.ctypes.data, uvw=uvw.ctypes.data, freqs=fr.ctypes.data, grp_freq_start=fptr,
                               ant_dly=float(ant_dly), horizon=float(horizon), offset=float(offset), min_dly=float(min_dly),
                               tol=factor_tol(eigenval_cutoff), scratch_bytes=int(scratch_bytes or 0))
    handle = C.c_void_p()
    t0 = time.perf_counter()
    _lib.check(lib.cal_mixed_comps_create(C.byref(handle), int(device), C.byref(desc)))
    try:
        times = {"create": time.perf_counter() - t0}
        rank, status, chunk = np.zeros(ng, dtype=np.int32), np.zeros(ng, dtype=np.int32), np.zeros(ng, dtype=np.int32)
        max_d, resid, ms = np.zeros(ng), np.zeros(ng), np.zeros(3)
        _lib.check(lib.cal_mixed_comps_info(handle, rank.ctypes.data, status.ctypes.data, chunk.ctypes.data, max_d.ctypes.data, resid.ctypes.data,
                                            ms.ctypes.data))
        times.update(factor=ms[0] * 1e-3, gram=ms[1] * 1e-3, certificate=ms[2] * 1e-3)
        goff = np.concatenate([[0], np.cumsum(rank.astype(np.int64) ** 2)])
        gram = np.zeros(max(1, int(goff[-1])))
        _lib.check(lib.cal_mixed_comps_gram(handle, gram.ctypes.data, gram.size))
        grams = [gram[goff[g] : goff[g + 1]].reshape(rank[g], rank[g]) for g in range(ng)]
        t0 = time.perf_counter()
        todo = [g for g in range(ng) if status[g] == 0 and rank[g] > 0]
        with concurrent.futures.ThreadPoolExecutor(max_workers=max(1, min(len(todo), usable_cores()))) as pool:
            eig = dict(zip(todo, pool.map(lambda g: np.linalg.eigh(grams[g]), todo)))
        times["eigh"] = time.perf_counter() - t0
        infos, nkeep, us, scales = [], np.zeros(ng, dtype=np.int32), [], []
        for g in range(ng):
            evals, evecs = eig.get(g, (np.zeros(0), np.zeros((0, 0))))
            keep, reason = keep_and_accept(evals, int(status[g]), float(resid[g]), eigenval_cutoff)
            nkeep[g] = len(keep)
            us.append(_f64(evecs[:, keep]).ravel())
            scales.append(1.0 / np.sqrt(evals[keep]))
            infos.append(dict(route="host" if reason else "device", reason=reason, n=len(uvws[g]) * nchan[g], k=int(rank[g]), kept=len(keep),
                              resid_fro=float(resid[g]), lambda_max=float(evals[-1]) if len(evals) else 0.0, max_d=float(max_d[g]),
                              status=_lib.MIXED_COMPS_STATUS[status[g]], chunk=int(chunk[g]), evals=evals[keep]))
        f32 = np.dtype(dtype) == np.float32
        sizes = [infos[g]["n"] * int(nkeep[g]) for g in range(ng)]
        vall = np.zeros(max(1, sum(sizes)), dtype=np.float32 if f32 else np.float64)
        uall, sall = _f64(np.concatenate(us + [np.zeros(1)])), _f64(np.concatenate(scales + [np.zeros(1)]))
        launch = C.c_double(0.0)
        t0 = time.perf_counter()
        _lib.check(lib.cal_mixed_comps_vectors(handle, _lib.CAL_F32 if f32 else _lib.CAL_F64, nkeep.ctypes.data, uall.ctypes.data, sall.ctypes.data,
                                               vall.ctypes.data, C.byref(launch)))
        times.update(vectors=time.perf_counter() - t0, backmul=launch.value * 1e-3)
        voff = np.concatenate([[0], np.cumsum(sizes)])
        vectors = [vall[voff[g] : voff[g + 1]].reshape(infos[g]["n"], nkeep[g]).astype(dtype, copy=True) if infos[g]["reason"] is None else None
                   for g in range(ng)]
        if return_factors:
            for g in range(ng):
                fac, piv = np.zeros((rank[g], infos[g]["n"])), np.zeros(rank[g], dtype=np.int32)
                _lib.check(lib.cal_mixed_comps_factor(handle, g, fac.ctypes.data, piv.ctypes.data))
                infos[g].update(L=fac.T, pivots=piv, G=grams[g].copy())
    finally:
        _lib.check(lib.cal_mixed_comps_destroy(handle))
    return vectors, infos, times


def model_comps_of_groups(blvecs_list, freqs, ant_dly=0.0, horizon=1.0, offset=0.0, min_dly=0.0, dtype=np.float64, eigenval_cutoff=1e-10,
                          device=None, verbose=False, scratch_bytes=0):
    """``(vectors, infos)`` of several fitting groups: by the host route for ``device=None``; else all of them in one call of the
    device route, and the groups it does not accept by the host route (said through ``echo(verbose)`` and in the group's info)."""
    kw = dict(ant_dly=ant_dly, horizon=horizon, offset=offset, min_dly=min_dly, dtype=dtype, eigenval_cutoff=eigenval_cutoff)
    bands, _ = _bands(freqs, len(blvecs_list))
    if device is None:
        vectors = [_host_model_comps(b, bands[g], **kw) for g, b in enumerate(blvecs_list)]
        infos = [dict(route="host", reason="no device asked for", n=v.shape[0], k=0, kept=v.shape[1], resid_fro=0.0, lambda_max=0.0) for v in vectors]
        return vectors, infos
    vectors, infos, _ = device_model_comps(blvecs_list, freqs, device=device, scratch_bytes=scratch_bytes, **kw)
    for g, info in enumerate(infos):
        if vectors[g] is None:
            echo(f"mixed-model components: group {g} (n = {info['n']}, k = {info['k']}) goes to the host route: {info['reason']} "
                 f"(resid_fro = {info['resid_fro']:.3e}, lambda_max = {info['lambda_max']:.3e})", verbose=verbose)
            vectors[g] = _host_model_comps(blvecs_list[g], bands[g], **kw)
            info["kept"] = vectors[g].shape[1]
    return vectors, infos


def yield_simple_multi_baseline_model_comps(
    blvecs, freqs, ant_dly=0.0, horizon=1.0, offset=0.0, min_dly=0.0, dtype=np.float64, verbose=False, eigenval_cutoff=1e-10,
    device=None, use_tensorflow=False, return_info=False, **_ignored
):
    """(Nbls * Nfreqs, Ncomponents) eigenvectors above the cutoff, strongest first -- simple_cov.py:110-189.  ``device`` (an index;
    ``use_tensorflow=True`` means 0) takes the device route, see the module's docstring; ``return_info`` adds the group's info."""
    dev = device_index(device, use_tensorflow)
    if dev is None and not return_info:
        return _host_model_comps(blvecs, freqs, ant_dly, horizon, offset, min_dly, dtype, eigenval_cutoff)
    vectors, infos = model_comps_of_groups([blvecs], freqs, ant_dly=ant_dly, horizon=horizon, offset=offset, min_dly=min_dly, dtype=dtype,
                                           eigenval_cutoff=eigenval_cutoff, device=dev, verbose=verbose)
    return (vectors[0], infos[0]) if return_info else vectors[0]
