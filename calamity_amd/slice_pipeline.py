"""The stages around the fit of a (polarization, time) slice of ``calibration.calibrate_and_model_tensor``, stated once for the loop
over the times (one slice on a ``HipFitSolver``) and for the batches (``nt`` slices on a ``SliceBatchFitter``)::

    tensorize (per slice) -> gather -> start -> fit_loop.drive -> report -> write (per slice)

``cfg`` is the call's settings object (``calibrate_and_model_tensor`` builds it once); arrays of a batch are slice-major.  The two
fitters answer to the same method names, so no stage asks which one it holds; the caller chooses the fitter, calls ``drive`` and, in
the loop, hands the parameters of one time to the next (``start(handed=...)``)."""
import datetime

import numpy as np

from . import utils
from .fit_loop import history_entry
from .utils import echo
from .uvcompat import polstr2num, vis3

_BATCH_ARRAYS = ("d_r", "d_i", "w", "s_r", "s_i", "g_r", "g_i", "r_w")


def slice_stats(uvdata, bltsel, polnum):
    """(fraction of unflagged samples, rms of the unflagged visibilities) of one (polarization, time) -- calibration.py:1168-1182
    -- in one threaded pass over the slice's rows (the reference's boolean fancy indexing copies the slice twice)."""
    rows = np.where(bltsel)[0]
    vis, flg = vis3(np.asarray(uvdata.data_array)), vis3(np.asarray(uvdata.flag_array))
    cnt = np.zeros(len(rows), dtype=np.int64)
    ssq = np.zeros(len(rows), dtype=np.float64)

    def chunk(lo, hi):
        keep = ~np.take(flg[:, :, polnum], rows[lo:hi], axis=0)
        d = np.take(vis[:, :, polnum], rows[lo:hi], axis=0)
        p = d.real * d.real + d.imag * d.imag
        cnt[lo:hi] = np.count_nonzero(keep, axis=1)
        ssq[lo:hi] = np.sum(p * keep, axis=1)

    utils.for_row_chunks(chunk, len(rows))
    n = int(cnt.sum())
    frac = n / (uvdata.Nbls * uvdata.Nfreqs)
    return frac, (float(np.sqrt(ssq.sum() / n)) if n else float("nan"))


def prior_sums(sky_r, sky_i, wgts):
    """``P_r, P_i = sum w * sky`` (calibration.py:619-625), accumulated in float64 baseline by baseline on the host's cores; the
    total does not depend on how the rows are chunked."""
    nb = len(wgts)
    pr, pi = np.zeros(nb, dtype=np.float64), np.zeros(nb, dtype=np.float64)

    def chunk(lo, hi):
        w64 = wgts[lo:hi].astype(np.float64)
        pr[lo:hi] = np.sum(sky_r[lo:hi] * w64, axis=1)
        pi[lo:hi] = np.sum(sky_i[lo:hi] * w64, axis=1)

    utils.for_row_chunks(chunk, nb)
    return float(pr.sum()), float(pi.sum())


def gram_factors(prob):
    """Per fitting-group Gram matrices ``sum_bl A_bl^T A_bl`` that are not the identity (DPSS columns are orthonormal,
    so for per-baseline DPSS this is empty).  Keyed by (basis, row blocks)."""
    cache = prob.__dict__.setdefault("_gram", None)
    if cache is not None:
        return cache
    F = prob.nfreqs
    keys, out = {}, {}
    for g in range(prob.ngrps):
        rbs = tuple(prob.bl_rowblk[prob.grp_bl_start[g] : prob.grp_bl_start[g + 1]].tolist())
        keys.setdefault((int(prob.grp_basis[g]), rbs), []).append(g)
    for (u, rbs), grps in keys.items():
        blk = prob.basis[u]
        gram = sum(blk[rb * F : (rb + 1) * F].T @ blk[rb * F : (rb + 1) * F] for rb in rbs)
        if not np.allclose(gram, np.eye(gram.shape[0]), atol=1e-9):
            out[(u, rbs)] = (gram, np.asarray(grps))
    prob.__dict__["_gram"] = out
    return out


def gram_solve(prob, c_r, c_i, nt=1):
    """``A^T d`` -> least-squares coefficients for ``nt`` slices of flat coefficients: every fitting group whose Gram matrix is not
    the identity is solved with it, in float64 (copies); the others keep their bits.  Without such a group the inputs come back."""
    grams = gram_factors(prob)
    if not grams:
        return c_r, c_i
    c_r = np.asarray(c_r, dtype=np.float64).copy()
    c_i = np.asarray(c_i, dtype=np.float64).copy()
    for gram, grps in grams.values():
        for t in range(nt):
            idx = t * prob.ncoeffs + prob.grp_coff[grps][None, :] + np.arange(gram.shape[0])[:, None]
            c_r[idx] = np.linalg.solve(gram, c_r[idx])
            c_i[idx] = np.linalg.solve(gram, c_i[idx])
    return c_r, c_i


def init_coeffs(fitter, prob, src_r, src_i, nt=1):
    """tensorize_fg_coeffs (calibration.py:828-913) for both components of ``nt`` slices at once: ``A^T (src * [w != 0])`` on the GPU
    (``w``: the weights of ``set_data``), then the (rarely needed) small Gram solves on the host, which go back to the fitter.
    Returns flat (c_r, c_i)."""
    fitter.init_coeffs(src_r, src_i)
    _, _, c_r, c_i = fitter.get_params()
    if gram_factors(prob):
        c_r, c_i = gram_solve(prob, c_r, c_i, nt)
        fitter.set_params(c_r=c_r, c_i=c_i)
    return c_r, c_i


def configure(fitter, gain_basis, priors, optimizer, opt_kwargs, gain_time_basis=None):
    """What every fit sets between its parameters and ``drive``: the gain bases (the fitter is kept between calls: ``None`` detaches an
    earlier call's; ``g0`` = the gains just set), the ``"sum"`` regulariser with ``priors = (P_r, P_i)`` (numbers, or one per slice)
    or none, the optimizer."""
    fitter.set_gain_basis(gain_basis)
    if gain_time_basis is not None:
        fitter.set_gain_time_basis(gain_time_basis)
    if priors is None:
        fitter.set_regularization(None)
    else:
        fitter.set_regularization("sum", priors[0], priors[1])
    fitter.set_optimizer(optimizer, **opt_kwargs)


def tensorize(cfg, sl):
    """Stage 1, one slice ``sl`` (``polnum``, ``pol``, ``time_index``, ``time``): the skip test and rms scale (calibration.py:1168-1182);
    a skipped slice is flagged in the three containers and gives ``None``.  Otherwise ``sl`` with ``rms`` and the flat rows: data and
    weights, the sky model (the data rows themselves where the data stand in for it), the weights of ``fix_degeneracies`` (the sky
    model's own, where the data have any), the gains of the container, and the priors of the ``"sum"`` regulariser unless they wait
    for the model-SNR weights."""
    uvdata, pol, time = cfg.uvdata, sl["pol"], sl["time"]
    bltsel = np.isclose(uvdata.time_array, time, atol=1e-7, rtol=0.0)
    frac_unflagged, rms = slice_stats(uvdata, bltsel, sl["polnum"])
    if frac_unflagged < cfg.skip_threshold:
        echo(f"{datetime.datetime.now()}: Only {frac_unflagged * 100}-percent of data unflagged. Skipping...\n", verbose=cfg.verbose)
        for container in (cfg.resid, cfg.gains, cfg.model):
            cal.flag_poltime(container, time=time, polarization=pol)
        return None
    flat = dict(polarization=pol, time=time, data_scale_factor=rms, dtype=cfg.dtype)
    d_r, d_i, w = cal._tensorize_flat(uvdata, cfg.prob, cfg.ants_map, weights=cfg.weights, nsamples_in_weights=cfg.nsamples_in_weights, **flat)
    s_r, s_i, r_w = d_r, d_i, None  # (the data stand in for the sky model: the same rows)
    if cfg.sky_model is not uvdata:
        s_r, s_i, s_w = cal._tensorize_flat(cfg.sky_model, cfg.prob, cfg.ants_map, **flat,
                                            **({"weights": cfg.weights} if cfg.degen is not None else {"want_weights": False}))
        if cfg.degen is not None:
            r_w = s_w * (w > 0)
    g_r, g_i = cal.tensorize_gains(cfg.gains, dtype=cfg.dtype, time=time, polarization=pol)
    pri = prior_sums(s_r, s_i, w) if cfg.model_regularization == "sum" and not cfg.use_model_snr_weights else None
    return dict(sl, rms=rms, d_r=d_r, d_i=d_i, w=w, s_r=s_r, s_i=s_i, r_w=r_w, g_r=g_r, g_i=g_i, pri=pri)


def gather(parts):
    """The arrays of the tensorized slices ``parts`` as one slice-major batch (one slice: its own arrays, not copies)."""
    cat = lambda a: a[0] if len(a) == 1 else np.concatenate(a)  # noqa: E731
    arrs = {k: None if parts[0][k] is None else cat([p[k] for p in parts]) for k in _BATCH_ARRAYS}
    arrs["pri"] = None if parts[0]["pri"] is None else np.asarray([p["pri"] for p in parts])
    arrs["time_index"] = [p["time_index"] for p in parts]
    arrs["polnum"], arrs["rms"] = [p["polnum"] for p in parts], [p["rms"] for p in parts]
    return arrs


def start(fitter, nt, arrs, cfg, handed=None):
    """Stage 2: everything between the arrays of ``gather`` and ``drive``.  ``set_data``; the initial coefficients of every slice
    (calibration.py:1219-1233; ``init_coeffs``) and, with ``use_model_snr_weights``, the weights ``|model|^2 w`` renormalised slice by
    slice (:1235-1242), unless the slice is ``handed`` its parameters ``(g_r, g_i, c_r, c_i)`` (the previous time's, which then are
    the gains the fit starts from); ``set_params``, the gain bases, the priors and regulariser, the optimizer (``configure``)."""
    prob, nb = cfg.prob, cfg.prob.nbls
    d_r, d_i, s_r, s_i = arrs["d_r"], arrs["d_i"], arrs["s_r"], arrs["s_i"]
    fitter.set_data(d_r, d_i, arrs["w"])
    if handed is not None:
        arrs["g_r"], arrs["g_i"], c_r, c_i = handed
    else:
        c_r, c_i = init_coeffs(fitter, prob, s_r, s_i, nt)
        if cfg.use_model_snr_weights:
            m_r, m_i = fitter.model()
            w_new = (np.square(m_r.astype(np.float64)) + np.square(m_i.astype(np.float64))) * arrs["w"]
            for t in range(nt):
                w_new[t * nb : (t + 1) * nb] /= np.sum(w_new[t * nb : (t + 1) * nb])
            arrs["w"] = w_new.astype(cfg.dtype)
            fitter.set_data(d_r, d_i, arrs["w"])
    arrs["c_r"], arrs["c_i"] = c_r, c_i  # what the fit was handed: what a frozen model reports
    fitter.set_params(arrs["g_r"], arrs["g_i"], c_r, c_i)
    priors = time_basis = None
    if cfg.model_regularization == "sum":
        # priors of calibration.py:619-625, one pair per slice (with model-SNR weights: under the new weights)
        pri = arrs["pri"]
        if pri is None:
            pri = np.asarray([prior_sums(s_r[t * nb : (t + 1) * nb], s_i[t * nb : (t + 1) * nb], arrs["w"][t * nb : (t + 1) * nb]) for t in range(nt)])
        priors = (pri[:, 0], pri[:, 1])
    if cfg.gain_time_basis is not None:
        # a joint fit: the rows of the fitted times, no more vectors than times (the first columns: the smoothest sequences), and
        # one pair of sums for the one fit
        time_basis = cfg.gain_time_basis[arrs["time_index"]][:, :nt]
        priors = None if priors is None else (float(np.sum(priors[0])), float(np.sum(priors[1])))
    configure(fitter, cfg.gain_basis, priors, cfg.optimizer, cfg.opt_kwargs, gain_time_basis=time_basis)


def report(fitter, nt, arrs, cfg, result):
    """Stage 3, after ``drive``: the reported parameters (every slice's own minimum with ``use_min``, calibration.py:702-710; the
    coefficients the fit was handed with ``freeze_model``, :730-732), the model rows from one ``A c`` pass (:1271-1292), then what
    was asked for at those parameters, on the data and weights the fit used: quality, errors (with the ``chisq_bl`` of the quality
    pass), delay spectra, their transfer, the cross spectra of paired times, the delay / fringe-rate planes of whole windows and those of the redundant groups' averages -- and the degeneracy fix last, which leaves the product they depend on as it is.  ``fitted``: the reported
    ``(g_r, g_i, c_r, c_i)`` before that fix, what the loop hands to the next time."""
    prob, errs, dspec, degen = cfg.prob, cfg.errs, cfg.dspec, cfg.degen
    results = result.loops * nt if cfg.gain_time_basis is not None else result.loops  # a joint fit is one loop: every time reports it
    cur = fitter.get_params(0)
    best = fitter.get_params(1) if cfg.use_min and any(len(r[0]) for r in results) else None
    gm_r, gm_i = np.array(cur[0]), np.array(cur[1])
    cm_r, cm_i = (arrs["c_r"], arrs["c_i"]) if cfg.freeze_model else (np.array(cur[2]), np.array(cur[3]))
    for t, res in enumerate(results):
        if best is not None and len(res[0]):
            ga, gb = slice(t * prob.nants, (t + 1) * prob.nants), slice(t * prob.ncoeffs, (t + 1) * prob.ncoeffs)
            gm_r[ga], gm_i[ga] = best[0][ga], best[1][ga]
            if not cfg.freeze_model:
                cm_r[gb], cm_i[gb] = best[2][gb], best[3][gb]
    fitter.set_params(c_r=cm_r, c_i=cm_i)
    m_r, m_i = fitter.model()
    out = dict(result=result, results=results, fitted=(gm_r, gm_i, cm_r, cm_i), quality=None, errors=None, spectra=None, transfer=None, cross=None, fringe=None, redundant=None, fixed=None)
    if cfg.fit_quality:
        out["quality"] = fitter.fit_quality(gm_r, gm_i)
    if errs is not None and (errs["with_gains"] or errs["basis_gains"] or not cfg.freeze_model):
        fitter.set_params(gm_r, gm_i)  # the reported gains; the fit is over, the next one sets its own
        out["errors"] = fitter.fit_errors(ridge=errs["ridge"], model_var=errs["samples"], gain_var=errs["with_gains"], coeffs=not cfg.freeze_model)
        if errs["basis_gains"]:  # the error bars of basis gains, and the parameters they spent (one per row of y)
            basis = fitter.gain_basis_errors(ridge=errs["ridge"], y_var=False)
            out["errors"].update(gain_var=basis["gain_var"], gain_dof=basis["gain_dof"])
        out["errors"]["chisq_bl"] = (out["quality"] if out["quality"] is not None else fitter.fit_quality(gm_r, gm_i))["chisq_bl"]
    if dspec is not None:  # every slice (a joint fit: every time) has bins of its own: bin_of_bl encodes (t, length bin)
        out["spectra"] = fitter.delay_spectrum(dspec["op"], dspec["norm_f"], calibrated=dspec["calibrated"], bin_of_bl=cal.delay_spectrum_slice_bins(dspec, nt),
                                               nbins=nt * dspec["nbins"], per_baseline=dspec["per_baseline"], g_r=gm_r, g_i=gm_i)
        if dspec["transfer_ridge"] is not None:  # the signal loss of the same spectrum: its operator, bins and gains
            out["transfer"] = fitter.delay_transfer(dspec["op"], ridge=dspec["transfer_ridge"], calibrated=dspec["calibrated"],
                                                    bin_of_bl=cal.delay_spectrum_slice_bins(dspec, nt), nbins=nt * dspec["nbins"],
                                                    per_baseline=dspec["per_baseline"], g_r=gm_r, g_i=gm_i)
        pairing = cal.delay_cross_pairing(arrs["polnum"], arrs["time_index"]) if dspec["cross"] is not None else []
        if pairing:  # the cross power of paired times: the spectrum's operator, calibrated switch and gains; a bin per (pair, length bin)
            pairs, scale, bins = cal.delay_cross_rows(pairing, dspec, arrs["rms"], prob.nbls)
            out["cross"] = dict(fitter.delay_cross_spectrum(dspec["op"], dspec["norm_f"], pairs, scale=scale, calibrated=dspec["calibrated"], bin_of_pair=bins,
                                                            nbins=len(pairing) * dspec["nbins"], per_pair=dspec["cross"] == "baselines", g_r=gm_r, g_i=gm_i),
                                pairing=pairing, time_index=list(arrs["time_index"]))
        fr = dspec["fringe"]
        windows = cal.delay_fringe_windows(arrs["polnum"], arrs["time_index"], fr["ntimes"], fr["times"], fr["dt"]) if fr is not None else []
        if windows:  # the delay / fringe-rate plane of whole windows: the spectrum's operator, calibrated switch and gains; a bin per (window, length bin)
            rows, scale, bins = cal.delay_fringe_rows(windows, dspec, arrs["rms"], prob.nbls)
            out["fringe"] = dict(fitter.delay_fringe_spectrum(dspec["op"], dspec["norm_f"], rows, fr["opt"], scale=scale, calibrated=dspec["calibrated"],
                                                              bin_of_group=bins, nbins=len(windows) * dspec["nbins"], per_group=fr["per_group"], g_r=gm_r, g_i=gm_i),
                                 windows=windows, time_index=list(arrs["time_index"]))
        rd = dspec.get("redundant")
        windows = cal.delay_fringe_windows(arrs["polnum"], arrs["time_index"], rd["ntimes"], rd["times"], rd["dt"]) if rd is not None else []
        if windows:  # the redundant groups' averages over whole windows: the spectrum's operator and gains, calibrated; a bin per (window, length bin of the groups)
            set_ptr, member_row, member_conj, scale, bins = cal.delay_redundant_sets(windows, rd, arrs["rms"], prob.nbls)
            out["redundant"] = dict(fitter.delay_coherent_spectrum(dspec["op"], dspec["norm_f"], set_ptr, member_row, rd["opt"], member_conj=member_conj,
                                                                   weighting=rd["weighting"], scale=scale, calibrated=True, bin_of_group=bins,
                                                                   nbins=len(windows) * rd["nbins"], per_group=rd["per_group"], g_r=gm_r, g_i=gm_i),
                                    windows=windows, time_index=list(arrs["time_index"]))
    if degen is not None:
        ref_phase = (arrs["g_r"], arrs["g_i"]) if degen["phase_ref"] else (None, None)
        out["fixed"] = fitter.fix_degeneracies(arrs["s_r"], arrs["s_i"], degen["antpos"], ref_w=arrs["r_w"], mode=degen["mode"], iters=degen["iters"],
                                               freqs=degen["freqs"], g_r=gm_r, g_i=gm_i, gref_r=ref_phase[0], gref_i=ref_phase[1])
        m_r, m_i, gm_r, gm_i = (out["fixed"][k] for k in ("model_r", "model_i", "g_r", "g_i"))
    return dict(out, m_r=m_r, m_i=m_i, gm_r=gm_r, gm_i=gm_i)


def write(cfg, sl, t, out):
    """Stage 4, slice ``t`` of a report into the containers (``sl``: what ``tensorize`` gave for it): model rows and gains
    (calibration.py:1271-1300), the slice's ``fit_history`` entry -- losses and what the loop's actions recorded, the reweighting in
    the data's units keyed by antenna numbers, quality, errors, degeneracies, delay spectrum --, the post-hoc renormalisation
    (:1311-1319), which leaves ``g_i conj(g_j) m`` as it is, then residual and calibration state of the outputs (:1322-1331).
    Returns the entry."""
    prob, gains, errs = cfg.prob, cfg.gains, cfg.errs
    pol, time, rms = sl["pol"], sl["time"], sl["rms"]
    rows, ga = slice(t * prob.nbls, (t + 1) * prob.nbls), slice(t * prob.nants, (t + 1) * prob.nants)
    cal._insert_model_rows(cfg.model, time, pol, cfg.ants_map, prob, out["m_r"][rows], out["m_i"][rows], scale_factor=rms)
    cal.insert_gains_into_uvcal(uvcal=gains, time=time, polarization=pol, gains_re=out["gm_r"][ga], gains_im=out["gm_i"][ga])
    result, loop = out["result"], 0 if cfg.gain_time_basis is not None else t
    rb = result.robust
    if rb is not None:  # the slice's rows of it, from solver units and row order
        rb = cal.robust_history(rb["rounds"][loop], rb["ndown_bl"][rows], rb["scale_bl"][rows], rms, prob, gains.ant_array)
    hist = history_entry(cfg.controls, result, loop, cfg.dtype, robust=rb)
    q, e = out["quality"], out["errors"]
    if q is not None:
        q = dict(chisq_ant=q["chisq_ant"][ga], wsum_ant=q["wsum_ant"][ga], chisq_bl=q["chisq_bl"][rows], wsum_bl=q["wsum_bl"][rows])
        cal.insert_fit_quality(gains, hist, time, pol, q, rms, prob)
    if e is not None:
        coefs = slice(t * prob.ncoeffs, (t + 1) * prob.ncoeffs)
        e = {k: e[k][{"gain_var": ga, "coeff_var": coefs}.get(k, rows)] for k in ("coeff_var", "model_var", "leverage_bl", "nsamp_bl", "gain_var", "chisq_bl") if k in e}
        if "coeff_var" in e:  # (the library counts over the batch: a slice's singular groups are those it left an all-zero coeff_var)
            e["nsingular"] = sum(1 for g in range(prob.ngrps) if not np.any(e["coeff_var"][prob.grp_coff[g] : prob.grp_coff[g + 1]]))
        dof, joint = out["errors"].get("gain_dof"), cfg.gain_time_basis is not None
        if dof is not None and not joint:
            dof = dof[ga]
        # (a joint fit shares an antenna's coefficients among its times: each is charged its share of them)
        cal.insert_fit_errors(errs["gain_std"], gains, hist, time, pol, e, e["chisq_bl"], rms, prob, gain_dof=dof, ntimes=len(out["results"]) if joint else 1)
    if out["fixed"] is not None:
        hist["degeneracies"] = entry = cal.degeneracy_entry(out["fixed"], t, cfg.degen)
        if errs is not None and errs["gain_std"] is not None:  # the slice's plane of gain_std follows the gains: times e^{-eta}
            polnum = np.where(np.asarray(gains.jones_array) == polstr2num(pol, x_orientation=gains.x_orientation))[0][0]
            gindt = np.where(np.isclose(gains.time_array, time, atol=1e-7, rtol=0.0))[0][0]
            errs["gain_std"][:, :, gindt, polnum] /= entry["amplitude"][None, :]
    if out["spectra"] is not None:
        hist["delay_spectrum"] = cal.delay_spectrum_entry(cal.delay_spectrum_of_slice(out["spectra"], cfg.dspec, t, prob.nbls), cfg.dspec, rms, prob, gains.ant_array)
        if out["transfer"] is not None:
            hist["delay_spectrum"].update(cal.delay_transfer_entry(cal.delay_transfer_of_slice(out["transfer"], cfg.dspec, t, prob.nbls), prob, gains.ant_array))
        if out["cross"] is not None:
            for k, pair in enumerate(out["cross"]["pairing"]):
                if t in pair:
                    partner = out["cross"]["time_index"][pair[1] if t == pair[0] else pair[0]]
                    hist["delay_spectrum"]["cross"] = cal.delay_cross_entry(out["cross"], cfg.dspec, k, partner, prob, gains.ant_array)
        if out["fringe"] is not None:
            for k, win in enumerate(out["fringe"]["windows"]):
                if t in win:
                    hist["delay_spectrum"]["fringe"] = cal.delay_fringe_entry(out["fringe"], cfg.dspec, k, [out["fringe"]["time_index"][m] for m in win], prob,
                                                                              gains.ant_array)
        if out["redundant"] is not None:
            for k, win in enumerate(out["redundant"]["windows"]):
                if t in win:
                    hist["delay_spectrum"]["redundant"] = cal.delay_redundant_entry(out["redundant"], cfg.dspec["redundant"], k,
                                                                                    [out["redundant"]["time_index"][m] for m in win], rms)
    if out["results"][t][1]:
        echo(f"Tolerance thresshold met for time {sl['time_index']}. Terminating...\n ", verbose=cfg.verbose)
    if not cfg.freeze_model and cfg.model_regularization == "post_hoc":
        if np.any(~cfg.model.flag_array[np.isclose(cfg.uvdata.time_array, time, atol=1e-7, rtol=0.0)]):
            cal.renormalize(uvdata_reference_model=cfg.sky_model, uvdata_deconv=cfg.model, gains=gains, polarization=pol, time=time,
                            additional_flags=cfg.uvdata.flag_array)
    cfg.finish(sl["polnum"], time)
    return hist


from . import calibration as cal  # noqa: E402 -- last: calibration takes names from this module while it loads, the stages use its write-back helpers when they run
