"""The time loop of calibrate_and_model_tensor as ONE batch, on one or several GPUs.

The reference fits the (polarization, time) slices of a data set one after another on one device
(/root/reference/calamity/calibration.py:1160-1167, :1244-1269; device selection :1796-1804).  The slices are independent
fits over the same array and the same modeling components, so here ``SliceBatchFitter`` puts T of them into one solver per
device (``FitProblem.nslices``: every slice keeps its own gains, weights, rms scale, priors, loss history, tolerance stop and
use_min snapshot -- include/calamity_hip.h: cal_solver_run_slices) and, with several devices, gives each device a share of the
fitting groups of EVERY slice (``distributed.partition_groups``): coefficients are local to the device that owns the group,
gains are replicated, and each train step exchanges the per-antenna gain gradients and the per-slice loss scalars once
(RCCL between distinct devices; through the library's exchange hook between workers that share a device).

The caller's process stays the only one: a worker is a thread that drives one ``HipFitSolver`` (ctypes releases the GIL for
the duration of a library call, so the workers' launches and collectives run side by side).
"""
import threading

import numpy as np

from . import distributed
from .problem import FitProblem
from .solver import HipFitSolver, comm_unique_id


def replicate_slices(prob, nt, groups=None, share_tiles=True):
    """The (data-less) problem of ``nt`` time slices of ``prob`` -- optionally only the fitting groups ``groups`` of every
    slice (a device's share).  Slice ``t`` uses antennas ``[t * nants, (t + 1) * nants)``; its baselines read the basis tiles of
    slice 0's (``bl_alias``: the STREAM layout then holds one copy and processes the slices of a baseline together).
    Returns (FitProblem with ``nslices = nt``, baseline indices of one slice, coefficient indices of one slice)."""
    groups = np.arange(prob.ngrps) if groups is None else np.asarray(groups)

    def runs(starts, counts):  # concatenation of arange(start, start + count) without a python loop over 61 075 groups
        starts, counts = np.asarray(starts, dtype=np.int64), np.asarray(counts, dtype=np.int64)
        ends = np.cumsum(counts)
        return np.repeat(starts - (ends - counts), counts) + np.arange(ends[-1] if len(ends) else 0, dtype=np.int64)

    starts, nbl_g = prob.grp_bl_start[groups], np.diff(prob.grp_bl_start)[groups]
    bl = runs(starts, nbl_g)
    coff = prob.grp_coff
    cidx = runs(coff[groups], coff[groups + 1] - coff[groups])
    used = np.unique(prob.grp_basis[groups])
    remap = -np.ones(len(prob.basis), dtype=np.int64)
    remap[used] = np.arange(len(used))
    nb = len(bl)
    single = bool(np.all(nbl_g == 1))
    sub = FitProblem(
        nants=prob.nants * nt,
        nfreqs=prob.nfreqs,
        basis=[prob.basis[u] for u in used],
        grp_basis=np.tile(remap[prob.grp_basis[groups]].astype(np.int32), nt),
        grp_bl_start=np.concatenate([[0], np.cumsum(np.tile(nbl_g, nt))]).astype(np.int32),
        bl_ant0=np.concatenate([prob.bl_ant0[bl] + t * prob.nants for t in range(nt)]).astype(np.int32),
        bl_ant1=np.concatenate([prob.bl_ant1[bl] + t * prob.nants for t in range(nt)]).astype(np.int32),
        bl_rowblk=np.tile(prob.bl_rowblk[bl], nt).astype(np.int32),
        data_r=None,
        data_i=None,
        wgts=None,
        bl_alias=(np.concatenate([np.full(nb, -1, dtype=np.int32)] + [np.arange(nb, dtype=np.int32)] * (nt - 1))
                  if share_tiles and single and nt > 1 else None),
        nslices=nt,
        chunk_of_grp=None if prob.chunk_of_grp is None else np.tile(np.asarray(prob.chunk_of_grp)[groups], nt).astype(np.int32),
    )
    return sub, bl, cidx


def split_pairs(pairs, rows, nbls):
    """Share out ``pairs`` ``[npairs, 2]`` of global rows over the workers whose global rows are ``rows[r]`` (in the worker's local
    order): ``(sel, local)`` with ``sel[r]`` the positions of worker ``r``'s pairs in ``pairs`` and ``local[r]`` those pairs as its
    local rows.  ``ValueError`` for a pair whose rows lie on two workers and for a worker without a pair."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    owner, where = np.full(nbls, -1, dtype=np.int64), np.zeros(nbls, dtype=np.int64)
    for r, idx in enumerate(rows):
        owner[idx], where[idx] = r, np.arange(len(idx))
    own = owner[pairs]
    split = np.nonzero(own[:, 0] != own[:, 1])[0]
    if len(split):
        p = int(split[0])
        raise ValueError(f"pair {p} = ({pairs[p, 0]}, {pairs[p, 1]}) joins rows of two workers ({own[p, 0]}, {own[p, 1]})")
    sel = [np.nonzero(own[:, 0] == r)[0] for r in range(len(rows))]
    for r, s in enumerate(sel):
        if len(s) == 0:
            raise ValueError(f"worker {r} holds no pair: every worker must take part in the exchange of the bins")
    return sel, [where[pairs[s]].astype(np.int32) for s in sel]


def split_groups(groups, rows, nbls):
    """``split_pairs`` for groups of any length: share out ``groups`` ``[ngroups, T]`` of global rows over the workers whose global
    rows are ``rows[r]`` (in the worker's local order): ``(sel, local)`` with ``sel[r]`` the positions of worker ``r``'s groups in
    ``groups`` and ``local[r]`` those groups as its local rows.  ``ValueError`` for a group whose rows lie on several workers and for a
    worker without a group."""
    groups = np.asarray(groups, dtype=np.int64)
    groups = groups.reshape(-1, groups.shape[-1])
    owner, where = np.full(nbls, -1, dtype=np.int64), np.zeros(nbls, dtype=np.int64)
    for r, idx in enumerate(rows):
        owner[idx], where[idx] = r, np.arange(len(idx))
    own = owner[groups]
    split = np.nonzero((own != own[:, :1]).any(axis=1))[0]
    if len(split):
        g = int(split[0])
        raise ValueError(f"group {g} = {tuple(int(v) for v in groups[g])} joins rows of several workers {tuple(int(v) for v in own[g])}")
    sel = [np.nonzero(own[:, 0] == r)[0] for r in range(len(rows))]
    for r, s in enumerate(sel):
        if len(s) == 0:
            raise ValueError(f"worker {r} holds no group: every worker must take part in the exchange of the bins")
    return sel, [where[groups[s]].astype(np.int32) for s in sel]


def split_member_groups(set_ptr, member_row, ntimes, rows, nbls):
    """``split_groups`` for groups of ``ntimes`` ragged sets (``HipFitSolver.delay_coherent_spectrum``): ``(sel, parts)`` with
    ``sel[r]`` the positions of worker ``r``'s groups and ``parts[r] = (set_ptr, member_row, members)`` those groups' sets over its
    local rows and the positions of their members in the caller's member arrays.  A group without members goes to worker 0.
    ``ValueError`` for a group whose member rows lie on several workers and for a worker without a group."""
    set_ptr, member_row = np.asarray(set_ptr, dtype=np.int64), np.asarray(member_row, dtype=np.int64)
    ngroups = (len(set_ptr) - 1) // int(ntimes)
    owner, where = np.full(nbls, -1, dtype=np.int64), np.zeros(nbls, dtype=np.int64)
    for r, idx in enumerate(rows):
        owner[idx], where[idx] = r, np.arange(len(idx))
    gptr = set_ptr[:: int(ntimes)]  # the members of group g are gptr[g] .. gptr[g + 1]
    own = np.zeros(ngroups, dtype=np.int64)
    for g in range(ngroups):
        o = owner[member_row[gptr[g]:gptr[g + 1]]]
        if len(o) and np.any(o != o[0]):
            raise ValueError(f"group {g} joins rows of several workers {tuple(int(v) for v in np.unique(o))}")
        own[g] = o[0] if len(o) else 0
    sel, parts = [np.nonzero(own == r)[0] for r in range(len(rows))], []
    for r, s in enumerate(sel):
        if len(s) == 0:
            raise ValueError(f"worker {r} holds no group: every worker must take part in the exchange of the bins")
        sets = (s[:, None] * int(ntimes) + np.arange(int(ntimes))[None, :]).ravel()
        counts = set_ptr[sets + 1] - set_ptr[sets]
        members = np.concatenate([np.arange(set_ptr[v], set_ptr[v + 1]) for v in sets]) if len(sets) else np.zeros(0, dtype=np.int64)
        parts.append((np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), where[member_row[members.astype(np.int64)]].astype(np.int32),
                      members.astype(np.int64)))
    return sel, parts


class _HostExchange:
    """In-process all-reduce between worker threads (cal_solver_set_exchange_hook): every worker leaves a view of its staging
    buffer, all of them reduce the views in rank order -- the same arithmetic on every worker -- and each writes the result
    back into its own buffer.

    Every worker also leaves the signature of its call, (dtype, size, op), and after the first barrier every worker checks
    ALL of them: workers that issue different exchanges (a rank that took another path through a step) all raise the same
    ExchangeMismatch, naming every rank's call, instead of reducing unrelated buffers or leaving one of them waiting alone."""

    def __init__(self, n):
        self.n = n
        self.barrier = threading.Barrier(n)
        self.slots = [None] * n
        self.sigs = [None] * n
        self.error = None  # the first mismatch seen (every worker raises it)

    def hook(self, rank):
        def all_reduce(arr, op):
            self.slots[rank] = arr
            self.sigs[rank] = (arr.dtype.str, int(arr.size), op)
            self.barrier.wait(timeout=600)
            sigs = list(self.sigs)  # (all workers read the same slots: all raise, or none)
            if any(s != sigs[0] for s in sigs):
                err = ExchangeMismatch("the workers issued different exchanges: "
                                       + "; ".join(f"rank {r}: dtype {s[0]}, {s[1]} elements, {s[2]}" for r, s in enumerate(sigs)))
                if self.error is None:
                    self.error = err
                raise err
            if op == "min":
                out = np.minimum.reduce([self.slots[r] for r in range(self.n)])
            else:
                out = self.slots[0].copy()
                for r in range(1, self.n):
                    out += self.slots[r]
            self.barrier.wait(timeout=600)
            arr[:] = out
            self.barrier.wait(timeout=600)

        return all_reduce

    def abort(self):
        self.barrier.abort()


class ExchangeMismatch(RuntimeError):
    """Workers of one fit issued exchanges of different dtype, size or reduction."""


class SliceBatchFitter:
    """``nt`` time slices of the data-less single-slice problem ``prob`` on ``devices`` (one worker per entry; an entry may
    repeat, the workers then share that GPU and exchange through host memory).  Arrays handed in and out are GLOBAL and
    slice-major: per-sample arrays ``[nt * nbls, nfreqs]``, gains ``[nt * nants, nfreqs]``, coefficients ``[nt * ncoeffs]``."""

    def __init__(self, prob, nt, dtype=np.float32, layout="shared", devices=(0,), kernel_path="auto", communicator_of_one=False, joint=False):
        """``joint``: the slices are ONE fit with one loop state whose loss is the sum over them (``nslices = 1``, the layout of
        ``distributed.batch_time_slices(per_slice=False)``): what a gain time basis needs (``set_gain_time_basis``).  ``run_slices``
        then returns one result.
        ``communicator_of_one``: with a single device, join a one-rank RCCL communicator anyway (from the worker thread, like the
        workers of several devices do) so that the exchange path -- the set-up agreement, an all-reduce per step -- runs on a
        one-GPU box; the numbers are those of the plain fit."""
        self.prob, self.nt, self.dtype = prob, int(nt), np.dtype(dtype)
        self.devices = [int(d) for d in devices]
        D = self.nworkers = len(self.devices)
        if D > 1:
            shares = distributed.partition_groups(prob.grp_nvec, prob.grp_basis, np.diff(prob.grp_bl_start), D)
            if any(len(s) == 0 for s in shares):
                raise ValueError(f"{prob.ngrps} fitting groups cannot be shared out over {D} devices")
        else:
            shares = [None]
        self.subs, self.rows, self.cidx = [], [], []
        for r in range(D):
            sub, bl, cidx = replicate_slices(prob, self.nt, shares[r])
            if joint:
                sub.nslices = 1
            self.subs.append(sub)
            # rows / coefficients of this worker in the global slice-major arrays
            self.rows.append(np.concatenate([bl + t * prob.nbls for t in range(self.nt)]))
            self.cidx.append(np.concatenate([cidx + t * prob.ncoeffs for t in range(self.nt)]))
        self.solvers, self._host_exchange = [], None
        try:
            self._set_up(prob, layout, kernel_path, communicator_of_one)
        except BaseException:
            self.close()  # (the solvers created so far: their device memory goes back at once)
            raise

    def _set_up(self, prob, layout, kernel_path, communicator_of_one):
        D = self.nworkers
        for d in self.devices:  # (every device index is checked here, before any worker waits for a peer in the communicator set-up)
            self.solvers.append(HipFitSolver(dtype=self.dtype, device=d))
        if D == 1 and communicator_of_one:
            uid = comm_unique_id()
            self._each_threaded(lambda r, s: s.comm_init(uid, 0, 1))
        if D > 1:
            if len(set(self.devices)) == D:
                uid = comm_unique_id()
                self._each(lambda r, s: s.comm_init(uid, r, D))
            else:
                self._host_exchange = _HostExchange(D)
                for r, s in enumerate(self.solvers):
                    s.set_exchange_hook(self._host_exchange.hook(r), r, D)
        # (with a communicator set_problem ends in an agreement between the workers: concurrently)
        self._each(lambda r, s: s.set_problem(self.subs[r], layout=layout, kernel_path=kernel_path))
        self.nbls, self.ncoeffs, self.nants, self.nfreqs = prob.nbls * self.nt, prob.ncoeffs * self.nt, prob.nants * self.nt, prob.nfreqs

    def _each(self, fn):
        """fn(rank, solver) on every worker, side by side; the first exception is raised in the caller."""
        if self.nworkers == 1:
            return [fn(0, self.solvers[0])]
        return self._each_threaded(fn)

    def _each_threaded(self, fn):
        out, errs = [None] * self.nworkers, [None] * self.nworkers

        def work(r):
            try:
                out[r] = fn(r, self.solvers[r])
            except BaseException as e:  # noqa: BLE001 -- handed to the caller below
                errs[r] = e
                if self._host_exchange is not None:
                    self._host_exchange.abort()  # the others must not wait for this worker in an exchange

        threads = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(self.nworkers)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        if self._host_exchange is not None and self._host_exchange.error is not None and any(e is not None for e in errs):
            # (the library reports a failed hook by its return code only: name what the workers disagreed on)
            raise self._host_exchange.error from next(e for e in errs if e is not None)
        for e in errs:
            if e is not None:
                raise e
        return out

    def close(self):
        for s in self.solvers:
            s.close()

    def memory_bytes(self):
        return max(s.memory_bytes() for s in self.solvers)

    # ---- pass-throughs on global arrays
    def _take(self, a, r):
        return a if self.nworkers == 1 else np.take(a, self.rows[r], axis=0)

    def set_data(self, data_r, data_i, wgts):
        self._each(lambda r, s: s.set_data(self._take(data_r, r), self._take(data_i, r), self._take(wgts, r)))

    def init_coeffs(self, src_r, src_i):
        self._each(lambda r, s: s.init_coeffs(self._take(src_r, r), self._take(src_i, r)))

    def set_params(self, g_r=None, g_i=None, c_r=None, c_i=None):
        def one(r, s):
            sel = (lambda c: None if c is None else (c if self.nworkers == 1 else c[self.cidx[r]]))
            s.set_params(g_r, g_i, sel(c_r), sel(c_i))

        self._each(one)

    def _scatter(self, parts, index):
        """The global array of the workers' ``parts``, worker ``r``'s at ``index[r]`` (``self.rows``: baseline rows, ``self.cidx``:
        coefficients); one worker's part is the array already."""
        if self.nworkers == 1:
            return parts[0]
        out = np.empty((sum(len(i) for i in index),) + parts[0].shape[1:], dtype=parts[0].dtype)
        for i, part in zip(index, parts):
            out[i] = part
        return out

    def get_params(self, which=0):
        outs = self._each(lambda r, s: s.get_params(which))
        return (*outs[0][:2], *(self._scatter([o[k] for o in outs], self.cidx) for k in (2, 3)))  # the gains are replicated

    def eval_grads(self):
        """(loss, gain gradients, coefficient gradients) of the current parameters, like ``get_params``: the loss is the global
        sum over slices, the gain gradients are all-reduced (every worker holds them), the coefficient gradients gathered."""
        outs = self._each(lambda r, s: s.eval_grads())
        return (*outs[0][:3], *(self._scatter([o[k] for o in outs], self.cidx) for k in (3, 4)))

    def slice_losses(self):
        """Every slice's loss as of the last eval_grads (all-reduced: the same on every worker)."""
        return self.solvers[0].slice_losses()

    def model(self):
        outs = self._each(lambda r, s: s.model())
        return tuple(self._scatter([o[k] for o in outs], self.rows) for k in (0, 1))

    def fit_quality(self, g_r=None, g_i=None):
        """``HipFitSolver.fit_quality`` on the global arrays: ``chisq_ant``, ``wsum_ant`` ``[nt * nants, nfreqs]`` (with several
        workers the library has summed them over the workers: worker 0's), ``chisq_bl``, ``wsum_bl`` ``[nt * nbls]`` put back into
        the global slice-major row order like the rows of ``model()``."""
        outs = self._each(lambda r, s: s.fit_quality(g_r, g_i))
        return dict(outs[0], **{k: self._scatter([o[k] for o in outs], self.rows) for k in ("chisq_bl", "wsum_bl")})

    def delay_spectrum(self, op, norm_f, what=("data", "model", "resid"), calibrated=False, bin_of_bl=None, nbins=0, per_baseline=False,
                       g_r=None, g_i=None):
        """``HipFitSolver.delay_spectrum`` on the global arrays: ``bin_of_bl`` ``[nt * nbls]`` in the global slice-major row order (it
        decides which rows of which slices are summed together); the binned arrays and ``count_bin`` are worker 0's (with several
        workers the library has summed them over the workers), ``norm_bl`` and the ``per_baseline`` arrays are put back into the
        global row order like the rows of ``model()``."""
        bins = None if bin_of_bl is None else np.asarray(bin_of_bl)
        outs = self._each(lambda r, s: s.delay_spectrum(op, norm_f, what=what, calibrated=calibrated, bin_of_bl=None if bins is None else self._take(bins, r),
                                                        nbins=nbins, per_baseline=per_baseline, g_r=g_r, g_i=g_i))
        out = dict(outs[0], norm_bl=self._scatter([o["norm_bl"] for o in outs], self.rows))
        if per_baseline:
            out["per_baseline"] = {q: self._scatter([o["per_baseline"][q] for o in outs], self.rows) for q in outs[0]["per_baseline"]}
        return out

    def fix_degeneracies(self, ref_r, ref_i, antpos, ref_w=None, mode="channel", iters=6, freqs=None, g_r=None, g_i=None, gref_r=None,
                         gref_i=None):
        """``HipFitSolver.fix_degeneracies`` for all slices of the batch on the global arrays: ``ref_r``, ``ref_i``, ``ref_w``
        ``[nt * nbls, nfreqs]`` slice-major, ``antpos`` ``[nants of one slice, 2]``; the per-channel results are ``[nt, nfreqs]``.  A
        slice's sums need the slice whole on one worker: with several workers (the fitting groups shared out) the library refuses the
        call, since the channel sums would need an exchange per iteration."""
        return self._each(lambda r, s: s.fix_degeneracies(self._take(np.asarray(ref_r), r), self._take(np.asarray(ref_i), r), antpos,
                                                          ref_w=None if ref_w is None else self._take(np.asarray(ref_w), r), mode=mode, iters=iters,
                                                          freqs=freqs, g_r=g_r, g_i=g_i, gref_r=gref_r, gref_i=gref_i))[0]

    def _set_delay_spectrum_scratch(self, nbytes):
        self._each(lambda r, s: s._set_delay_spectrum_scratch(nbytes))

    def delay_cross_spectrum(self, op, norm_f, pairs, scale=None, what=("data", "model", "resid"), stats=("cross", "diff"), calibrated=False,
                             bin_of_pair=None, nbins=0, per_pair=False, g_r=None, g_i=None):
        """``HipFitSolver.delay_cross_spectrum`` on global slice-major rows: ``pairs`` ``[npairs, 2]`` rows of the batch.  Every worker
        takes the pairs whose two rows it holds, mapped to its local rows; a pair split over two workers raises ``ValueError`` (it
        cannot happen for the same baseline in two slices: the groups of a share are replicated over the slices), and so does a
        worker left without a pair (it could not join the exchange).  The binned arrays and ``count_bin`` are worker 0's (with several
        workers the library has summed them over the workers); ``norm_pair`` and the ``per_pair`` arrays are put back into the
        caller's pair order."""
        pairs = np.asarray(pairs, dtype=np.int64)
        if pairs.ndim != 2 or pairs.shape[1] != 2 or pairs.shape[0] < 1:
            raise ValueError(f"pairs must be [npairs >= 1, 2], got shape {pairs.shape}")
        if pairs.min() < 0 or pairs.max() >= self.nbls:
            raise ValueError(f"pairs must hold rows in [0, {self.nbls})")
        kw = dict(what=what, stats=stats, calibrated=calibrated, nbins=nbins, per_pair=per_pair, g_r=g_r, g_i=g_i)
        scale = None if scale is None else np.asarray(scale, dtype=np.float64)
        bins = None if bin_of_pair is None else np.asarray(bin_of_pair)
        if self.nworkers == 1:
            return self.solvers[0].delay_cross_spectrum(op, norm_f, pairs, scale=scale, bin_of_pair=bins, **kw)
        sel, local = split_pairs(pairs, self.rows, self.nbls)
        outs = self._each(lambda r, s: s.delay_cross_spectrum(op, norm_f, local[r], scale=None if scale is None else scale[sel[r]],
                                                              bin_of_pair=None if bins is None else bins[sel[r]], **kw))
        out = dict(outs[0], norm_pair=self._scatter([o["norm_pair"] for o in outs], sel))
        if per_pair:
            out["per_pair"] = {k: {q: self._scatter([o["per_pair"][k][q] for o in outs], sel) for q in v} for k, v in outs[0]["per_pair"].items()}
        return out

    def delay_fringe_spectrum(self, op, norm_f, rows, opt, scale=None, what=("data", "model", "resid"), calibrated=False,
                              bin_of_group=None, nbins=0, per_group=False, g_r=None, g_i=None):
        """``HipFitSolver.delay_fringe_spectrum`` on global slice-major rows: ``rows`` ``[ngroups, T]`` rows of the batch.  Every worker
        takes the groups whose rows it all holds, mapped to its local rows; a group split over workers raises ``ValueError`` (it cannot
        happen for one baseline in several slices: the groups of a share are replicated over the slices), and so does a worker left
        without a group (it could not join the exchange).  The binned arrays and ``count_bin`` are worker 0's (with several workers the
        library has summed them over the workers); ``norm_grp`` and the ``per_group`` arrays are put back into the caller's order."""
        rows = np.asarray(rows, dtype=np.int64)
        if rows.ndim != 2 or rows.shape[0] < 1 or rows.shape[1] < 1:
            raise ValueError(f"rows must be [ngroups >= 1, ntimes >= 1], got shape {rows.shape}")
        if rows.min() < 0 or rows.max() >= self.nbls:
            raise ValueError(f"rows must hold rows in [0, {self.nbls})")
        kw = dict(what=what, calibrated=calibrated, nbins=nbins, per_group=per_group, g_r=g_r, g_i=g_i)
        scale = None if scale is None else np.asarray(scale, dtype=np.float64)
        bins = None if bin_of_group is None else np.asarray(bin_of_group)
        if self.nworkers == 1:
            return self.solvers[0].delay_fringe_spectrum(op, norm_f, rows, opt, scale=scale, bin_of_group=bins, **kw)
        sel, local = split_groups(rows, self.rows, self.nbls)
        outs = self._each(lambda r, s: s.delay_fringe_spectrum(op, norm_f, local[r], opt, scale=None if scale is None else scale[sel[r]],
                                                               bin_of_group=None if bins is None else bins[sel[r]], **kw))
        out = dict(outs[0], norm_grp=self._scatter([o["norm_grp"] for o in outs], sel))
        if per_group:
            out["per_group"] = {q: self._scatter([o["per_group"][q] for o in outs], sel) for q in outs[0]["per_group"]}
        return out

    def delay_coherent_spectrum(self, op, norm_f, set_ptr, member_row, opt, member_wgt=None, member_conj=None, weighting="uniform", scale=None,
                                what=("data", "model", "resid"), calibrated=False, bin_of_group=None, nbins=0, per_group=False, g_r=None, g_i=None):
        """``HipFitSolver.delay_coherent_spectrum`` on global slice-major rows: ``member_row`` holds rows of the batch.  Every worker
        takes the groups whose member rows it all holds, mapped to its local rows (a group without members goes to worker 0); a group
        split over workers raises ``ValueError``, and so does a worker left without a group, as in ``delay_fringe_spectrum``.  The
        binned arrays and ``count_bin`` are worker 0's (with several workers the library has summed them over the workers);
        ``norm_grp`` and the ``per_group`` arrays are put back into the caller's order."""
        set_ptr = np.asarray(set_ptr, dtype=np.int64)
        member_row = np.asarray(member_row, dtype=np.int64)
        ntimes = np.asarray(opt).shape[0] if np.asarray(opt).ndim == 2 else 0
        if ntimes < 1 or set_ptr.ndim != 1 or len(set_ptr) < ntimes + 1 or (len(set_ptr) - 1) % ntimes:
            raise ValueError(f"set_ptr must be [ngroups ntimes + 1] with ntimes = opt.shape[0] and ngroups >= 1, got shape {set_ptr.shape}")
        if set_ptr[0] != 0 or np.any(np.diff(set_ptr) < 0) or set_ptr[-1] != len(member_row):
            raise ValueError("set_ptr must start at 0, never fall and end at len(member_row)")
        if len(member_row) and (member_row.min() < 0 or member_row.max() >= self.nbls):
            raise ValueError(f"member_row must hold rows in [0, {self.nbls})")
        kw = dict(weighting=weighting, what=what, calibrated=calibrated, nbins=nbins, per_group=per_group, g_r=g_r, g_i=g_i)
        scale = None if scale is None else np.asarray(scale, dtype=np.float64)
        bins = None if bin_of_group is None else np.asarray(bin_of_group)
        wgt = None if member_wgt is None else np.asarray(member_wgt, dtype=np.float64)
        cj = None if member_conj is None else np.asarray(member_conj)
        if self.nworkers == 1:
            return self.solvers[0].delay_coherent_spectrum(op, norm_f, set_ptr, member_row, opt, member_wgt=wgt, member_conj=cj, scale=scale,
                                                           bin_of_group=bins, **kw)
        sel, parts = split_member_groups(set_ptr, member_row, ntimes, self.rows, self.nbls)
        outs = self._each(lambda r, s: s.delay_coherent_spectrum(
            op, norm_f, parts[r][0], parts[r][1], opt, member_wgt=None if wgt is None else wgt[parts[r][2]],
            member_conj=None if cj is None else cj[parts[r][2]], scale=None if scale is None else scale[sel[r]],
            bin_of_group=None if bins is None else bins[sel[r]], **kw))
        out = dict(outs[0], norm_grp=self._scatter([o["norm_grp"] for o in outs], sel))
        if per_group:
            out["per_group"] = {q: self._scatter([o["per_group"][q] for o in outs], sel) for q in outs[0]["per_group"]}
        return out

    def delay_transfer(self, op, ridge=1e-6, calibrated=False, bin_of_bl=None, nbins=0, per_baseline=False, g_r=None, g_i=None):
        """``HipFitSolver.delay_transfer`` on the global arrays, like ``delay_spectrum``: ``bin_of_bl`` ``[nt * nbls]`` in the global
        slice-major row order; ``absorbed_bin`` and ``count_bin`` are worker 0's (with several workers the library has summed them
        over the workers), ``absorbed_bl`` and ``noise_bl`` are put back into the global row order like the rows of ``model()``; the
        counts of groups are summed."""
        bins = None if bin_of_bl is None else np.asarray(bin_of_bl)
        outs = self._each(lambda r, s: s.delay_transfer(op, ridge=ridge, calibrated=calibrated, bin_of_bl=None if bins is None else self._take(bins, r),
                                                        nbins=nbins, per_baseline=per_baseline, g_r=g_r, g_i=g_i))
        out = dict(outs[0], **{k: sum(o[k] for o in outs) for k in ("nsolved", "nsingular")})
        if per_baseline:
            out.update({k: self._scatter([o[k] for o in outs], self.rows) for k in ("absorbed_bl", "noise_bl")})
        return out

    def _set_delay_transfer_scratch(self, nbytes):
        self._each(lambda r, s: s._set_delay_transfer_scratch(nbytes))

    def fit_errors(self, ridge=1e-6, model_var=True, gain_var=True, coeffs=True):
        """``HipFitSolver.fit_errors`` on the global arrays: ``gain_var`` ``[nt * nants, nfreqs]`` (with several workers the library
        has summed ``den`` over the workers: worker 0's), ``model_var``, ``leverage_bl``, ``nsamp_bl`` with their rows and
        ``coeff_var`` with its coefficients put back into the global slice-major order like ``model()`` and ``get_params()``; the
        counts are summed."""
        outs = self._each(lambda r, s: s.fit_errors(ridge=ridge, model_var=model_var, gain_var=gain_var, coeffs=coeffs))
        out = {k: sum(o[k] for o in outs) for k in ("nsolved", "nsingular")}
        for k in ("model_var", "leverage_bl", "nsamp_bl"):
            if k in outs[0]:
                out[k] = self._scatter([o[k] for o in outs], self.rows)
        if "coeff_var" in outs[0]:
            out["coeff_var"] = self._scatter([o["coeff_var"] for o in outs], self.cidx)
        if "gain_var" in outs[0]:
            out["gain_var"] = outs[0]["gain_var"]
        return out

    def robust_weights(self, kind="huber", threshold=3.0, slice_mask=None):
        """``HipFitSolver.robust_weights`` on every worker (``slice_mask``: one entry per slice of the batch; one entry for a ``joint``
        fitter): each worker reweights its own baseline rows, nothing is exchanged.  ``scale_bl``, ``ndown_bl`` ``[nt * nbls]`` put
        back into the global slice-major row order like the rows of ``model()``."""
        outs = self._each(lambda r, s: s.robust_weights(kind=kind, threshold=threshold, slice_mask=slice_mask))
        return {k: self._scatter([o[k] for o in outs], self.rows) for k in ("scale_bl", "ndown_bl")}

    def get_weights(self, which=0):
        """``HipFitSolver.get_weights`` of every worker, the rows put back into the global slice-major order."""
        return self._scatter(self._each(lambda r, s: s.get_weights(which)), self.rows)

    def solve_gains(self, nsweeps, damping=0.5, slice_mask=None, reset_gain_moments=False):
        """``HipFitSolver.solve_gains`` on every worker (``slice_mask``: one entry per slice of the batch; one entry for a ``joint``
        fitter).  With several workers each sweep sums the three antenna planes of the workers' baselines in one exchange, and every
        worker applies the same update to its replica of the gains."""
        self._each(lambda r, s: s.solve_gains(nsweeps, damping=damping, slice_mask=slice_mask, reset_gain_moments=reset_gain_moments))

    def solve_coeffs(self, niters=1, damping=1.0, ridge=1e-6, slice_mask=None, reset_coeff_moments=False):
        """``HipFitSolver.solve_coeffs`` on every worker (``slice_mask``: one entry per slice of the batch; one entry for a ``joint``
        fitter).  Every fitting group belongs to one worker and the gains are replicated: no exchange.  The counts are summed."""
        outs = self._each(lambda r, s: s.solve_coeffs(niters=niters, damping=damping, ridge=ridge, slice_mask=slice_mask,
                                                      reset_coeff_moments=reset_coeff_moments))
        return {k: sum(o[k] for o in outs) for k in ("nsolved", "nsingular")}

    def gauss_newton_step(self, ncg=20, lam=1e-3, cg_tol=1e-3, slice_mask=None, reset_moments=False):
        """``HipFitSolver.gauss_newton_step`` (``lam``, ``slice_mask``: one entry per slice of the batch).  A slice's step needs the slice
        whole on one worker: with several workers (the fitting groups shared out) the library refuses the call, since the per-slice
        scalars of conjugate gradients would need an exchange.  Returns the dict of per-slice arrays, the slices in global order."""
        return self._each(lambda r, s: s.gauss_newton_step(ncg=ncg, lam=lam, cg_tol=cg_tol, slice_mask=slice_mask, reset_moments=reset_moments))[0]

    def lbfgs(self, nsteps, history=8, max_ls=20, c1=1e-4, shrink=0.5, ftol=0.0, curvature_eps=1e-8, slice_mask=None, freeze_model=False,
              reset_moments=False):
        """``HipFitSolver.lbfgs`` (``slice_mask``: one entry per slice of the batch; one entry for a ``joint`` fitter).  A slice's
        iterations need the slice whole on one worker: with several workers (the fitting groups shared out) the library refuses the
        call, since the dot products of the history would need an exchange.  Returns the dict of per-slice arrays and ``losses``, the
        slices in global order."""
        return self._each(lambda r, s: s.lbfgs(nsteps, history=history, max_ls=max_ls, c1=c1, shrink=shrink, ftol=ftol, curvature_eps=curvature_eps,
                                               slice_mask=slice_mask, freeze_model=freeze_model, reset_moments=reset_moments))[0]

    def gain_basis_errors(self, ridge=1e-6, y_var=True):
        """``HipFitSolver.gain_basis_errors`` on every worker: ``gain_var`` ``[nt * nants, nfreqs]``, ``y_var`` and ``gain_dof`` in the
        layout of ``y``.  ``y`` is replicated and the library has summed ``den`` over the workers, so every worker computes the same
        planes and counts: worker 0's are returned, as ``fit_errors`` does for ``gain_var``."""
        return self._each(lambda r, s: s.gain_basis_errors(ridge=ridge, y_var=y_var))[0]

    def solve_gain_coeffs(self, nsweeps, damping=0.5, ridge=1e-6, slice_mask=None, reset_gain_moments=False):
        """``HipFitSolver.solve_gain_coeffs`` on every worker (``slice_mask``: one entry per slice of the batch).  With several workers
        each sweep sums the three antenna planes of the workers' baselines in one exchange; ``y`` is replicated, so every worker then
        computes the same update of its replica: the counts are worker 0's."""
        outs = self._each(lambda r, s: s.solve_gain_coeffs(nsweeps, damping=damping, ridge=ridge, slice_mask=slice_mask,
                                                           reset_gain_moments=reset_gain_moments))
        return outs[0]

    def solve_gain_time_coeffs(self, nsweeps, damping=0.5, ridge=1e-6, reset_gain_moments=False):
        """``HipFitSolver.solve_gain_time_coeffs`` on every worker of a ``joint`` fitter with a time basis.  With several workers each
        sweep sums the three antenna planes of the workers' baselines in one exchange; ``y`` is replicated, so every worker then
        computes the same update of its replica: the counts are worker 0's."""
        outs = self._each(lambda r, s: s.solve_gain_time_coeffs(nsweeps, damping=damping, ridge=ridge, reset_gain_moments=reset_gain_moments))
        return outs[0]

    def hold_slices(self, mask=None):
        """``HipFitSolver.hold_slices`` on every worker."""
        self._each(lambda r, s: s.hold_slices(mask))

    def set_regularization(self, mode=None, prior_r=None, prior_i=None):
        if mode == "sum":
            self._each(lambda r, s: s.set_regularization("sum", np.asarray(prior_r, dtype=np.float64), np.asarray(prior_i, dtype=np.float64)))
        else:
            self._each(lambda r, s: s.set_regularization(None))

    def set_optimizer(self, optimizer, **kw):
        self._each(lambda r, s: s.set_optimizer(optimizer, **kw))

    def set_gain_basis(self, basis):
        """One gain basis ``[nfreqs, K]`` for every slice (``HipFitSolver.set_gain_basis``; ``None`` detaches it).  The gains are
        replicated over the workers, so every worker gets the same basis; with several workers a train step then exchanges the
        projected gain gradients."""
        self._each(lambda r, s: s.set_gain_basis(basis))

    def set_gain_time_basis(self, basis_t):
        """One time basis ``[nt, L]`` over the slices of a ``joint`` fitter (``HipFitSolver.set_gain_time_basis``; ``None`` detaches it)."""
        self._each(lambda r, s: s.set_gain_time_basis(basis_t))

    def get_gain_coeffs(self, which=0):
        """``(y_r, y_i)``, ``[nt * nants, K]`` (replicated over the workers, like the gains); ``[nants, L, K]`` with a time basis."""
        return self.solvers[0].get_gain_coeffs(which)

    def timing_enable(self, on):
        self._each(lambda r, s: s.timing_enable(on))

    def timing_get(self):
        return self.solvers[0].timing_get()

    def run_slices(self, nsteps, **kw):
        """Per slice (recorded losses, stopped, nupdates); the loop decisions are taken on the all-reduced sums, so every
        worker reports the same."""
        return self._each(lambda r, s: s.run_slices(nsteps, **kw))[0]
