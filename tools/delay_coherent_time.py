#!/usr/bin/env python3
"""What cal_solver_delay_coherent_spectrum costs at HERA-350 (350 antennas, 61 075 baselines x 1024 channels, fp32) with 1024 delays:
``--slices`` slices in ONE solver (tools/delay_fringe_time.py's: every slice holds the first's data plus independent noise), the
array's OWN redundant groups (baselines with the same vector up to sign, to 0.1 m; a row that points the other way is conjugated),
one group of ``--slices`` sets per redundant group, ``--rates`` rates, all three quantities, weighted by the weights, binned only --
beside cal_solver_delay_fringe_spectrum over the same rows and times in the same process.  The coherent call reads every member row
once (the rows kernel) and then transforms ngroups x slices averaged rows where the fringe call transforms nbls x slices.

Every call is bracketed by two HIP events (recorded on the null stream around the synchronous call; best of ``--reps`` after one
dropped round that allocates).  ``rows_bytes`` is what the rows kernel must read and write at least: five planes and two gain rows
per member, the averaged planes and the masks; its own time comes from a kernel trace, not from this tool.
``--host-groups N`` also runs the float64 NumPy restatement (tests/delay_coherent_ref.py) for the first N groups on ``--host-threads``
threads and scales the wall time by the MEMBERS those groups hold to all members (labelled as scaled).  Prints one JSON object;
``--out`` also writes it to a file."""
import argparse
import concurrent.futures
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from delay_fringe_time import slices_of  # noqa: E402
from fit_errors_time import Events  # noqa: E402


def redundant_groups(p, antpos, tol=0.1):
    """(rows of every group, conjugation flags, lengths): the baselines of ``p`` with the same vector up to sign."""
    vec = antpos[p.bl_ant1] - antpos[p.bl_ant0]
    key = np.round(vec[:, :2] / tol).astype(np.int64)
    flip = (key[:, 0] < 0) | ((key[:, 0] == 0) & (key[:, 1] < 0))
    key[flip] = -key[flip]
    _, inv = np.unique(key, axis=0, return_inverse=True)
    inv = np.asarray(inv).ravel()
    order = np.argsort(inv, kind="stable")
    cuts = np.flatnonzero(np.diff(inv[order])) + 1
    rows = np.split(order.astype(np.int32), cuts)
    return rows, [flip[r].astype(np.uint8) for r in rows], np.asarray([np.linalg.norm(vec[r[0]]) for r in rows])


def member_lists(rows, conj, nb, T):
    sizes = np.repeat([len(r) for r in rows], T)
    member_row = np.concatenate([t * nb + r for r in rows for t in range(T)]).astype(np.int32)
    member_conj = np.concatenate([c for c in conj for _ in range(T)]).astype(np.uint8)
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), member_row, member_conj


def measure(sub, params, nb, T, nrates, dtype, layout, reps, ev, op, norm_f, nbins, groups):
    from calamity_amd import _lib, modeling
    from calamity_amd.solver import HipFitSolver

    rows, conj, lengths = groups
    s = HipFitSolver(dtype=dtype)
    s.set_problem(sub, layout=layout)
    s.set_data(sub.data_r, sub.data_i, sub.wgts)
    s.set_params(params["g_r"], params["g_i"], params["c_r"], params["c_i"])
    nd, ng = op.shape[1], len(rows)
    op_r, op_i = (np.ascontiguousarray(a, dtype=dtype) for a in (op.real, op.imag))
    set_ptr, member_row, member_conj = member_lists(rows, conj, nb, T)
    frows = np.ascontiguousarray(np.stack([t * nb + np.arange(nb) for t in range(T)], axis=1), dtype=np.int32)
    opt = modeling.fringe_rate_transform(T, 10.7)[0][:, :nrates]
    opt_r, opt_i = np.ascontiguousarray(opt.real), np.ascontiguousarray(opt.imag)
    cbins = np.minimum((lengths / (lengths.max() + 1e-9) * nbins).astype(np.int32), nbins - 1)
    fbins = (np.arange(nb) % nbins).astype(np.int32)
    k_bin, kc_bin, norm_k = np.empty((3, nbins, nrates, nd)), np.empty(nbins), np.empty(ng)
    f_bin, fc_bin, norm_f_grp = np.empty((3, nbins, nrates, nd)), np.empty(nbins), np.empty(nb)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    dk = _lib.DelayCoherentDesc(nd, 7, 1, ng, T, nrates, set_ptr.ctypes.data, member_row.ctypes.data, None, member_conj.ctypes.data, 1, None, nbins,
                                cbins.ctypes.data, op_r.ctypes.data, op_i.ctypes.data, norm_f.ctypes.data, opt_r.ctypes.data, opt_i.ctypes.data, len(member_row))
    df = _lib.DelayFringeDesc(nd, 7, 1, nb, T, nrates, frows.ctypes.data, None, nbins, fbins.ctypes.data, op_r.ctypes.data, op_i.ctypes.data, norm_f.ctypes.data,
                              opt_r.ctypes.data, opt_i.ctypes.data)
    forms = {"delay_coherent_spectrum": lambda: _lib.check(s._lib.cal_solver_delay_coherent_spectrum(s._h, C.byref(dk), None, None, None, ptr(norm_k), ptr(k_bin),
                                                                                                      ptr(kc_bin))),
             "delay_fringe_spectrum": lambda: _lib.check(s._lib.cal_solver_delay_fringe_spectrum(s._h, C.byref(df), None, None, None, ptr(norm_f_grp), ptr(f_bin),
                                                                                                  ptr(fc_bin)))}
    ms = {k: [] for k in forms}
    for _ in range(reps + 1):  # (the first round allocates: dropped)
        for k, fn in forms.items():
            ms[k].append(ev.time_ms(fn)[0])
    best = {k: min(v[1:]) for k, v in ms.items()}
    size = np.dtype(dtype).itemsize
    fpad = -(-sub.nfreqs // 8) * 8
    xpitch = -(-fpad // 32) * 32
    rows_bytes = len(member_row) * fpad * size * (5 + 2 * 2) + ng * T * xpitch * (3 * 2 * size + 1)
    kcount, fcount = np.where(kc_bin > 0, kc_bin, 1.0)[None, :, None, None], np.where(fc_bin > 0, fc_bin, 1.0)[None, :, None, None]
    out = dict(layout=layout, ngroups=int(ng), nmembers=int(len(member_row)), largest_group=int(max(len(r) for r in rows)), ntimes=T, nrates=nrates,
               ms_best={k: round(v, 3) for k, v in best.items()}, ms_all={k: [round(x, 3) for x in v[1:]] for k, v in ms.items()},
               coherent_over_fringe=round(best["delay_coherent_spectrum"] / best["delay_fringe_spectrum"], 3), rows_bytes=int(rows_bytes),
               transform_flops={"delay_coherent_spectrum": 3 * 8.0 * T * ng * sub.nfreqs * nd, "delay_fringe_spectrum": 3 * 8.0 * T * nb * sub.nfreqs * nd},
               groups_counted=float(kc_bin.sum()),
               # solver units, residual, mean over bins and delays per rate: the average of N members against the mean of their powers
               resid_mean_per_rate={"coherent": [float(v) for v in (k_bin / kcount)[2].mean(axis=(0, 2))],
                                    "fringe": [float(v) for v in (f_bin / fcount)[2].mean(axis=(0, 2))]}, memory_bytes=int(s.memory_bytes()))
    s.close()
    return out


def host_route(sub, params, p0, nb, T, nrates, dtype, op, norm_f, groups, ngroups, threads):
    """Wall time of the restatement for the first ``ngroups`` groups on ``threads`` threads (one group per task), scaled by members to
    all groups.  The inputs of those groups' rows -- data, weights, G and the model rows ``A c`` -- are formed before the clock starts."""
    from calamity_amd import modeling
    from delay_coherent_ref import restated

    rows, conj, _ = groups
    ngroups = min(ngroups, len(rows))
    used = np.unique(np.concatenate(rows[:ngroups]))
    where = {int(b): i for i, b in enumerate(used)}
    nu = len(used)
    sel = np.concatenate([t * nb + used for t in range(T)])
    cast = lambda a: np.asarray(a).astype(dtype).astype(np.float64)  # noqa: E731
    d = cast(sub.data_r[sel]) + 1j * cast(sub.data_i[sel])
    w = cast(sub.wgts[sel])
    na, nc, F = p0.nants, p0.ncoeffs, p0.nfreqs
    m = np.empty((T * nu, F), dtype=np.complex128)
    grp_of = np.repeat(np.arange(p0.ngrps), np.diff(p0.grp_bl_start))
    for t in range(T):
        c = cast(params["c_r"][t * nc : (t + 1) * nc]) + 1j * cast(params["c_i"][t * nc : (t + 1) * nc])
        for i, b in enumerate(used):
            g = grp_of[b]
            blk = cast(p0.basis[p0.grp_basis[g]][p0.bl_rowblk[b] * F : (p0.bl_rowblk[b] + 1) * F])
            m[t * nu + i] = blk @ c[p0.grp_coff[g] : p0.grp_coff[g + 1]]
    g = cast(params["g_r"]) + 1j * cast(params["g_i"])
    G = np.concatenate([g[t * na + p0.bl_ant0[used]] * np.conj(g[t * na + p0.bl_ant1[used]]) for t in range(T)])
    op64 = op.astype(np.complex128)
    opt = modeling.fringe_rate_transform(T, 10.7)[0][:, :nrates]

    def one(k):
        local = np.asarray([where[int(b)] for b in rows[k]])
        set_ptr = np.arange(T + 1, dtype=np.int64) * len(local)
        member_row = np.concatenate([t * nu + local for t in range(T)])
        ref = restated(d, m, G, w, op64, norm_f, set_ptr, member_row, opt, member_conj=np.tile(conj[k], T), weighting=1, calibrated=True)
        return float(ref["per_group"]["resid"].sum())

    t0 = time.perf_counter()
    with concurrent.futures.ThreadPoolExecutor(max_workers=threads) as pool:
        total = sum(pool.map(one, range(ngroups)))
    wall = time.perf_counter() - t0
    run, everything = sum(len(r) for r in rows[:ngroups]), sum(len(r) for r in rows)
    return dict(groups_run=int(ngroups), members_run=int(run * T), threads=threads, wall_s=round(wall, 3),
                scaled_to_all_members_s=round(wall * everything / run, 1), checksum=total,
                note="scaled linearly by members from groups_run to all groups: not a measurement of the whole")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="hera350")
    ap.add_argument("--dtype", default="f32")
    ap.add_argument("--layouts", default="shared")
    ap.add_argument("--slices", type=int, default=8)
    ap.add_argument("--rates", type=int, default=8)
    ap.add_argument("--ndelays", type=int, default=1024)
    ap.add_argument("--nbins", type=int, default=64)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--host-groups", type=int, default=0)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from calamity_amd import _lib, modeling, synthetic

    _lib.load()
    dtype = np.float32 if args.dtype == "f32" else np.float64
    p, truth, start = synthetic.make_config(args.config)
    full, norm_f, _ = modeling.delay_transform(150e6 + 100e3 * np.arange(p.nfreqs))
    lo = (p.nfreqs - min(args.ndelays, p.nfreqs)) // 2
    op = np.ascontiguousarray(full[:, lo : lo + min(args.ndelays, p.nfreqs)])
    norm_f = np.ascontiguousarray(norm_f, dtype=np.float64)
    T, nrates = args.slices, min(args.rates, args.slices)
    groups = redundant_groups(p, np.asarray(truth["antpos"], dtype=np.float64))
    sub, params = slices_of(p, start, T, dtype)
    ev = Events() if args.layouts else None  # (--layouts "": the host route alone)
    result = dict(workload=f"{args.config} x {T} slices, {args.dtype}, {op.shape[1]} delays, {nrates} rates, {len(groups[0])} redundant groups",
                  nants=p.nants, nbls=p.nbls, nfreqs=p.nfreqs, reps=args.reps,
                  runs=[measure(sub, params, p.nbls, T, nrates, dtype, layout, args.reps, ev, op, norm_f, args.nbins, groups)
                        for layout in args.layouts.split(",") if layout])
    if args.host_groups > 0:
        result["host"] = host_route(sub, params, p, p.nbls, T, nrates, dtype, op, norm_f, groups, args.host_groups, args.host_threads)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
