#!/usr/bin/env python3
"""What cal_solver_gain_basis_errors costs at HERA-350 (350 antennas, 61 075 baselines x 1024 channels), SHARED layout, beside the host
route on the same planes, for the three basis configurations:

  freq        the DPSS basis of ``--gain_max_dly`` ns (100 ns: K = 30), one time
  time_freq   the same with a [T, L] time basis (the Q of a QR of a seeded normal matrix, L = ``--time_nvec`` = 8) over ``--ntimes`` = 8
              jointly fitted times: n = L K = 240 unknowns per antenna
  time        the time basis alone: L x L systems per (antenna, channel)

Every call is timed with the host clock around the synchronous call (it ends in the download of its outputs behind a stream
synchronise); best of ``--reps`` after one dropped round that allocates.  Two forms go through the C interface: without outputs (the
model pass, the antenna walk, the Gram and Kronecker kernels, the factorisation and W = L^-1) and with gain_var as well
(gain_error_var_kernel and the download of [nants, nfreqs] doubles); their difference bounds the kernel's time from above, and
``useful_flops`` = nants nfreqs n^2 (the lower triangle of W: half of a full product's 2 n^2) over it is a lower bound of its rate.
The host route: ``den`` read back (1 / gain_var of cal_solver_fit_errors before the bases are attached, the same device pass), then per
antenna the dense N, its inverse and b^T N^-1 b in NumPy with the cores this process may use.  Prints one JSON object and a table;
``--out`` also writes the JSON to a file."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MATRIX_PEAK = {"f32": 157.3e12, "f64": 78.6e12}  # v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64, flop/s


def host_route(den, Bt, B, ridge):
    """gain_var by the dense inverse per system, as tests/gain_basis_errors_ref.py does it."""
    rows, F = den.shape
    out = np.zeros((rows, F))
    T = 1 if Bt is None else Bt.shape[0]
    na = rows // T
    if B is None:  # every (antenna, channel) at once
        d = den.reshape(T, na, F)
        N = np.einsum("tl,tm,taf->aflm", Bt, Bt, d)
        tr = np.trace(N, axis1=2, axis2=3)
        ok = tr > 0
        L = Bt.shape[1]
        Nr = N + (ridge * tr / L)[..., None, None] * np.eye(L)
        Nr[~ok] = np.eye(L)
        Cinv = np.linalg.inv(Nr)
        var = np.einsum("tl,aflm,tm->taf", Bt, Cinv, Bt) * ok[None]
        return var.reshape(rows, F)
    X = B if Bt is None else np.kron(Bt, B)
    n = X.shape[1]
    for a in range(na):
        d = den[a::na].reshape(-1)
        N = X.T @ (d[:, None] * X)
        tr = np.trace(N)
        if not tr > 0:
            continue
        Cinv = np.linalg.inv(N + ridge * (tr / n) * np.eye(n))
        out[a::na] = np.einsum("ik,ik->i", X @ Cinv, X).reshape(T, F)
    return out


def best_ms(fn, reps):
    secs = []
    for _ in range(reps + 1):  # (the first round allocates: dropped)
        t0 = time.perf_counter()
        out = fn()
        secs.append(time.perf_counter() - t0)
    return 1e3 * min(secs[1:]), out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="hera350")
    ap.add_argument("--dtype", default="f32")
    ap.add_argument("--cases", default="freq,time_freq,time")
    ap.add_argument("--ntimes", type=int, default=8)
    ap.add_argument("--time_nvec", type=int, default=8)
    ap.add_argument("--gain_max_dly", type=float, default=100.0)
    ap.add_argument("--ridge", type=float, default=1e-6)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from calamity_amd import _lib, modeling, synthetic
    from calamity_amd.batched import replicate_slices
    from calamity_amd.solver import HipFitSolver
    from calamity_amd.utils import usable_cores

    dtype = np.float32 if args.dtype == "f32" else np.float64
    p, truth, start = synthetic.make_config(args.config)
    B = np.array(modeling.gain_dpss_basis(np.asarray(truth["freqs"], dtype=np.float64), args.gain_max_dly))
    Bt = np.ascontiguousarray(np.linalg.qr(np.random.default_rng(1).standard_normal((args.ntimes, args.time_nvec)))[0])
    rows = []
    for case in args.cases.split(","):
        T = 1 if case == "freq" else args.ntimes
        big = p
        if T > 1:
            big, _, _ = replicate_slices(p, T)
            big.nslices = 1  # one fit: distributed.batch_time_slices(per_slice=False)
        tile = lambda a: np.tile(np.asarray(a, dtype=dtype), (T,) + (1,) * (np.ndim(a) - 1))  # noqa: E731
        s = HipFitSolver(dtype=dtype)
        s.set_problem(big, layout="shared")
        s.set_data(tile(p.data_r), tile(p.data_i), tile(p.wgts))
        s.set_params(tile(start["g_r"]), tile(start["g_i"]), tile(truth["c"].real), tile(truth["c"].imag))
        read_ms, gv = best_ms(lambda: s.fit_errors(model_var=False, coeffs=False)["gain_var"], 1)
        den = np.divide(1.0, gv, out=np.zeros_like(gv), where=gv > 0)
        cb, ct = (B if case != "time" else None), (Bt if case != "freq" else None)
        if cb is not None:
            s.set_gain_basis(cb)
        if ct is not None:
            s.set_gain_time_basis(ct)
        cnt = _lib.FitErrorsCounts()
        none_ms, _ = best_ms(lambda: _lib.check(s._lib.cal_solver_gain_basis_errors(s._h, args.ridge, None, None, None, C.byref(cnt))), args.reps)
        gain_var = np.empty((big.nants, big.nfreqs))
        var_ms, _ = best_ms(lambda: _lib.check(s._lib.cal_solver_gain_basis_errors(s._h, args.ridge, gain_var.ctypes.data, None, None, C.byref(cnt))), args.reps)
        all_ms, out = best_ms(lambda: s.gain_basis_errors(ridge=args.ridge), args.reps)
        mem = s.memory_bytes()
        s.close()
        cast = lambda a: None if a is None else a.astype(dtype).astype(np.float64)  # noqa: E731
        t0 = time.perf_counter()
        want = host_route(den, cast(ct), cast(cb), args.ridge)
        host_ms = 1e3 * (time.perf_counter() - t0)
        n = (1 if ct is None else ct.shape[1]) * (0 if cb is None else cb.shape[1])
        flops = float(big.nants) * big.nfreqs * n * n
        row = dict(case=case, dtype=args.dtype, ntimes=T, nants=big.nants, nbls=big.nbls, nfreqs=big.nfreqs, unknowns=n or ct.shape[1],
                   nsolved=out["nsolved"], nsingular=out["nsingular"], device_ms=dict(no_outputs=round(none_ms, 3), with_gain_var=round(var_ms, 3),
                                                                                      all_outputs=round(all_ms, 3)),
                   host_ms=dict(planes_read_back=round(read_ms, 3), numpy=round(host_ms, 3)), host_over_device=round((read_ms + host_ms) / all_ms, 2),
                   parity=float(np.max(np.abs(out["gain_var"] - want)) / np.max(np.abs(want))), memory_bytes=int(mem))
        if n:
            row.update(useful_flops=flops, var_kernel_ms_at_most=round(var_ms - none_ms, 3),
                       var_kernel_share_of_matrix_peak_at_least=round(flops / (1e-3 * max(var_ms - none_ms, 1e-6)) / MATRIX_PEAK[args.dtype], 4))
        rows.append(row)
    result = dict(device=_lib.device_info(0)["name"], host_cores=usable_cores(), reps=args.reps, ridge=args.ridge, rows=rows)
    text = json.dumps(result, indent=1)
    print(text)
    print("| case | dtype | unknowns | no outputs ms | + gain_var ms | all outputs ms | host: planes + NumPy ms | host / device | parity |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['case']} | {r['dtype']} | {r['unknowns']} | {r['device_ms']['no_outputs']} | {r['device_ms']['with_gain_var']} | {r['device_ms']['all_outputs']} | "
              f"{r['host_ms']['planes_read_back']} + {r['host_ms']['numpy']} | {r['host_over_device']} | {r['parity']:.1e} |")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
