#!/usr/bin/env python3
"""What cal_solver_fit_errors costs at HERA-350 (350 antennas, 61 075 baselines x 1024 channels, fp32), SHARED and STREAM layout in
one process, beside one cal_solver_solve_coeffs call of the same solver.

Every call is bracketed by two HIP events (recorded on the null stream around the synchronous call; best of ``--reps`` after one
dropped round that allocates).  Three forms of the call are timed through the C interface:
  coeff_var alone                  model pass, q, Gram, factorisation and W = L^-1   (the per-sample kernel is not launched)
  coeff_var, leverage_bl, nsamp_bl the same plus fit_error_leverage_kernel and the row sums
  the above and gain_var           plus the second model pass and the antenna walk
The difference of the first two is the leverage kernel's share.  It issues F sum nvec^2 flops (the lower triangle of W: half of the
2 F sum nvec^2 of a full product), half of coeff_gram_kernel's count.  Prints one JSON object; ``--out`` also writes it to a file."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class Events:
    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        self.a, self.b = C.c_void_p(), C.c_void_p()
        for e in (self.a, self.b):
            assert self.hip.hipEventCreate(C.byref(e)) == 0

    def time_ms(self, fn):
        assert self.hip.hipEventRecord(self.a, None) == 0
        out = fn()
        assert self.hip.hipEventRecord(self.b, None) == 0 and self.hip.hipEventSynchronize(self.b) == 0
        ms = C.c_float()
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.a, self.b) == 0
        return float(ms.value), out


def measure(p, start, dtype, layout, reps, ev):
    from calamity_amd import _lib
    from calamity_amd.solver import HipFitSolver

    rng = np.random.default_rng(2)
    s = HipFitSolver(dtype=dtype)
    s.set_problem(p, layout=layout)
    s.set_params(1.0 + 0.05 * rng.standard_normal((p.nants, p.nfreqs)), 0.05 * rng.standard_normal((p.nants, p.nfreqs)), start["c_r"], start["c_i"])
    cv, lev, ns, gv = np.empty(p.ncoeffs), np.empty(p.nbls), np.empty(p.nbls), np.empty((p.nants, p.nfreqs))
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    cnt = _lib.FitErrorsCounts()

    def call(*outs):
        args = [ptr(a) if a is not None else None for a in outs]
        return lambda: _lib.check(s._lib.cal_solver_fit_errors(s._h, 1e-6, args[0], None, args[1], args[2], args[3], C.byref(cnt)))

    forms = {"coeff_var": call(cv, None, None, None), "coeff_var_leverage": call(cv, lev, ns, None), "all_but_model_var": call(cv, lev, ns, gv)}
    ms = {k: [] for k in list(forms) + ["solve_coeffs"]}
    for _ in range(reps + 1):  # (the first round allocates: dropped)
        for k, fn in forms.items():
            ms[k].append(ev.time_ms(fn)[0])
        s.set_params(c_r=start["c_r"], c_i=start["c_i"])
        ms["solve_coeffs"].append(ev.time_ms(s.solve_coeffs)[0])
    best = {k: min(v[1:]) for k, v in ms.items()}
    nvec2 = float(np.sum(np.asarray(p.grp_nvec, dtype=np.float64) ** 2))
    size = np.dtype(dtype).itemsize
    lev_ms = best["coeff_var_leverage"] - best["coeff_var"]
    out = dict(layout=layout, basis_folded=s.timing_get()["basis_folded"], nsolved=int(cnt.nsolved), nsingular=int(cnt.nsingular),
               ms_best={k: round(v, 3) for k, v in best.items()}, ms_all={k: [round(x, 3) for x in v[1:]] for k, v in ms.items()},
               leverage_kernel_ms=round(lev_ms, 3), leverage_share_of_call=round(lev_ms / best["all_but_model_var"], 3),
               call_over_solve_coeffs=round(best["all_but_model_var"] / best["solve_coeffs"], 3),
               leverage_flops=p.nfreqs * nvec2, leverage_tflops=p.nfreqs * nvec2 / (lev_ms * 1e-3) / 1e12 if lev_ms > 0 else None,
               # what the leverage kernel reads once: the tiles, W (padded to 16), q; what it writes: the partial sums
               leverage_bytes=dict(tiles=float(p.nfreqs) * float(np.sum(p.grp_nvec)) * size, w=float(np.sum(((np.asarray(p.grp_nvec, dtype=np.float64) + 15) // 16 * 16) ** 2)) * size, q=float(p.nbls) * p.nfreqs * size),
               mean_leverage=float(lev.sum() / max(1, cnt.nsolved)), memory_bytes=int(s.memory_bytes()))
    s.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="hera350")
    ap.add_argument("--dtype", default="f32")
    ap.add_argument("--layouts", default="shared,stream")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from calamity_amd import _lib, synthetic

    _lib.load()
    dtype = np.float32 if args.dtype == "f32" else np.float64
    p, _, start = synthetic.make_config(args.config)
    ev = Events()
    result = dict(workload=f"{args.config}, {args.dtype}", nants=p.nants, nbls=p.nbls, nfreqs=p.nfreqs, reps=args.reps,
                  runs=[measure(p, start, dtype, layout, args.reps, ev) for layout in args.layouts.split(",")])
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
