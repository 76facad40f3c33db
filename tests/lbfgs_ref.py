"""NumPy restatement of cal_solver_lbfgs (include/calamity_hip.h) for one time slice, on top of gauss_newton_ref.Ref.  Arithmetic in
float64 on inputs rounded to the solver's dtype ``T``; what the device stores in ``T`` is rounded here too (the variables, the gradient,
the direction, the pairs), so both follow the same statement:

    start      f_0, g_0.  f_0 not finite or |g_0| zero / not finite: status 3
    direction  no pair: d = -g_k, t = min(1, 1 / |g_k|).  Else the CLASSIC two-loop recursion on full vectors (the device runs it on the
               Gram matrix), gamma = s.y / y.y of the newest pair, t = 1.  slope = g_k . d; slope >= 0 or not finite: pairs dropped, d = -g_k
    search     at most max_ls trials round_T(x_k + t d); accept iff the loss is finite and <= f_k + c1 t slope, else t *= shrink.  None
               accepted: with pairs, drop them and search the same iteration again along -g_k; without, status 2 and x_k stays
    pair       s = round_T(x_{k+1} - x_k), y = round_T(g_{k+1} - g_k) enter the ring iff s.y is finite and > eps sqrt(s.s y.y)
    stop       status 1 once ftol > 0 and f_k - f_{k+1} <= ftol |f_k|; status 0 after nsteps iterations

The variables are the gains (complex [nants, nfreqs]) or, with a basis, y with gains = g0 + Bt (x) B y, and the coefficients unless
``freeze_model``.  The gradient with a basis follows the chain rule through B and Bt.  ``run`` also returns ``margin``: the smallest
relative margin of every discrete decision it took -- Armijo |f_trial - bound| / |f_k|, curvature |s.y / sqrt(s.s y.y) - eps|, with ftol
|(f_k - f_{k+1}) / |f_k| - ftol| -- which
a parity test asserts before it compares trajectories (a decision inside the device's rounding error may go either way)."""
import numpy as np


class LbfgsRef:
    def __init__(self, ref, dtype, g0=None, B=None, Bt=None, priors=None, freeze_model=False):
        """``ref``: gauss_newton_ref.Ref of the problem.  ``B`` [nfreqs, K]: frequency gain basis; ``Bt`` [ntimes, L]: time gain basis
        (antenna a at time t is row t * na + a); ``g0``: the gains the basis was attached at (complex [nants, nfreqs])."""
        self.ref, self.dtype, self.priors, self.freeze = ref, np.dtype(dtype), priors, bool(freeze_model)
        self.rnd = lambda a: np.asarray(a, dtype=np.float64).astype(self.dtype).astype(np.float64)  # noqa: E731
        self.B = None if B is None else self.rnd(B)
        self.Bt = None if Bt is None else self.rnd(Bt)
        self.g0 = g0
        self.basis = B is not None or Bt is not None

    # ---- the variables as one real vector: (gain variables re, im; coefficients re, im)
    def gains_of(self, v):
        """The full gains from the gain variables (y with a basis: rounded to T like the device's expanded gains)."""
        if not self.basis:
            return v
        z = v
        if self.Bt is not None:  # v: [na, L, W] -> [T na, W]
            z = np.einsum("tl,alw->taw", self.Bt, v).reshape(-1, v.shape[-1])
        if self.B is not None:
            z = z @ self.B.T
        g = self.g0 + z
        return self.rnd(g.real) + 1j * self.rnd(g.imag)

    def project(self, gg):
        """Chain rule: the gradient with respect to the gains onto the gain variables."""
        if self.B is not None:
            gg = gg @ self.B
        if self.Bt is not None:
            nt = self.Bt.shape[0]
            gg = np.einsum("tl,taw->alw", self.Bt, gg.reshape(nt, -1, gg.shape[-1]))
        return gg

    def pack(self, v, c):
        parts = [v.real.ravel(), v.imag.ravel()]
        if not self.freeze:
            parts += [c.real, c.imag]
        return np.concatenate(parts)

    def unpack(self, x, v_shape, c0):
        n = int(np.prod(v_shape))
        v = (x[:n] + 1j * x[n : 2 * n]).reshape(v_shape)
        if self.freeze:
            return v, c0
        nc = c0.size
        return v, x[2 * n : 2 * n + nc] + 1j * x[2 * n + nc :]

    def loss(self, v, c):
        return self.ref.loss(self.gains_of(v), c, self.priors)

    def loss_and_grad(self, v, c):
        r = self.ref
        g = self.gains_of(v)
        m = r.model(c)
        mod = g[r.i] * np.conj(g[r.j]) * m
        u = -2.0 * r.w * (r.d - mod)
        f = float(np.sum(r.w * np.abs(r.d - mod) ** 2))
        if self.priors is not None:
            a = (np.sum(mod.real * r.w) - self.priors[0]) + 1j * (np.sum(mod.imag * r.w) - self.priors[1])
            f += abs(a) ** 2
            u = u + 2.0 * r.w * a
        gg, gc = r.jhvp(g, c, u, m)
        return f, self.rnd(self.pack(self.project(gg), gc))  # (the device's gradient is held in T)

    def run(self, v, c, nsteps, history=8, max_ls=20, c1=1e-4, shrink=0.5, ftol=0.0, curvature_eps=1e-8):
        """``v``: the gain variables (the gains, or y), ``c``: the coefficients, both complex and already rounded to T.  Returns
        dict(v, c, losses [nsteps + 1] (NaN past iters), iters, evals, pairs_dropped, status, margin, margins: per iteration, stored: per
        iteration whether its pair entered the ring)."""
        rnd, v_shape = self.rnd, v.shape
        x = self.pack(v, c)
        f, g = self.loss_and_grad(v, c)
        losses = np.full(nsteps + 1, np.nan)
        out = dict(v=v, c=c, losses=losses, iters=0, evals=0, pairs_dropped=0, status=3, margin=np.inf, margins=[], stored=[])
        gn = float(np.sqrt(g @ g))
        if not np.isfinite(f) or not np.isfinite(gn) or gn == 0.0:
            return out
        losses[0] = f
        pairs = []  # (s, y), oldest first
        status = 0
        for _ in range(nsteps):
            accepted = False
            out["margins"].append(np.inf)
            while True:
                if pairs:
                    q = g.copy()
                    alphas = []
                    for s, y in reversed(pairs):
                        a = (s @ q) / (s @ y)
                        alphas.append(a)
                        q = q - a * y
                    s, y = pairs[-1]
                    q = q * ((s @ y) / (y @ y))
                    for (s, y), a in zip(pairs, reversed(alphas)):
                        q = q + s * (a - (y @ q) / (s @ y))
                    d, t = -q, 1.0
                    slope = float(g @ d)
                    if not np.isfinite(slope) or slope >= 0.0:
                        out["pairs_dropped"] += len(pairs)
                        pairs = []
                        continue
                    d = rnd(d)
                else:
                    d, slope = -g, -float(g @ g)
                    t = min(1.0, 1.0 / float(np.sqrt(g @ g)))
                for _trial in range(max_ls):
                    xt = rnd(x + t * d)
                    vt, ct = self.unpack(xt, v_shape, c)
                    ft = self.loss(vt, ct)
                    out["evals"] += 1
                    bound = f + c1 * t * slope
                    if np.isfinite(ft):
                        out["margins"][-1] = min(out["margins"][-1], abs(ft - bound) / abs(f))
                    if np.isfinite(ft) and ft <= bound:
                        accepted = True
                        break
                    t *= shrink
                if accepted or not pairs:
                    break
                out["pairs_dropped"] += len(pairs)
                pairs = []
            if not accepted:
                status = 2
                break
            fn, gnew = self.loss_and_grad(vt, ct)
            s, y = rnd(xt - x), rnd(gnew - g)
            sy, ss, yy = float(s @ y), float(s @ s), float(y @ y)
            if ss > 0 and yy > 0:
                out["margins"][-1] = min(out["margins"][-1], abs(sy / np.sqrt(ss * yy) - curvature_eps))
            out["stored"].append(bool(np.isfinite(sy) and sy > curvature_eps * np.sqrt(ss * yy)))
            if out["stored"][-1]:
                pairs.append((s, y))
                pairs = pairs[-history:]
            else:
                out["pairs_dropped"] += 1
            fk, f, x, g, v, c = f, fn, xt, gnew, vt, ct
            out["iters"] += 1
            losses[out["iters"]] = f
            if ftol > 0.0:
                out["margins"][-1] = min(out["margins"][-1], abs((fk - f) / abs(fk) - ftol))
            if ftol > 0.0 and fk - f <= ftol * abs(fk):
                status = 1
                break
        out.update(v=v, c=c, status=status, margin=min(out["margins"], default=np.inf))
        return out


def two_loop(pairs, g):
    """The classic two-loop recursion: d = -H g for pairs [(s, y)] oldest first."""
    q = np.array(g, dtype=np.float64)
    alphas = []
    for s, y in reversed(pairs):
        a = (s @ q) / (s @ y)
        alphas.append(a)
        q = q - a * y
    if pairs:
        s, y = pairs[-1]
        q = q * ((s @ y) / (y @ y))
    for (s, y), a in zip(pairs, reversed(alphas)):
        q = q + s * (a - (y @ q) / (s @ y))
    return -q
