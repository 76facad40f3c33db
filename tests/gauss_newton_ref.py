"""NumPy restatement of cal_solver_normal_product / cal_solver_gauss_newton_step (include/calamity_hip.h), shared by the
Gauss-Newton tests.  Everything in float64 and complex128, one time slice:

    G = g_i conj(g_j),  m = A c,  r = d - G m
    (J p)[b][f] = (dg_i conj(g_j) + g_i conj(dg_j)) m + G (A dc)            autocorrelation rows by the same formula
    J^H y:  gains  i: += y conj(m) g_j,   j: += conj(y) m g_i;   coefficients: A^T (conj(G) y)
    N p = J^H W J p,   rhs = J^H W r         (minus half the chi-square gradient differences)
    D_g[a][f] = sum over the cross-correlations of a of w |m|^2 |g_other|^2,   D_c[k in gamma] = sum_{b in gamma} mean_f w |G|^2
    (entries <= 0 or non-finite become 1)

``step`` solves (N + lam D) p = rhs by at most ``ncg`` iterations of conjugate gradients preconditioned with D from p = 0, forms the
trial parameters g + dg, c + dc and accepts them iff their loss (with the "sum" regulariser when priors are given) is finite and
strictly below the loss before.  The inner product is the real one of the (re, im) planes: Re sum conj(a) b."""
import numpy as np


class Ref:
    def __init__(self, p, data=None, dtype=np.float64):
        """``p``: a FitProblem; ``data``: (data_r, data_i, wgts) instead of the problem's; ``dtype``: inputs are rounded to it first
        (what a solver of that dtype holds), the arithmetic stays float64."""
        self.p = p
        self.cast = lambda a: np.asarray(a).astype(dtype).astype(np.float64)  # noqa: E731
        d_r, d_i, w = (self.cast(a) for a in (data if data is not None else (p.data_r, p.data_i, p.wgts)))
        self.d, self.w = d_r + 1j * d_i, w
        self.i, self.j = np.asarray(p.bl_ant0), np.asarray(p.bl_ant1)
        self.coff = np.asarray(p.grp_coff)
        self.blocks = [self.cast(b) for b in p.basis]

    def _rows(self, b, grp):
        blk = self.blocks[self.p.grp_basis[grp]]
        return blk[self.p.bl_rowblk[b] * self.p.nfreqs : (self.p.bl_rowblk[b] + 1) * self.p.nfreqs]

    def model(self, c):
        p = self.p
        m = np.empty((p.nbls, p.nfreqs), dtype=np.complex128)
        for grp in range(p.ngrps):
            for b in range(p.grp_bl_start[grp], p.grp_bl_start[grp + 1]):
                m[b] = self._rows(b, grp) @ c[self.coff[grp] : self.coff[grp + 1]]
        return m

    def model_adjoint(self, u):
        p = self.p
        out = np.zeros(p.ncoeffs, dtype=np.complex128)
        for grp in range(p.ngrps):
            for b in range(p.grp_bl_start[grp], p.grp_bl_start[grp + 1]):
                out[self.coff[grp] : self.coff[grp + 1]] += self._rows(b, grp).T @ u[b]
        return out

    def jvp(self, g, c, dg, dc, m=None):
        m = self.model(c) if m is None else m
        i, j = self.i, self.j
        return (dg[i] * np.conj(g[j]) + g[i] * np.conj(dg[j])) * m + g[i] * np.conj(g[j]) * self.model(dc)

    def jhvp(self, g, c, y, m=None):
        """J^H y: (gains [nants, nfreqs], coefficients [ncoeffs])."""
        m = self.model(c) if m is None else m
        i, j = self.i, self.j
        out = np.zeros_like(g)
        np.add.at(out, i, y * np.conj(m) * g[j])
        np.add.at(out, j, np.conj(y) * m * g[i])
        return out, self.model_adjoint(np.conj(g[i] * np.conj(g[j])) * y)

    def normal_product(self, g, c, dg, dc):
        m = self.model(c)
        return self.jhvp(g, c, self.w * self.jvp(g, c, dg, dc, m), m)

    def rhs(self, g, c):
        m = self.model(c)
        return self.jhvp(g, c, self.w * (self.d - g[self.i] * np.conj(g[self.j]) * m), m)

    def precond(self, g, c):
        p = self.p
        m = self.model(c)
        i, j = self.i, self.j
        q = self.w * np.abs(m) ** 2
        cross = i != j
        d_g = np.zeros((p.nants, p.nfreqs))
        np.add.at(d_g, i[cross], (q * np.abs(g[j]) ** 2)[cross])
        np.add.at(d_g, j[cross], (q * np.abs(g[i]) ** 2)[cross])
        rows = np.sum(self.w * np.abs(g[i] * np.conj(g[j])) ** 2, axis=1) / p.nfreqs
        d_c = np.zeros(p.ncoeffs)
        for grp in range(p.ngrps):
            d_c[self.coff[grp] : self.coff[grp + 1]] = np.sum(rows[p.grp_bl_start[grp] : p.grp_bl_start[grp + 1]])
        fix = lambda a: np.where(np.isfinite(a) & (a > 0), a, 1.0)  # noqa: E731
        return fix(d_g), fix(d_c)

    def loss(self, g, c, priors=None):
        mod = g[self.i] * np.conj(g[self.j]) * self.model(c)
        out = float(np.sum(self.w * np.abs(self.d - mod) ** 2))
        if priors is not None:
            out += (np.sum(mod.real * self.w) - priors[0]) ** 2 + (np.sum(mod.imag * self.w) - priors[1]) ** 2
        return out

    def step(self, g, c, lam=1e-3, ncg=20, cg_tol=1e-3, priors=None):
        """One damped Gauss-Newton step.  Returns dict(g, c, dg, dc, loss_before, loss_after, accepted, cg_iters, cg_residual, rz0,
        residuals); ``g``, ``c`` are the inputs where the step is rejected.  ``residuals[k]`` is the relative preconditioned residual
        sqrt(rz / rz0) after iteration k + 1 (``cg_iters`` entries), ``rz0`` the first res . z."""
        dot = lambda a, b: float(np.sum(a[0].real * b[0].real + a[0].imag * b[0].imag) + np.sum(a[1].real * b[1].real + a[1].imag * b[1].imag))  # noqa: E731
        rhs, D = self.rhs(g, c), self.precond(g, c)
        x = [np.zeros_like(g), np.zeros_like(c)]
        res = [rhs[0].copy(), rhs[1].copy()]
        z = [res[0] / D[0], res[1] / D[1]]
        s = [z[0].copy(), z[1].copy()]
        rz = rz0 = dot(res, z)
        iters, resid, trace = 0, 0.0, []
        if rz0 > 0 and np.isfinite(rz0):
            resid = 1.0
            for _ in range(ncg):
                Ns = self.normal_product(g, c, s[0], s[1])
                Ns = [Ns[0] + lam * D[0] * s[0], Ns[1] + lam * D[1] * s[1]]
                sNs = dot(s, Ns)
                if not (sNs > 0 and np.isfinite(sNs)):
                    break
                alpha = rz / sNs
                for k in range(2):
                    x[k] += alpha * s[k]
                    res[k] -= alpha * Ns[k]
                    z[k] = res[k] / D[k]
                rz_new = dot(res, z)
                iters += 1
                resid = float(np.sqrt(rz_new / rz0))
                trace.append(resid)
                if not np.isfinite(rz_new) or resid <= cg_tol:
                    break
                beta = rz_new / rz
                rz = rz_new
                for k in range(2):
                    s[k] = z[k] + beta * s[k]
        before = self.loss(g, c, priors)
        after = self.loss(g + x[0], c + x[1], priors)
        ok = bool(np.isfinite(after) and after < before)
        return dict(g=g + x[0] if ok else g, c=c + x[1] if ok else c, dg=x[0], dc=x[1], loss_before=before, loss_after=after, accepted=ok,
                    cg_iters=iters, cg_residual=resid, rz0=rz0, residuals=tuple(trace))


def dense_normal_matrix(ref, g, c):
    """The real (2 nants nfreqs + 2 ncoeffs)-square matrix J^T W J built column by column from ``jvp`` (small problems only), over
    the variables (g_r, g_i, c_r, c_i) flattened in that order."""
    p = ref.p
    ng, nc = p.nants * p.nfreqs, p.ncoeffs
    n = 2 * ng + 2 * nc
    m = ref.model(c)
    J = np.empty((2 * p.nbls * p.nfreqs, n))
    for k in range(n):
        e = np.zeros(n)
        e[k] = 1.0
        dg = (e[:ng] + 1j * e[ng : 2 * ng]).reshape(p.nants, p.nfreqs)
        dc = e[2 * ng : 2 * ng + nc] + 1j * e[2 * ng + nc :]
        col = ref.jvp(g, c, dg, dc, m)
        J[:, k] = np.concatenate([col.real.ravel(), col.imag.ravel()])
    w2 = np.concatenate([ref.w.ravel(), ref.w.ravel()])
    return J.T @ (w2[:, None] * J)


def flatten(vg, vc):
    return np.concatenate([vg.real.ravel(), vg.imag.ravel(), vc.real, vc.imag])
