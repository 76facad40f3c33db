"""The folded form of the streaming kernel (fit_kernels.hpp: process_item, FOLD): a mirror-symmetric basis is kept and read as
its lower half band only.  Comparator: the fp64 C oracle (oracle/ref_c.c) on the FULL basis; bounds: the project's own (fp32
loss 1e-5, gradients 1e-4 relative; fp64 1e-10).  The unfolded kernel (kernel_path="general_full") runs beside it and has to
meet the same bounds; both paths' measured errors are printed side by side (DESIGN.md section 5 quotes them).

The C oracle evaluates loss and gradients.  The foreground model (MODE_MODEL) and the least-squares initialisation (MODE_INIT)
are linear maps it has no entry for: they are compared with their definition evaluated in fp64 by NumPy on the full basis,
A c and A^T (src [w != 0]) (calibration.py:1587-1590, :875-902), as vectors under the gradient bound.
"""
import numpy as np
import pytest

from calamity_amd import synthetic
from calamity_amd.problem import FitProblem

pytestmark = pytest.mark.gpu

TOL = {np.float32: (1e-5, 1e-4), np.float64: (1e-10, 1e-10)}


def relnorm(a, b):
    a = np.asarray(a, dtype=np.complex128 if np.iscomplexobj(a) else np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def model_and_init_reference(p, c_r, c_i, src_r, src_i):
    """fp64: A c per baseline, and A^T (src [w != 0]) per fitting group (one baseline per group)."""
    coff = p.grp_coff
    m = np.empty((p.nbls, p.nfreqs), dtype=np.complex128)
    c0 = np.empty(p.ncoeffs, dtype=np.complex128)
    msk = (~np.isclose(p.wgts, 0.0)).astype(np.float64)
    for u in range(len(p.basis)):
        bls = np.where(np.asarray(p.grp_basis) == u)[0]
        if len(bls) == 0:
            continue
        A = np.asarray(p.basis[u], dtype=np.float64)
        idx = coff[bls][None, :] + np.arange(A.shape[1])[:, None]
        m[bls] = (A @ c_r[idx]).T + 1j * (A @ c_i[idx]).T
        c0[idx] = A.T @ (src_r[bls] * msk[bls]).T + 1j * (A.T @ (src_i[bls] * msk[bls]).T)
    return m, c0


def measure(p, start, dtype, layout="stream", paths=("auto", "general_full"), expect_folded=True, regs=(False, True), rows=None):
    """Errors of every path against the oracle; asserts the bounds and the reported form.  Returns {(path, what): error}."""
    from calamity_amd.solver import HipFitSolver
    from oracle.ref_c import CRef

    tol_l, tol_g = TOL[dtype]
    c = CRef(p, np.float64, nthreads=16)
    ref_m, ref_c0 = model_and_init_reference(p, start["c_r"], start["c_i"], p.sky_r, p.sky_i)
    out = {}
    for path in paths:
        s = HipFitSolver(dtype=dtype)
        s.set_problem(p, layout=layout, kernel_path=path)
        folded = s.timing_get()["basis_folded"]
        assert folded == (1 if (expect_folded and path != "general_full") else 0), (path, folded)
        s.set_params(start["g_r"], start["g_i"], start["c_r"], start["c_i"])
        for reg in regs:
            pr, pi = (float(np.sum(p.sky_r * p.wgts)) * 0.9, float(np.sum(p.sky_i * p.wgts)) * 1.1) if reg else (0.0, 0.0)
            c.set_regularization("sum" if reg else None, pr, pi)
            ref = c.loss_grads(start["g_r"], start["g_i"], start["c_r"], start["c_i"])
            s.set_regularization("sum" if reg else None, pr, pi)
            tag = "sum" if reg else "none"
            out[(path, f"loss_only/{tag}")] = abs(s.eval_loss() - ref[0]) / abs(ref[0])
            got = s.eval_grads()
            out[(path, f"loss/{tag}")] = abs(got[0] - ref[0]) / abs(ref[0])
            for name, a, b in zip(("g_r", "g_i", "c_r", "c_i"), got[1:], ref[1:]):
                out[(path, f"{name}/{tag}")] = relnorm(a, b)
        s.set_regularization(None, 0.0, 0.0)
        m_r, m_i = s.model()
        out[(path, "model")] = relnorm(np.asarray(m_r, np.float64) + 1j * np.asarray(m_i, np.float64), ref_m)
        s.init_coeffs(p.sky_r, p.sky_i)
        _, _, ic_r, ic_i = s.get_params()
        out[(path, "init")] = relnorm(np.asarray(ic_r, np.float64) + 1j * np.asarray(ic_i, np.float64), ref_c0)
        s.close()
    whats = sorted({k[1] for k in out})
    for w in whats:
        line = "  ".join(f"{path}={out[(path, w)]:.3e}" for path in paths)
        print(f"{np.dtype(dtype).name} {w:14s} {line}")
        if rows is not None:
            rows[w] = {path: out[(path, w)] for path in paths}
    for (path, w), e in out.items():
        assert e <= (tol_l if w.startswith("loss") else tol_g), (path, w, e)
    return out


def test_hera350_fp32_stream_folded_and_full_meet_the_bounds():
    """Full hera350 size, fp32, stream layout: the default path folds, "general_full" does not, both meet the bounds for the loss,
    the gradients (with and without the "sum" regulariser), the model and the least-squares initialisation.

    Measured on MI355X (relative errors against the fp64 oracle, folded / unfolded; DESIGN.md section 5 holds the table):
    loss 4.12e-08 / 4.17e-08 (with the regulariser 4.15e-08 / 4.18e-08); gain gradient re 4.29e-07 / 4.29e-07, im 1.39e-07 /
    1.40e-07; coefficient gradient re 5.07e-07 / 5.14e-07, im 5.07e-07 / 5.13e-07; model 9.02e-08 / 9.02e-08; least-squares
    initialisation 5.99e-08 / 9.93e-08."""
    p, truth, start = synthetic.make_config("hera350", with_sky=True)
    rng = np.random.default_rng(2)
    start = dict(start)
    start["g_r"] = 1.0 + 0.05 * rng.standard_normal((p.nants, p.nfreqs))
    start["g_i"] = 0.05 * rng.standard_normal((p.nants, p.nfreqs))
    measure(p, start, np.float32)


# ---- small shapes ------------------------------------------------------------------------------------------------
def mirror_block(rng, nfreqs, nvec, exact=True):
    """[nfreqs][nvec] with A[F-1-f, k] = (-1)^k A[f, k] exactly (in fp64, hence also after a cast to fp32)."""
    half = rng.standard_normal((nfreqs // 2, nvec)) / np.sqrt(nfreqs)
    sign = np.where(np.arange(nvec) % 2 == 0, 1.0, -1.0)
    return np.ascontiguousarray(np.concatenate([half, half[::-1] * sign]))


def small_problem(blocks, grp_basis, nants=7, seed=0, nslices=1):
    """One baseline per fitting group; with nslices > 1 the groups are repeated slice by slice over disjoint antennas."""
    rng = np.random.default_rng(seed)
    nfreqs = blocks[0].shape[0]
    a0, a1, gb = [], [], []
    for t in range(nslices):
        for u in grp_basis:
            i, j = rng.choice(nants, size=2, replace=False)
            a0.append(t * nants + i)
            a1.append(t * nants + j)
            gb.append(u)
    nbls = len(a0)
    w = rng.uniform(0.0, 1.0, size=(nbls, nfreqs)) * (rng.random((nbls, nfreqs)) > 0.1)
    p = FitProblem(nants=nants * nslices, nfreqs=nfreqs, basis=list(blocks), grp_basis=np.asarray(gb, np.int32),
                   grp_bl_start=np.arange(nbls + 1, dtype=np.int32), bl_ant0=np.asarray(a0, np.int32), bl_ant1=np.asarray(a1, np.int32),
                   bl_rowblk=np.zeros(nbls, np.int32), data_r=rng.standard_normal((nbls, nfreqs)), data_i=rng.standard_normal((nbls, nfreqs)),
                   wgts=w / w.sum() * nslices)
    p.nslices = nslices
    p.sky_r, p.sky_i = rng.standard_normal((nbls, nfreqs)), rng.standard_normal((nbls, nfreqs))
    start = dict(g_r=1.0 + 0.1 * rng.standard_normal((p.nants, nfreqs)), g_i=0.1 * rng.standard_normal((p.nants, nfreqs)),
                 c_r=rng.standard_normal(p.ncoeffs), c_i=rng.standard_normal(p.ncoeffs))
    return p, start


# vectors per block that select each tile width: fp32 FB 128/64/32/16/8 and fp64 FB 64/32/16/8/4 (kTileBytes = 28 KB)
NVEC_PER_FB = [40, 100, 200, 400, 800]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_every_tile_width_folded_against_full_and_oracle(dtype):
    """One block per tile width (several baselines each, 1024 channels): more than 2 NS vectors, so the wide instance (L = 7)."""
    rng = np.random.default_rng(10)
    blocks = [mirror_block(rng, 1024, n) for n in NVEC_PER_FB]
    p, start = small_problem(blocks, [0, 1, 2, 3, 4] * 3, seed=11)
    measure(p, start, dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_narrow_instance_folded(dtype):
    """Blocks of at most 2 NS vectors run the L = 2 instance (loss / gradient passes): fp32 NS = 8 at FB 128, fp64 NS = 8 at FB 64."""
    rng = np.random.default_rng(12)
    blocks = [mirror_block(rng, 512, n) for n in (3, 16, 9)]
    p, start = small_problem(blocks, [0, 1, 2, 1, 0], seed=13)
    measure(p, start, dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_items_split_across_workgroups_folded(dtype):
    """Few groups with many tiles: the groups are cut along their (folded) tiles and the partial coefficient gradients summed."""
    rng = np.random.default_rng(14)
    blocks = [mirror_block(rng, 4096, 300), mirror_block(rng, 4096, 120)]
    p, start = small_problem(blocks, [0, 1, 0], seed=15)
    measure(p, start, dtype)


def test_band_shorter_than_the_row_padding_folded():
    """192 channels in rows padded to 256: the folded tiles cover the band, the padding stays untouched (zero gbar_G)."""
    rng = np.random.default_rng(16)
    blocks = [mirror_block(rng, 192, 150), mirror_block(rng, 192, 210)]  # fp32 FB 32: 96 = 3 tiles
    p, start = small_problem(blocks, [0, 1, 0, 1], seed=17)
    measure(p, start, np.float32)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_several_time_slices_without_shared_tiles_folded(dtype):
    rng = np.random.default_rng(18)
    blocks = [mirror_block(rng, 512, 60), mirror_block(rng, 512, 130)]
    p, start = small_problem(blocks, [0, 1, 1, 0], seed=19, nslices=3)
    from calamity_amd.solver import HipFitSolver

    got = {}
    for path in ("auto", "general_full"):
        s = HipFitSolver(dtype=dtype)
        s.set_problem(p, layout="stream", kernel_path=path)
        assert s.timing_get()["basis_folded"] == (1 if path == "auto" else 0)
        s.set_params(start["g_r"], start["g_i"], start["c_r"], start["c_i"])
        got[path] = s.eval_grads()
        sl = s.slice_losses()
        assert abs(np.sum(sl) - got[path][0]) <= 1e-12 * abs(got[path][0])
        s.close()
    # every slice is an independent fit: the oracle on each slice's own problem
    from oracle.ref_c import CRef

    tol_l, tol_g = TOL[dtype]
    na, nb = p.nants // 3, p.nbls // 3
    coff = p.grp_coff
    total = 0.0
    for t in range(3):
        bl = slice(t * nb, (t + 1) * nb)
        q = FitProblem(nants=na, nfreqs=p.nfreqs, basis=p.basis, grp_basis=p.grp_basis[bl], grp_bl_start=np.arange(nb + 1, dtype=np.int32),
                       bl_ant0=p.bl_ant0[bl] - t * na, bl_ant1=p.bl_ant1[bl] - t * na, bl_rowblk=p.bl_rowblk[bl], data_r=p.data_r[bl],
                       data_i=p.data_i[bl], wgts=p.wgts[bl])
        cs = slice(coff[t * nb], coff[(t + 1) * nb])
        ref = CRef(q, np.float64).loss_grads(start["g_r"][t * na:(t + 1) * na], start["g_i"][t * na:(t + 1) * na], start["c_r"][cs], start["c_i"][cs])
        total += ref[0]
        for path in got:
            g = got[path]
            assert relnorm(g[1][t * na:(t + 1) * na], ref[1]) <= tol_g and relnorm(g[2][t * na:(t + 1) * na], ref[2]) <= tol_g, (path, t)
            assert relnorm(g[3][cs], ref[3]) <= tol_g and relnorm(g[4][cs], ref[4]) <= tol_g, (path, t)
    for path in got:
        assert abs(got[path][0] - total) <= tol_l * abs(total), path


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_block_that_does_not_fold_keeps_the_whole_problem_unfolded(dtype):
    rng = np.random.default_rng(20)
    blocks = [mirror_block(rng, 512, 60), rng.standard_normal((512, 90)) / np.sqrt(512)]
    p, start = small_problem(blocks, [0, 1, 0, 1], seed=21)
    measure(p, start, dtype, expect_folded=False)


def test_fp64_dpss_blocks_stay_unfolded_and_fp32_ones_fold():
    """A basis of real DPSS blocks (symmetric to 1e-12, not exactly): fp64 keeps the full band, fp32 folds."""
    p, truth, start = synthetic.make_problem(8, 256, f0=150e6, df=400e3, seed=0, with_sky=True)
    measure(p, start, np.float64, expect_folded=False)
    measure(p, start, np.float32, expect_folded=True)


def test_shared_layout_is_never_folded():
    rng = np.random.default_rng(22)
    p, start = small_problem([mirror_block(rng, 512, 60)], [0, 0, 0], seed=23)
    measure(p, start, np.float32, layout="shared", paths=("general", "general_full"), expect_folded=False)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_folded_fit_is_bitwise_reproducible(dtype):
    """Two solvers, five steps each: equal bits in losses and parameters (fixed summation order, no atomics)."""
    from calamity_amd.solver import HipFitSolver

    rng = np.random.default_rng(24)
    blocks = [mirror_block(rng, 1024, n) for n in (40, 200, 300)]
    p, start = small_problem(blocks, [0, 1, 2, 1, 0, 2], seed=25)
    runs = []
    for _ in range(2):
        s = HipFitSolver(dtype=dtype)
        s.set_problem(p, layout="stream")
        assert s.timing_get()["basis_folded"] == 1
        s.set_params(start["g_r"], start["g_i"], start["c_r"], start["c_i"])
        s.set_regularization("sum", 0.3, -0.2)
        s.set_optimizer("Adam", learning_rate=1e-2)
        losses, _, _ = s.run(5, record=True, tol=0.0)
        runs.append((np.asarray(losses), *[np.asarray(a) for a in s.get_params()]))
        s.close()
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes()
