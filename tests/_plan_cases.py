"""Seeded problems that reach every branch of the set-up planner (calamity_amd/csrc/problem_plan.hpp), shared by
tests/test_plan_host.py and the recording of tests/golden/plan/.  Small on purpose: the shapes are the smallest at which the
planner takes each path; ``kernel_path`` forces the paths that AUTO would only take at size.

``CASES[name]() -> (FitProblem without data, dtype, layout, kernel_path)``."""
import numpy as np

from calamity_amd import modeling
from calamity_amd.batched import replicate_slices
from calamity_amd.problem import FitProblem


def _pairs(nants, n, base=0):
    i, j = np.triu_indices(nants, k=1)
    assert n <= len(i)
    return (i[:n] + base).astype(np.int32), (j[:n] + base).astype(np.int32)


def _problem(nants, nfreqs, basis, grp_basis, grp_nbl, a0, a1, rowblk=None, **kw):
    start = np.concatenate([[0], np.cumsum(grp_nbl)]).astype(np.int32)
    nbls = int(start[-1])
    return FitProblem(nants=nants, nfreqs=nfreqs, basis=basis, grp_basis=np.asarray(grp_basis, np.int32), grp_bl_start=start,
                      bl_ant0=np.asarray(a0, np.int32), bl_ant1=np.asarray(a1, np.int32),
                      bl_rowblk=np.zeros(nbls, np.int32) if rowblk is None else np.asarray(rowblk, np.int32),
                      data_r=None, data_i=None, wgts=None, **kw)


def _random_blocks(rng, nfreqs, nvecs, nrowblk=1):
    return [rng.standard_normal((nrowblk * nfreqs, k)) / np.sqrt(nfreqs) for k in nvecs]


def dpss_stream(nfreqs):
    """45 single-baseline groups (10 antennas) over DPSS blocks of five delays: tile widths 128, 64, 32 and (fp32, 256 channels)
    16 -- the widest block is cut into two items, so the groups' gradients are summed from partials."""
    freqs = 100e6 + 400e3 * np.arange(nfreqs)
    basis = [modeling.yield_dpss_model_comps_bl_grp(length, freqs) for length in (14.6, 70.0, 140.0, 280.0, 350.0)]
    a0, a1 = _pairs(10, 45)
    return _problem(10, nfreqs, basis, np.arange(45) % len(basis), np.ones(45, int), a0, a1)


def groups(seed=1):
    """Multi-baseline groups of 1 / 3 / 20 / 70 baselines over two row blocks, one of 300 baselines (more than kRunMax in a run)."""
    rng = np.random.default_rng(seed)
    nbl = [1, 3, 20, 70, 300]
    basis = _random_blocks(rng, 96, [5, 12, 30, 7, 9], nrowblk=2)
    n = sum(nbl)
    a0, a1 = _pairs(30, n)
    rowblk = np.concatenate([np.zeros(1, int), [0, 1, 1], np.repeat([0, 1, 0], [9, 6, 5]), np.repeat([1, 0], [40, 30]), np.repeat([0, 1], [290, 10])])
    return _problem(30, 96, basis, np.arange(5), nbl, a0, a1, rowblk)


def alias(nt, dtype, seed=2):
    """``nt`` time slices of 72 single-baseline groups that share tiles (bl_alias) on a 256-channel band: 66 head items for the
    matrix-core multi kernel (the XCD deal runs from 64), blocks wider than kMmMaxVec (230, 240 vectors) whose heads stay on
    fused_multi_kernel, one block wider than kMmMaxVecOnePass of the dtype.  With 10 slices two sets lose one member (its copy in
    the last slice owns its tiles): 9 baselines are two heads and a lone leftover on either kernel."""
    rng = np.random.default_rng(seed)
    wide = 224 if np.dtype(dtype) == np.float32 else 200  # on the matrix-core kernel, too wide for its one-pass form in fp64
    nvecs = [8, 20, 33, 56, 60, 100, wide, 230, 240]
    basis = _random_blocks(rng, 256, nvecs)
    ngrps = 72
    a0, a1 = _pairs(13, ngrps)
    grp_basis = np.concatenate([np.arange(66) % 6, [6, 6, 7, 7, 8, 8]])
    prob, _, _ = replicate_slices(_problem(13, 256, basis, grp_basis, np.ones(ngrps, int), a0, a1), nt)
    if nt == 10:
        for g in (3, 69):  # a set on each kernel
            prob.bl_alias[(nt - 1) * ngrps + g] = -1
    return prob


def dense(nvecs, nfreqs=256, seed=3):
    """SHARED layout, 2 slices of 75 single-baseline groups over 5 blocks; baselines per (block, slice) 23, 9, 17, 21, 5 and
    19, 13, 11, 25, 7: no multiple of 8, 16 or 64."""
    rng = np.random.default_rng(seed)
    basis = _random_blocks(rng, nfreqs, nvecs)
    gb, a0, a1 = [], [], []
    for t, counts in enumerate(([23, 9, 17, 21, 5], [19, 13, 11, 25, 7])):
        u = np.repeat(np.arange(5), counts)
        gb.append(rng.permutation(u))
        i, j = _pairs(13, 75, base=13 * t)
        a0.append(i)
        a1.append(j)
    return _problem(26, nfreqs, basis, np.concatenate(gb), np.ones(150, int), np.concatenate(a0), np.concatenate(a1), nslices=2)


def shared_auto(nants, nbls, seed=4):
    """SHARED layout, single-baseline groups over three 16-vector blocks at 128 channels."""
    rng = np.random.default_rng(seed)
    basis = _random_blocks(rng, 128, [16, 16, 16])
    a0, a1 = _pairs(nants, nbls)
    return _problem(nants, 128, basis, rng.integers(0, 3, nbls), np.ones(nbls, int), a0, a1)


def grp_var(ids, seed=5):
    """Two slices of six single-baseline groups with optimizer variables ``ids`` (cal_problem_desc::grp_var) per slice."""
    rng = np.random.default_rng(seed)
    basis = _random_blocks(rng, 64, [4, 9, 6])
    a0, a1 = _pairs(4, 6)
    base = _problem(4, 64, basis, np.arange(6) % 3, np.ones(6, int), a0, a1, chunk_of_grp=np.asarray(ids, np.int32))
    return replicate_slices(base, 2)[0]


F32, F64 = np.float32, np.float64
CASES = {
    "stream_fold_f32": lambda: (dpss_stream(256), F32, "stream", "auto"),
    "stream_full_f32": lambda: (dpss_stream(256), F32, "stream", "general_full"),
    "stream_f64": lambda: (dpss_stream(256), F64, "stream", "auto"),
    "stream_200_f32": lambda: (dpss_stream(200), F32, "stream", "auto"),
    "stream_200_f64": lambda: (dpss_stream(200), F64, "stream", "auto"),
    "groups_stream_f32": lambda: (groups(), F32, "stream", "auto"),
    "groups_shared_f32": lambda: (groups(), F32, "shared", "auto"),
    "groups_stream_f64": lambda: (groups(), F64, "stream", "auto"),
    "groups_shared_f64": lambda: (groups(), F64, "shared", "auto"),
    "alias_3_f32": lambda: (alias(3, F32), F32, "stream", "auto"),
    "alias_10_f64": lambda: (alias(10, F64), F64, "stream", "auto"),
    "dense_split2_f32": lambda: (dense([20, 45, 77, 130, 200]), F32, "shared", "dense"),
    "dense_split1_f32": lambda: (dense([20, 45, 77, 130, 200]), F32, "shared", "dense_split1"),
    "dense_f32_f32": lambda: (dense([20, 45, 77, 130, 200]), F32, "shared", "dense_f32"),
    "dense_240_f32": lambda: (dense([20, 45, 77, 130, 240]), F32, "shared", "dense"),
    "dense_f64": lambda: (dense([20, 45, 127, 129, 200]), F64, "shared", "dense"),
    "shared_auto_2080_f32": lambda: (shared_auto(65, 2080), F32, "shared", "auto"),
    "shared_auto_1000_f32": lambda: (shared_auto(65, 1000), F32, "shared", "auto"),
    "grp_var_ordered_f32": lambda: (grp_var([0, 0, 1, 1, 2, 2]), F32, "stream", "auto"),
    "grp_var_unordered_f32": lambda: (grp_var([0, 0, 2, 1, 1, 2]), F32, "stream", "auto"),
}

# cal_debug_plan's arrays: what -> (name, numpy dtype of the raw bytes).  Records are read as int32 words, 64-bit fields as int64.
ARRAYS = {
    0: ("scalars", np.int64), 1: ("fb", np.int32), 2: ("tile_off", np.int64), 3: ("bl_tile", np.int64), 4: ("copy_jobs", np.int64),
    5: ("grp_coff", np.int32), 6: ("slice_coff", np.int32), 7: ("slice_cblk", np.int32), 8: ("lamb_vars", np.int64),
    9: ("lamb_cvar_ptr", np.int32), 10: ("lamb_cvar_slice", np.int32), 11: ("lamb_cvar_id", np.int32), 12: ("runs", np.int32),
    13: ("items", np.int32), 14: ("item_goff", np.int32), 15: ("grp_item_ptr", np.int32), 16: ("coef_grp", np.int32),
    17: ("slice_ipart_ptr", np.int32), 18: ("slice_ipart_idx", np.int32), 19: ("slice_ppart_ptr", np.int32),
    20: ("slice_ppart_idx", np.int32), 21: ("members", np.int32), 22: ("heads", np.int32), 23: ("panels", np.int32),
    24: ("panel_map", np.int32), 25: ("op_off", np.int64), 26: ("cs_grp", np.int32), 27: ("ant_ptr", np.int32), 28: ("ant_ent", np.int32),
}
SCALARS = ("fpad ncoef nslices na_slice fold small_loads nitems nitems_simple nitems_plain gc_direct gcp_len basis_bytes steps_per_sync "
           "lds_bytes lds_group_bytes lds_multi_bytes lds_multi_mfma_bytes mf_ok mf_split mf_split2 mf_npanels mf_grid mf_lds_grad "
           "mf_lds_loss nheads nheads_mfma heads_one_pass_local mm_grid lamb_ok lamb_nvar lamb_ncvar").split()


def plan(lib, prob, dtype, layout, kernel_path, whats=None):
    """{name: array} of the host planner's arrays for the problem (raises _lib.CalamityHipError when it is refused)."""
    import ctypes as C

    from calamity_amd import _lib
    from calamity_amd.solver import problem_desc

    d, keep = problem_desc(prob, dtype, layout, kernel_path)
    code = _lib.CAL_F32 if np.dtype(dtype) == np.float32 else _lib.CAL_F64
    out = {}
    for what in ARRAYS if whats is None else whats:
        name, dt = ARRAYS[what]
        n = C.c_int64(0)
        buf = np.empty(8, np.uint8)
        rc = lib.cal_debug_plan(code, C.byref(d), what, buf.ctypes.data_as(C.c_void_p), 0, C.byref(n))  # too small: learns the size
        if n.value > 0:
            buf = np.empty(n.value, np.uint8)
            rc = lib.cal_debug_plan(code, C.byref(d), what, buf.ctypes.data_as(C.c_void_p), buf.nbytes, C.byref(n))
        _lib.check(rc)
        out[name] = buf[: n.value].view(dt).copy()
    del keep
    return out


# ---- the plans of the closed-form calls (calamity_amd/csrc/solve_plan.hpp; cal_debug_solve_plan) ---------------------------------
SOLVE_CASES = ("groups_stream_f32", "groups_shared_f64", "stream_fold_f32", "dense_split2_f32", "dense_f64")
# what -> (name, numpy dtype of the raw bytes); the fit-error plan's arrays are what + 10, named "fe_" instead of "cs_"
SOLVE_ARRAYS = {0: ("cs_scalars", np.int64), 1: ("cs_grp", np.int32), 2: ("cs_order", np.int32), 3: ("cs_work", np.int32),
                4: ("cs_chunks", np.int32), 5: ("cs_woff", np.int64), 6: ("cs_lwork", np.int32)}
SOLVE_ARRAYS.update({10 + w: ("fe_" + nm[3:], dt) for w, (nm, dt) in list(SOLVE_ARRAYS.items())})
SOLVE_LISTS = {20: ("gs_ptr", np.int32), 21: ("gs_ent", np.int32)}  # independent of the bound
SOLVE_ARRAYS.update(SOLVE_LISTS)
SOLVE_SCALARS = "n_max d_max x_max npieces nchunks".split()
WHAT_ROW_CHUNKS = 30
ROW_SCALARS = "rows in_lds lds n m_row n_row d_row".split()
CS_DEFAULT_BOUND = 256 << 20  # kCsScratchDefault
CS_LDS_DOUBLES = 16384        # kCsLdsDoubles
TIME_TILE = 8                 # kTimeTile


def solve_bounds(nvec, itemsize):
    """{tag: scratch bound in bytes} for groups of ``nvec`` vectors: the default (0: one chunk), 1 byte (every group its own chunk),
    and what holds the two heaviest groups but not a third -- by solve_coeffs' count (N in the dtype, the factor in double) and by
    fit_errors' (W, padded to whole 16 x 16 tiles, on top)."""
    n = np.sort(np.asarray(nvec, np.int64))[::-1][:2]
    cs = int((n * n * itemsize + (n + 2) * n * 8).sum())
    pad = (n + 15) // 16 * 16
    return {"default": 0, "one": 1, "two_cs": cs, "two_fe": cs + int((pad * pad * itemsize).sum())}


def solve_plan(call, prob, dtype, layout, kernel_path, bound, whats, row_shape=None):
    """{name: array} of arrays ``whats`` at scratch bound ``bound``.  ``call(dtype code, desc pointer, bound, what, out pointer, capacity,
    bytes pointer)`` is cal_debug_solve_plan (the recording of tests/golden/solve_plan/ passes the parent's loops instead).
    ``row_shape``: (K, L, T) for WHAT_ROW_CHUNKS."""
    import ctypes as C

    from calamity_amd import _lib
    from calamity_amd.solver import problem_desc

    d, keep = problem_desc(prob, dtype, layout, kernel_path)
    code = _lib.CAL_F32 if np.dtype(dtype) == np.float32 else _lib.CAL_F64
    buf = np.empty(1 << 20, np.uint8)
    out = {}
    for what in whats:
        name, dt = ("row_chunks", np.int64) if what == WHAT_ROW_CHUNKS else SOLVE_ARRAYS[what]
        if what == WHAT_ROW_CHUNKS:
            buf[:24].view(np.int64)[:] = row_shape
        n = C.c_int64(0)
        _lib.check(call(code, C.byref(d), bound, what, buf.ctypes.data_as(C.c_void_p), buf.nbytes, C.byref(n)))
        out[name] = buf[: n.value].view(dt).copy()
    del keep
    return out
