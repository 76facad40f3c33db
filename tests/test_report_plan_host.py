"""What cal_solver_delay_spectrum and cal_solver_fix_degeneracies plan on the host before they launch (`cal_debug_report_plan`:
calamity_amd/csrc/report_plan.hpp run with no device), against the rules restated here in NumPy.  The plans decide the order in which
dspec_bin_kernel adds a bin's rows and degen_sum_kernel a slice's segments, which is what the calls' bit-for-bit guarantees rest on.

Everything is compared as integers or bytes.  The floating-point fields d_b, maxd and ratio are compared exactly too: the restatement
does the same float64 subtractions, products, sqrt and division, and adds the frequencies one by one as the planner does.

Problems (single-baseline groups over one random block; only the rows' antennas, nfreqs and fpad matter to these plans):
  rows22   7 antennas, the 21 cross-correlations and the autocorrelation of antenna 2: the rows of
           test_chunks_and_repeated_calls_give_the_same_bits (61 channels, fpad 64)
  rows300  25 antennas, 300 cross-correlations: the smallest triangle past two blocks of the transform's 128 rows
  slices   16 antennas per slice: 120 cross-correlations + 8 autocorrelations = 128 rows (one full segment), + 9 = 129 rows (a second
           segment of one row), and a slice of 22 rows (the rows of rows22 on its first 7 antennas)
  joint    3 times of 5 antennas in ONE problem slice, the rows of the times interleaved: the joint time-basis layout"""
import ctypes as C

import numpy as np
import pytest

import _plan_cases as pc
from calamity_amd import _lib
from calamity_amd.solver import problem_desc

DS_ROWS, DS_COLS, DS_STEP, DG_SEG = 128, 64, 32, 128  # kDsRows, kDsCols, kDsStep (delay_spectrum_kernels.hpp), kDgSeg (degeneracy_kernels.hpp)
DEFAULT_BOUND = 256 << 20                              # kCsScratchDefault
DTYPES = [np.float32, np.float64]
SPECTRUM = {0: ("scalars", np.int64), 1: ("bin_ent", np.int32), 2: ("chunk_ptr", np.int32), 3: ("image", None), 4: ("norm_f", np.float64)}
DEGENERACY = {10: ("scalars", np.int64), 11: ("d_b", np.float64), 12: ("pos", np.float64), 13: ("ratio", np.float64), 14: ("maxd", np.float64),
              15: ("ent", np.int32), 16: ("segptr", np.int32), 17: ("segs", np.int32), 18: ("geo", np.float64), 19: ("idx", np.int32)}
SPECTRUM_SCALARS = "nq xpitch ndpad crows nchunks n_x n_pow n_out".split()


# ---- problems ---------------------------------------------------------------------------------------------------------------------------
def problem_of(nants, a0, a1, nfreqs, nslices=1):
    n = len(a0)
    basis = pc._random_blocks(np.random.default_rng(0), nfreqs, [3])
    kw = {"nslices": nslices} if nslices > 1 else {}
    return pc._problem(nants, nfreqs, basis, np.zeros(n, int), np.ones(n, int), a0, a1, **kw)


def triangle(nants, autos=(), base=0):
    i, j = np.triu_indices(nants, k=1)
    return np.concatenate([i, autos]).astype(np.int32) + base, np.concatenate([j, autos]).astype(np.int32) + base


def rows22(nfreqs=61):
    return problem_of(7, *triangle(7, [2]), nfreqs)


def rows300(nfreqs=61):
    return problem_of(25, *triangle(25), nfreqs)


SLICE_ROWS = {128: lambda base: triangle(16, range(8), base), 129: lambda base: triangle(16, range(9), base), 22: lambda base: triangle(7, [2], base)}


def slices(counts, nfreqs=20):
    """One slice of 16 antennas per entry of ``counts`` (rows per slice), listed slice by slice."""
    parts = [SLICE_ROWS[n](16 * t) for t, n in enumerate(counts)]
    assert [len(p[0]) for p in parts] == list(counts)
    return problem_of(16 * len(counts), np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), nfreqs, nslices=len(counts))


def joint(ntimes=3, na=5, nfreqs=20):
    """Antenna row t na + a is time t, antenna a; one problem slice; row order: pair by pair, every time of a pair in turn."""
    i, j = triangle(na, [1])
    t = np.tile(np.arange(ntimes), len(i))
    return problem_of(ntimes * na, np.repeat(i, ntimes) + t * na, np.repeat(j, ntimes) + t * na, nfreqs)


# ---- the entry ----------------------------------------------------------------------------------------------------------------------------
def fpad_of(prob, dtype):
    return int(pc.plan(_lib.load(), prob, dtype, "stream", "auto", whats=[0])["scalars"][0])


def ptr(a):
    return None if a is None else a.ctypes.data


def spectrum_desc(dtype, op, norm_f, what=7, nbins=0, bin_of_bl=None):
    """(_lib.DelaySpectrumDesc, the arrays it points into)"""
    keep = [np.ascontiguousarray(op.real, dtype), np.ascontiguousarray(op.imag, dtype), np.ascontiguousarray(norm_f, np.float64),
            None if bin_of_bl is None else np.ascontiguousarray(bin_of_bl, np.int32)]
    return _lib.DelaySpectrumDesc(op.shape[1], what, 0, nbins, ptr(keep[3]), ptr(keep[0]), ptr(keep[1]), ptr(keep[2])), keep


def degeneracy_desc(mode, antpos, freqs=None):
    keep = [np.ascontiguousarray(antpos, np.float64), None if freqs is None else np.ascontiguousarray(freqs, np.float64)]
    return _lib.DegeneracyDesc(_lib.DEGENERACY_MODES[mode], 1, None, None, None, ptr(keep[0]), ptr(keep[1]), None, None, None, None), keep


def raw_call(prob, dtype, report, what, cap=1 << 21):
    """(status, bytes written as uint8, size reported) of one cal_debug_report_plan call; ``report``: a _lib.ReportPlanDesc or None"""
    d, keep = problem_desc(prob, dtype, "stream", "auto")
    code = _lib.CAL_F32 if np.dtype(dtype) == np.float32 else _lib.CAL_F64
    buf, n = np.zeros(cap, np.uint8), C.c_int64(0)
    rc = _lib.load().cal_debug_report_plan(code, C.byref(d), None if report is None else C.byref(report), what, buf.ctypes.data_as(C.c_void_p), cap, C.byref(n))
    del keep
    return rc, buf[: max(0, min(cap, n.value))], n.value


def report_plan(prob, dtype, table, **fields):
    """{name: array} of every array of ``table`` (SPECTRUM or DEGENERACY); raises _lib.CalamityHipError where the planner refuses"""
    report = _lib.ReportPlanDesc(**fields)
    out = {}
    for what, (name, dt) in table.items():
        rc, got, _ = raw_call(prob, dtype, report, what)
        _lib.check(rc)
        out[name] = got.view(dtype if dt is None else dt).copy()
    return out


def spectrum_plan(prob, dtype, op, norm_f, bound=0, with_power_bl=False, **kw):
    desc, keep = spectrum_desc(dtype, op, norm_f, **kw)
    return report_plan(prob, dtype, SPECTRUM, spectrum=C.pointer(desc), scratch_bytes=bound, with_power_bl=int(with_power_bl))


def degeneracy_plan(prob, mode, antpos, freqs=None, nslices=0, dtype=np.float32):
    desc, keep = degeneracy_desc(mode, antpos, freqs)
    return report_plan(prob, dtype, DEGENERACY, degeneracy=C.pointer(desc), nslices=nslices)


def refusal(prob, dtype, what, **fields):
    rc, _, _ = raw_call(prob, dtype, _lib.ReportPlanDesc(**fields), what)
    return rc, _lib.load().cal_last_error().decode()


# ---- the rules, restated ------------------------------------------------------------------------------------------------------------------
def spectrum_rule(nbls, nfreqs, fpad, dtype, op, norm_f, what=7, nbins=0, bin_of_bl=None, bound=0, with_power_bl=False):
    size, nd = np.dtype(dtype).itemsize, op.shape[1]
    nq = bin(what).count("1")
    xpitch, ndpad = -(-fpad // DS_STEP) * DS_STEP, -(-nd // DS_COLS) * DS_COLS
    with_power = with_power_bl or nbins > 0
    row_bytes = nq * 2 * xpitch * size + (nq * nd * 8 if with_power else 0)
    crows = max(1, (bound or DEFAULT_BOUND) // row_bytes)
    if crows > DS_ROWS:
        crows -= crows % DS_ROWS
    crows = min(crows, nbls)
    nchunks = -(-nbls // crows)
    lists = [np.flatnonzero(np.asarray(bin_of_bl) == n) for n in range(nbins)]  # ascending rows
    first = np.concatenate([[0], np.cumsum([len(r) for r in lists])]).astype(np.int64)
    chunk_ptr = np.zeros((nchunks, nbins, 2), np.int32)
    for c in range(nchunks):
        b0, b1 = c * crows, min(nbls, (c + 1) * crows)
        for n in range(nbins):
            chunk_ptr[c, n] = first[n] + np.searchsorted(lists[n], [b0, b1])
    image = np.zeros((2, xpitch, ndpad), dtype)
    image[0, :nfreqs, :nd], image[1, :nfreqs, :nd] = op.real, op.imag
    padded = np.zeros(xpitch)
    padded[:nfreqs] = norm_f
    scalars = [nq, xpitch, ndpad, crows, nchunks, nq * 2 * crows * xpitch, nq * crows * nd if with_power else 0, nbls + nq * nbins * nd + nbins]
    return dict(scalars=np.asarray(scalars, np.int64), bin_ent=np.concatenate(lists + [np.zeros(0, np.int64)]).astype(np.int32),
                chunk_ptr=chunk_ptr.ravel(), image=image.ravel(), norm_f=padded), lists


def degeneracy_rule(a0, a1, nants, nsl, nfreqs, fpad, mode, antpos, freqs):
    na, nbls = nants // nsl, len(a0)
    pos = np.asarray(antpos, np.float64)[:na]
    de, dn = pos[a0 % na, 0] - pos[a1 % na, 0], pos[a0 % na, 1] - pos[a1 % na, 1]
    length = np.sqrt(de * de + dn * dn)
    t_of = a0 // na
    maxd = np.asarray([max([0.0] + length[t_of == t].tolist()) for t in range(nsl)])
    ratio = np.zeros(fpad)
    ratio[:nfreqs] = 1.0
    if mode == "band":
        mean = np.float64(0.0)
        for f in freqs:  # one by one, as the planner adds them
            mean = mean + np.float64(f)
        ratio[:nfreqs] = np.asarray(freqs, np.float64) / (mean / nfreqs)
    lists = [np.flatnonzero(t_of == t) for t in range(nsl)]
    first = np.concatenate([[0], np.cumsum([len(r) for r in lists])])
    segs, segptr = [], []
    for t in range(nsl):
        segptr.append(len(segs))
        segs += [[t, e, min(e + DG_SEG, first[t + 1]), 0] for e in range(first[t], first[t + 1], DG_SEG)]
    segptr.append(len(segs))
    P = dict(d_b=np.column_stack([de, dn]).ravel(), pos=pos.ravel(), ratio=ratio, maxd=maxd, ent=np.concatenate(lists).astype(np.int32),
             segptr=np.asarray(segptr, np.int32), segs=np.asarray(segs, np.int32).reshape(-1, 4).ravel())
    P["geo"] = np.concatenate([P[k] for k in ("d_b", "pos", "ratio", "maxd")])
    P["idx"] = np.concatenate([P[k] for k in ("ent", "segptr", "segs")])
    n = [len(segs), 2 * nbls, 2 * nbls + 2 * na, 2 * nbls + 2 * na + fpad, nbls, nbls + nsl + 1]
    P["scalars"] = np.asarray(n, np.int64)
    return P


def assert_same(got, want, label):
    assert sorted(got) == sorted(want), label
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (label, k, got[k].shape, want[k].shape)
        assert got[k].tobytes() == want[k].tobytes(), (label, k, np.flatnonzero(got[k] != want[k])[:8])


def operator(nfreqs, ndelays, seed=1):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((nfreqs, ndelays)) + 1j * rng.standard_normal((nfreqs, ndelays)), 0.5 + rng.random(nfreqs)


def bins_of(nbls, nbins=4):
    """Rows dealt over the bins 0 .. nbins - 2 (bin nbins - 1 stays empty); row 3 is left out (-1)."""
    b = (np.arange(nbls) % (nbins - 1)).astype(np.int32)
    b[3] = -1
    return b


# ---- delay spectrum -----------------------------------------------------------------------------------------------------------------------
def check_spectrum(prob, dtype, op, norm_f, label, **kw):
    fpad = fpad_of(prob, dtype)
    got = spectrum_plan(prob, dtype, op, norm_f, **kw)
    want, lists = spectrum_rule(prob.nbls, prob.nfreqs, fpad, dtype, op, norm_f, **kw)
    assert_same(got, want, label)
    sc = dict(zip(SPECTRUM_SCALARS, got["scalars"].tolist()))
    nbins = kw.get("nbins", 0)
    # every bin's pieces over the chunks concatenate to its sorted row list; no row appears twice
    pieces = got["chunk_ptr"].reshape(sc["nchunks"], nbins, 2)
    for n in range(nbins):
        rows = np.concatenate([got["bin_ent"][pieces[c, n, 0]: pieces[c, n, 1]] for c in range(sc["nchunks"])])
        assert rows.tolist() == lists[n].tolist() and (np.diff(rows) > 0).all(), (label, n)
        for c in range(sc["nchunks"]):
            piece = got["bin_ent"][pieces[c, n, 0]: pieces[c, n, 1]]
            assert ((piece >= c * sc["crows"]) & (piece < (c + 1) * sc["crows"])).all(), (label, n, c)
    assert len(np.unique(got["bin_ent"])) == len(got["bin_ent"]) == (0 if nbins == 0 else int(np.sum(np.asarray(kw["bin_of_bl"]) >= 0)))
    return sc, pieces


@pytest.mark.parametrize("dtype", DTYPES)
def test_chunk_cuts(dtype):
    prob = rows22()
    assert prob.nbls == 22 and fpad_of(prob, dtype) == 64
    op, norm_f = operator(61, 37)
    bins = bins_of(22)
    per_row = 3 * 2 * 64 * np.dtype(dtype).itemsize + 3 * 37 * 8  # the masked planes in the dtype and the power in double: the row bytes differ
    sc, pieces = check_spectrum(prob, dtype, op, norm_f, "7.5 rows", bound=7 * per_row + per_row // 2, nbins=4, bin_of_bl=bins)
    assert (sc["crows"], sc["nchunks"]) == (7, 4) and 22 - 3 * 7 == 1  # four chunks, the last of one row
    assert (pieces[:, 3, 0] == pieces[:, 3, 1]).all()                   # the empty bin has no piece in any chunk
    assert ((pieces[:, :3, 1] - pieces[:, :3, 0]) > 0).sum(axis=0).min() >= 2  # every live bin straddles a cut
    sc, _ = check_spectrum(prob, dtype, op, norm_f, "less than a row", bound=per_row - 1, nbins=4, bin_of_bl=bins)
    assert (sc["crows"], sc["nchunks"]) == (1, 22)
    sc, _ = check_spectrum(prob, dtype, op, norm_f, "default", nbins=4, bin_of_bl=bins)
    assert (sc["crows"], sc["nchunks"]) == (22, 1)
    # without bins and without power_bl the power is not counted in a row; with power_bl it is
    lean = 3 * 2 * 64 * np.dtype(dtype).itemsize
    sc, _ = check_spectrum(prob, dtype, op, norm_f, "no power", bound=7 * lean)
    assert (sc["crows"], sc["n_pow"], sc["nq"]) == (7, 0, 3)
    sc, _ = check_spectrum(prob, dtype, op, norm_f, "power_bl", bound=7 * lean, with_power_bl=True, what=5)
    assert sc["nq"] == 2 and sc["crows"] == 7 * lean // (2 * 2 * 64 * np.dtype(dtype).itemsize + 2 * 37 * 8) and sc["n_pow"] == 2 * sc["crows"] * 37


@pytest.mark.parametrize("dtype", DTYPES)
def test_chunks_are_rounded_to_the_transform_s_rows(dtype):
    prob = rows300()
    assert prob.nbls == 300
    op, norm_f = operator(61, 37)
    per_row = 3 * 2 * 64 * np.dtype(dtype).itemsize + 3 * 37 * 8
    bins = (np.arange(300) // 100).astype(np.int32)  # bin 1 (rows 100 .. 199) straddles the cut at 128
    sc, pieces = check_spectrum(prob, dtype, op, norm_f, "200 rows", bound=200 * per_row, nbins=3, bin_of_bl=bins)
    assert (sc["crows"], sc["nchunks"]) == (DS_ROWS, 3)
    assert (pieces[:, 1, 1] - pieces[:, 1, 0]).tolist() == [28, 72, 0]
    sc, _ = check_spectrum(prob, dtype, op, norm_f, "128 rows stay", bound=128 * per_row, nbins=3, bin_of_bl=bins)
    assert sc["crows"] == 128
    sc, _ = check_spectrum(prob, dtype, op, norm_f, "127 rows are not rounded", bound=127 * per_row + 1, nbins=3, bin_of_bl=bins)
    assert (sc["crows"], sc["nchunks"]) == (127, 3)


@pytest.mark.parametrize("dtype", DTYPES)
def test_bins(dtype):
    prob = rows22()
    op, norm_f = operator(61, 37)
    per_row = 3 * 2 * 64 * np.dtype(dtype).itemsize + 3 * 37 * 8
    sc, _ = check_spectrum(prob, dtype, op, norm_f, "no bins", bound=7 * per_row, with_power_bl=True)
    assert sc["n_out"] == 22
    none = np.full(22, -1, np.int32)
    sc, pieces = check_spectrum(prob, dtype, op, norm_f, "every row left out", bound=7 * per_row, nbins=2, bin_of_bl=none)
    assert not pieces.any() and sc["n_out"] == 22 + 3 * 2 * 37 + 2
    mixed = np.asarray([2, -1, 0, 0, 2, -1, 2, 2, 0, -1, 2, 0, 0, 0, -1, 2, 2, 0, 2, -1, 0, 2], np.int32)  # bin 1 is empty
    check_spectrum(prob, dtype, op, norm_f, "unsorted bins", bound=7 * per_row, nbins=3, bin_of_bl=mixed)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nfreqs,ndelays", [(61, 37), (64, 64), (200, 200)])
def test_the_operator_image(nfreqs, ndelays, dtype):
    prob = rows22(nfreqs)
    fpad = fpad_of(prob, dtype)
    op, norm_f = operator(nfreqs, ndelays)
    got = spectrum_plan(prob, dtype, op, norm_f)
    sc = dict(zip(SPECTRUM_SCALARS, got["scalars"].tolist()))
    assert sc["xpitch"] % DS_STEP == 0 and fpad <= sc["xpitch"] < fpad + DS_STEP and sc["ndpad"] % DS_COLS == 0 and ndelays <= sc["ndpad"] < ndelays + DS_COLS
    if (nfreqs, ndelays) == (64, 64):
        assert sc["xpitch"] == fpad == nfreqs and sc["ndpad"] == ndelays  # nothing to pad
    image = got["image"].reshape(2, sc["xpitch"], sc["ndpad"])
    assert image.dtype == np.dtype(dtype)
    assert np.array_equal(image[0, :nfreqs, :ndelays], op.real.astype(dtype)) and np.array_equal(image[1, :nfreqs, :ndelays], op.imag.astype(dtype))
    assert not image[:, nfreqs:].any() and not image[:, :, ndelays:].any()
    assert np.array_equal(got["norm_f"][:nfreqs], norm_f) and not got["norm_f"][nfreqs:].any() and len(got["norm_f"]) == sc["xpitch"]
    assert_same(got, spectrum_rule(22, nfreqs, fpad, dtype, op, norm_f)[0], "image")


@pytest.mark.parametrize("dtype", DTYPES)
def test_spectrum_refusals_keep_their_texts(dtype):
    prob = rows22()
    op, norm_f = operator(61, 37)
    bins = bins_of(22)
    bins[5] = 9
    desc, keep = spectrum_desc(dtype, op, norm_f, nbins=4, bin_of_bl=bins)
    assert refusal(prob, dtype, 0, spectrum=C.pointer(desc)) == (_lib.CAL_ERR_INVALID, "delay_spectrum: bin_of_bl[5] = 9 lies outside [-1, 4)")
    bins[5] = -2
    assert refusal(prob, dtype, 1, spectrum=C.pointer(desc)) == (_lib.CAL_ERR_INVALID, "delay_spectrum: bin_of_bl[5] = -2 lies outside [-1, 4)")
    many = (2 ** 31 - 1) // (3 * 37 + 1) + 1  # nwhat nbins ndelays + nbins no longer fits an int
    desc, keep = spectrum_desc(dtype, op, norm_f, nbins=many, bin_of_bl=np.zeros(22, np.int32))
    assert refusal(prob, dtype, 0, spectrum=C.pointer(desc)) == (_lib.CAL_ERR_INVALID, f"delay_spectrum: nbins = {many} is too many")


# ---- degeneracies -------------------------------------------------------------------------------------------------------------------------
def positions(na, seed=2):
    return np.random.default_rng(seed).uniform(-150.0, 150.0, size=(na, 2))


def check_degeneracy(prob, mode, antpos, freqs, nsl, label, nslices=0):
    fpad = fpad_of(prob, np.float32)
    got = degeneracy_plan(prob, mode, antpos, freqs, nslices=nslices)
    want = degeneracy_rule(prob.bl_ant0, prob.bl_ant1, prob.nants, nsl, prob.nfreqs, fpad, mode, antpos, freqs)
    assert_same(got, want, label)
    na = prob.nants // nsl
    segs, segptr, ent = got["segs"].reshape(-1, 4), got["segptr"], got["ent"]
    assert len(segptr) == nsl + 1 and segptr[0] == 0 and segptr[-1] == len(segs) == got["scalars"][0] and (np.diff(segptr) >= 0).all()
    assert sorted(ent.tolist()) == list(range(prob.nbls))
    e = 0
    for t in range(nsl):
        mine = segs[segptr[t]: segptr[t + 1]]
        assert (mine[:, 0] == t).all() and not mine[:, 3].any(), (label, t)
        for s in mine:  # the segments of a slice tile its rows in increasing order, every one full but the last
            assert s[1] == e and e < s[2] <= e + DG_SEG, (label, t, s)
            e = s[2]
        assert (np.diff(mine[:, 1]) == DG_SEG).all()
        rows = ent[(mine[0, 1] if len(mine) else e): e]
        assert (np.diff(rows) > 0).all() and (prob.bl_ant0[rows] // na == t).all() and (prob.bl_ant1[rows] // na == t).all(), (label, t)
        assert len(rows) == int(np.sum(prob.bl_ant0 // na == t))
    assert e == prob.nbls
    return got


@pytest.mark.parametrize("counts,nseg", [((128,), [1]), ((129,), [2]), ((22,), [1]), ((128, 129), [1, 2]), ((129, 22, 128), [2, 1, 1])])
@pytest.mark.parametrize("mode", ["channel", "band"])
def test_rows_and_segments_of_the_slices(counts, nseg, mode):
    prob = slices(counts)
    freqs = 150e6 + 1e6 * np.arange(prob.nfreqs)
    got = check_degeneracy(prob, mode, positions(16), freqs if mode == "band" else None, len(counts), f"{counts} {mode}")
    assert np.diff(got["segptr"]).tolist() == nseg
    segs = got["segs"].reshape(-1, 4)
    assert (segs[:, 2] - segs[:, 1]).tolist() == [n for c in counts for n in ([128, c - 128] if c > 128 else [c])]  # 129 rows: a second segment of one row


def test_geometry():
    prob = slices((129, 22, 128))
    pos = positions(16)
    freqs = 150e6 + 1e6 * np.arange(prob.nfreqs) ** 1.1
    fpad = fpad_of(prob, np.float32)
    assert fpad > prob.nfreqs
    chan = check_degeneracy(prob, "channel", pos, None, 3, "channel")
    assert (chan["ratio"][: prob.nfreqs] == 1.0).all() and not chan["ratio"][prob.nfreqs:].any() and len(chan["ratio"]) == fpad
    band = check_degeneracy(prob, "band", pos, freqs, 3, "band")
    assert np.allclose(band["ratio"][: prob.nfreqs], freqs / freqs.mean(), rtol=1e-15, atol=0) and not band["ratio"][prob.nfreqs:].any()
    # maxd per slice: the 22-row slice reaches only its first 7 antennas
    d = pos[:, None, :] - pos[None, :, :]
    length = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])
    assert band["maxd"].tolist() == [length.max(), length[:7, :7].max(), length.max()] and band["maxd"][1] < band["maxd"][0]
    # an autocorrelation row has d_b = 0
    autos = prob.bl_ant0 == prob.bl_ant1
    assert autos.sum() == 9 + 1 + 8 and not band["d_b"].reshape(-1, 2)[autos].any() and band["d_b"].reshape(-1, 2)[~autos].any(axis=1).all()


def test_the_joint_time_basis_layout_has_one_slice_per_time():
    prob = joint()
    assert prob.nants == 15 and prob.nbls == 33 and prob.nslices == 1
    got = check_degeneracy(prob, "channel", positions(5), None, 3, "joint", nslices=3)
    assert got["ent"].tolist() == [b for t in range(3) for b in range(t, 33, 3)]  # the rows of time t, ascending
    assert got["segs"].reshape(-1, 4).tolist() == [[0, 0, 11, 0], [1, 11, 22, 0], [2, 22, 33, 0]]
    assert got["maxd"][0] == got["maxd"][1] == got["maxd"][2] > 0
    one = check_degeneracy(prob, "channel", positions(15), None, 1, "one slice of 15 antennas")  # nslices = 0: the problem's own
    assert one["ent"].tolist() == list(range(33)) and len(one["pos"]) == 30


def test_degeneracy_refusals_keep_their_texts():
    prob = joint()
    pos = positions(5)
    freqs = 150e6 + 1e6 * np.arange(prob.nfreqs)

    def refused(what, mode, antpos, f=None, nslices=3, p=prob):
        desc, keep = degeneracy_desc(mode, antpos, f)
        return refusal(p, np.float32, what, degeneracy=C.pointer(desc), nslices=nslices)

    a0, a1 = prob.bl_ant0.copy(), prob.bl_ant1.copy()
    a0[7], a1[7] = 3, 12  # times 0 and 2
    a0[20], a1[20] = 1, 6  # a later row is not the one reported
    crossed = problem_of(15, a0, a1, prob.nfreqs)
    assert refused(15, "channel", pos, p=crossed) == (_lib.CAL_ERR_INVALID, "fix_degeneracies: baseline row 7 joins antennas of two slices (3, 12; 5 antennas per slice)")
    for bad in ([0.0] * prob.nfreqs, [np.inf] + [1.0] * (prob.nfreqs - 1), [1.0, -1.0] * (prob.nfreqs // 2)):
        assert refused(13, "band", pos, np.asarray(bad)) == (_lib.CAL_ERR_INVALID, "fix_degeneracies: the mean of freqs must be finite and not zero")
    assert refused(13, "channel", pos, np.zeros(prob.nfreqs))[0] == 0  # freqs are read in band mode only
    for k, value in ((4, np.nan), (5, np.inf)):
        broken = pos.copy()
        broken.ravel()[k] = value
        assert refused(10, "band", broken, freqs) == (_lib.CAL_ERR_INVALID, "fix_degeneracies: antenna position 2 is not finite")


# ---- the entry itself -----------------------------------------------------------------------------------------------------------------------
def test_refusals_of_the_entry():
    prob = rows22()
    op, norm_f = operator(61, 37)
    sdesc, keep_s = spectrum_desc(np.float32, op, norm_f)
    gdesc, keep_g = degeneracy_desc("channel", positions(7))
    full = dict(spectrum=C.pointer(sdesc), degeneracy=C.pointer(gdesc))
    lib = _lib.load()
    for what in (-1, 5, 9, 20, 30):
        assert refusal(prob, np.float32, what, **full) == (_lib.CAL_ERR_INVALID, f"cal_debug_report_plan: what = {what}")
    rc, _, _ = raw_call(prob, np.float32, None, 0)  # a null descriptor
    assert rc == _lib.CAL_ERR_INVALID and lib.cal_last_error().decode() == "cal_debug_report_plan: bad argument"
    d, keep = problem_desc(prob, np.float32, "stream", "auto")
    n = C.c_int64(0)
    assert lib.cal_debug_report_plan(7, C.byref(d), C.byref(_lib.ReportPlanDesc(**full)), 0, np.zeros(8, np.uint8).ctypes.data_as(C.c_void_p), 8, C.byref(n)) == _lib.CAL_ERR_INVALID
    assert lib.cal_last_error().decode() == "cal_debug_report_plan: bad argument"  # an unknown dtype
    # the call's own description is missing, or not one the solver's call would plan for
    assert refusal(prob, np.float32, 0, degeneracy=C.pointer(gdesc))[0] == _lib.CAL_ERR_INVALID
    assert refusal(prob, np.float32, 10, spectrum=C.pointer(sdesc))[0] == _lib.CAL_ERR_INVALID
    assert refusal(prob, np.float32, 0, scratch_bytes=-1, **full)[0] == _lib.CAL_ERR_INVALID
    assert refusal(prob, np.float32, 10, nslices=2, **full)[0] == _lib.CAL_ERR_INVALID  # 2 does not divide 7 antennas
    # a short buffer: the size is reported, nothing is written
    for what, size in ((0, 64), (3, 2 * 64 * 64 * 4), (11, 22 * 2 * 8), (17, 16)):
        rc, got, n = raw_call(prob, np.float32, _lib.ReportPlanDesc(**full), what, cap=size - 1)
        assert rc == _lib.CAL_ERR_INVALID and n == size and not got.any()
        assert lib.cal_last_error().decode() == f"cal_debug_report_plan: the array has {size} bytes, the buffer {size - 1}"
        rc, got, n = raw_call(prob, np.float32, _lib.ReportPlanDesc(**full), what, cap=size)
        assert rc == 0 and n == size
    # a bound of 0 is the default bound, as in set_delay_spectrum_scratch
    a = spectrum_plan(prob, np.float32, op, norm_f, bound=0)
    assert_same(a, spectrum_plan(prob, np.float32, op, norm_f, bound=DEFAULT_BOUND), "default bound")
    del keep, keep_s, keep_g
