"""The six post-fit reports -- ``fit_errors``, ``gain_basis_errors``, ``delay_spectrum``, ``delay_cross_spectrum``, ``delay_transfer``,
``fix_degeneracies`` -- on the solver configurations production calls them in (``slice_pipeline`` runs them one after another at the end of every slice): the
dense matrix-core kernel paths, the "sum" regulariser set, a descent continued through them at graph length, several slices.

The argument is the one of tests/test_gpu_solve_paths.py: every report goes through ``model_pass``, which launches
the general MODE_MODEL kernels on the tile buffer whatever kernels the descent runs on; the row, factor and antenna kernels behind it
read that model, the data, the weights and the plan scalars, none of which depends on the kernel path; no report reads the regulariser;
and a call puts the loop state back where it found it.  So everything a report returns is compared BIT FOR BIT between the paths, with
and without the regulariser, and a descent continued behind the reports with one that never called them.  Two things are no output of
a report and are the path's OWN kernels (``eval_pass``): ``eval_loss()`` and ``eval_grads()`` afterwards.  The dense kernels sum the
chi-square and the gradients on the matrix cores in another order than the general ones, by design (tests/test_gpu_fp32_families.py
bounds every family against the oracle), so across paths they are held to ``TOL["loss"]`` and ``TOL["plane"]``; that the report left
nothing behind that they read is pinned more sharply: they equal, to the bit, those of a solver of the SAME path that made no call.

Cases, inputs, restatements and checks: tests/report_cases.py (the smallest shapes that qualify for the dense paths; the restatement
and ``check`` of every report's own test file; no tolerance of this file's own).  Every solver asserts the kernel path it asked for,
before and after the call.  tests/test_report_paths_host.py holds the cases to their preconditions without a device.

Shown once on scratch copies of the library (each inside its buffers: wrong numbers, no fault; each passes the older report files):

  * a report's ``model_pass`` on a dense path overwrites the loop state as ``set_optimizer`` does (iteration count, bias-correction
    powers) and nothing puts it back (dropping the restore alone fails nothing and cannot: DESIGN.md section 5): fails the 48 dense
    cases of ``test_a_descent_continued_behind_all_the_reports_equals_the_plain_512_steps`` (3 kinds x 4 dense paths x 2 x 2) and the
    8 dense cases of ``test_a_fresh_solver_resumed_behind_the_reports_continues_identically``; every ``general`` case passes;
  * ``fix_degeneracies``' reference planes aliased onto the model planes of ``model_buf`` on the dense paths only (same size): fails the
    16 dense ``fix_degeneracies`` cases of ``test_every_report_equals_its_restatement_on_every_path``, the 16 of
    ``test_every_report_gives_the_bits_of_the_general_path`` and the 4 dense ``fix_degeneracies`` cases of
    tests/test_gpu_robust_reports.py against the restatement (solvers A and B there are wrong alike).

The same for the sixth report, ``delay_cross_spectrum``, each shown once and each passing tests/test_gpu_delay_cross.py,
test_gpu_delay_cross_dropin.py and test_gpu_delay_cross_ranks.py as they stood before the report joined this file (60 tests):

  * the cross call's ``model_pass`` on a dense path overwrites the loop state as ``set_optimizer`` does and nothing puts it back: fails
    the same 48 + 8 dense cases of the two descent tests, through ``all_reports``; every ``general`` case passes.  With the restore
    ALONE dropped for this call on the dense paths nothing fails, here or anywhere, and nothing can, for the reason above:
    ``begin_pass_state`` changes only ``done`` / ``done_after`` of the mirror, and every entry that reads them writes them first;
  * the two builds that read ``rw_w0`` in ``dcross_rows_kernel`` fail no test of this file (it never reweights), and the one that skips
    the upload of ``ds_ptr`` / ``ds_ent`` behind a spectrum call none either (``all_reports`` gives both calls the same three bins over
    the same rows, and ``slice_reports`` likewise: the stale lists are the right ones): see tests/test_gpu_robust_reports.py and
    tests/test_gpu_report_order.py.

Both pass tests/test_gpu_fit_errors.py, test_gpu_gain_basis_errors.py, test_gpu_delay_spectrum.py, test_gpu_delay_transfer.py,
test_gpu_degeneracy.py, test_gpu_robust_consumers.py and test_gpu_solve_paths.py (742 tests), which run the reports on the default
path.  The six builds that read ``w0`` behind a reweight fail no test of this file (it never reweights): see
tests/test_gpu_robust_reports.py."""
import copy
import functools

import numpy as np
import pytest

import degeneracy_ref as R
import report_cases as C
import test_gpu_degeneracy as DG
import test_gpu_delay_cross as DC
import test_gpu_delay_spectrum as DS
from test_gpu_fit_quality import TOL, plane_err
from test_gpu_solve_paths import (DENSE, DTYPES, NSTEPS, PATHS, PRIORS, REG_IDS, REG_PATHS, REGS, assert_path, assert_same_bits, assert_same_state,
                                  descent_inputs, full_state, path_id, path_solver, three_slices)

pytestmark = pytest.mark.gpu

PATH_IDS = list(map(path_id, PATHS))
CASE_IDS = list(map(C.case_id, C.CASES))
OWN_PASS = ("loss", "grad_loss", "gg_r", "gg_i", "gc_r", "gc_i")  # eval_loss() / eval_grads() afterwards: the path's own kernels


def solver(case, dtype, path, reg=False):
    """SHARED layout, the kernel path asked for and no other (asserted), the case's gain bases attached."""
    p, params, B, Bt = C.inputs(*case)
    if case[0] != "fix_degeneracies":
        return path_solver(p, params, dtype, path, B, Bt, reg)
    s = DG.solver_of(p, params, dtype, "shared", path)
    if reg:
        s.set_regularization("sum", *PRIORS)
    assert_path(s, path)
    return s


def afterwards(s):
    """What a solver gives behind a call: fit quality (bit for bit across the paths), then its own loss and gradient passes."""
    out = {f"quality_{k}": v for k, v in s.fit_quality().items()}
    out.update(zip(OWN_PASS[1:], s.eval_grads()))
    out["loss"] = s.eval_loss()
    return out


@functools.lru_cache(maxsize=None)
def outputs(case, dtype_name, path, reg=False, with_call=True):
    """One report on a fresh solver: everything it returns (flat), and fit quality, the gradients and the loss afterwards."""
    s = solver(case, np.dtype(dtype_name).type, path, reg)
    raw = C.call(s, *case) if with_call else {}
    assert_path(s, path)
    out = dict(C.flat(raw), **afterwards(s))
    assert_path(s, path)
    s.close()
    return raw, out


def label_of(case, dtype, path):
    return f"{C.case_id(case)} {path} {np.dtype(dtype).name}"


# ---- (a) parity with the restatement on every path
@pytest.mark.parametrize("dtype,path", PATHS, ids=PATH_IDS)
@pytest.mark.parametrize("case", C.CASES, ids=CASE_IDS)
def test_every_report_equals_its_restatement_on_every_path(case, dtype, path):
    name = np.dtype(dtype).name
    raw, out = outputs(case, name, path)
    ref = C.restatement(*case, dtype, model=C.device_model(raw)) if case[0] == "fix_degeneracies" else C.reference(*case, name)
    C.check(*case, raw, ref, dtype, label_of(case, dtype, path))
    assert np.isfinite(out["loss"]) and out["loss"] > 0


# ---- (b) across the paths, and with the regulariser
def without_own_pass(out):
    out = dict(out)
    return out, {k: out.pop(k) for k in OWN_PASS}


def check_own_pass(got, want, dtype, label):
    """The loss and the gradients of two kernel paths: the paths' own sums, at the project's tolerances."""
    tol = TOL[np.dtype(dtype)]
    errs = {k: abs(got[k] - want[k]) / want[k] for k in ("loss", "grad_loss")}
    planes = {k: plane_err(got[k], want[k]) for k in OWN_PASS[2:]}
    print(f"{label}: against the general path  " + "  ".join(f"{k} {v:.2e}" for k, v in {**errs, **planes}.items()))
    assert max(errs.values()) <= tol["loss"] and max(planes.values()) <= tol["plane"], (label, errs, planes)


@pytest.mark.parametrize("dtype,path", DENSE, ids=map(path_id, DENSE))
@pytest.mark.parametrize("case", C.CASES, ids=CASE_IDS)
def test_every_report_gives_the_bits_of_the_general_path(case, dtype, path):
    name = np.dtype(dtype).name
    got, own = without_own_pass(outputs(case, name, path)[1])
    want, own_general = without_own_pass(outputs(case, name, "general")[1])
    assert_same_bits(got, want, label_of(case, dtype, path))
    check_own_pass(own, own_general, dtype, label_of(case, dtype, path))


@pytest.mark.parametrize("dtype,path", PATHS, ids=PATH_IDS)
@pytest.mark.parametrize("case", C.CASES, ids=CASE_IDS)
def test_a_report_leaves_nothing_behind_that_the_loss_and_gradient_passes_read(case, dtype, path):
    """``eval_grads()`` and ``eval_loss()`` behind the report against a solver of the same path that never called it: the same bits."""
    name = np.dtype(dtype).name
    got, want = outputs(case, name, path)[1], outputs(case, name, path, with_call=False)[1]
    assert_same_bits({k: got[k] for k in want}, want, label_of(case, dtype, path) + " behind the call")


@pytest.mark.parametrize("dtype,path", REG_PATHS, ids=map(path_id, REG_PATHS))
@pytest.mark.parametrize("case", C.CASES, ids=CASE_IDS)
def test_the_sum_regulariser_changes_no_bit_of_any_report(case, dtype, path):
    """No report reads the regulariser; fit quality afterwards is unregularised.  ``eval_loss`` / ``eval_grads`` are DEFINED with it."""
    name = np.dtype(dtype).name
    with_reg, own_reg = without_own_pass(outputs(case, name, path, True)[1])
    without, own = without_own_pass(outputs(case, name, path)[1])
    assert_same_bits(with_reg, without, label_of(case, dtype, path) + " with the regulariser")
    assert own_reg["loss"] > own["loss"] and own_reg["grad_loss"] > own["grad_loss"]  # (the priors are far from the model's sums: it is on)


# ---- (c) a descent continued through all the reports
DESCENT_KINDS = ["free", "basis", "time"]  # edge_problem(12, 129) without and with a frequency gain basis; (4, 5, 72) with both bases


def all_reports(s, kind):
    """The reports one after another, as ``slice_pipeline`` calls them at the end of a slice."""
    p, _, B, Bt = descent_inputs(kind)
    basis = kind != "free"
    op, norm_f = DS.operator(p.nfreqs, p.nfreqs)
    bins = (np.arange(p.nbls) % 3).astype(np.int32)
    out = [s.fit_errors(gain_var=not basis)]
    if basis:
        out.append(s.gain_basis_errors())
    out.append(s.delay_spectrum(op, norm_f, bin_of_bl=bins, nbins=3))
    pairs = np.stack([np.arange(p.nbls), (np.arange(p.nbls) + 1) % p.nbls], axis=1).astype(np.int32)
    cross = s.delay_cross_spectrum(op, norm_f, pairs, bin_of_pair=bins, nbins=3)
    assert cross["diff"]["resid"].sum() > 0
    out.append(s.delay_transfer(op, bin_of_bl=bins, nbins=3))
    na = p.nants // (Bt.shape[0] if Bt is not None else 1)
    gref = s.get_params()[:2]
    out.append(s.fix_degeneracies(p.data_r, p.data_i, R.hex_array(na), mode="band", freqs=150e6 + 400e3 * np.arange(p.nfreqs), gref_r=gref[0], gref_i=gref[1]))
    assert out[0]["leverage_bl"].sum() > 0 and out[-3]["resid"].sum() > 0 and out[-2]["absorbed_bin"].sum() > 0 and out[-1]["nsamples"].sum() > 0
    assert not basis or np.any(out[1]["gain_var"])
    return out


def descent_solver(kind, dtype, path, reg, mode):
    p, params, B, Bt = descent_inputs(kind)
    s = path_solver(p, params, dtype, path, B, Bt, reg)
    s.set_launch_mode(mode)
    s.set_optimizer("Adam", learning_rate=1e-2)
    return s


@functools.lru_cache(maxsize=None)
def descent(kind, dtype_name, path, reg, mode, reports):
    """run(256), all the reports (or none), run(256): the losses, the state behind the reports and at the end, the weight planes
    before and behind the reports."""
    s = descent_solver(kind, np.dtype(dtype_name).type, path, reg, mode)
    first = s.run(NSTEPS, tol=0.0)[0]
    weights = [s.get_weights(0), s.get_weights(1)]
    if reports:
        all_reports(s, kind)
        assert_path(s, path)
    weights += [s.get_weights(0), s.get_weights(1)]
    middle = full_state(s, kind)
    second = s.run(NSTEPS, tol=0.0)[0]
    final = full_state(s, kind)
    assert_path(s, path)
    s.close()
    losses = np.concatenate([first, second])
    assert len(losses) == 2 * NSTEPS and np.all(np.isfinite(losses))
    return losses, middle, final, weights


@pytest.mark.parametrize("mode", ["graph", "kernels"])
@pytest.mark.parametrize("reg", REGS, ids=REG_IDS)
@pytest.mark.parametrize("dtype,path", PATHS, ids=PATH_IDS)
@pytest.mark.parametrize("kind", DESCENT_KINDS)
def test_a_descent_continued_behind_all_the_reports_equals_the_plain_512_steps(kind, dtype, path, reg, mode):
    """Losses, parameters, ``y`` and the optimizer's slots, bit for bit, replayed as a hipGraph and launched kernel by kernel (the plain
    descent is the replayed one: the launch forms agree to the bit); the two weight planes keep their bits through the reports."""
    name = np.dtype(dtype).name
    losses, middle, final, weights = descent(kind, name, path, reg, mode, True)
    plain_losses, plain_middle, plain_final, _ = descent(kind, name, path, reg, "graph", False)
    label = f"{kind} {path} {name} {mode}"
    np.testing.assert_array_equal(losses, plain_losses, err_msg=label)
    assert_same_state(middle, plain_middle, label + " behind the reports")
    assert_same_state(final, plain_final, label)
    assert losses[-1] < losses[0]
    for k in (0, 1):
        np.testing.assert_array_equal(weights[2 + k], weights[k], err_msg=f"{label}: get_weights({k})")


@pytest.mark.parametrize("reg", REGS, ids=REG_IDS)
@pytest.mark.parametrize("dtype,path", PATHS, ids=PATH_IDS)
def test_a_fresh_solver_resumed_behind_the_reports_continues_identically(dtype, path, reg):
    """The parameters and moments read behind the reports, given to a fresh solver: its next 256 steps are those of the solver that
    called the reports (``set_moments`` is refused under a gain basis, so this is the fit without one)."""
    name = np.dtype(dtype).name
    losses, middle, final, _ = descent("free", name, path, reg, "graph", True)
    p, start = descent_inputs("free")[:2]
    fresh = path_solver(p, start, dtype, path, reg=reg)
    fresh.set_params(*(middle[k] for k in ("g_r", "g_i", "c_r", "c_i")))
    fresh.set_optimizer("Adam", learning_rate=1e-2)
    moments = {k: v for k, v in middle.items() if k[:2] in ("gm", "gv", "cm", "cv")}
    assert middle["t"] == NSTEPS
    fresh.set_moments(**moments, t=NSTEPS)
    got_losses = fresh.run(NSTEPS, tol=0.0)[0]
    got = full_state(fresh, "free")
    assert_path(fresh, path)
    fresh.close()
    np.testing.assert_array_equal(got_losses, losses[NSTEPS:])
    assert_same_state(got, final, f"resumed {path} {name}")


# ---- (d) several slices on the dense path
def slice_reports(s, nb, nslices):
    """The reports of every slice; the cross spectrum with the within-slice pairs (t nb + b, t nb + (b + 3) % nb), pair t nb + b in row
    t nb + b's bin, the same seeded unequal scales in every slice: what a solver of ONE slice can restate."""
    op, norm_f = DS.operator(200, 200)
    bins = (np.repeat(np.arange(nslices), nb) * 2 + np.tile(np.arange(nb) % 2, nslices)).astype(np.int32)
    pairs = np.array([(t * nb + b, t * nb + (b + 3) % nb) for t in range(nslices) for b in range(nb)], dtype=np.int32)
    scale = np.tile(np.random.default_rng(9).uniform(0.5, 2.0, size=(nb, 2)), (nslices, 1))
    return dict(fit_errors=s.fit_errors(), delay_spectrum=C.flat(s.delay_spectrum(op, norm_f, bin_of_bl=bins, nbins=2 * nslices, per_baseline=True)),
                delay_cross=C.flat(s.delay_cross_spectrum(op, norm_f, pairs, scale=scale, bin_of_pair=bins, nbins=2 * nslices, per_pair=True)),
                delay_transfer=s.delay_transfer(op, bin_of_bl=bins, nbins=2 * nslices, per_baseline=True))


def rows_of_slice(name, key, arr, t, p0):
    """Slice ``t`` of one output of a solver of several slices (the bins encode (slice, bin) with two bins a slice; of the cross
    spectrum ``cross_<quantity>`` and ``diff_<quantity>`` are bins, ``per_pair_...`` and ``norm_pair`` one pair a row)."""
    if np.isscalar(arr):
        return None
    binned = key in ("data", "model", "resid", "count_bin", "absorbed_bin") or (name == "delay_cross" and key.startswith(("cross_", "diff_")))
    n = {"coeff_var": p0.ncoeffs, "gain_var": p0.nants}.get(key, 2 if binned else p0.nbls)
    return arr[t * n : (t + 1) * n]


@pytest.mark.parametrize("dtype", DTYPES)
def test_three_slices_on_the_dense_path_equal_three_single_slice_solvers(dtype):
    from calamity_amd.solver import HipFitSolver

    p0, sub, data, start = three_slices()
    nb, na, nc = p0.nbls, p0.nants, p0.ncoeffs
    s = HipFitSolver(dtype=dtype)
    s.set_problem(sub, layout="shared", kernel_path="dense")
    s.set_data(*data)
    s.set_params(start["g_r"], start["g_i"], start["c_r"], start["c_i"])
    assert_path(s, "dense")
    batch = slice_reports(s, nb, 3)
    assert_path(s, "dense")
    s.close()
    assert (batch["fit_errors"]["nsolved"], batch["delay_transfer"]["nsolved"]) == (3 * p0.ngrps, 3 * p0.ngrps)
    for t in range(3):
        one = HipFitSolver(dtype=dtype)
        shell = copy.copy(p0)
        shell.data_r = shell.data_i = shell.wgts = None
        one.set_problem(shell, layout="shared", kernel_path="dense")
        one.set_data(*[a[t * nb : (t + 1) * nb] for a in data])
        one.set_params(*[start[k][t * n : (t + 1) * n] for k, n in (("g_r", na), ("g_i", na), ("c_r", nc), ("c_i", nc))])
        assert_path(one, "dense")
        alone = slice_reports(one, nb, 1)
        assert_path(one, "dense")
        one.close()
        for name in batch:
            for key, arr in batch[name].items():
                rows = rows_of_slice(name, key, arr, t, p0)
                if rows is None:
                    assert alone[name][key] * 3 == arr, (name, key)  # the counts
                else:
                    assert rows.shape == alone[name][key].shape, (name, key)
                    np.testing.assert_array_equal(rows, alone[name][key], err_msg=f"slice {t} {np.dtype(dtype).name}: {name} {key}")


# ---- the pairs production asks for: the same baseline in adjacent slices (no solver of one slice can restate them)
def cross_slice_problem():
    """``three_slices()`` as the cross spectrum's reference takes it: (problem with data and weights, p0, per-slice parameters)."""
    p0, sub, data, start = three_slices()
    full = copy.copy(sub)
    full.data_r, full.data_i, full.wgts = data
    sizes = dict(g_r=p0.nants, g_i=p0.nants, c_r=p0.ncoeffs, c_i=p0.ncoeffs)
    pars = [{k: start[k][t * n : (t + 1) * n] for k, n in sizes.items()} for t in range(3)]
    return full, p0, pars


def cross_slice_pairs(nb):
    """(pairs, scale, bins, nbins, forward, reversed, bb): (t nb + b, (t + 1) nb + b) for t = 0, 1, then (nb + 4, 4) -- pair 4 reversed,
    with its scales exchanged -- and (nb + 2, nb + 2) with unit scales."""
    pairs = np.array([(t * nb + b, (t + 1) * nb + b) for t in range(2) for b in range(nb)] + [(nb + 4, 4), (nb + 2, nb + 2)], dtype=np.int32)
    forward, rev, bb = 4, 2 * nb, 2 * nb + 1
    scale = np.random.default_rng(10).uniform(0.5, 2.0, size=(len(pairs), 2))
    scale[rev] = scale[forward][::-1]
    scale[bb] = 1.0
    return (pairs, scale) + DC.bins_of_pairs(len(pairs)) + (forward, rev, bb)


@functools.lru_cache(maxsize=None)
def cross_slices(dtype_name, path, calibrated):
    full, p0, pars = cross_slice_problem()
    pairs, scale, bins, nbins = cross_slice_pairs(p0.nbls)[:4]
    op, norm_f = DS.operator(200, 200)
    s = DC.solver_of(full, DC.joined(pars), np.dtype(dtype_name).type, "shared", path)
    assert_path(s, path)
    out = s.delay_cross_spectrum(op, norm_f, pairs, scale=scale, calibrated=calibrated, bin_of_pair=bins, nbins=nbins, per_pair=True)
    assert_path(s, path)
    after = afterwards(s)
    s.close()
    return out, after


@pytest.mark.parametrize("calibrated", [False, True], ids=["raw", "calibrated"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_pairs_across_adjacent_slices_on_the_dense_path(dtype, calibrated):
    """Both paths against the restatement (``bound_ratio <= 1`` in tests/test_gpu_delay_cross.py's ``check``), ``dense`` against
    ``general`` to the bit -- fit quality afterwards too --, the reversed pair against the forward one to the bit."""
    name = np.dtype(dtype).name
    full, p0, pars = cross_slice_problem()
    nb = p0.nbls
    pairs, scale, bins, nbins, forward, rev, bb = cross_slice_pairs(nb)
    # every slice draws its own flags: the common mask of a pair is neither row's own
    m0, m1 = full.wgts[pairs[:, 0]] != 0, full.wgts[pairs[:, 1]] != 0
    own = np.any((m0 & m1) != m0, axis=1) & np.any((m0 & m1) != m1, axis=1)
    assert own[: 2 * nb].sum() > nb and not own[bb]
    op, norm_f = DS.operator(200, 200)
    ref = DC.reference(full, p0, pars, dtype, op, norm_f, pairs, scale, calibrated, bins, nbins)
    got = {}
    for path in ("general", "dense"):
        out, after = cross_slices(name, path, calibrated)
        DC.check(out, ref, dtype, f"adjacent slices {path} {name} calibrated={calibrated}", bins=bins, nbins=nbins)
        for st in DC.STATS:
            for k in DC.NAMES:
                np.testing.assert_array_equal(out["per_pair"][st][k][rev], out["per_pair"][st][k][forward], err_msg=f"{path} {st} {k}: the reversed pair")
            assert np.all(np.abs(out["per_pair"][st]["resid"][: 2 * nb]).max(axis=1) > 0), (path, st)
        assert not np.any(out["per_pair"]["diff"]["data"][bb]) and np.all(out["norm_pair"] > 0)
        got[path] = dict(C.flat(out), **{k: v for k, v in after.items() if k.startswith("quality_")})
    assert_same_bits(got["dense"], got["general"], f"adjacent slices {name} calibrated={calibrated}")
