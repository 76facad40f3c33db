"""``delay_spectrum``, ``delay_cross_spectrum`` and ``delay_transfer`` in every order on ONE solver.  The cross spectrum reuses the
spectrum's device buffers (``ds_x``, ``ds_pow``, ``ds_out``, ``ds_op``, ``ds_ent``, ``ds_ptr``, under the one scratch bound) at sizes of
its own -- pairs instead of rows, ``nstat * nq`` planes --, the bins are zeroed by chunk 0's ``dspec_bin_kernel`` alone, and the transfer
runs that kernel too: a call that read what another left behind would show only when calls of DIFFERENT sizes follow one another.

One solver on ``batch(13, 61, 2)`` of tests/test_gpu_delay_cross.py (156 rows, 78 a slice; 84 pairs: one full block of 64 and a ragged
one), default kernel path, both dtypes, three calls of deliberately different sizes:

  * ``delay_spectrum`` at 61 delays, 5 bins over the rows, ``per_baseline``;
  * ``delay_cross_spectrum`` at 37 delays, 4 bins over the pairs, ``per_pair``, both statistics of all three quantities;
  * ``delay_transfer`` at 61 delays, 3 bins over the rows, ``per_baseline``.

All six orders, each followed by a repeat of its first call; two of the orders again with the scratch bound set so that the cross
spectrum runs in chunks of 7 pairs and the spectrum in chunks of fewer rows than it has; and a cross call for the residual's half
difference alone directly behind one for everything (a smaller output that must carry none of the larger one's planes or bins).  Every
output equals, TO THE BIT, the same call made alone on a fresh solver at the default bound.  No tolerance in this file.

Shown once on a scratch copy of the library (wrong numbers, no fault): the cross call skipping its upload of ``ds_ptr`` / ``ds_ent`` when
a spectrum call has filled them.  To stay inside its buffers the wrong build skips only where every stale entry still indexes inside
``ds_out`` and ``ds_pow`` (one chunk, the spectrum's bins no fewer), so its chunked calls are right.  It fails 14 of the 25 tests here:
10 of ``test_every_order_gives_the_bits_of_each_call_alone`` (both dtypes of the five orders in which a spectrum call comes before a
cross call, the repeat of the first call counted; ``transfer > cross > spectrum > transfer`` has none and passes) and the 4 ``whole`` cases
of ``test_a_smaller_cross_call_carries_nothing_of_the_larger_one``; only binned outputs and ``count_bin`` are wrong.  It passes every
other test of the three report suites and tests/test_gpu_delay_cross.py, test_gpu_delay_cross_dropin.py and
test_gpu_delay_cross_ranks.py as they stood before this file (60 tests), none of which makes a spectrum call before a binned cross call."""
import functools
import itertools

import numpy as np
import pytest

import report_cases as C
import test_gpu_delay_cross as DC
from test_gpu_solve_paths import assert_same_bits

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
NAMES = ("spectrum", "cross", "transfer")
ORDERS = list(itertools.permutations(NAMES))
CHUNKED = [("spectrum", "cross", "transfer"), ("transfer", "cross", "spectrum")]


def setup():
    full, p0, pars = DC.batch(13, 61, 2)
    assert (p0.nbls, full.nbls) == (78, 156)
    return full, p0, pars


def calls(full, p0):
    """The three calls, by name: functions of a solver that return the flat output."""
    op61, norm_f = DC.operator(61, 61)
    op37, _ = DC.operator(61, 37)
    rows = np.arange(full.nbls)
    bins5 = (rows % 4).astype(np.int32)  # bin 4 stays empty
    bins5[7] = -1
    bins3 = (rows % 3).astype(np.int32)
    pairs, scale, _ = DC.pair_list(p0.nbls, 2)
    assert len(pairs) == 84
    bins4, nbins4 = DC.bins_of_pairs(len(pairs))
    cross_kw = dict(scale=scale, bin_of_pair=bins4, nbins=nbins4, per_pair=True)
    return {"spectrum": lambda s: C.flat(s.delay_spectrum(op61, norm_f, bin_of_bl=bins5, nbins=5, per_baseline=True)),
            "cross": lambda s: C.flat(s.delay_cross_spectrum(op37, norm_f, pairs, **cross_kw)),
            "cross_small": lambda s: C.flat(s.delay_cross_spectrum(op37, norm_f, pairs, what=("resid",), stats=("diff",), **cross_kw)),
            "transfer": lambda s: C.flat(s.delay_transfer(op61, bin_of_bl=bins3, nbins=3, per_baseline=True))}


def fresh(dtype):
    full, p0, pars = setup()
    return DC.solver_of(full, DC.joined(pars), dtype)


@functools.lru_cache(maxsize=None)
def alone(name, dtype_name):
    """The call ``name`` made alone on a fresh solver at the default scratch bound."""
    full, p0, _ = setup()
    s = fresh(np.dtype(dtype_name).type)
    out = calls(full, p0)[name](s)
    s.close()
    return out


def run_sequence(s, sequence, dtype, label):
    full, p0, _ = setup()
    todo = calls(full, p0)
    for i, name in enumerate(sequence):
        assert_same_bits(todo[name](s), alone(name, np.dtype(dtype).name), f"{label}: call {i} ({name}) of {' > '.join(sequence)}")


def test_the_three_calls_have_three_sizes():
    """What the orders are for: other delays, other bins, other counts of rows, and outputs that are not trivially equal."""
    sp, cr, tr = (alone(k, "float64") for k in NAMES)
    small = alone("cross_small", "float64")
    assert sp["per_baseline_resid"].shape == (156, 61) and sp["resid"].shape == (5, 61) and not np.any(sp["resid"][4]) and np.all(sp["count_bin"][:4] > 0)
    assert cr["per_pair_diff_resid"].shape == (84, 37) and cr["diff_resid"].shape == (4, 37) and np.all(cr["count_bin"][:3] > 0)
    assert tr["absorbed_bl"].shape == (156, 61) and tr["absorbed_bin"].shape == (3, 61) and np.all(tr["count_bin"] > 0)
    assert sorted(small) == ["count_bin", "diff_resid", "norm_pair", "per_pair_diff_resid"]
    for out in (sp, cr, tr):
        assert all(np.all(np.isfinite(v)) for v in out.values() if not np.isscalar(v))
    assert cr["per_pair_cross_data"].max() > 0 and sp["per_baseline_data"].max() > 0 and tr["absorbed_bin"].max() > 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("order", ORDERS, ids="-".join)
def test_every_order_gives_the_bits_of_each_call_alone(order, dtype):
    s = fresh(dtype)
    run_sequence(s, order + order[:1], dtype, np.dtype(dtype).name)
    s.close()


def chunk_bound(dtype):
    """The scratch bound at which the cross call (three quantities, two statistics, 37 delays) runs in chunks of 7 pairs, by the planner's
    rule (tests/test_delay_cross_host.py, tests/test_report_plan_host.py); the spectrum's rows per chunk under it."""
    size, xpitch = np.dtype(dtype).itemsize, 64  # 61 channels: fpad 64, one step of the transform
    pair_bytes = 3 * 2 * 2 * xpitch * size + 2 * 3 * 37 * 8
    bound = 7 * pair_bytes + pair_bytes // 2
    row_bytes = 3 * 2 * xpitch * size + 3 * 61 * 8
    return bound, bound // pair_bytes, bound // row_bytes


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("order", CHUNKED, ids="-".join)
def test_two_orders_in_chunks_of_seven_pairs(order, dtype):
    bound, cpairs, crows = chunk_bound(dtype)
    assert cpairs == 7 and 84 // cpairs == 12 and 1 <= crows <= 13  # twelve chunks of pairs; twelve or more of rows
    s = fresh(dtype)
    s._set_delay_spectrum_scratch(bound)
    run_sequence(s, order + order[:1], dtype, f"{np.dtype(dtype).name} in chunks")
    s._set_delay_spectrum_scratch(0)
    run_sequence(s, order[:1], dtype, f"{np.dtype(dtype).name} back at the default bound")
    s.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("order", CHUNKED, ids="-".join)
@pytest.mark.parametrize("chunked", [False, True], ids=["whole", "chunks"])
def test_a_smaller_cross_call_carries_nothing_of_the_larger_one(order, dtype, chunked):
    """``stats=("diff",)``, ``what=("resid",)`` directly behind the call for everything: one plane where six were, one set of bins where
    six were, other chunk sizes under the same bound."""
    at = order.index("cross") + 1
    sequence = order[:at] + ("cross_small",) + order[at:] + ("cross", "cross_small")
    s = fresh(dtype)
    if chunked:
        s._set_delay_spectrum_scratch(chunk_bound(dtype)[0])
    run_sequence(s, sequence, dtype, f"{np.dtype(dtype).name} {'in chunks' if chunked else 'whole'}")
    s._set_delay_spectrum_scratch(0)
    s.close()
