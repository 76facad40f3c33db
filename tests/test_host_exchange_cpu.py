"""The in-process exchange of workers that share a GPU (batched._HostExchange), without a GPU: matched calls reduce in rank order
as before; calls that differ in size, dtype or reduction raise the same error on EVERY worker at once, instead of pairing
unrelated buffers or leaving a worker waiting at a barrier."""
import threading

import numpy as np
import pytest

from calamity_amd.batched import ExchangeMismatch, _HostExchange


def run_workers(n, arrays, ops):
    """Worker r calls the exchange with (arrays[r], ops[r]) on its own thread; returns (arrays after the call, exceptions)."""
    ex = _HostExchange(n)
    errs = [None] * n

    def work(r):
        try:
            ex.hook(r)(arrays[r], ops[r])
        except BaseException as e:  # noqa: BLE001 -- checked by the caller
            errs[r] = e

    threads = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(n)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=60)
    assert not any(t.is_alive() for t in threads), "a worker is still waiting in the exchange"
    return arrays, errs, ex


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_matched_calls_sum_in_rank_order(n, dtype):
    rng = np.random.default_rng(n)
    src = [rng.standard_normal(37).astype(dtype) for _ in range(n)]
    want = src[0].copy()
    for r in range(1, n):
        want += src[r]
    arrays, errs, ex = run_workers(n, [a.copy() for a in src], ["sum"] * n)
    assert errs == [None] * n and ex.error is None
    for a in arrays:
        np.testing.assert_array_equal(a, want)  # the same arithmetic, in rank order, on every worker


@pytest.mark.parametrize("n", [2, 3])
def test_matched_calls_min(n):
    src = [np.asarray([5 - r, 2 + r, 7, -r], dtype=np.int32) for r in range(n)]
    arrays, errs, _ = run_workers(n, [a.copy() for a in src], ["min"] * n)
    assert errs == [None] * n
    for a in arrays:
        np.testing.assert_array_equal(a, np.minimum.reduce(src))


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("what", ["size", "dtype", "op"])
def test_mismatched_calls_raise_on_every_worker(n, what):
    odd = n - 1  # the last worker differs
    arrays = [np.ones(16, dtype=np.float64) for _ in range(n)]
    ops = ["sum"] * n
    if what == "size":
        arrays[odd] = np.ones(8, dtype=np.float64)
    elif what == "dtype":
        arrays[odd] = np.ones(16, dtype=np.float32)
    else:
        ops[odd] = "min"
    before = [a.copy() for a in arrays]
    arrays, errs, ex = run_workers(n, arrays, ops)
    assert all(isinstance(e, ExchangeMismatch) for e in errs), errs
    assert len({str(e) for e in errs}) == 1  # the same message on every worker ...
    msg = str(errs[0])
    for r in range(n):  # ... naming every worker's call
        assert f"rank {r}: dtype {arrays[r].dtype.str}, {arrays[r].size} elements, {ops[r]}" in msg, msg
    assert ex.error is not None and str(ex.error) == msg
    for a, b in zip(arrays, before):
        np.testing.assert_array_equal(a, b)  # nothing was reduced


def test_the_exchange_is_usable_again_after_matched_calls():
    """Two rounds in a row on the same exchange (the barrier cycles back): both reduce."""
    ex = _HostExchange(2)
    out = [[None, None], [None, None]]

    def work(r):
        h = ex.hook(r)
        for k in range(2):
            a = np.full(4, float(r + 1 + 10 * k))
            h(a, "sum")
            out[k][r] = a

    threads = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=60)
    assert not any(t.is_alive() for t in threads)
    for r in range(2):
        np.testing.assert_array_equal(out[0][r], np.full(4, 3.0))
        np.testing.assert_array_equal(out[1][r], np.full(4, 23.0))
