"""The rows of the exact robust-weight tests (tests/test_gpu_robust_exact.py on the device, tests/test_robust_host.py for the two
selectors of tests/robust_ref.py): NumPy only.  Every builder returns ``(d_r, d_i, w0)``, arrays ``[rows, nfreqs]`` of the solver's
dtype.  With the foreground coefficients at zero the device's ``e`` is ``robust_ref.residual_power_exact`` of them, so a row is stated
through the ``e`` it gives:

* data 1 + 0j and ``w0 = x`` give ``e = x`` to the bit for any ``x > 0`` (``x * (1 * 1 + 0 * 0)``);
* ``w0 = 1`` and data ``d`` give ``e = d_r * d_r + d_i * d_i`` as the dtype rounds it: zero, subnormal, +inf, NaN;
* ``w0 = 0`` flags a sample.  Flagged samples carry data of 1e3 and more, and a selector that counted them would move the median.

``V`` is the number of channels a lane owns per trip (16 bytes) and ``W = 64 V`` the channels a wave covers per trip: 256 in float32, 128
in float64."""
import numpy as np


def lanes(dtype):
    v = 16 // np.dtype(dtype).itemsize
    return v, 64 * v


def _flag(rng, d_r, d_i, w0, idx):
    """Flag the channels ``idx`` of one row and give them large data."""
    w0[idx] = 0
    d_r[idx] = 1e3 * (1.0 + rng.random(len(idx)))
    d_i[idx] = -1e3 * (1.0 + rng.random(len(idx)))


def _new(nrows, nfreqs, dtype):
    return np.ones((nrows, nfreqs), dtype=dtype), np.zeros((nrows, nfreqs), dtype=dtype), np.ones((nrows, nfreqs), dtype=dtype)


def spaced(rng, n, dtype):
    """``n`` distinct positive numbers of ``dtype`` in random order, neighbours at least 1e-3 relative apart."""
    x = np.cumprod(1.0 + rng.uniform(1e-3, 2e-2, n)).astype(dtype)
    assert len(np.unique(x)) == n
    return rng.permutation(x)


def one_ulp_middle(rng, n, dtype):
    """``n`` (even) positive numbers whose two middle order statistics are neighbours in ``dtype``; returns (row, the lower one).  The
    lower one is 0.6: its quotient by ln 2 lies in the same binade, where the quotients of two neighbours are 1.44 ulp apart and differ."""
    assert n % 2 == 0
    lo = rng.uniform(0.1, 0.5, n // 2 - 1).astype(dtype)
    x = np.asarray(0.6, dtype=dtype)
    hi = rng.uniform(1.0, 4.0, n // 2 - 1).astype(dtype)
    row = np.concatenate([lo, [x, np.nextafter(x, np.asarray(2, dtype=dtype))], hi]).astype(dtype)
    return rng.permutation(row), x


def first_of_a_run(rng, n, dtype):
    """``n`` (odd) positive numbers whose median is the first of a run of 21 equal values (0.6) and whose next smaller order statistic
    is the neighbour below it."""
    assert n % 2 == 1 and n >= 45
    rank = (n + 1) // 2
    x = np.asarray(0.6, dtype=dtype)
    lo = rng.uniform(0.1, 0.5, rank - 2).astype(dtype)
    hi = rng.uniform(1.0, 4.0, n - (rank - 1) - 21).astype(dtype)
    row = np.concatenate([lo, [np.nextafter(x, np.asarray(0, dtype=dtype))], np.full(21, x), hi]).astype(dtype)
    return rng.permutation(row)


def ties(nfreqs, dtype, seed=1):
    """Five rows.  0: data quantised to the integers of [-3, 3], ``w0 = 1``: ``e`` takes about ten values.  1: the same with 30 % flagged.
    2: one repeated value.  3: ``n_b`` even, the two middle order statistics one ulp apart (``nfreqs`` even).  4: ``n_b = nfreqs - 1`` odd, the
    median the first of a run of equal values and the sample below it one ulp smaller."""
    rng = np.random.default_rng(seed)
    d_r, d_i, w0 = _new(5, nfreqs, dtype)
    for b in (0, 1):
        d_r[b] = rng.integers(-3, 4, nfreqs)
        d_i[b] = rng.integers(-3, 4, nfreqs)
    _flag(rng, d_r[1], d_i[1], w0[1], np.flatnonzero(rng.random(nfreqs) < 0.3))
    d_r[2], d_i[2] = 1.5, -0.5
    w0[3] = one_ulp_middle(rng, nfreqs, dtype)[0]
    at = rng.permutation(nfreqs)
    w0[4, at[1:]] = first_of_a_run(rng, nfreqs - 1, dtype)
    _flag(rng, d_r[4], d_i[4], w0[4], at[:1])
    return d_r, d_i, w0


def counts(nfreqs, dtype, seed=2):
    """Eight rows of ``nfreqs`` = W + 1 or 2 W + 3 channels whose good samples have distinct ``e``; (n_b, where): see ``count_plan``."""
    rng = np.random.default_rng(seed)
    plan = count_plan(nfreqs, dtype)
    d_r, d_i, w0 = _new(len(plan), nfreqs, dtype)
    for b, good in enumerate(plan):
        good = np.arange(nfreqs) if good is None else np.asarray(good)
        if good[0] < 0:  # (-n: n channels at random)
            good = np.sort(rng.permutation(nfreqs)[: -good[0]])
        w0[b, good] = spaced(rng, len(good), dtype)
        _flag(rng, d_r[b], d_i[b], w0[b], np.setdiff1d(np.arange(nfreqs), good))
    return d_r, d_i, w0


def count_plan(nfreqs, dtype):
    """The good channels of each row of ``counts``: a list of channels, ``[-n]`` for n channels at random, ``None`` for all."""
    v, w = lanes(dtype)
    last = nfreqs - 1
    if nfreqs == w + 1:  # the second trip holds channel W alone
        return [[last], [0], [0, last], [-2], [-3], [-(w - 1)], [-w], None]
    assert nfreqs == 2 * w + 3  # the last three channels are the partly filled end of the third trip
    return [[last], [0], [last - 1, last], [last - 2, last - 1, last], [-(w - 1)], [-w], [-(w + 1)], [-(2 * w)]]


def whole_range(nfreqs, dtype, seed=3):
    """Four rows.  0: ``w0 = 1``, ``d_i = 0``, ``|d_r|`` log-uniform from a quarter of the square root of the smallest subnormal to the
    largest number of the dtype, signs at random: ``e`` is zero for a few samples, subnormal, normal, and +inf for about a third.  1: the
    same with 30 % flagged.  2: keys that share every bit but the lowest eight.  3: such keys with 30 % flagged."""
    rng = np.random.default_rng(seed)
    fi = np.finfo(dtype)
    d_r, d_i, w0 = _new(4, nfreqs, dtype)
    lo = 0.5 * np.log2(float(fi.smallest_subnormal)) - 2.0
    hi = np.log2(float(fi.max))
    for b in (0, 1):
        mag = np.exp2(rng.uniform(lo, hi, nfreqs)).astype(dtype)
        mag[:3] = np.sqrt(np.asarray(fi.tiny, dtype=np.float64)) * np.array([2.0**-2, 2.0**-5, 2.0**-9])  # e = tiny 2^-4, 2^-10, 2^-18: subnormal
        d_r[b] = rng.permutation(mag) * rng.choice([-1.0, 1.0], nfreqs)
    _flag(rng, d_r[1], d_i[1], w0[1], np.flatnonzero(rng.random(nfreqs) < 0.3))
    ut = {4: np.uint32, 8: np.uint64}[np.dtype(dtype).itemsize]
    for b in (2, 3):
        base = np.array([1.2345678901234567], dtype=dtype).view(ut)[0] & ~ut(0xFF)
        w0[b] = (base | rng.integers(0, 256, nfreqs).astype(ut)).view(dtype)
    _flag(rng, d_r[3], d_i[3], w0[3], np.flatnonzero(rng.random(nfreqs) < 0.3))
    return d_r, d_i, w0


def zero_median(nfreqs, dtype, seed=4):
    """Four rows under ``w0`` uniform in [0.5, 1.5] with 20 % flagged; the rest of ``S_b`` has distinct ``e > 0``.  0: more than half of
    ``S_b`` has zero data.  1: ``n_b`` even, exactly half zero (the lower median is the zero).  2: ``n_b`` even, half minus one zero (the
    median is the smallest positive sample).  3: ``n_b`` odd, (n_b + 1) / 2 zero."""
    rng = np.random.default_rng(seed)
    d_r, d_i, w0 = _new(4, nfreqs, dtype)
    for b in range(4):
        w0[b] = rng.uniform(0.5, 1.5, nfreqs)
        d_r[b] = np.sqrt(spaced(rng, nfreqs, np.float64))
        d_i[b] = -0.5 * d_r[b]
        n = int(0.8 * nfreqs) // 2 * 2 - (b == 3)
        good = rng.permutation(nfreqs)
        _flag(rng, d_r[b], d_i[b], w0[b], good[n:])
        nzero = {0: n // 2 + 5, 1: n // 2, 2: n // 2 - 1, 3: (n + 1) // 2}[b]
        d_r[b, good[:nzero]] = 0
        d_i[b, good[:nzero]] = 0
    return d_r, d_i, w0


def non_finite(nfreqs, dtype, seed=5):
    """Four rows, ``w0`` uniform in [0.5, 1.5] with 20 % flagged, finite data of order one elsewhere.  0: 30 % of ``S_b`` NaN (in ``d_r``,
    ``d_i`` or both) and five infinite samples.  1: ``n_b`` even, exactly n_b / 2 NaN: the median is the largest number of the row.
    2: n_b / 2 + 1 NaN: the median is a NaN.  3: all of ``S_b`` but two samples NaN."""
    rng = np.random.default_rng(seed)
    d_r, d_i, w0 = _new(4, nfreqs, dtype)
    for b in range(4):
        w0[b] = rng.uniform(0.5, 1.5, nfreqs)
        d_r[b] = rng.standard_normal(nfreqs)
        d_i[b] = rng.standard_normal(nfreqs)
        n = int(0.8 * nfreqs) // 2 * 2
        good = rng.permutation(nfreqs)
        _flag(rng, d_r[b], d_i[b], w0[b], good[n:])
        nnan = {0: int(0.3 * n), 1: n // 2, 2: n // 2 + 1, 3: n - 2}[b]
        third = nnan // 3
        d_r[b, good[: 2 * third]] = np.nan
        d_i[b, good[third:nnan]] = np.nan
        if b == 0:
            d_r[b, good[nnan : nnan + 3]] = np.inf
            d_i[b, good[nnan + 3 : nnan + 5]] = -np.inf
    return d_r, d_i, w0


def lds_limit(nfreqs, dtype, seed=6):
    """Four rows at the longest row of the LDS form (4096 channels in float32, 2048 in float64): quantised data, the middle pair one ulp
    apart, the whole exponent range, the whole range with 30 % flagged."""
    t = ties(nfreqs, dtype, seed)
    r = whole_range(nfreqs, dtype, seed + 1)
    return tuple(np.concatenate([a[[0, 3]], b[[0, 1]]]) for a, b in zip(t, r))


def one_more_flagged_channel(rows, seed=7):
    """The same rows with one channel appended that is flagged and carries large data: ``S_b`` and ``e`` on it do not change."""
    rng = np.random.default_rng(seed)
    d_r, d_i, w0 = (np.concatenate([a, np.zeros((len(a), 1), dtype=a.dtype)], axis=1) for a in rows)
    d_r[:, -1] = 1e3 * (1.0 + rng.random(len(d_r)))
    d_i[:, -1] = -1e3 * (1.0 + rng.random(len(d_r)))
    return d_r, d_i, w0


def short_families(dtype):
    """name -> rows, for the short-row cases of both dtypes."""
    v, w = lanes(dtype)
    return {"ties": ties(200, dtype), "counts_W+1": counts(w + 1, dtype), "counts_2W+3": counts(2 * w + 3, dtype),
            "whole_range": whole_range(300, dtype), "zero_median": zero_median(200, dtype), "non_finite": non_finite(200, dtype)}


def all_families(dtype):
    n = 65536 // (4 * np.dtype(dtype).itemsize)
    return dict(short_families(dtype), lds_limit=lds_limit(n, dtype))
