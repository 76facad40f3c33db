"""Which basis blocks the streaming kernel may fold (`cal_basis_foldable`, host only: no device is touched).

A block is foldable when its upper half band is the lower half read backwards with alternating sign,
A[F-1-f, k] = (-1)^k A[f, k], as the discrete prolate spheroidal sequences of `modeling.dpss_windows` are.  fp32: to half a
unit in the last place of the block's largest element (what the cast from fp64 leaves); fp64: exactly.
"""
import ctypes as C

import numpy as np
import pytest

from calamity_amd import _lib, modeling, synthetic

F32, F64 = 0, 1
ULP32 = 2.0**-23


def foldable(block, dtype):
    """(verdict, largest mirror residual, largest |A|) of a [nrowblk * nfreqs][nvec] block given as [rows, nvec] with nfreqs = rows."""
    return foldable_rows(block, dtype, block.shape[0], 1)


def foldable_rows(block, dtype, nfreqs, nrowblk):
    lib = _lib.load()
    a = np.ascontiguousarray(block, dtype=np.float32 if dtype == F32 else np.float64)
    resid, amax = C.c_double(), C.c_double()
    r = lib.cal_basis_foldable(dtype, a.ctypes.data_as(C.c_void_p), nfreqs, a.shape[1], nrowblk, C.byref(resid), C.byref(amax))
    assert r in (0, 1), _lib.load().cal_last_error()
    return bool(r), resid.value, amax.value


@pytest.fixture(scope="module")
def hera350_blocks():
    """The unique basis blocks of the hera350 configuration (one per distinct delay), as synthetic.make_problem builds them."""
    nants, nfreqs, f0, df = synthetic.CONFIGS["hera350"]
    freqs = f0 + df * np.arange(nfreqs)
    antpos = synthetic.hex_positions(nants)
    i_idx, j_idx = np.triu_indices(nants, k=1)
    lengths = np.linalg.norm(antpos[i_idx] - antpos[j_idx], axis=1)
    dlys = np.asarray([modeling.dly_ns(L) for L in lengths])
    uniq = np.unique(dlys)
    cache = {}
    return [modeling.yield_dpss_model_comps_bl_grp(lengths[np.where(dlys == d)[0][0]], freqs, operator_cache=cache) for d in uniq]


def test_every_hera350_block_folds_in_fp32_and_none_in_fp64(hera350_blocks):
    assert len(hera350_blocks) == 120
    worst = 0.0
    for b in hera350_blocks:
        ok, resid, amax = foldable(b, F32)
        worst = max(worst, resid / (ULP32 * amax))
        assert ok and resid <= 0.5 * ULP32 * amax, (b.shape, resid, amax)
    print(f"largest fp32 mirror residual: {worst:.3f} ulp of the block's largest element")
    assert worst <= 0.5
    n64 = sum(foldable(b, F64)[0] for b in hera350_blocks)
    print(f"fp64 blocks that fold as built: {n64} of {len(hera350_blocks)}")
    assert n64 == 0


def symmetrised(b):
    """The block with its upper half band replaced by the mirrored lower half: exactly symmetric in any precision."""
    out = np.array(b, dtype=np.float64)
    F = out.shape[0]
    sign = np.where(np.arange(out.shape[1]) % 2 == 0, 1.0, -1.0)
    out[F - F // 2:] = out[: F // 2][::-1] * sign
    return out


def test_exactly_symmetric_fp64_block_folds(hera350_blocks):
    b = symmetrised(hera350_blocks[3])
    ok, resid, _ = foldable(b, F64)
    assert ok and resid == 0.0
    assert foldable(b, F32)[0]


def test_blocks_that_must_not_fold(hera350_blocks):
    rng = np.random.default_rng(0)
    assert not foldable(rng.standard_normal((1024, 40)), F32)[0]
    assert not foldable(rng.standard_normal((1024, 40)), F64)[0]
    # one vector with the wrong sign pattern (an even vector made antisymmetric)
    b = symmetrised(hera350_blocks[5])
    b[512:, 2] *= -1.0
    assert not foldable(b, F32)[0] and not foldable(b, F64)[0]
    # the right vectors in another order: symmetric / antisymmetric, but not alternating from an even first vector
    b = symmetrised(hera350_blocks[5])[:, ::-1] if hera350_blocks[5].shape[1] % 2 == 0 else symmetrised(hera350_blocks[5])[:, 1:]
    assert not foldable(b, F32)[0]
    # an odd band has a centre channel of its own
    b = symmetrised(hera350_blocks[5])
    odd = np.concatenate([b[:512], b[511:]])  # 1025 rows, still mirror-symmetric
    assert not foldable(odd, F32)[0] and not foldable(odd, F64)[0]
    # half the band is not a whole number of tiles: 40 vectors take 128-channel tiles in fp32 (64 in fp64); 2 x 96 channels
    small = symmetrised(np.concatenate([b[:96, :40], b[:96, :40]]))
    assert small.shape == (192, 40) and not foldable(small, F32)[0] and not foldable(small, F64)[0]
    # ... while 2 x 128 channels are
    ok256 = symmetrised(np.concatenate([b[:128, :40], b[:128, :40]]))
    assert foldable(ok256, F32)[0] and foldable(ok256, F64)[0]
    # several row blocks per basis block are left alone
    two = np.concatenate([ok256, ok256])
    assert not foldable_rows(two, F32, 256, 2)[0]
    # a non-finite element
    bad = ok256.copy()
    bad[3, 1] = np.nan
    assert not foldable(bad, F32)[0]
