"""The one Gram solve of the initial foreground coefficients (``slice_pipeline.gram_solve``: what ``calibration._init_coeffs`` and the
batches' own copy became) against ``np.linalg.solve`` with every fitting group's Gram matrix, on a redundant array small enough for
NumPy.  No device is touched."""
import numpy as np
import pytest

from calamity_amd import calibration, modeling, slice_pipeline, synthetic


@pytest.fixture(scope="module")
def prob():
    uvd, _, _ = synthetic.make_uvdata(nants=4, nfreqs=16, ntimes=1, seed=2, redundant=True)
    vecs = modeling.yield_pbl_dpss_model_comps(uvd, offset=2.0 / 0.3, min_dly=2.0 / 0.3, use_redundancy=True)  # groups of 2, 1, 2, 1 baselines
    ants_map = {int(a): i for i, a in enumerate(np.unique(np.concatenate([uvd.ant_1_array, uvd.ant_2_array])))}
    return calibration.tensorize_fg_model_comps_dict(vecs, ants_map, 16, use_redundancy=True, dtype=np.float64)[0]


def _grams(prob):
    """Every fitting group's ``sum_bl A_bl^T A_bl``, straight from the problem's arrays."""
    F, out = prob.nfreqs, []
    for g in range(prob.ngrps):
        blk = prob.basis[prob.grp_basis[g]]
        out.append(sum(blk[rb * F : (rb + 1) * F].T @ blk[rb * F : (rb + 1) * F] for rb in prob.bl_rowblk[prob.grp_bl_start[g] : prob.grp_bl_start[g + 1]]))
    return out


@pytest.mark.parametrize("nt", [1, 3])
def test_gram_solve_equals_numpy_group_by_group(prob, nt):
    grams = _grams(prob)
    identity = [np.allclose(G, np.eye(len(G)), atol=1e-9) for G in grams]
    assert any(identity) and not all(identity)  # the array has redundant groups and lone baselines
    rng = np.random.default_rng(nt)
    c_r, c_i = rng.standard_normal(nt * prob.ncoeffs), rng.standard_normal(nt * prob.ncoeffs)
    s_r, s_i = slice_pipeline.gram_solve(prob, c_r.copy(), c_i.copy(), nt)
    for t in range(nt):
        for g, G in enumerate(grams):
            sel = slice(t * prob.ncoeffs + prob.grp_coff[g], t * prob.ncoeffs + prob.grp_coff[g + 1])
            for got, src in ((s_r, c_r), (s_i, c_i)):
                if identity[g]:
                    assert np.array_equal(got[sel], src[sel])  # left alone, to the bit
                else:
                    np.testing.assert_allclose(got[sel], np.linalg.solve(G, src[sel]), rtol=1e-12)


def test_without_a_gram_to_solve_the_inputs_come_back():
    uvd, _, vecs = synthetic.make_uvdata(nants=4, nfreqs=16, ntimes=1, seed=2)
    ants_map = {int(a): i for i, a in enumerate(np.unique(np.concatenate([uvd.ant_1_array, uvd.ant_2_array])))}
    prob = calibration.tensorize_fg_model_comps_dict(vecs, ants_map, 16, dtype=np.float64)[0]
    c = np.arange(prob.ncoeffs, dtype=np.float32)
    s_r, s_i = slice_pipeline.gram_solve(prob, c, c)
    assert s_r is c and s_i is c
    assert calibration._init_coeffs is slice_pipeline.init_coeffs
