"""The set-up planner on the host (`cal_debug_plan`: calamity_amd/csrc/problem_plan.hpp run with no device).

Every array and scalar it produces for the seeded problems of tests/_plan_cases.py equals, byte for byte, what the solver of
commit b726cc4 -- where set-up was one function that planned and uploaded in one go -- held on the device after
`set_problem` (tests/golden/plan/*.npz, read back from its buffers on an MI355X).  Item and panel order decide the order of
floating-point partial sums, so an unchanged plan is what keeps results bit for bit.  Arrays the earlier code never kept are
covered through what they produce: the operand offsets of the pack kernels through `PanelItem::a_kf4`; the item tables it uploaded
only for problems whose groups are cut into several items are compared for those problems.

Every refusal of the planner gives the code and the message of the earlier set-up (texts copied from it)."""
import ctypes as C
import os

import numpy as np
import pytest

import _plan_cases as pc
from calamity_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan")


@pytest.mark.parametrize("name", list(pc.CASES))
def test_plan_equals_recorded(name):
    gold = np.load(os.path.join(GOLDEN, name + ".npz"))
    assert str(gold["parent"]) == "b726cc4"
    prob, dtype, layout, kernel_path = pc.CASES[name]()
    got = pc.plan(_lib.load(), prob, dtype, layout, kernel_path)
    want = {nm for nm, _ in pc.ARRAYS.values()} - {"op_off"}
    scalars = dict(zip(pc.SCALARS, gold["scalars"].tolist()))
    if scalars["gc_direct"]:
        want -= {"item_goff", "grp_item_ptr", "coef_grp"}
    assert set(gold.files) - {"parent"} == want
    for nm in sorted(want):
        assert got[nm].dtype == gold[nm].dtype and got[nm].shape == gold[nm].shape, nm
        if nm == "scalars":
            diff = [(k, a, b) for k, a, b in zip(pc.SCALARS, got[nm].tolist(), gold[nm].tolist()) if a != b]
            assert not diff, diff
        assert got[nm].tobytes() == gold[nm].tobytes(), (nm, np.flatnonzero(got[nm] != gold[nm])[:8])


def _scalars(name):
    return dict(zip(pc.SCALARS, np.load(os.path.join(GOLDEN, name + ".npz"))["scalars"].tolist()))


def test_cases_reach_the_branches():
    """The recorded plans are of the kind each case is there for."""
    s = _scalars("stream_fold_f32")
    fb = np.load(os.path.join(GOLDEN, "stream_fold_f32.npz"))["fb"]
    assert s["fold"] and not s["gc_direct"] and not s["small_loads"] and len(set(fb.tolist())) >= 3
    assert not _scalars("stream_full_f32")["fold"] and not _scalars("stream_f64")["fold"]
    assert _scalars("stream_200_f32")["fpad"] == 256 and not _scalars("stream_200_f32")["fold"]
    for nm in ("groups_stream_f32", "groups_shared_f64"):
        g = np.load(os.path.join(GOLDEN, nm + ".npz"))
        runs = g["runs"].reshape(-1, 2)
        assert (runs[:, 1] - runs[:, 0]).max() == 256 and _scalars(nm)["nitems_simple"] == 1
    s = _scalars("alias_3_f32")
    assert s["nheads_mfma"] >= 64 and s["nheads"] > s["nheads_mfma"] and s["mm_grid"] % 8 == 0 and not s["heads_one_pass_local"]
    s = _scalars("alias_10_f64")
    assert s["nheads_mfma"] >= 64 and s["nheads"] > s["nheads_mfma"] and s["nitems_plain"] == 5  # two lone leftovers; the two copies that own their tiles, one of them cut in two
    for nm, split, split2 in (("dense_split2_f32", 1, 1), ("dense_split1_f32", 1, 0), ("dense_f32_f32", 0, 0), ("dense_240_f32", 0, 0), ("dense_f64", 0, 0)):
        s = _scalars(nm)
        assert s["mf_ok"] and s["mf_split"] == split and s["mf_split2"] == split2 and s["nslices"] == 2, nm
    assert _scalars("shared_auto_2080_f32")["mf_ok"] and not _scalars("shared_auto_1000_f32")["mf_ok"]
    assert _scalars("grp_var_ordered_f32")["lamb_ok"] and not _scalars("grp_var_unordered_f32")["lamb_ok"]


def _base():
    """Three single-baseline groups over two blocks (4 and 9 vectors), 4 antennas, 64 channels."""
    return dict(nants=4, nfreqs=64, ngrps=3, nbls=3, nbasis=2, layout=_lib.CAL_LAYOUT_STREAM, kernel_path=_lib.CAL_PATH_AUTO, nslices=1,
                basis_offset=np.asarray([0, 256, 832], np.int64), basis_nvec=np.asarray([4, 9], np.int32), basis_nrowblk=np.asarray([1, 1], np.int32),
                basis_data=np.ones(832 + 64 * 897, np.float64), grp_basis=np.asarray([0, 1, 0], np.int32), grp_bl_start=np.asarray([0, 1, 2, 3], np.int32),
                bl_ant0=np.asarray([0, 0, 1], np.int32), bl_ant1=np.asarray([1, 2, 2], np.int32), bl_rowblk=np.zeros(3, np.int32), bl_alias=None, grp_var=None)


INV, UNS = _lib.CAL_ERR_INVALID, _lib.CAL_ERR_UNSUPPORTED
two_slices = dict(nslices=2)
REFUSALS = {
    "dimension": (dict(nants=0), "f32", INV, "set_problem: non-positive dimension"),
    "null": (dict(bl_ant1=None), "f32", INV, "set_problem: null pointer in problem description"),
    "layout": (dict(layout=2), "f32", INV, "set_problem: bad layout"),
    "grp_bl_start": (dict(grp_bl_start=[1, 1, 2, 3]), "f32", INV, "set_problem: grp_bl_start must run from 0 to nbls"),
    "empty_block": (dict(basis_nvec=[4, 0]), "f32", INV, "set_problem: empty basis block 1"),
    "block_size": (dict(basis_offset=[0, 256, 833]), "f32", INV, "set_problem: basis block 1 has 577 elements, expected 576"),
    "too_wide": (dict(basis_nvec=[4, 897], basis_offset=[0, 256, 256 + 64 * 897]), "f32", UNS,
                 "set_problem: basis block 1 has 897 vectors; at most 896 are supported for this dtype"),
    "kernel_path": (dict(kernel_path=9), "f32", INV, "set_problem: bad kernel_path 9"),
    "dense_f32_in_f64": (dict(kernel_path=_lib.CAL_PATH_DENSE_F32), "f64", UNS,
                         "set_problem: CAL_PATH_DENSE_F32 is the fp32 kernel on v_mfma_f32_32x32x2_f32; this solver is fp64"),
    "split1_in_f64": (dict(kernel_path=_lib.CAL_PATH_DENSE_SPLIT1), "f64", UNS,
                      "set_problem: CAL_PATH_DENSE_SPLIT1 is an fp32 kernel (split-bf16 operands); this solver is fp64"),
    "dense_refused": (dict(kernel_path=_lib.CAL_PATH_DENSE), "f32", UNS,
                      "set_problem: CAL_PATH_DENSE needs the SHARED layout, one baseline per fitting group, basis_nvec <= 256 and nfreqs > 64"),
    "antenna": (dict(bl_ant1=[1, 2, 4]), "f32", INV, "set_problem: baseline 2 has an antenna index outside [0, 4)"),
    "too_many_slices": (dict(nslices=257), "f32", UNS, "set_problem: 257 time slices; at most 256 are supported"),
    "slices_divide": (dict(nslices=3), "f32", INV, "set_problem: nants = 4 is not a multiple of nslices = 3"),
    "slice_empty_group": (dict(two_slices, grp_bl_start=[0, 1, 1, 3]), "f32", INV, "set_problem: group 1 has no baselines"),
    "leaves_slice": (dict(two_slices), "f32", INV, "set_problem: baseline 1 of group 1 leaves time slice 0 (antennas 0, 2; 2 antennas per slice)"),
    "slice_order": (dict(two_slices, bl_ant0=[2, 0, 0], bl_ant1=[3, 1, 1]), "f32", INV, "set_problem: fitting groups must be listed slice by slice (group 1)"),
    "slice_unused": (dict(two_slices, bl_ant0=[0, 0, 0], bl_ant1=[1, 1, 1]), "f32", INV, "set_problem: time slice 1 has no fitting group"),
    "grp_basis": (dict(grp_basis=[0, 1, 2]), "f32", INV, "set_problem: group 2 points at basis 2"),
    "empty_group": (dict(grp_bl_start=[0, 1, 1, 3]), "f32", INV, "set_problem: group 1 has no baselines"),
    "rowblk": (dict(bl_rowblk=[0, 1, 0]), "f32", INV, "set_problem: baseline 1 row block 1 out of range"),
    "grp_var": (dict(grp_var=[0, -1, 0]), "f32", INV, "set_problem: grp_var[1] = -1 is negative"),
    "alias_owner": (dict(bl_alias=[-1, 5, -1]), "f32", INV, "set_problem: bl_alias[1] = 5 must name a baseline that owns its tiles"),
    "alias_rows": (dict(bl_alias=[-1, 0, -1]), "f32", INV, "set_problem: bl_alias[1] = 0: the two baselines use different basis rows"),
    "alias_group": (dict(ngrps=2, grp_basis=[0, 0], grp_bl_start=[0, 2, 3], bl_alias=[-1, -1, 0]), "f32", INV,
                    "set_problem: bl_alias is for single-baseline fitting groups (baseline 2)"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusal_code_and_message(name):
    """One refusal per fail() of the planner, in the order of its checks (the tile-width check against the row padding is an
    internal error no description reaches)."""
    change, dt, code, message = REFUSALS[name]
    f = _base()
    for k, v in change.items():
        f[k] = v if v is None or np.isscalar(v) else np.asarray(v, f[k].dtype if f[k] is not None else np.int32)
    f["basis_data"] = f["basis_data"].astype(np.float32 if dt == "f32" else np.float64)
    d = _lib.ProblemDesc(**{k: (v if v is None or np.isscalar(v) else v.ctypes.data_as(C.c_void_p)) for k, v in f.items()})
    lib = _lib.load()
    buf, n = np.empty(4096, np.uint8), C.c_int64(0)
    rc = lib.cal_debug_plan(_lib.CAL_F32 if dt == "f32" else _lib.CAL_F64, C.byref(d), 0, buf.ctypes.data_as(C.c_void_p), buf.nbytes, C.byref(n))
    assert rc == code
    assert lib.cal_last_error().decode() == message
