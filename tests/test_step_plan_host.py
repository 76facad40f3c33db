"""The shape of a pass or train step on the host (`cal_debug_step_shape`: calamity_amd/csrc/step_plan.hpp run with no device).

`plan_step` is total, so the table holds every combination of its inputs, the unreachable ones included: 2^13 flag settings x 4
launch modes.  tests/golden/step_plan/shape_table.npz was recorded once, on the CPU, by a program that held the expressions of
commit 52d55df verbatim -- written there at their points of use in enqueue_pass, enqueue_update, enqueue_update_y and run -- and
composed them as that commit's call sites do.  A second test asserts what those copies only implied: finalize_kernel and
coeff_partial_reduce_kernel run exactly once per step, in a launch of their own or inside the update."""
import ctypes as C
import os

import numpy as np

from calamity_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_plan", "shape_table.npz")
UPDATE_NONE, UPDATE_TAIL, UPDATE_FUSED, UPDATE_LAMB, UPDATE_ADAM2 = range(5)
_table = {}


def _shapes():
    """(inputs, recorded shapes, shapes of the library), computed once."""
    if not _table:
        gold = np.load(GOLDEN)
        assert str(gold["commit"]) == "52d55df"
        inputs = gold["inputs"].astype(np.int32)
        got = np.empty((len(inputs), gold["shape"].shape[1]), np.int32)
        fn = _lib.load().cal_debug_step_shape
        p32 = C.POINTER(C.c_int32)
        for row, out in zip(inputs, got):
            assert fn(row.ctypes.data_as(p32), out.ctypes.data_as(p32)) == 0
        _table.update(gold=gold, inputs=inputs, got=got)
    return _table["gold"], _table["inputs"], _table["got"]


def test_every_input_has_the_recorded_shape():
    gold, inputs, got = _shapes()
    names = gold["input_names"].tolist()
    # the table is complete: every flag setting under every launch mode, once
    assert inputs.shape == (4 << 13, 14) and len(np.unique(inputs, axis=0)) == 4 << 13
    flags = np.delete(inputs, names.index("launch_mode"), axis=1)
    assert set(np.unique(flags)) == {0, 1} and set(np.unique(inputs[:, names.index("launch_mode")])) == {0, 1, 2, 3}
    want = gold["shape"].astype(np.int32)
    for k, nm in enumerate(gold["shape_names"].tolist()):
        bad = np.flatnonzero(got[:, k] != want[:, k])
        assert bad.size == 0, (nm, dict(zip(names, inputs[bad[0]].tolist())), int(got[bad[0], k]), int(want[bad[0], k]))


def test_bookkeeping_and_partial_sums_run_exactly_once():
    gold, inputs, got = _shapes()
    i = {nm: inputs[:, k] for k, nm in enumerate(gold["input_names"].tolist())}
    s = {nm: got[:, k] for k, nm in enumerate(gold["shape_names"].tolist())}
    upd = i["apply_update"] == 1
    assert np.array_equal(s["update"] != UPDATE_NONE, upd)
    # the fused update and the one-launch tail do the loop bookkeeping themselves; every other update needs finalize_kernel before it
    own = np.isin(s["update"], (UPDATE_FUSED, UPDATE_TAIL))
    assert np.array_equal(s["finalize"][upd] == 1, ~own[upd])
    assert np.array_equal(s["fused_update"] == 1, s["update"] == UPDATE_FUSED) and np.array_equal(s["tail1"] == 1, s["update"] == UPDATE_TAIL)
    # ... and sum the partial coefficient gradients themselves: never together with the reduce kernel
    assert not np.any((s["partial_reduce"] == 1) & own)
    # partials that a gradient pass leaves are summed by exactly one of the two
    need = (i["grads"] == 1) & (s["partials"] == 1)
    assert np.array_equal(s["partial_reduce"] == 1, need & ~own)
    # without an update the pass ends in finalize_kernel
    assert np.all(s["finalize"][~upd] == 1)
    assert np.array_equal(s["planes"], np.where(s["Rk"] == 1, 3, 1))
    assert not np.any((s["expand"] == 1) & (i["gain_basis"] == 0)) and not np.any((s["replay"] == 1) & ~upd)
