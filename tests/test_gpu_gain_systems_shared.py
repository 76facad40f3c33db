"""One solver across calls: solve_gain_coeffs / solve_gain_time_coeffs and gain_basis_errors build their projected systems in ONE set of
scratch buffers (sized by whichever call comes, grown by the next, released by a new scratch bound), so a call must not see what another
call, another chunking or another bound left there.

On one solver: sweep, errors, scratch bound 1 (one row per chunk), errors, sweep, bound 0, sweep, errors.  Every call's outputs (gains and
y and the counts of a sweep; gain_var, y_var, gain_dof and the counts of the errors) equal, bit for bit, the same call on a fresh solver
that has never made a call of the other kind: it reaches the call's parameters by the sweeps that came before (the only calls that move
them), takes the call's bound -- which releases every scratch buffer -- and makes the call.  The bytes a solver holds after sweep and
errors do not depend on their order.

Cases: the four of test_gpu_gain_time_solve.CHUNKED (n = L K = 72: the factor in LDS, past one 64-block of N; 128, 260: in scratch; the
time basis alone at L = 9: the channel systems in scratch), and a frequency basis alone on 5 antennas x 96 channels at K = 10 and 70."""
import numpy as np
import pytest

from test_gain_time_solve_host import bases_of, flagged_case, rand_basis
from test_gpu_fit_quality import solver_of
from test_gpu_gain_time_solve import CHUNKED, time_solver

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
SEQUENCE = ["sweep", "errors", 1, "errors", "sweep", 0, "sweep", "errors"]  # (an int: the scratch bound from there on)


def time_case(shape, kind, LK):
    p, params = flagged_case(*shape)
    Bt, B = bases_of(shape, kind, LK)
    return lambda dtype: time_solver(p, params, dtype, Bt, B), "solve_gain_time_coeffs"


def freq_case(K):
    p, params = flagged_case(1, 5, 96)
    B = rand_basis(96, K, 2)

    def make(dtype):
        s = solver_of(p, params, dtype)
        s.set_gain_basis(B)
        return s

    return make, "solve_gain_coeffs"


def call(s, what, sweep):
    """The outputs of one call as a flat list of arrays and numbers."""
    if what == "sweep":
        counts = getattr(s, sweep)(2)
        return [counts["nsolved"], counts["nsingular"], *s.get_params()[:2], *s.get_gain_coeffs()]
    out = s.gain_basis_errors()
    return [out["nsolved"], out["nsingular"], out["gain_var"], out["y_var"], out["gain_dof"]]


def fresh_call(make, dtype, sweep, nsweeps_before, bound, what):
    s = make(dtype)
    for _ in range(nsweeps_before):
        getattr(s, sweep)(2)
    s._set_coeff_solve_scratch(bound)  # every scratch buffer goes: the call sizes its own
    out = call(s, what, sweep)
    s.close()
    return out


def run_sequence(make, sweep, dtype):
    s = make(dtype)
    bound, nsweeps, nerrors = 0, 0, 0
    for step, what in enumerate(SEQUENCE):
        if isinstance(what, int):
            bound = what
            s._set_coeff_solve_scratch(bound)
            continue
        got = call(s, what, sweep)
        want = fresh_call(make, dtype, sweep, nsweeps, bound, what)
        assert got[:2] == want[:2] and got[0] > 0, (step, what, got[:2], want[:2])
        for k, (a, b) in enumerate(zip(got[2:], want[2:])):
            assert np.any(a), (step, what, k)
            np.testing.assert_array_equal(a, b, err_msg=f"step {step} ({what}, bound {bound}), output {k}")
        nsweeps += what == "sweep"
        nerrors += what == "errors"
    assert (nsweeps, nerrors) == (3, 3)
    held = s.memory_bytes()
    s.close()
    # sweep then errors, errors then sweep: the same bytes, which are also what the long sequence ends with (its last bound is 0 too)
    sizes = []
    for order in (("sweep", "errors"), ("errors", "sweep")):
        s = make(dtype)
        for what in order:
            call(s, what, sweep)
        sizes.append(s.memory_bytes())
        s.close()
    assert sizes[0] == sizes[1] == held, (sizes, held)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,kind,LK", CHUNKED)
def test_time_basis_sweeps_and_errors_share_their_scratch_without_seeing_each_other(shape, kind, LK, dtype):
    make, sweep = time_case(shape, kind, LK)
    run_sequence(make, sweep, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [10, 70])
def test_frequency_basis_sweeps_and_errors_share_their_scratch_without_seeing_each_other(K, dtype):
    make, sweep = freq_case(K)
    run_sequence(make, sweep, dtype)
