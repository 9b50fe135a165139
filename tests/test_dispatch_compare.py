"""CPU only: the comparison the dispatch parity tests apply (test_gpu_dispatch_parity.compare_with_oracle) does notice what it is
there to notice.  Oracle records of a batch with lifted instances stand in for the device's; each single change below must raise, the
unchanged records must pass."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def case(built_libs):
    import quadruped_gait_generation_ismpc_amd as q
    from oracle import oracle as O
    from test_gpu_dispatch_parity import matrix_batch
    tin = matrix_batch(100, batch=64)
    ref, _ = O.Oracle(O.default_params(100)).solve(tin)
    dev = ref.copy()
    act = (ref["status"] & q.ST_Z_INEQ_ACTIVE) != 0
    dev["iters"][act] |= 1 << 16                                     # the device reports its fallback iterations there
    ok = (ref["status"] & q.ST_ERROR_MASK) == 0
    run = ok & ((ref["status"] & q.ST_FLIGHT) == 0)
    assert (act & ok).sum() >= 8 and (~act & run).sum() >= 8
    return q, ref, dev, int(np.flatnonzero(~act & run)[3]), int(np.flatnonzero(act & ok)[2])


def never_on_boundary(i):
    return False


def test_unmodified_records_pass(case):
    from test_gpu_dispatch_parity import compare_with_oracle
    q, ref, dev, _, _ = case
    assert compare_with_oracle(q, dev, ref, never_on_boundary).sum() >= 32


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_a_com_component_moved_by_1e5_relative_raises(case, axis):
    from test_gpu_dispatch_parity import compare_with_oracle
    q, ref, dev, i, _ = case
    bad = dev.copy()
    bad["com_pos"][i, axis] += 1e-5 * max(np.abs(ref["com_pos"][i]).max(), 1e-3)
    with pytest.raises(AssertionError):
        compare_with_oracle(q, bad, ref, never_on_boundary)


@pytest.mark.parametrize("comp", [0, 1, 2])
def test_a_u0_moved_by_1e5_of_its_scale_raises(case, comp):
    from test_gpu_dispatch_parity import compare_with_oracle
    q, ref, dev, i, _ = case
    bad = dev.copy()
    bad["u0"][i, comp] += 1e-5 * max((490.5, 1.0, 1.0)[comp], abs(ref["u0"][i, comp]))
    with pytest.raises(AssertionError):
        compare_with_oracle(q, bad, ref, never_on_boundary)


@pytest.mark.parametrize("bit", ["ST_X_INFEASIBLE", "ST_Y_INFEASIBLE", "ST_FLIGHT", "ST_Z_NAN", "ST_Z_FAILED"])
def test_a_flipped_status_bit_raises(case, bit):
    from test_gpu_dispatch_parity import compare_with_oracle
    q, ref, dev, i, _ = case
    bad = dev.copy()
    bad["status"][i] ^= getattr(q, bit)
    with pytest.raises(AssertionError):
        compare_with_oracle(q, bad, ref, never_on_boundary)


def test_a_flipped_infeasibility_bit_passes_only_on_the_feasibility_boundary(case):
    from test_gpu_dispatch_parity import compare_with_oracle
    q, ref, dev, i, _ = case
    bad = dev.copy()
    bad["status"][i] ^= q.ST_X_INFEASIBLE
    compare_with_oracle(q, bad, ref, lambda j: j == i)
    with pytest.raises(AssertionError):
        compare_with_oracle(q, bad, ref, lambda j: j != i)


def test_a_cleared_active_bit_raises(case):
    from test_gpu_dispatch_parity import compare_with_oracle
    q, ref, dev, _, j = case
    bad = dev.copy()
    bad["status"][j] &= ~q.ST_Z_INEQ_ACTIVE
    with pytest.raises(AssertionError):
        compare_with_oracle(q, bad, ref, never_on_boundary)


def test_missing_fallback_iterations_raise(case):
    from test_gpu_dispatch_parity import compare_with_oracle
    q, ref, dev, _, j = case
    bad = dev.copy()
    bad["iters"][j] &= 0xFFFF
    with pytest.raises(AssertionError):
        compare_with_oracle(q, bad, ref, never_on_boundary)
