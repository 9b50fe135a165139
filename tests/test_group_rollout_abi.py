"""CPU-only: the rollout entry points of the multi-GPU layer (include/ismpc_group.h) -- the symbols are exported and listed, a null group
is refused by every one of them, and ismpc_records_to_instance_major_device says its argument errors before a device is touched (the
pointers below are never dereferenced: the call returns on its arguments)."""
import ctypes as C

import pytest

NEW = ["ismpc_group_rollout_mc_device", "ismpc_group_rollout_wait_on", "ismpc_group_reserve_rollout",
       "ismpc_a_group_rollout_mc_device", "ismpc_a_group_rollout_wait_on", "ismpc_a_group_reserve_rollout",
       "ismpc_records_to_instance_major_device"]


def test_rollout_symbols_are_exported_and_listed(built_libs):
    from quadruped_gait_generation_ismpc_amd import group as G
    lib = G._l()
    for name in NEW:
        assert name in G.EXPORTS_GROUP and getattr(lib, name) is not None, name
    assert len(set(G.EXPORTS_GROUP)) == len(G.EXPORTS_GROUP)


def test_a_null_group_is_refused_by_every_rollout_entry_point(built_libs):
    from quadruped_gait_generation_ismpc_amd import group as G
    lib = G._l()
    one = (C.c_void_p * 1)(C.c_void_p(1 << 20))
    calls = [lambda: lib.ismpc_group_rollout_mc_device(None, 4, one, 0, 10, None, 0, 1, None, None),
             lambda: lib.ismpc_group_rollout_wait_on(None, 0, None),
             lambda: lib.ismpc_group_reserve_rollout(None, 4, 10),
             lambda: lib.ismpc_a_group_rollout_mc_device(None, 4, one, None, 10, None, 0, 1, None, None),
             lambda: lib.ismpc_a_group_rollout_wait_on(None, 0, None),
             lambda: lib.ismpc_a_group_reserve_rollout(None, 4, 10)]
    for k, call in enumerate(calls):
        assert call() == -1, k                                  # ISMPC_E_INVALID
        assert lib.ismpc_group_last_error().decode(), k


@pytest.mark.parametrize("what,args,text", [
    # (tick_major, rows, count, dst_block, stream)
    ("negative rows", (1 << 20, -1, 4, 1 << 21, None), "negative"),
    ("negative count", (1 << 20, 4, -1, 1 << 21, None), "negative"),
    ("null source", (None, 4, 4, 1 << 21, None), "null"),
    ("null destination", (1 << 20, 4, 4, None, None), "null"),
    ("misaligned source", ((1 << 20) + 8, 4, 4, 1 << 21, None), "aligned"),
    ("misaligned destination", (1 << 20, 4, 4, (1 << 21) + 4, None), "aligned"),
])
def test_records_to_instance_major_argument_errors_need_no_device(built_libs, what, args, text):
    from quadruped_gait_generation_ismpc_amd import group as G
    lib = G._l()
    assert lib.ismpc_records_to_instance_major_device(*args) == -1, what
    msg = lib.ismpc_group_last_error().decode()
    assert text in msg, (what, msg)


def test_records_to_instance_major_of_an_empty_shape_is_nothing(built_libs):
    """rows = 0 or count = 0 enqueues nothing -- also with null pointers, and on a machine without a device."""
    from quadruped_gait_generation_ismpc_amd import group as G
    lib = G._l()
    assert lib.ismpc_records_to_instance_major_device(None, 0, 7, None, None) == 0
    assert lib.ismpc_records_to_instance_major_device(None, 7, 0, None, None) == 0
    assert lib.ismpc_records_to_instance_major_device(1 << 20, 0, 0, 1 << 21, None) == 0
