"""CPU-only: the C ABI of Formulation A's disturbed closed loop with swing feet (ismpc_a_rollout_mc_feet_device) and of the foot files
on the device (ismpc_a_foot_trajectories_device) -- ismpc_a_feet_summary as a C compiler lays it out against the numpy dtype, the
exported symbols, and the argument errors that are reported before a device is touched."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "ismpc_a.h"
#define F(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void)
{
    printf("ismpc_a_feet_summary %zu\n", sizeof(ismpc_a_feet_summary));
    F(ismpc_a_feet_summary, moved_rows); F(ismpc_a_feet_summary, first_moved_row); F(ismpc_a_feet_summary, last_moved_row);
    F(ismpc_a_feet_summary, nonfinite); F(ismpc_a_feet_summary, max_abs_shift);
    printf("ISMPC_A_FEET_PAD %d\n", (int)ISMPC_A_FEET_PAD);
    return 0;
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """What a C compiler makes of include/ismpc_a.h: {name: value}."""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is needed for the layout probe"
    d = tmp_path_factory.mktemp("mc_feet_abi")
    src, exe = d / "probe.c", d / "probe"
    src.write_text(PROBE)
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True)
    return {k: int(v) for k, v in (line.split() for line in out.splitlines())}


def test_feet_summary_layout_matches_the_numpy_dtype(probe):
    import quadruped_gait_generation_ismpc_amd as q
    from quadruped_gait_generation_ismpc_amd import formulation_a as FA
    assert probe["ismpc_a_feet_summary"] == FA.FEET_SUMMARY_A.itemsize == 32
    fields = {k: v for k, v in probe.items() if k.startswith("ismpc_a_feet_summary.")}
    assert sorted(f.split(".")[1] for f in fields) == sorted(FA.FEET_SUMMARY_A.names)
    for f, off in fields.items():
        assert FA.FEET_SUMMARY_A.fields[f.split(".")[1]][1] == off, f
    assert [FA.FEET_SUMMARY_A.fields[n][1] for n in ("moved_rows", "first_moved_row", "last_moved_row", "nonfinite", "max_abs_shift")] == [0, 4, 8, 12, 16]
    assert FA.FEET_SUMMARY_A["max_abs_shift"].shape == (2,)
    assert probe["ISMPC_A_FEET_PAD"] == FA.FEET_PAD
    assert q.FEET_SUMMARY_A is FA.FEET_SUMMARY_A


def test_symbols_are_exported_and_listed(built_libs):
    from quadruped_gait_generation_ismpc_amd import _lib, formulation_a as FA
    lib = _lib.load()
    for name in ("ismpc_a_rollout_mc_feet_device", "ismpc_a_foot_trajectories_device", "ismpc_a_rollout_mc_device"):
        assert name in FA.EXPORTS_A
        assert getattr(lib, name) is not None
    assert callable(FA.GaitGenerator.rollout_mc_feet_device) and callable(FA.GaitGenerator.rollout_mc_feet_torch)
    assert callable(FA.GaitGenerator.foot_trajectories_torch)


P = 1 << 20           # a pointer that is never dereferenced: the calls below return on their arguments


@pytest.mark.parametrize("what,args,text", [
    # (handle, batch, state, inst, ticks, pushes, n_push, stride, traj, summary, feet, feet_summary, stream)
    ("null handle", (None, 4, P, None, 10, None, 0, 1, None, None, P, None, None), "null handle"),
    ("negative batch", (None, -1, None, None, 10, None, 0, 1, None, None, None, None, None), "negative batch"),
    ("negative ticks", (None, 4, P, None, -1, None, 0, 1, None, None, P, None, None), "ticks"),
    ("stride 0", (None, 4, P, None, 10, None, 0, 0, None, None, P, None, None), "traj_stride"),
    ("stride -2", (None, 4, P, None, 10, None, 0, -2, None, None, P, None, None), "traj_stride"),
    ("negative n_push", (None, 4, P, None, 10, None, -1, 1, None, None, P, None, None), "n_push"),
    ("null table", (None, 4, P, None, 10, None, 3, 1, None, None, P, None, None), "null push table"),
    ("null state", (None, 4, None, None, 10, None, 0, 1, None, None, P, None, None), "null state"),
    ("null feet", (None, 4, P, None, 10, None, 0, 1, None, None, None, None, None), "null feet_dev"),
])
def test_rollout_argument_errors_need_no_device(built_libs, what, args, text):
    """Every argument error is said before the handle is looked at, let alone the device: none of these calls has a handle."""
    from quadruped_gait_generation_ismpc_amd import formulation_a as FA
    lib = FA._l()
    rc = lib.ismpc_a_rollout_mc_feet_device(*args)
    assert rc == -1, what
    msg = lib.ismpc_a_last_error().decode()
    assert msg and text in msg and "ismpc_a_rollout_mc_feet_device" in msg, (what, msg)


@pytest.mark.parametrize("what,args,text", [
    # (handle, batch, inst, feet, sim_duration, dst, nrows, stream)
    ("null handle", (None, 4, None, P, 100, P, None, None), "null handle"),
    ("negative batch", (None, -1, None, P, 100, P, None, None), "negative batch"),
    ("sim_duration 0", (None, 4, None, P, 0, P, None, None), "sim_duration"),
    ("sim_duration -5", (None, 4, None, P, -5, P, None, None), "sim_duration"),
    ("null feet", (None, 4, None, None, 100, P, None, None), "null feet_dev"),
    ("null dst", (None, 4, None, P, 100, None, None, None), "null dst_dev"),
])
def test_foot_files_argument_errors_need_no_device(built_libs, what, args, text):
    from quadruped_gait_generation_ismpc_amd import formulation_a as FA
    lib = FA._l()
    rc = lib.ismpc_a_foot_trajectories_device(*args)
    assert rc == -1, what
    msg = lib.ismpc_a_last_error().decode()
    assert msg and text in msg and "ismpc_a_foot_trajectories_device" in msg, (what, msg)


def test_python_wrappers_raise_with_the_message(built_libs):
    from quadruped_gait_generation_ismpc_amd import formulation_a as FA
    g = FA.GaitGenerator.__new__(FA.GaitGenerator)
    g._h = None
    with pytest.raises(FA.IsmpcAError) as e:
        g.rollout_mc_feet_device(4, P, P, 10, stride=0)
    assert "traj_stride" in str(e.value) and "ismpc_a_rollout_mc_feet_device" in str(e.value)
    with pytest.raises(FA.IsmpcAError) as e:
        g.rollout_mc_feet_device(4, P, None, 10)
    assert "null feet_dev" in str(e.value)
