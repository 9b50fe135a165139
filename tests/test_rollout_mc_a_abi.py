"""CPU-only: the C ABI of Formulation A's disturbed closed loop (ismpc_a_rollout_mc_device) -- the two records as a C compiler lays
them out against the numpy dtypes, the exported symbol, the error mask, and the argument errors that are reported before a device is
touched."""
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
    printf("ismpc_a_push %zu\n", sizeof(ismpc_a_push));
    F(ismpc_a_push, tick); F(ismpc_a_push, reserved); F(ismpc_a_push, dv);
    printf("ismpc_a_rollout_summary %zu\n", sizeof(ismpc_a_rollout_summary));
    F(ismpc_a_rollout_summary, status_or); F(ismpc_a_rollout_summary, first_error_tick); F(ismpc_a_rollout_summary, error_ticks);
    F(ismpc_a_rollout_summary, iter_limit_ticks); F(ismpc_a_rollout_summary, iters_sum_x); F(ismpc_a_rollout_summary, iters_sum_y);
    F(ismpc_a_rollout_summary, max_active_x); F(ismpc_a_rollout_summary, max_active_y);
    F(ismpc_a_rollout_summary, max_abs_vel); F(ismpc_a_rollout_summary, max_abs_u0);
    printf("ISMPC_A_ST_ERROR_MASK %d\n", (int)ISMPC_A_ST_ERROR_MASK);
    return 0;
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """What a C compiler makes of include/ismpc_a.h: {name: value}."""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "a C compiler is needed for the layout probe"
    d = tmp_path_factory.mktemp("mc_a_abi")
    src, exe = d / "probe.c", d / "probe"
    src.write_text(PROBE)
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True)
    return {k: int(v) for k, v in (line.split() for line in out.splitlines())}


def test_record_layouts_match_the_numpy_dtypes(probe):
    from quadruped_gait_generation_ismpc_amd import formulation_a as FA
    assert probe["ismpc_a_push"] == FA.PUSH_A.itemsize == 24
    assert probe["ismpc_a_rollout_summary"] == FA.ROLLOUT_SUMMARY_A.itemsize == 64
    for cname, dt in (("ismpc_a_push", FA.PUSH_A), ("ismpc_a_rollout_summary", FA.ROLLOUT_SUMMARY_A)):
        fields = {k: v for k, v in probe.items() if k.startswith(cname + ".")}
        assert sorted(f.split(".")[1] for f in fields) == sorted(dt.names)
        for f, off in fields.items():
            assert dt.fields[f.split(".")[1]][1] == off, f
    assert FA.PUSH_A["dv"].shape == (2,)
    assert FA.ROLLOUT_SUMMARY_A["max_abs_vel"].shape == (2,) and FA.ROLLOUT_SUMMARY_A["max_abs_u0"].shape == (2,)


def test_error_mask_is_the_python_one(probe):
    import quadruped_gait_generation_ismpc_amd as q
    from quadruped_gait_generation_ismpc_amd import formulation_a as FA
    assert probe["ISMPC_A_ST_ERROR_MASK"] == FA.ST_ERROR_MASK_A == 15
    assert FA.ST_ERROR_MASK_A == FA.ST_X_INFEASIBLE | FA.ST_Y_INFEASIBLE | FA.ST_OVERFLOW | FA.ST_BAD_INDEX
    assert q.ST_ERROR_MASK_A == 15 and q.PUSH_A is FA.PUSH_A and q.ROLLOUT_SUMMARY_A is FA.ROLLOUT_SUMMARY_A


def test_symbol_is_exported_and_listed(built_libs):
    from quadruped_gait_generation_ismpc_amd import _lib, formulation_a as FA
    assert "ismpc_a_rollout_mc_device" in FA.EXPORTS_A
    lib = _lib.load()
    assert lib.ismpc_a_rollout_mc_device is not None


@pytest.mark.parametrize("what,args,text", [
    # (handle, batch, state, inst, ticks, pushes, n_push, stride, traj, summary, stream)
    ("null handle", (None, 4, 1 << 20, None, 10, None, 0, 1, None, None, None), "null handle"),
    ("negative batch", (None, -1, None, None, 10, None, 0, 1, None, None, None), "negative batch"),
    ("negative ticks", (None, 4, 1 << 20, None, -1, None, 0, 1, None, None, None), "ticks"),
    ("stride 0", (None, 4, 1 << 20, None, 10, None, 0, 0, None, None, None), "traj_stride"),
    ("stride -2", (None, 4, 1 << 20, None, 10, None, 0, -2, None, None, None), "traj_stride"),
    ("negative n_push", (None, 4, 1 << 20, None, 10, None, -1, 1, None, None, None), "n_push"),
    ("null table", (None, 4, 1 << 20, None, 10, None, 3, 1, None, None, None), "null push table"),
    ("null state", (None, 4, None, None, 10, None, 0, 1, None, None, None), "null state"),
])
def test_argument_errors_need_no_device(built_libs, what, args, text):
    """Every argument error is said before the handle is looked at, let alone the device: none of these calls has a handle.  (The
    pointers are never dereferenced: the call returns on its arguments.)"""
    from quadruped_gait_generation_ismpc_amd import formulation_a as FA
    lib = FA._l()
    rc = lib.ismpc_a_rollout_mc_device(*args)
    assert rc == -1, what
    msg = lib.ismpc_a_last_error().decode()
    assert msg and text in msg and "ismpc_a_rollout_mc_device" in msg, (what, msg)


def test_python_wrapper_raises_on_a_bad_stride(built_libs):
    from quadruped_gait_generation_ismpc_amd import formulation_a as FA
    g = FA.GaitGenerator.__new__(FA.GaitGenerator)
    g._h = None
    with pytest.raises(FA.IsmpcAError) as e:
        g.rollout_mc_device(4, 1 << 20, 10, stride=0)
    assert "traj_stride" in str(e.value)
