"""CPU-only: how the library finds RCCL at run time (csrc/ismpc_rccl_load.hpp, used by csrc/ismpc_group.hip).  RCCL is optional
(include/ismpc_group.h): a candidate that does not open, or a library that lacks an entry point, costs the group entry points
(ISMPC_E_NO_DEVICE, rccl_version 0) and never the process.  The loader itself runs in a stand-alone program under ASan + UBSan; the
shipped library is driven from torch-free child processes (a torch process maps torch's RCCL first, which would hide every candidate)."""
import ctypes.util
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "quadruped_gait_generation_ismpc_amd")
LIB = os.path.join(PKG, "libismpc_hip.so")

CHILD = r"""
import ctypes, sys
lib = ctypes.CDLL(sys.argv[1])
lib.ismpc_group_last_error.restype = ctypes.c_char_p
v = lib.ismpc_group_rccl_version()
uid = ctypes.create_string_buffer(128)
rc = lib.ismpc_group_unique_id(uid) if len(sys.argv) > 2 else 0
print("version=%d rc=%d" % (v, rc))
print("error=" + lib.ismpc_group_last_error().decode())
"""


def _child(extra_env, unique_id=False):
    env = dict(os.environ, **extra_env)                                    # the parent's environment plus what the case names
    r = subprocess.run([sys.executable, "-c", CHILD, LIB] + (["uid"] if unique_id else []), capture_output=True, text=True, env=env, timeout=120)
    return r


def _fields(r):
    m = re.search(r"version=(-?\d+) rc=(-?\d+)\nerror=(.*)", r.stdout)
    assert m, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    return int(m.group(1)), int(m.group(2)), m.group(3)


def test_loader_probe_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "rccl_load_probe")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "helpers", "rccl_load_probe.cpp"), "-o", exe, "-ldl"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr.lower() or "ubsan" in r.stderr.lower() or "sanitize" in r.stderr.lower()):
        pytest.skip("g++ without the sanitizer runtimes: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-2000:]
    exists = ctypes.util.find_library("m") or "libm.so.6"                  # any small system library, by the name the loader resolves
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, exists], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    out = r.stdout.splitlines()
    assert out[-1] == "OK rccl_load_probe" and f"opened {exists}" in out and sum(l.startswith("missing[") for l in out) == 2, r.stdout
    for l in out:
        if l.startswith("missing["):
            assert "cannot open shared object file" in l, l                # the loader's real message, not "?"
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]


def test_a_missing_rccl_candidate_is_skipped_not_crashed_on(built_libs):
    """$ISMPC_RCCL_LIB names a file that is not there: the later candidates are still tried and the answer is the one without the
    variable (above 20000 where librccl.so.1 resolves, 0 where nothing does)."""
    base = _child({})
    assert base.returncode == 0, (base.returncode, base.stderr[-2000:])
    v0, _, _ = _fields(base)
    assert v0 == 0 or v0 > 20000, v0
    r = _child({"ISMPC_RCCL_LIB": "/nonexistent/librccl.so"})
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    assert _fields(r)[0] == v0


def test_a_library_without_the_entry_points_is_not_bound(built_libs, tmp_path):
    """A library that opens but is no RCCL (it exports ncclGetVersion alone): version 0, ISMPC_E_NO_DEVICE, and the error names the
    symbol that is missing and the file it was looked for in."""
    cxx = shutil.which("g++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = tmp_path / "stub.cpp"
    src.write_text('extern "C" int ncclGetVersion(int* v)\n{ *v = 99999; return 0;\n}\n')
    stub = str(tmp_path / "librccl_stub.so")
    subprocess.check_call([cxx, "-shared", "-fPIC", str(src), "-o", stub])
    r = _child({"ISMPC_RCCL_LIB": stub}, unique_id=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    v, rc, err = _fields(r)
    assert v == 0 and rc == -2, (v, rc, err)                               # ISMPC_E_NO_DEVICE
    assert re.search(r"\bnccl[A-Z]\w+ missing\b", err) and stub in err, err
