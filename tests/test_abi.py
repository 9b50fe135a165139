"""CPU-only: the C-ABI library loads, exports every symbol include/ismpc.h declares, agrees with
the header on record layouts and refuses to compute without a GPU (no silent fallback)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_functions():
    txt = open(os.path.join(ROOT, "include", "ismpc.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(ismpc_[a-z_0-9]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol(built_libs):
    import quadruped_gait_generation_ismpc_amd as q
    from quadruped_gait_generation_ismpc_amd import _lib
    lib = _lib.load()
    declared = _header_functions()
    assert declared, "no functions parsed from include/ismpc.h"
    assert sorted(q.EXPORTS) == declared
    for name in declared:
        assert getattr(lib, name) is not None
    assert lib.ismpc_abi_version() == 1


def test_record_layouts_match_header(built_libs):
    import quadruped_gait_generation_ismpc_amd as q
    from oracle import oracle as O
    assert q.TICK_IN.itemsize == 72 and q.TICK_OUT.itemsize == 80
    assert q.TICK_IN == O.TICK_IN and q.TICK_OUT == O.TICK_OUT
    assert C.sizeof(q.Params) == C.sizeof(O.Params) == 16 + 13 * 8


def test_default_params_are_the_reference_constants(built_libs):
    import quadruped_gait_generation_ismpc_amd as q
    from oracle import oracle as O
    p, o = q.default_params(), O.default_params()
    for name, _ in q.Params._fields_:
        assert getattr(p, name) == getattr(o, name), name
    assert (p.N, p.S, p.F, p.M) == (100, 35, 10, 2)           # parameters.cpp:42-45
    assert (p.q_p, p.q_u, p.q_v) == (1005000.0, 0.01, 100.0)   # MPCSolver.cpp:253-255


def test_reference_plan_matches_controller(built_libs):
    import quadruped_gait_generation_ismpc_amd as q
    from oracle import oracle as O
    a, b = q.reference_plan(), O.reference_plan()
    assert a.shape == (40, 4) and np.array_equal(a, b)
    assert np.all(a[0] == 0) and a[1, 0] == 0.0 and a[2, 0] == 0.2 and a[1, 1] == 0.08 and a[2, 1] == -0.08
    assert a[3, 3] == 135.0


def test_no_cpu_fallback(built_libs):
    import torch
    import quadruped_gait_generation_ismpc_amd as q
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible here")
    with pytest.raises(q.IsmpcError) as e:
        q.MPCSolver(q.reference_plan())
    assert e.value.code == -2 and "no CPU fallback" in str(e.value)


def test_product_never_imports_the_oracle():
    """No import / dlopen / include of anything under oracle/ from the product package (comments may name it)."""
    pkg = os.path.join(ROOT, "quadruped_gait_generation_ismpc_amd")
    pat = re.compile(r"(from\s+oracle|import\s+oracle|libismpc_oracle|libqpoases_ref|[\"'<]\.*/*oracle/|orc_[a-z_]+\s*\()")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".cpp", ".hpp", ".h")):
                txt = open(os.path.join(dirpath, f)).read()
                assert not pat.search(txt), f
    for f in ("ismpc.h", "ismpc_a.h", "ismpc_group.h", "MPCSolver.hpp", "ismpc_mini_types.hpp"):
        assert not pat.search(open(os.path.join(ROOT, "include", f)).read()), f


def test_formulation_a_abi(built_libs):
    """include/ismpc_a.h: every declared symbol is exported; layouts; the host plan generators match the oracle."""
    from quadruped_gait_generation_ismpc_amd import _lib, formulation_a as FA
    from oracle import oracle_a as A
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ismpc_a.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(ismpc_a_[a-z_0-9]+)\s*\(", txt)))
    assert declared == sorted(FA.EXPORTS_A)
    lib = _lib.load()
    for name in declared:
        assert getattr(lib, name) is not None
    assert FA.STATE_A.itemsize == 96 and FA.OUT_A.itemsize == 80
    for kind, phi, dA in [(0, 0.0, 0.15), (0, np.pi / 4, 0.1), (0, np.pi / 2, 0.15), (1, 0.0, 0.1), (1, np.pi / 4, 0.1), (1, np.pi / 2, 0.1)]:
        fp, ce = FA.plan(FA.default_gait(kind, phi, dA))           # product: csrc/ismpc_a_hip.hip (host code)
        fo, co = A.plan(A.gait(kind, phi, dA))                     # oracle: init_quadruped*.m restated
        assert fp.shape == fo.shape and np.array_equal(fp, fo) and np.array_equal(ce, co)
    pw, ow = FA.default_params(FA.WALK), A.params(A.WALK)
    for name, _ in FA.ParamsA._fields_:
        assert getattr(pw, name) == getattr(ow, name), name


def test_sweep_validation_and_no_cpu_fallback(built_libs):
    """ismpc_create_sweep: sets that disagree on the shape of the problem are refused before anything touches a device; without a GPU
    a valid sweep fails like ismpc_create does (no CPU table build in disguise)."""
    import torch
    import quadruped_gait_generation_ismpc_amd as q
    a, b = q.default_params(N=100), q.default_params(N=50)
    with pytest.raises(q.IsmpcError) as e:
        q.MPCSolver.sweep(q.reference_plan(params=a), [a, b])
    assert e.value.code == -1 and "share N" in str(e.value)
    c = q.default_params(N=100); c.mass = -1.0
    with pytest.raises(q.IsmpcError) as e:
        q.MPCSolver.sweep(q.reference_plan(params=a), [a, c])
    assert e.value.code == -1
    if not torch.cuda.is_available():
        with pytest.raises(q.IsmpcError) as e:
            q.MPCSolver.sweep(q.reference_plan(params=a), [a, q.default_params(N=100)])
        assert e.value.code == -2 and "no CPU fallback" in str(e.value)


def test_more_than_64_double_support_samples_are_refused_before_the_device(built_libs):
    """include/ismpc.h: F <= ISMPC_F_MAX = 64 (the vertical fallback keeps one pinned sample per lane of a wavefront).  F = 65 is refused
    by all three constructors with ISMPC_E_UNSUPPORTED whether or not a GPU is there; F = 64 gets past the argument checks."""
    import torch
    import quadruped_gait_generation_ismpc_amd as q
    assert "#define ISMPC_F_MAX 64" in open(os.path.join(ROOT, "include", "ismpc.h")).read()
    p = q.default_params(N=100, S=20, F=65)
    plan = q.reference_plan(params=p)
    for make in (lambda: q.MPCSolver(plan, params=p), lambda: q.MPCSolver.sweep(plan, [p, p]),
                 lambda: q.MPCSolver.plans([plan], p), lambda: q.MPCSolver.plans([plan, plan], [p, p])):
        with pytest.raises(q.IsmpcError) as e:
            make()
        assert e.value.code == -5 and "F > 64" in str(e.value), str(e.value)
    p = q.default_params(N=100, S=20, F=64)
    if not torch.cuda.is_available():
        with pytest.raises(q.IsmpcError) as e:
            q.MPCSolver(q.reference_plan(params=p), params=p)
        assert e.value.code == -2 and "no CPU fallback" in str(e.value)
