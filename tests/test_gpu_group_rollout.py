"""GPU: disturbed closed-loop rollouts through the multi-GPU group (include/ismpc_group.h) on the ONE GPU of the test box.
  - the record transposition kernel (ismpc_records_to_instance_major_device) against numpy, between sentinels, at the tile edges;
  - tests/cpp/test_group_rollout.cpp: groups of 1 rank on the real RCCL and of 2, 3, 8 ranks through the in-process RCCL test double
    (tests/helpers/fake_rccl.cpp), each also with the all-gather-v form forced -- every byte against per-shard plain handles;
  - group.py: Group.rollout_mc / GroupA.rollout_mc against MPCSolver.rollout_mc_torch / GaitGenerator.rollout_mc_torch."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The kernel's tile is 8 rows x 32 instances, 4096 workgroups at most (more tiles are walked grid-stride): the issue's shapes, one shape
# on each side of a tile edge on both axes (7 | 8 | 9 rows, 31 | 32 | 33 instances; 15 .. 17 too), and one with more tiles (2 x 2188)
# than workgroups.
SHAPES = [(1, 1), (1, 1000), (7, 1), (3, 65), (64, 64), (65, 63), (37, 4099), (200, 1031),
          (7, 33), (8, 32), (9, 31), (15, 17), (16, 16), (17, 15), (31, 33), (9, 70000)]
PAD = 320              # sentinel records on each side of the destination block: more than one tile (8 x 32 = 256 records)


@pytest.mark.parametrize("rows,count", SHAPES)
def test_records_to_instance_major(built_libs, rows, count):
    """Every 4 bytes of the source are distinct (a counter), so a piece that lands anywhere else shows.  The block sits between sentinel
    regions; once directly behind the first one, once as the block of a shard that starts at instance 5 of a larger buffer."""
    import torch
    from quadruped_gait_generation_ismpc_amd import group as G
    lib = G._l()
    src = np.arange(rows * count * 20, dtype=np.uint32).view(np.uint8)
    want = src.reshape(rows, count, 80).transpose(1, 0, 2)
    d_src = torch.from_numpy(src).to("cuda:0")
    for first in (0, 5):
        total = 2 * PAD + (count + first + 4) * rows
        d_dst = torch.full((total, 80), 0xA5, dtype=torch.uint8, device="cuda:0")
        off = PAD + first * rows
        if first == 0:
            stream = torch.cuda.current_stream().cuda_stream
            rc = lib.ismpc_records_to_instance_major_device(C.c_void_p(d_src.data_ptr()), rows, count, C.c_void_p(d_dst.data_ptr() + 80 * off),
                                                            C.c_void_p(stream) if stream else None)
            assert rc == 0, lib.ismpc_group_last_error()
        else:
            block = d_dst[off:off + count * rows].view(count, rows, 80)
            assert G.records_to_instance_major(d_src.view(rows, count, 80), out=block) is block
        torch.cuda.synchronize()
        got = d_dst.cpu().numpy()
        assert np.array_equal(got[off:off + count * rows].reshape(count, rows, 80), want), (rows, count, first)
        assert (got[:off] == 0xA5).all() and (got[off + count * rows:] == 0xA5).all(), (rows, count, first)
    out = G.records_to_instance_major(d_src.view(rows, count, 80))
    assert np.array_equal(out.cpu().numpy(), want)


@pytest.fixture(scope="module")
def rollout_programs(built_libs, tmp_path_factory):
    """The RCCL test double, the C++ caller, and the inputs every world shares."""
    from quadruped_gait_generation_ismpc_amd import workload, formulation_a as FA
    build = os.path.join(ROOT, "tests", "_build"); os.makedirs(build, exist_ok=True)
    pkg = os.path.join(ROOT, "quadruped_gait_generation_ismpc_amd")
    double, exe = os.path.join(build, "libfake_rccl.so"), os.path.join(build, "test_group_rollout")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "tests", "helpers", "fake_rccl.cpp"), "-o", double])
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_group_rollout.cpp"), "-o", exe, "-L", pkg, "-lismpc_hip", f"-Wl,-rpath,{pkg}"])
    d = tmp_path_factory.mktemp("group_rollout")
    B, BA = 4099, 768                                                     # the program's B_MAX, A_MAX
    workload.make_batch(100, B, seed=95).tofile(d / "tick_in.bin")
    w = workload.make_batch_a("walk_C100", BA)
    assert (w["kind"], w["C"], w["F"]) == (1, 100, 3) and abs(w["phi"] - np.pi / 4) < 1e-15 and w["disp_A"] == 0.1      # what the program's defaults build
    w["state"].tofile(d / "a_state.bin")
    rng = np.random.Generator(np.random.Philox(key=96))
    inst = np.zeros(BA, dtype=FA.INST_A)
    inst["height"] = rng.uniform(0.50, 0.62, BA); inst["Qf"] = 1e9; inst["step"] = 50; inst["ds"] = 30; inst["F"] = 3; inst["plan"] = np.arange(BA) % 2
    inst.tofile(d / "a_inst.bin")
    return exe, double, [str(d / n) for n in ("tick_in.bin", "a_state.bin", "a_inst.bin")]


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_cpp_group_rollouts_equal_per_shard_plain_handles(rollout_programs, world, ragged):
    """One child per configuration (no torch in it).  World 1 binds the real RCCL; the others the double through ISMPC_RCCL_LIB."""
    exe, double, files = rollout_programs
    env = dict(os.environ)
    env.pop("ISMPC_RCCL_LIB", None); env.pop("ISMPC_GROUP_FORCE_RAGGED", None)
    if world > 1:
        env["ISMPC_RCCL_LIB"] = double
    if ragged:
        env["ISMPC_GROUP_FORCE_RAGGED"] = "1"
    res = subprocess.run([exe, str(world)] + files, capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, (res.stdout[-500:], res.stderr[-3000:])
    last = res.stdout.strip().splitlines()[-1]
    assert last.startswith(f"OK world={world} rccl=") and f"ragged={'forced' if ragged else 'no'}" in last, last
    version = int(last.split("rccl=")[1].split()[0])
    assert version > 20000 if world == 1 else version == 1
    # batches x (ticks, stride) x pushes x outputs, and the four sequenced calls: none was skipped
    assert f"b_calls={1 * 4 * 2 * 3 if ragged else 3 * 4 * 2 * 3 + 4} " in last and last.endswith(f"a_calls={2 * 1 * 3 * 2 * 3 if ragged else 2 * 2 * 3 * 2 * 3}"), last


def test_python_group_rollout(built_libs):
    """group.py at devices=[0] inside a torch process (RCCL = the copy torch mapped): host records in and out against the single-device
    torch calls, byte for byte after transposing; then the device form, read on a torch stream behind rollout_wait_on, without sync."""
    import torch
    import quadruped_gait_generation_ismpc_amd as q
    from quadruped_gait_generation_ismpc_amd import group as G, workload, formulation_a as FA
    # ---- Formulation B
    p = q.default_params(N=100)
    plan = q.reference_plan(params=p)
    B, ticks, stride = 3001, 24, 5
    tin = workload.make_batch(100, B, seed=97)
    pushes = np.zeros((B, 2), dtype=q.PUSH)
    pushes["tick"][:, 0] = np.arange(B) % 3; pushes["tick"][:, 1] = 5 + np.arange(B) % 4
    pushes["dv"][:, 0, 0] = np.where(np.arange(B) % 3 == 0, 1.0, 0.004 * (np.arange(B) % 5)); pushes["dv"][:, 1, 1] = 0.005 * (np.arange(B) % 4)
    plain = q.MPCSolver(plan, params=p)
    d_st = q.to_device(tin)
    traj, summ = plain.rollout_mc_torch(d_st, 0, ticks, pushes=q.to_device(pushes.reshape(-1)).view(B, 2, 32), stride=stride)
    torch.cuda.synchronize()
    ref_fin, ref_traj, ref_summ = q.from_device(d_st, q.TICK_IN), q.from_device(traj, q.TICK_OUT), q.from_device(summ, q.ROLLOUT_SUMMARY)
    assert ref_traj.shape == (ticks // stride, B) and (ref_summ["error_ticks"] > 0).any()
    g = G.Group(plan, p, devices=[0])
    g.reserve_rollout(B, ticks // stride)
    fin, tr, sm = g.rollout_mc(tin, 0, ticks, pushes=pushes, stride=stride)
    assert tr.shape == (B, ticks // stride)
    assert fin.tobytes() == ref_fin.tobytes() and tr.tobytes() == np.ascontiguousarray(ref_traj.T).tobytes() and sm.tobytes() == ref_summ.tobytes()
    fin2, tr2, sm2 = g.rollout_mc(tin, 0, 3, stride=5, want_summary=False)               # zero rows
    assert tr2.shape == (B, 0) and sm2 is None and fin2.tobytes() != tin.tobytes()
    # the device form: the caller's stream waits for the rollout, nobody calls sync
    d_st2, d_pu = q.to_device(tin), q.to_device(pushes.reshape(-1))
    d_tr = torch.zeros((B * (ticks // stride), 80), dtype=torch.uint8, device="cuda:0"); d_sm = torch.zeros((B, 48), dtype=torch.uint8, device="cuda:0")
    side = torch.cuda.Stream()
    g.order_after(0, torch.cuda.current_stream().cuda_stream)
    g.rollout_mc_device(B, [d_st2.data_ptr()], 0, ticks, [d_pu.data_ptr()], 2, stride, [d_tr.data_ptr()], [d_sm.data_ptr()])
    g.rollout_wait_on(0, side.cuda_stream)
    with torch.cuda.stream(side):
        got_sm, got_tr, got_st = d_sm.clone(), d_tr.clone(), d_st2.clone()
    side.synchronize()
    assert q.from_device(got_sm, q.ROLLOUT_SUMMARY).tobytes() == ref_summ.tobytes()
    assert q.from_device(got_tr, q.TICK_OUT).reshape(B, -1).tobytes() == np.ascontiguousarray(ref_traj.T).tobytes()
    assert q.from_device(got_st, q.TICK_IN).tobytes() == ref_fin.tobytes()
    g.sync(); g.close(); plain.close()
    # ---- Formulation A
    gait = FA.default_gait(FA.WALK, np.pi / 4, 0.1)
    _, ce = FA.plan(gait)
    pa = FA.default_params(FA.WALK)
    gen = FA.GaitGenerator(pa, ce)
    BA, ta, sa = 257, 12, 4
    st0 = gen.initial_state(gait.disp_C, batch=BA)
    pu = np.zeros((BA, 2), dtype=FA.PUSH_A)
    pu["tick"][:, 0] = np.arange(BA) % 3; pu["tick"][:, 1] = 5 + np.arange(BA) % 4
    pu["dv"][:, 0, 0] = np.where(np.arange(BA) % 3 == 0, 2.0, 0.004 * (np.arange(BA) % 5)); pu["dv"][:, 0, 1] = -pu["dv"][:, 0, 0]
    pu["dv"][:, 1, 1] = 0.005 * (np.arange(BA) % 4)
    d_sa = q.to_device(st0)
    traj, summ = gen.rollout_mc_torch(d_sa, ta, pushes=q.to_device(pu.reshape(-1)).view(BA, 2, 24), stride=sa)
    torch.cuda.synchronize()
    ref_fin, ref_traj, ref_summ = q.from_device(d_sa, FA.STATE_A), q.from_device(traj, FA.OUT_A), q.from_device(summ, FA.ROLLOUT_SUMMARY_A)
    assert (ref_summ["error_ticks"] > 0).any() and (ref_summ["error_ticks"] == 0).any()
    ga = G.GroupA(pa, ce, devices=[0])
    ga.reserve_rollout(BA, ta // sa)
    fin, tr, sm = ga.rollout_mc(st0, ta, pushes=pu, stride=sa)
    assert tr.shape == (BA, ta // sa)
    assert fin.tobytes() == ref_fin.tobytes() and tr.tobytes() == np.ascontiguousarray(ref_traj.T).tobytes() and sm.tobytes() == ref_summ.tobytes()
    ga.close(); gen.close()
