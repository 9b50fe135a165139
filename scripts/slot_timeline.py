#!/usr/bin/env python3
"""Which wavefront ran in which wave slot, and when the slots stood empty (diagnostic build with -DISMPC_STAMPS): every wavefront of the
per-tick lane-group kernels stamps s_memrealtime (100 MHz) at 6 points and leaves HW_ID | XCC_ID << 32 in word 6 of its stamp record.  For
ONE launch this rebuilds the sequence of wavefronts of every (XCC, SE, SH, CU, SIMD, slot) and splits the slot time of the launch -- first
wave start to last stamp, over the slots that ran anything -- into
    busy         a wavefront between its first stamp and its last one (stores issued)
    ramp         before the slot's first wavefront
    refill gaps  from the last stamp of one wavefront to the first stamp of the next one in that slot (wave teardown, the wait for a
                 workgroup's worth of slots and LDS, dispatch)
    tail         after the slot's last wavefront
and prints the distribution of the refill gaps.  HW_ID's slot number is the hardware's (a SIMD has more slot ids than the two wavefronts
249 VGPRs admit), so the same split is given per SIMD too, against `--occ` wavefronts per SIMD: resident wavefronts integrated over time.
usage: python -c "from quadruped_gait_generation_ismpc_amd import build; build.build(out='build/variants/libismpc_stamps.so', flags='-DISMPC_STAMPS')"
       ISMPC_LIB=build/variants/libismpc_stamps.so python scripts/slot_timeline.py [--occ 2] [batch ...]      (default: 65536)"""
import ctypes as C, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def decode(word):
    """word 6 of a stamp record -> (xcc, se, sh, cu, simd, slot)"""
    hw, xcc = word & 0xFFFFFFFF, (word >> 32) & 0xF
    return xcc, (hw >> 13) & 7, (hw >> 12) & 1, (hw >> 8) & 15, (hw >> 4) & 3, hw & 15


def pct(a, ps=(10, 50, 90, 99)):
    a = np.asarray(a, dtype=np.float64)
    if a.size == 0:
        return None
    d = {f"p{p}": float(np.percentile(a, p)) for p in ps}
    d["max"] = float(a.max()); d["mean"] = float(a.mean()); d["n"] = int(a.size)
    return d


def timeline(start, end, where, occ):
    """start, end: ns per wavefront; where: word 6 per wavefront.  Returns the report of one launch."""
    T0, T1 = int(start.min()), int(end.max())
    span = T1 - T0
    slot_key = where & np.uint64(0xF0000FFFF) & ~np.uint64(0xC0)         # XCC, SE, SH, CU, SIMD, slot (the pipe bits dropped)
    simd_key = slot_key & ~np.uint64(0xF)
    rep = {"waves": int(len(start)), "span_ns": span, "slots_used": int(len(np.unique(slot_key))), "simds_used": int(len(np.unique(simd_key))),
           "xccs": int(len(np.unique((where >> np.uint64(32)) & np.uint64(0xF)))),
           "slot_ids_seen": sorted(int(v) for v in np.unique(where & np.uint64(0xF))),
           "waves_per_slot": pct(np.unique(slot_key, return_counts=True)[1], (50,)), "wave_life_ns": pct(end - start)}
    # per hardware slot
    busy = ramp = tail = gap_sum = 0
    gaps, overlaps = [], 0
    order = np.lexsort((start, slot_key))
    k, s, e = slot_key[order], start[order], end[order]
    first = np.r_[True, k[1:] != k[:-1]]; last = np.r_[first[1:], True]
    busy = int((e - s).sum()); ramp = int((s[first] - T0).sum()); tail = int((T1 - e[last]).sum())
    g = (s[1:] - e[:-1])[~first[1:]]
    overlaps = int((g < 0).sum())
    gaps = np.maximum(g, 0)
    total = rep["slots_used"] * span
    rep["per_slot"] = {"busy": busy / total, "ramp": ramp / total, "refill_gaps": float(gaps.sum()) / total, "tail": tail / total,
                       "overlapping_successors": overlaps}
    rep["refill_gap_ns"] = pct(gaps)
    # per SIMD: resident wavefronts over time against `occ`
    total = rep["simds_used"] * span * occ
    sramp = stail = 0
    for key in np.unique(simd_key):
        m = simd_key == key
        sramp += (int(start[m].min()) - T0) * occ; stail += (T1 - int(end[m].max())) * occ
    mid = total - busy - sramp - stail
    rep["per_simd"] = {"occ": occ, "busy": busy / total, "ramp": sramp / total, "tail": stail / total, "empty_between": mid / total}
    return rep


def main():
    args = sys.argv[1:]
    occ = 2
    if "--occ" in args:
        occ = int(args[args.index("--occ") + 1]); del args[args.index("--occ"):args.index("--occ") + 2]
    import torch
    import quadruped_gait_generation_ismpc_amd as q
    from quadruped_gait_generation_ismpc_amd import workload, _lib
    lib = _lib.load()
    lib.ismpc_debug_stamps.argtypes = [C.c_void_p, C.c_int]
    N = 100
    p = q.default_params(N=N)
    solver = q.MPCSolver(q.reference_plan(params=p), params=p, device=0)
    for B in [int(a) for a in args] or [65536]:
        d_in = q.to_device(workload.make_batch(N, B), "cuda:0"); d_out = torch.empty((B, 80), dtype=torch.uint8, device="cuda:0")
        for _ in range(20):
            solver.solve_batch_torch(d_in, d_out)
        torch.cuda.synchronize()
        lib.ismpc_debug_stamps(None, 1)
        solver.solve_batch_torch(d_in, d_out); torch.cuda.synchronize()
        info = solver.launch_info()
        buf = np.zeros(16384 * 8, dtype=np.uint64)
        lib.ismpc_debug_stamps(buf.ctypes.data_as(C.c_void_p), 0)
        waves = min((B * info["lanes"] + 63) // 64, 16384)
        t = buf.reshape(16384, 8)[:waves]
        assert (t[:, 0] != 0).all() and (t[:, 5] != 0).all(), "wavefronts without stamps: not the -DISMPC_STAMPS build?"
        rep = timeline(t[:, 0].astype(np.int64) * 10, t[:, 5].astype(np.int64) * 10, t[:, 6].copy(), occ)
        rep.update({"batch": B, "family": info["family"], "lanes": info["lanes"], "R": info["R"]})
        print(json.dumps(rep), flush=True)
    solver.close()


if __name__ == "__main__":
    main()
