#!/usr/bin/env python3
"""Copies the reference's own known-answer DATA for Formulation A into small committed fixtures:
the checked-in MATLAB trajectories AMR_code_DART/MATLAB_trajectories/**/Com{Trajectory,Velocity}_*.txt
(3 columns, %e with 7 significant digits, one row per 10 ms tick).  Data only --
no reference source text.  Also records the per-fixture generator parameters that reproduce them.

Run:  python tests/golden/make_golden_a.py      (needs /root/reference)
"""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/AMR_code_DART/MATLAB_trajectories"

# name -> (directory, gait, phi, disp_A)            parameters per SURVEY.md A.3
FIXTURES = {
    "walk_phi0":      ("walking/phi0_10cm_50",   "walk", 0.0,        0.10),
    "walk_phipi4":    ("walking/phipi4_10cm_50", "walk", np.pi / 4,  0.10),
    "walk_phipi2":    ("walking/phipi2_10cm_50", "walk", np.pi / 2,  0.10),
    "trot_phi0":      ("trotting/phi0",          "trot", 0.0,        0.15),
    "trot_phipi4":    ("trotting/phipi4",        "trot", np.pi / 4,  0.10),
    "trot_phipi4_15": ("trotting/phipi4/15cm",   "trot", np.pi / 4,  0.15),
    "trot_phipi2":    ("trotting/phipi2",        "trot", np.pi / 2,  0.15),
}


def main():
    meta = {}
    for name, (d, gait, phi, dA) in FIXTURES.items():
        files = os.listdir(os.path.join(REF, d))
        traj = [f for f in files if f.startswith("ComTrajectory")][0]
        vel = [f for f in files if f.startswith("ComVelocity")]
        com = np.loadtxt(os.path.join(REF, d, traj))
        arrs = {"com": com}
        if vel:
            arrs["vel"] = np.loadtxt(os.path.join(REF, d, vel[0]))
        for ft in ("fl", "fr", "rl", "rr"):                       # swing-foot files
            ff = [f for f in files if f.startswith(f"foot_{ft}_")]
            if ff:
                arrs[f"foot_{ft}"] = np.loadtxt(os.path.join(REF, d, ff[0]))
        np.savez_compressed(os.path.join(HERE, f"formA_matlab_{name}.npz"), **arrs)
        meta[name] = {"source": f"AMR_code_DART/MATLAB_trajectories/{d}/{traj}", "gait": gait, "phi": phi, "disp_A": dA,
                      "rows": int(com.shape[0]), "has_velocity": bool(vel)}
        print(name, com.shape, "vel" if vel else "-")
    json.dump(meta, open(os.path.join(HERE, "formA_matlab_meta.json"), "w"), indent=1)


if __name__ == "__main__":
    main()


def make_prerolls():
    """Nominal closed-loop state tables for the Formulation-A batch generator:
    the instance state at the start of every tick, in the product's ismpc_a_state layout.  CPU oracle (GI)."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from oracle import oracle_a as A
    from quadruped_gait_generation_ismpc_amd.formulation_a import STATE_A
    cases = {"walk_C100": (A.WALK, np.pi / 4, 0.1, dict()),
             "walk_C150": (A.WALK, np.pi / 4, 0.1, dict(C_=150, P=300, F=4)),        # BASELINE config 4
             "trot_C160": (A.TROT, np.pi / 4, 0.1, dict())}
    for name, (kind, phi, dA, over) in cases.items():
        sim = A.SimA(A.gait(kind, phi, dA), A.params(kind, **over), backend="gi")
        _, ce = A.plan(A.gait(kind, phi, dA))
        ticks = 1500
        tab = np.zeros(ticks, dtype=STATE_A)
        for t in range(ticks):
            o = sim.state
            fsx, fsy, _, _ = sim.get_plan()
            for k in ("x", "xd", "xz", "y", "yd", "yz", "cur_x", "cur_y", "fc", "j"):
                tab[k][t] = o[k]
            tab["off_x"][t] = fsx[0] - ce[0, 0]; tab["off_y"][t] = fsy[0] - ce[0, 1]; tab["rebuilt"][t] = int(o["fc"] >= 2)
            r = sim.tick()
            assert r["rv"][0] == 0 and r["rv"][1] == 0, (name, t)
        np.savez_compressed(os.path.join(HERE, f"prerollA_{name}.npz"), state=tab.view(np.uint8).reshape(ticks, -1),
                            gait=np.int64(kind), phi=np.float64(phi), disp_A=np.float64(dA),
                            C=np.int64(sim.p.C), P=np.int64(sim.p.P), F=np.int64(sim.p.F))
        print("preroll", name, "x_end", tab["x"][-1], tab["y"][-1])


def make_feet_states():
    """States of the swing-foot tests (tests/helpers/feet_cases.py): the oracle's unpushed closed loop at two ticks per footstep
    counter 1 .. 10, in the product's ismpc_a_state layout, with the oracle's first predicted footstep of the tick from each."""
    import importlib.util
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    spec = importlib.util.spec_from_file_location("feet_cases", os.path.join(os.path.dirname(HERE), "helpers", "feet_cases.py"))
    F = importlib.util.module_from_spec(spec); spec.loader.exec_module(F)
    arrs = {}
    for name, (kind, phi) in F.CONFIGS.items():
        st, f0 = F.harvest_from_oracle(kind, phi)
        arrs[name + "_state"] = st.view(np.uint8).reshape(len(st), -1); arrs[name + "_f0"] = f0
        print("feet states", name, len(st))
    np.savez_compressed(os.path.join(HERE, "feetA_states.npz"), **arrs)


if __name__ == "__main__":
    make_prerolls()
    make_feet_states()
