#!/usr/bin/env python3
"""Generate tests/golden/plant_params/plant_params.npz by running the REFERENCE's own vehicleSimulator.main() loop (read from the
reference tree at generation time only) with a vehicle of its own per case: the parameter dict that rospy.get_param reads sets lf,
lr, m, Iz and simulator/mu, which Simulator.__init__ reads (vehicleSimulator.py:128-137), next to the actuator's simulator/delay_a,
simulator/delay_df and simulator/lowLevelDyn.  The loop, the command schedule (held 7, 7, 6 steps) and the recording are those of
../actuator/make_actuator_golden.py (its run_case), over STEPS steps.  The reference's tyre is the constant 60, so this fixture
pins lf, lr, m, Iz and mu; tests/_plant_params_ref.py restates Cf and Cr.

Captured, per case c (all float64 / int32):
  params[c]                  [lf, lr, m, Iz, Cf, Cr, mu] of the case (Cf = Cr = 60: the reference's tyre)
  delay_a[c], delay_df[c]    seconds; La[c], Ld[c] = int(delay / dt); lld[c] simulator/lowLevelDyn
  cmd[c][k]                  [motor, servo] the ecu callback had delivered when step k ran
  applied[c][k]              [a, delta] Simulator.f received at step k
  state[c][k]                [x y vx vy ax ay yaw psiDot] after step k
  plant0, hold, dt
The key set is recorded in MANIFEST.json next to the fixture.

Usage:  python tests/golden/plant_params/make_plant_params_golden.py [--out DIR]   (needs the reference tree; not run on the GPU machine)
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.dirname(HERE)
ROOT = os.path.dirname(os.path.dirname(GOLDEN))
sys.path.insert(0, ROOT)
sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.join(GOLDEN, "estimator"))
sys.path.insert(0, os.path.join(GOLDEN, "actuator"))

STEPS = 300
# (lf, lr, m, Iz, mu, delay_a, delay_df, lowLevelDyn): the nominal car, heavier / lighter, other yaw inertias, asymmetric axles,
# no drag and more drag; delays and the servo lag on some cases
CASES = ((0.125, 0.125, 1.98, 0.03, 0.05, 0.0, 0.0, False),
         (0.125, 0.125, 2.40, 0.04, 0.08, 0.0, 0.0, False),
         (0.14, 0.11, 1.70, 0.03, 0.05, 0.0, 0.0, False),
         (0.125, 0.125, 2.20, 0.025, 0.03, 0.02, 0.035, True),
         (0.10, 0.15, 1.98, 0.045, 0.0, 0.0, 0.0, False),
         (0.125, 0.125, 1.60, 0.02, 0.10, 0.145, 0.1, True),
         (0.13, 0.12, 2.50, 0.035, 0.06, 0.0, 0.145, True),
         (0.125, 0.125, 2.277, 0.0255, 0.025, 0.0, 0.0, True))


def main():
    out_dir = HERE
    if "--out" in sys.argv:
        out_dir = sys.argv[sys.argv.index("--out") + 1]
    import make_estimator_golden as EG
    from lpvmpc.observer import observer_vertex_gains
    EG.install_estimator_stubs(observer_vertex_gains(EG.LIM_LS), observer_vertex_gains(EG.LIM_HS))
    _EST, SIM = EG.import_estimator()
    import make_golden as MG
    import make_actuator_golden as AG
    AG.STEPS = STEPS
    DT = AG.DT
    plant0 = np.array([0.01, 0.0, MG.PARAMS["simulator/init_vx"], 0.0, 0.0, 0.0, 0.0, 0.0])
    saved = {k: MG.PARAMS[k] for k in ("lf", "lr", "m", "Iz", "simulator/mu")}
    data = {k: [] for k in ("params", "delay_a", "delay_df", "La", "Ld", "lld", "cmd", "applied", "state")}
    try:
        for c, (lf, lr, m, Iz, mu, da, dd, lld) in enumerate(CASES):
            MG.PARAMS.update({"lf": lf, "lr": lr, "m": m, "Iz": Iz, "simulator/mu": mu})
            cmd, applied, st = AG.run_case(SIM, 2000 + c, da, dd, lld)
            data["params"].append([lf, lr, m, Iz, 60.0, 60.0, mu])
            data["delay_a"].append(da); data["delay_df"].append(dd)
            data["La"].append(int(da / DT)); data["Ld"].append(int(dd / DT)); data["lld"].append(int(lld))
            data["cmd"].append(cmd[:STEPS]); data["applied"].append(applied); data["state"].append(st)
    finally:
        MG.PARAMS.update(saved)
    out = {k: np.array(v, dtype=np.int32 if k in ("La", "Ld", "lld") else np.float64) for k, v in data.items()}
    assert out["state"].shape == (len(CASES), STEPS, 8) and out["applied"].shape == (len(CASES), STEPS, 2)
    out["plant0"] = plant0
    out["hold"] = np.array(AG.HOLD, np.int32)
    out["dt"] = np.array(DT)
    np.savez(os.path.join(out_dir, "plant_params.npz"), **out)
    manifest = {"plant_params.npz": {k: {"shape": list(np.shape(v)), "dtype": str(np.asarray(v).dtype)} for k, v in sorted(out.items())}}
    with open(os.path.join(out_dir, "MANIFEST.json"), "w") as fh:
        json.dump(manifest, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote plant_params.npz:", ", ".join("%s%s" % (k, list(np.shape(v))) for k, v in sorted(out.items())))


if __name__ == "__main__":
    main()
