#!/usr/bin/env python3
"""Generate tests/golden/actuator/actuator.npz by running the REFERENCE's own vehicleSimulator.main() loop (read from the
reference tree at generation time only), converted with lib2to3 and imported with stub ROS modules as
../estimator/make_estimator_golden.py does:

  * rospy.get_param reads a dict (the case's simulator/delay_a, simulator/delay_df, simulator/lowLevelDyn);
  * the `ecu` subscriber's callback is driven from a command schedule inside the Rate.sleep stub: after simulator step k the
    callback receives the command of step k + 1 (step 0 runs on EcuClass's initial [0, 0]);
  * rospy.is_shutdown turns true after STEPS steps;
  * the plant state is recorded from the simulator's own histories (Simulator.saveHistory: x, y, vx, vy, ax, ay, psiDot)
    and the published simulatorStates message (psi = Simulator.yaw); the input Simulator.f received is recorded as well.

The schedule holds each command for 7, 7, 6 simulator steps in turn, as the fleets do (one control tick = 7 or 6 steps of 5 ms).

Captured, per case c (all float64 / int32):
  delay_a[c], delay_df[c]    seconds (simulator/delay_a, simulator/delay_df)
  La[c], Ld[c]               the FIFO lengths main() built: int(delay / dt), kept as data
  lld[c]                     simulator/lowLevelDyn
  cmd[c][k]                  [motor, servo] the ecu callback had delivered when step k ran (ecu.u)
  applied[c][k]              [a, delta] Simulator.f received at step k
  state[c][k]                [x y vx vy ax ay yaw psiDot] after step k
  plant0                     the Simulator's initial state
  hold                       the schedule's hold lengths
The key set is recorded in MANIFEST.json next to the fixture.

Usage:  python tests/golden/actuator/make_actuator_golden.py [--out DIR]   (needs the reference tree; not run on the GPU machine)
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

DT = 0.005
STEPS = 400
HOLD = (7, 7, 6)
# (delay_a, delay_df, lowLevelDyn): none, a few steps, 0.145 s (int(0.145 / 0.005) = 28, not 29), 0.035 s (7.000000000000001 -> 7),
# the 64-step cap, each with the servo lag off and on
CASES = ((0.0, 0.0, False), (0.0, 0.0, True), (0.02, 0.035, False), (0.015, 0.025, True), (0.145, 0.145, False),
         (0.145, 0.1, True), (0.0, 0.145, True), (0.32, 0.32, False))


def schedule(case, steps=STEPS):
    """[steps][2] = (motor, servo) commands, one per hold of 7 / 7 / 6 steps; a fixed pseudo-random sequence per case."""
    rng = np.random.default_rng(1000 + case)
    out, k, h = np.zeros((steps, 2)), 0, 0
    while k < steps:
        n = HOLD[h % 3]
        out[k:k + n] = (rng.uniform(-0.6, 1.6), rng.uniform(-0.3, 0.3))
        k += n; h += 1
    return out


def run_case(SIM, case, delay_a, delay_df, lld):
    import make_golden as MG
    import make_estimator_golden as EG
    rospy = sys.modules["rospy"]
    MG.PARAMS.update({"simulator/delay_a": delay_a, "simulator/delay_df": delay_df, "simulator/lowLevelDyn": lld})
    EG.TOPICS.clear()
    EG.CLOCK[0] = 0.0
    sched = schedule(case)
    rec = {"applied": [], "yaw": [], "cmd": []}
    sims = []
    count = [0]

    class _Rate(object):
        def __init__(self, *a, **k):
            pass

        def sleep(self):                          # end of simulator step count[0]: deliver the next step's command
            count[0] += 1
            EG.CLOCK[0] = count[0] * DT
            if count[0] < STEPS:
                m = type("ECU", (object,), {})()
                m.motor, m.servo = float(sched[count[0], 0]), float(sched[count[0], 1])
                for cb in EG.TOPICS.get("ecu", []):
                    cb(m)

    orig_f, orig_init = SIM.Simulator.f, SIM.Simulator.__init__

    def f(self, u):
        rec["applied"].append([float(u[0]), float(u[1])])
        return orig_f(self, u)

    def init(self):
        orig_init(self)
        sims.append(self)

    SIM.Simulator.f, SIM.Simulator.__init__ = f, init
    EG.TOPICS.setdefault("simulatorStates", []).append(lambda msg: rec["yaw"].append(float(msg.psi)))
    rospy.Rate = _Rate
    rospy.is_shutdown = lambda: count[0] >= STEPS
    # the command the callback has delivered when each step runs: ecu.u is [motor, servo]; step 0 sees EcuClass's [0, 0]
    cmd = np.vstack([np.zeros((1, 2)), sched[1:]])
    try:
        SIM.main()
    finally:
        SIM.Simulator.f, SIM.Simulator.__init__ = orig_f, orig_init
    sim = sims[0]
    st = np.column_stack([sim.x_his, sim.y_his, sim.vx_his, sim.vy_his, sim.ax_his, sim.ay_his, rec["yaw"], sim.psiDot_his])
    return cmd, np.array(rec["applied"]), st


def main():
    out_dir = HERE
    if "--out" in sys.argv:
        out_dir = sys.argv[sys.argv.index("--out") + 1]
    import make_estimator_golden as EG
    from lpvmpc.observer import observer_vertex_gains
    EG.install_estimator_stubs(observer_vertex_gains(EG.LIM_LS), observer_vertex_gains(EG.LIM_HS))
    _EST, SIM = EG.import_estimator()
    import make_golden as MG
    plant0 = np.array([0.01, 0.0, MG.PARAMS["simulator/init_vx"], 0.0, 0.0, 0.0, 0.0, 0.0])
    data = {k: [] for k in ("delay_a", "delay_df", "La", "Ld", "lld", "cmd", "applied", "state")}
    for c, (da, dd, lld) in enumerate(CASES):
        cmd, applied, st = run_case(SIM, c, da, dd, lld)
        data["delay_a"].append(da); data["delay_df"].append(dd)
        data["La"].append(int(da / DT)); data["Ld"].append(int(dd / DT)); data["lld"].append(int(lld))
        data["cmd"].append(cmd); data["applied"].append(applied); data["state"].append(st)
    out = {k: np.array(v, dtype=np.int32 if k in ("La", "Ld", "lld") else np.float64) for k, v in data.items()}
    out["plant0"] = plant0
    out["hold"] = np.array(HOLD, np.int32)
    out["dt"] = np.array(DT)
    np.savez(os.path.join(out_dir, "actuator.npz"), **out)
    manifest = {"actuator.npz": {k: {"shape": list(np.shape(v)), "dtype": str(np.asarray(v).dtype)} for k, v in sorted(out.items())}}
    with open(os.path.join(out_dir, "MANIFEST.json"), "w") as fh:
        json.dump(manifest, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote actuator.npz:", ", ".join("%s%s" % (k, list(np.shape(v))) for k, v in sorted(out.items())))


if __name__ == "__main__":
    main()
