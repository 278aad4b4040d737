#!/usr/bin/env python3
"""Generate tests/golden/tyre/tyre.npz from the REFERENCE's own Simulator.pacejka (vehicleSimulator.py:202-205; read from the
reference tree at generation time only, imported with stub ROS modules as ../estimator/make_estimator_golden.py does).  Per case a
Simulator is built from the parameter dict that rospy.get_param reads -- m, simulator/B, simulator/C, simulator/c_f, which
Simulator.__init__ reads -- and its BOUND METHOD pacejka is what computes every force below.

  1. Curve: pacejka(alpha) at 257 angles in [-1, 1] rad for each parameter set (the launch file's first).
  2. Trajectories: STEPS steps of a step function whose FyF, FyR come from that bound method.  In the reference the two calls
     `FyF = self.pacejka(a_F)`, `FyR = self.pacejka(a_R)` in Simulator.f are COMMENTED OUT (vehicleSimulator.py:172-173; f uses
     60 * a_F): so the curve is the reference's, and the recursion around it is the restatement of Simulator.f in
     tests/_tyre_ref.py (simulator_f_forces; with the linear tyre it is tests/_plant_params_ref.py's, which
     tests/golden/plant_params/ pins to the reference's loop), with the actuator of tests/_actuator_ref.py (pinned by
     tests/golden/actuator/).  A kind 0 case steps the linear tyre of its plant row.

Captured (float64 / int32):
  curve_sets[s] = [m, B, C, c_f], curve_alpha [257], curve_force[s][257]
  params[c] = [lf lr m Iz Cf Cr mu], tyre[c] = [kind B C c_f], La[c], Ld[c], lld[c]
  cmd[c][k] = [motor, servo], applied[c][k] = [a, delta], state[c][k] = [x y vx vy ax ay yaw psiDot] after step k,
  slip[c][k] = [a_F, a_R] of step k; plant0, dt
The key set is recorded in MANIFEST.json next to the fixture.

Usage:  python tests/golden/tyre/make_tyre_golden.py [--out DIR]   (needs the reference tree; not run on the GPU machine)
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
DT = 0.005
# (m, B, C, c_f): the launch file's, a soft tyre, a stiff grippy one on a heavy car, a light car on a slippery surface, C below 1
CURVE_SETS = ((1.98, 6.0, 1.6, 0.8), (1.98, 4.0, 1.3, 0.5), (2.5, 9.0, 1.9, 1.1), (1.6, 5.0, 1.45, 0.35), (2.2, 7.5, 0.9, 0.8))
# (lf, lr, m, Iz, Cf, Cr, mu), (kind, B, C, c_f), La, Ld, lowLevelDyn, command: "square" = motor 1.5, servo +-0.40 every 40 steps;
# "sched" = the actuator fixture's schedule of held pseudo-random commands
CASES = (((0.125, 0.125, 1.98, 0.03, 60.0, 60.0, 0.05), (1, 6.0, 1.6, 0.8), 0, 0, False, "square"),
         ((0.125, 0.125, 2.40, 0.04, 60.0, 60.0, 0.08), (1, 4.0, 1.3, 0.5), 0, 0, False, "square"),
         ((0.14, 0.11, 1.70, 0.03, 60.0, 60.0, 0.05), (1, 6.0, 1.6, 0.8), 0, 0, False, "sched"),
         ((0.125, 0.125, 2.20, 0.025, 45.0, 70.0, 0.03), (1, 9.0, 1.9, 1.1), 4, 7, True, "square"),
         ((0.10, 0.15, 1.98, 0.045, 52.0, 66.0, 0.0), (0, 6.0, 1.6, 0.8), 0, 0, False, "square"),
         ((0.125, 0.125, 1.60, 0.02, 60.0, 60.0, 0.10), (1, 5.0, 1.45, 0.35), 28, 20, True, "sched"),
         ((0.13, 0.12, 2.50, 0.035, 60.0, 60.0, 0.06), (1, 7.5, 0.9, 0.8), 0, 28, True, "sched"),
         ((0.125, 0.125, 2.277, 0.0255, 60.0, 60.0, 0.025), (1, 6.6, 1.7, 0.95), 0, 0, True, "square"))


def commands(case, kind):
    if kind == "square":
        k = np.arange(STEPS)
        return np.column_stack([np.full(STEPS, 1.5), np.where((k // 40) % 2 == 0, 0.40, -0.40)])
    import make_actuator_golden as AG
    return AG.schedule(3000 + case, STEPS)


def reference_simulator(SIM, MG, m, B, C, c_f):
    """A Simulator of the reference built with the case's mass and tyre words."""
    MG.PARAMS.update({"m": m, "simulator/B": B, "simulator/C": C, "simulator/c_f": c_f})
    sim = SIM.Simulator()
    assert (sim.m, sim.B, sim.C, sim.c_f) == (m, B, C, c_f)
    return sim


def main():
    out_dir = HERE
    if "--out" in sys.argv:
        out_dir = sys.argv[sys.argv.index("--out") + 1]
    import make_estimator_golden as EG
    from lpvmpc.observer import observer_vertex_gains
    EG.install_estimator_stubs(observer_vertex_gains(EG.LIM_LS), observer_vertex_gains(EG.LIM_HS))
    _EST, SIM = EG.import_estimator()
    import make_golden as MG
    from tests import _tyre_ref as T
    saved = {k: MG.PARAMS[k] for k in ("m", "simulator/B", "simulator/C", "simulator/c_f")}
    plant0 = np.array([0.01, 0.0, MG.PARAMS["simulator/init_vx"], 0.0, 0.0, 0.0, 0.0, 0.0])
    alpha = np.linspace(-1.0, 1.0, 257)
    out = {"curve_sets": np.array(CURVE_SETS), "curve_alpha": alpha, "plant0": plant0, "dt": np.array(DT)}
    data = {k: [] for k in ("params", "tyre", "La", "Ld", "lld", "cmd", "applied", "state", "slip")}
    try:
        assert len(CURVE_SETS) >= 4 and CURVE_SETS[0] == (1.98, 6.0, 1.6, 0.8)
        out["curve_force"] = np.array([[float(reference_simulator(SIM, MG, *s).pacejka(a)) for a in alpha] for s in CURVE_SETS])
        beyond_peak = 0
        for c, (row, tyre, La, Ld, lld, kind) in enumerate(CASES):
            sim = reference_simulator(SIM, MG, row[2], *tyre[1:])
            pac = lambda aF, aR, _row, sim=sim: (float(sim.pacejka(aF)), float(sim.pacejka(aR)))      # the reference's bound method
            cmd = commands(c, kind)
            st, ap, slip = T.simulate(plant0, cmd, row, pac if tyre[0] else T.linear_forces, La, Ld, lld, DT)
            lin = T.simulate(plant0, cmd, row, T.linear_forces, La, Ld, lld, DT)[0]
            assert np.all(np.isfinite(st)), c
            if tyre[0]:
                assert np.max(np.abs(st[:, 7] - lin[:, 7])) > 1e-3, c                      # the tyre matters to the trajectory
                beyond_peak += np.max(np.abs(slip)) > 0.3
            else:
                assert np.array_equal(st, lin)
            for k, v in zip(("params", "tyre", "La", "Ld", "lld", "cmd", "applied", "state", "slip"), (row, tyre, La, Ld, int(lld), cmd, ap, st, slip)):
                data[k].append(v)
            print("case %d: max |alpha| %.3f, max |psiDot - linear| %.3e" % (c, np.max(np.abs(slip)), np.max(np.abs(st[:, 7] - lin[:, 7]))))
    finally:
        MG.PARAMS.update(saved)
    out.update({k: np.array(v, dtype=np.int32 if k in ("La", "Ld", "lld") else np.float64) for k, v in data.items()})
    # the case rules
    assert len(CASES) == 8 and out["state"].shape == (8, STEPS, 8)
    for i in (2, 3, 6):                                                                    # m, Iz, mu vary; so do lf / lr and the tyre words
        assert len(set(out["params"][:, i])) >= 4
    assert len({tuple(r[:2]) for r in out["params"]}) >= 3 and len({tuple(r) for r in out["tyre"]}) >= 6
    assert np.sum((out["La"] > 0) | (out["Ld"] > 0) | (out["lld"] > 0)) >= 2 and np.sum(out["tyre"][:, 0] == 0) == 1
    assert beyond_peak >= 2, beyond_peak
    np.savez(os.path.join(out_dir, "tyre.npz"), **out)
    manifest = {"tyre.npz": {k: {"shape": list(np.shape(v)), "dtype": str(np.asarray(v).dtype)} for k, v in sorted(out.items())}}
    with open(os.path.join(out_dir, "MANIFEST.json"), "w") as fh:
        json.dump(manifest, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote tyre.npz:", ", ".join("%s%s" % (k, list(np.shape(v))) for k, v in sorted(out.items())))


if __name__ == "__main__":
    main()
