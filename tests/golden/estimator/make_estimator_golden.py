#!/usr/bin/env python3
"""Generate tests/golden/estimator/estimator.npz by running the REFERENCE's own stateEstimator.py and vehicleSimulator.py
(read from the reference tree at generation time only), the way ../make_golden.py does: the modules are copied to a temp dir,
converted with lib2to3 and imported with stub ROS modules.  Here the stubs also carry messages: rospy.Publisher / Subscriber
connect the simulator's sensor topics to the estimator's callbacks, and rospy.get_rostime reads a simulated clock that the
generator advances by dt per step (the estimator's start-up test `curr_time > 0.02` then sees t = k dt).

scipy.io.loadmat is patched to return synthetic gains from lpvmpc.observer_vertex_gains (the reference's .mat files are not
available); the tables are stored in the fixture.

Captured (numbers only, all float64):
  * grid_*   single GS_LPV_Est steps over both polytopes, the start-up branch and points outside the polytopes:
             inputs (est, y, u, k) and outputs (L_gain, A_obs, B_obs, new state);
  * trace_*  2 s open loop of the reference Simulator + sensors + Estimator under a scripted command, stds 0: per step the
             plant state, the measurement y the observer used, the command and the estimate.
The key set is recorded in MANIFEST.json next to the fixture.

Usage:  python tests/golden/estimator/make_estimator_golden.py   (needs the reference tree; not run on the GPU machine)
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.dirname(HERE)
ROOT = os.path.dirname(os.path.dirname(GOLDEN))
sys.path.insert(0, ROOT)
sys.path.insert(0, GOLDEN)

import make_golden as MG  # noqa: E402
from lpvmpc.observer import observer_vertex_gains  # noqa: E402

LIM_LS = np.array([[0.1, 1.1], [-0.3, 0.3], [-3.0, 3.0], [-0.3, 0.3], [-1.0, 1.0], [-np.pi, np.pi]])
LIM_HS = np.array([[1.0, 4.0], [-0.3, 0.3], [-3.0, 3.0], [-0.3, 0.3], [-1.0, 1.0], [-np.pi, np.pi]])
DT = 0.005
CLOCK = [0.0]
TOPICS = {}


def install_estimator_stubs(L_ls, L_hs):
    MG.install_stubs()
    rospy = sys.modules["rospy"]

    class _Time(object):
        def __init__(self, t):
            self.t = t

        def to_sec(self):
            return self.t

    class _Pub(object):
        def __init__(self, topic, *a, **k):
            self.topic = topic

        def publish(self, msg):
            for cb in TOPICS.get(self.topic, []):
                cb(msg)

    rospy.get_rostime = lambda: _Time(CLOCK[0])
    rospy.Publisher = _Pub
    rospy.Subscriber = lambda topic, typ, cb, **k: TOPICS.setdefault(topic, []).append(cb)
    rospy.init_node = lambda *a, **k: None
    MG.PARAMS.update({"simulator/gps_freq_update": 1000.0, "simulator/lowLevelDyn": False, "simulator/delay_a": 0.0,
                      "simulator/delay_df": 0.0, "simulator/n_bound": 0.5, "simulator/x_std": 0.0, "simulator/y_std": 0.0,
                      "simulator/psi_std": 0.0, "simulator/v_std": 0.0, "simulator/psiDot_std": 0.0,
                      "simulator/ax_std": 0.0, "simulator/ay_std": 0.0})
    for name in ("std_msgs", "std_msgs.msg"):
        sys.modules[name] = sys.modules["barc"].__class__(name)
    import scipy.io as sio
    sio.loadmat = lambda path, *a, **k: ({"Llmi": L_hs, "SchedVars_Limits": LIM_HS} if "_HS" in path
                                          else {"Llmi": L_ls, "SchedVars_Limits": LIM_LS})


def import_estimator():
    import shutil
    import subprocess
    import tempfile
    tmp = tempfile.mkdtemp(prefix="estimport_")
    for rel in ("Utilities/trackInitialization.py", "vehicleSimulator.py", "stateEstimator.py"):
        shutil.copy(os.path.join(MG.REF, rel), tmp)
    subprocess.run([sys.executable, "-m", "lib2to3", "-w", "-n", tmp], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    for f in ("vehicleSimulator.py", "stateEstimator.py"):
        p = os.path.join(tmp, f)
        with open(p) as fh:
            lines = [ln.expandtabs(8) for ln in fh]
        with open(p, "w") as fh:
            fh.writelines(lines)
    sys.path.insert(0, tmp)
    import stateEstimator as EST
    import vehicleSimulator as SIM
    return EST, SIM


def grid(EST):
    rng = np.random.default_rng(2026)
    rows = []
    # (vx range, k) pairs: LS, HS, start-up (k <= 4), far outside both polytopes
    for vlo, vhi, ks in ((0.15, 1.05, (10, 50)), (1.1, 3.9, (10, 200)), (0.2, 3.0, (1, 2, 3, 4)), (4.5, 6.0, (9,)),
                         (0.02, 0.09, (12,))):
        for _ in range(24):
            k = int(rng.choice(ks))
            est = np.array([rng.uniform(vlo, vhi), rng.uniform(-0.5, 0.5), rng.uniform(-4, 4), rng.uniform(-5, 5),
                            rng.uniform(-5, 5), rng.uniform(-5, 5)])
            y = np.array([rng.uniform(vlo, vhi), rng.uniform(-4, 4), est[3] + rng.normal(0, 0.1), est[4] + rng.normal(0, 0.1),
                          est[5] + rng.normal(0, 0.1)])
            u = np.array([rng.uniform(-0.45, 0.45), rng.uniform(-1.0, 1.0)])
            rows.append((est, y, u, k))
    out = {k: [] for k in ("est", "y", "u", "k", "L", "A", "B", "new")}
    for est, y, u, k in rows:
        e = EST.Estimator(0.0, 1.0 / DT, 0.0, 0.0)
        e.states_est = est.copy()
        e.prev_time = (k - 1) * DT
        CLOCK[0] = k * DT
        e.GS_LPV_Est(est, y, u, e.Continuous_AB_Comp, e.L_Gain_Comp)
        for key, v in (("est", est), ("y", y), ("u", u), ("k", k), ("L", e.L_gain), ("A", e.A_obs), ("B", e.B_obs),
                       ("new", e.states_est)):
            out[key].append(np.array(v, dtype=float))
    return {"grid_" + k: np.array(v) for k, v in out.items()}


def trace(EST, SIM, steps=400):
    TOPICS.clear()
    CLOCK[0] = 0.0
    sim = SIM.Simulator(); imu = SIM.ImuClass(); gps = SIM.GpsClass(1000.0, DT); enc = SIM.EncClass()
    e_imu = EST.ImuClass(0.0); e_gps = EST.GpsClass(0.0); e_enc = EST.EncClass(0.0); e_ecu = EST.EcuClass(0.0)
    e_sim = EST.SimulatorClass(0.0)
    est = EST.Estimator(0.0, 1.0 / DT, 0.0, 0.0)
    pub_sim = sys.modules["rospy"].Publisher("simulatorStates")
    msg_cls = type("simulatorStates", (object,), {})
    rec = {k: [] for k in ("plant", "y", "u", "est")}
    plant0 = np.array([sim.x, sim.y, sim.vx, sim.vy, sim.ax, sim.ay, sim.yaw, sim.psiDot])
    est0 = est.states_est.copy()
    for k in range(1, steps + 1):
        t = k * DT
        servo = 0.25 * np.sin(2.0 * t) + 0.05
        motor = 1.0 if t < 1.0 else 0.2 * np.cos(3.0 * t)
        e_ecu.a, e_ecu.df = motor, servo
        sim.f([motor, servo])
        m = msg_cls(); m.x, m.y, m.vx, m.vy, m.psi, m.psiDot = sim.x, sim.y, sim.vx, sim.vy, sim.yaw, sim.psiDot
        pub_sim.publish(m)
        imu.update(sim); gps.update(sim); enc.update(sim)
        gps.gps_pub(); imu.imu_pub(); enc.enc_pub()
        CLOCK[0] = t
        est.prev_time = t - DT
        y = (np.array([e_enc.v_meas, e_imu.psiDot, e_gps.x, e_gps.y, e_imu.yaw]) if t > 0.02
             else np.array([est.vx_est, e_imu.psiDot, e_gps.x, e_gps.y, e_sim.yaw]))
        est.estimateState(e_imu, e_gps, e_enc, e_ecu, e_sim, est.GS_LPV_Est, est.Continuous_AB_Comp, est.L_Gain_Comp)
        rec["plant"].append([sim.x, sim.y, sim.vx, sim.vy, sim.ax, sim.ay, sim.yaw, sim.psiDot])
        rec["y"].append(y); rec["u"].append([servo, motor]); rec["est"].append(est.states_est.copy())
    out = {"trace_" + k: np.array(v, dtype=float) for k, v in rec.items()}
    out["trace_plant0"] = plant0
    out["trace_est0"] = np.array(est0, dtype=float)
    return out


def main():
    L_ls, L_hs = observer_vertex_gains(LIM_LS), observer_vertex_gains(LIM_HS)
    install_estimator_stubs(L_ls, L_hs)
    EST, SIM = import_estimator()
    data = dict(L_ls=L_ls, lim_ls=LIM_LS, L_hs=L_hs, lim_hs=LIM_HS, dt=np.array(DT))
    data.update(grid(EST))
    data.update(trace(EST, SIM))
    np.savez(os.path.join(HERE, "estimator.npz"), **data)
    manifest = {"estimator.npz": {k: {"shape": list(np.shape(v)), "dtype": str(np.asarray(v).dtype)} for k, v in sorted(data.items())}}
    with open(os.path.join(HERE, "MANIFEST.json"), "w") as fh:
        json.dump(manifest, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote estimator.npz:", ", ".join("%s%s" % (k, list(np.shape(v))) for k, v in sorted(data.items())))


if __name__ == "__main__":
    main()
