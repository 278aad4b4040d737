#!/usr/bin/env python3
"""Cost of the gain-scheduled LPV estimator in the loop: vehicle-ticks/s of the f1 closed-loop fleet (lap-0 controller + plant
+ map) at 1024 and 8192 vehicles with the estimator off, on with zero noise and on with sensor noise, and of the planner +
controller cascade (tools/cascade_bench.py's cfg5 setup: lap-event starts, L-shape track) with the estimator off and on.

Gains: the synthetic vertex gains of tests/golden/estimator/estimator.npz (lpvmpc.observer_vertex_gains).  Each row is one
timed run of --ticks control ticks after a warm-up; "delta" is the extra wall time per control tick against the row with the
estimator off (the fused plant + sensors + observer launch replaces the plant launch; the solve is unchanged).
"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import lpvmpc
from lpvmpc import workloads as W

ap = argparse.ArgumentParser()
ap.add_argument("--fleets", default="1024,8192")
ap.add_argument("--ticks", type=int, default=200)
ap.add_argument("--cascade-ticks", type=int, default=150)
ap.add_argument("--no-cascade", action="store_true")
args = ap.parse_args()

g = np.load(os.path.join(ROOT, "tests", "golden", "estimator", "estimator.npz"))
NOISE = dict(psi_std=0.01, psiDot_std=0.05, x_std=0.01, y_std=0.01, v_std=0.02, seed=1)
MODES = (("off", None), ("on, zero noise", {}), ("on, noise", NOISE))


def obs_cfg(kw):
    return lpvmpc.observer_config(g["L_ls"], g["lim_ls"], g["L_hs"], g["lim_hs"], **kw)


Q, R, dR = W.CTRL_TUNINGS["path"]
mp = lpvmpc.Map("oval", 0.2)
for B in [int(v) for v in args.fleets.split(",")]:
    base = None
    for name, kw in MODES:
        eng = lpvmpc.BatchedSolver("controller", 20, 1 / 30.0, Q, R, dR, track=mp.PointAndTangent)
        rng = np.random.default_rng(3)
        s0 = rng.uniform(0.05, 12.5, B); ey0 = rng.normal(0, 0.03, B)
        xyth = eng.global_position(np.column_stack([s0, ey0]))
        plant0 = np.column_stack([xyth[:, 0], xyth[:, 1], rng.uniform(0.8, 1.2, B), np.zeros(B), np.zeros(B), np.zeros(B), xyth[:, 2], np.zeros(B)])
        if kw is not None:
            eng.observer_setup(obs_cfg(kw))
        eng.cl_init(plant0, mp.halfWidth, mp.slack, q9_swap=True, n_sub=7)
        eng.cl_tick(20); eng.cl_read()                     # seed phase + warm-up
        T = args.ticks
        t = time.perf_counter(); eng.cl_tick(T); o = eng.cl_read(); t = time.perf_counter() - t
        ms = t / T * 1e3
        base = ms if kw is None else base
        print("f1      B=%5d estimator %-15s %d ticks in %.3f s -> %.3f ms/tick, %.0f vehicle-ticks/s, solved %.3f, iters mean %.1f%s"
              % (B, name, T, t, ms, B * T / t, np.mean(np.isin(o["status"], (1, 2))), o["iters"].mean(),
                 "" if kw is None else ", delta %+.3f ms/tick" % (ms - base)), flush=True)
        eng.close()

if not args.no_cascade:
    c = np.load(os.path.join(ROOT, "tests", "golden", "cascade.npz"))
    mpl = lpvmpc.Map("L_shape", 0.2)
    Qr, Rr, dRr = W.CTRL_TUNINGS["race"]
    for B in [int(v) for v in args.fleets.split(",")]:
        rng = np.random.default_rng(3)
        plant0 = np.tile(c["plant0"], (B, 1))
        plant0[:, 1] += rng.normal(0, 0.01, B); plant0[:, 6] += rng.normal(0, 0.01, B); plant0[:, 2] += rng.uniform(-0.05, 0.3, B)
        cmd0 = np.tile(c["cmd0"], (B, 1)); uPred0 = np.tile(c["uPred0"], (B, 1, 1))
        base = None
        for name, kw in (MODES[0], MODES[1]):
            plan = lpvmpc.BatchedSolver("planner", 40, 0.05, W.PLAN_Q, W.PLAN_R, W.PLAN_dR, L_cf=W.PLAN_L, track=mpl.PointAndTangent)
            plan.handoff_setup()
            ctrl = lpvmpc.BatchedSolver("controller", 20, 1 / 30.0, Qr, Rr, dRr, track=mpl.PointAndTangent)
            if kw is not None:
                ctrl.observer_setup(obs_cfg(kw))
            ctrl.cascade_init(plan, plant0, cmd0, uPred0, half_width=mpl.halfWidth, slack=mpl.slack, plan_max_ey=0.2)
            ctrl.cascade_tick(3); ctrl.cascade_read(full=False)
            T = args.cascade_ticks
            t = time.perf_counter(); ctrl.cascade_tick(T); o = ctrl.cascade_read(full=False); t = time.perf_counter() - t
            ms = t / T * 1e3
            base = ms if kw is None else base
            alive = np.all(np.isfinite(o["plant"]), axis=1)
            print("cascade B=%5d estimator %-15s %d ctrl ticks in %.3f s -> %.3f ms/tick, %.0f vehicle-ticks/s, alive %.4f%s"
                  % (B, name, T, t, ms, B * T / t, alive.mean(), "" if kw is None else ", delta %+.3f ms/tick" % (ms - base)), flush=True)
            ctrl.close(); plan.close()
