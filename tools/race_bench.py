#!/usr/bin/env python3
"""Race engine cost (lpvmpc_race_*) against the engines it composes, at B = 1024 and 8192 vehicles:
  lap0     every vehicle in lap 0 (ticks 10 .. 10+K of a race from the grid)        vs lpvmpc_cl_tick at the same B
  inphase  every vehicle racing, one common event tick (cascade.npz's lap-0 start)   vs lpvmpc_cascade_tick, prefetch 0
  stagger  events spread over the last quarter of the lap (the engine's real case)   reported, not gated
Prints ms per controller tick and alive vehicle-ticks per second; one line per (regime, B).
--estimator: instead, the lap0 and inphase races run without and with the state estimator in the loop (lpvmpc_race_init_observed,
the reference's gain tables, noisy sensors), alternated --reps times per (regime, B); one line per (regime, B) with the median of each
and the added ms per controller tick.
--actuator: instead, the lap0 and inphase races run on the old entry (lpvmpc_race_init), on lpvmpc_race_init_actuated with the actuator
all off, with plant delays La = Ld = 20 steps and the servo lag (steeringDelay 0), and the same with steeringDelay 3 on both
controllers; alternated --reps times per (regime, B), medians and differences against the old entry.
--record: instead, the lap0 and inphase races run with recording off and on (lpvmpc_race_record, stride 1, a ring as long as the timed
window), alternated --reps times per (regime, B); medians and the added ms per controller tick.
--plant-params: instead, the lap0 and inphase races run on lpvmpc_race_init_actuated with the actuator all off, on
lpvmpc_race_init_vehicles with the nominal rows and with rows from plant.sample_plant_params (seed 1); alternated --reps times per
(regime, B), medians and differences against the all-off entry.  The sampled rows drive other trajectories, so their in-phase
lines also carry the solvers' changed iteration counts.
--models: instead, the lap0 and inphase races run unbound and with explicit nominal model rows bound to the three engines
(lpvmpc_set_model_params: the per-vehicle forms of the LPV kernels), and, with --parent-lib FILE (another build of the library, a file
name inside the package directory), unbound on that build; alternated --reps times per (regime, B), one child process per run (a
process loads one build); medians, each configuration's spread over the alternations and the differences against the unbound race.
--tunings: the same protocol for the per-vehicle tunings (lpvmpc_set_tunings): unbound, each handle's own tuning row bound to every
vehicle of the three engines (the cost of the binding: one 512-byte row per workgroup at set-up), and sampled rows on all three
(tuning.sample_tunings, seed 1, weights +-30 %: other QPs, so other iteration counts -- a launch ends in its slowest instance; reported,
not a regression), and, with --parent-lib FILE, unbound on that build.
--tyres: the same protocol for the tyre model: the lpvmpc_race_init_vehicles race with nominal rows (the baseline), the
lpvmpc_race_init_tyres race with kind 0 rows (the tyre forms of the kernels on the linear tyre) and with the launch file's Pacejka tyre on
every vehicle (other trajectories, so its in-phase lines also carry the solvers' changed iteration counts), and, with --parent-lib FILE,
the _vehicles race on that build.
--observer-vehicles: the same protocol for the per-vehicle estimator: the lpvmpc_race_init_vehicles race with nominal rows and the
estimator in the loop (the fixture's gain tables, noisy sensors), unbound (the baseline) and with a per-vehicle estimator bound to the
path engine (lpvmpc_set_observer_vehicles: nominal rows, tables designed on the device -- 7.7 KB of gain words per vehicle and observer
step from global memory instead of one table in LDS), and, with --parent-lib FILE, the unbound race on that build.
--tracks: the same protocol for the per-vehicle tracks (lpvmpc_set_tracks): the lpvmpc_race_init_tyres race with kind 0 rows, unbound
(the baseline), with a one-entry palette of the handles' own track bound to the three engines (the bound forms of every kernel that reads
the track, all lanes on one table), with the six-entry palette of track.palette(), track_of cycling (lap 0 from each track's grid; in
phase: every vehicle as far before the end of its own lap as the fixture's start is on the L shape -- other circuits, so other QPs and
other survivors), the same six tracks as six homogeneous sub-fleets of B / 6 vehicles ticked in turn in one process (the engines have
no stream of their own to run side by side on), and, with --parent-lib FILE, the unbound race on that build.  Every line carries
alive vehicle-ticks per second.
--disturbance: the same protocol for the plant disturbances (lpvmpc_set_disturbances): the lpvmpc_race_init_tyres race with kind 0 rows and
nothing attached (the baseline: the launches of the parent's tick), the same race with all three disturbances attached to every vehicle
(gusts of 0.3 on the three channels, a grip patch of 0.7 over the first 3 m of the lap, a kick at plant step 400: one more launch per
tick, and other trajectories, so the lines also carry the solvers' changed iteration counts), and, with --parent-lib FILE, the
nothing-attached race on that build.
--fork: the race's snapshot, restore and clone (lpvmpc_race_snapshot / _restore / _clone).  First the same protocol with one
configuration, the lpvmpc_race_init_tyres race with kind 0 rows that calls none of them, and, with --parent-lib FILE, the same race on
that build: nothing called, nothing paid.  Then, per B, in the in-phase regime at the first timed tick (every vehicle racing): the
median over --reps calls, in ms, of a snapshot (device to host, the blob's bytes), a restore of that blob, a clone with every vehicle
moved (a rotation by one) and a clone with 10 % of the vehicles moved (random slots from random sources), beside the ms per race tick
of the same regime as the scale (the parent's where --parent-lib is given); the blob's bytes per vehicle; and for the full clone
the GB/s over the bytes its two kernels read plus write (the state goes through the staging buffer: four times its size).
--heats SIZE: instead, the lap0 and inphase races run with heats detached and with heats of SIZE consecutive vehicles attached
(lpvmpc_race_heats: one more launch per tick, one workgroup per heat), alternated --reps times per (regime, B) in one process; medians, each
configuration's spread over the alternations and the added ms per controller tick; and, with --parent-lib FILE, the detached race on that
build, one child process per run: the launches are identical, so it must lie within the alternation's spread.
--interactions [--heats SIZE]: the --disturbance protocol for the interactions (lpvmpc_race_interactions): the lpvmpc_race_init_tyres race with
kind 0 rows and heats of SIZE (default 16) consecutive vehicles attached (the baseline: the launches of the parent's tick), the same race
with the all-off interactions attached (draft_gain 0, contact off: the same race word for word, so the difference is the launch), and
with the default interactions attached (another race: other trajectories, other QPs), alternated --reps times per (regime, B), each run in
a fresh process; with --parent-lib FILE the parent's library on the baseline as well.
--walls: the --interactions protocol for the walls (lpvmpc_race_walls): the lpvmpc_race_init_tyres race with kind 0 rows and nothing attached
(the baseline: the launches of the parent's tick), the same race with walls attached whose margin is so large that nothing touches (margin
50: the same race word for word, so the difference is the launch), and with the default walls attached (another race where a car meets a
wall); with --parent-lib FILE the parent's library on the baseline as well.
--contact [--heats SIZE]: the same protocol for the contact model (lpvmpc_race_contact): the --interactions race with the default interactions
attached (the baseline: the interactions' own launch; the bench's starts put a heat on one pose, so this is the pile-up start), the same
race with the contact model attached with friction 0 and yaw_response 0 (the same race word for word, so the difference is the new kernel
in place of the interactions'), and with the default contact model attached (another race); with --parent-lib FILE the parent's library
on the baseline as well.

Usage: tools/race_bench.py [--ticks K] [--sizes 1024,8192] [--estimator | --actuator | --record | --heats SIZE | --plant-params | --models |
       --tunings | --tyres | --observer-vehicles | --tracks | --disturbance | --sensor-faults | --interactions | --walls | --contact | --fork [--parent-lib FILE] [--reps R]]
       [--out FILE]
--sensor-faults: the same protocol for the sensor faults (lpvmpc_set_sensor_faults): the lpvmpc_race_init_tyres race with kind 0 rows and the
estimator in the loop with nothing attached (the baseline: the launches of the parent's tick), with all-off rows attached (the faulted
kernel in place of the fused observe kernel on the same trajectories: the kernel's own cost), the same race with every fault attached to
every vehicle (a GPS outage, a random loss, a jump, a gyro bias, a yaw drift, a slipping and a stuck encoder: the faulted kernel in place
of the fused observe kernel, no extra launch; other trajectories, so the lines also carry the solvers' changed iteration counts), and,
with --parent-lib FILE, the race with nothing attached on that build."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def engines(mp, sd=0):
    import lpvmpc
    from lpvmpc import workloads as W
    Qp, Rp, dRp = W.CTRL_TUNINGS["path"]; Qr, Rr, dRr = W.CTRL_TUNINGS["race"]
    kw = {"steering_delay": sd} if sd else {}
    path = lpvmpc.BatchedSolver("controller", 20, 1 / 30.0, Qp, Rp, dRp, track=mp.PointAndTangent, **kw)
    tt = lpvmpc.BatchedSolver("controller", 20, 1 / 30.0, Qr, Rr, dRr, track=mp.PointAndTangent, **kw)
    plan = lpvmpc.BatchedSolver("planner", 40, 0.05, W.PLAN_Q, W.PLAN_R, W.PLAN_dR, L_cf=W.PLAN_L, track=mp.PointAndTangent)
    plan.handoff_setup()
    return path, tt, plan


def timed(tick, read, K):
    read()
    t0 = time.perf_counter()
    tick(K)
    read()
    return (time.perf_counter() - t0) * 1e3 / K


def race_run(mp, plant0, half, warm, K, estimator=None, actuator=None, sd=0, record=False, plant_params=None, model_params=None, tunings=None,
             tyre_params=None, observer_vehicles=False, tracks=None, disturbance=None, heats=0, sensor_faults=None, interactions=None, walls=None,
             contact=None):
    path, tt, plan = engines(mp, sd)
    if tracks is not None:                                            # (maps, track_of) bound to the three engines
        for e in (path, tt, plan):
            e.set_tracks(*tracks)
    if observer_vehicles:                                             # nominal estimator rows, tables designed on the configuration's limits
        from lpvmpc.observer import OBS_PARAMS
        row = [OBS_PARAMS[k] for k in ("lf", "lr", "m", "I", "Cf", "Cr", "mu")]
        path.set_observer_vehicles(np.tile(row, (plant0.shape[0], 1)),
                                   design=dict(lim_ls=np.array(estimator.lim_ls[:]).reshape(6, 2), lim_hs=np.array(estimator.lim_hs[:]).reshape(6, 2)))
    if tunings is not None:                                           # "own": each handle's own row; "sampled": sample_tunings around it
        from lpvmpc import tuning
        for e in (path, tt, plan):
            B = plant0.shape[0]
            e.set_tunings(tuning.tuning_rows(B, e) if tunings == "own" else tuning.sample_tunings(B, 1, engine=e))
    if model_params is not None:
        for e in (path, tt, plan):
            e.set_model_params(model_params)
    path.race_init(tt, plan, plant0, half_track0=half, laps=5, half_width=mp.halfWidth, slack=mp.slack, estimator=estimator,
                   actuator=actuator, plant_params=plant_params, **({} if tyre_params is None else {"tyre_params": tyre_params}))
    if disturbance is not None:                                       # rows attached before the first tick
        path.set_disturbances(disturbance, seed=1)
    if sensor_faults is not None:                                     # rows attached before the first tick
        path.set_sensor_faults(sensor_faults, seed=1)
    path.race_tick(warm)
    if record:
        path.race_record(K, 1)
    if heats:                                                         # heats of `heats` consecutive vehicles
        path.race_heats(np.arange(plant0.shape[0]) // int(heats))
    if interactions is not None:                                      # a dict of configuration words, on the heats just attached
        path.race_interactions(interactions)
    if contact is not None:                                           # a dict of configuration words, on the interactions just attached
        path.race_contact(contact)
    if walls is not None:                                             # a dict of configuration words
        path.race_walls(walls)
    a0 = path.race_laps()[1].sum()
    ms = timed(path.race_tick, path.race_read, K)
    alive = path.race_laps()[1].sum() - a0
    ph = np.bincount(path.race_read()["phase"], minlength=4)
    for e in (path, tt, plan):
        e.close()
    return ms, alive / (ms * K * 1e-3), ph


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=30)
    ap.add_argument("--sizes", default="1024,8192")
    ap.add_argument("--out", default=None)
    ap.add_argument("--estimator", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--actuator", action="store_true")
    ap.add_argument("--record", action="store_true")
    ap.add_argument("--heats", type=int, default=0, metavar="SIZE")
    ap.add_argument("--plant-params", action="store_true")
    ap.add_argument("--models", action="store_true")
    ap.add_argument("--tunings", action="store_true")
    ap.add_argument("--tyres", action="store_true")
    ap.add_argument("--observer-vehicles", action="store_true")
    ap.add_argument("--tracks", action="store_true")
    ap.add_argument("--disturbance", action="store_true")
    ap.add_argument("--sensor-faults", action="store_true")
    ap.add_argument("--interactions", action="store_true")
    ap.add_argument("--walls", action="store_true")
    ap.add_argument("--contact", action="store_true")
    ap.add_argument("--fork", action="store_true")
    ap.add_argument("--fork-child", default=None, help=argparse.SUPPRESS)                  # B: the fork measurements of one fleet size
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--models-child", nargs=4, default=None, help=argparse.SUPPRESS)      # lib regime B bind: one run of --models
    a = ap.parse_args()
    if a.models_child:
        return models_child(a)
    if a.fork_child:
        return fork_child(a)
    if a.fork:
        return fork_main(a)
    if a.models:
        return models_main(a)
    if a.tunings:
        return models_main(a, [("unbound", "liblpvmpc.so", 0), ("own rows bound", "liblpvmpc.so", 2), ("sampled rows bound", "liblpvmpc.so", 3)])
    if a.tyres:
        return models_main(a, [("vehicles, nominal rows", "liblpvmpc.so", 4), ("tyres, kind 0 rows", "liblpvmpc.so", 5),
                               ("tyres, Pacejka", "liblpvmpc.so", 6)], parent=("parent, vehicles", 4))
    if a.observer_vehicles:
        return models_main(a, [("estimator, unbound", "liblpvmpc.so", 7), ("estimator, rows bound", "liblpvmpc.so", 8)],
                           parent=("parent, estimator", 7))
    if a.tracks:
        return models_main(a, [("tyres, unbound", "liblpvmpc.so", 9), ("own track bound", "liblpvmpc.so", 10), ("six tracks bound", "liblpvmpc.so", 11),
                               ("six sub-fleets", "liblpvmpc.so", 12)], parent=("parent, tyres", 9))
    if a.disturbance:
        return models_main(a, [("tyres, nothing attached", "liblpvmpc.so", 9), ("disturbances attached", "liblpvmpc.so", 13)],
                           parent=("parent, tyres", 9))
    if a.sensor_faults:
        return models_main(a, [("estimator, nothing attached", "liblpvmpc.so", 14), ("off rows attached", "liblpvmpc.so", 16),
                               ("sensor faults attached", "liblpvmpc.so", 15)],
                           parent=("parent, estimator", 14))
    if a.interactions:
        a.heats = a.heats or 16
        return models_main(a, [("tyres + heats of %d" % a.heats, "liblpvmpc.so", 17), ("all-off interactions", "liblpvmpc.so", 18),
                               ("interactions attached", "liblpvmpc.so", 19)], parent=("parent, tyres + heats", 17))
    if a.contact:
        a.heats = a.heats or 16
        return models_main(a, [("interactions attached", "liblpvmpc.so", 19), ("contact, no friction/yaw", "liblpvmpc.so", 24),
                               ("contact attached", "liblpvmpc.so", 25)], parent=("parent, interactions", 19))
    if a.walls:
        return models_main(a, [("tyres, nothing attached", "liblpvmpc.so", 20), ("far-margin walls", "liblpvmpc.so", 21),
                               ("walls attached", "liblpvmpc.so", 22)], parent=("parent, tyres", 20))
    if a.plant_params:
        return plant_params_main(a)
    if a.record:
        return record_main(a)
    if a.heats:
        return heats_main(a)
    if a.estimator:
        return estimator_main(a)
    if a.actuator:
        return actuator_main(a)
    import lpvmpc
    from lpvmpc import workloads as W
    from tests._golden import load
    from oracle import plant_ref as PR
    mp = lpvmpc.Map("L_shape", 0.2)
    c = load("cascade")
    lines = []
    for B in [int(x) for x in a.sizes.split(",")]:
        rng = np.random.default_rng(3)
        K = a.ticks
        # lap 0: small offsets around the origin
        grid = np.zeros((B, 8)); grid[:, 1] = rng.normal(0, 0.02, B); grid[:, 2] = rng.uniform(0.9, 1.1, B)
        ms_r, vps_r, ph = race_run(mp, grid, 0, 10, K)
        Qp, Rp, dRp = W.CTRL_TUNINGS["path"]
        cl = lpvmpc.BatchedSolver("controller", 20, 1 / 30.0, Qp, Rp, dRp, track=mp.PointAndTangent)
        cl.cl_init(grid, mp.halfWidth, mp.slack, q9_swap=True, n_sub=7)
        cl.cl_tick(10)
        ms_c = timed(cl.cl_tick, cl.cl_read, K)
        cl.close()
        lines.append("lap0     B=%5d  race %.3f ms/tick (%.3g alive vehicle-ticks/s, phases %s)  cl_tick %.3f ms/tick  ratio %.3f"
                     % (B, ms_r, vps_r, ph.tolist(), ms_c, ms_r / ms_c))
        # in phase: every vehicle at the fixture's lap-0 start, event on tick pre_ticks - 1; time racing ticks
        P = int(c["pre_ticks"])
        same = np.tile(c["pre_plant"][0], (B, 1))
        ms_r, vps_r, ph = race_run(mp, same, 1, P + 3, K)
        path, tt, plan = engines(mp)
        tt.set_option("cascade_prefetch", 0)
        tt.cascade_init(plan, np.tile(c["plant0"], (B, 1)), np.tile(c["cmd0"], (B, 1)), np.tile(c["uPred0"], (B, 1, 1)), lap0=1,
                        half_width=mp.halfWidth, slack=mp.slack, plan_max_ey=0.2, q9_swap=True)
        tt.cascade_tick(3)
        ms_c = timed(tt.cascade_tick, lambda: tt.cascade_read(full=False), K)
        for e in (path, tt, plan):
            e.close()
        lines.append("inphase  B=%5d  race %.3f ms/tick (%.3g alive vehicle-ticks/s, phases %s)  cascade %.3f ms/tick  ratio %.3f"
                     % (B, ms_r, vps_r, ph.tolist(), ms_c, ms_r / ms_c))
        # staggered: vehicles spread over the last quarter of the lap
        L = mp.TrackLength
        st = np.zeros((B, 8))
        for b in range(B):
            s = rng.uniform(0.8, 0.97) * L
            x, y, th = PR.get_global_position(mp.PointAndTangent, s, rng.normal(0, 0.02))
            st[b] = [x, y, rng.uniform(0.9, 1.1), 0, 0, 0, th, 0]
        ms_r, vps_r, ph = race_run(mp, st, 1, 40, K)
        lines.append("stagger  B=%5d  race %.3f ms/tick (%.3g alive vehicle-ticks/s, phases %s)" % (B, ms_r, vps_r, ph.tolist()))
        for l in lines[-3:]:
            print(l, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def estimator_main(a):
    import lpvmpc
    from lpvmpc.observer import observer_config
    from tests._golden import load
    f = np.load(os.path.join(ROOT, "tests", "golden", "estimator", "estimator.npz"))
    obs = observer_config(f["L_ls"], f["lim_ls"], f["L_hs"], f["lim_hs"], psi_std=0.01, psiDot_std=0.05, x_std=0.01, y_std=0.01,
                          v_std=0.02, seed=7)
    mp = lpvmpc.Map("L_shape", 0.2)
    c = load("cascade")
    P = int(c["pre_ticks"])
    lines = []
    for B in [int(x) for x in a.sizes.split(",")]:
        rng = np.random.default_rng(3)
        grid = np.zeros((B, 8)); grid[:, 1] = rng.normal(0, 0.02, B); grid[:, 2] = rng.uniform(0.9, 1.1, B)
        same = np.tile(c["pre_plant"][0], (B, 1))
        for name, plant0, half, warm in (("lap0", grid, 0, 10), ("inphase", same, 1, P + 3)):
            ms = {False: [], True: []}
            ph = {}
            for _ in range(a.reps):
                for est in (False, True):
                    m, _vps, ph[est] = race_run(mp, plant0, half, warm, a.ticks, obs if est else None)
                    ms[est].append(m)
            m0, m1 = float(np.median(ms[False])), float(np.median(ms[True]))
            lines.append("%-8s B=%5d  race %.3f ms/tick (runs %s, phases %s)  with estimator %.3f ms/tick (runs %s, phases %s)  "
                         "added %+.3f ms/tick" % (name, B, m0, " ".join("%.3f" % x for x in ms[False]), ph[False].tolist(), m1,
                                                  " ".join("%.3f" % x for x in ms[True]), ph[True].tolist(), m1 - m0))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


def actuator_main(a):
    import lpvmpc
    from tests._golden import load
    mp = lpvmpc.Map("L_shape", 0.2)
    c = load("cascade")
    P = int(c["pre_ticks"])
    cfgs = (("old", None, 0), ("all-off", lpvmpc.actuator_config(), 0),
            ("La=Ld=20+servo", _act20(), 0), ("La=Ld=20+servo,sd=3", _act20(), 3))
    lines = []
    for B in [int(x) for x in a.sizes.split(",")]:
        rng = np.random.default_rng(3)
        grid = np.zeros((B, 8)); grid[:, 1] = rng.normal(0, 0.02, B); grid[:, 2] = rng.uniform(0.9, 1.1, B)
        same = np.tile(c["pre_plant"][0], (B, 1))
        for name, plant0, half, warm in (("lap0", grid, 0, 10), ("inphase", same, 1, P + 3)):
            ms = {k: [] for k, _, _ in cfgs}
            ph = {}
            for _ in range(a.reps):
                for k, act, sd in cfgs:
                    m, _vps, ph[k] = race_run(mp, plant0, half, warm, a.ticks, actuator=act, sd=sd)
                    ms[k].append(m)
            m0 = float(np.median(ms["old"]))
            for k, _, _ in cfgs:
                m = float(np.median(ms[k]))
                lines.append("%-8s B=%5d  %-20s %.3f ms/tick (runs %s, phases %s)  vs old %+.3f ms/tick"
                             % (name, B, k, m, " ".join("%.3f" % x for x in ms[k]), ph[k].tolist(), m - m0))
                print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def plant_params_main(a):
    import lpvmpc
    from tests._golden import load
    mp = lpvmpc.Map("L_shape", 0.2)
    c = load("cascade")
    P = int(c["pre_ticks"])
    lines = []
    for B in [int(x) for x in a.sizes.split(",")]:
        rng = np.random.default_rng(3)
        grid = np.zeros((B, 8)); grid[:, 1] = rng.normal(0, 0.02, B); grid[:, 2] = rng.uniform(0.9, 1.1, B)
        same = np.tile(c["pre_plant"][0], (B, 1))
        cfgs = (("all-off", dict(actuator=lpvmpc.actuator_config())), ("nominal rows", dict(plant_params=lpvmpc.plant_params(B))),
                ("sampled rows", dict(plant_params=lpvmpc.sample_plant_params(B, 1))))
        for name, plant0, half, warm in (("lap0", grid, 0, 10), ("inphase", same, 1, P + 3)):
            ms = {k: [] for k, _ in cfgs}
            ph = {}
            for _ in range(a.reps):
                for k, kw in cfgs:
                    m, _vps, ph[k] = race_run(mp, plant0, half, warm, a.ticks, **kw)
                    ms[k].append(m)
            m0 = float(np.median(ms["all-off"]))
            for k, _ in cfgs:
                m = float(np.median(ms[k]))
                lines.append("%-8s B=%5d  %-13s %.3f ms/tick (runs %s, phases %s)  vs all-off %+.3f ms/tick"
                             % (name, B, k, m, " ".join("%.3f" % x for x in ms[k]), ph[k].tolist(), m - m0))
                print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def _models_starts(B):
    from tests._golden import load
    c = load("cascade")
    rng = np.random.default_rng(3)
    grid = np.zeros((B, 8)); grid[:, 1] = rng.normal(0, 0.02, B); grid[:, 2] = rng.uniform(0.9, 1.1, B)
    return {"lap0": (grid, 0, 10), "inphase": (np.tile(c["pre_plant"][0], (B, 1)), 1, int(c["pre_ticks"]) + 3)}


def _tracks_starts(B, regime, maps, of, plant0):
    """The starts of _models_starts on each vehicle's own track: lap 0 from the grid (every table starts at the origin, heading 0);
    in phase: as far before the end of its own lap, and as far off the centre line and the tangent, as the fixture's start is on the
    L shape."""
    if regime == "lap0":
        return plant0
    from oracle import plant_ref as PR
    import lpvmpc
    ls = lpvmpc.Map("L_shape", 0.2)
    s, ey, epsi, _ = PR.get_local_position(ls.PointAndTangent, ls.halfWidth, ls.slack, plant0[0, 0], plant0[0, 1], plant0[0, 6])
    out = plant0.copy()
    for t, m in enumerate(maps):
        x, y, th = PR.get_global_position(m.PointAndTangent, m.TrackLength - (ls.TrackLength - s), ey)
        out[of == t, 0], out[of == t, 1], out[of == t, 6] = x, y, th + epsi
    return out


def tracks_child(a, regime, B, bind):
    """bind 10: the own track bound; 11: the six-entry palette; 12: the palette's tracks as six homogeneous sub-fleets ticked in turn."""
    import lpvmpc
    from lpvmpc import track as TK
    mp = lpvmpc.Map("L_shape", 0.2)
    plant0, half, warm = _models_starts(B)[regime]
    tyres = lpvmpc.tyre_params(B, kind=0)
    if bind == 10:
        return race_run(mp, plant0, half, warm, a.ticks, tyre_params=tyres, tracks=([mp], np.zeros(B, np.int32)))
    maps, of = TK.palette(), TK.cycle(B)
    plant0 = _tracks_starts(B, regime, maps, of, plant0)
    if bind == 11:
        return race_run(mp, plant0, half, warm, a.ticks, tyre_params=tyres, tracks=(maps, of))
    fleets = []
    for t, m in enumerate(maps):
        path, tt, plan = engines(m)
        path.race_init(tt, plan, plant0[of == t], half_track0=half, laps=5, half_width=m.halfWidth, slack=m.slack,
                       tyre_params=tyres[of == t])
        fleets.append((path, tt, plan))
    for _ in range(warm):
        for f in fleets:
            f[0].race_tick(1)
    a0 = sum(f[0].race_laps()[1].sum() for f in fleets)
    t0 = time.perf_counter()
    for _ in range(a.ticks):
        for f in fleets:
            f[0].race_tick(1)
    for f in fleets:
        f[0].race_read()
    ms = (time.perf_counter() - t0) * 1e3 / a.ticks
    alive = sum(f[0].race_laps()[1].sum() for f in fleets) - a0
    ph = sum(np.bincount(f[0].race_read()["phase"], minlength=4) for f in fleets)
    for f in fleets:
        for e in f:
            e.close()
    return ms, alive / (ms * a.ticks * 1e-3), ph


def mp_length():
    import lpvmpc
    return float(lpvmpc.Map("L_shape", 0.2).TrackLength)


def models_child(a):
    lib, regime, B, bind = a.models_child
    from lpvmpc import _ffi
    _ffi.LIB_PATH = os.path.join(os.path.dirname(_ffi.LIB_PATH), lib)
    import lpvmpc
    if int(bind) in (10, 11, 12):
        ms, vps, ph = tracks_child(a, regime, int(B), int(bind))
        print("MODELS_RUN %.6f %s %.4g" % (ms, ",".join(str(int(x)) for x in ph), vps), flush=True)
        return
    mp = lpvmpc.Map("L_shape", 0.2)
    plant0, half, warm = _models_starts(int(B))[regime]
    rows = lpvmpc.model_params(int(B)) if int(bind) == 1 else None                # bind: 0 nothing, 1 nominal model rows, 2 / 3 tuning rows,
    tyres = {5: lpvmpc.tyre_params(int(B), kind=0), 6: "pacejka", 9: lpvmpc.tyre_params(int(B), kind=0),
             13: lpvmpc.tyre_params(int(B), kind=0), 14: lpvmpc.tyre_params(int(B), kind=0),
             15: lpvmpc.tyre_params(int(B), kind=0), 16: lpvmpc.tyre_params(int(B), kind=0), 17: lpvmpc.tyre_params(int(B), kind=0),
             18: lpvmpc.tyre_params(int(B), kind=0), 19: lpvmpc.tyre_params(int(B), kind=0), 20: lpvmpc.tyre_params(int(B), kind=0),
             21: lpvmpc.tyre_params(int(B), kind=0), 22: lpvmpc.tyre_params(int(B), kind=0), 23: lpvmpc.tyre_params(int(B), kind=0),
             24: lpvmpc.tyre_params(int(B), kind=0), 25: lpvmpc.tyre_params(int(B), kind=0)}.get(int(bind))               # 4 nominal plant rows (_vehicles), 5 / 6 tyre rows on top
    dist = None                                                                    # 13: 9 with gusts, a patch and a kick on every vehicle
    if int(bind) == 13:
        from lpvmpc.disturbance import parse_disturbance
        dist = parse_disturbance("gusts:0.3+patch:0,3,0.7+kick:400,0.1,0.3", int(B), mp_length())
    obs = None                                                                     # 7 / 8: _vehicles with the estimator, unbound / rows bound
    faults = None                                                                  # 14 / 16 / 15: _tyres with the estimator; nothing, all-off rows
    if int(bind) == 16:                                                            # (the faulted kernel on the healthy race's trajectories), every fault
        from lpvmpc.sensor_faults import fault_rows
        faults = fault_rows(int(B), 0.005)
    if int(bind) == 15:
        from lpvmpc.sensor_faults import fault_rows
        faults = fault_rows(int(B), 0.005, gps_outage=(1.0, 1.0), gps_loss_p=0.2, gps_jump=(3.0, 0.5, 0.05, -0.05), imu_w_bias=0.02,
                            imu_yaw_drift=0.001, enc_scale=0.98, enc_outage=(4.0, 0.1))
    if int(bind) in (7, 8, 14, 15, 16):
        from lpvmpc.observer import observer_config
        f = np.load(os.path.join(ROOT, "tests", "golden", "estimator", "estimator.npz"))
        obs = observer_config(f["L_ls"], f["lim_ls"], f["L_hs"], f["lim_hs"], psi_std=0.01, psiDot_std=0.05, x_std=0.01, y_std=0.01,
                              v_std=0.02, seed=7)
    ms, vps, ph = race_run(mp, plant0, half, warm, a.ticks, model_params=rows, tunings={2: "own", 3: "sampled"}.get(int(bind)),
                            plant_params="nominal" if int(bind) in (4, 5, 6, 7, 8) else None, tyre_params=tyres, estimator=obs,
                            observer_vehicles=int(bind) == 8, disturbance=dist, sensor_faults=faults,
                            heats=(a.heats or 16) if int(bind) in (17, 18, 19, 23, 24, 25) else 0,       # 17: 9 with heats; 18 / 19: the interactions on top, all off / defaults
                            interactions={18: dict(draft_gain=0.0, contact=0), 19: {}, 23: {}, 24: {}, 25: {}}.get(int(bind)),
                            contact={24: dict(friction=0.0, yaw_response=0), 25: {}}.get(int(bind)),   # 24 / 25: 19 with the contact model, centres-form words / defaults
                            walls={21: dict(margin=50.0), 22: {}, 23: {}}.get(int(bind)))   # 20: 9 again; 21 / 22: walls on top, out of reach / defaults; 23: 19 with walls
    print("MODELS_RUN %.6f %s %.4g" % (ms, ",".join(str(int(x)) for x in ph), vps), flush=True)


def fork_child(a):
    """One fleet size: the in-phase race of bind 9 at its first timed tick; medians of --reps calls each."""
    import lpvmpc
    B = int(a.fork_child)
    mp = lpvmpc.Map("L_shape", 0.2)
    plant0, half, warm = _models_starts(B)["inphase"]
    path, tt, plan = engines(mp)
    path.race_init(tt, plan, plant0, half_track0=half, laps=5, half_width=mp.halfWidth, slack=mp.slack,
                   tyre_params=lpvmpc.tyre_params(B, kind=0))
    path.race_tick(warm)
    ph = np.bincount(path.race_read()["phase"], minlength=4)
    rng = np.random.default_rng(1)
    rot = ((np.arange(B) + 1) % B).astype(np.int32)
    tenth = np.arange(B, dtype=np.int32)
    slots = rng.choice(B, max(B // 10, 1), replace=False)
    tenth[slots] = rng.integers(0, B, slots.size)
    blob = path.race_snapshot(raw=True)

    def med(call):
        call()                                                            # (the first call pays for code loading)
        t = []
        for _ in range(max(a.reps, 3)):
            t0 = time.perf_counter(); call(); t.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(t))
    ms = [med(lambda: path.race_snapshot(raw=True)), med(lambda: path.race_restore(blob)), med(lambda: path.race_clone(rot)),
          med(lambda: path.race_clone(tenth))]
    path.race_restore(blob)
    state = len(blob) - 64 - 40 * lpvmpc.RaceSnapshot.from_bytes(blob).header["count"]
    path.race_tick(2); path.race_read()                                   # the race goes on
    for e in (path, tt, plan):
        e.close()
    print("FORK_RUN %d %s %d %d %s %d" % (B, ",".join(str(int(x)) for x in ph), len(blob), state, " ".join("%.4f" % m for m in ms),
                                          int(np.sum(tenth != np.arange(B)))), flush=True)


def fork_main(a):
    import subprocess
    lines = models_main(a, [("tyres, unforked", "liblpvmpc.so", 9)], parent=("parent, tyres", 9), write=False)
    scale_of = "parent, tyres" if a.parent_lib else "tyres, unforked"
    for B in [int(x) for x in a.sizes.split(",")]:
        tick = [float(l.split("ms/tick")[0].split()[-1]) for l in lines if l.startswith("inphase  B=%5d  %-22s" % (B, scale_of))][0]
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--fork-child", str(B)], check=True,
                             capture_output=True, text=True, timeout=600).stdout
        f = [l for l in out.splitlines() if l.startswith("FORK_RUN")][-1].split()
        size, state = int(f[3]), int(f[4])
        snap, rest, full, part = (float(x) for x in f[5:9])
        lines.append("fork     B=%5d  phases [%s]  blob %d B = %.0f B/vehicle  snapshot %.3f ms  restore %.3f ms  clone, all moved %.3f ms "
                     "(%.1f GB/s over 4 x %.2f MB read + written)  clone, %d moved %.3f ms  scale: %s %.3f ms per race tick"
                     % (B, f[2], size, size / B, snap, rest, full, 4 * state / (full * 1e-3) / 1e9, state / 1e6, int(f[9]), part, scale_of, tick))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


def models_main(a, cfgs=None, parent=("parent, unbound", 0), write=True):
    import subprocess
    cfgs = list(cfgs or [("unbound", "liblpvmpc.so", 0), ("nominal rows bound", "liblpvmpc.so", 1)])
    base = cfgs[0][0]                                                                 # the differences are against the first configuration
    if a.parent_lib:
        cfgs.append((parent[0], a.parent_lib, parent[1]))
    lines = []
    for B in [int(x) for x in a.sizes.split(",")]:
        for regime in ("lap0", "inphase"):
            ms = {k: [] for k, _, _ in cfgs}
            ph, vps = {}, {}
            for _ in range(a.reps):
                for k, lib, bind in cfgs:
                    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--ticks", str(a.ticks), "--models-child", lib, regime, str(B),
                                          str(bind)] + (["--heats", str(a.heats)] if a.heats else []), check=True, capture_output=True, text=True, timeout=600).stdout
                    f = [l for l in out.splitlines() if l.startswith("MODELS_RUN")][-1].split()
                    ms[k].append(float(f[1])); ph[k] = f[2]; vps.setdefault(k, []).append(float(f[3]))
            m0 = float(np.median(ms[base]))
            for k, _, _ in cfgs:
                m = float(np.median(ms[k]))
                lines.append("%-8s B=%5d  %-22s %.3f ms/tick (runs %s, spread %.3f, phases [%s], %.4g alive vehicle-ticks/s)  vs %s %+.3f ms/tick"
                             % (regime, B, k, m, " ".join("%.3f" % x for x in ms[k]), max(ms[k]) - min(ms[k]), ph[k], float(np.median(vps[k])),
                                base.split(",")[0], m - m0))
                print(lines[-1], flush=True)
    if a.out and write:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return lines


def record_main(a):
    import lpvmpc
    from tests._golden import load
    mp = lpvmpc.Map("L_shape", 0.2)
    c = load("cascade")
    P = int(c["pre_ticks"])
    lines = []
    for B in [int(x) for x in a.sizes.split(",")]:
        rng = np.random.default_rng(3)
        grid = np.zeros((B, 8)); grid[:, 1] = rng.normal(0, 0.02, B); grid[:, 2] = rng.uniform(0.9, 1.1, B)
        same = np.tile(c["pre_plant"][0], (B, 1))
        for name, plant0, half, warm in (("lap0", grid, 0, 10), ("inphase", same, 1, P + 3)):
            ms = {False: [], True: []}
            ph = {}
            for _ in range(a.reps):
                for rec in (False, True):
                    m, _vps, ph[rec] = race_run(mp, plant0, half, warm, a.ticks, record=rec)
                    ms[rec].append(m)
            m0, m1 = float(np.median(ms[False])), float(np.median(ms[True]))
            lines.append("%-8s B=%5d  race %.3f ms/tick (runs %s, phases %s)  recording %.3f ms/tick (runs %s, phases %s)  "
                         "added %+.3f ms/tick" % (name, B, m0, " ".join("%.3f" % x for x in ms[False]), ph[False].tolist(), m1,
                                                  " ".join("%.3f" % x for x in ms[True]), ph[True].tolist(), m1 - m0))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


def heats_main(a):
    import subprocess
    import lpvmpc
    mp = lpvmpc.Map("L_shape", 0.2)
    lines = []
    for B in [int(x) for x in a.sizes.split(",")]:
        for name, (plant0, half, warm) in _models_starts(B).items():
            ms = {"detached": [], "attached": [], "parent": []}
            ph = {}
            for _ in range(a.reps):
                for k in ("detached", "attached"):
                    m, _vps, ph[k] = race_run(mp, plant0, half, warm, a.ticks, heats=a.heats if k == "attached" else 0)
                    ms[k].append(m)
                if a.parent_lib:
                    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--ticks", str(a.ticks), "--models-child", a.parent_lib, name,
                                          str(B), "0"], check=True, capture_output=True, text=True, timeout=600).stdout
                    ms["parent"].append(float([l for l in out.splitlines() if l.startswith("MODELS_RUN")][-1].split()[1]))
            m0, m1 = float(np.median(ms["detached"])), float(np.median(ms["attached"]))
            line = ("%-8s B=%5d  heats of %d  detached %.3f ms/tick (runs %s, spread %.3f, phases %s)  attached %.3f ms/tick (runs %s, spread %.3f)  "
                    "added %+.3f ms/tick" % (name, B, a.heats, m0, " ".join("%.3f" % x for x in ms["detached"]), max(ms["detached"]) - min(ms["detached"]),
                                             ph["detached"].tolist(), m1, " ".join("%.3f" % x for x in ms["attached"]),
                                             max(ms["attached"]) - min(ms["attached"]), m1 - m0))
            if a.parent_lib:
                mp_ = float(np.median(ms["parent"]))
                line += "  parent, detached %.3f ms/tick (runs %s)  vs detached %+.3f ms/tick" % (mp_, " ".join("%.3f" % x for x in ms["parent"]), mp_ - m0)
            lines.append(line)
            print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


def _act20():
    import lpvmpc
    cfg = lpvmpc.actuator_config(low_level_dyn=True)
    cfg.delay_a = cfg.delay_df = 20
    return cfg



if __name__ == "__main__":
    main()
