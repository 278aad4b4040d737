#!/usr/bin/env python3
"""Model-mismatch sweep: one race of B vehicles (default 8192) whose plants carry their own parameters (lpvmpc_race_init_vehicles,
rows from plant.sample_plant_params) while the controllers and the planner keep the nominal model.  Default spreads: m, Iz +-15 %,
Cf, Cr +-30 %, mu x [0.5, 1.5]; two racing laps, the recorder on (its per-lap statistics).  The vehicles start near the end of the
lap (HalfTrack = 1), so lap 0 is short.  The race runs until every vehicle has finished or is lost (or --max-ticks).
Reports, binned by each sampled parameter (quartiles of its factor against the nominal row): vehicles, the fractions finished and
lost, the median and p90 racing lap time (laps 1 .. laps of the finished vehicles' laps) and the median per-lap RMSE_ey of the
racing laps (RaceFleet.lap_stats, CMAIN:101-106).
--tracks oval,L_shape,... puts vehicle b on track b mod their number (lpvmpc_set_tracks, RaceFleet(track_map=<sequence>, track_of=...)):
one race, one launch sequence, every vehicle with its own lap length, half width and slack; the report is the same.
--model selects the controllers' and the planner's model of each vehicle (lpvmpc_set_model_params, RaceFleet(model_params=...)):
nominal (default: today's run, same output), plant (each vehicle's model is its plant row: the matched experiment) or noisy:REL
(the plant row times an independent uniform factor in [1 - REL, 1 + REL] per field: an identification error).  The nominal-car
baseline race keeps the nominal model.
--tyre selects the plants' tyre (lpvmpc_race_init_tyres, RaceFleet(tyre_params=...)): linear (default: today's run, same output:
the plant rows' Cf, Cr) or pacejka (the launch file's Simulator.pacejka on every vehicle, the baseline race included: a tyre that
saturates; the rows' Cf, Cr are then not read, so their bins show no trend of their own).  Every model keeps the linear tyre.
--estimator puts the state estimator in the loop (the fixture's limit tables and nominal gain tables, the sensors without noise),
in the baseline race as well: nominal (the estimator keeps its own constants and the nominal tables) or plant (each vehicle's
estimator takes its plant row, with gain tables designed on the device for that row: RaceFleet(estimator_params="plant")).  Without
the flag the race runs on ground truth: today's run, same output.
--disturbance pushes back on the swept race (lpvmpc_set_disturbances, RaceFleet(disturbance=...)), the same rows for every vehicle:
gusts:SIGMA (a Gauss-Markov gust of that standard deviation on ax, ay and the yaw acceleration, per-tick correlation 0.8, seeded with
--seed), patch:S0,LEN,GAMMA (grip times GAMMA from S0 m on, LEN m long, on every vehicle's own track) or kick:STEP,VY,W (a side push
at plant step STEP); several joined with +.  The nominal-car baseline race stays undisturbed.  Without the flag the race is today's
run, same output.
--respawn K refills the swept race every K ticks (RaceFleet.respawn, lpvmpc_race_clone): every lost slot takes the state of a vehicle
that is still driving (of the slot's own track), drawn with --seed + the tick, keeps its own plant row and, where gusts are attached,
draws its own future -- the resampling step of importance splitting; the weights are the caller's and this report keeps none, so
its bins then describe the slots' rows, not independent vehicles.  The recorder cannot follow a clone, so the run records nothing and
RMSE_ey is not reported.  The report gains one line: slots respawned, alive vehicle-ticks and alive vehicle-ticks per second of the
swept race.  --respawn 0 adds the same line to an unchanged run (recorder on, nothing respawned), for the comparison.  The baseline
race is never refilled.  Without the flag the output is today's.
--sensor-faults breaks the swept race's sensors (lpvmpc_set_sensor_faults, RaceFleet(sensor_faults=...)), the same rows for every
vehicle: gps_outage:LEN_S and enc_outage:LEN_S (a GPS without publications / a stuck encoder for LEN_S seconds, from one second
into the race), gps_loss:P (each publication lost with probability P, seeded with --seed), imu_bias:W (a rate-gyro bias, rad/s),
imu_drift:W, enc_scale:S; several joined with +.  It needs --estimator (the sensors feed the estimator); the baseline race keeps
healthy sensors.  The answer it is for: does estimator + controller survive one second without GPS?  Without the flag the output is
today's.
--interactions SIZE[:WORD=VALUE,...] lets the vehicles of the swept race act on each other (lpvmpc_race_heats + lpvmpc_race_interactions,
RaceFleet(heats=..., interactions=...)): heats of SIZE consecutive vehicles (on one track each; with --tracks, consecutive vehicles of
one track) whose members take drag off each other in the wake and exchange impulses where their footprints overlap; WORD=VALUE sets
configuration words (draft_gain, wake_length, wake_half_width, contact, restitution, push).  The baseline race keeps to itself.  The
report gains one line: vehicles hit, total hit ticks, drafting ticks.  Without the flag the output is today's.
--walls [WORD=VALUE,...] puts walls at the edges of the swept race's tracks (lpvmpc_race_walls, RaceFleet(walls=...)): a corner of a
footprint beyond half_width + margin gets an impulse there and the car is pushed back; WORD=VALUE sets configuration words (margin, reach,
half_length, half_width_car, restitution, friction, push, yaw_response).  The baseline race has none.  The report gains one line:
vehicles that hit a wall, total hit ticks, the largest impulse, vehicles outside at the end.  Without the flag the output is today's.
Usage: tools/robustness_sweep.py [--B 8192] [--laps 2] [--seed 1] [--max-ticks 3000] [--model nominal|plant|noisy:REL]
       [--tyre linear|pacejka] [--estimator nominal|plant] [--disturbance SPEC] [--sensor-faults SPEC] [--interactions SPEC] [--walls [SPEC]] [--respawn K] [--out FILE]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8192)
    ap.add_argument("--laps", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--max-ticks", type=int, default=3000)
    ap.add_argument("--model", default="nominal")
    ap.add_argument("--tyre", default="linear", choices=("linear", "pacejka"))
    ap.add_argument("--estimator", default=None, choices=("nominal", "plant"))
    ap.add_argument("--tracks", default=None, help="comma-separated track shapes (oval, L_shape, 3110, Euge_Track): vehicle b races on track b mod their number")
    ap.add_argument("--disturbance", default=None, help="gusts:SIGMA | patch:S0,LEN,GAMMA | kick:STEP,VY,W (joined with +)")
    ap.add_argument("--sensor-faults", default=None, help="gps_outage:LEN_S | enc_outage:LEN_S | gps_loss:P | imu_bias:W | imu_drift:W | enc_scale:S (joined with +)")
    ap.add_argument("--interactions", default=None, metavar="SIZE[:WORD=VALUE,...]",
                    help="heats of SIZE consecutive vehicles whose members draft and hit each other, e.g. 16 or 16:draft_gain=0.5,contact=0")
    ap.add_argument("--walls", default=None, nargs="?", const="", metavar="WORD=VALUE,...",
                    help="walls at the track's edges with the default configuration, or e.g. margin=0.2,restitution=0.5")
    ap.add_argument("--respawn", type=int, default=None, help="refill the lost slots every K ticks (0: never, but report the alive vehicle-ticks)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.interactions and a.respawn:
        ap.error("--respawn clones vehicles, which a race refuses while heats are attached: not with --interactions")
    if a.respawn is not None and a.respawn < 0:
        ap.error("--respawn must be >= 0")
    if a.sensor_faults and not a.estimator:
        ap.error("--sensor-faults needs --estimator: the sensors feed the estimator")
    if a.model not in ("nominal", "plant") and not a.model.startswith("noisy:"):
        ap.error("--model must be nominal, plant or noisy:REL")
    import lpvmpc
    from lpvmpc import model, plant
    from tests._race_observer_ref import start_line_fleet
    mp = lpvmpc.Map("L_shape", 0.2)
    B = a.B
    spread = plant.DEFAULT_SPREAD
    rows = lpvmpc.sample_plant_params(B, a.seed, spread)
    nom = lpvmpc.plant_params(B)
    plant0 = start_line_fleet(mp.PointAndTangent, B, a.seed, 0.8, 0.97)
    maps = track_of = None
    if a.tracks:                                # the track axis: the same starts (same seed), each on the last quarter of the vehicle's own lap
        maps = [lpvmpc.Map(t, 0.2) for t in a.tracks.split(",")]
        track_of = (np.arange(B) % len(maps)).astype(np.int32)
        for t, m in enumerate(maps):
            plant0[track_of == t] = start_line_fleet(m.PointAndTangent, B, a.seed, 0.8, 0.97)[track_of == t]

    if a.model == "nominal":
        model_rows, model_text = None, "keep the nominal model (lf = lr = 0.125, m = 1.98, Iz = 0.03, Cf = Cr = 60, mu = 0.05)"
    elif a.model == "plant":
        model_rows, model_text = rows, "take each vehicle's plant row as its model (--model plant: no mismatch)"
    else:
        rel = float(a.model.split(":", 1)[1])
        model_rows = model.perturb_rows(rows, a.seed, {k: rel for k in plant.WORDS})
        model_text = "take each vehicle's plant row times an independent uniform factor in [%g, %g] per field as its model (--model %s)" % (1 - rel, 1 + rel, a.model)

    obs = None
    if a.estimator:
        from lpvmpc.observer import observer_config
        g = np.load(os.path.join(ROOT, "tests", "golden", "estimator", "estimator.npz"))
        obs = observer_config(g["L_ls"], g["lim_ls"], g["L_hs"], g["lim_hs"])

    dist = None
    if a.disturbance:
        from lpvmpc.disturbance import parse_disturbance
        lap = [float(m.PointAndTangent[-1, 3] + m.PointAndTangent[-1, 4]) for m in (maps or [mp])]
        dist = dict(rows=parse_disturbance(a.disturbance, B, np.array(lap)[track_of] if maps else lap[0]), seed=a.seed)

    faults = None
    if a.sensor_faults:
        from lpvmpc.sensor_faults import parse_sensor_faults
        faults = dict(rows=parse_sensor_faults(a.sensor_faults, B), seed=a.seed)

    inter = None
    if a.interactions:
        size, _, words = a.interactions.partition(":")
        cfg = {k: (int(v) if k == "contact" else float(v)) for k, v in (w.split("=") for w in words.split(",") if w)}
        heat = np.zeros(B, np.int32)
        for t in (np.unique(track_of) if maps else [0]):               # consecutive vehicles of one track
            on = np.nonzero(track_of == t)[0] if maps else np.arange(B)
            heat[on] = (heat.max() + 1 if t else 0) + np.arange(on.shape[0]) // int(size)
        inter = dict(heats=dict(heat=heat), interactions=cfg or True)
    contacts = {}
    if a.walls is not None:
        wcfg = {k: (int(v) if k == "yaw_response" else float(v)) for k, v in (w.split("=") for w in a.walls.split(",") if w)}
        inter = dict(inter or {}, walls=wcfg or True)
    walled = {}

    fork = dict(slots=0, alive=0)                                     # of the swept race, with --respawn

    def race(r, m=None, est_rows=None, disturbance=None, respawn=None, sensor_faults=None, interact=None):
        f = lpvmpc.RaceFleet(mp if maps is None else maps, plant0, laps=a.laps, half_track0=1, plant_params=r, model_params=m, track_of=track_of,
                             tyre_params="pacejka" if a.tyre == "pacejka" else None, estimator=obs, estimator_params=est_rows,
                             disturbance=disturbance, sensor_faults=sensor_faults, **(interact or {}))
        assert np.array_equal(f.plant_params(), r)
        assert a.tyre == "linear" or np.array_equal(f.tyre_params(), lpvmpc.tyre_params(B))
        assert m is None or np.array_equal(f.model_params(), m)
        if not respawn:
            f.record(1, 1 << 20)                                      # statistics of every tick; one record kept
        step = respawn if respawn else 100
        t0, n = time.perf_counter(), 0
        while n < a.max_ticks:
            before = int(f.path.race_laps()[1].sum()) if respawn is not None else 0
            f.run(step); n += step
            if respawn is not None:                                   # (alive ticks are state: a clone carries its source's count)
                fork["alive"] += int(f.path.race_laps()[1].sum()) - before
            if np.all(f.state()["phase"] >= 2):
                break
            if respawn and n < a.max_ticks:                             # (nothing after the last tick: the report shows the slots as they ended)
                src = f.respawn(a.seed + n)
                fork["slots"] += int(np.sum(src != np.arange(B)))
        return f, n, time.perf_counter() - t0

    base, _n, _w = race(nom)                                          # the same starts with the nominal car: the baseline
    ph_nom = base.state()["phase"]
    base.close()
    fleet, ticks, wall = race(rows, model_rows, "plant" if a.estimator == "plant" else None, dist, a.respawn, faults, inter)
    if a.interactions:
        io = fleet.interactions()
        contacts.update(hit=int((io["hit_ticks"] > 0).sum()), hit_ticks=int(io["hit_ticks"].sum()), draft_ticks=int(io["draft_ticks"].sum()))
    if a.walls is not None:
        wo = fleet.walls()
        walled.update(hit=int((wo["hit_ticks"] > 0).sum()), hit_ticks=int(wo["hit_ticks"].sum()), most=float(wo["max_impulse"].max()),
                      outside=int(wo["outside"].sum()))
    ph = fleet.state()["phase"]
    lt = fleet.lap_times()[:, 1:a.laps + 1]                          # racing laps, seconds (NaN: not completed)
    rmse = fleet.lap_stats()["rmse_ey"][:, 1:a.laps + 1] if not a.respawn else np.full(lt.shape, np.nan)
    fin, lost = ph == 2, ph == 3
    fin_nom = ph_nom == 2
    lines = ["# tools/robustness_sweep.py --B %d --laps %d --seed %d%s on one MI355X: one race, rows from sample_plant_params(B, %d) with spreads %s"
             % (B, a.laps, a.seed, " --tyre pacejka" if a.tyre == "pacejka" else "", a.seed,
                ", ".join("%s %+.0f %%" % (k, 100 * v) for k, v in spread.items())),
             "# the controllers and the planner %s." % model_text] + ([] if not a.estimator else [
             "# the state estimator is in the loop (--estimator %s): %s." % (a.estimator, "each vehicle's estimator takes its plant row and gain tables "
              "designed for it" if a.estimator == "plant" else "it keeps its own constants and the nominal gain tables")]) + ([] if not dist else [
             "# the swept race is disturbed (--disturbance %s): the same rows for every vehicle, gusts seeded with --seed; the baseline race is not."
             % a.disturbance]) + ([] if not faults else [
             "# the swept race's sensors are faulted (--sensor-faults %s): the same rows for every vehicle, losses seeded with --seed; the "
             "baseline race's are healthy." % a.sensor_faults]) + [
             "# %d ticks (%.1f s wall); all vehicles: %.1f %% finished, %.1f %% lost, %.1f %% still running; racing lap time median %.3f s, "
             "p90 %.3f s; RMSE_ey median %.4f m" % (ticks, wall, 100 * fin.mean(), 100 * lost.mean(), 100 * (ph < 2).mean(),
                                                     np.nanmedian(lt), np.nanpercentile(lt, 90), np.nanmedian(rmse)),
             ] + ([] if a.walls is None else [
             "# the swept race's tracks have walls (--walls %s): %d vehicles hit one, %d hit ticks, largest impulse %.3g N s, %d vehicles "
             "outside at the end; the baseline race's tracks have none." % (a.walls, walled["hit"], walled["hit_ticks"], walled["most"], walled["outside"])]) + (
             [] if not a.interactions else [
             "# the swept race's vehicles act on each other (--interactions %s): %d vehicles hit, %d hit ticks, %d drafting ticks; the baseline "
             "race's do not." % (a.interactions, contacts["hit"], contacts["hit_ticks"], contacts["draft_ticks"])]) + ([] if a.respawn is None else [
             "# --respawn %d: %d slots respawned, %d alive vehicle-ticks, %.4g alive vehicle-ticks/s over the %d ticks%s"
             % (a.respawn, fork["slots"], fork["alive"], fork["alive"] / wall, ticks,
                " (lost slots refilled every %d ticks: a different experiment, not a faster one; nothing recorded)" % a.respawn if a.respawn else "")]) + [
             "# the same starts with the nominal car: %.1f %% finished, %.1f %% lost (the starts near the end of the lap lose vehicles in "
             "lap 0 and on the first racing laps whatever the car); of the vehicles that finish with the nominal car, %.1f %% are lost "
             "with their own" % (100 * fin_nom.mean(), 100 * (ph_nom == 3).mean(), 100 * lost[fin_nom].mean()),
             "# bins: quartiles of each parameter's factor (row / nominal); lost|nom: lost among the bin's vehicles that finish with the "
             "nominal car; lap time and RMSE_ey over the completed racing laps of the bin",
             "%-4s %-15s %6s %9s %7s %9s %11s %9s %12s" % ("par", "factor bin", "veh", "finished", "lost", "lost|nom", "lap med s", "lap p90",
                                                           "RMSE_ey med")]
    for i, k in enumerate(plant.WORDS):
        if k not in spread:
            continue
        f = rows[:, i] / nom[:, i]
        edges = np.quantile(f, [0, 0.25, 0.5, 0.75, 1.0])
        for j in range(4):
            sel = (f >= edges[j]) & ((f < edges[j + 1]) if j < 3 else (f <= edges[j + 1]))
            l_, r_ = lt[sel], rmse[sel]
            has = np.isfinite(l_).any()
            lines.append("%-4s [%.3f, %.3f] %6d %8.1f%% %6.1f%% %8.1f%% %11s %9s %12s"
                         % (k, edges[j], edges[j + 1], sel.sum(), 100 * fin[sel].mean(), 100 * lost[sel].mean(), 100 * lost[sel & fin_nom].mean(),
                            "%.3f" % np.nanmedian(l_) if has else "-", "%.3f" % np.nanpercentile(l_, 90) if has else "-",
                            "%.4f" % np.nanmedian(r_) if np.isfinite(r_).any() else "-"))
    fleet.close()
    print("\n".join(lines), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
