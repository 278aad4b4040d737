#!/usr/bin/env python3
"""Tuning sweep: ONE recorded race of B vehicles (default 8192), each racing with a trajectory-tracking tuning of its own
(lpvmpc_set_tunings on the tt handle, rows from tuning.sample_tunings around the reference's racing tuning CTRL_TUNINGS["race"]):
B closed-loop evaluations of B tunings in one race.  Default spreads: every diagonal weight of Q and R and both entries of dR
+-SPREAD (default 50 %); the limits, the path controller of lap 0 and the planner keep the reference's tuning.  The vehicles start
near the end of the lap (HalfTrack = 1), so lap 0 is short; two racing laps, the recorder on (its per-lap statistics).  The race
runs until every vehicle has finished or is lost (or --max-ticks).
--plant nominal (default) races the nominal car in every vehicle; --plant sampled gives each vehicle the plant row of
tools/robustness_sweep.py (plant.sample_plant_params(B, seed)): the tuning of a vehicle then meets a car of its own.
Reports survival, racing lap time and per-lap RMSE quantiles over the tunings, the same race with the reference's tuning in every
vehicle (the baseline: same starts, same plants), survival and lap time binned by each weight's factor, and the best rows (finished,
by mean racing lap time) with their factors.
Usage: tools/tuning_sweep.py [--B 8192] [--laps 2] [--seed 1] [--spread 0.5] [--plant nominal|sampled] [--max-ticks 3000] [--best 8]
       [--out FILE]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

# the weights the sweep varies: name, word of the row
VARIED = (("Q_vx", 0), ("Q_vy", 7), ("Q_wz", 14), ("Q_epsi", 21), ("Q_ey", 35), ("dR_delta", 40), ("dR_a", 41))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8192)
    ap.add_argument("--laps", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--spread", type=float, default=0.5)
    ap.add_argument("--plant", default="nominal", choices=("nominal", "sampled"))
    ap.add_argument("--max-ticks", type=int, default=3000)
    ap.add_argument("--best", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import lpvmpc
    from lpvmpc import tuning
    from tests._race_observer_ref import start_line_fleet
    mp = lpvmpc.Map("L_shape", 0.2)
    B = a.B
    plant0 = start_line_fleet(mp.PointAndTangent, B, a.seed, 0.8, 0.97)
    plant_rows = lpvmpc.sample_plant_params(B, a.seed) if a.plant == "sampled" else None

    def race(tt_rows):
        f = lpvmpc.RaceFleet(mp, plant0, laps=a.laps, half_track0=1, plant_params=plant_rows, tt_tunings=tt_rows)
        f.record(1, 1 << 20)                                          # statistics of every tick; one record kept
        t0, n = time.perf_counter(), 0
        while n < a.max_ticks:
            f.run(100); n += 100
            if np.all(f.state()["phase"] >= 2):
                break
        return f, n, time.perf_counter() - t0

    base, _n, _w = race(None)                                         # the reference's tuning in every vehicle
    own = tuning.tuning_rows(1, base.tt)[0]
    ph0 = base.state()["phase"]
    lt0 = base.lap_times()[:, 1:a.laps + 1]
    rows = tuning.sample_tunings(B, a.seed, dict(Q=a.spread, R=a.spread, dR=a.spread), base.tt)
    base.close()
    fleet, ticks, wall = race(rows)
    assert np.array_equal(fleet.tunings()[1], rows)
    ph = fleet.state()["phase"]
    lt = fleet.lap_times()[:, 1:a.laps + 1]
    st = fleet.lap_stats()
    fin, lost = ph == 2, ph == 3
    fin0 = ph0 == 2
    q = lambda v, p: float(np.nanpercentile(v, p)) if np.isfinite(v).any() else float("nan")
    lines = ["# tools/tuning_sweep.py --B %d --laps %d --seed %d --spread %g --plant %s on one MI355X: one recorded race, tt rows from "
             "sample_tunings(B, %d, Q, R, dR +-%.0f %%) around CTRL_TUNINGS[\"race\"]" % (B, a.laps, a.seed, a.spread, a.plant, a.seed, 100 * a.spread),
             "# plants: %s; path controller, planner and all limits: the reference's." %
             ("the nominal car" if plant_rows is None else "sample_plant_params(B, %d) (tools/robustness_sweep.py's perturbed cars)" % a.seed),
             "# %d ticks (%.1f s wall): %.1f %% finished, %.1f %% lost, %.1f %% still running" % (ticks, wall, 100 * fin.mean(), 100 * lost.mean(), 100 * (ph < 2).mean()),
             "# baseline, the reference's tuning in every vehicle: %.1f %% finished, %.1f %% lost; racing lap time median %.3f s" %
             (100 * fin0.mean(), 100 * (ph0 == 3).mean(), q(lt0, 50)),
             "# of the vehicles that finish with the reference's tuning %.1f %% are lost with their own; of those lost with it %.1f %% finish with their own"
             % (100 * lost[fin0].mean() if fin0.any() else float("nan"), 100 * fin[~fin0].mean() if (~fin0).any() else float("nan")),
             "%-22s %10s %10s %10s %10s %10s" % ("over the tunings", "p10", "p25", "median", "p75", "p90")]
    for name, v in (("racing lap time s", lt), ("RMSE_v m/s", st["rmse_v"][:, 1:a.laps + 1]), ("RMSE_ey m", st["rmse_ey"][:, 1:a.laps + 1]),
                    ("RMSE_epsi rad", st["rmse_epsi"][:, 1:a.laps + 1])):
        lines.append("%-22s %10.4f %10.4f %10.4f %10.4f %10.4f" % (name, q(v, 10), q(v, 25), q(v, 50), q(v, 75), q(v, 90)))
    lines.append("# bins: quartiles of each weight's factor (row / reference); lost|ref: lost among the bin's vehicles that finish with the reference's tuning")
    lines.append("%-9s %-15s %6s %9s %7s %9s %11s %9s" % ("weight", "factor bin", "veh", "finished", "lost", "lost|ref", "lap med s", "lap p90"))
    fac = {name: rows[:, w] / own[w] for name, w in VARIED if own[w] != 0}
    for name, f in fac.items():
        edges = np.quantile(f, [0, 0.25, 0.5, 0.75, 1.0])
        for j in range(4):
            sel = (f >= edges[j]) & ((f < edges[j + 1]) if j < 3 else (f <= edges[j + 1]))
            l_ = lt[sel]
            has = np.isfinite(l_).any()
            lines.append("%-9s [%.3f, %.3f] %6d %8.1f%% %6.1f%% %8.1f%% %11s %9s"
                         % (name, edges[j], edges[j + 1], sel.sum(), 100 * fin[sel].mean(), 100 * lost[sel].mean(),
                            100 * lost[sel & fin0].mean() if (sel & fin0).any() else float("nan"),
                            "%.3f" % np.nanmedian(l_) if has else "-", "%.3f" % np.nanpercentile(l_, 90) if has else "-"))
    mean_lap = np.where(fin, np.nanmean(np.where(np.isfinite(lt), lt, np.nan), axis=1), np.inf)
    best = np.argsort(mean_lap)[:a.best]
    lines.append("# the best rows: finished, by mean racing lap time (factors against the reference's tuning)")
    lines.append("%-7s %9s %9s  %s" % ("vehicle", "mean lap", "RMSE_ey", "  ".join("%-8s" % n for n in fac)))
    for b in best:
        if not np.isfinite(mean_lap[b]):
            break
        lines.append("%-7d %9.3f %9.4f  %s" % (b, mean_lap[b], float(np.nanmean(st["rmse_ey"][b, 1:a.laps + 1])), "  ".join("%-8.3f" % fac[n][b] for n in fac)))
    fleet.close()
    print("\n".join(lines), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
