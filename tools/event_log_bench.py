#!/usr/bin/env python3
"""What a race tick costs with the event log attached (lpvmpc_race_events), on one MI355X.

The race: the lpvmpc_race_init_tyres race (kind 0 tyre rows) of B vehicles in heats of --heat consecutive vehicles, heats and default
walls attached.  Two regimes:
  quiet    tools/race_bench.py's lap-0 grid: the vehicles leave one spot at 0.9 .. 1.1 m/s and string out; few events
  busy     every vehicle starts within 5 cm of s = 1 at 1 m/s, across the width of the track, under gusts of 1 m/s^2 on ax (plant
           disturbances, drawn per vehicle) and with footprints of 10 cm x 6 cm: the order inside every heat keeps changing and
           footprints meet and part, tick after tick
Method.  One process.  Per regime --reps races from the same start; in each, after 12 warm ticks (two of them with the log), two
windows of --ticks ticks, one with the log detached and one with it attached, in alternating order from race to race (off-on, on-off,
...), so that both configurations cover the same ticks of the same race equally often.  A window is ONE lpvmpc_race_tick call between
two hipEvents recorded on the engines' stream (the null stream); the host clock around the call and a synchronising read is printed
next to it.  The windows lie in lap 0 (a lap of the L-shaped track at 1 m/s is about 570 ticks: 12 + 2 * ticks stays below).  A tick
of the second window costs more than one of the first whatever is attached (the fleet has strung out), so the two configurations are
compared window by window, never across them: per window the medians over the races that ran it either way, every single figure, and
for the attached windows the events per tick (mean, and min / median / max over the window's ticks, from the log itself).
--lib FILE runs another build's library (the parent commit's): both windows of every race run without the log, the same ticks.
--trace REGIME: no timing; one race, one window with the log attached, for a kernel trace of the run (the heats' launch on the same
ticks is the yardstick).

usage: event_log_bench.py [--B 1024] [--heat 16] [--ticks 200] [--reps 4] [--lib FILE] [--trace quiet|busy] [--out FILE]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def starts(B, mp):
    from oracle import plant_ref as PR
    rng = np.random.default_rng(3)
    grid = np.zeros((B, 8)); grid[:, 1] = rng.normal(0, 0.02, B); grid[:, 2] = rng.uniform(0.9, 1.1, B)
    tab = np.asarray(mp.PointAndTangent, float)
    busy = np.zeros((B, 8))
    for b in range(B):
        x, y, th = PR.get_global_position(tab, 1.0 + 0.05 * rng.random(), rng.uniform(-0.15, 0.15))
        busy[b] = [x, y, 1.0, 0.0, 0.0, 0.0, th, 0.0]
    return {"quiet": grid, "busy": busy}


class DeviceTimer(object):
    """hipEvent time on the null stream, which is the engines' stream; the runtime is the one the library is bound to."""

    def __init__(self, lib):
        self.lib = lib
        for name, args in (("hipEventCreate", [C.POINTER(C.c_void_p)]), ("hipEventRecord", [C.c_void_p, C.c_void_p]),
                           ("hipEventSynchronize", [C.c_void_p]), ("hipEventElapsedTime", [C.POINTER(C.c_float), C.c_void_p, C.c_void_p])):
            f = getattr(lib, name)
            f.argtypes = args; f.restype = C.c_int
        self.e0, self.e1 = C.c_void_p(), C.c_void_p()
        self.ok(lib.hipEventCreate(C.byref(self.e0))); self.ok(lib.hipEventCreate(C.byref(self.e1)))

    @staticmethod
    def ok(rc):
        if rc != 0:
            raise RuntimeError("a HIP event call failed with %d" % rc)

    def time(self, call):
        self.ok(self.lib.hipEventRecord(self.e0, None))
        call()
        self.ok(self.lib.hipEventRecord(self.e1, None))
        self.ok(self.lib.hipEventSynchronize(self.e1))
        ms = C.c_float(0)
        self.ok(self.lib.hipEventElapsedTime(C.byref(ms), self.e0, self.e1))
        return float(ms.value)


def new_race(a, regime, plant0, mp):
    import lpvmpc
    from lpvmpc import disturbance as D
    from tools.race_bench import engines
    path, tt, plan = engines(mp)
    path.race_init(tt, plan, plant0, half_track0=0, laps=50, half_width=mp.halfWidth, slack=mp.slack, tyre_params=lpvmpc.tyre_params(a.B, kind=0))
    heat = np.arange(a.B) // a.heat
    if regime == "busy":
        path.set_disturbances(D.disturbance_rows(a.B, float(mp.TrackLength), sigma_ax=1.0, rho=0.5), seed=1)
        path.race_heats(heat, half_length=0.05, half_width=0.03)
    else:
        path.race_heats(heat)
    path.race_walls({})
    return path, tt, plan


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--heat", type=int, default=16)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--trace", default=None, choices=("quiet", "busy"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from lpvmpc import _ffi
    if a.lib:
        _ffi.LIB_PATH = os.path.abspath(a.lib)
    import lpvmpc
    lib = _ffi.load()
    has_log = hasattr(lib, "lpvmpc_race_events")
    which = "the library given with --lib" if a.lib else "this build"
    mp = lpvmpc.Map("L_shape", 0.2)
    cap = 1 << 20
    lines = []
    for regime, plant0 in starts(a.B, mp).items():
        if a.trace and regime != a.trace:
            continue
        dev = {}; host = {}; events = {}                                       # by (window, log attached)
        phases = None
        for rep in range(1 if a.trace else a.reps):
            path, tt, plan = new_race(a, regime, plant0, mp)
            timer = DeviceTimer(lib)
            path.race_tick(10); path.race_read()                               # warm: every kernel of a tick has run
            if has_log:
                path.race_events(dict(capacity=cap))
            path.race_tick(2); path.race_read()
            if has_log:
                path.race_events(detach=True)
            order = [True] if a.trace else ([False, True] if rep % 2 == 0 else [True, False])
            for w, on in enumerate(order):
                log = on and has_log
                if log:
                    path.race_events(dict(capacity=cap))
                path.race_read()
                t0 = time.perf_counter()
                ms = timer.time(lambda: path.race_tick(a.ticks))
                path.race_read()
                host.setdefault((w, log), []).append((time.perf_counter() - t0) * 1e3 / a.ticks)
                dev.setdefault((w, log), []).append(ms / a.ticks)
                if log:
                    r = path.race_events_read()
                    per = np.bincount(r["events"]["tick"] - r["events"]["tick"].min(), minlength=1) if r["kept"] else np.zeros(1, int)
                    per = np.concatenate([per, np.zeros(max(0, a.ticks - per.shape[0]), int)])     # (quiet ticks at the window's ends)
                    events.setdefault(w, []).append("%.1f (%d / %d / %d%s)" % (r["total"] / a.ticks, per.min(), int(np.median(per)), per.max(),
                                                              ", ring overran" if r["total"] > cap else ""))
                    path.race_events(detach=True)
            phases = np.bincount(path.race_read()["phase"], minlength=4).tolist()
            for e in (path, tt, plan):
                e.close()
        if a.trace:
            print("traced %s: %d ticks with the log, events per tick %s, phases %s" % (regime, a.ticks, events, phases), flush=True)
            continue
        fmt = lambda v: " ".join("%.4f" % x for x in v)
        n0 = len(lines)
        for w in (0, 1):
            first = 12 + w * a.ticks
            off = float(np.median(dev[(w, False)]))
            lines.append("%-6s B=%5d heats of %d  ticks %3d .. %3d  log off  device %.4f ms/tick (races %s)  host clock %.4f (%s)  %s"
                         % (regime, a.B, a.heat, first, first + a.ticks - 1, off, fmt(dev[(w, False)]), float(np.median(host[(w, False)])),
                            fmt(host[(w, False)]), which))
            if (w, True) in dev:
                on = float(np.median(dev[(w, True)]))
                lines.append("%-6s B=%5d heats of %d  ticks %3d .. %3d  log on   device %.4f ms/tick (races %s)  host clock %.4f (%s)  %+.4f ms/tick on the device"
                             "  events per tick, mean (min / median / max): %s"
                             % (regime, a.B, a.heat, first, first + a.ticks - 1, on, fmt(dev[(w, True)]), float(np.median(host[(w, True)])),
                                fmt(host[(w, True)]), on - off, "  ".join(events[w])))
        lines.append("%-6s phases after the last race %s" % (regime, phases))
        for l in lines[n0:]:
            print(l, flush=True)
    if a.out and lines:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
