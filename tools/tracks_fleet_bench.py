#!/usr/bin/env python3
"""Lap-0 fleet tick time with per-vehicle tracks (lpvmpc_set_tracks): tools/tracks_fleet_bench.py [--parent-lib FILE] [--sizes 1024,8192]
Every leg starts a controller N = 20 fleet through lpvmpc_cl_init_tyres with NULL rows, runs 12 warm-up ticks and times five blocks
of 20 ticks on the host (lpvmpc_cl_tick(20) + a read-back); one JSON line per leg with the median block, one child process per leg,
three alternations.  Legs: unbound; unbound on another build of the library (--parent-lib: a file name inside the package directory);
own = a one-entry palette of the handle's own track; copies = six copies of the own track, track_of cycling (the unbound workload
with a mixed fleet's divergent table reads); palette = the six-entry palette of track.palette() (other circuits: another workload;
its line names, per track, the share of solved QPs, the vehicles off their track and the largest iteration count)."""
import json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

def starts(B, seed, maps, of):
    """plant0 [B, 8]: every vehicle on its own track in the first 45 % of the lap, a few centimetres off the centre line and a
    little off its heading, at 0.9 .. 1.1 m/s."""
    from oracle import plant_ref as PR
    rng = np.random.default_rng(seed)
    s = rng.uniform(0.02, 0.45, B) * np.array([m.TrackLength for m in maps])[of]
    ey = rng.normal(0, 0.02, B)
    plant0 = np.zeros((B, 8))
    for b in range(B):
        x, y, th = PR.get_global_position(maps[of[b]].PointAndTangent, s[b], ey[b])
        plant0[b, 0], plant0[b, 1], plant0[b, 6] = x, y, th + rng.normal(0, 0.02)
    plant0[:, 2] = rng.uniform(0.9, 1.1, B)
    return plant0


def child(lib, leg, B):
    from lpvmpc import _ffi
    _ffi.LIB_PATH = os.path.join(os.path.dirname(_ffi.LIB_PATH), lib)
    import lpvmpc
    from lpvmpc import workloads as W
    from lpvmpc import track as TK
    Q, R, dR = W.CTRL_TUNINGS["path"]
    own = lpvmpc.Map("L_shape", 0.2)
    maps = TK.palette() if leg == "palette" else [own] * 6 if leg == "copies" else [own]
    of = TK.cycle(B) if leg in ("palette", "copies") else np.zeros(B, np.int32)
    plant0 = starts(B, 99, maps, of)
    e = lpvmpc.BatchedSolver("controller", 20, 1 / 30.0, Q, R, dR, track=own.PointAndTangent)
    if leg in ("own", "palette", "copies"):
        e.set_tracks(maps, of)
    e.cl_init(plant0, own.halfWidth, own.slack, q9_swap=True, n_sub=7, tyre_params="linear")
    e.cl_tick(12); e.cl_read()
    ts = []
    for _ in range(5):
        t = time.perf_counter(); e.cl_tick(20); e.cl_read(); ts.append((time.perf_counter() - t) / 20 * 1e3)
    o = e.cl_read()
    per = {}
    if leg == "palette":
        names = ("oval", "L_shape", "3110", "Euge_Track", "mirrored L_shape", "oval x 1.3")
        per = {n: dict(solved=float(np.mean(np.isin(o["status"][of == t], (1, 2)))), off_track=int(np.sum(o["local"][of == t, 4] > 9999)),
                       lost=int(np.sum(~np.isfinite(o["plant"][of == t]).all(axis=1))), max_iters=int(o["iters"][of == t].max()))
               for t, n in enumerate(names)}
    print(json.dumps(dict(lib=lib, leg=leg, B=B, ms_per_tick=float(np.median(ts)), ms_blocks=[round(x, 4) for x in ts],
                          solved=float(np.mean(np.isin(o["status"], (1, 2)))), per_track=per)))
    e.close()

if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3], int(sys.argv[4])); sys.exit(0)
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--sizes", default="1024,8192")
    a = ap.parse_args()
    legs = [("liblpvmpc.so", "unbound")] + ([(a.parent_lib, "unbound")] if a.parent_lib else []) + [("liblpvmpc.so", l) for l in ("own", "copies", "palette")]
    for B in [int(x) for x in a.sizes.split(",")]:
        for rep in range(3):
            for lib, leg in legs:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib, leg, str(B)], timeout=180)
                if r.returncode != 0:
                    print("leg failed", lib, leg, B, r.returncode); sys.exit(1)
