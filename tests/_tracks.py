"""Shared by tests/test_tracks_host.py and tests/test_gpu_tracks.py: the palette, the mixed batches and the per-track reference
runs of the per-vehicle tracks (include/lpvmpc.h, "Per-vehicle tracks").

PALETTE: the four shipped tracks plus mirrored(L_shape) and scaled(oval, 1.3); track_of cycles through it (vehicle b is on entry
b mod 6).  Six tables of 6, 7, 12, 14, 7 and 6 rows, lengths 13 .. 19.3 m, right and left turns, three half widths and two slacks.

The batches are the workloads of tests/test_gpu_horizons.py (drawn on the oval or the L shape) with every instance's arc length moved
onto its own track: an instance that starts within a horizon's travel of the lap end keeps its distance to the lap end (its
roll-out still wraps), every other one keeps its fraction of the lap."""
import numpy as np

from oracle import plant_ref as PR

SIZES = (1, 5, 67)


def palette():
    from lpvmpc import track as T
    return T.palette()


def cycle(B, T=6):
    from lpvmpc import track
    return track.cycle(B, T)


def lengths(maps):
    return np.array([float(m.PointAndTangent[-1, 3] + m.PointAndTangent[-1, 4]) for m in maps])


def _move(s, L_from, L_to, near):
    """Arc lengths drawn on a track of length L_from, on tracks of length L_to [B]: the distance to the lap end is kept where it is
    below ``near`` [B], the fraction of the lap elsewhere."""
    s = np.asarray(s, float)
    d = L_from - s
    return np.where(d < near, L_to - d, s / L_from * L_to)


def ctrl_lap0(B, N, seed, maps, of):
    """Controller batch on lap 0 (curvature from each vehicle's map at the rolled-out s), inputs varying from stage to stage."""
    from tests.test_gpu_horizons import ctrl_workload
    w = ctrl_workload(B, N, seed, lap=0, vary=True, vmin=1.2)
    L0 = float(w["track"][-1, 3] + w["track"][-1, 4])
    x0 = w["x0"].copy()
    x0[:, 4] = _move(x0[:, 4], L0, lengths(maps)[of], x0[:, 0] * w["dt"] * N)
    return dict(w, x0=x0, track=None)


def plan(B, N, seed, maps, of):
    """Planner batch whose SS rows run along each vehicle's own track, every third one across the lap end."""
    from tests.test_gpu_horizons import plan_workload
    w = plan_workload(B, N, seed, vary=True)
    L0 = float(w["track"][-1, 3] + w["track"][-1, 4])
    SS = w["curv_s"].copy()
    step = SS[:, 1] - SS[:, 0]
    s0 = _move(SS[:, 0], L0, lengths(maps)[of], step * N)
    return dict(w, curv_s=s0[:, None] + np.arange(N + 1)[None, :] * step[:, None], track=None)


def seed_inputs(B, N, kind, seed, maps, of):
    """Trajectories and steering angles for the seed-mode linearisation; s runs past each vehicle's lap end."""
    rng = np.random.default_rng(seed)
    Lt = lengths(maps)[of][:, None]
    vx = rng.uniform(0.8, 3.0, (B, N)); vy = rng.normal(0, 0.05, (B, N)); wz = rng.normal(0, 0.3, (B, N))
    epsi = rng.normal(0, 0.1, (B, N)); ey = rng.normal(0, 0.1, (B, N)); s = rng.uniform(0.0, 1.5, (B, N)) * Lt
    delta = rng.uniform(-0.24, 0.24, (B, N))
    xx = np.stack([vx, vy, wz, epsi, s, ey], axis=2) if kind == "controller" else np.stack([vx, vy, wz, ey, epsi, s], axis=2)
    return xx, delta


def sub(w, idx):
    """The instances idx of a workload dict."""
    B = w["x0"].shape[0]
    return {k: (v[idx] if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == B and k != "track" else v) for k, v in w.items()}


def groups(of):
    """[(palette entry, indices)] of the entries in use."""
    return [(int(t), np.nonzero(of == t)[0]) for t in np.unique(of)]


def transform_points(B, seed, maps, of):
    """(s, ey) [B, 2] and (x, y, psi) [B, 3] per vehicle on its own track: four of five points inside the track (|ey| below the half
    width, heading off the tangent), every fifth beyond half width + slack (the 10000 sentinels); every seventh s beyond the lap end,
    every eleventh inside the closing row."""
    rng = np.random.default_rng(seed)
    L = lengths(maps)[of]
    hw = np.array([m.halfWidth for m in maps])[of]; sl = np.array([m.slack for m in maps])[of]
    s = rng.uniform(0.02, 0.98, B) * L
    # every eleventh s inside its track's closing row (the last 0.4 % of the lap on 3110 and Euge_Track), from a stream of its own so
    # that every other point stays what it was; a closing row that is empty in float64 (the oval's 6e-16 m) cannot be entered
    u = np.random.default_rng(seed + 77).uniform(0.05, 0.95, B)
    for b in range(10, B, 11):
        last = maps[of[b]].PointAndTangent[-1]
        if last[3] + last[4] > last[3]:
            s[b] = last[3] + u[b] * last[4]
    ey = rng.uniform(-0.9, 0.9, B) * hw
    off = np.arange(B) % 5 == 4
    ey[off] = (hw[off] + sl[off]) * rng.uniform(1.5, 3.0, int(off.sum())) * rng.choice([-1.0, 1.0], int(off.sum()))
    sey = np.column_stack([s, ey])
    pts = np.empty((B, 3))
    for b in range(B):
        x, y, th = PR.get_global_position(maps[of[b]].PointAndTangent, s[b], ey[b])
        pts[b] = (x, y, th + rng.normal(0, 0.2))
    sey[np.arange(B) % 7 == 6, 0] += L[np.arange(B) % 7 == 6]
    return sey, pts


def fleet_starts(B, seed, maps, of):
    """plant0 [B, 8]: every vehicle on its own track, in the first 45 % of the lap (no lap event within a short run), a few
    centimetres off the centre line and a little off its heading, at 0.9 .. 1.1 m/s."""
    rng = np.random.default_rng(seed)
    s = rng.uniform(0.02, 0.45, B) * lengths(maps)[of]
    ey = rng.normal(0, 0.02, B)
    plant0 = np.zeros((B, 8))
    for b in range(B):
        x, y, th = PR.get_global_position(maps[of[b]].PointAndTangent, s[b], ey[b])
        plant0[b, 0], plant0[b, 1], plant0[b, 6] = x, y, th + rng.normal(0, 0.02)
    plant0[:, 2] = rng.uniform(0.9, 1.1, B)
    return plant0


def lap0_replay(maps, of, plant0, T):
    """Host replay of a mixed lap-0 fleet on ground truth (tests/_race_ref.py: oracle/lpv_ref.py, the OSQP restatement and
    oracle/plant_ref.py), one vehicle at a time on its own track with that track's half width and slack: per tick plant, local, cmd,
    iters and status."""
    from tests._race_ref import RaceRef
    refs = [RaceRef(maps[of[b]].PointAndTangent, plant0[b][None], half_width=maps[of[b]].halfWidth, slack=maps[of[b]].slack)
            for b in range(plant0.shape[0])]
    out = []
    for _ in range(T):
        for r in refs:
            r.tick()
        out.append(dict(plant=np.concatenate([r.plant for r in refs]), local=np.concatenate([r.local for r in refs]),
                        cmd=np.concatenate([r.cmd for r in refs]), iters=np.concatenate([r.iters for r in refs]),
                        status=np.concatenate([r.status for r in refs])))
    return out


# ---- the mixed race ----------------------------------------------------------------------------------------------------------
RACE_ENTRIES = (0, 1, 2, 5)          # oval, L shape, 3110, oval x 1.3: four lap lengths (13, 19.23, 19.27, 16.9 m), three half widths
RACE_B = 12
RACE_EVENT_TICKS = (12, 14, 11, 17, 13, 15, 13, 18, 11, 14, 12, 17)      # race_event_ticks of these starts (tests/test_tracks_host.py holds them to it)
RACE_DIST = (0.40, 0.46, 0.52, 0.58, 0.43, 0.49, 0.56, 0.61, 0.38, 0.47, 0.53, 0.59)     # metres before the lap end, per vehicle


def race_palette():
    p = palette()
    return [p[i] for i in RACE_ENTRIES]


def race_starts(maps, of):
    """plant0 [12, 8]: vehicle b RACE_DIST[b] metres before the end of its own lap (HalfTrack = 1), on the centre line and along the
    tangent, at 1 m/s: its lap event falls between the 9 seed ticks and tick 20."""
    plant0 = np.zeros((RACE_B, 8))
    L = lengths(maps)[of]
    for b in range(RACE_B):
        x, y, th = PR.get_global_position(maps[of[b]].PointAndTangent, L[b] - RACE_DIST[b], 0.0)
        plant0[b] = [x, y, 1.0, 0.0, 0.0, 0.0, th, 0.0]
    return plant0


def race_event_ticks(maps, of, plant0, T=24):
    """The tick of each vehicle's lap event in the host replay (tests/_race_ref.py, one vehicle at a time on its own track with that
    track's half width and slack; a vehicle's replay stops at its event), -1: none within T ticks."""
    from tests._race_ref import RaceRef
    ev = np.full(plant0.shape[0], -1)
    for b in range(plant0.shape[0]):
        m = maps[of[b]]
        r = RaceRef(m.PointAndTangent, plant0[b][None], half_track0=1, half_width=m.halfWidth, slack=m.slack)
        for _ in range(T):
            r.tick()
            if r.event_tick[0] >= 0:
                ev[b] = r.event_tick[0]
                break
    return ev
