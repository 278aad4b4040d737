"""Fleets and configurations of tests/test_gpu_race_snapshot.py.

Starts: vehicle b of B stands DIST_LO + (DIST_HI - DIST_LO) * b / (B - 1) metres before the end of its own lap (HalfTrack = 1), at
1 m/s with a little lateral offset and heading error, like tests/_tracks.py's race_starts, whose 0.38 .. 0.61 m give lap events on
ticks 11 .. 18.  At B = 67 the events are spread evenly over those ticks, so at the fork tick T0 = 14 the fleet holds lap-0
vehicles, vehicles on their event tick and racing vehicles at different planner phases.

Configurations:
  C0  plain lpvmpc_race_init on the L shape
  C1  lpvmpc_race_init_tyres: every fourth vehicle on the launch file's Pacejka tyre, actuator delays 4 / 6 steps with the servo
      lag, steeringDelay 3, the estimator behind noisy sensors, gusts, a grip patch behind the start line and a kick at plant step
      KICK_STEP (tick 17: after the fork tick)
  C2  C1 on a two-track palette (oval and L shape, vehicle b on entry b mod 2)"""
import numpy as np

from oracle import plant_ref as PR

T0 = 14                                  # the fork tick: ticks run before the snapshot
DIST_LO, DIST_HI = 0.38, 0.61
KICK_STEP = 120
KV = 0
STD = dict(psi_std=0.01, psiDot_std=0.05, x_std=0.01, y_std=0.01, v_std=0.02)
SIZES = (1, 5, 67)


def lshape():
    import lpvmpc
    return lpvmpc.Map("L_shape", 0.2)


def maps_of(cfg, B):
    """(maps, track_of): one map and None, or C2's palette."""
    if cfg != "C2":
        return [lshape()], None
    from tests import _tracks as TK
    p = TK.race_palette()
    return [p[0], p[1]], (np.arange(B) % 2).astype(np.int32)


def starts(maps, of, B, seed=5):
    rng = np.random.default_rng(seed)
    plant0 = np.zeros((B, 8))
    for b in range(B):
        tab = np.asarray(maps[0 if of is None else of[b]].PointAndTangent, float)
        L = float(tab[-1, 3] + tab[-1, 4])
        d = DIST_LO + (DIST_HI - DIST_LO) * (b / (B - 1) if B > 1 else 0.5)
        x, y, th = PR.get_global_position(tab, L - d, rng.normal(0, 0.01))
        plant0[b] = [x, y, 1.0, 0.0, 0.0, 0.0, th + rng.normal(0, 0.01), 0.0]
    return plant0


def other_starts(maps, of, B):
    """Another fleet on the same tracks: near the middle of the lap (HalfTrack = 0), for the race that a blob is restored into."""
    rng = np.random.default_rng(77)
    plant0 = np.zeros((B, 8))
    for b in range(B):
        tab = np.asarray(maps[0 if of is None else of[b]].PointAndTangent, float)
        L = float(tab[-1, 3] + tab[-1, 4])
        x, y, th = PR.get_global_position(tab, rng.uniform(0.3, 0.5) * L, rng.normal(0, 0.02))
        plant0[b] = [x, y, rng.uniform(0.8, 1.2), 0.0, 0.0, 0.0, th, 0.0]
    return plant0


def disturbance_rows(B):
    from tests._disturbance_ref import ALL_OFF
    rows = np.tile(ALL_OFF, (B, 1))
    rows[:, 0:3] = (0.2, 0.2, 0.3); rows[:, 3] = 0.8                        # gusts
    rows[:, 4:7] = (KICK_STEP, 0.05, -0.15)                                  # the kick
    rows[:, 7:10] = (0.2, 3.0, 0.8)                                          # a patch behind the start line: on the racing lap
    return rows


def obs_cfg(**kw):
    from lpvmpc.observer import observer_config
    from tests._race_observer_ref import estimator_gains
    g = estimator_gains()
    return observer_config(g["L_ls"], g["lim_ls"], g["L_hs"], g["lim_hs"], **kw)


def fleet(cfg, B, plant0=None, half_track0=1):
    """A RaceFleet of configuration cfg, two racing laps (nobody finishes inside a test), started but not ticked."""
    import lpvmpc
    maps, of = maps_of(cfg, B)
    if plant0 is None:
        plant0 = starts(maps, of, B)
    kw = dict(laps=2, half_track0=half_track0, kernel_variant=KV)
    if cfg != "C0":
        kw.update(tyre_params=lpvmpc.tyre_params(B, kind=(np.arange(B) % 4 == 0).astype(float)),
                  actuator=lpvmpc.actuator_config(0.02, 0.03, low_level_dyn=True), steering_delay=3,
                  estimator=obs_cfg(init_vx=1.0, **dict(STD, seed=5)), disturbance=dict(rows=disturbance_rows(B), seed=41))
    if of is not None:
        return lpvmpc.RaceFleet(maps, plant0, track_of=of, **kw)
    return lpvmpc.RaceFleet(maps[0], plant0, **kw)


def reads(f, cfg):
    """Everything the read-backs return: race_read, race_laps, race_predictions and, where present, actuator_read, observer_read and
    disturbances_read."""
    p = f.path
    o = p.race_read()
    o["lap_step"], o["alive"] = p.race_laps()
    o["path_uPred"], o["tt_uPred"] = p.race_predictions()
    if cfg != "C0":
        a = p.actuator_read()
        o["act_state"], o["path_hist"], o["tt_hist"] = a["act_state"], a["path"], a["tt"]
        o["est"], o["meas"] = p.observer_read()
        o["dist_state"] = p.disturbances_read()[1]
    return o


def run_reading(f, cfg, n):
    """n ticks, everything read after each.  plan_valid [B]: the planner has reported for the vehicle -- it runs from the tick after
    the lap event on, so the vehicle entered this or an earlier tick of the window racing; before that plan_iters / plan_status are
    whatever the planner's workspace held when the race was built."""
    out = []
    prev, valid = f.state()["phase"], None
    for _ in range(n):
        f.run(1)
        o = reads(f, cfg)
        valid = (prev == 1) if valid is None else valid | (prev == 1)
        o["plan_valid"] = valid.copy()
        prev = o["phase"]
        out.append(o)
    return out


def same(a, b):
    """Bit for bit: integers exactly, doubles through their 64-bit patterns, except that NaN matches NaN whatever its payload."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind == "f":
        return bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))
    return bool(np.array_equal(a, b))


def assert_reads_equal(a, b, what, idx_a=None, idx_b=None, other_race=False):
    """Two run_reading results; idx_a / idx_b: compare vehicles idx_a of a with vehicles idx_b of b.  other_race: a and b are races
    built separately, whose planner workspaces started with different words: plan_iters / plan_status are compared where the planner
    has reported (plan_valid, itself compared); within one race, or after a restore, they are compared everywhere."""
    assert len(a) == len(b)
    for t, (x, y) in enumerate(zip(a, b)):
        assert sorted(x) == sorted(y)
        for k in x:
            if k == "ticks":
                assert x[k] == y[k], (what, t, k)
                continue
            u = x[k] if idx_a is None else x[k][idx_a]
            v = y[k] if idx_b is None else y[k][idx_b]
            if other_race and k in ("plan_iters", "plan_status"):
                m = x["plan_valid"] if idx_a is None else x["plan_valid"][idx_a]
                u, v = u[m], v[m]
            assert same(u, v), (what, "tick +%d" % (t + 1), k, np.argwhere(np.atleast_1d(u != v))[:4].tolist())


def snaps_equal(a, b, what):
    assert a.header == b.header and a.directory == b.directory, what
    for k in a.arrays:
        assert same(a.arrays[k], b.arrays[k]), (what, k)


def three_phases(snap):
    """Vehicles in lap 0, on their event tick (racing, no racing tick counted before this one) and racing, of a snapshot."""
    ph, rk = snap.arrays["phase"][:, 0], snap.arrays["rk"][:, 0]
    return int(np.sum(ph == 0)), int(np.sum((ph == 1) & (rk == 0))), int(np.sum((ph == 1) & (rk > 0)))


def alive_count(o):
    return int(np.sum((o["phase"] < 2) & np.all(np.isfinite(o["plant"]), axis=1)))
