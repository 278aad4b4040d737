"""GPU: the track geometry on the edge grid of tests/_track_edges.py -- seams, one ulp either side of them, lap ends, closing rows,
the width limit, headings half a turn and several turns off the tangent -- against the float64-exact lookup rules and the long
double restatement: a decided case must be met (flags and sentinels exactly, coordinates within E.GPU_BOUND_*), an undecided one
must be one of its forced variants.  Stand-alone transforms (plain handles, a bound handle with all eight tracks in one batch,
Map's own methods), the curvature lookup through the seed-mode linearisation and through the lap-0 roll-out of lpv, the lap-0
fleet's and the race's measurement beside seams, in closing rows and off the track, the recorder's track channels, and the
planner pose of the hand-off with stages beside seams.  Plain and bound forms throughout.  NaN compares as NaN."""
import numpy as np
import pytest

from oracle import lpv_ref as L
from tests import _track_edges as E

pytestmark = pytest.mark.gpu
P = dict(L.DEFAULT_PARAMS)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def plain_engine(track=None):
    import lpvmpc
    return lpvmpc.BatchedSolver("controller", 8, 1.0 / 30.0, np.eye(6), np.eye(2), np.ones(2), track=track)


@pytest.fixture(scope="module")
def grid():
    return E.grid()


@pytest.fixture(scope="module")
def plain(grid):
    """(local [n, 4], global [n, 3]) of a plain handle per track, on the whole grid of that track: one call per route."""
    out = []
    for g in grid:
        e = plain_engine(g["tab"])
        out.append((e.local_position(g["loc"]["pts"], g["map"].halfWidth, g["map"].slack), e.global_position(g["glob"]["sey"])))
        e.close()
    return out


def check_global(g, got):
    """NaN exactly where the rule finds no row; elsewhere the pose within E.GPU_BOUND_GLOBAL of the long double restatement on the
    rule's row.  What that pins of the lookup: a wrong row is caught wherever its pose differs -- every point more than the bound
    (in metres) from a seam, and both sides of a seam without a common tangent (the backward closing rows of 3110 and Euge_Track,
    the closing rows of `full` and of the mirrored and scaled tracks).  At a seam with a common tangent, centre line and offset
    curves of the two rows are continuous: within one ulp of it, the neighbour's formula gives the same x, y and theta to 1e-15, so
    there global_position's choice of row has no observable consequence and this check cannot see it.  The row itself is observable
    through the curvature: test_curvature_through_the_seed_mode_linearisation and test_lpv_roll_out_from_a_seam hold
    track_curvature to the rule's row at the same abscissae."""
    row = g["glob"]["row"]
    assert np.array_equal(np.isnan(got).any(axis=1), row < 0) and np.array_equal(np.isnan(got).all(axis=1), row < 0), g["map"].shape
    worst = 0.0
    for n in np.nonzero(row >= 0)[0]:
        x, y, th, r = E.global_ld(g["tab"], *g["glob"]["sey"][n])
        dev = max(abs(float(x) - got[n, 0]), abs(float(y) - got[n, 1]), abs(float(th) - got[n, 2]))
        assert dev <= E.GPU_BOUND_GLOBAL, (g["map"].shape, n, g["glob"]["sey"][n], dev)
        worst = max(worst, dev)
    return worst


def test_plain_transforms_on_the_grid(grid, plain):
    wl, wg = np.zeros(3), 0.0
    for g, (loc, glob) in zip(grid, plain):
        bad, w = E.check_local(loc, g["exp"])
        assert not bad, (g["map"].shape, len(bad), bad[:5], loc[bad[:5]], [g["exp"][n].rows for n in bad[:5]])
        wl, wg = np.maximum(wl, w), max(wg, check_global(g, glob))
        assert np.all(loc[loc[:, 3] == 0, :3] == 10000) and set(np.unique(loc[:, 3])) <= {0.0, 1.0}
    print("plain transforms on the grid: worst deviation on decided cases local s %.3e ey %.3e epsi %.3e (bounds %.1e %.1e %.1e), global %.3e (bound %.1e)"
          % (tuple(wl) + E.LOCAL_BOUNDS + (wg, E.GPU_BOUND_GLOBAL)))


@pytest.mark.parametrize("B", (1, 63, 65))
def test_slices_equal_the_rows_of_the_full_call(grid, plain, B):
    for t in (2, 6):                                        # 3110 and the 16-row track
        g, (loc, glob) = grid[t], plain[t]
        e = plain_engine(g["tab"])
        for start in (0, 200):
            assert same(e.local_position(g["loc"]["pts"][start:start + B], g["map"].halfWidth, g["map"].slack), loc[start:start + B])
            assert same(e.global_position(g["glob"]["sey"][start:start + B]), glob[start:start + B])
        n = g["glob"]["sey"].shape[0]
        assert same(e.global_position(g["glob"]["sey"][n - B:]), glob[n - B:])             # the specials: -0.0, 4096 L, inf, nan
        e.close()


def test_bound_transforms_equal_the_plain_ones(grid, plain):
    """All eight tracks in one batch on a handle without a table of its own: word for word the plain handles' rows."""
    maps = [g["map"] for g in grid]
    of_l = np.concatenate([np.full(g["loc"]["pts"].shape[0], g["t"], np.int32) for g in grid])
    of_g = np.concatenate([np.full(g["glob"]["sey"].shape[0], g["t"], np.int32) for g in grid])
    rng = np.random.default_rng(3)
    pl, pg = rng.permutation(of_l.size), rng.permutation(of_g.size)        # neighbouring lanes on different tracks
    e = plain_engine()
    e.set_tracks(maps, of_l[pl])
    loc = e.local_position(np.concatenate([g["loc"]["pts"] for g in grid])[pl], 123.0, 456.0)
    e.set_tracks(maps, of_g[pg])
    glob = e.global_position(np.concatenate([g["glob"]["sey"] for g in grid])[pg])
    e.close()
    assert same(loc, np.concatenate([p[0] for p in plain])[pl])
    assert same(glob, np.concatenate([p[1] for p in plain])[pg])


def test_map_methods_on_a_handful_of_points(grid, plain):
    for t in (0, 2, 3):
        g, (loc, glob) = grid[t], plain[t]
        m = g["map"]
        for n in np.linspace(0, loc.shape[0] - 1, 6).astype(int):
            assert same(np.array(m.getLocalPosition(*g["loc"]["pts"][n]), float), loc[n])
        for n in np.linspace(0, glob.shape[0] - 1, 6).astype(int):
            assert same(np.array(m.getGlobalPosition(*g["glob"]["sey"][n]), float), glob[n])


@pytest.mark.parametrize("kind,N", [("controller", 9), ("planner", 13)])
def test_curvature_through_the_seed_mode_linearisation(grid, kind, N):
    """estimate_abc with the stage abscissae on the grid's s values, plain and bound: where the rule finds a row the blocks are those
    of the oracle given that row's curvature (1e-12 relative, the bar of test_estimate_abc_batch), and they are non-finite exactly
    where it finds none."""
    import lpvmpc
    dt = 1 / 30.0 if kind == "controller" else 0.05

    def engine(track=None):
        if kind == "controller":
            return lpvmpc.BatchedSolver("controller", N, dt, np.eye(6), np.eye(2), np.ones(2), track=track)
        return lpvmpc.BatchedSolver("planner", N, dt, np.eye(5), np.eye(2), np.ones(2), L_cf=np.zeros(5), track=track)

    vx, vy, wz, epsi, ey, delta = 1.5, 0.02, 0.1, 0.05, 0.07, 0.1
    xs, of, As, Bs = [], [], [], []
    worst = 0.0
    for g in grid:
        s = E.s_grid(g["tab"])[0]
        s = np.concatenate([s, np.full(-s.size % N, s[0])]).reshape(-1, N)
        o = np.ones_like(s)
        xx = np.stack([vx * o, vy * o, wz * o, epsi * o, s, ey * o] if kind == "controller" else [vx * o, vy * o, wz * o, ey * o, epsi * o, s], axis=2)
        e = engine(g["tab"])
        A, Bm = e.estimate_abc(xx, delta * o)
        e.close()
        ref = {}
        for b in range(s.shape[0]):
            for i in range(N):
                cur = E.curvature_rule(g["tab"], s[b, i])
                fin = bool(np.all(np.isfinite(A[b, i])) and np.all(np.isfinite(Bm[b, i])))
                assert fin == (not np.isnan(cur)), (g["map"].shape, s[b, i], cur)
                if fin:
                    if cur not in ref:
                        ref[cur] = L.ctrl_AB(P, dt, vx, vy, epsi, ey, cur, delta) if kind == "controller" else L.plan_AB(P, dt, vx, vy, ey, epsi, cur, delta)
                    for got, want in ((A[b, i], ref[cur][0]), (Bm[b, i], ref[cur][1])):
                        err = float(np.max(np.abs(got - want))) / max(1.0, float(np.max(np.abs(want))))
                        assert err <= 1e-12, (g["map"].shape, s[b, i], err)
                        worst = max(worst, err)
        xs.append(xx); of.append(np.full(s.shape[0], g["t"], np.int32)); As.append(A); Bs.append(Bm)
    xx, of = np.concatenate(xs), np.concatenate(of)
    perm = np.random.default_rng(4).permutation(of.size)
    e = engine()
    e.set_tracks([g["map"] for g in grid], of[perm])
    A, Bm = e.estimate_abc(xx[perm], np.full(xx.shape[:2], delta))
    e.close()
    assert same(A, np.concatenate(As)[perm]) and same(Bm, np.concatenate(Bs)[perm])
    print("%s N=%d: curvature on %d abscissae, plain and bound word for word, max rel err %.2e" % (kind, N, xx.shape[0] * N, worst))


# ---- the lap-0 roll-out of lpv from a seam ---------------------------------------------------------------------------------------
def test_lpv_roll_out_from_a_seam(grid):
    """lpv(lap = 0), controller N = 9, with x0's s on every seam and every offset of the grid (the lap itself) and on the specials
    that have no row, plain and bound.  Where the rule finds a row for x0's s the states and blocks are the oracle's (1e-11 of each
    array's largest magnitude, the bar of tests/test_gpu_horizons.py for lpv); where it finds none, stage 0 is non-finite."""
    import lpvmpc
    N, dt = 9, 1 / 30.0
    engine = lambda track=None: lpvmpc.BatchedSolver("controller", N, dt, np.eye(6), np.eye(2), np.ones(2), track=track)
    xs, ofs, outs = [], [], []
    worst = 0.0
    for g in grid:
        tab = g["tab"]
        s, j, d, lap = E.s_grid(tab)
        top = E.MAX_WRAP_LAPS * E.lap_length(tab)
        s = s[((j >= 0) & (lap == 0)) | ((j < 0) & ~(s == top))]             # (from 4096 L the roll-out leaves the range at stage 1)
        B = s.size
        x0 = np.column_stack([np.full(B, 1.4), np.full(B, 0.02), np.full(B, 0.1), np.full(B, 0.05), s, np.full(B, 0.07)])
        u_prev = np.tile([0.05, 0.3], (B, N, 1)); vel = np.full((B, N + 1), 1.4)
        e = engine(tab)
        S, A, Bm = e.lpv(x0, u_prev, vel, None, cf_new=60.0, lap=0)
        e.close()
        for b in range(B):
            if E.lookup_row(tab, s[b])[0] < 0:
                assert not np.all(np.isfinite(A[b, 0])), (g["map"].shape, s[b])
                continue
            Sr, Ar, Br = L.ctrl_lpv_prediction(P, dt, N, tab, x0[b], u_prev[b], vel[b], None, 60.0, 0)
            for got, want in ((S[b], Sr), (A[b], Ar), (Bm[b], Br)):
                err = float(np.max(np.abs(got - want))) / max(1.0, float(np.max(np.abs(want))))
                assert err <= 1e-11, (g["map"].shape, s[b], err)
                worst = max(worst, err)
        xs.append(x0); ofs.append(np.full(B, g["t"], np.int32)); outs.append((S, A, Bm))
    x0, of = np.concatenate(xs), np.concatenate(ofs)
    perm = np.random.default_rng(6).permutation(of.size)
    e = engine()
    e.set_tracks([g["map"] for g in grid], of[perm])
    got = e.lpv(x0[perm], np.tile([0.05, 0.3], (of.size, N, 1)), np.full((of.size, N + 1), 1.4), None, cf_new=60.0, lap=0)
    e.close()
    for k in range(3):
        assert same(got[k], np.concatenate([o[k] for o in outs])[perm]), k
    print("lpv lap-0 roll-out from %d abscissae on seams: plain and bound word for word, max rel err %.2e" % (of.size, worst))


# ---- the lap-0 fleet's and the race's measurement ----------------------------------------------------------------------------
def fleet_starts(g, n_in=48, n_off=16):
    """Case indices of at most 64 decided starts of one track beside seams (|ds| = 1e-9, 1e-6): n_in on the track, a quarter of
    them at the lap end and in the closing row, headings on the tangent, 0.3 off it and one and three turns (+ 0.1) ahead of it;
    and n_off off the track, at |ey| = (hw + slack)(1 + 1e-9) and 2 (hw + slack)."""
    loc, exp = g["loc"], g["exp"]
    base = np.array([e.decided for e in exp]) & (loc["kind"] == E.KIND_GRID) & (loc["lap"] == 0) & np.isin(loc["ds"], (3, 4, 5, 6))
    base &= np.isin(loc["idpsi"], (0, 1, 4, 6))
    inside = np.array([e.rows[0, 3] == 1 for e in exp])
    ok = base & inside & np.isin(loc["iey"], (0, 1, 2, 3, 4))
    close = np.nonzero(ok & (loc["seam"] >= g["tab"].shape[0] - 1))[0]
    rest = np.nonzero(ok & (loc["seam"] < g["tab"].shape[0] - 1))[0]
    off = np.nonzero(base & ~inside & np.isin(loc["iey"], (5, 6, 7, 8)))[0]
    close = close[np.linspace(0, close.size - 1, min(close.size, n_in // 4)).astype(int)]
    rest = rest[np.linspace(0, rest.size - 1, n_in - close.size).astype(int)]
    off = off[np.linspace(0, off.size - 1, n_off).astype(int)]
    return np.concatenate([close, rest, off])


def starts_and_measurement(g):
    """plant0 [B, 8] of fleet_starts, every eighth vehicle below the vx clamp, and the measurement the restatement expects of it in
    the q9_swap ordering [vx, vy, wz, ey, s, epsi] with vx clamped at 0.01 -- the 10000 sentinels for a start off the track."""
    idx = fleet_starts(g)
    assert 48 <= idx.size <= 64
    pts = g["loc"]["pts"][idx]
    plant0 = np.zeros((idx.size, 8))
    plant0[:, 0], plant0[:, 1], plant0[:, 6] = pts[:, 0], pts[:, 1], pts[:, 2]
    plant0[:, 2] = np.where(np.arange(idx.size) % 8 == 7, 0.005, 1.0)
    rows = np.array([g["exp"][n].rows[0] for n in idx])
    assert np.sum(rows[:, 3] == 0) == 16 and np.all(rows[rows[:, 3] == 0, :3] == 10000)
    want = np.column_stack([np.maximum(plant0[:, 2], 0.01), np.zeros(idx.size), np.zeros(idx.size), rows[:, 1], rows[:, 0], rows[:, 2]])
    return plant0, want


def measured(got, want, what):
    """Sentinels exactly; s and ey within E.GPU_BOUND_LOCAL, epsi within E.GPU_BOUND_EPSI; vx, vy, wz exactly.  Returns the worst."""
    off = want[:, 4] == 10000
    assert np.array_equal(got[off], want[off]), what
    assert np.array_equal(got[:, :3], want[:, :3]), what
    dev = np.abs(got[~off, 3:] - want[~off, 3:])
    assert np.all(dev <= np.array([E.GPU_BOUND_LOCAL, E.GPU_BOUND_LOCAL, E.GPU_BOUND_EPSI])), (what, dev.max(axis=0))
    return float(dev.max())


def test_lap0_fleet_measurement_beside_seams(grid):
    """cl_init (plain kernels), cl_init with the tyre rows on a handle of the track, and the bound fleet with all eight tracks: after
    one tick, cl_read()["local"] is the restatement of plant0; a start off the track is not refused and delivers the sentinels; the
    three routes agree word for word."""
    from lpvmpc import workloads as W
    import lpvmpc
    Q, R, dR = W.CTRL_TUNINGS["path"]
    engine = lambda track=None: lpvmpc.BatchedSolver("controller", 20, 1 / 30.0, Q, R, dR, track=track)
    p0s, ofs, locs = [], [], []
    worst = 0.0
    for g in grid:
        plant0, want = starts_and_measurement(g)
        got = []
        for kw in ({}, dict(tyre_params="linear")):
            e = engine(g["tab"])
            e.cl_init(plant0, g["map"].halfWidth, g["map"].slack, q9_swap=True, n_sub=7, **kw)
            e.cl_tick(1)
            got.append(e.cl_read()["local"])
            e.cl_release()
            e.close()
        assert same(got[0], got[1]), g["map"].shape
        worst = max(worst, measured(got[0], want, g["map"].shape))
        p0s.append(plant0); ofs.append(np.full(plant0.shape[0], g["t"], np.int32)); locs.append(got[0])
    plant0, of = np.concatenate(p0s), np.concatenate(ofs)
    perm = np.random.default_rng(5).permutation(of.size)
    e = engine()
    e.set_tracks([g["map"] for g in grid], of[perm])
    e.cl_init(plant0[perm], 123.0, 456.0, q9_swap=True, n_sub=7, tyre_params="linear")
    e.cl_tick(1)
    loc = e.cl_read()["local"]
    e.cl_release()
    e.close()
    assert same(loc, np.concatenate(locs)[perm])
    print("lap-0 fleet measurement on %d starts beside seams, %d of them off the track: worst deviation %.3e" % (of.size, 16 * len(grid), worst))


def test_race_measurement_and_track_channels(grid):
    """One race_tick in lap 0 (HalfTrack = 0: no lap event) with the recorder on, on handles of the track and on bound handles, the
    starts of the fleet test.  race_read()["local"] is the restatement of plant0; the recorder's track channels and inside flag of
    that tick are local_position of the plant it recorded, word for word (as tests/test_gpu_race_record.py defines them); plain
    and bound agree word for word."""
    from tests.test_gpu_tracks import race_engines

    def one_tick(plant0, mp=None, bind=None):
        path, tt, plan = race_engines(mp, bind)
        kw = dict(half_width=mp.halfWidth, slack=mp.slack) if bind is None else dict(tyre_params="linear", half_width=123.0, slack=456.0)
        path.race_init(tt, plan, plant0, half_track0=0, laps=1, **kw)
        path.race_record(1)
        path.race_tick(1)
        o, rec = path.race_read(), path.race_record_read()
        for e in (path, tt, plan):
            e.close()
        return o["local"], o["phase"], rec

    worst = 0.0
    for t in (0, 2, 3, 6):                                  # oval (a 6e-16 m closing row), 3110 and Euge_Track (backward ones), 16 rows
        g = grid[t]
        m = g["map"]
        plant0, want = starts_and_measurement(g)
        loc, phase, rec = one_tick(plant0, mp=m)
        assert np.all(phase == 0), phase
        worst = max(worst, measured(loc, want, m.shape))
        e = plain_engine(g["tab"])
        lp = e.local_position(np.stack([rec["x"][0], rec["y"][0], rec["yaw"][0]], axis=1), m.halfWidth, m.slack)
        e.close()
        assert same(rec["track"][0], lp[:, :3]) and np.array_equal(rec["inside"][0], lp[:, 3].astype(np.int32)), m.shape
        of = np.zeros(plant0.shape[0], np.int32)
        loc_b, phase_b, rec_b = one_tick(plant0, bind=([m], of))
        assert same(loc_b, loc) and same(phase_b, phase) and same(rec_b["track"], rec["track"]) and same(rec_b["inside"], rec["inside"]), m.shape
    print("race measurement beside seams on 4 tracks, plain and bound: worst deviation %.3e" % worst)


# ---- the planner pose of the hand-off ----------------------------------------------------------------------------------------
def test_planner_pose_with_stages_beside_seams(grid):
    """handoff, N = 40, vx = 1 and everything else 0, so SS advances by dt = 0.05 per stage.  SS[0] is chosen so that stage 5 lands
    at seam + d for every seam of the track (the closing row's start and the lap end included) and d = +-1e-9, +-1e-6: the stages
    cross the lap end and run through the closing rows of 3110 and Euge_Track.  SS, pose and sig against
    oracle.handoff_ref.planner_pose_refs at 1e-11 (test_handoff_other_horizon_vs_oracle's); no stage falls in another segment: the
    rule's row of every stage of the device's SS is that of the oracle's.  Plain and bound word for word."""
    import lpvmpc
    from lpvmpc import workloads as W
    from oracle import handoff_ref as H
    N, dt = 40, 0.05
    engine = lambda track=None: lpvmpc.BatchedSolver("planner", N, dt, W.PLAN_Q, W.PLAN_R, W.PLAN_dR, L_cf=W.PLAN_L, track=track)
    n_seams = 0
    for t in (0, 2, 3, 4, 6):                               # oval, 3110, Euge_Track, mirrored(L_shape), the 16-row track
        g = grid[t]
        tab = g["tab"]
        Lt = E.lap_length(tab)
        s0 = np.array([seam + d - 5 * dt for seam in E.seams(tab) for d in (-1e-9, 1e-9, -1e-6, 1e-6)])
        s0 = np.where(s0 < 0, s0 + Lt, s0)
        B = s0.size
        x = np.zeros((B, N + 1, 5)); x[:, :, 0] = 1.0
        SS = s0[:, None] + np.arange(N + 1)[None, :] * dt
        pose = np.array([H.get_global_position(tab, s, 0.0) for s in s0], float)
        e = engine(tab)
        e.handoff_setup()
        o = e.handoff(x, SS, pose, want_sig=True)
        e.close()
        entered = set()
        for b in range(B):
            SSr, last, xp, yp, yaw, vel, curv = H.planner_pose_refs(tab, x[b], SS[b], tuple(pose[b]), dt)
            assert np.max(np.abs(o["SS"][b] - SSr)) <= 1e-11 and np.max(np.abs(o["pose"][b] - np.array(last))) <= 1e-11, (g["map"].shape, b)
            assert np.max(np.abs(o["sig"][b] - np.array([xp, yp, yaw, vel, curv]))) <= 1e-11, (g["map"].shape, b)
            rows_dev = [E.lookup_row(tab, v)[0] for v in o["SS"][b]]
            assert rows_dev == [E.lookup_row(tab, v)[0] for v in SSr] and min(rows_dev) >= 0, (g["map"].shape, b)
            entered |= set(rows_dev)
            assert abs(SSr[5] - (s0[b] + 5 * dt)) <= 1e-12                       # stage 5 is where it was aimed: 1e-9 or 1e-6 from the seam
        assert np.any(o["SS"] > Lt), g["map"].shape                            # stages beyond the lap end
        if tab[-1, 3] + tab[-1, 4] > tab[-1, 3]:
            assert tab.shape[0] - 1 in entered, g["map"].shape                 # and inside the closing row
        n_seams += B // 4
        eb = engine()
        eb.set_tracks([g["map"]], np.zeros(B, np.int32))
        eb.handoff_setup()
        ob = eb.handoff(x, SS, pose, want_sig=True)
        eb.close()
        for k in ("SS", "pose", "sig", "refs"):
            assert same(ob[k], o[k]), (g["map"].shape, k)
    print("planner pose with stages beside %d seams: plain and bound word for word" % n_seams)
