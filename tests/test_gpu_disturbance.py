"""GPU: plant disturbances (lpvmpc_set_disturbances, lpvmpc_disturbances_read, lpvmpc_plant_step_disturbed_batch).  All-off rows change
no word of a step, a lap-0 fleet or a race; the stand-alone step, the patch geometry, the kick and the gusts match the numpy
restatement (tests/_disturbance_ref.py) under the project's 1e-11 bar for device plant steps; draws are independent of sharding; the
gusts' statistics sit inside five standard errors; disturbed fleets and races match the host replay under the bars of the tyre
model's tests; read-back and refusals."""
import ctypes as C

import numpy as np
import pytest

from tests import _disturbance_ref as D
from tests import _race_observer_ref as RO
from tests import _tyre_ref as T
from tests.test_gpu_delayed_fleets import STD, close, ctrl, engines, lshape, obs_cfg, same
from tests.test_gpu_plant_params import NOM, RACE_KEYS, _race_same

pytestmark = pytest.mark.gpu

HW0, SLACK0 = 0.3, 0.15                  # lpvmpc_race_default_config: the stand-alone step's map width on an unbound handle
LINEAR = (0.0, 6.0, 1.6, 0.8)


def off(B):
    return np.tile(D.ALL_OFF, (B, 1))


def around(mp, B, seed):
    """B poses spread along the map with a little lateral offset, heading error, speed and yaw rate."""
    from oracle import plant_ref as PR
    rng = np.random.default_rng(seed)
    L = D.lap_length(mp.PointAndTangent)
    st = np.zeros((B, 8))
    for b in range(B):
        x, y, th = PR.get_global_position(mp.PointAndTangent, (b + 0.37) / B * L, rng.normal(0, 0.03))
        st[b] = [x, y, rng.uniform(0.8, 1.4), rng.normal(0, 0.02), 0.0, 0.0, th + rng.normal(0, 0.02), rng.normal(0, 0.2)]
    return st


def local_s(mp, st, hw, slack):
    from oracle import plant_ref as PR
    return np.array([PR.get_local_position(mp.PointAndTangent, hw, slack, p[0], p[1], p[6])[0] for p in st])


# ---- 1. all-off rows attached against nothing attached ------------------------------------------------------------------------
def test_all_off_step_is_the_tyre_step():
    import lpvmpc
    mp = lshape()
    B = 16
    st0 = around(mp, B, 1)
    u = np.column_stack([np.full(B, 0.8), np.where(np.arange(B) % 2, 0.2, -0.2)])
    rows, tyres = lpvmpc.sample_plant_params(B, 2), lpvmpc.sample_tyre_params(B, 2, kind=(np.arange(B) % 2).astype(float))
    e = ctrl(mp)
    a = e.plant_step_vehicles(st0, u, rows, None, n_sub=7, tyre_params=tyres)
    b = e.plant_step_disturbed(st0, u, off(B), None, plant_params=rows, tyre_params=tyres, n_sub=7, seed=9)
    assert same(a[0], b[0]) and same(a[1], b[1])
    assert same(b[2], np.column_stack([np.zeros((B, 3)), np.ones(B), np.ones(B)]))
    e.close()


def cl_run(mp, plant0, n_ticks, est=None, dist=None, attach_tick=0, **kw):
    e = ctrl(mp)
    if est is not None:
        e.observer_setup(est)
    e.cl_init(plant0, mp.halfWidth, mp.slack, q9_swap=True, n_sub=7, **kw)
    out = []
    for t in range(n_ticks):
        if dist is not None and t == attach_tick:
            e.set_disturbances(**dist)
        e.cl_tick(1)
        o = e.cl_read()
        if est is not None:
            o["est"], o["meas"] = e.observer_read()
        o.update(e.actuator_read())
        out.append(o)
    if dist is not None:
        out.append(e.disturbances_read()[1])
    e.close()
    return out


CL_KEYS = ("plant", "local", "cmd", "iters", "status", "act_state", "path")


@pytest.mark.parametrize("est", [False, True])
def test_all_off_lap0_fleet_is_the_undisturbed_fleet(est):
    import lpvmpc
    mp = lshape()
    B, n = 16, 20
    plant0 = RO.grid_fleet(B, 3)
    kw = dict(plant_params=lpvmpc.sample_plant_params(B, 5), tyre_params=lpvmpc.sample_tyre_params(B, 5),
              est=obs_cfg(**dict(STD, seed=5)) if est else None)
    a = cl_run(mp, plant0, n, **kw)
    b = cl_run(mp, plant0, n, dist=dict(rows=off(B), seed=11), **kw)
    for t in range(n):
        for k in CL_KEYS + (("est", "meas") if est else ()):
            assert np.array_equal(a[t][k], b[t][k]), (t, k)
    assert same(b[n], np.column_stack([np.zeros((B, 3)), np.full(B, float(n)), np.ones(B)]))


def race_run(mp, plant0, n_ticks, dist=None, **kw):
    path, tt, plan = engines(mp)
    path.race_init(tt, plan, plant0, laps=2, half_width=mp.halfWidth, slack=mp.slack, **kw)
    if dist is not None:
        path.set_disturbances(**dist)
    out = []
    for _ in range(n_ticks):
        path.race_tick(1)
        o = path.race_read()
        o.update(path.actuator_read())
        out.append(o)
    last = dict(zip(("path_uPred", "tt_uPred"), path.race_predictions()))
    last.update(zip(("lap_step", "alive"), path.race_laps()))
    out.append(last)
    close(path, tt, plan)
    return out


def test_all_off_race_is_the_undisturbed_race():
    import lpvmpc
    mp = lshape()
    B, n = 8, 30
    plant0 = RO.start_line_fleet(mp.PointAndTangent, B, 7, 0.975, 0.985)
    kw = dict(half_track0=1, plant_params=lpvmpc.sample_plant_params(B, 4), tyre_params=lpvmpc.tyre_params(B))
    a = race_run(mp, plant0, n, **kw)
    b = race_run(mp, plant0, n, dist=dict(rows=off(B), seed=3), **kw)
    _race_same(a, b, n, RACE_KEYS + ("act_state", "path", "tt"))            # (the planner's report from each vehicle's first planner tick on)
    assert np.any(a[n - 1]["phase"] == 1)                                   # through a lap event


# ---- 2. the stand-alone step against the restatement ---------------------------------------------------------------------------
def component_rows(B, s, L):
    """Quarters of the batch: gusts alone, the kick alone, a patch under the vehicle alone, all three."""
    rows = off(B)
    q = np.arange(B) * 4 // B
    g, k, p = (q == 0) | (q == 3), (q == 1) | (q == 3), (q == 2) | (q == 3)
    rows[g, 0:3] = (0.6, 0.9, 1.5); rows[g, 3] = 0.8
    rows[k, 4:7] = (17.0, 0.15, -0.6)                                       # in the third of the five calls
    rows[p, 7] = np.mod(s[p] - 0.3, L); rows[p, 8] = 2.0; rows[p, 9] = 0.45
    rows[q == 3, 10] = np.mod(s[q == 3] - 1.0, L); rows[q == 3, 11] = 1.5; rows[q == 3, 12] = 0.8
    return rows


@pytest.mark.parametrize("tyre", [LINEAR, T.LAUNCH_FILE], ids=["linear", "pacejka"])
def test_step_matches_the_restatement(tyre):
    """B = 32 around the L shape, n_sub = 7, five chained calls carrying dist_state and act_state: plant and d_* within 1e-11 of the
    restatement, ticks and gamma exact; the restatement without the rows misses psiDot by more than 1e-3."""
    import lpvmpc
    mp = lshape()
    B, n, calls = 32, 7, 5
    tr, L = mp.PointAndTangent, D.lap_length(mp.PointAndTangent)
    st0 = around(mp, B, 4)
    prow, tyres = lpvmpc.sample_plant_params(B, 6), np.tile(tyre, (B, 1))
    rows = component_rows(B, local_s(mp, st0, HW0, SLACK0), L)
    u = np.column_stack([np.full(B, 0.6), np.where(np.arange(B) % 2, 0.25, -0.25)])
    model = D.Model(rows, seed=77, vehicle_offset=5, n_bound=2.5)
    e = ctrl(mp)
    st, act, ds = st0, None, None
    ref, plain = st0.copy(), st0.copy()
    worst = worst_d = miss = 0.0
    gammas = set()
    for c in range(calls):
        st, act, ds = e.plant_step_disturbed(st, u, rows, ds, seed=77, vehicle_offset=5, n_bound=2.5, plant_params=prow, tyre_params=tyres,
                                             act_state=act, n_sub=n)
        for b in range(B):
            ref[b] = D.step_tick(model, b, ref[b], n * c, u[b], prow[b], tyres[b], n, 0.005, tr, HW0, SLACK0)
            plain[b] = D.step_tick(model, b, plain[b], n * c, u[b], prow[b], tyres[b], n, 0.005, tr, HW0, SLACK0, ignore_rows=True)
        worst = max(worst, float(np.max(np.abs(st - ref))))
        worst_d = max(worst_d, float(np.max(np.abs(ds[:, :3] - model.state[:, :3]))))
        assert np.array_equal(ds[:, 3:], model.state[:, 3:]), c
        miss = max(miss, float(np.max(np.abs(st[:, 7] - plain[:, 7]))))
        gammas |= set(ds[:, 4].tolist())
    print("disturbed step (%s): plant %.3e, d %.3e vs the restatement; without the rows psiDot misses by %.3g; gammas %s"
          % ("pacejka" if tyre[0] else "linear", worst, worst_d, miss, sorted(gammas)))
    assert worst <= 1e-11 and worst_d <= 1e-11
    assert miss > 1e-3
    assert {1.0, 0.45, 0.45 * 0.8} <= gammas and np.all(act[:, -1] == n * calls)
    e.close()


# ---- 3. patch geometry on the device -------------------------------------------------------------------------------------------
PATCH_CASES = ("before", "inside", "after", "across_from_behind", "across_from_ahead", "overlap", "off_map", "whole_lap")


def patch_case(name, L):
    """(s, ey, row words 7 .. 12, gamma) of a vehicle at s with patches placed around it."""
    if name == "before":
        return 3.0, 0.05, (3.5, 1.0, 0.5, 0, 0, 1), 1.0
    if name == "inside":
        return 3.0, 0.05, (2.5, 1.0, 0.5, 0, 0, 1), 0.5
    if name == "after":
        return 3.0, 0.05, (1.5, 1.0, 0.5, 0, 0, 1), 1.0
    if name == "across_from_behind":                                        # the vehicle before the line, the patch ends after it
        return L - 0.4, -0.05, (L - 1.0, 2.0, 0.25, 0, 0, 1), 0.25
    if name == "across_from_ahead":                                         # the vehicle after the line, the patch starts before it
        return 0.6, 0.05, (L - 1.0, 2.0, 0.25, 0, 0, 1), 0.25
    if name == "overlap":
        return 3.0, 0.0, (2.0, 2.0, 0.5, 2.5, 3.0, 0.75), 0.375
    if name == "off_map":
        return 3.0, 1.0, (2.5, 1.0, 0.5, 0, 0, 1), 1.0
    return 3.0, 0.05, (7.0, L, 0.7, 0, 0, 1), 0.7


def test_patch_geometry_on_a_two_track_palette():
    """16 vehicles placed with global_position on (oval, L shape), eight cases on each: gamma exact; the step equals the undisturbed
    step with Cf, Cr, c_f = gamma * base, word for word (the live words are gamma * base); a fleet reads its base rows back."""
    import lpvmpc
    maps = [lpvmpc.Map("oval", 0.2), lpvmpc.Map("L_shape", 0.2)]
    B = 16
    of = (np.arange(B) // 8).astype(np.int32)
    Ls = np.array([D.lap_length(m.PointAndTangent) for m in maps])[of]
    sey, rows, want = np.zeros((B, 2)), off(B), np.zeros(B)
    for b in range(B):
        s, ey, words, g = patch_case(PATCH_CASES[b % 8], Ls[b])
        sey[b] = (s, ey); rows[b, 7:13] = words; want[b] = g
    e = ctrl(maps[0])
    e.set_tracks(maps, of)
    xyth = e.global_position(sey)
    loc = e.local_position(xyth, 0, 0)
    assert np.array_equal(loc[:, 3] == 0, np.arange(B) % 8 == 6)            # only the off-map case is outside
    st0 = np.zeros((B, 8)); st0[:, 0:2] = xyth[:, 0:2]; st0[:, 6] = xyth[:, 2]; st0[:, 2] = 1.2; st0[:, 7] = 0.3
    u = np.column_stack([np.full(B, 0.5), np.full(B, 0.2)])
    prow = lpvmpc.sample_plant_params(B, 8)
    tyres = lpvmpc.sample_tyre_params(B, 8, kind=(np.arange(B) % 2).astype(float))
    st, act, ds = e.plant_step_disturbed(st0, u, rows, None, plant_params=prow, tyre_params=tyres, n_sub=7)
    assert np.array_equal(ds[:, 4], want), (ds[:, 4], want)
    sp, sty = prow.copy(), tyres.copy()
    sp[:, 4] = want * prow[:, 4]; sp[:, 5] = want * prow[:, 5]; sty[:, 3] = want * tyres[:, 3]
    ref = e.plant_step_vehicles(st0, u, sp, None, n_sub=7, tyre_params=sty)
    assert same(st, ref[0]) and same(act, ref[1])
    plain = e.plant_step_vehicles(st0, u, prow, None, n_sub=7, tyre_params=tyres)
    assert np.array_equal(np.any(st != plain[0], axis=1), want != 1.0)
    # the same rows on a bound lap-0 fleet: gamma after one tick, and the base rows read back while the live words are scaled
    e.cl_init(st0, 0, 0, q9_swap=True, n_sub=7, plant_params=prow, tyre_params=tyres)
    e.set_disturbances(rows)
    e.cl_tick(1)
    r, state = e.disturbances_read()
    assert np.array_equal(r, rows) and np.array_equal(state[:, 4], want) and np.all(state[:, 3] == 1)
    assert same(e.plant_params_read(), prow) and same(e.tyre_params_read(), tyres)
    e.set_disturbances(None)                                                # detached: the reads come from the live tables again
    assert same(e.plant_params_read(), prow) and same(e.tyre_params_read(), tyres)
    e.close()


# ---- 4. the kick ---------------------------------------------------------------------------------------------------------------
def test_kick_is_applied_once():
    """kick_step 3 inside the first call of 7 steps; kick_step 7 == k0 + n belongs to the second call; neither comes again."""
    mp = lshape()
    B, n = 2, 7
    st0 = around(mp, B, 9)
    rows = off(B); rows[:, 4:7] = ((3.0, 0.2, -0.5), (7.0, 0.2, -0.5))
    u = np.tile([0.5, 0.1], (B, 1))
    tyres = np.tile(T.LAUNCH_FILE, (B, 1))
    e = ctrl(mp)
    model = D.Model(rows)
    st, act, ds = st0, None, None
    ref = st0.copy()
    for c in range(3):
        prev, prev_act = st, act
        st, act, ds = e.plant_step_disturbed(st, u, rows, ds, tyre_params=tyres, act_state=act, n_sub=n)
        quiet = e.plant_step_vehicles(prev, u, None, prev_act, n_sub=n, tyre_params=tyres)[0]      # the same call without a kick
        for b in range(B):
            ref[b] = D.step_tick(model, b, ref[b], n * c, u[b], NOM, tyres[b], n, 0.005, mp.PointAndTangent, HW0, SLACK0)
        assert np.max(np.abs(st - ref)) <= 1e-11, c
        kicked = [not same(st[b], quiet[b]) for b in range(B)]
        assert kicked == [c == 0, c == 1], (c, kicked)
    e.close()


def test_frozen_race_vehicle_is_not_touched():
    """A race vehicle that takes no plant step because it is lost (on the first tick) gets neither kick nor gust, and its tick count
    stays 0; the finished case is the next test."""
    import lpvmpc
    mp = lshape()
    B = 8
    plant0 = RO.start_line_fleet(mp.PointAndTangent, B, 5)
    plant0[2, 2] = np.inf
    rows = off(B); rows[:, 0:4] = (0.3, 0.3, 0.3, 0.5); rows[:, 4:7] = (0.0, 0.2, 0.3)
    path, tt, plan = engines(mp)
    path.race_init(tt, plan, plant0, half_track0=1, half_width=mp.halfWidth, slack=mp.slack, tyre_params="linear")
    path.set_disturbances(rows, seed=2)
    path.race_tick(3)
    o, (_, state) = path.race_read(), path.disturbances_read()
    live = np.arange(B) != 2
    assert o["phase"][2] == 3 and same(o["plant"][2], plant0[2]) and state[2].tolist() == [0.0, 0.0, 0.0, 0.0, 1.0]
    assert np.all(state[live, 3] == 3) and np.all(state[live, :3] != 0) and np.all(o["phase"][live] < 2)
    close(path, tt, plan)


def test_finished_race_vehicle_is_not_touched():
    """A one-lap race: four vehicles at the reference trace's start just before the line race their lap and finish while four that
    started from the grid are still in lap 0.  Disturbances attached then leave the finished vehicles' plant, state and tick count
    alone and reach the others."""
    from tests._golden import load
    mp = lshape()
    B = 8
    plant0 = RO.grid_fleet(B, 4)
    plant0[:4] = load("cascade")["pre_plant"][0]
    half = (np.arange(B) < 4).astype(np.int32)
    path, tt, plan = engines(mp)
    path.race_init(tt, plan, plant0, half_track0=half, laps=1, half_width=mp.halfWidth, slack=mp.slack, tyre_params="linear")
    ticks = 0
    while ticks < 1500 and not np.any(path.race_read()["phase"][:4] == 2):
        path.race_tick(25); ticks += 25
    before = path.race_read()
    done = before["phase"] == 2
    print("finished after <= %d ticks: phases %s" % (ticks, before["phase"].tolist()))
    assert np.any(done[:4]) and np.all(before["phase"][4:] == 0)
    rows = off(B); rows[:, 0:4] = (0.3, 0.3, 0.3, 0.5)
    rows[:, 4:7] = (float(path.actuator_read()["act_state"][4, -1]), 0.2, 0.3)      # the kick inside the next tick of the lap-0 vehicles
    path.set_disturbances(rows, seed=2)
    path.race_tick(3)
    o, (_, state) = path.race_read(), path.disturbances_read()
    assert same(o["plant"][done], before["plant"][done]) and np.all(o["phase"][done] == 2)
    assert np.all(state[done] == [0.0, 0.0, 0.0, 0.0, 1.0])
    assert np.all(state[4:, 3] == 3) and np.all(state[4:, :3] != 0) and not same(o["plant"][4:], before["plant"][4:])
    close(path, tt, plan)


# ---- 5. sharding ---------------------------------------------------------------------------------------------------------------
def test_gusts_do_not_depend_on_sharding():
    """A 64-vehicle lap-0 fleet with gusts over 15 ticks equals two 32-vehicle fleets with vehicle_offset 0 / 32 bit for bit, and
    itself run again."""
    import lpvmpc
    mp = lshape()
    B, n, h = 64, 15, 32
    plant0 = RO.grid_fleet(B, 6)
    rows = lpvmpc.sample_disturbances(B, 4)
    prow, tyres = lpvmpc.sample_plant_params(B, 4), lpvmpc.sample_tyre_params(B, 4)

    def run(lo, hi):
        return cl_run(mp, plant0[lo:hi], n, plant_params=prow[lo:hi], tyre_params=tyres[lo:hi], dist=dict(rows=rows[lo:hi], seed=21, vehicle_offset=lo))

    whole, again, a, b = run(0, B), run(0, B), run(0, h), run(h, B)
    for t in range(n):
        for k in CL_KEYS:
            assert same(whole[t][k], again[t][k]) and same(whole[t][k], np.concatenate([a[t][k], b[t][k]])), (t, k)
    assert same(whole[n], again[n]) and same(whole[n], np.concatenate([a[n], b[n]]))
    quiet = cl_run(mp, plant0, n, plant_params=prow, tyre_params=tyres)
    assert np.max(np.abs(whole[n - 1]["plant"] - quiet[n - 1]["plant"])) > 1e-4 and np.all(whole[n][:, :3] != 0)


# ---- 6. gust statistics --------------------------------------------------------------------------------------------------------
def test_gust_statistics():
    """B = 4096, n_sub = 1, sigma 1, rho 0.8, n_bound 10, 22 chained calls: across vehicles at tick 20, each channel within five
    standard errors (|std - 1| <= 5 / sqrt(2 B), |mean| <= 5 / sqrt(B), lag-1 correlation against tick 21 within 5 (1 - rho^2) /
    sqrt(B) of rho), and within 1e-11 of the restatement's process."""
    from tests.test_disturbance_host import gust_run
    c = D.GUST_CASE
    B = c["B"]
    mp = lshape()
    rows = off(B); rows[:, :3] = c["sigma"]; rows[:, 3] = c["rho"]
    st = np.tile([0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0], (B, 1))
    u = np.zeros((B, 2))
    e = ctrl(mp)
    act = ds = None
    hist = []
    for _ in range(c["calls"]):
        st, act, ds = e.plant_step_disturbed(st, u, rows, ds, seed=c["seed"], n_bound=c["n_bound"], act_state=act, n_sub=1)
        hist.append(ds[:, :3].copy())
    e.close()
    assert np.all(ds[:, 3] == c["calls"]) and np.all(np.isfinite(st))
    ref = gust_run(**c)
    b_std, b_mean, b_rho = D.gust_bars(B, c["rho"])
    for ch in range(3):
        sd, mean, r = D.gust_stats(hist[20][:, ch], hist[21][:, ch])
        print("channel %d: std %.4f (bar %.4f), mean %.4f (bar %.4f), lag-1 %.4f (bar %.4f)" % (ch, sd, b_std, mean, b_mean, r, b_rho))
        assert abs(sd - 1.0) <= b_std and abs(mean) <= b_mean and abs(r - c["rho"]) <= b_rho
    assert max(float(np.max(np.abs(hist[t] - ref[t]))) for t in (0, 20, 21)) <= 1e-11


# ---- 7. lap-0 fleet against the host replay ------------------------------------------------------------------------------------
def fleet_rows(B):
    rows = off(B)
    rows[:, 0:3] = (0.3, 0.5, 1.0); rows[:, 3] = 0.8
    rows[:, 4:7] = (70.0, 0.1, -0.4)
    rows[:, 7:10] = (0.3, 1.0, 0.6)
    rows[B // 2:, 10:13] = (0.8, 2.0, 0.8)
    return rows


@pytest.mark.parametrize("est", [False, True])
def test_disturbed_lap0_fleet_matches_the_replay(est):
    """A Pacejka fleet with gusts, a patch behind the grid and a kick at plant step 70 over 30 ticks against the host replay: plant,
    measurement and command within 2e-6, identical iteration counts and statuses (test_pacejka_lap0_fleet_matches_the_replay's
    rule); the undisturbed replay differs."""
    import lpvmpc
    mp = lshape()
    B, n = 16, 30
    plant0 = RO.grid_fleet(B, 21)
    plant0[:, 7] = np.where(np.arange(B) % 2, 0.5, -0.5)
    prow, tyres = lpvmpc.sample_plant_params(B, 17), lpvmpc.sample_tyre_params(B, 17)
    rows = fleet_rows(B)
    e = ctrl(mp)
    if est:
        e.observer_setup(obs_cfg(**dict(STD, seed=3)))
    e.cl_init(plant0, mp.halfWidth, mp.slack, q9_swap=True, n_sub=7, plant_params=prow, tyre_params=tyres)
    e.set_disturbances(rows, seed=41, vehicle_offset=3)
    rkw = dict(plant_params=prow, tyre_params=tyres, half_track0=0, laps=1, half_width=mp.halfWidth, slack=mp.slack,
               **(dict(gains=RO.estimator_gains(), stds=(0.01, 0.05, 0.01, 0.01, 0.02), seed=3) if est else {}))
    ref = D.DisturbedRaceRef(mp.PointAndTangent, plant0, rows, dist_seed=41, dist_offset=3, **rkw)
    quiet = T.TyreRaceRef(mp.PointAndTangent, plant0, **rkw)
    worst = differs = 0.0
    seen = set()
    for t in range(n):
        e.cl_tick(1); ref.tick(); quiet.tick()
        o = e.cl_read()
        differs = max(differs, float(np.max(np.abs(quiet.plant - ref.plant))))
        assert np.all(ref.phase == 0), t
        assert np.array_equal(o["iters"], ref.iters) and np.array_equal(o["status"], ref.status), t
        worst = max(worst, *(float(np.max(np.abs(o[k] - v))) for k, v in (("plant", ref.plant), ("local", ref.local), ("cmd", ref.cmd))))
        if est:
            worst = max(worst, float(np.max(np.abs(e.observer_read()[0] - ref.estimate()))))
        seen |= set(e.disturbances_read()[1][:, 4].tolist())
    state = e.disturbances_read()[1]
    print("disturbed lap-0 fleet est %d: vs replay %.2e over %d ticks; the undisturbed replay differs by %.3g" % (est, worst, n, differs))
    assert worst <= 2e-6
    assert np.array_equal(state[:, 3:], ref.model.state[:, 3:]) and np.max(np.abs(state[:, :3] - ref.model.state[:, :3])) <= 1e-11
    assert differs > 1e-3 and {1.0, 0.6, 0.6 * 0.8} <= seen <= {1.0, 0.6, 0.8, 0.6 * 0.8}      # both patches were driven through
    e.close()


# ---- 8. race against the host replay -------------------------------------------------------------------------------------------
RACE_SEED = 17


def race_rows(B):
    rows = off(B)
    rows[:, 4:7] = (150.0, 0.1, -0.3)                                       # plant step 150: tick 21
    rows[:, 7:10] = (0.2, 3.0, 0.7)                                         # behind the start line: on the racing lap
    return rows


def test_disturbed_race_matches_the_replay():
    """8 vehicles on the launch file's Pacejka tyre through their lap events, a patch on the racing lap and a kick, attached at tick
    10, against the host replay under test_pacejka_race_matches_the_replay's rule: lap 0 within 2e-6, the same event ticks, the same
    vehicles lost, and in each survivor's first 24 racing ticks two thirds within 1e-5 / 1e-4, all within 2e-2, >= 95 % equal
    iteration counts, equal statuses, at least four different event ticks (its vehicle counts, 8 of 12, are two thirds of the fleet:
    here 5 of 8).  Detach returns the base
    rows to the live tables."""
    import lpvmpc
    mp = lshape()
    B, W_, attach = 8, 24, 10
    plant0 = RO.start_line_fleet(mp.PointAndTangent, B, RACE_SEED, 0.90, 0.975)
    prow, tyres = lpvmpc.sample_plant_params(B, 23), lpvmpc.tyre_params(B)
    rows = race_rows(B)
    path, tt, plan = engines(mp)
    path.race_init(tt, plan, plant0, half_track0=1, laps=3, half_width=mp.halfWidth, slack=mp.slack, plant_params=prow, tyre_params=tyres)
    ref = D.DisturbedRaceRef(mp.PointAndTangent, plant0, rows, attach_tick=attach, tyre_params=tyres, plant_params=prow, half_track0=1, laps=3,
                             half_width=mp.halfWidth, slack=mp.slack)
    racing = np.zeros(B, int)
    ev_dev = np.full(B, -1)
    w_state = np.zeros(B); w_cmd = np.zeros(B); same_it = n_it = 0
    lost_dev, lost_ref, st_diff = {}, {}, []
    err0 = np.zeros(B)
    gammas = set()
    t = 0
    while np.any(racing < W_) and t < 200:
        if t == attach:
            path.set_disturbances(rows)
        ph_before = ref.phase.copy()
        path.race_tick(1); ref.tick()
        o = path.race_read()
        if t >= attach:
            gammas |= set(path.disturbances_read()[1][:, 4].tolist())
        ev_dev[(ev_dev < 0) & (o["phase"] == 1)] = t
        lap0 = (o["phase"] == 0) & (ref.phase == 0)
        assert np.array_equal(o["phase"] == 0, ref.phase == 0), t
        lost0 = (ph_before == 0) & (o["phase"] == 3)
        assert np.array_equal(lost0, (ph_before == 0) & (ref.phase == 3)), t
        if np.any(lap0):
            for a_, b_ in ((o["plant"], ref.plant), (o["local"], ref.local), (o["cmd"], ref.cmd)):
                for v, ev in zip(np.nonzero(lap0)[0], np.abs(a_[lap0] - b_[lap0]).max(axis=1)):
                    err0[v] = max(err0[v], float(ev))
            assert np.array_equal(o["iters"][lap0], ref.iters[lap0]) and np.array_equal(o["status"][lap0], ref.status[lap0]), t
        w = (o["phase"] == 1) & (ref.phase == 1) & (ref.event_tick < t) & (racing < W_)
        for v in np.nonzero(w)[0]:
            fin_d, fin_r = np.all(np.isfinite(o["cmd"][v])), np.all(np.isfinite(ref.cmd[v]))
            if not fin_d and v not in lost_dev:
                lost_dev[int(v)] = int(racing[v])
            if not fin_r and v not in lost_ref:
                lost_ref[int(v)] = int(racing[v])
            if not (fin_d and fin_r):
                continue
            w_state[v] = max(w_state[v], float(np.max(np.abs(o["plant"][v] - ref.plant[v]))), float(np.max(np.abs(o["local"][v] - ref.local[v]))))
            w_cmd[v] = max(w_cmd[v], float(np.max(np.abs(o["cmd"][v] - ref.cmd[v]))))
            if o["status"][v] != ref.status[v]:
                st_diff.append((t, int(v), int(o["status"][v]), int(ref.status[v])))
            same_it += int(o["iters"][v] == ref.iters[v]); n_it += 1
        racing[w] += 1
        done = (racing >= W_) | (ref.phase >= 2) | (o["phase"] >= 2)
        racing[done] = W_
        ref.phase[done] = np.maximum(ref.phase[done], 2)
        t += 1
    need = 2 * B // 3
    surv = np.array([v not in lost_dev for v in range(B)])
    surv_ref = np.array([v not in lost_ref and ref.event_tick[v] >= 0 for v in range(B)])
    strict = surv & (w_state <= 1e-5) & (w_cmd <= 1e-4)
    kept = np.array([ref.phase[v] != 3 or ref.event_tick[v] >= 0 for v in range(B)])
    print("disturbed race vs replay: %d ticks, events %s, lap 0 worst %.3g, survivors within 1e-5 / 1e-4: %d of %d, worst survivor %.3g / %.3g, "
          "lost %s, iterations %d / %d, gammas %s" % (t, sorted(ref.event_tick.tolist()), err0[kept].max(), strict.sum(), surv.sum(),
                                                      w_state[surv].max(), w_cmd[surv].max(), lost_dev, same_it, n_it, sorted(gammas)))
    assert surv_ref.sum() >= need                                                           # the replay alone, on the CPU
    assert np.all((racing >= W_) | (ev_dev < 0)) and n_it > 0 and np.sum(ev_dev >= 0) >= need
    assert np.array_equal(ev_dev, ref.event_tick) and len(set(ev_dev[ev_dev >= 0].tolist())) >= 4
    assert kept.sum() >= need and np.all(err0[kept] <= 2e-6)
    assert lost_dev == lost_ref
    assert not st_diff, st_diff
    assert same_it >= 0.95 * n_it
    assert strict.sum() >= 2 * surv.sum() // 3
    assert np.all(w_state[surv] <= 2e-2) and np.all(w_cmd[surv] <= 2e-2)
    assert gammas == {1.0, 0.7} and np.all(ev_dev[ev_dev >= 0] > attach)                    # the patch was driven through, racing
    assert same(path.plant_params_read(), prow) and same(path.tyre_params_read(), tyres)    # the base rows while attached
    path.set_disturbances(None)
    assert same(path.plant_params_read(), prow) and same(path.tyre_params_read(), tyres)    # and the live tables after the detach
    with pytest.raises(lpvmpc.LpvMpcError):
        path.disturbances_read()
    close(path, tt, plan)


# ---- 9. read-back and refusals -------------------------------------------------------------------------------------------------
def test_read_back_and_refusals_leave_a_running_fleet_untouched():
    """disturbances_read returns the rows given; each refusal gives LPVMPC_E_ARG and the fleet it was tried on runs on, equal word
    for word to one that was never asked; fleets without the tables, a release and a new fleet carry no binding."""
    import lpvmpc
    from lpvmpc import _ffi
    mp = lshape()
    B = 8
    L = D.lap_length(mp.PointAndTangent)
    plant0 = RO.grid_fleet(B, 2)
    prow, tyres = lpvmpc.sample_plant_params(B, 3), lpvmpc.sample_tyre_params(B, 3, kind=[0, 1] * 4)
    rows = lpvmpc.sample_disturbances(B, 5, lap_length=L, spread=dict(sigma_ay=(0.2, 0.5), rho=(0.5, 0.9), p0_s0=(0, 1), p0_len=(1, 2), p0_gamma=(0.4, 0.9)))
    e, f = ctrl(mp), ctrl(mp)
    with pytest.raises(lpvmpc.LpvMpcError):
        e.disturbances_read()                                                 # no fleet
    lib = e._lib
    cfg = _ffi.default_disturbance_config()
    assert lib.lpvmpc_set_disturbances(e._h, B, C.byref(cfg), _ffi.ptr(rows)) == _ffi.E_ARG     # no fleet
    for x in (e, f):
        x.cl_init(plant0, mp.halfWidth, mp.slack, plant_params=prow, tyre_params=tyres)
        x.set_disturbances(rows, seed=7)
        x.cl_tick(3)
    r, state = e.disturbances_read()
    assert same(r, rows) and np.all(state[:, 3] == 3) and np.all(state[:, 1] != 0) and np.all(state[:, [0, 2]] == 0)
    assert lib.lpvmpc_disturbances_read(e._h, None, None) == 0
    bad_words = [(0, -0.1), (1, np.nan), (2, np.inf), (3, 1.0), (3, -0.01), (4, 2.5), (4, 2.0 ** 31), (5, np.nan), (6, -np.inf), (7, -0.1), (7, L),
                 (8, -1.0), (8, L * 1.001), (9, -0.5), (10, L), (11, 2 * L), (12, np.nan)]
    for i, v in bad_words:
        bad = rows.copy(); bad[B - 1, i] = v
        assert lib.lpvmpc_set_disturbances(e._h, B, C.byref(cfg), _ffi.ptr(bad)) == _ffi.E_ARG, (i, v)
        e2 = ctrl(mp)
        st = np.tile(plant0[:1], (B, 1)); u = np.zeros((B, 2))
        rc = e2._lib.lpvmpc_plant_step_disturbed_batch(e2._h, B, _ffi.ptr(st), None, _ffi.ptr(u), 1, 0.005, 0.05, None, None, None, None, None,
                                                      C.byref(cfg), _ffi.ptr(bad), None)
        assert rc == _ffi.E_ARG, (i, v)
        e2.close()
    e2 = ctrl(mp)
    for i, v in ((0, np.nan), (1, np.inf), (2, -np.inf), (3, 1.5), (3, -1.0), (3, np.nan)):                # the carried state's words
        st = np.tile(plant0[:1], (B, 1)); u = np.zeros((B, 2)); ds = np.tile([0.0, 0.0, 0.0, 2.0, 1.0], (B, 1)); ds[B - 1, i] = v
        rc = e2._lib.lpvmpc_plant_step_disturbed_batch(e2._h, B, _ffi.ptr(st), None, _ffi.ptr(u), 1, 0.005, 0.05, None, None, None, None, None,
                                                      C.byref(cfg), _ffi.ptr(rows), _ffi.ptr(ds))
        assert rc == _ffi.E_ARG and same(st, np.tile(plant0[:1], (B, 1))), (i, v)
    e2.close()
    for nb in (0.0, -1.0, np.nan, np.inf):
        c2 = _ffi.default_disturbance_config(); c2.n_bound = nb
        assert lib.lpvmpc_set_disturbances(e._h, B, C.byref(c2), _ffi.ptr(rows)) == _ffi.E_ARG, nb
    assert lib.lpvmpc_set_disturbances(e._h, B - 1, C.byref(cfg), _ffi.ptr(rows)) == _ffi.E_ARG             # B mismatch
    st = np.tile(plant0[:1], (B, 1)); u = np.zeros((B, 2))
    rc = lib.lpvmpc_plant_step_disturbed_batch(e._h, B, _ffi.ptr(st), None, _ffi.ptr(u), 1, 0.005, 0.05, None, None, None, None, None,
                                               C.byref(cfg), _ffi.ptr(rows), None)
    assert rc == _ffi.E_ARG                                                   # a batch call on a handle that runs a fleet
    assert same(e.disturbances_read()[0], rows) and same(e.plant_params_read(), prow) and same(e.tyre_params_read(), tyres)
    e.cl_tick(5); f.cl_tick(5)
    a, b = e.cl_read(), f.cl_read()
    for k in ("plant", "local", "cmd", "iters", "status"):
        assert same(a[k], b[k]), k
    assert same(e.disturbances_read()[1], f.disturbances_read()[1])
    # a release frees the binding; a new fleet starts undisturbed; fleets without the tables have nothing to scale
    e.cl_release()
    with pytest.raises(lpvmpc.LpvMpcError):
        e.disturbances_read()
    e.cl_init(plant0, mp.halfWidth, mp.slack, plant_params=prow, tyre_params=tyres)
    with pytest.raises(lpvmpc.LpvMpcError):
        e.disturbances_read()
    g = ctrl(mp)
    g.cl_init(plant0, mp.halfWidth, mp.slack, plant_params=prow, tyre_params=tyres)
    e.cl_tick(4); g.cl_tick(4)
    assert same(e.cl_read()["plant"], g.cl_read()["plant"])
    for kw in (dict(), dict(plant_params=prow)):
        g.cl_init(plant0, mp.halfWidth, mp.slack, **kw)
        assert g._lib.lpvmpc_set_disturbances(g._h, B, C.byref(cfg), _ffi.ptr(rows)) == _ffi.E_ARG
        g.cl_tick(1)
    close(e, f, g)
    path, tt, plan = engines(mp)
    path.race_init(tt, plan, plant0, half_width=mp.halfWidth, slack=mp.slack, plant_params=prow)
    assert path._lib.lpvmpc_set_disturbances(path._h, B, C.byref(cfg), _ffi.ptr(rows)) == _ffi.E_ARG         # a race without tyre rows
    path.cl_release()
    path.race_init(tt, plan, plant0, half_width=mp.halfWidth, slack=mp.slack, plant_params=prow, tyre_params=tyres)
    assert tt._lib.lpvmpc_set_disturbances(tt._h, B, C.byref(cfg), _ffi.ptr(rows)) == _ffi.E_ARG            # not the path handle
    path.set_disturbances(rows, seed=7)
    path.race_tick(2)
    bad = rows.copy(); bad[0, 3] = 1.5
    assert path._lib.lpvmpc_set_disturbances(path._h, B, C.byref(cfg), _ffi.ptr(bad)) == _ffi.E_ARG
    r, state = path.disturbances_read()
    assert same(r, rows) and np.all(state[:, 3] == 2)
    assert same(path.plant_params_read(), prow) and same(path.tyre_params_read(), tyres)
    close(path, tt, plan)
