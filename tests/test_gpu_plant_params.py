"""GPU: per-vehicle plant parameters (lpvmpc_plant_step_vehicles_batch, lpvmpc_cl_init_vehicles, lpvmpc_race_init_vehicles,
lpvmpc_plant_params_read).  The device plant with a row per vehicle matches the reference simulator's own loop (fixture) and the
host restatement with other tyre stiffnesses; nominal rows give the _actuated and plain entry points' words; vehicles with
different rows are independent of each other; mismatched fleets and races match the host replay (tests/_plant_params_ref.py)
under the bars of the delayed fleets' tests; read-back, refusals and lifetime."""
import os

import numpy as np
import pytest

from tests import _plant_params_ref as P
from tests import _race_observer_ref as RO
from tests.test_gpu_delayed_fleets import STD, close, ctrl, engines, lshape, obs_cfg, same

pytestmark = pytest.mark.gpu

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plant_params", "plant_params.npz")
NOM = np.array([0.125, 0.125, 1.98, 0.03, 60.0, 60.0, 0.05])
RACE_KEYS = ("plant", "local", "cmd", "phase", "lap", "iters", "status")
PLAN_KEYS = ("plan_iters", "plan_status")        # the planner handle's report: written for a vehicle from its first planner tick on


def chunks(K, hold):
    out, k, h = [], 0, 0
    while k < K:
        n = int(hold[h % 3]); out.append((k, min(k + n, K))); k += n; h += 1
    return [(0, 1), (1, out[0][1])] + out[1:]


@pytest.mark.parametrize("lld", [0, 1])
def test_plant_step_vehicles_matches_the_reference_loop(lld):
    """The fixture's cases of one lowLevelDyn setting in one batch, each with its own row and delays: one call per held command
    matches the reference's states to 1e-11 after every call; per-step calls give the same words (the trace split over calls)."""
    import lpvmpc
    fx = np.load(FIX)
    cases = np.nonzero(fx["lld"] == lld)[0]
    B, K = len(cases), fx["cmd"].shape[1]
    cfg = lpvmpc.actuator_config(low_level_dyn=bool(lld))
    La, Ld, rows = fx["La"][cases], fx["Ld"][cases], fx["params"][cases]
    e = ctrl(lshape())
    st, act = np.tile(fx["plant0"], (B, 1)), None
    st1, act1 = st.copy(), None
    worst = 0.0
    for a, b in chunks(K, fx["hold"]):
        u = fx["cmd"][cases, a]
        st, act = e.plant_step_vehicles(st, u, rows, act, n_sub=b - a, actuator=cfg, delay_a=La, delay_df=Ld)
        worst = max(worst, float(np.max(np.abs(st - fx["state"][cases, b - 1]))))
        for _ in range(a, b):
            st1, act1 = e.plant_step_vehicles(st1, u, rows, act1, n_sub=1, actuator=cfg, delay_a=La, delay_df=Ld)
    print("lld %d: max |device - reference| = %.3e over %d steps, %d vehicles" % (lld, worst, K, B))
    assert worst <= 1e-11
    assert same(st, st1) and same(act, act1)
    e.close()


def test_tyre_stiffness_and_nominal_rows():
    """Rows with Cf, Cr != 60 (and the fixture's other words) match the host restatement to 1e-11; the nominal row (explicit or
    NULL) equals lpvmpc_plant_step_actuated_batch and, all off, lpvmpc_plant_step_batch word for word."""
    import lpvmpc
    fx = np.load(FIX)
    rng = np.random.default_rng(4)
    B, K = 12, 200
    rows = np.tile(NOM, (B, 1)) * rng.uniform(0.7, 1.3, (B, 7))
    cmd = np.repeat(rng.uniform([-0.5, -0.3], [1.5, 0.3], (K // 5, B, 2)), 5, axis=0)
    e = ctrl(lshape())
    st, act = np.tile(fx["plant0"], (B, 1)), None
    for k in range(0, K, 5):
        st, act = e.plant_step_vehicles(st, cmd[k], rows, act, n_sub=5)
    worst = max(float(np.max(np.abs(st[b] - P.simulate(fx["plant0"], cmd[:, b], rows[b])[0][-1]))) for b in range(B))
    print("Cf / Cr rows: max |device - restatement| = %.3e" % worst)
    assert worst <= 1e-11
    st0 = np.tile(fx["plant0"], (B, 1)); st0[:, 2] = rng.uniform(0.5, 2.0, B); st0[:, 7] = rng.normal(0, 0.3, B)
    cfg = lpvmpc.actuator_config(0.02, 0.03, low_level_dyn=True)
    a = e.plant_step_actuated(st0, None, cmd[0], n_sub=9, mu_sim=0.07, actuator=cfg)
    b = e.plant_step_vehicles(st0, cmd[0], None, None, n_sub=9, mu_sim=0.07, actuator=cfg)
    c = e.plant_step_vehicles(st0, cmd[0], lpvmpc.plant_params(B, e, mu_sim=0.07), None, n_sub=9, mu_sim=0.3, actuator=cfg)
    assert same(a[0], b[0]) and same(a[1], b[1]) and same(a[0], c[0]) and same(a[1], c[1])
    d = e.plant_step(st0, cmd[0], n_sub=9)
    assert same(d, e.plant_step_vehicles(st0, cmd[0], None, None, n_sub=9)[0])
    e.close()


def cl_run(mp, plant0, T, est=None, **kw):
    e = ctrl(mp)
    if est is not None:
        e.observer_setup(est)
    e.cl_init(plant0, mp.halfWidth, mp.slack, q9_swap=True, n_sub=7, **kw)
    out = []
    for _ in range(T):
        e.cl_tick(1)
        o = e.cl_read()
        if est is not None:
            o["est"], o["meas"] = e.observer_read()
        if kw.get("actuator") is not None or kw.get("plant_params") is not None:
            o.update(e.actuator_read())
        out.append(o)
    if kw.get("plant_params") is not None:
        out.append(e.plant_params_read())
    e.close()
    return out


@pytest.mark.parametrize("est", [False, True])
def test_nominal_rows_are_the_old_lap0_fleet(est):
    """Over 60 ticks: plant_params NULL and the explicit nominal rows equal cl_init(actuator=all off) and cl_init, word for word."""
    import lpvmpc
    mp = lshape()
    B, T = 48, 60
    plant0 = RO.grid_fleet(B, 3)
    oc = obs_cfg(**dict(STD, seed=5)) if est else None
    old = cl_run(mp, plant0, T, est=oc)
    act = cl_run(mp, plant0, T, est=oc, actuator=lpvmpc.actuator_config())
    nul = cl_run(mp, plant0, T, est=oc, plant_params="nominal")
    exp = cl_run(mp, plant0, T, est=oc, plant_params=np.tile(NOM, (B, 1)), mu_sim=0.9)      # mu_sim ignored with rows
    assert same(nul[T], np.tile(NOM, (B, 1))) and same(exp[T], np.tile(NOM, (B, 1)))
    for t in range(T):
        for k in ("plant", "local", "cmd", "iters", "status") + (("est", "meas") if est else ()):
            assert same(old[t][k], act[t][k]) and same(act[t][k], nul[t][k]) and same(act[t][k], exp[t][k]), (t, k)
        for k in ("act_state", "path"):
            assert same(act[t][k], nul[t][k]) and same(act[t][k], exp[t][k]), (t, k)


def race_run(mp, plant0, T, d=0, record=False, **kw):
    path, tt, plan = engines(mp, d)
    path.race_init(tt, plan, plant0, laps=2, half_width=mp.halfWidth, slack=mp.slack, **kw)
    rows = []
    for _ in range(T):
        path.race_tick(1)
        o = path.race_read()
        if kw.get("estimator") is not None:
            o["est"], o["meas"] = path.observer_read()
        if kw.get("actuator") is not None or kw.get("plant_params") is not None:
            o.update(path.actuator_read())
        rows.append(o)
    last = dict(zip(("path_uPred", "tt_uPred"), path.race_predictions()))
    last.update(zip(("lap_step", "alive"), path.race_laps()))
    if kw.get("plant_params") is not None:
        last["rows"] = path.plant_params_read()
    rows.append(last)
    close(path, tt, plan)
    return rows


def _race_same(a, b, T, keys, vehicles=None):
    v = slice(None) if vehicles is None else vehicles
    ev = np.full(len(a[0]["phase"]), T)
    for t in range(T):
        for k in keys:
            if k in a[t] and k in b[t]:
                assert same(np.asarray(a[t][k])[v], np.asarray(b[t][k])[v]), (t, k)
        ev = np.where((ev == T) & (a[t]["phase"] >= 1), t, ev)
        run = (ev < t) if vehicles is None else (ev < t) & vehicles          # the planner has run for these vehicles
        for k in PLAN_KEYS:
            assert same(a[t][k][run], b[t][k][run]), (t, k)
    for k in ("path_uPred", "tt_uPred", "lap_step", "alive"):
        assert same(np.asarray(a[T][k])[v], np.asarray(b[T][k])[v]), k


@pytest.mark.parametrize("case", ["ground", "estimator", "delayed"])
def test_nominal_rows_are_the_old_race(case):
    """Over 90 ticks of a staggered race (ground truth; the noisy estimator; La / Ld 4 / 6 steps with the servo lag and steeringDelay
    3): plant_params NULL and the explicit nominal rows equal race_init_actuated and, all off, race_init / race_init_observed, in
    every output the reads return."""
    import lpvmpc
    mp = lshape()
    B, T = 24, 90
    plant0 = RO.start_line_fleet(mp.PointAndTangent, B, 7)
    kw = dict(half_track0=1)
    d = 3 if case == "delayed" else 0
    if case == "estimator":
        kw["estimator"] = obs_cfg(**dict(STD, seed=9))
    act = lpvmpc.actuator_config(0.02, 0.03, low_level_dyn=True) if case == "delayed" else lpvmpc.actuator_config()
    a = race_run(mp, plant0, T, d, actuator=act, **kw)
    b = race_run(mp, plant0, T, d, actuator=act, plant_params="nominal", **kw)
    c = race_run(mp, plant0, T, d, actuator=act, plant_params=np.tile(NOM, (B, 1)), mu_sim=0.2, **kw)
    keys = RACE_KEYS + ("est", "meas", "act_state", "path", "tt")
    _race_same(a, b, T, keys); _race_same(a, c, T, keys)
    assert same(b[T]["rows"], np.tile(NOM, (B, 1))) and same(c[T]["rows"], np.tile(NOM, (B, 1)))
    if case != "delayed":
        o = race_run(mp, plant0, T, **kw)
        n = race_run(mp, plant0, T, plant_params="nominal", **kw)           # act NULL: all off
        _race_same(o, a, T, RACE_KEYS + ("est", "meas")); _race_same(o, n, T, RACE_KEYS + ("est", "meas"))
    assert np.any(a[T - 1]["phase"] >= 1)


def _rows_k(B, K, seed):
    uni = np.array(lpvmpc_sample(K, seed))
    return uni, uni[np.arange(B) % K]


def lpvmpc_sample(K, seed):
    import lpvmpc
    s = lpvmpc.sample_plant_params(K, seed)
    s[0] = NOM                                                              # one of them the nominal car
    return s


def test_distinct_rows_equal_uniform_fleets():
    """A lap-0 fleet whose vehicles carry K = 4 interleaved rows equals, vehicle for vehicle and bit for bit, the K fleets run with
    one row each (with the estimator and delays)."""
    import lpvmpc
    mp = lshape()
    B, T, K = 16, 40, 4
    plant0 = RO.grid_fleet(B, 8)
    uni, mixed = _rows_k(B, K, 21)
    kw = dict(est=obs_cfg(**dict(STD, seed=2)), actuator=lpvmpc.actuator_config(0.01, 0.02, low_level_dyn=True))
    m = cl_run(mp, plant0, T, plant_params=mixed, **kw)
    assert same(m[T], mixed)
    for k in range(K):
        u = cl_run(mp, plant0, T, plant_params=np.tile(uni[k], (B, 1)), **kw)
        v = np.arange(B) % K == k
        for t in range(T):
            for key in ("plant", "local", "cmd", "iters", "status", "est", "act_state"):
                assert same(m[t][key][v], u[t][key][v]), (k, t, key)


def test_distinct_rows_equal_uniform_races_and_shards():
    """A race of 24 vehicles with K = 3 interleaved rows (the estimator in the loop) equals the 3 uniform races vehicle for vehicle
    over 300 ticks with lap events spread out; the race run as two vehicle_offset halves, each with its rows, equals the whole."""
    mp = lshape()
    B, T, K = 24, 300, 3
    plant0 = RO.start_line_fleet(mp.PointAndTangent, B, 13, 0.6, 0.97)
    uni, mixed = _rows_k(B, K, 5)
    kw = dict(half_track0=1)
    whole = race_run(mp, plant0, T, plant_params=mixed, estimator=obs_cfg(**dict(STD, seed=4)), **kw)
    ev = [int(np.argmax([r["phase"][v] >= 1 for r in whole[:T]])) for v in range(B)]
    assert len(set(ev)) >= 4, ev
    for k in range(K):
        u = race_run(mp, plant0, T, plant_params=np.tile(uni[k], (B, 1)), estimator=obs_cfg(**dict(STD, seed=4)), **kw)
        _race_same(whole, u, T, ("plant", "local", "cmd", "phase", "lap", "iters", "status", "est"), np.arange(B) % K == k)
    h = B // 2
    lo = race_run(mp, plant0[:h], T, plant_params=mixed[:h], estimator=obs_cfg(vehicle_offset=0, **dict(STD, seed=4)), half_track0=1)
    hi = race_run(mp, plant0[h:], T, plant_params=mixed[h:], estimator=obs_cfg(vehicle_offset=h, **dict(STD, seed=4)), half_track0=1)
    for t in range(T):
        for key in ("plant", "local", "cmd", "phase", "lap", "iters", "status", "est"):
            assert same(whole[t][key], np.concatenate([lo[t][key], hi[t][key]])), (t, key)


@pytest.mark.parametrize("d,lld,est", [(0, False, False), (3, True, True)])
def test_mismatched_lap0_fleet_matches_the_replay(d, lld, est):
    """Rows from sample_plant_params over 40 ticks (all off with steeringDelay 0; La = 6 / Ld = 4 with the servo lag, steeringDelay 3
    and the estimator): plant, measurement and command within 2e-6 of the host replay, identical iteration counts and statuses."""
    import lpvmpc
    mp = lshape()
    B, T = 16, 40
    plant0 = RO.grid_fleet(B, 21)
    rows = lpvmpc.sample_plant_params(B, 17)
    oc = obs_cfg(**dict(STD, seed=3)) if est else None
    act = lpvmpc.actuator_config(0.03, 0.02, low_level_dyn=lld) if d else None
    e = ctrl(mp, "path", d)
    if oc is not None:
        e.observer_setup(oc)
    e.cl_init(plant0, mp.halfWidth, mp.slack, q9_swap=True, n_sub=7, actuator=act, plant_params=rows)
    ref = P.vehicle_lap0_replay(mp.PointAndTangent, plant0, plant_params=rows, steering_delay=d, delay_a=6 if d else 0, delay_df=4 if d else 0,
                                low_level_dyn=lld, laps=1, half_width=mp.halfWidth, slack=mp.slack,
                                **(dict(gains=RO.estimator_gains(), stds=(0.01, 0.05, 0.01, 0.01, 0.02), seed=3) if est else {}))
    worst = 0.0
    for t in range(T):
        e.cl_tick(1); ref.tick()
        o = e.cl_read()
        assert np.all(ref.phase == 0), t
        assert np.array_equal(o["iters"], ref.iters) and np.array_equal(o["status"], ref.status), t
        worst = max(worst, *(float(np.max(np.abs(o[k] - v))) for k, v in (("plant", ref.plant), ("local", ref.local), ("cmd", ref.cmd))))
        if est:
            worst = max(worst, float(np.max(np.abs(e.observer_read()[0] - ref.estimate()))))
    # the rows matter: the nominal replay is far from this fleet
    nom = P.vehicle_lap0_replay(mp.PointAndTangent, plant0, laps=1, half_width=mp.halfWidth, slack=mp.slack, steering_delay=d,
                                delay_a=6 if d else 0, delay_df=4 if d else 0, low_level_dyn=lld,
                                **(dict(gains=RO.estimator_gains(), stds=(0.01, 0.05, 0.01, 0.01, 0.02), seed=3) if est else {}))
    for _ in range(T):
        nom.tick()
    print("mismatched lap-0 fleet d %d est %d: vs replay %.2e over %d ticks; nominal replay differs by %.3g" % (d, est, worst, T,
                                                                                                          np.max(np.abs(nom.plant - ref.plant))))
    assert worst <= 2e-6
    assert np.max(np.abs(nom.plant - ref.plant)) > 1e-3
    e.close()


@pytest.mark.parametrize("est", [False, True])
def test_mismatched_race_matches_the_replay(est):
    """12 vehicles with sampled rows and staggered lap events (La = 4 / Ld = 6 with the servo lag, steeringDelay 3 on path and tt
    when the estimator runs; all off on ground truth) against the host replay: lap 0 within 2e-6 for the vehicles that reach their
    event, the same event ticks, the same vehicles lost on the same ticks, and in each survivor's first 24 racing ticks the bars of
    the delayed race's test (two thirds within 1e-5 / 1e-4, all within 2e-2, >= 95 % equal iteration counts, equal statuses)."""
    import lpvmpc
    mp = lshape()
    B, W_ = 12, 24
    d = 3 if est else 0
    plant0 = RO.start_line_fleet(mp.PointAndTangent, B, 17, 0.85, 0.97)
    # (seed 23 with the delays and the estimator drives a vehicle whose racing roll-out leaves the track table: the host oracle raises
    # there, oracle/lpv_ref.py, where the device reports UNSOLVED -- not a replay it can make)
    rows = lpvmpc.sample_plant_params(B, 29 if est else 23)
    stds = (0.01, 0.05, 0.01, 0.01, 0.02)
    path, tt, plan = engines(mp, d)
    path.race_init(tt, plan, plant0, half_track0=1, laps=3, half_width=mp.halfWidth, slack=mp.slack, plant_params=rows,
                   estimator=obs_cfg(**dict(STD, seed=5)) if est else None,
                   actuator=lpvmpc.actuator_config(0.02, 0.03, low_level_dyn=True) if est else None)
    ref = P.VehicleRaceRef(mp.PointAndTangent, plant0, plant_params=rows, steering_delay=d, delay_a=4 if est else 0, delay_df=6 if est else 0,
                           low_level_dyn=est, half_track0=1, laps=3, half_width=mp.halfWidth, slack=mp.slack,
                           **(dict(gains=RO.estimator_gains(), stds=stds, seed=5) if est else {}))
    racing = np.zeros(B, int)
    ev_dev = np.full(B, -1)
    w_state = np.zeros(B); w_cmd = np.zeros(B); same_it = n_it = 0
    lost_dev, lost_ref, st_diff = {}, {}, []
    err0 = np.zeros(B)
    t = 0
    while np.any(racing < W_) and t < 200:
        ph_before = ref.phase.copy()
        path.race_tick(1); ref.tick()
        o = path.race_read()
        e_dev, e_ref = (path.observer_read()[0], ref.estimate()) if est else (o["plant"], ref.plant)
        ev_dev[(ev_dev < 0) & (o["phase"] == 1)] = t
        lap0 = (o["phase"] == 0) & (ref.phase == 0)
        assert np.array_equal(o["phase"] == 0, ref.phase == 0), t
        lost0 = (ph_before == 0) & (o["phase"] == 3)
        assert np.array_equal(lost0, (ph_before == 0) & (ref.phase == 3)), t
        if np.any(lap0):
            for a_, b_ in ((o["plant"], ref.plant), (e_dev, e_ref), (o["local"], ref.local), (o["cmd"], ref.cmd)):
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
            w_state[v] = max(w_state[v], float(np.max(np.abs(o["plant"][v] - ref.plant[v]))), float(np.max(np.abs(e_dev[v] - e_ref[v]))),
                             float(np.max(np.abs(o["local"][v] - ref.local[v]))))
            w_cmd[v] = max(w_cmd[v], float(np.max(np.abs(o["cmd"][v] - ref.cmd[v]))))
            if o["status"][v] != ref.status[v]:
                st_diff.append((t, int(v), int(o["status"][v]), int(ref.status[v])))
            same_it += int(o["iters"][v] == ref.iters[v]); n_it += 1
        racing[w] += 1
        done = (racing >= W_) | (ref.phase >= 2) | (o["phase"] >= 2)
        racing[done] = W_
        ref.phase[done] = np.maximum(ref.phase[done], 2)
        t += 1
    surv = np.array([v not in lost_dev for v in range(B)])
    strict = surv & (w_state <= 1e-5) & (w_cmd <= 1e-4)
    kept = np.array([ref.phase[v] != 3 or ref.event_tick[v] >= 0 for v in range(B)])
    print("mismatched race vs replay (estimator %s): %d ticks, events %s, lap 0 worst %.3g, survivors within 1e-5 / 1e-4: %d of %d, "
          "worst survivor %.3g / %.3g, lost %s, iterations %d / %d" % (est, t, sorted(ref.event_tick.tolist()), err0[kept].max(), strict.sum(),
                                                                      surv.sum(), w_state[surv].max(), w_cmd[surv].max(), lost_dev, same_it, n_it))
    assert np.all((racing >= W_) | (ev_dev < 0)) and n_it > 0 and np.sum(ev_dev >= 0) >= 8
    assert np.array_equal(ev_dev, ref.event_tick) and len(set(ev_dev[ev_dev >= 0].tolist())) >= 4
    assert kept.sum() >= 8 and np.all(err0[kept] <= 2e-6)
    assert lost_dev == lost_ref
    assert not st_diff, st_diff
    assert same_it >= 0.95 * n_it
    assert strict.sum() >= 2 * surv.sum() // 3
    assert np.all(w_state[surv] <= 2e-2) and np.all(w_cmd[surv] <= 2e-2)
    close(path, tt, plan)


def test_read_back_refusals_and_lifetime():
    """plant_params_read returns the rows given; each refusal gives LPVMPC_E_ARG and leaves the handle usable (a fleet it ran keeps
    running); after cl_release a plain cl_init equals a fresh handle's fleet; a read without a per-vehicle fleet is refused."""
    import ctypes as C
    import lpvmpc
    from lpvmpc import _ffi
    mp = lshape()
    B = 8
    plant0 = RO.grid_fleet(B, 2)
    rows = lpvmpc.sample_plant_params(B, 3)
    e = ctrl(mp)
    with pytest.raises(lpvmpc.LpvMpcError):
        e.plant_params_read()                                                 # no fleet
    e.cl_init(plant0, mp.halfWidth, mp.slack, plant_params=rows)
    assert same(e.plant_params_read(), rows)
    e.cl_tick(3)
    before = e.cl_read()
    lib, p0 = e._lib, np.ascontiguousarray(plant0)
    for b, i, v in ((0, 0, np.nan), (1, 2, 0.0), (2, 3, -0.01), (3, 4, -1.0), (4, 6, -1e-3), (5, 1, np.inf)):
        bad = rows.copy(); bad[b, i] = v
        rc = lib.lpvmpc_cl_init_vehicles(e._h, B, _ffi.ptr(p0), mp.halfWidth, mp.slack, 1, 7, 0.005, 0.05, None, None, None, _ffi.ptr(bad))
        assert rc == _ffi.E_ARG, (b, i, v)
        st = np.tile(plant0[:1], (B, 1)); act = np.zeros((B, _ffi.ACT_WORDS)); u = np.zeros((B, 2))
        e2 = ctrl(mp)
        rc = e2._lib.lpvmpc_plant_step_vehicles_batch(e2._h, B, _ffi.ptr(st), _ffi.ptr(act), _ffi.ptr(u), 1, 0.005, 0.05, None, None, None,
                                                     _ffi.ptr(bad))
        assert rc == _ffi.E_ARG, (b, i, v)
        e2.close()
    bad_cfg = lpvmpc.actuator_config(); bad_cfg.delay_a = 65
    rc = lib.lpvmpc_cl_init_vehicles(e._h, B, _ffi.ptr(p0), mp.halfWidth, mp.slack, 1, 7, 0.005, 0.05, C.byref(bad_cfg), None, None, _ffi.ptr(rows))
    assert rc == _ffi.E_ARG
    assert same(e.plant_params_read(), rows)                                  # the refused calls started nothing: the fleet runs on
    e.cl_tick(1)
    assert not same(e.cl_read()["plant"], before["plant"])
    with pytest.raises(ValueError):
        e.cl_init(plant0, mp.halfWidth, mp.slack, plant_params=rows[:4])
    e.cl_release()
    with pytest.raises(lpvmpc.LpvMpcError):
        e.plant_params_read()
    e.cl_init(plant0, mp.halfWidth, mp.slack)
    e.cl_tick(20)
    a = e.cl_read()
    f = ctrl(mp)
    f.cl_init(plant0, mp.halfWidth, mp.slack)
    f.cl_tick(20)
    b = f.cl_read()
    for k in ("plant", "local", "cmd", "iters", "status"):
        assert same(a[k], b[k]), k
    close(e, f)
    # the race: rows read back from the path handle; refused rows start nothing
    path, tt, plan = engines(mp)
    cfg = _ffi.default_race_config()
    bad = rows.copy(); bad[0, 2] = -1.0
    rc = path._lib.lpvmpc_race_init_vehicles(path._h, tt._h, plan._h, B, _ffi.ptr(p0), None, C.byref(cfg), None, None, None, None, _ffi.ptr(bad))
    assert rc == _ffi.E_ARG
    path.race_init(tt, plan, plant0, plant_params=rows, half_width=mp.halfWidth, slack=mp.slack)
    assert same(path.plant_params_read(), rows)
    path.race_tick(5)
    close(path, tt, plan)
