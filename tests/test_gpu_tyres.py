"""GPU: the tyre model (lpvmpc_plant_step_tyres_batch, lpvmpc_cl_init_tyres, lpvmpc_race_init_tyres, lpvmpc_tyre_params_read,
lpvmpc_tyre_force_batch).  The device curve and the device plant with a tyre row per vehicle match the fixture made with the
reference's own Simulator.pacejka; kind 0 rows give the _vehicles entry points' words; vehicles with different tyre rows are
independent of each other; Pacejka fleets and races match the host replay (tests/_tyre_ref.py) under the bars of the per-vehicle
fleets' tests; read-back, refusals, threads and a large fleet."""
import os
import threading

import numpy as np
import pytest

from tests import _race_observer_ref as RO
from tests import _tyre_ref as T
from tests.test_gpu_delayed_fleets import STD, close, ctrl, engines, lshape, obs_cfg, same
from tests.test_gpu_plant_params import NOM, RACE_KEYS, _race_same

pytestmark = pytest.mark.gpu

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tyre", "tyre.npz")
RACE_SEED = 17             # start states of test_pacejka_race_matches_the_replay


def test_tyre_force_is_the_reference_curve():
    """lpvmpc_tyre_force_batch at the fixture's 257 angles, every parameter set, in batches of at most 64 (the last one a single
    angle): within 1e-11 of the reference's Simulator.pacejka; a kind 0 row gives 60 * alpha."""
    fx = np.load(FIX)
    e = ctrl(lshape())
    al = fx["curve_alpha"]
    worst = 0.0
    for (m, B, C, cf), f in zip(fx["curve_sets"], fx["curve_force"]):
        out = np.concatenate([e.tyre_force(np.tile([1.0, B, C, cf], (len(al[k:k + 64]), 1)), m, al[k:k + 64]) for k in range(0, len(al), 64)])
        worst = max(worst, float(np.max(np.abs(out - f))))
    print("tyre curve: max |device - reference| = %.3e N over %d sets x %d angles" % (worst, len(fx["curve_sets"]), len(al)))
    assert worst <= 1e-11
    # one batch mixing the sets, masses and a linear row
    rows = np.array([[1.0] + list(s[1:]) for s in fx["curve_sets"]] + [[0.0, 6.0, 1.6, 0.8]])
    out = e.tyre_force(rows, np.append(fx["curve_sets"][:, 0], 1.98), np.full(len(rows), al[200]))
    assert np.max(np.abs(out[:-1] - fx["curve_force"][:, 200])) <= 1e-11 and out[-1] == 60 * al[200]
    e.close()


def _runs(cmd):
    """[(a, b)]: maximal step ranges over which no vehicle's command changes; cmd [cases, K, 2]."""
    K = cmd.shape[1]
    cut = [0] + [k for k in range(1, K) if not np.array_equal(cmd[:, k], cmd[:, k - 1])] + [K]
    return list(zip(cut[:-1], cut[1:]))


@pytest.mark.parametrize("lld", [0, 1])
def test_plant_step_tyres_matches_the_fixture_trajectories(lld):
    """The fixture's cases of one lowLevelDyn setting in one batch, each with its plant row, tyre row and delays, one call per run of
    held commands: within 1e-11 of the fixture's states after every call (the bar tests/test_gpu_plant_params.py holds for this
    kernel over the same 300 steps)."""
    import lpvmpc
    fx = np.load(FIX)
    cases = np.nonzero(fx["lld"] == lld)[0]
    B = len(cases)
    cfg = lpvmpc.actuator_config(low_level_dyn=bool(lld))
    La, Ld, rows, tyres = fx["La"][cases], fx["Ld"][cases], fx["params"][cases], fx["tyre"][cases]
    e = ctrl(lshape())
    st, act = np.tile(fx["plant0"], (B, 1)), None
    worst = np.zeros(B)
    for a, b in _runs(fx["cmd"][cases]):
        st, act = e.plant_step_vehicles(st, fx["cmd"][cases, a], rows, act, n_sub=b - a, actuator=cfg, delay_a=La, delay_df=Ld, tyre_params=tyres)
        worst = np.maximum(worst, np.max(np.abs(st - fx["state"][cases, b - 1]), axis=1))
    for c, w in zip(cases, worst):
        print("case %d (kind %d, max |alpha| %.3f): max |device - fixture| = %.3e over 300 steps" % (c, fx["tyre"][c, 0], np.max(np.abs(fx["slip"][c])), w))
    assert np.all(worst <= 1e-11)
    e.close()


def test_one_call_equals_split_calls():
    """300 steps under one held command in one call equal the same steps in calls of 7 / 7 / 6, word for word (state and actuator)."""
    import lpvmpc
    B = 33
    rng = np.random.default_rng(8)
    rows, tyres = lpvmpc.sample_plant_params(B, 4), lpvmpc.sample_tyre_params(B, 4, kind=(np.arange(B) % 3 > 0).astype(float))
    st0 = np.tile(np.load(FIX)["plant0"], (B, 1)); st0[:, 2] = rng.uniform(0.3, 1.5, B)
    u = np.column_stack([rng.uniform(0.5, 1.5, B), rng.choice([-0.4, 0.4], B)])
    cfg = lpvmpc.actuator_config(0.02, 0.035, low_level_dyn=True)
    e = ctrl(lshape())
    one = e.plant_step_vehicles(st0, u, rows, None, n_sub=300, actuator=cfg, tyre_params=tyres)
    st, act, k = st0, None, 0
    while k < 300:
        for n in (7, 7, 6):
            st, act = e.plant_step_vehicles(st, u, rows, act, n_sub=n, actuator=cfg, tyre_params=tyres)
            k += n
    assert k == 300 and same(one[0], st) and same(one[1], act) and np.all(np.isfinite(st))
    e.close()


def test_kind0_rows_are_the_per_vehicle_step():
    """tyre_params NULL and explicit kind 0 rows (with other B, C, c_f) equal lpvmpc_plant_step_vehicles_batch word for word."""
    import lpvmpc
    B = 37
    rng = np.random.default_rng(2)
    rows = lpvmpc.sample_plant_params(B, 9)
    st0 = np.tile(np.load(FIX)["plant0"], (B, 1)); st0[:, 2] = rng.uniform(0.1, 2.0, B); st0[:, 7] = rng.normal(0, 0.5, B)
    u = np.column_stack([rng.uniform(-0.5, 1.5, B), rng.uniform(-0.4, 0.4, B)])
    cfg = lpvmpc.actuator_config(0.02, 0.03, low_level_dyn=True)
    e = ctrl(lshape())
    a = e.plant_step_vehicles(st0, u, rows, None, n_sub=40, actuator=cfg)
    b = e.plant_step_vehicles(st0, u, rows, None, n_sub=40, actuator=cfg, tyre_params="linear")
    c = e.plant_step_vehicles(st0, u, rows, None, n_sub=40, actuator=cfg, tyre_params=lpvmpc.sample_tyre_params(B, 3, kind=0))
    d = e.plant_step_vehicles(st0, u, rows, None, n_sub=40, actuator=cfg, tyre_params="pacejka")
    assert same(a[0], b[0]) and same(a[1], b[1]) and same(a[0], c[0]) and same(a[1], c[1])
    assert not same(a[0], d[0]) and same(a[1], d[1])                                            # the tyre reaches the plant, not the actuator
    e.close()


def cl_run(mp, plant0, T, est=None, d=0, **kw):
    e = ctrl(mp, "path", d)
    if est is not None:
        e.observer_setup(est)
    e.cl_init(plant0, mp.halfWidth, mp.slack, q9_swap=True, n_sub=7, **kw)
    out = []
    for _ in range(T):
        e.cl_tick(1)
        o = e.cl_read()
        if est is not None:
            o["est"], o["meas"] = e.observer_read()
        o.update(e.actuator_read())
        out.append(o)
    out.append(e.tyre_params_read() if kw.get("tyre_params") is not None else None)
    e.close()
    return out


CL_KEYS = ("plant", "local", "cmd", "iters", "status", "act_state", "path")


@pytest.mark.parametrize("est", [False, True])
def test_kind0_rows_are_the_per_vehicle_lap0_fleet(est):
    """Over 60 ticks: tyre_params NULL and explicit kind 0 rows equal cl_init(plant_params=rows), word for word."""
    import lpvmpc
    mp = lshape()
    B, T = 48, 60
    plant0 = RO.grid_fleet(B, 3)
    rows = lpvmpc.sample_plant_params(B, 5)
    oc = obs_cfg(**dict(STD, seed=5)) if est else None
    veh = cl_run(mp, plant0, T, est=oc, plant_params=rows)
    nul = cl_run(mp, plant0, T, est=oc, plant_params=rows, tyre_params="linear")
    exp = cl_run(mp, plant0, T, est=oc, plant_params=rows, tyre_params=lpvmpc.tyre_params(B, kind=0, c_f=0.3))
    assert same(nul[T], np.zeros((B, 4))) and same(exp[T], lpvmpc.tyre_params(B, kind=0, c_f=0.3))
    for t in range(T):
        for k in CL_KEYS + (("est", "meas") if est else ()):
            assert same(veh[t][k], nul[t][k]) and same(veh[t][k], exp[t][k]), (t, k)


def race_run(mp, plant0, T, d=0, **kw):
    path, tt, plan = engines(mp, d)
    path.race_init(tt, plan, plant0, laps=2, half_width=mp.halfWidth, slack=mp.slack, **kw)
    rows = []
    for _ in range(T):
        path.race_tick(1)
        o = path.race_read()
        if kw.get("estimator") is not None:
            o["est"], o["meas"] = path.observer_read()
        o.update(path.actuator_read())
        rows.append(o)
    last = dict(zip(("path_uPred", "tt_uPred"), path.race_predictions()))
    last.update(zip(("lap_step", "alive"), path.race_laps()))
    if kw.get("tyre_params") is not None:
        last["tyres"] = path.tyre_params_read()
    rows.append(last)
    close(path, tt, plan)
    return rows


ALL_KEYS = RACE_KEYS + ("est", "meas", "act_state", "path", "tt")


@pytest.mark.parametrize("case", ["ground", "delayed"])
def test_kind0_rows_are_the_per_vehicle_race(case):
    """Over 90 ticks of a staggered race (ground truth; La / Ld 4 / 6 steps with the servo lag and steeringDelay 3): tyre_params
    NULL and explicit kind 0 rows equal race_init(plant_params=rows) in every output the reads return."""
    import lpvmpc
    mp = lshape()
    B, T = 24, 90
    plant0 = RO.start_line_fleet(mp.PointAndTangent, B, 7)
    d = 3 if case == "delayed" else 0
    kw = dict(half_track0=1, plant_params=np.tile(NOM, (B, 1)),
              actuator=lpvmpc.actuator_config(0.02, 0.03, low_level_dyn=True) if case == "delayed" else None)
    a = race_run(mp, plant0, T, d, **kw)
    b = race_run(mp, plant0, T, d, tyre_params="linear", **kw)
    c = race_run(mp, plant0, T, d, tyre_params=lpvmpc.tyre_params(B, kind=0), **kw)
    _race_same(a, b, T, ALL_KEYS); _race_same(a, c, T, ALL_KEYS)
    assert same(b[T]["tyres"], np.zeros((B, 4))) and same(c[T]["tyres"], lpvmpc.tyre_params(B, kind=0))
    assert np.any(a[T - 1]["phase"] >= 1)


def four_rows(B):
    """The linear row, the launch file's, a soft one and a sampled one, interleaved over B vehicles."""
    import lpvmpc
    uni = np.array([[0.0, 6.0, 1.6, 0.8], T.LAUNCH_FILE, T.SOFT, lpvmpc.sample_tyre_params(1, 31)[0]])
    return uni, uni[np.arange(B) % 4]


def test_interleaved_tyre_rows_equal_uniform_fleets():
    """A lap-0 fleet of 64 vehicles with four interleaved tyre rows equals, vehicle for vehicle and bit for bit over 120 ticks, the four
    fleets run with one row each (sampled plant rows, the estimator and delays)."""
    import lpvmpc
    mp = lshape()
    B, T_ = 64, 120
    plant0 = RO.grid_fleet(B, 8)
    uni, mixed = four_rows(B)
    kw = dict(est=obs_cfg(**dict(STD, seed=2)), actuator=lpvmpc.actuator_config(0.01, 0.02, low_level_dyn=True),
              plant_params=lpvmpc.sample_plant_params(B, 12))
    m = cl_run(mp, plant0, T_, tyre_params=mixed, **kw)
    assert same(m[T_], mixed)
    for k in range(4):
        u = cl_run(mp, plant0, T_, tyre_params=np.tile(uni[k], (B, 1)), **kw)
        v = np.arange(B) % 4 == k
        for t in range(T_):
            for key in CL_KEYS + ("est",):
                assert same(m[t][key][v], u[t][key][v]), (k, t, key)
    assert not same(m[T_ - 1]["plant"][0], m[T_ - 1]["plant"][1])


def test_interleaved_tyre_rows_equal_uniform_races_and_shards():
    """A race of 64 vehicles with the four interleaved tyre rows (the estimator in the loop) equals the four uniform races vehicle for
    vehicle over 120 ticks; the race run as two vehicle_offset halves, each with its rows, equals the whole."""
    mp = lshape()
    B, T_ = 64, 120
    plant0 = RO.start_line_fleet(mp.PointAndTangent, B, 13, 0.8, 0.97)
    uni, mixed = four_rows(B)
    keys = ("plant", "local", "cmd", "phase", "lap", "iters", "status", "est")
    whole = race_run(mp, plant0, T_, tyre_params=mixed, estimator=obs_cfg(**dict(STD, seed=4)), half_track0=1)
    assert same(whole[T_]["tyres"], mixed) and np.sum(whole[T_ - 1]["phase"] >= 1) >= 16
    for k in range(4):
        u = race_run(mp, plant0, T_, tyre_params=np.tile(uni[k], (B, 1)), estimator=obs_cfg(**dict(STD, seed=4)), half_track0=1)
        _race_same(whole, u, T_, keys, np.arange(B) % 4 == k)
    h = B // 2
    lo = race_run(mp, plant0[:h], T_, tyre_params=mixed[:h], estimator=obs_cfg(vehicle_offset=0, **dict(STD, seed=4)), half_track0=1)
    hi = race_run(mp, plant0[h:], T_, tyre_params=mixed[h:], estimator=obs_cfg(vehicle_offset=h, **dict(STD, seed=4)), half_track0=1)
    for t in range(T_):
        for key in keys:
            assert same(whole[t][key], np.concatenate([lo[t][key], hi[t][key]])), (t, key)


@pytest.mark.parametrize("d,lld,est", [(0, False, False), (3, True, True)])
def test_pacejka_lap0_fleet_matches_the_replay(d, lld, est):
    """An all-Pacejka fleet (sampled tyre and plant rows) over 40 ticks (all off with steeringDelay 0; La = 6 / Ld = 4 with the servo
    lag, steeringDelay 3 and the estimator): plant, measurement and command within 2e-6 of the host replay, identical iteration counts
    and statuses -- tests/test_gpu_plant_params.py's bars."""
    import lpvmpc
    mp = lshape()
    B, T_ = 16, 40
    plant0 = RO.grid_fleet(B, 21)
    plant0[:, 7] = np.where(np.arange(B) % 2, 0.5, -0.5)          # a yaw rate at the start: lateral forces from the first step on, in both cases
    rows, tyres = lpvmpc.sample_plant_params(B, 17), lpvmpc.sample_tyre_params(B, 17)
    oc = obs_cfg(**dict(STD, seed=3)) if est else None
    act = lpvmpc.actuator_config(0.03, 0.02, low_level_dyn=lld) if d else None
    e = ctrl(mp, "path", d)
    if oc is not None:
        e.observer_setup(oc)
    e.cl_init(plant0, mp.halfWidth, mp.slack, q9_swap=True, n_sub=7, actuator=act, plant_params=rows, tyre_params=tyres)
    rkw = dict(plant_params=rows, steering_delay=d, delay_a=6 if d else 0, delay_df=4 if d else 0, low_level_dyn=lld, half_track0=0, laps=1,
               half_width=mp.halfWidth, slack=mp.slack, **(dict(gains=RO.estimator_gains(), stds=(0.01, 0.05, 0.01, 0.01, 0.02), seed=3) if est else {}))
    ref = T.TyreRaceRef(mp.PointAndTangent, plant0, tyre_params=tyres, **rkw)
    lin = T.TyreRaceRef(mp.PointAndTangent, plant0, **rkw)
    worst = differs = 0.0
    for t in range(T_):
        e.cl_tick(1); ref.tick(); lin.tick()
        o = e.cl_read()
        differs = max(differs, float(np.max(np.abs(lin.plant - ref.plant))))
        assert np.all(ref.phase == 0), t
        assert np.array_equal(o["iters"], ref.iters) and np.array_equal(o["status"], ref.status), t
        worst = max(worst, *(float(np.max(np.abs(o[k] - v))) for k, v in (("plant", ref.plant), ("local", ref.local), ("cmd", ref.cmd))))
        if est:
            worst = max(worst, float(np.max(np.abs(e.observer_read()[0] - ref.estimate()))))
    print("Pacejka lap-0 fleet d %d est %d: vs replay %.2e over %d ticks; the linear replay differs by %.3g" % (d, est, worst, T_, differs))
    assert worst <= 2e-6
    assert differs > 1e-3                                                                   # the tyre matters to this fleet
    e.close()


def test_pacejka_race_matches_the_replay():
    """12 vehicles on the launch file's Pacejka tyre with sampled plant rows and staggered lap events, on ground truth, against the
    host replay: lap 0 within 2e-6 for the vehicles that reach their event, the same event ticks, the same vehicles lost on the same
    ticks, and in each survivor's first 24 racing ticks tests/test_gpu_race.py's bars (two thirds within 1e-5 / 1e-4, all within 2e-2,
    >= 95 % equal iteration counts, equal statuses).  Start states: the replay alone keeps at least 8 survivors (asserted on it)."""
    import lpvmpc
    mp = lshape()
    B, W_ = 12, 24
    plant0 = RO.start_line_fleet(mp.PointAndTangent, B, RACE_SEED, 0.90, 0.975)
    rows, tyres = lpvmpc.sample_plant_params(B, 23), lpvmpc.tyre_params(B)
    path, tt, plan = engines(mp)
    path.race_init(tt, plan, plant0, half_track0=1, laps=3, half_width=mp.halfWidth, slack=mp.slack, plant_params=rows, tyre_params=tyres)
    ref = T.TyreRaceRef(mp.PointAndTangent, plant0, tyre_params=tyres, plant_params=rows, half_track0=1, laps=3, half_width=mp.halfWidth,
                        slack=mp.slack)
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
    surv = np.array([v not in lost_dev for v in range(B)])
    surv_ref = np.array([v not in lost_ref and ref.event_tick[v] >= 0 for v in range(B)])
    strict = surv & (w_state <= 1e-5) & (w_cmd <= 1e-4)
    kept = np.array([ref.phase[v] != 3 or ref.event_tick[v] >= 0 for v in range(B)])
    print("Pacejka race vs replay: %d ticks, events %s, lap 0 worst %.3g, survivors within 1e-5 / 1e-4: %d of %d, worst survivor %.3g / %.3g, "
          "lost %s, iterations %d / %d" % (t, sorted(ref.event_tick.tolist()), err0[kept].max(), strict.sum(), surv.sum(), w_state[surv].max(),
                                           w_cmd[surv].max(), lost_dev, same_it, n_it))
    assert surv_ref.sum() >= 8                                                              # the replay alone, on the CPU
    assert np.all((racing >= W_) | (ev_dev < 0)) and n_it > 0 and np.sum(ev_dev >= 0) >= 8
    assert np.array_equal(ev_dev, ref.event_tick) and len(set(ev_dev[ev_dev >= 0].tolist())) >= 4
    assert kept.sum() >= 8 and np.all(err0[kept] <= 2e-6)
    assert lost_dev == lost_ref
    assert not st_diff, st_diff
    assert same_it >= 0.95 * n_it
    assert strict.sum() >= 2 * surv.sum() // 3
    assert np.all(w_state[surv] <= 2e-2) and np.all(w_cmd[surv] <= 2e-2)
    close(path, tt, plan)



def test_read_back_and_refusals_leave_a_running_fleet_untouched():
    """tyre_params_read returns the rows given; each refusal gives LPVMPC_E_ARG and the fleet it was tried on runs on, equal word for
    word to an undisturbed one; a read without a tyre fleet is refused; a race refuses and reads back alike."""
    import ctypes as C
    import lpvmpc
    from lpvmpc import _ffi
    mp = lshape()
    B = 8
    plant0 = RO.grid_fleet(B, 2)
    rows, tyres = lpvmpc.sample_plant_params(B, 3), lpvmpc.sample_tyre_params(B, 3, kind=[0, 1] * 4)
    e, f = ctrl(mp), ctrl(mp)
    with pytest.raises(lpvmpc.LpvMpcError):
        e.tyre_params_read()                                                  # no fleet
    for x in (e, f):
        x.cl_init(plant0, mp.halfWidth, mp.slack, plant_params=rows, tyre_params=tyres)
        x.cl_tick(3)
    assert same(e.tyre_params_read(), tyres) and same(e.plant_params_read(), rows)
    lib, p0 = e._lib, np.ascontiguousarray(plant0)
    for b, i, v in ((0, 0, 2.0), (1, 0, 0.5), (2, 0, -1.0), (3, 0, np.nan), (4, 1, np.nan), (5, 2, np.inf), (6, 3, -0.1), (7, 1, -1e-9)):
        bad = tyres.copy(); bad[b, i] = v
        rc = lib.lpvmpc_cl_init_tyres(e._h, B, _ffi.ptr(p0), mp.halfWidth, mp.slack, 1, 7, 0.005, 0.05, None, None, None, _ffi.ptr(rows), _ffi.ptr(bad))
        assert rc == _ffi.E_ARG, (b, i, v)
        st = np.tile(plant0[:1], (B, 1)); u = np.zeros((B, 2))
        e2 = ctrl(mp)
        rc = e2._lib.lpvmpc_plant_step_tyres_batch(e2._h, B, _ffi.ptr(st), None, _ffi.ptr(u), 1, 0.005, 0.05, None, None, None, _ffi.ptr(rows),
                                                  _ffi.ptr(bad))
        assert rc == _ffi.E_ARG, (b, i, v)
        m = np.full(B, 1.98)
        assert e2._lib.lpvmpc_tyre_force_batch(e2._h, B, _ffi.ptr(bad), _ffi.ptr(m), _ffi.ptr(u[:, 0].copy()), _ffi.ptr(np.empty(B))) == _ffi.E_ARG
        e2.close()
    badrow = rows.copy(); badrow[0, 2] = -1.0
    rc = lib.lpvmpc_cl_init_tyres(e._h, B, _ffi.ptr(p0), mp.halfWidth, mp.slack, 1, 7, 0.005, 0.05, None, None, None, _ffi.ptr(badrow), _ffi.ptr(tyres))
    assert rc == _ffi.E_ARG
    with pytest.raises(ValueError):
        e.cl_init(plant0, mp.halfWidth, mp.slack, tyre_params=tyres[:4])      # B of the wrong size
    with pytest.raises(lpvmpc.LpvMpcError):
        e.tyre_force("pacejka", 1.98, np.zeros(4))                            # a batch call on a handle that runs a fleet
    assert same(e.tyre_params_read(), tyres)
    e.cl_tick(5); f.cl_tick(5)
    a, b = e.cl_read(), f.cl_read()
    for k in ("plant", "local", "cmd", "iters", "status"):
        assert same(a[k], b[k]), k
    e.cl_release()
    with pytest.raises(lpvmpc.LpvMpcError):
        e.tyre_params_read()
    e.cl_init(plant0, mp.halfWidth, mp.slack, plant_params=rows)              # a _vehicles fleet has no tyre rows
    with pytest.raises(lpvmpc.LpvMpcError):
        e.tyre_params_read()
    close(e, f)
    path, tt, plan = engines(mp)
    cfg = _ffi.default_race_config()
    bad = tyres.copy(); bad[0, 0] = 3.0
    rc = path._lib.lpvmpc_race_init_tyres(path._h, tt._h, plan._h, B, _ffi.ptr(p0), None, C.byref(cfg), None, None, None, None, None, _ffi.ptr(bad))
    assert rc == _ffi.E_ARG
    path.race_init(tt, plan, plant0, tyre_params=tyres, half_width=mp.halfWidth, slack=mp.slack)
    assert same(path.tyre_params_read(), tyres) and same(path.plant_params_read(), np.tile(NOM, (B, 1)))
    path.race_tick(5)
    rc = path._lib.lpvmpc_race_init_tyres(path._h, tt._h, plan._h, B, _ffi.ptr(p0), None, C.byref(cfg), None, None, None, None, None, _ffi.ptr(bad))
    assert rc == _ffi.E_ARG and same(path.tyre_params_read(), tyres)
    close(path, tt, plan)


def test_two_handles_on_two_threads():
    """Two Pacejka fleets with different rows, each on its own handle and thread, equal the same fleets run one after the other."""
    import lpvmpc
    mp = lshape()
    B, T_ = 32, 30
    plant0 = RO.grid_fleet(B, 6)
    tyres = [lpvmpc.sample_tyre_params(B, s) for s in (1, 2)]
    serial = [cl_run(mp, plant0, T_, tyre_params=ty)[T_ - 1] for ty in tyres]
    out = [None, None]

    def work(i):
        out[i] = cl_run(mp, plant0, T_, tyre_params=tyres[i])[T_ - 1]

    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    for i in range(2):
        for k in CL_KEYS:
            assert same(out[i][k], serial[i][k]), (i, k)
    assert not same(serial[0]["plant"], serial[1]["plant"])


def test_large_sampled_fleet_stays_finite_or_lost():
    """8192 vehicles with sampled plant and tyre rows (every fourth one linear) over 30 race ticks: a vehicle's plant is finite or the
    vehicle is lost (on the tick after its plant diverged), and a lost vehicle stays lost."""
    import lpvmpc
    mp = lshape()
    B = 8192
    plant0 = RO.start_line_fleet(mp.PointAndTangent, B, 3, 0.9, 0.99)
    tyres = lpvmpc.sample_tyre_params(B, 7, kind=(np.arange(B) % 4 > 0).astype(float))
    path, tt, plan = engines(mp)
    path.race_init(tt, plan, plant0, half_track0=1, laps=1, half_width=mp.halfWidth, slack=mp.slack,
                   plant_params=lpvmpc.sample_plant_params(B, 7), tyre_params=tyres)
    lost = pending = np.zeros(B, bool)
    for block in range(7):                                                        # 30 ticks, and one more for the last tick's findings
        path.race_tick(5 if block < 6 else 1)
        o = path.race_read()
        fin = np.all(np.isfinite(o["plant"]), axis=1)
        now = o["phase"] == 3
        # (a vehicle whose plant diverges on a tick is lost on the next one, race_measure_kernel)
        assert np.all(now[pending]) and np.all(now[lost]) and not np.any(fin[now])
        lost, pending = now, ~fin & ~now
    assert np.sum(~lost) > B // 2 and np.any(o["phase"] == 1)
    assert same(path.tyre_params_read(), tyres)
    close(path, tt, plan)
