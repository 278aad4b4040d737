"""GPU: the per-vehicle state estimator (lpvmpc_set_observer_vehicles, lpvmpc_observer_vehicles_read,
lpvmpc_observer_step_vehicles_batch): each vehicle's observer step runs on its own model row and its own gain tables, in the
stand-alone step, in the lap-0 fleets of lpvmpc_cl_init_vehicles and in the races of lpvmpc_race_init_vehicles / _tyres.  Checked
against the numpy restatement (tests/_observer_design_ref.py) and the host replays of the per-vehicle fleets
(tests/_plant_params_ref.py) whose estimators are that restatement's."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from tests import _plant_params_ref as P
from tests import _race_observer_ref as RO
from tests.test_gpu_delayed_fleets import STD, close, ctrl, engines, lshape, obs_cfg, same

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _observer_design_ref as D  # noqa: E402

pytestmark = pytest.mark.gpu
B67 = 67                                   # more than one workgroup, not a multiple of the wavefront
STDS = (0.01, 0.05, 0.01, 0.01, 0.02)      # STD in the restatement's channel order


@pytest.fixture(scope="module")
def fx():
    f = D.fixture()
    f["idx"] = np.arange(B67) % 40
    f["rows67"] = np.ascontiguousarray(f["rows"][f["idx"]])
    f["g"] = RO.estimator_gains()
    return f


def design_of(f):
    return dict(lim_ls=f["lim_ls"], lim_hs=f["lim_hs"])


def nominal_binding(e, f, B):
    """The nominal row and the configuration's own tables for every vehicle: the unbound estimator's words."""
    e.set_observer_vehicles(np.tile(D.NOMINAL_ROW, (B, 1)), np.tile(f["g"]["L_ls"], (B, 1, 1, 1)), np.tile(f["g"]["L_hs"], (B, 1, 1, 1)))


def test_step_vehicles_against_the_restatement(fx):
    est = dict(np.load(os.path.join(HERE, "golden", "estimator", "estimator.npz")))
    dt = float(est["dt"])
    rng = np.random.default_rng(12)
    n0 = len(est["grid_k"])                                           # both polytopes, start-up steps, points outside the polytopes
    B = 333
    m = B - n0
    x = np.empty((B, 6)); y = np.empty((B, 5)); u = np.empty((B, 2)); k = np.empty(B, np.int32)
    x[:n0], y[:n0], u[:n0], k[:n0] = est["grid_est"], est["grid_y"], est["grid_u"], est["grid_k"]
    x[n0:] = np.column_stack([rng.uniform(0.05, 5.0, m), rng.uniform(-0.6, 0.6, m), rng.uniform(-4, 4, m), rng.uniform(-5, 5, m),
                              rng.uniform(-5, 5, m), rng.uniform(-6, 6, m)])
    y[n0:] = x[n0:, [0, 2, 3, 4, 5]] + rng.normal(0, 0.1, (m, 5))
    y[n0:, 0] = np.abs(y[n0:, 0]) + 0.05
    u[n0:] = np.column_stack([rng.uniform(-0.5, 0.5, m), rng.uniform(-1, 1, m)])
    k[n0:] = rng.integers(1, 400, m)
    idx = np.arange(B) % 40                                           # a row and tables of its own per instance
    rows, L_ls, L_hs = fx["rows"][idx], fx["L_ls"][idx], fx["L_hs"][idx]
    e = ctrl(lshape())
    cfg = obs_cfg()
    new, (L, A, Bm) = e.observer_step_vehicles(cfg, x, y, u, k, rows, L_ls, L_hs, want_aux=True)
    worst = 0.0
    for i in range(B):
        xn, Lr, Ar, Br = D.observer_step(rows[i], L_ls[i], L_hs[i], fx["lim_ls"], fx["lim_hs"], x[i], y[i], u[i], int(k[i]), dt)
        for got, want in ((new[i], xn), (L[i], Lr), (A[i], Ar), (Bm[i], Br)):
            worst = max(worst, float(np.max(np.abs(got - want)) / max(1.0, np.max(np.abs(want)))))
    print("observer_step_vehicles vs restatement, %d instances: worst relative deviation %.3e" % (B, worst))
    assert worst <= 1e-12
    vx = np.where(k * dt > 0.02, x[:, 0], y[:, 0])
    assert (vx > fx["lim_ls"][0, 1]).sum() > 50 and (vx <= fx["lim_ls"][0, 1]).sum() > 50
    assert (k <= 4).sum() > 20 and (vx > fx["lim_hs"][0, 1]).sum() > 20 and (vx < fx["lim_ls"][0, 0]).sum() > 10
    # the nominal row with the configuration's tables: the unbound step's words, aux included
    a = e.observer_step(cfg, x, y, u, k, want_aux=True)
    b = e.observer_step_vehicles(cfg, x, y, u, k, np.tile(D.NOMINAL_ROW, (B, 1)), np.tile(fx["g"]["L_ls"], (B, 1, 1, 1)),
                                 np.tile(fx["g"]["L_hs"], (B, 1, 1, 1)), want_aux=True)
    assert same(a[0], b[0]) and all(same(p, q) for p, q in zip(a[1], b[1]))
    assert not same(a[0], new)
    e.close()


def cl_words(e, T):
    e.cl_tick(T)
    o = e.cl_read()
    o["est"], o["meas"] = e.observer_read()
    return o


def test_nominal_binding_is_the_unbound_fleet_and_race(fx):
    mp = lshape()
    oc = obs_cfg(**dict(STD, seed=5))
    plant0 = RO.grid_fleet(B67, 3)
    out = []
    for bound in (False, True):
        e = ctrl(mp)
        e.observer_setup(oc)
        if bound:
            nominal_binding(e, fx, B67)
        e.cl_init(plant0, mp.halfWidth, mp.slack, q9_swap=True, n_sub=7, plant_params="nominal")
        out.append(cl_words(e, 6))
        e.close()
    for k in out[0]:
        assert same(out[0][k], out[1][k]), k
    plant0 = RO.start_line_fleet(mp.PointAndTangent, B67, 7)
    out = []
    for bound in (False, True):
        path, tt, plan = engines(mp)
        if bound:
            nominal_binding(path, fx, B67)
        path.race_init(tt, plan, plant0, half_track0=1, laps=2, half_width=mp.halfWidth, slack=mp.slack, estimator=oc, plant_params="nominal")
        path.race_tick(6)
        o = path.race_read()
        o["est"], o["meas"] = path.observer_read()
        out.append(o)
        close(path, tt, plan)
    assert np.all(out[0]["phase"] == 0)
    for k in out[0]:
        if k not in ("plan_iters", "plan_status"):          # the planner handle's report: not written before a vehicle's first planner tick
            assert same(out[0][k], out[1][k]), k


def replay_fleet(fx, mp, e, plant0, rows, tabs, noisy, T, vid0=0):
    """The bound lap-0 fleet of e against the host replay whose vehicle b has the restated per-vehicle estimator with tabs[b]."""
    B = len(plant0)
    ref = P.vehicle_lap0_replay(mp.PointAndTangent, plant0, plant_params=rows, laps=1, half_width=mp.halfWidth, slack=mp.slack,
                                gains=fx["g"], stds=STDS if noisy else (0, 0, 0, 0, 0), seed=3, vehicle_offset=vid0)
    ref.veh = [D.Vehicle(rows[b], tabs[0][b], tabs[1][b], fx["lim_ls"], fx["lim_hs"], plant0[b], stds=STDS if noisy else (0, 0, 0, 0, 0),
                         seed=3, vid=vid0 + b) for b in range(B)]
    worst, same_it = 0.0, 0
    for t in range(T):
        e.cl_tick(1); ref.tick()
        o = e.cl_read()
        est, meas = e.observer_read()
        assert np.all(ref.phase == 0) and np.array_equal(o["status"], ref.status), t
        same_it += int(np.sum(o["iters"] == ref.iters))
        worst = max(worst, *(float(np.max(np.abs(a - b))) for a, b in ((o["plant"], ref.plant), (o["local"], ref.local), (o["cmd"], ref.cmd),
                                                                        (est, ref.estimate()), (meas, np.array([v.y for v in ref.veh])))))
    return worst, same_it, ref


@pytest.mark.parametrize("tables", ["design", "scipy"])
@pytest.mark.parametrize("noisy", [False, True])
def test_bound_fleet_matches_the_host_replay(fx, tables, noisy):
    """67 vehicles, plant rows = estimator rows (the fixture's, recycled): tables designed on the device into the binding, or
    scipy's from the fixture bound explicitly; 10 ticks within 2e-6 of the oracle plant + the restated per-vehicle estimator
    running on the tables read back from the device."""
    mp = lshape()
    rows = fx["rows67"]
    plant0 = RO.grid_fleet(B67, 21)
    e = ctrl(mp)
    e.observer_setup(obs_cfg(**(dict(STD, seed=3) if noisy else {})))
    if tables == "design":
        e.set_observer_vehicles(rows, design=design_of(fx))
    else:
        e.set_observer_vehicles(rows, fx["L_ls"][fx["idx"]], fx["L_hs"][fx["idx"]])
    r, L_ls, L_hs = e.observer_vehicles_read()
    assert same(r, rows)
    if tables == "scipy":
        assert same(L_ls, fx["L_ls"][fx["idx"]]) and same(L_hs, fx["L_hs"][fx["idx"]])
    e.cl_init(plant0, mp.halfWidth, mp.slack, q9_swap=True, n_sub=7, plant_params=rows)
    worst, same_it, ref = replay_fleet(fx, mp, e, plant0, rows, (L_ls, L_hs), noisy, 10)
    # the rows and tables matter: the nominal estimator on the same plants is far away
    nom = P.vehicle_lap0_replay(mp.PointAndTangent, plant0, plant_params=rows, laps=1, half_width=mp.halfWidth, slack=mp.slack,
                                gains=fx["g"], stds=STDS if noisy else (0, 0, 0, 0, 0), seed=3)
    for _ in range(10):
        nom.tick()
    far = float(np.max(np.abs(nom.estimate() - ref.estimate())))
    print("bound fleet (%s tables, noisy %s) vs replay: %.3e over 10 ticks, %d of %d iteration counts equal; the nominal estimator differs by %.3g"
          % (tables, noisy, worst, same_it, 10 * B67, far))
    assert worst <= 2e-6
    assert far > 1e-4
    e.close()


def test_sharded_fleets_equal_the_whole(fx):
    mp = lshape()
    rows = fx["rows67"]
    plant0 = RO.grid_fleet(B67, 8)
    kw = dict(STD, seed=99)

    def run(lo, hi):
        e = ctrl(mp)
        e.observer_setup(obs_cfg(vehicle_offset=lo, **kw))
        e.set_observer_vehicles(rows[lo:hi], design=design_of(fx))
        e.cl_init(plant0[lo:hi], mp.halfWidth, mp.slack, q9_swap=True, n_sub=7, plant_params=rows[lo:hi])
        o = cl_words(e, 8)
        o["tabs"] = np.concatenate([t.reshape(hi - lo, -1) for t in e.observer_vehicles_read()], axis=1)
        e.close()
        return o

    whole, a, b = run(0, B67), run(0, 33), run(33, B67)
    for k in whole:
        assert same(whole[k], np.concatenate([a[k], b[k]])), k


def test_bound_race_matches_the_host_replay(fx):
    """12 vehicles near the line with sampled plant rows, estimator rows = plant rows, designed tables, noisy sensors: lap 0 within
    2e-6 of the replay, lap events on the same ticks, and the racing ticks that follow inside the bars of
    tests/test_gpu_plant_params.py::test_mismatched_race_matches_the_replay."""
    import lpvmpc
    mp = lshape()
    B, T = 12, 26
    plant0 = RO.start_line_fleet(mp.PointAndTangent, B, 17, 0.962, 0.978)
    rows = lpvmpc.sample_plant_params(B, 23)
    path, tt, plan = engines(mp)
    path.set_observer_vehicles(rows, design=design_of(fx))
    _r, L_ls, L_hs = path.observer_vehicles_read()
    path.race_init(tt, plan, plant0, half_track0=1, laps=3, half_width=mp.halfWidth, slack=mp.slack, plant_params=rows,
                   estimator=obs_cfg(**dict(STD, seed=5)))
    ref = P.VehicleRaceRef(mp.PointAndTangent, plant0, plant_params=rows, half_track0=1, laps=3, half_width=mp.halfWidth, slack=mp.slack,
                           gains=fx["g"], stds=STDS, seed=5)
    ref.veh = [D.Vehicle(rows[b], L_ls[b], L_hs[b], fx["lim_ls"], fx["lim_hs"], plant0[b], stds=STDS, seed=5, vid=b) for b in range(B)]
    ev_dev = np.full(B, -1)
    err0 = 0.0
    w_state = np.zeros(B); w_cmd = np.zeros(B); racing = np.zeros(B, int)
    same_it = n_it = 0
    for t in range(T):
        path.race_tick(1); ref.tick()
        o = path.race_read()
        est, rest = path.observer_read()[0], ref.estimate()
        ev_dev[(ev_dev < 0) & (o["phase"] == 1)] = t
        assert np.array_equal(o["phase"], ref.phase), t
        lap0 = o["phase"] == 0
        if np.any(lap0):
            err0 = max(err0, *(float(np.max(np.abs(a[lap0] - b[lap0]))) for a, b in ((o["plant"], ref.plant), (est, rest), (o["local"], ref.local),
                                                                                      (o["cmd"], ref.cmd))))
            assert np.array_equal(o["status"][lap0], ref.status[lap0]), t
        for v in np.nonzero((o["phase"] == 1) & (ref.event_tick < t))[0]:
            assert np.all(np.isfinite(o["cmd"][v])) and o["status"][v] == ref.status[v], (t, v)
            w_state[v] = max(w_state[v], float(np.max(np.abs(o["plant"][v] - ref.plant[v]))), float(np.max(np.abs(est[v] - rest[v]))),
                             float(np.max(np.abs(o["local"][v] - ref.local[v]))))
            w_cmd[v] = max(w_cmd[v], float(np.max(np.abs(o["cmd"][v] - ref.cmd[v]))))
            same_it += int(o["iters"][v] == ref.iters[v]); n_it += 1
            racing[v] += 1
    raced = racing > 0
    strict = raced & (w_state <= 1e-5) & (w_cmd <= 1e-4)
    print("bound race vs replay: events %s, lap 0 worst %.3g, %d vehicles with racing ticks (%d ticks): within 1e-5 / 1e-4: %d, worst %.3g / %.3g, "
          "iterations %d / %d" % (sorted(ev_dev.tolist()), err0, raced.sum(), racing.sum(), strict.sum(), w_state.max(), w_cmd.max(), same_it, n_it))
    assert np.array_equal(ev_dev, ref.event_tick) and np.all(ev_dev[ev_dev >= 0] >= 9)
    assert raced.sum() >= 1 and err0 <= 2e-6
    assert strict.sum() >= 2 * raced.sum() // 3 and same_it >= 0.95 * n_it
    assert np.all(w_state <= 2e-2) and np.all(w_cmd <= 2e-2)
    close(path, tt, plan)


def test_binding_semantics(fx):
    import lpvmpc
    from lpvmpc import _ffi, api, workloads as W
    mp = lshape()
    B = 9
    rows = np.ascontiguousarray(fx["rows"][:B])
    plant0 = RO.grid_fleet(B, 4)
    oc = obs_cfg()
    e = ctrl(mp)
    assert e.observer_vehicles_read() is None
    # designed into the binding = the stand-alone design's words
    e.set_observer_vehicles(rows, design=design_of(fx))
    r, L_ls, L_hs = e.observer_vehicles_read()
    d_ls, d_hs = e.observer_design(rows, fx["lim_ls"], fx["lim_hs"])
    assert same(r, rows) and same(L_ls, d_ls) and same(L_hs, d_hs)
    # refused, the binding kept: neither / both of tables and design, one table only, bad rows, a design that does not converge
    lib, h = e._lib, e._h
    good = api.observer_design_config(fx["lim_ls"], fx["lim_hs"])
    bad_rows = rows.copy(); bad_rows[2, 2] = -1.0
    nan_tab = d_ls.copy(); nan_tab[1, 0, 0, 0] = np.nan
    for args in ((B, _ffi.ptr(rows), None, None, None), (B, _ffi.ptr(rows), _ffi.ptr(d_ls), _ffi.ptr(d_hs), C.byref(good)),
                 (B, _ffi.ptr(rows), _ffi.ptr(d_ls), None, None), (B, _ffi.ptr(bad_rows), None, None, C.byref(good)),
                 (B, _ffi.ptr(rows), _ffi.ptr(nan_tab), _ffi.ptr(d_hs), None), (-1, None, None, None, None), (B, None, None, None, C.byref(good)),
                 (B, _ffi.ptr(rows), None, None, C.byref(api.observer_design_config(fx["lim_ls"], fx["lim_hs"], np.zeros((6, 6)),
                                                                                           np.diag([1e300] * 5))))):
        assert lib.lpvmpc_set_observer_vehicles(h, *args) == _ffi.E_ARG, args[0]
        assert same(e.observer_vehicles_read()[1], d_ls)
    assert "vehicle 0" in lib.lpvmpc_last_error(h).decode() and "vertex" in lib.lpvmpc_last_error(h).decode()
    plan = lpvmpc.BatchedSolver("planner", 40, 0.05, W.PLAN_Q, W.PLAN_R, W.PLAN_dR, L_cf=W.PLAN_L, track=mp.PointAndTangent)
    assert plan._lib.lpvmpc_set_observer_vehicles(plan._h, B, _ffi.ptr(rows), None, None, C.byref(good)) == _ffi.E_ARG
    plan.close()
    # starts: the starts that do not run the binding refuse the bound handle when an estimator is attached ...
    e.observer_setup(oc)
    for kw in (dict(), dict(actuator=lpvmpc.actuator_config())):
        with pytest.raises(lpvmpc.LpvMpcError):
            e.cl_init(plant0, mp.halfWidth, mp.slack, **kw)
    with pytest.raises(lpvmpc.LpvMpcError) as err:                              # ... another B ...
        e.cl_init(plant0[:B - 1], mp.halfWidth, mp.slack, plant_params="nominal")
    assert "%d vehicles" % B in str(err.value)
    lim = fx["lim_hs"].copy(); lim[0, 1] = 4.5                                  # ... and a design on other limits than the configuration's
    from lpvmpc.observer import observer_config
    e.observer_setup(observer_config(fx["g"]["L_ls"], fx["lim_ls"], fx["g"]["L_hs"], lim))
    with pytest.raises(lpvmpc.LpvMpcError):
        e.cl_init(plant0, mp.halfWidth, mp.slack, plant_params="nominal")
    e.observer_setup(None)                                                      # without an estimator the binding is not read
    e.cl_init(plant0, mp.halfWidth, mp.slack)
    with pytest.raises(lpvmpc.LpvMpcError):                                     # refused while the fleet runs
        e.set_observer_vehicles(rows, design=design_of(fx))
    with pytest.raises(lpvmpc.LpvMpcError):
        e.set_observer_vehicles(None)
    e.cl_release()
    assert same(e.observer_vehicles_read()[1], d_ls)                            # cl_release keeps the binding
    # bound, then B = 0: the unbound fleet's words again; explicit tables under other limits are the caller's business
    e.observer_setup(oc)
    e.cl_init(plant0, mp.halfWidth, mp.slack, plant_params="nominal")
    bound = cl_words(e, 5)
    e.cl_release()
    e.set_observer_vehicles(None)
    assert e.observer_vehicles_read() is None
    e.cl_init(plant0, mp.halfWidth, mp.slack, plant_params="nominal")
    unbound = cl_words(e, 5)
    e.cl_release()
    f = ctrl(mp)
    f.observer_setup(oc)
    f.cl_init(plant0, mp.halfWidth, mp.slack, plant_params="nominal")
    fresh = cl_words(f, 5)
    f.close()
    assert all(same(unbound[k], fresh[k]) for k in fresh) and not same(bound["est"], fresh["est"])
    e.set_observer_vehicles(rows, d_ls, d_hs)
    e.observer_setup(observer_config(fx["g"]["L_ls"], fx["lim_ls"], fx["g"]["L_hs"], lim))
    e.cl_init(plant0, mp.halfWidth, mp.slack, plant_params="nominal")
    e.close()                                                                   # destroy frees a bound handle with a running fleet
    # the race: bound on the path handle; the starts without per-vehicle rows refuse it, RaceFleet binds before race_init
    path, tt, plan = engines(mp)
    path.set_observer_vehicles(rows, design=design_of(fx))
    with pytest.raises(lpvmpc.LpvMpcError):
        path.race_init(tt, plan, plant0, half_width=mp.halfWidth, slack=mp.slack, estimator=oc)
    with pytest.raises(lpvmpc.LpvMpcError):
        path.race_init(tt, plan, plant0[:4], half_width=mp.halfWidth, slack=mp.slack, estimator=oc, plant_params="nominal")
    path.race_init(tt, plan, plant0, half_width=mp.halfWidth, slack=mp.slack)      # ground truth: not read
    close(path, tt, plan)
    fleet = lpvmpc.RaceFleet(mp, plant0, estimator=oc, plant_params=rows, estimator_params="plant", tyre_params="pacejka")
    r, L_ls, _ = fleet.path.observer_vehicles_read()
    assert same(r, rows) and same(L_ls, d_ls)
    fleet.run(3)
    assert np.all(np.isfinite(fleet.estimate()[0]))
    fleet.close()
