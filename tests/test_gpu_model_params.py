"""GPU: per-vehicle model parameters (lpvmpc_set_model_params, lpvmpc_model_params_read; include/lpvmpc.h, "Per-vehicle model
parameters").  A handle with model rows bound linearises vehicle b with row b:
  * against the oracle with each vehicle's row (LPV, seed mode, solves; tests/_model_params.py: ROWS, BATCHES);
  * word for word against the per-handle path that exists without a binding -- one plain handle per row, created with
    BatchedSolver(params=row) -- on every solve route;
  * nominal rows change nothing (stand-alone calls, lap-0 fleet, cascade, race), and unbinding restores a fresh handle;
  * vehicles are independent through the lap event and the racing phase; lap 0 against the host replay; refusals and lifetime;
    the full-size race.

The controller roll-out of a bound handle takes the row's Cf for BOTH axles and ignores the call's cf_new.  On the per-handle path
the same quantity is the call's cf_new, so a plain handle reproduces a bound one where the caller passes cf_new = the row's Cf
(the stand-alone tests below do).  The fleet, cascade and race ENGINES pass the literal 60.0, and so does the host replay
(tests/_race_ref.py): a fleet of plain handles or a replay can only reproduce bound rows whose Cf is 60.  The fleet tests that
compare against them therefore bind ROWS with Cf set to 60 (rows60: each row's lf, lr, m, Iz, Cr and mu kept; Cr still differs from
Cf in three of the four rows, and the seed-mode ticks and the planner read both); rows with Cf != 60 are held to the oracle and to
the per-handle path by the stand-alone tests, and run through the engines in the full-size race."""
import ctypes as C
import threading

import numpy as np
import pytest

from oracle import lpv_ref as L
from tests import _model_params as M
from tests import _race_observer_ref as RO
from tests import _tolerance as T
from tests.test_gpu_delayed_fleets import STD, close, ctrl, engines, lshape, obs_cfg, same
from tests.test_gpu_horizons import delay_workload, relclose
from tests.test_gpu_plant_params import RACE_KEYS, _race_same

pytestmark = pytest.mark.gpu

NOM = np.array([0.125, 0.125, 1.98, 0.03, 60.0, 60.0, 0.05])
_B = {}


def batch(name):
    if not _B:
        _B.update(M.batches())
    return _B[name]


NAMES = ("ctrl8", "ctrl20", "ctrl8_lap0", "ctrl20_lap0", "plan30", "plan40")


def engine(w, params=None, variant=0, **settings):
    import lpvmpc
    d = int(np.asarray(w["u_old"]).reshape(w["x0"].shape[0], -1).shape[1] - 2) if w["kind"] == "controller" else 0
    e = lpvmpc.BatchedSolver(w["kind"], w["N"], w["dt"], w["Q"], w["R"], w["dR"], L_cf=w["L_cf"], track=w["track"], params=params,
                             steering_delay=d, **settings)
    e.set_option("kernel_variant", variant)
    return e


def solve(e, w):
    return e.solve(w["x0"], w["u_prev"], w["vel_ref"], w["curv_s"], w["u_old"], w["max_ey"], w["cf_new"], w["lap"])


def lpv(e, w):
    return e.lpv(w["x0"], w["u_prev"], w["vel_ref"], w["curv_s"], cf_new=w["cf_new"], lap=w["lap"])


def seed_inputs(w, kind, seed):
    """Trajectories and steering angles for the seed-mode linearisation (as test_vehicle_lpv_and_seed_mode draws them)."""
    B, N = w["x0"].shape[0], int(w["N"])
    rng = np.random.default_rng(seed)
    tab = w["track"]; Lt = float(tab[-1, 3] + tab[-1, 4])
    vx = rng.uniform(0.8, 3.0, (B, N)); vy = rng.normal(0, 0.05, (B, N)); wz = rng.normal(0, 0.3, (B, N))
    epsi = rng.normal(0, 0.1, (B, N)); ey = rng.normal(0, 0.1, (B, N)); s = rng.uniform(0.0, 0.99 * Lt, (B, N))
    delta = rng.uniform(-0.24, 0.24, (B, N))
    xx = np.stack([vx, vy, wz, epsi, s, ey], axis=2) if kind == "controller" else np.stack([vx, vy, wz, ey, epsi, s], axis=2)
    return xx, delta


# ---- 5. against the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_bound_rows_against_the_oracle(name):
    """ROWS interleaved and bound: lpv() states and [A | B] and the seed-mode [A | B] against oracle.lpv_ref with each vehicle's
    row (1e-12 of each array's largest magnitude, the bar of test_vehicle_lpv_and_seed_mode); the solves against
    tick_batch_qp(params=row), run per row group and reassembled, under check_batch as it stands."""
    kind, w = batch(name)
    B, N, tab = w["x0"].shape[0], int(w["N"]), w["track"]
    rows = M.interleaved(B)
    e = engine(w)
    e.set_model_params(rows)
    S, A, Bm = lpv(e, w)
    xx, delta = seed_inputs(w, kind, 9100 + N)
    Ae, Be = e.estimate_abc(xx, delta)
    out = solve(e, w)
    e.close()
    worst = 0.0
    for j in range(B):
        p = dict(L.DEFAULT_PARAMS, **M.params_of(rows[j]))
        if kind == "controller":
            Sr, Ar, Br = L.ctrl_lpv_prediction(p, w["dt"], N, tab, w["x0"][j], w["u_prev"][j], w["vel_ref"][j],
                                               None if w["curv_s"] is None else w["curv_s"][j], float(rows[j, 4]), w["lap"])
            Aer, Ber = L.ctrl_estimate_abc(p, w["dt"], N, tab, xx[j], np.stack([delta[j], np.zeros(N)], axis=1))
        else:
            Sr, Ar, Br = L.plan_lpv_prediction(p, w["dt"], N, tab, w["x0"][j], w["curv_s"][j], w["u_prev"][j])
            Aer, Ber = L.plan_estimate_abc(p, w["dt"], N, tab, xx[j], delta[j])
        for got, want, what in ((S[j], Sr, "states"), (A[j], Ar, "A"), (Bm[j], Br, "B"), (Ae[j], Aer, "abc A"), (Be[j], Ber, "abc B")):
            worst = max(worst, relclose(got, want, 1e-12, "%s #%d %s" % (name, j, what)))
    ref = M.oracle_rows(w, kind, rows)
    assert not np.any(ref["status"] == -10)                       # (tests/test_model_params_host.py: the oracle answers every instance)
    total = {}
    for row, idx in M.groups(rows):
        g = M.group_workload(w, kind, idx, row)
        c = T.check_batch(g, kind, {k: v[idx] for k, v in out.items()}, {k: v[idx] for k, v in ref.items()}, params=M.params_of(row))
        for k, v in c.items():
            total[k] = total.get(k, 0) + v
    print("%s: lpv / seed-mode max rel err %.2e; solves iters %d..%d %s" % (name, worst, out["iters"].min(), out["iters"].max(), total))
    assert set(total) == {"A", "B", "C", "D", "no_solution", "flips"}


# ---- 6. word for word against the per-handle path ----------------------------------------------------------------------------
def _dev_solve(e, w):
    import torch
    dev = torch.device("cuda", 0)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    B, N, nx = w["x0"].shape[0], int(w["N"]), (6 if w["kind"] == "controller" else 5)
    e.reserve(B)
    ins = [t(w[k]) for k in ("x0", "u_prev", "vel_ref", "curv_s", "u_old", "max_ey")]
    o = dict(xPred=torch.zeros((B, N + 1, nx), dtype=torch.float64, device=dev), uPred=torch.zeros((B, N, 2), dtype=torch.float64, device=dev),
             status=torch.zeros(B, dtype=torch.int32, device=dev), iters=torch.zeros(B, dtype=torch.int32, device=dev),
             resid=torch.zeros((B, 4), dtype=torch.float64, device=dev), polish=torch.zeros(B, dtype=torch.int32, device=dev))
    e.solve_dev(B, *ins, o["xPred"], o["uPred"], o["status"], o["iters"], o["resid"], o["polish"], cf_new=w["cf_new"], lap=w["lap"])
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def _defer(e, w, tail):
    B = w["x0"].shape[0]
    e.reserve(B)
    e.set_option("defer_after", 25); e.set_option("defer_budget", -1); e.set_option("defer_pool", B); e.set_option("defer_tail", tail)


def run_route(e, w, route):
    """Every output of one route as a list of dicts (one per tick)."""
    if route == "masked":
        return [e.solve_batch_masked(w["active"], w["x0"], w["u_prev"], w["vel_ref"], w["curv_s"], w["u_old"], w["max_ey"], w["cf_new"], w["lap"])]
    if route == "dev":
        return [_dev_solve(e, w)]
    if route == "warm":
        e.set_option("warm_start", 1)
        return [solve(e, w) for _ in range(3)]
    if route in ("defer", "tail"):
        _defer(e, w, 0 if route == "defer" else 1)
        return [solve(e, w)]
    return [solve(e, w)]


def compare_routes(name, w, kind, route, variant=0):
    B = w["x0"].shape[0]
    rows = M.interleaved(B)
    w = dict(w, active=(np.arange(B) % 3 != 0).astype(np.int32))
    e = engine(w, variant=variant)
    e.set_model_params(rows)
    S, A, Bm = lpv(e, w)
    got = run_route(e, w, route)
    e.close()
    worst = 0.0
    for row, idx in M.groups(rows):
        g = M.group_workload(w, kind, idx, row)                   # cf_new = the row's Cf
        p = engine(g, params=M.params_of(row), variant=variant)
        Sg, Ag, Bg = lpv(p, g)
        assert same(S[idx], Sg) and same(A[idx], Ag) and same(Bm[idx], Bg), (name, route, "lpv")
        ref = run_route(p, g, route)
        p.close()
        for a, r in zip(got, ref):
            for k in ("status", "iters", "polish"):
                assert np.array_equal(a[k][idx], r[k]), (name, route, variant, k)
            if route == "tail":
                # which instances the whole-CU tail kernel finishes depends on what else is parked: the deferred path's own bar
                pol = (r["status"] == 1) & (r["polish"] == 1)
                for k in ("xPred", "uPred"):
                    d = np.abs(a[k][idx] - r[k]).reshape(len(idx), -1)
                    d = np.where(np.isnan(d), 0.0, d).max(axis=1)
                    assert np.array_equal(np.isnan(a[k][idx]), np.isnan(r[k])), (name, k)
                    assert np.all(d[pol] <= 1e-7) and np.all(d[~pol] <= 1e-6), (name, k, float(d.max()))
                    worst = max(worst, float(d.max()))
            else:
                for k in ("xPred", "uPred", "resid"):
                    assert same(a[k][idx], r[k]), (name, route, variant, k)
    return worst


@pytest.mark.parametrize("name", NAMES)
def test_bound_handle_equals_one_handle_per_row(name):
    """The bound handle's states, [A | B], xPred, uPred, status, iterations, polish flag and residuals equal, word for word, those of
    four plain handles created with BatchedSolver(params=row) on their sub-batches (cf_new = the row's Cf): the default route,
    kernel_variant 1, 3 and 9, deferral with defer_tail 0, lpvmpc_solve_batch_masked, the device-pointer call and warm start 1 over
    three ticks; with the default tail kernel the deferred path's own comparison."""
    kind, w = batch(name)
    for route, variant in (("plain", 0), ("plain", 1), ("plain", 3), ("plain", 9), ("defer", 0), ("masked", 0), ("dev", 0), ("warm", 0)):
        compare_routes(name, w, kind, route, variant)
    worst = compare_routes(name, w, kind, "tail")
    print("%s: every route word for word; default tail kernel max difference %.2e" % (name, worst))


def test_bound_handle_with_steering_delay_equals_one_handle_per_row():
    w = delay_workload(71, 20, 1, seed=9201)
    for route in ("plain", "masked", "warm"):
        compare_routes("ctrl20d1", w, "controller", route)


# ---- 7. nominal rows change nothing ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ctrl20", "ctrl8_lap0", "plan30", "plan40"])
def test_nominal_rows_change_no_stand_alone_call(name):
    """Rows equal to the handle's words (Cf = 60 = the workload's cf_new), bound explicitly: every word of lpv, estimate_abc and
    solve equals the unbound handle's; after unbinding the handle equals a fresh one again."""
    import lpvmpc
    kind, w = batch(name)
    B = w["x0"].shape[0]
    assert w["cf_new"] == 60.0
    xx, delta = seed_inputs(w, kind, 9300)

    def everything(e):
        return list(lpv(e, w)) + list(e.estimate_abc(xx, delta)) + [v for _, v in sorted(solve(e, w).items())]

    fresh = engine(w)
    want = everything(fresh)
    fresh.close()
    e = engine(w)
    assert e.model_params_read() is None
    rows = lpvmpc.model_params(B, e)
    assert same(rows, np.tile(NOM, (B, 1)))
    e.set_model_params(rows)
    assert same(e.model_params_read(), rows)
    for a, b in zip(everything(e), want):
        assert same(a, b), name
    e.set_model_params(M.interleaved(B))                          # other rows in between, then none
    assert not same(everything(e)[1], want[1])
    e.set_model_params(None)
    assert e.model_params_read() is None
    for a, b in zip(everything(e), want):
        assert same(a, b), name
    e.close()


def cl_run(mp, plant0, T, bind=None, est=None, params=None, **kw):
    import lpvmpc
    from lpvmpc import workloads as W
    if params is None:
        e = ctrl(mp)
    else:
        Q, R, dR = W.CTRL_TUNINGS["path"]
        e = lpvmpc.BatchedSolver("controller", 20, 1 / 30.0, Q, R, dR, track=mp.PointAndTangent, params=params)
    if bind is not None:
        e.set_model_params(bind)
    if est is not None:
        e.observer_setup(est)
    e.cl_init(plant0, mp.halfWidth, mp.slack, q9_swap=True, n_sub=7, **kw)
    out = []
    for _ in range(T):
        e.cl_tick(1)
        o = e.cl_read()
        if est is not None:
            o["est"], o["meas"] = e.observer_read()
        out.append(o)
    e.close()
    return out


@pytest.mark.parametrize("est", [False, True])
def test_nominal_rows_change_no_lap0_fleet(est):
    mp = lshape()
    B, T = 48, 60
    plant0 = RO.grid_fleet(B, 3)
    oc = obs_cfg(**dict(STD, seed=5)) if est else None
    a = cl_run(mp, plant0, T, est=oc)
    b = cl_run(mp, plant0, T, bind=np.tile(NOM, (B, 1)), est=oc)
    for t in range(T):
        for k in ("plant", "local", "cmd", "iters", "status") + (("est", "meas") if est else ()):
            assert same(a[t][k], b[t][k]), (t, k)


def test_nominal_rows_change_no_cascade():
    from tests._golden import load
    from tests.test_gpu_cascade import controller_tt, fleet_start, planner
    c = load("cascade")
    B, K = 24, 30
    plant0 = fleet_start(c, 5, B)
    runs = []
    for bind in (False, True):
        plan, mp = planner()
        plan.handoff_setup()
        e = controller_tt(mp)
        if bind:
            e.set_model_params(np.tile(NOM, (B, 1))); plan.set_model_params(np.tile(NOM, (B, 1)))
        e.cascade_init(plan, plant0, np.tile(c["cmd0"], (B, 1)), np.tile(c["uPred0"], (B, 1, 1)), lap0=1, half_width=mp.halfWidth,
                       slack=mp.slack, plan_max_ey=0.2, q9_swap=True)
        out = []
        for _ in range(K):
            e.cascade_tick(1)
            out.append(e.cascade_read())
        runs.append(out)
        close(e, plan)
    for t in range(K):
        assert sorted(runs[0][t]) == sorted(runs[1][t])
        for k in runs[0][t]:
            assert same(runs[0][t][k], runs[1][t][k]), (t, k)


def race_run(mp, plant0, T, d=0, bind=None, params=None, laps=2, **kw):
    """bind: rows for (path, tt, planner), or one table for all three; params: the vehicle the three engines are created with."""
    import lpvmpc
    from lpvmpc import workloads as W
    if params is None:
        path, tt, plan = engines(mp, d)
    else:
        mk = lambda role: lpvmpc.BatchedSolver("controller", 20, 1 / 30.0, *W.CTRL_TUNINGS[role], track=mp.PointAndTangent, params=params)
        path, tt = mk("path"), mk("race")
        plan = lpvmpc.BatchedSolver("planner", 40, 0.05, W.PLAN_Q, W.PLAN_R, W.PLAN_dR, L_cf=W.PLAN_L, track=mp.PointAndTangent, params=params)
        plan.handoff_setup()
    if bind is not None:
        for e, r in zip((path, tt, plan), bind if isinstance(bind, tuple) else (bind,) * 3):
            e.set_model_params(r)
    path.race_init(tt, plan, plant0, laps=laps, half_width=mp.halfWidth, slack=mp.slack, **kw)
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
    rows.append(last)
    close(path, tt, plan)
    return rows


@pytest.mark.parametrize("case", ["ground", "estimator", "delayed", "plant_rows"])
def test_nominal_rows_change_no_race(case):
    """90 ticks from the start line (ground truth; the noisy estimator; La / Ld 4 / 6 with the servo lag and steeringDelay 3; plant
    rows): every word read back equals the unbound race's."""
    import lpvmpc
    mp = lshape()
    B, T = 24, 90
    plant0 = RO.start_line_fleet(mp.PointAndTangent, B, 7)
    kw, d = dict(half_track0=1), 0
    if case == "estimator":
        kw["estimator"] = obs_cfg(**dict(STD, seed=9))
    if case == "delayed":
        kw["actuator"] = lpvmpc.actuator_config(0.02, 0.03, low_level_dyn=True); d = 3
    if case == "plant_rows":
        kw["plant_params"] = lpvmpc.sample_plant_params(B, 31)
    a = race_run(mp, plant0, T, d, **kw)
    b = race_run(mp, plant0, T, d, bind=np.tile(NOM, (B, 1)), **kw)
    _race_same(a, b, T, RACE_KEYS + ("est", "meas", "act_state", "path", "tt"))
    assert np.any(a[T - 1]["phase"] >= 1)


# ---- 8. vehicles are independent, through the lap event and the racing phase -------------------------------------------------
def rows60(B=None):
    """ROWS with Cf = 60, the engines' cf_new (module docstring); interleaved over B vehicles, or the four rows."""
    r = M.rows4().copy()
    r[:, 4] = 60.0
    return r if B is None else M.interleaved(B, r)


def test_interleaved_rows_equal_uniform_lap0_fleets():
    """A lap-0 fleet (60 ticks) with the four rows interleaved, bound as model rows and given as plant rows, equals vehicle for
    vehicle and bit for bit the four fleets of a handle CREATED with that row (nothing bound, uniform plant rows)."""
    mp = lshape()
    B, T = 16, 60
    plant0 = RO.grid_fleet(B, 8)
    uni, mixed = rows60(), rows60(B)
    m = cl_run(mp, plant0, T, bind=mixed, plant_params=mixed)
    for k in range(4):
        u = cl_run(mp, plant0, T, params=M.params_of(uni[k]), plant_params=np.tile(uni[k], (B, 1)))
        v = np.arange(B) % 4 == k
        for t in range(T):
            for key in ("plant", "local", "cmd", "iters", "status"):
                assert same(m[t][key][v], u[t][key][v]), (k, t, key)
    assert not same(m[T - 1]["plant"][0, 2:], m[T - 1]["plant"][1, 2:])


def test_interleaved_rows_equal_uniform_races_and_shards():
    """A race of 24 vehicles over 300 ticks, lap events spread out, model rows = plant rows ("plant") interleaved: equal, per vehicle
    and bit for bit, to the four uniform races whose three engines were created with that row (nothing bound, uniform plant rows) --
    through the lap event and the racing phase; the race split into two halves with the rows split likewise equals the whole."""
    import lpvmpc
    mp = lshape()
    B, T = 24, 300
    plant0 = RO.start_line_fleet(mp.PointAndTangent, B, 13, 0.6, 0.97)
    uni, mixed = rows60(), rows60(B)
    f = lpvmpc.RaceFleet(mp, plant0, laps=2, half_track0=1, plant_params=mixed, model_params="plant")
    assert same(f.model_params(), mixed) and same(f.plant_params(), mixed)
    assert same(f.tt.model_params_read(), mixed) and same(f.planner.model_params_read(), mixed)
    f.close()
    keys = ("plant", "local", "cmd", "phase", "lap", "iters", "status")
    whole = race_run(mp, plant0, T, bind=mixed, plant_params=mixed, half_track0=1)
    ev = [int(np.argmax([r["phase"][v] >= 1 for r in whole[:T]])) for v in range(B)]
    assert len(set(ev)) >= 4, ev
    assert np.sum(np.isin(whole[T - 1]["phase"], (1, 2))) >= 4                    # the racing phase is compared, not only lost cars
    for k in range(4):
        u = race_run(mp, plant0, T, params=M.params_of(uni[k]), plant_params=np.tile(uni[k], (B, 1)), half_track0=1)
        _race_same(whole, u, T, keys, np.arange(B) % 4 == k)
    h = B // 2
    lo = race_run(mp, plant0[:h], T, bind=mixed[:h], plant_params=mixed[:h], half_track0=1)
    hi = race_run(mp, plant0[h:], T, bind=mixed[h:], plant_params=mixed[h:], half_track0=1)
    for t in range(T):                        # (the planner's report of a vehicle is written from its first planner tick on: _race_same)
        for key in keys:
            assert same(whole[t][key], np.concatenate([lo[t][key], hi[t][key]])), (t, key)


# ---- 9. lap 0 against the host replay ----------------------------------------------------------------------------------------
def test_bound_lap0_fleet_matches_the_host_replay():
    """8 vehicles, two per row, model rows bound and matched plant rows (each row's lf, lr, m, Iz; Cf = Cr = 60 and the simulator's
    mu: what RaceRef(params=) steps) against one RaceRef(params=row) per row over 40 ticks: the bars of
    test_vehicle_lap0_fleet_matches_the_host_replay (2e-6, identical iteration counts and statuses)."""
    import lpvmpc
    from tests._race_ref import RaceRef
    mp = lshape()
    B, T = 8, 40
    plant0 = RO.grid_fleet(B, 41)
    model = rows60(B)
    plant = model.copy(); plant[:, 4:] = (60.0, 60.0, 0.05)
    e = ctrl(mp)
    e.set_model_params(model)
    e.cl_init(plant0, mp.halfWidth, mp.slack, q9_swap=True, n_sub=7, plant_params=plant)
    refs = [RaceRef(mp.PointAndTangent, plant0[k::4], laps=1, half_width=mp.halfWidth, slack=mp.slack, params=M.params_of(rows60()[k]))
            for k in range(4)]
    worst = 0.0
    for t in range(T):
        e.cl_tick(1)
        o = e.cl_read()
        for k, ref in enumerate(refs):
            ref.tick()
            assert np.all(ref.phase == 0), t
            assert np.array_equal(o["status"][k::4], ref.status) and np.array_equal(o["iters"][k::4], ref.iters), (t, k)
            d = max(float(np.max(np.abs(o["plant"][k::4] - ref.plant))), float(np.max(np.abs(o["local"][k::4] - ref.local))),
                    float(np.max(np.abs(o["cmd"][k::4] - ref.cmd))))
            worst = max(worst, d)
    e.close()
    print("bound lap-0 fleet against the host replay: B=%d, %d ticks, max difference %.2e" % (B, T, worst))
    assert worst <= 2e-6


# ---- 10. refusals and lifetime -----------------------------------------------------------------------------------------------
def test_refusals_and_lifetime():
    import lpvmpc
    from lpvmpc import _ffi
    kind, w = batch("ctrl20")
    B = w["x0"].shape[0]
    rows = M.interleaved(B)
    e = engine(w)
    lib = e._lib
    e.set_model_params(rows)
    assert same(e.model_params_read(), rows)
    before = solve(e, w)

    def refused(rc):
        assert rc == _ffi.E_ARG, rc
        assert same(e.model_params_read(), rows)
        after = solve(e, w)
        for k in before:
            assert same(before[k], after[k]), k

    for b, i, v in ((0, 0, np.nan), (1, 2, 0.0), (2, 3, -0.01), (3, 4, -1.0), (4, 6, -1e-3), (5, 1, np.inf), (6, 1, 0.0), (7, 5, -2.0)):
        bad = rows.copy(); bad[b, i] = v
        refused(lib.lpvmpc_set_model_params(e._h, B, _ffi.ptr(bad)))
        assert "vehicle %d" % b in lib.lpvmpc_last_error(e._h).decode()
    refused(lib.lpvmpc_set_model_params(e._h, -1, _ffi.ptr(rows)))
    refused(lib.lpvmpc_set_model_params(e._h, B, None))
    # another batch size at the batch calls: refused before anything is launched, whatever the route
    sub = M.sub_batch(w, np.arange(B - 3))
    for call in (lambda: solve(e, sub), lambda: lpv(e, sub), lambda: e.estimate_abc(*seed_inputs(sub, kind, 1)),
                 lambda: e.solve_batch_masked(np.ones(B - 3, np.int32), sub["x0"], sub["u_prev"], sub["vel_ref"], sub["curv_s"], sub["u_old"]),
                 lambda: _dev_solve(e, sub)):
        with pytest.raises(lpvmpc.LpvMpcError) as err:
            call()
        assert err.value.code == _ffi.E_ARG
    refused(_ffi.E_ARG)
    # lpvmpc_solve_batch_AB takes the caller's blocks: any batch size
    S, A, Bm = lpv(e, w)
    o = e.solve_AB(w["x0"][:5], A[:5], Bm[:5], w["vel_ref"][:5], w["u_old"][:5])
    assert np.array_equal(o["iters"], before["iters"][:5]) and np.allclose(o["uPred"], before["uPred"][:5], rtol=0, atol=1e-9)
    e.close()
    # the engines check B at init; binding is refused while a fleet runs and accepted after lpvmpc_cl_release
    mp = lshape()
    Bf = 8
    plant0 = RO.grid_fleet(Bf, 2)
    f = ctrl(mp)
    f.set_model_params(rows60(Bf + 1))
    with pytest.raises(lpvmpc.LpvMpcError) as err:
        f.cl_init(plant0, mp.halfWidth, mp.slack)
    assert err.value.code == _ffi.E_ARG
    f.set_model_params(rows60(Bf))
    f.cl_init(plant0, mp.halfWidth, mp.slack)
    f.cl_tick(12)
    for r in (rows60(Bf), None):
        with pytest.raises(lpvmpc.LpvMpcError) as err:
            f.set_model_params(r)
        assert err.value.code == _ffi.E_ARG
    assert same(f.model_params_read(), rows60(Bf))
    f.cl_tick(1)
    f.cl_release()
    f.set_model_params(None)
    f.cl_init(plant0, mp.halfWidth, mp.slack)
    f.cl_tick(20)
    a = f.cl_read()
    g = ctrl(mp)
    g.cl_init(plant0, mp.halfWidth, mp.slack)
    g.cl_tick(20)
    b = g.cl_read()
    for k in ("plant", "local", "cmd", "iters", "status"):
        assert same(a[k], b[k]), k
    close(f, g)
    # cascade and race: each handle's binding is checked at init
    from tests._golden import load
    from tests.test_gpu_cascade import controller_tt, fleet_start, planner
    c = load("cascade")
    for who in ("controller", "planner"):
        plan, mp2 = planner()
        plan.handoff_setup()
        tt = controller_tt(mp2)
        (tt if who == "controller" else plan).set_model_params(rows60(Bf + 2))
        with pytest.raises(lpvmpc.LpvMpcError) as err:
            tt.cascade_init(plan, fleet_start(c, 5, Bf), np.tile(c["cmd0"], (Bf, 1)), np.tile(c["uPred0"], (Bf, 1, 1)), lap0=1,
                            half_width=mp2.halfWidth, slack=mp2.slack, plan_max_ey=0.2, q9_swap=True)
        assert err.value.code == _ffi.E_ARG, who
        close(tt, plan)
    for i in range(3):
        es = engines(mp)
        es[i].set_model_params(rows60(Bf + 2))
        with pytest.raises(lpvmpc.LpvMpcError) as err:
            es[0].race_init(es[1], es[2], plant0, half_width=mp.halfWidth, slack=mp.slack)
        assert err.value.code == _ffi.E_ARG, i
        es[i].set_model_params(rows60(Bf))
        es[0].race_init(es[1], es[2], plant0, half_width=mp.halfWidth, slack=mp.slack)
        es[0].race_tick(3)
        for x in es:                                                  # all three take part in the race: binding refused
            with pytest.raises(lpvmpc.LpvMpcError):
                x.set_model_params(None)
        close(*es)
    # the library's own read-back with a NULL table returns the batch size only
    h = engine(w)
    n = C.c_int32(-1)
    assert h._lib.lpvmpc_model_params_read(h._h, C.byref(n), None) == 0 and n.value == 0
    h.set_model_params(rows)
    assert h._lib.lpvmpc_model_params_read(h._h, C.byref(n), None) == 0 and n.value == B
    h.close()


def test_two_bound_handles_on_two_host_threads():
    """Two handles with different bindings, each on its own host thread (the pattern of test_two_handles_on_two_host_threads): every
    result equals the serial run's, word for word."""
    kind, w = batch("ctrl20")
    B = w["x0"].shape[0]
    tables = (M.interleaved(B), M.interleaved(B, shift=2))

    def run(rows):
        e = engine(w)
        e.set_model_params(rows)
        out = [solve(e, w) for _ in range(3)]
        assert same(e.model_params_read(), rows)
        e.close()
        return out

    serial = [run(r) for r in tables]
    assert not same(serial[0][0]["uPred"], serial[1][0]["uPred"])
    results, errors = [None, None], []

    def worker(i):
        try:
            results[i] = run(tables[i])
        except Exception as e:          # noqa: BLE001 -- reported by the main thread
            errors.append(repr(e))

    th = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors
    for i in range(2):
        for a, b in zip(results[i], serial[i]):
            for k in a:
                assert same(a[k], b[k]), (i, k)


# ---- 11. full size -----------------------------------------------------------------------------------------------------------
def test_full_size_matched_race_properties():
    """8192 vehicles, sampled plant rows, each vehicle's model its plant row ("plant"), 300 ticks.  The size-independent properties of
    test_full_size_cfg5_fleet_properties that apply to a race: a vehicle is alive exactly as long as its plant state is finite, a lost
    vehicle stays lost, statuses are valid, lap counters never decrease.  No survivor count is asserted.  Valid: the per-instance
    statuses include/lpvmpc.h defines for a finished solve (OSQP's status_val; LPVMPC_PENDING belongs to the deferral, which a race does
    not use) and 0, the value of a vehicle whose controller or planner has not solved yet.  That list has LPVMPC_NON_CVX (-7), which
    the cascade's test does not meet: OSQP's rule for a residual beyond 1e30, reported by the planner of vehicles about to be lost."""
    import lpvmpc
    mp = lshape()
    B = 8192
    plant0 = RO.start_line_fleet(mp.PointAndTangent, B, 3, 0.6, 0.97)
    rows = lpvmpc.sample_plant_params(B, 1)
    f = lpvmpc.RaceFleet(mp, plant0, laps=2, half_track0=1, plant_params=rows, model_params="plant")
    assert same(f.model_params(), rows)
    valid = {0} | (set(lpvmpc._ffi.STATUS_TEXT) - {-11})
    assert valid == {0, 1, 2, 3, 4, -2, -3, -4, -7, -10}
    lost_prev = np.zeros(B, bool); lap_prev = np.zeros(B, int)
    for block in range(6):
        f.run(50)
        o = f.state()
        finite = np.all(np.isfinite(o["plant"]), axis=1)
        lost = o["phase"] == 3
        assert not np.any(finite[lost]) and np.all(finite[o["phase"] == 2])         # lost <=> the plant is not finite (found on the next tick)
        assert not np.any(~finite & ~lost & lost_prev)
        assert not np.any(lost_prev & ~lost)                                        # lost stays lost
        assert set(np.unique(o["status"]).tolist()) <= valid and set(np.unique(o["plan_status"]).tolist()) <= valid
        assert np.all(o["lap"] >= lap_prev)
        lost_prev, lap_prev = lost, o["lap"].copy()
    print("full-size matched race: phases after 300 ticks %s" % dict(zip(*np.unique(o["phase"], return_counts=True))))
    f.close()
