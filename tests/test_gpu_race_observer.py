"""GPU: the race engine with the state estimator in the loop (lpvmpc_race_init_observed / race_init(estimator=...)) against the
lap-0 fleet with an estimator (lpvmpc_cl_* after lpvmpc_observer_setup), against the race without one, against the host replay
(tests/_race_observer_ref.py), and its reproducibility, sharding, frozen / lost vehicles, refusals and lifetime."""
import ctypes as C

import numpy as np
import pytest

from tests import _race_observer_ref as RO

pytestmark = pytest.mark.gpu

KV = 0          # kernel_variant fixed on every handle: kernel routes may depend on B
STD = dict(psi_std=0.01, psiDot_std=0.05, x_std=0.01, y_std=0.01, v_std=0.02)      # as test_noisy_fleet_runs_and_the_estimate_tracks_the_plant


def lshape():
    import lpvmpc
    return lpvmpc.Map("L_shape", 0.2)


def obs_cfg(**kw):
    from lpvmpc.observer import observer_config
    g = RO.estimator_gains()
    return observer_config(g["L_ls"], g["lim_ls"], g["L_hs"], g["lim_hs"], **kw)


def engines(mp):
    import lpvmpc
    from lpvmpc import workloads as W
    Qp, Rp, dRp = W.CTRL_TUNINGS["path"]; Qr, Rr, dRr = W.CTRL_TUNINGS["race"]
    path = lpvmpc.BatchedSolver("controller", 20, 1 / 30.0, Qp, Rp, dRp, track=mp.PointAndTangent)
    tt = lpvmpc.BatchedSolver("controller", 20, 1 / 30.0, Qr, Rr, dRr, track=mp.PointAndTangent)
    plan = lpvmpc.BatchedSolver("planner", 40, 0.05, W.PLAN_Q, W.PLAN_R, W.PLAN_dR, L_cf=W.PLAN_L, track=mp.PointAndTangent)
    for e in (path, tt, plan):
        e.set_option("kernel_variant", KV)
    plan.handoff_setup()
    return path, tt, plan


def close(*es):
    for e in es:
        e.close()


def run_race(mp, plant0, ticks, est=None, half=1, laps=3):
    """Race `ticks` ticks; returns every tick's race_read (+ estimate, meas) and the final laps / alive ticks."""
    path, tt, plan = engines(mp)
    path.race_init(tt, plan, plant0, half_track0=half, laps=laps, half_width=mp.halfWidth, slack=mp.slack, estimator=est)
    out = []
    for _ in range(ticks):
        path.race_tick(1)
        o = path.race_read()
        if est is not None:
            o["est"], o["meas"] = path.observer_read()
        out.append(o)
    ls, al = path.race_laps()
    pu, tu = path.race_predictions()
    close(path, tt, plan)
    return out, dict(lap_step=ls, alive=al, path_uPred=pu, tt_uPred=tu)


def same(a, b):
    return np.array_equal(a, b, equal_nan=True) and np.asarray(a).tobytes() == np.asarray(b).tobytes()


@pytest.mark.parametrize("noisy", [False, True])
def test_lap0_equals_the_observed_fleet_bit_for_bit(noisy):
    """64 vehicles from the grid, no lap event in the window: the race with an estimator is lpvmpc_cl_tick with the estimator,
    word for word, every tick -- plant, measurement, command, iterations, status and the estimator's state."""
    import lpvmpc
    from lpvmpc import workloads as W
    mp = lshape()
    B = 64
    plant0 = RO.grid_fleet(B, 5)
    kw = dict(STD, seed=11) if noisy else {}           # the launch file's sensors: every std 0
    path, tt, plan = engines(mp)
    path.race_init(tt, plan, plant0, half_track0=0, laps=1, half_width=mp.halfWidth, slack=mp.slack, q9_swap=1, n_sub_lap0=7,
                   dt_sim=0.005, mu_sim=0.05, estimator=obs_cfg(**kw))
    Qp, Rp, dRp = W.CTRL_TUNINGS["path"]
    cl = lpvmpc.BatchedSolver("controller", 20, 1 / 30.0, Qp, Rp, dRp, track=mp.PointAndTangent)
    cl.set_option("kernel_variant", KV)
    cl.observer_setup(obs_cfg(**kw))
    cl.cl_init(plant0, mp.halfWidth, mp.slack, q9_swap=True, n_sub=7, dt_sim=0.005, mu_sim=0.05)
    for t in range(40):
        path.race_tick(1); cl.cl_tick(1)
        a, b = path.race_read(), cl.cl_read()
        assert np.all(a["phase"] == 0), t
        for k in ("plant", "local", "cmd", "iters", "status"):
            assert same(a[k], b[k]), (t, k)
        for x, y in zip(path.observer_read(), cl.observer_read()):
            assert same(x, y), t
    # the controller measured the estimate, not the plant
    assert not np.array_equal(a["local"][:, 1], a["plant"][:, 3])
    close(path, tt, plan, cl)


def test_no_estimator_is_the_race():
    """race_init_observed(..., NULL) is lpvmpc_race_init, word for word, on a staggered 48-vehicle race."""
    from lpvmpc import _ffi
    mp = lshape()
    B, T = 48, 120
    plant0 = RO.start_line_fleet(mp.PointAndTangent, B, 7)
    a, fa = run_race(mp, plant0, T)
    path, tt, plan = engines(mp)
    c = _ffi.default_race_config()
    c.laps, c.half_width, c.slack = 3, mp.halfWidth, mp.slack
    p0 = np.ascontiguousarray(plant0, np.float64); ht = np.ones(B, np.int32)
    path._chk(path._lib.lpvmpc_race_init_observed(path._h, tt._h, plan._h, B, p0.ctypes.data_as(C.c_void_p), ht.ctypes.data_as(C.c_void_p),
                                                  C.byref(c), None))
    path._race = (B, 3, tt, plan)
    for t in range(T):
        path.race_tick(1)
        o = path.race_read()
        for k in ("plant", "local", "cmd", "phase", "lap", "iters", "status"):
            assert same(o[k], a[t][k]), (t, k)
        planned = a[t - 1]["phase"] >= 1 if t else np.zeros(B, bool)     # (the planner's outputs exist from its first tick on)
        for k in ("plan_iters", "plan_status"):
            assert same(o[k][planned], a[t][k][planned]), (t, k)
    ls, al = path.race_laps()
    pu, tu = path.race_predictions()
    assert same(ls, fa["lap_step"]) and same(al, fa["alive"]) and same(pu, fa["path_uPred"]) and same(tu, fa["tt_uPred"])
    assert len(set(np.argmax(np.array([o["phase"] for o in a]) >= 1, axis=0).tolist())) >= 10       # staggered events
    with pytest.raises(Exception):
        path.observer_read()                          # no estimator in this race
    close(path, tt, plan)


@pytest.mark.parametrize("noisy", [False, True])
def test_against_the_host_replay(noisy):
    """24 vehicles with their events spread over the last quarter of the lap.  Lap 0 to 2e-6, lap events on the same ticks.  In
    each vehicle's first 24 racing ticks: the same vehicles lost on the same racing tick (a planner QP turned infeasible: NaN from
    then on), equal statuses while the solve's data are finite, >= 95 % equal iteration counts, and the bars of
    test_cascade_with_observer_vs_oracle_cascade (plant, estimate, measurement 1e-5, command 1e-4) for most survivors, the
    cascade trace's loose bar 2e-2 for all of them.  The planner's open-loop recursion amplifies eps-level differences of its
    un-polished iterates: the race without an estimator has survivors beyond 1e-5 against its own replay
    in the same window on this fleet, so a vehicle is compared within its window only."""
    mp = lshape()
    B, W_ = 24, 24
    plant0 = RO.start_line_fleet(mp.PointAndTangent, B, 17, 0.85, 0.97)
    kw = dict(STD, seed=5) if noisy else {}
    path, tt, plan = engines(mp)
    path.race_init(tt, plan, plant0, half_track0=1, laps=3, half_width=mp.halfWidth, slack=mp.slack, estimator=obs_cfg(**kw))
    stds = tuple(kw.get(n + "_std", 0.0) for n in ("psi", "psiDot", "x", "y", "v"))
    ref = RO.ObservedRaceRef(RO.estimator_gains(), mp.PointAndTangent, plant0, stds=stds, seed=kw.get("seed", 0), half_track0=1, laps=3,
                             half_width=mp.halfWidth, slack=mp.slack)
    racing = np.zeros(B, int)              # racing ticks compared so far
    ev_dev = np.full(B, -1)
    worst0 = 0.0; w_state = np.zeros(B); w_cmd = np.zeros(B); same_it = n_it = 0; differs = False
    lost_dev, lost_ref, st_diff = {}, {}, []
    t = 0
    while np.any(racing < W_) and t < 200:
        path.race_tick(1); ref.tick()
        o = path.race_read(); est, _ = path.observer_read()
        rest = ref.estimate()
        ev_dev[(ev_dev < 0) & (o["phase"] >= 1)] = t
        lap0 = (o["phase"] == 0) & (ref.phase == 0)
        assert np.array_equal(o["phase"] == 0, ref.phase == 0), t
        if np.any(lap0):
            worst0 = max(worst0, float(np.max(np.abs(o["plant"][lap0] - ref.plant[lap0]))), float(np.max(np.abs(est[lap0] - rest[lap0]))),
                         float(np.max(np.abs(o["local"][lap0] - ref.local[lap0]))), float(np.max(np.abs(o["cmd"][lap0] - ref.cmd[lap0]))))
        w = (o["phase"] == 1) & (ref.phase == 1) & (ref.event_tick < t) & (racing < W_)
        for v in np.nonzero(w)[0]:
            fin_d, fin_r = np.all(np.isfinite(o["cmd"][v])), np.all(np.isfinite(ref.cmd[v]))
            if not fin_d and v not in lost_dev:
                lost_dev[int(v)] = int(racing[v])
            if not fin_r and v not in lost_ref:
                lost_ref[int(v)] = int(racing[v])
            if not (fin_d and fin_r):
                continue
            w_state[v] = max(w_state[v], float(np.max(np.abs(o["plant"][v] - ref.plant[v]))), float(np.max(np.abs(est[v] - rest[v]))),
                             float(np.max(np.abs(o["local"][v] - ref.local[v]))))
            w_cmd[v] = max(w_cmd[v], float(np.max(np.abs(o["cmd"][v] - ref.cmd[v]))))
            if o["status"][v] != ref.status[v]:
                st_diff.append((t, int(v), int(o["status"][v]), int(ref.status[v])))
            same_it += int(o["iters"][v] == ref.iters[v]); n_it += 1
        racing[w] += 1
        done = (racing >= W_) | (ref.phase >= 2) | (o["phase"] >= 2)
        racing[done] = W_
        # the measurement differs from the ground-truth measurement: the controller read the estimate
        differs = differs or bool(np.any(np.abs(est[:, 1] - o["plant"][:, 3]) > 0))
        ref.phase[done] = np.maximum(ref.phase[done], 2)                      # the replay stops a vehicle after its window
        t += 1
    surv = np.array([v not in lost_dev for v in range(B)])
    strict = surv & (w_state <= 1e-5) & (w_cmd <= 1e-4)
    print("observed race vs replay (noisy=%s): %d ticks, events %s, lap 0 %.3g, survivors within 1e-5 / 1e-4: %d of %d, worst survivor "
          "%.3g / %.3g, lost (vehicle: racing tick) %s, iterations %d / %d" % (noisy, t, sorted(ref.event_tick.tolist()), worst0, strict.sum(),
                                                                          surv.sum(), w_state[surv].max(), w_cmd[surv].max(), lost_dev, same_it, n_it))
    assert np.all(racing >= W_) and n_it > 0
    assert np.array_equal(ev_dev, ref.event_tick) and len(set(ev_dev.tolist())) >= 6
    assert worst0 <= 2e-6
    assert lost_dev == lost_ref
    assert not st_diff, st_diff
    assert same_it >= 0.95 * n_it
    assert strict.sum() >= 2 * surv.sum() // 3
    assert np.all(w_state[surv] <= 2e-2) and np.all(w_cmd[surv] <= 2e-2)
    assert differs
    close(path, tt, plan)


def test_reproducible_and_shardable():
    mp = lshape()
    B, T = 64, 90
    plant0 = RO.start_line_fleet(mp.PointAndTangent, B, 9)
    kw = dict(STD, seed=99)
    a, fa = run_race(mp, plant0, T, obs_cfg(**kw))
    b, fb = run_race(mp, plant0, T, obs_cfg(**kw))
    lo, flo = run_race(mp, plant0[:32], T, obs_cfg(vehicle_offset=0, **kw))
    hi, fhi = run_race(mp, plant0[32:], T, obs_cfg(vehicle_offset=32, **kw))
    keys = ("plant", "local", "cmd", "phase", "lap", "iters", "status", "est", "meas")
    for t in range(T):
        for k in keys:
            assert same(a[t][k], b[t][k]), (t, k)
            assert same(a[t][k], np.concatenate([lo[t][k], hi[t][k]])), (t, k)
    for k in ("lap_step", "alive"):
        assert same(fa[k], fb[k]) and same(fa[k], np.concatenate([flo[k], fhi[k]])), k
    ph = a[-1]["phase"]
    assert np.sum(ph >= 1) >= B // 2
    c, _ = run_race(mp, plant0, 3, obs_cfg(**dict(kw, seed=100)))
    assert not np.array_equal(a[2]["meas"], c[2]["meas"])


def test_frozen_and_lost():
    """A vehicle with a NaN in plant0, last in the fleet, is lost from tick 0: its plant, estimate and sensor reading never
    change, and the other vehicles equal the race of the fleet without it.  A vehicle in phase >= 2 keeps its estimate."""
    mp = lshape()
    B, T = 16, 120
    plant0 = RO.start_line_fleet(mp.PointAndTangent, B, 23, 0.9, 0.97)
    bad = np.vstack([plant0, plant0[:1]]); bad[-1, 2] = np.nan
    kw = dict(STD, seed=3)
    a, fa = run_race(mp, plant0, T, obs_cfg(**kw), laps=1)
    b, fb = run_race(mp, bad, T, obs_cfg(**kw), laps=1)
    for t in range(T):
        assert b[t]["phase"][-1] == 3 and b[t]["iters"][-1] == 0, t
        for k in ("plant", "est", "meas", "cmd", "local"):
            assert same(b[t][k][-1], b[0][k][-1]), (t, k)
        for k in ("plant", "local", "cmd", "phase", "lap", "iters", "status", "est", "meas"):
            assert same(a[t][k], b[t][k][:B]), (t, k)
    assert fb["alive"][-1] == 0 and same(fb["lap_step"][:B], fa["lap_step"])
    # phase >= 2: the estimate row stays constant from the tick it froze
    frozen = 0
    for v in range(B):
        ph = np.array([o["phase"][v] for o in a])
        if np.any(ph >= 2):
            t0 = int(np.argmax(ph >= 2))
            frozen += 1
            for t in range(t0, T):
                assert same(a[t]["est"][v], a[t0]["est"][v]) and same(a[t]["plant"][v], a[t0]["plant"][v]), (v, t)
    print("frozen / lost vehicles in the window:", frozen)


def test_refusals_and_lifetime():
    import lpvmpc
    from lpvmpc import _ffi
    mp = lshape()
    p0 = RO.grid_fleet(4, 1)
    kw = dict(half_width=mp.halfWidth, slack=mp.slack)
    path, tt, plan = engines(mp)

    def refused(fn, *a, **k):
        with pytest.raises(lpvmpc.LpvMpcError) as e:
            fn(*a, **k)
        return str(e.value)

    path.observer_setup(obs_cfg())
    assert "obs argument" in refused(path.race_init, tt, plan, p0, estimator=obs_cfg(), **kw)
    assert "estimator" in refused(path.race_init, tt, plan, p0, **kw)
    path.observer_setup(None)
    bad = obs_cfg(); bad.loop_rate = 0.0
    assert "loop_rate" in refused(path.race_init, tt, plan, p0, estimator=bad, **kw)
    bad = obs_cfg(); bad.x_std = -1.0
    assert "standard deviations" in refused(path.race_init, tt, plan, p0, estimator=bad, **kw)
    with pytest.raises(TypeError):
        path.race_init(tt, plan, p0, estimator=obs_cfg(), no_such_option=1, **kw)
    with pytest.raises(TypeError):
        path.race_init(tt, plan, p0, estimator={"seed": 1}, **kw)
    # observer_read on a race without an estimator
    path.race_init(tt, plan, p0, **kw)
    path.race_tick(2)
    refused(path.observer_read)
    path.cl_release()
    # with one; cl_release frees it: observer_read is refused and the handle's next fleet runs on ground truth
    path.race_init(tt, plan, p0, estimator=obs_cfg(**STD), **kw)
    path.race_tick(3)
    est, meas = path.observer_read()
    assert est.shape == (4, 6) and meas.shape == (4, 5) and np.all(np.isfinite(est))
    path.cl_release()
    refused(path.observer_read)
    path.cl_init(p0, mp.halfWidth, mp.slack, n_sub=7)
    path.cl_tick(12)
    from lpvmpc import workloads as W
    Qp, Rp, dRp = W.CTRL_TUNINGS["path"]
    fresh = lpvmpc.BatchedSolver("controller", 20, 1 / 30.0, Qp, Rp, dRp, track=mp.PointAndTangent)
    fresh.set_option("kernel_variant", KV)
    fresh.cl_init(p0, mp.halfWidth, mp.slack, n_sub=7)
    fresh.cl_tick(12)
    x, y = path.cl_read(), fresh.cl_read()
    for k in ("plant", "local", "cmd", "iters", "status"):
        assert same(x[k], y[k]), k
    refused(path.observer_read)
    path.cl_release()
    # destroying a handle the race drives ends the race and its estimator
    path.race_init(tt, plan, p0, estimator=obs_cfg(), **kw)
    path.race_tick(1)
    plan.close()
    refused(path.race_tick, 1)
    refused(path.observer_read)
    close(path, tt, fresh)
    # RaceFleet with an estimator
    f = lpvmpc.RaceFleet(mp, p0, laps=1, half_track0=0, estimator=obs_cfg(**STD), kernel_variant=KV)
    f.run(5)
    est, meas = f.estimate()
    assert est.shape == (4, 6) and np.all(np.isfinite(est)) and np.all(f.state()["phase"] == 0)
    f.close()


def test_full_size_from_the_grid():
    """1024 noisy vehicles from the grid, 900 ticks: alive <=> finite plant and estimate, frozen vehicles stay frozen, laps are
    monotone, and the estimate tracks the plant of the alive vehicles (the bars of test_noisy_fleet_runs_and_the_estimate_tracks_the_plant)."""
    mp = lshape()
    B, T = 1024, 900
    plant0 = RO.grid_fleet(B, 12)
    path, tt, plan = engines(mp)
    path.race_init(tt, plan, plant0, half_track0=0, laps=1, half_width=mp.halfWidth, slack=mp.slack, estimator=obs_cfg(**STD, seed=21))
    prev = path.race_read(); prev_est, _ = path.observer_read()
    frozen = {}
    tracked = 0
    for t in range(T):
        path.race_tick(1)
        o = path.race_read(); est, meas = path.observer_read()
        live = (o["phase"] <= 1) & np.all(np.isfinite(o["plant"]), axis=1) & np.all(np.isfinite(est), axis=1)
        if t % 150 == 149 and np.sum(live) >= B // 2:
            # the estimate follows the plant of the vehicles still racing
            e, p = est[live], o["plant"][live]
            assert np.median(np.abs(e[:, 3] - p[:, 0])) < 10 * 0.5 * STD["x_std"], t
            assert np.median(np.abs(e[:, 4] - p[:, 1])) < 10 * 0.5 * STD["y_std"], t
            assert np.median(np.abs(e[:, 5] - p[:, 6])) < 10 * 0.5 * STD["psi_std"], t
            assert np.median(np.abs(e[:, 0] - p[:, 2])) < 10 * 0.5 * STD["v_std"] + 0.05, t
            tracked += 1
        assert np.all(o["phase"] >= prev["phase"]) and np.all(o["lap"] >= prev["lap"]), t
        # a vehicle is lost exactly when it entered the tick with a non-finite plant or estimate
        fin = np.all(np.isfinite(prev["plant"]), axis=1) & np.all(np.isfinite(prev_est), axis=1)
        entered = prev["phase"] <= 1
        assert np.array_equal(o["phase"][entered] == 3, ~fin[entered]), t
        for b in np.nonzero(o["phase"] >= 2)[0]:
            b = int(b)
            row = (o["plant"][b].copy(), est[b].copy(), meas[b].copy(), o["cmd"][b].copy())
            if b in frozen:
                assert all(same(x, y) for x, y in zip(row, frozen[b])), (t, b)
            else:
                frozen[b] = row
        prev, prev_est = o, est
    ls, alive = path.race_laps()
    ph = prev["phase"]
    print("full size: phases", np.bincount(ph, minlength=4).tolist())
    assert np.sum(ph >= 1) >= B // 2
    for b in range(B):
        reached = ls[b][ls[b] >= 0]
        assert np.all(np.diff(reached) > 0) and ls[b, 0] == 0
    assert tracked >= 4
    assert np.sum(alive) > 0 and np.all(alive <= T)
    close(path, tt, plan)
