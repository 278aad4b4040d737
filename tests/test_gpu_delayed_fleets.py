"""GPU: the fleets with the actuator in the plant and delayed controllers (lpvmpc_cl_init_actuated, lpvmpc_race_init_actuated):
the all-off configuration equals the old entry points word for word, the controllers' OldSteering histories follow the list
recursion exactly, the pinned steering rows hold in closed loop, the plant equals the host restatement of the actuator under the
commands the fleet issued, per-vehicle delays equal uniform fleets, the race's lap-0 ticks equal the delayed lap-0 fleet and its
event tick shows the reference's [0, .., 0, last servo] quirk, frozen vehicles keep their actuator, and the refusals."""
import numpy as np
import pytest

from tests import _actuator_ref as AR
from tests import _race_observer_ref as RO

pytestmark = pytest.mark.gpu

KV = 0
STD = dict(psi_std=0.01, psiDot_std=0.05, x_std=0.01, y_std=0.01, v_std=0.02)
PINNED_TOL = 1e-3      # equality rows of the QP: held to the solver's primal tolerance (eps_abs = eps_rel = 1e-3, OSQP defaults)


def lshape():
    import lpvmpc
    return lpvmpc.Map("L_shape", 0.2)


def obs_cfg(**kw):
    from lpvmpc.observer import observer_config
    g = RO.estimator_gains()
    return observer_config(g["L_ls"], g["lim_ls"], g["L_hs"], g["lim_hs"], **kw)


def ctrl(mp, role="path", d=0):
    import lpvmpc
    from lpvmpc import workloads as W
    Q, R, dR = W.CTRL_TUNINGS[role]
    kw = {"steering_delay": d} if d else {}
    e = lpvmpc.BatchedSolver("controller", 20, 1 / 30.0, Q, R, dR, track=mp.PointAndTangent, **kw)
    e.set_option("kernel_variant", KV)
    return e


def engines(mp, d=0):
    import lpvmpc
    from lpvmpc import workloads as W
    plan = lpvmpc.BatchedSolver("planner", 40, 0.05, W.PLAN_Q, W.PLAN_R, W.PLAN_dR, L_cf=W.PLAN_L, track=mp.PointAndTangent)
    plan.set_option("kernel_variant", KV)
    plan.handoff_setup()
    return ctrl(mp, "path", d), ctrl(mp, "race", d), plan


def close(*es):
    for e in es:
        e.close()


def same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def cl_run(mp, plant0, T, act=None, d=0, est=None, **kw):
    e = ctrl(mp, "path", d)
    if est is not None:
        e.observer_setup(est)
    e.cl_init(plant0, mp.halfWidth, mp.slack, q9_swap=True, n_sub=7, actuator=act, **kw)
    out = []
    for _ in range(T):
        e.cl_tick(1)
        o = e.cl_read()
        if est is not None:
            o["est"], o["meas"] = e.observer_read()
        if act is not None:
            o.update(e.actuator_read())
        out.append(o)
    e.close()
    return out


@pytest.mark.parametrize("est", [False, True])
def test_all_off_is_the_old_lap0_fleet(est):
    """cl_init(actuator=all off) with steeringDelay 0 equals cl_init, word for word, over 60 ticks (with the estimator: also its state)."""
    import lpvmpc
    mp = lshape()
    plant0 = RO.grid_fleet(48, 3)
    oc = obs_cfg(**dict(STD, seed=5)) if est else None
    a = cl_run(mp, plant0, 60, est=oc)
    b = cl_run(mp, plant0, 60, act=lpvmpc.actuator_config(), est=oc)
    for t in range(60):
        for k in ("plant", "local", "cmd", "iters", "status") + (("est", "meas") if est else ()):
            assert same(a[t][k], b[t][k]), (t, k)
        assert same(b[t]["path"], b[t]["cmd"])                 # d = 0: the history is the last command
    assert b[-1]["act_state"][0, -1] == 60 * 7


@pytest.mark.parametrize("est", [False, True])
def test_all_off_is_the_old_race(est):
    """race_init(actuator=all off) equals race_init / race_init_observed word for word over 90 ticks of a staggered race."""
    import lpvmpc
    mp = lshape()
    B, T = 24, 90
    plant0 = RO.start_line_fleet(mp.PointAndTangent, B, 7)
    oc = obs_cfg(**dict(STD, seed=9)) if est else None
    res = []
    for act in (None, lpvmpc.actuator_config()):
        path, tt, plan = engines(mp)
        path.race_init(tt, plan, plant0, half_track0=1, laps=2, half_width=mp.halfWidth, slack=mp.slack, estimator=oc, actuator=act)
        rows = []
        for _ in range(T):
            path.race_tick(1)
            o = path.race_read()
            if est:
                o["est"], o["meas"] = path.observer_read()
            rows.append(o)
        rows.append(dict(zip(("path_uPred", "tt_uPred"), path.race_predictions())))
        res.append(rows)
        close(path, tt, plan)
    a, b = res
    for t in range(T):
        for k in ("plant", "local", "cmd", "phase", "lap", "iters", "status") + (("est", "meas") if est else ()):
            assert same(a[t][k], b[t][k]), (t, k)
    assert same(a[T]["path_uPred"], b[T]["path_uPred"]) and same(a[T]["tt_uPred"], b[T]["tt_uPred"])
    assert np.any(a[T - 1]["phase"] >= 1)


def replay_plant(plant0, cmds, La, Ld, lld, n_sub=7):
    """Host restatement of one vehicle's plant under the fleet's commands, each held n_sub steps through the actuator."""
    act = AR.Actuator(La, Ld, lld)
    st = np.array(plant0, float)
    from oracle import plant_ref as PR
    for s, m in cmds:
        for _ in range(n_sub):
            st = PR.simulator_f(st, act.step(m, s))
    return st, act


@pytest.mark.parametrize("d,lld", [(1, False), (3, True), (3, False)])
def test_delayed_lap0_fleet(d, lld):
    """Plant delays La = 6 / Ld = 4 steps with a controller of steeringDelay d over 40 ticks: the read-back history equals the list
    recursion of the issued commands exactly; every tick the command's steering (uPred[0]) is the pinned OldSteering[1] of the
    history its solve read (to the solver's tolerance); the plant and the actuator state equal the host restatement under the
    issued commands word for word."""
    import lpvmpc
    mp = lshape()
    B, T = 16, 40
    plant0 = RO.grid_fleet(B, 21)
    rows = cl_run(mp, plant0, T, act=lpvmpc.actuator_config(0.03, 0.02, low_level_dyn=lld), d=d)
    hist = np.zeros((B, 2 + d))
    hist = np.array([AR.uold_push(h, 0.0, 0.0) for h in hist])            # tick 0's measurement pushes the initial command (0, 0)
    worst_pin = worst_plant = 0.0
    for t in range(T):
        cmd = rows[t]["cmd"]
        worst_pin = max(worst_pin, float(np.max(np.abs(cmd[:, 0] - hist[:, 2]))))      # uPred[0, steer] = OldSteering[1]
        hist = np.array([AR.uold_push(hist[b], cmd[b, 0], cmd[b, 1]) for b in range(B)])
        assert same(rows[t]["path"], hist), t
    assert np.all(rows[-1]["status"] == 1)
    for b in range(B):
        st, act = replay_plant(plant0[b], [r["cmd"][b] for r in rows], 6, 4, lld)
        worst_plant = max(worst_plant, float(np.max(np.abs(st - rows[-1]["plant"][b]))))
        assert st.tobytes() == rows[-1]["plant"][b].tobytes(), b             # word for word (the objects build with -ffp-contract=off)
        assert act.words().tobytes() == rows[-1]["act_state"][b].tobytes() and rows[-1]["act_state"][b, -1] == T * 7
    print("d %d lld %d: pinned |u - OldSteering[1]| <= %.2e, plant vs restatement <= %.2e" % (d, lld, worst_pin, worst_plant))
    assert worst_pin <= PINNED_TOL


@pytest.mark.parametrize("d,lld,est", [(1, False, False), (3, True, False), (3, False, False), (3, True, True)])
def test_delayed_lap0_fleet_matches_the_replay(d, lld, est):
    """The delayed lap-0 fleet (La = 6 / Ld = 4 steps, steeringDelay d, servo lag on / off, with and without the estimator) against
    the host replay (tests/_delayed_race_ref.py: the reference's FIFOs, the list recursion, the QP with d pinned rows) over 40
    ticks: plant, measurement and command to 2e-6 with identical iteration counts and statuses, and the history the next solve
    reads to 2e-6 (the device's equals the list recursion of its own commands exactly, test_delayed_lap0_fleet)."""
    import lpvmpc
    from tests._delayed_race_ref import delayed_lap0_replay
    mp = lshape()
    B, T = 16, 40
    plant0 = RO.grid_fleet(B, 21)
    stds = (0.01, 0.05, 0.01, 0.01, 0.02)
    oc = obs_cfg(**dict(STD, seed=3)) if est else None
    rows = cl_run(mp, plant0, T, act=lpvmpc.actuator_config(0.03, 0.02, low_level_dyn=lld), d=d, est=oc)
    ref = delayed_lap0_replay(mp.PointAndTangent, plant0, steering_delay=d, delay_a=6, delay_df=4, low_level_dyn=lld, laps=1,
                              half_width=mp.halfWidth, slack=mp.slack, **(dict(gains=RO.estimator_gains(), stds=stds, seed=3) if est else {}))
    worst = 0.0
    for t in range(T):
        ref.tick()
        o = rows[t]
        assert np.all(ref.phase == 0), t
        assert np.array_equal(o["iters"], ref.iters) and np.array_equal(o["status"], ref.status), t
        nxt = np.array([AR.uold_push(ref.p_hist[b], ref.cmd[b, 0], ref.cmd[b, 1]) for b in range(B)])
        worst = max(worst, *(float(np.max(np.abs(o[k] - v))) for k, v in (("plant", ref.plant), ("local", ref.local), ("cmd", ref.cmd),
                                                                           ("path", nxt))))
        if est:
            worst = max(worst, float(np.max(np.abs(o["est"] - ref.estimate()))))
    print("d %d lld %d est %d: fleet vs replay %.2e over %d ticks" % (d, lld, est, worst, T))
    assert worst <= 2e-6


@pytest.mark.parametrize("est", [False, True])
def test_delayed_race_matches_the_replay(est):
    """12 vehicles with staggered lap events, plant delays La = 4 / Ld = 6 with the servo lag, steeringDelay 3 on path and tt,
    on ground truth and with the estimator fed the commanded input, against the host replay (tests/_delayed_race_ref.py): lap 0 to 2e-6, lap events
    on the same ticks, and in each vehicle's first 24 racing ticks the bars of test_gpu_race_observer.test_against_the_host_replay
    (same vehicles lost, equal statuses, >= 95 % equal iteration counts, plant / measurement 1e-5 and command 1e-4 for most
    survivors, 2e-2 for all: the planner recursion's amplification).  Where a solve leaves its pinned rows loose (an un-polished
    ADMM iterate meets OSQP's relative stopping rule), the replay's same solve leaves them as loose: every device pin error is
    within 1e-3 of the replay's."""
    import lpvmpc
    from tests._delayed_race_ref import DelayedRaceRef
    mp = lshape()
    B, W_, d = 12, 24, 3
    plant0 = RO.start_line_fleet(mp.PointAndTangent, B, 17, 0.85, 0.97)
    stds = (0.01, 0.05, 0.01, 0.01, 0.02)
    path, tt, plan = engines(mp, d)
    path.race_init(tt, plan, plant0, half_track0=1, laps=3, half_width=mp.halfWidth, slack=mp.slack,
                   estimator=obs_cfg(**dict(STD, seed=5)) if est else None, actuator=lpvmpc.actuator_config(0.02, 0.03, low_level_dyn=True))
    ref = DelayedRaceRef(mp.PointAndTangent, plant0, steering_delay=d, delay_a=4, delay_df=6, low_level_dyn=True, half_track0=1, laps=3,
                         half_width=mp.halfWidth, slack=mp.slack, **(dict(gains=RO.estimator_gains(), stds=stds, seed=5) if est else {}))
    racing = np.zeros(B, int)
    ev_dev = np.full(B, -1)
    worst0 = 0.0; w_state = np.zeros(B); w_cmd = np.zeros(B); same_it = n_it = 0
    lost_dev, lost_ref, st_diff, pin_gap = {}, {}, [], 0.0
    err0 = np.zeros(B)                                                        # absolute lap-0 error per vehicle
    t = 0
    while np.any(racing < W_) and t < 200:
        ph_before = ref.phase.copy()
        path.race_tick(1); ref.tick()
        o = path.race_read()
        e_dev, e_ref = (path.observer_read()[0], ref.estimate()) if est else (o["plant"], ref.plant)
        h = path.actuator_read(); pu, tu = path.race_predictions()
        ev_dev[(ev_dev < 0) & (o["phase"] == 1)] = t
        lap0 = (o["phase"] == 0) & (ref.phase == 0)
        assert np.array_equal(o["phase"] == 0, ref.phase == 0), t
        lost0 = (ph_before == 0) & (o["phase"] == 3)
        assert np.array_equal(lost0, (ph_before == 0) & (ref.phase == 3)), t       # lost in lap 0 on the same tick
        if np.any(lap0):
            for a_, b_ in ((o["plant"], ref.plant), (e_dev, e_ref), (o["local"], ref.local), (o["cmd"], ref.cmd), (h["path"], ref.p_hist)):
                e_ = np.abs(a_[lap0] - b_[lap0]).max(axis=1)
                worst0 = max(worst0, float(np.max(e_ / np.maximum(1.0, np.abs(b_[lap0]).max(axis=1)))))
                for v, ev in zip(np.nonzero(lap0)[0], e_):
                    err0[v] = max(err0[v], float(ev))
            assert np.array_equal(o["iters"][lap0], ref.iters[lap0]) and np.array_equal(o["status"][lap0], ref.status[lap0]), t
        for v in range(B):                                    # pinned rows against the replay's same solve
            if t < 9 or o["iters"][v] == 0 or ph_before[v] != o["phase"][v] or o["phase"][v] >= 2:
                continue                                      # seed ticks, no solve, event / finishing tick
            if o["phase"][v] == 0:
                dv = np.abs(pu[v, :d, 0] - h["path"][v, 2:]); rv = np.abs(ref.uPred_path[v][:d, 0] - ref.p_hist[v, 2:])
            elif racing[v] < W_ and ref.phase[v] == 1:
                dv = np.abs(tu[v, :d, 0] - h["tt"][v, 2:]); rv = np.abs(ref.casc[v].uPred[0, :d, 0] - ref.t_hist[v, 2:])
            else:
                continue
            if np.all(np.isfinite(dv)) and np.all(np.isfinite(rv)):
                pin_gap = max(pin_gap, float(np.max(dv) - np.max(rv)))
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
        ref.phase[done] = np.maximum(ref.phase[done], 2)                      # the replay stops a vehicle after its window
        t += 1
    surv = np.array([v not in lost_dev for v in range(B)])
    strict = surv & (w_state <= 1e-5) & (w_cmd <= 1e-4)
    print("delayed race vs replay (estimator %s): %d ticks, events %s, lap 0 %.3g, survivors within 1e-5 / 1e-4: %d of %d, worst survivor %.3g / %.3g, "
          "lost %s, iterations %d / %d, pin error beyond the replay's %.3g" % (est, t, sorted(ref.event_tick.tolist()), worst0, strict.sum(), surv.sum(),
                                                                                 w_state[surv].max(), w_cmd[surv].max(), lost_dev, same_it, n_it, pin_gap))
    # every vehicle that had its event was compared over its window; vehicles still in lap 0 after 200 ticks were compared there
    assert np.all((racing >= W_) | (ev_dev < 0)) and n_it > 0 and np.sum(ev_dev >= 0) >= 8
    assert np.array_equal(ev_dev, ref.event_tick) and len(set(ev_dev[ev_dev >= 0].tolist())) >= 4
    # lap 0 to 2e-6 for the vehicles that reach their lap event.  A vehicle that leaves the track in lap 0 is held, like a vehicle
    # lost in its racing window, to being lost on the same tick with equal statuses and iteration counts on every tick before
    # (asserted above): its state grows until it turns non-finite, and round-off grows with it
    kept = np.array([ref.phase[v] != 3 or ref.event_tick[v] >= 0 for v in range(B)])
    print("lap 0: worst absolute of the vehicles that reach their event %.3g; of the vehicles lost in lap 0 %s (relative %.3g)"
          % (err0[kept].max(), err0[~kept], worst0))
    assert kept.sum() >= 8 and np.all(err0[kept] <= 2e-6)
    assert lost_dev == lost_ref
    assert not st_diff, st_diff
    assert same_it >= 0.95 * n_it
    assert strict.sum() >= 2 * surv.sum() // 3
    assert np.all(w_state[surv] <= 2e-2) and np.all(w_cmd[surv] <= 2e-2)
    assert pin_gap <= 1e-3
    close(path, tt, plan)


def test_per_vehicle_delays_equal_uniform_fleets():
    """A fleet with mixed per-vehicle (La, Ld) equals, vehicle for vehicle and bit for bit, fleets run with each uniform pair; a
    rerun is bit-identical, and so is the fleet run as two halves."""
    import lpvmpc
    mp = lshape()
    pairs = [(0, 0), (6, 4), (20, 20), (64, 28)]
    B, T = 16, 30
    plant0 = RO.grid_fleet(B, 4)
    La = np.array([pairs[b % 4][0] for b in range(B)]); Ld = np.array([pairs[b % 4][1] for b in range(B)])
    cfg = lpvmpc.actuator_config(low_level_dyn=True)
    mixed = cl_run(mp, plant0, T, act=cfg, d=3, delay_a=La, delay_df=Ld)
    again = cl_run(mp, plant0, T, act=cfg, d=3, delay_a=La, delay_df=Ld)
    halves = [cl_run(mp, plant0[s], T, act=cfg, d=3, delay_a=La[s], delay_df=Ld[s]) for s in (slice(0, 8), slice(8, 16))]
    for t in range(T):
        for k in ("plant", "local", "cmd", "iters", "status", "path", "act_state"):
            assert same(mixed[t][k], again[t][k]), (t, k)
            assert same(mixed[t][k], np.concatenate([halves[0][t][k], halves[1][t][k]])), (t, k)
    for p, (la, ld) in enumerate(pairs):
        idx = np.nonzero((La == la) & (Ld == ld))[0]
        u = cl_run(mp, plant0[idx], T, act=_steps_cfg(la, ld, True), d=3)
        for t in range(T):
            for k in ("plant", "local", "cmd", "iters", "status", "path", "act_state"):
                assert same(mixed[t][k][idx], u[t][k]), (p, t, k)


def _steps_cfg(la, ld, lld):
    import lpvmpc
    c = lpvmpc.actuator_config(low_level_dyn=lld)
    c.delay_a, c.delay_df = la, ld
    return c


@pytest.mark.parametrize("est", [False, True])
def test_delayed_race(est):
    """A race with plant delays and steeringDelay 3 on path and tt: before any lap event it equals the delayed lap-0 fleet word for
    word (with the estimator: fed the commanded input in both); on each vehicle's event tick tt's history is [0, .., 0, last servo]
    with OldAccelera = last motor, and tt's first d - 1 pinned steerings read those zeros; on every tick each solving
    controller's uPred[i, steer] for i < d equals its OldSteering[i + 1] where the solve converged (status 1; on ground truth)."""
    import lpvmpc
    mp = lshape()
    d = 3
    act = lpvmpc.actuator_config(0.02, 0.03, low_level_dyn=True)
    oc = obs_cfg(**dict(STD, seed=13)) if est else None
    # lap 0 from the grid: the delayed fleet
    B = 16
    plant0 = RO.grid_fleet(B, 8)
    path, tt, plan = engines(mp, d)
    path.race_init(tt, plan, plant0, half_track0=0, laps=1, half_width=mp.halfWidth, slack=mp.slack, estimator=oc, actuator=act)
    fleet = cl_run(mp, plant0, 40, act=act, d=d, est=oc)
    for t in range(40):
        path.race_tick(1)
        a = path.race_read()
        assert np.all(a["phase"] == 0), t
        for k in ("plant", "local", "cmd", "iters", "status"):
            assert same(a[k], fleet[t][k]), (t, k)
        r = path.actuator_read()
        assert same(r["act_state"], fleet[t]["act_state"]), t
    close(path, tt, plan)
    # staggered lap events
    B, T = 12, 110
    plant0 = RO.start_line_fleet(mp.PointAndTangent, B, 17)
    path, tt, plan = engines(mp, d)
    path.race_init(tt, plan, plant0, half_track0=1, laps=2, half_width=mp.halfWidth, slack=mp.slack, estimator=oc, actuator=act)
    prev_cmd, prev_phase = np.zeros((B, 2)), np.zeros(B, int)
    events = unsolved = 0
    worst, errs = 0.0, []
    for t in range(T):
        path.race_tick(1)
        o = path.race_read()
        h = path.actuator_read()
        pu, tu = path.race_predictions()
        for b in range(B):
            if o["iters"][b] == 0 or (t < 9 and o["lap"][b] != 0):
                continue      # did not solve this tick; or an event inside the 9 seed ticks, where `path` solves (ControllerNode.step)
            hist, up = (h["path"][b], pu[b]) if o["lap"][b] == 0 else (h["tt"][b], tu[b])
            steer = [hist[0]] + list(hist[2:])
            if o["status"][b] == 1:                               # pinned rows hold where the solver converged
                err = float(np.max(np.abs(up[:d, 0] - steer[1:])))
                errs.append(err)
                worst = max(worst, err)
            else:
                unsolved += 1
            if prev_phase[b] == 0 and o["phase"][b] == 1 and t >= 9:
                events += 1
                s, m = prev_cmd[b]
                assert same(h["tt"][b], np.array([0.0, m] + [0.0] * (d - 1) + [s])), (t, b)
        prev_cmd, prev_phase = o["cmd"].copy(), o["phase"].copy()
    errs = np.array(errs)
    print("events seen: %d, pinned rows within %.2e on solved ticks (%.1f%% within %.0e), %d unsolved vehicle-ticks"
          % (events, worst, 100 * np.mean(errs <= PINNED_TOL), PINNED_TOL, unsolved))
    assert events >= 4 and unsolved <= B * T // 20
    if not est:
        assert worst <= PINNED_TOL
    # with the estimator some solves end un-polished; test_delayed_race_matches_the_replay holds those pins to the replay's
    close(path, tt, plan)


def test_frozen_and_lost_keep_their_actuator():
    """A lost vehicle (NaN in plant0) never advances its actuator state; a finished vehicle's state stays put from the tick it froze."""
    import lpvmpc
    mp = lshape()
    B, T = 8, 150
    plant0 = RO.start_line_fleet(mp.PointAndTangent, B, 23, 0.9, 0.97)
    bad = np.vstack([plant0, plant0[:1]]); bad[-1, 2] = np.nan
    path, tt, plan = engines(mp, 2)
    path.race_init(tt, plan, bad, half_track0=1, laps=1, half_width=mp.halfWidth, slack=mp.slack,
                   actuator=lpvmpc.actuator_config(0.02, 0.02, low_level_dyn=True))
    frozen_at = {}
    for t in range(T):
        path.race_tick(1)
        o = path.race_read()
        a = path.actuator_read()["act_state"]
        assert o["phase"][-1] == 3 and np.all(a[-1] == 0), t
        for v in range(B):
            if o["phase"][v] >= 2:
                if v not in frozen_at:
                    frozen_at[v] = a[v].copy()
                assert same(a[v], frozen_at[v]), (t, v)
    close(path, tt, plan)


def test_refusals():
    """Old entries still refuse delayed handles with their messages; the cascade refuses them; delays above the cap, negative ones,
    path / tt of different delays and per-vehicle arrays of the wrong length are refused."""
    import lpvmpc
    mp = lshape()
    plant0 = RO.grid_fleet(4, 1)
    e = ctrl(mp, "path", 2)
    with pytest.raises(lpvmpc.LpvMpcError) as x:
        e.cl_init(plant0, mp.halfWidth, mp.slack)
    assert "steeringDelay" in str(x.value)
    bad = lpvmpc.actuator_config(); bad.delay_df = 65
    with pytest.raises(lpvmpc.LpvMpcError):
        e.cl_init(plant0, mp.halfWidth, mp.slack, actuator=bad)
    with pytest.raises(lpvmpc.LpvMpcError):
        e.cl_init(plant0, mp.halfWidth, mp.slack, actuator=lpvmpc.actuator_config(), delay_a=[0, 1, -1, 0])
    with pytest.raises(ValueError):
        e.cl_init(plant0, mp.halfWidth, mp.slack, actuator=lpvmpc.actuator_config(), delay_a=[0, 1, 2])
    e.close()
    path, tt, plan = engines(mp, 2)
    with pytest.raises(lpvmpc.LpvMpcError) as x:
        path.race_init(tt, plan, plant0, half_width=mp.halfWidth, slack=mp.slack)
    assert "steeringDelay" in str(x.value)
    tt1 = ctrl(mp, "race", 1)
    with pytest.raises(lpvmpc.LpvMpcError) as x:
        path.race_init(tt1, plan, plant0, half_width=mp.halfWidth, slack=mp.slack, actuator=lpvmpc.actuator_config())
    assert "steeringDelay" in str(x.value)
    with pytest.raises(ValueError):
        path.race_init(tt, plan, plant0, half_width=mp.halfWidth, slack=mp.slack, actuator=lpvmpc.actuator_config(), delay_df=[1, 2])
    with pytest.raises(lpvmpc.LpvMpcError) as x:
        tt.cascade_init(plan, plant0[:1], np.zeros((1, 2)), np.zeros((1, 20, 2)))
    assert "steeringDelay" in str(x.value)
    # a refused call leaves the handles usable: the race starts
    path.race_init(tt, plan, plant0, half_track0=0, half_width=mp.halfWidth, slack=mp.slack, actuator=lpvmpc.actuator_config())
    path.race_tick(2)
    assert path.actuator_read()["act_state"][0, -1] == 14
    close(path, tt, plan, tt1)
