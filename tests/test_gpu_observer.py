"""GPU tests of the gain-scheduled LPV estimator (observer.hip): the batched observer step and the drop-in class against the
reference fixture and the numpy restatement, and the f1 fleet with the estimator and the sensors in the loop."""
import os

import numpy as np
import pytest

from tests import _observer_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FIX = os.path.join(HERE, "golden", "estimator", "estimator.npz")
N_SUB = 7


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(FIX))


def gains(fx):
    return {k: fx[k] for k in ("L_ls", "lim_ls", "L_hs", "lim_hs")}


def cfg_of(fx, **kw):
    from lpvmpc.observer import observer_config
    return observer_config(fx["L_ls"], fx["lim_ls"], fx["L_hs"], fx["lim_hs"], **kw)


def fleet_engine():
    import lpvmpc
    from lpvmpc import workloads
    Q, Rm, dR = workloads.CTRL_TUNINGS["path"]
    mp = lpvmpc.Map("oval", 0.2)
    return lpvmpc.BatchedSolver("controller", 20, 1 / 30.0, Q, Rm, dR, track=mp.PointAndTangent), mp


def fleet_start(eng, B, seed=3):
    rng = np.random.default_rng(seed)
    s0 = rng.uniform(0.05, 12.5, B); ey0 = rng.normal(0, 0.03, B)
    xyth = eng.global_position(np.column_stack([s0, ey0]))
    return s0, np.column_stack([xyth[:, 0], xyth[:, 1], rng.uniform(0.8, 1.2, B), np.zeros(B), np.zeros(B), np.zeros(B),
                                xyth[:, 2], np.zeros(B)])


def run_fleet(fx, plant0, ticks, obs_kw=None, setup_then_remove=False):
    eng, mp = fleet_engine()
    if obs_kw is not None or setup_then_remove:
        eng.observer_setup(cfg_of(fx, **(obs_kw or {})))
    if setup_then_remove:
        eng.observer_setup(None)
    eng.cl_init(plant0, mp.halfWidth, mp.slack, q9_swap=True, n_sub=N_SUB)
    eng.cl_tick(ticks)
    o = eng.cl_read()
    o["est"], o["meas"] = eng.observer_read() if obs_kw is not None else (None, None)
    eng.close()
    return o


def test_observer_step_batch_matches_restatement_and_fixture(fx):
    import lpvmpc
    eng, _ = fleet_engine()
    cfg = cfg_of(fx)
    g, dt = gains(fx), float(fx["dt"])
    rng = np.random.default_rng(11)
    B = 4096
    n0 = len(fx["grid_k"])
    est = np.empty((B, 6)); y = np.empty((B, 5)); u = np.empty((B, 2)); k = np.empty(B, np.int32)
    est[:n0], y[:n0], u[:n0], k[:n0] = fx["grid_est"], fx["grid_y"], fx["grid_u"], fx["grid_k"]
    m = B - n0
    est[n0:] = np.column_stack([rng.uniform(0.05, 5.0, m), rng.uniform(-0.6, 0.6, m), rng.uniform(-4, 4, m),
                                rng.uniform(-5, 5, m), rng.uniform(-5, 5, m), rng.uniform(-6, 6, m)])
    y[n0:] = est[n0:, [0, 2, 3, 4, 5]] + rng.normal(0, 0.1, (m, 5))
    y[n0:, 0] = np.abs(y[n0:, 0]) + 0.05
    u[n0:] = np.column_stack([rng.uniform(-0.5, 0.5, m), rng.uniform(-1, 1, m)])
    k[n0:] = rng.integers(1, 400, m)
    new, (L, A, Bm) = eng.observer_step(cfg, est, y, u, k, want_aux=True)
    for i in range(n0):
        for got, want in ((new[i], fx["grid_new"][i]), (L[i], fx["grid_L"][i]), (A[i], fx["grid_A"][i]), (Bm[i], fx["grid_B"][i])):
            assert np.max(np.abs(got - want)) <= 1e-12 * max(1.0, np.max(np.abs(want))), i
    worst = 0.0
    for i in range(B):
        xn, Lr, Ar, Br = R.observer_step(g, est[i], y[i], u[i], int(k[i]), dt)
        scale = max(1.0, np.max(np.abs(xn)))
        worst = max(worst, np.max(np.abs(new[i] - xn)) / scale, np.max(np.abs(L[i] - Lr)) / max(1.0, np.max(np.abs(Lr))))
    assert worst <= 1e-12, worst
    # both polytopes, start-up steps and points outside the polytopes are covered
    vx = np.where(k * dt > 0.02, est[:, 0], y[:, 0])
    assert (vx > fx["lim_ls"][0, 1]).sum() > 100 and (vx <= fx["lim_ls"][0, 1]).sum() > 100
    assert (k <= 4).sum() > 20 and (vx > fx["lim_hs"][0, 1]).sum() > 100
    eng.close()
    # like the other batch calls, it is refused while the handle runs a fleet
    eng, mp = fleet_engine()
    _, plant0 = fleet_start(eng, 4)
    eng.cl_init(plant0, mp.halfWidth, mp.slack)
    with pytest.raises(lpvmpc.LpvMpcError):
        eng.observer_step(cfg, est[:4], y[:4], u[:4], k[:4])
    eng.close()


def test_drop_in_observer_reproduces_the_reference_trace(fx):
    from lpvmpc import GainScheduledLPVObserver
    ob = GainScheduledLPVObserver(fx["L_ls"], fx["lim_ls"], fx["L_hs"], fx["lim_hs"], loop_rate=200.0, init_vx=0.2)
    assert np.array_equal(ob.states_est, fx["trace_est0"])
    for k in range(len(fx["trace_u"])):
        ob.GS_LPV_Est(ob.states_est, fx["trace_y"][k], fx["trace_u"][k])
        want = fx["trace_est"][k]
        assert np.max(np.abs(ob.states_est - want)) <= 1e-10 * max(1.0, np.max(np.abs(want))), k
    assert ob.index == len(fx["trace_u"]) and ob.L_gain.shape == (6, 5) and ob.A_obs.shape == (6, 6) and ob.B_obs.shape == (6, 2)
    assert (ob.vx_est, ob.yaw_est) == (ob.states_est[0], ob.states_est[5])
    ob.close()


def replay(fx, plant0, ticks, obs_kw, vid0=0):
    """Run a fleet one tick at a time and restate, on the host, the plant (oracle/plant_ref.py) and the sensors + observer
    (tests/_observer_ref.py) under the commands the fleet applied.  Returns the worst plant / estimate deviation."""
    from oracle import plant_ref as P
    eng, mp = fleet_engine()
    eng.observer_setup(cfg_of(fx, **obs_kw))
    eng.cl_init(plant0, mp.halfWidth, mp.slack, q9_swap=True, n_sub=N_SUB)
    B = plant0.shape[0]
    stds = [obs_kw.get(n + "_std", 0.0) for n in R.CHANNELS]
    veh = [R.Vehicle(gains(fx), plant0[b], init_vx=obs_kw.get("init_vx", 0.2), stds=stds, n_bound=obs_kw.get("n_bound", 0.5),
                     seed=obs_kw.get("seed", 0), vid=vid0 + b) for b in range(B)]
    host = plant0.copy()
    worst_p = worst_e = worst_y = 0.0
    for t in range(ticks):
        est_before = np.array([v.est for v in veh])
        eng.cl_tick(1)
        o = eng.cl_read()
        est, meas = eng.observer_read()
        # this tick's controller measurement was made from the estimate at its start
        assert np.max(np.abs(o["local"][:, :3] - np.column_stack([np.maximum(est_before[:, 0], 0.01), est_before[:, 1:3]]))) <= 2e-6
        for b in range(B):
            servo, motor = o["cmd"][b]
            for _ in range(N_SUB):
                host[b] = P.simulator_f(host[b], [motor, servo])
                veh[b].substep(host[b], servo, motor)
        worst_p = max(worst_p, np.max(np.abs(o["plant"] - host)))
        worst_e = max(worst_e, np.max(np.abs(est - np.array([v.est for v in veh]))))
        worst_y = max(worst_y, np.max(np.abs(meas - np.array([v.y for v in veh]))))
        host = o["plant"].copy()                  # the host plant follows the fleet's: each tick's plant step is checked on its own
    eng.close()
    return worst_p, worst_e, worst_y, veh


def test_fleet_with_observer_matches_host_restatement(fx):
    eng, _ = fleet_engine()
    _, plant0 = fleet_start(eng, 8, seed=5)
    eng.close()
    wp, we, wy, _ = replay(fx, plant0, 40, {})
    assert wp <= 2e-6 and we <= 2e-6 and wy <= 2e-6, (wp, we, wy)


def test_fleet_noise_matches_restatement_and_is_clipped(fx):
    eng, _ = fleet_engine()
    _, plant0 = fleet_start(eng, 6, seed=6)
    eng.close()
    kw = dict(psi_std=0.02, psiDot_std=0.05, x_std=0.01, y_std=0.01, v_std=0.03, n_bound=0.5, seed=1234)
    wp, we, wy, veh = replay(fx, plant0, 12, kw, vid0=0)
    assert wp <= 2e-6 and we <= 2e-6 and wy <= 2e-6, (wp, we, wy)
    draws = np.array([d for v in veh for d in v.draws]).reshape(-1, 5)
    lim = 0.5 * np.array([0.02, 0.05, 0.01, 0.01, 0.03])
    assert np.all(np.abs(draws) <= lim + 1e-15) and np.all(np.max(np.abs(draws), axis=0) == lim)


def test_noise_is_reproducible_and_independent_of_sharding(fx):
    eng, _ = fleet_engine()
    _, plant0 = fleet_start(eng, 64, seed=8)
    eng.close()
    kw = dict(psi_std=0.02, psiDot_std=0.05, x_std=0.01, y_std=0.01, v_std=0.03, seed=99)
    a = run_fleet(fx, plant0, 12, kw)
    b = run_fleet(fx, plant0, 12, kw)
    lo = run_fleet(fx, plant0[:32], 12, dict(kw, vehicle_offset=0))
    hi = run_fleet(fx, plant0[32:], 12, dict(kw, vehicle_offset=32))
    for key in ("plant", "est", "meas", "cmd", "iters"):
        assert np.array_equal(a[key], b[key]), key
        assert np.array_equal(a[key], np.concatenate([lo[key], hi[key]])), key
    c = run_fleet(fx, plant0, 12, dict(kw, seed=100))
    assert not np.array_equal(a["meas"], c["meas"])


def test_noisy_fleet_runs_and_the_estimate_tracks_the_plant(fx):
    import lpvmpc
    eng, _ = fleet_engine()
    s0, plant0 = fleet_start(eng, 512, seed=3)
    eng.close()
    mp = lpvmpc.Map("oval", 0.2)
    std = dict(psi_std=0.01, psiDot_std=0.05, x_std=0.01, y_std=0.01, v_std=0.02)
    o = run_fleet(fx, plant0, 60, dict(std, seed=7))
    assert np.mean(np.isin(o["status"], (1, 2))) > 0.98
    ds = (o["local"][:, 4] - s0) % mp.TrackLength
    assert np.all(o["local"][:, 4] < 9999) and np.median(ds) > 1.0
    # the estimate follows the plant: position within 10 x the clipped GPS noise bound (0.5 x_std), yaw within 10 x the
    # clipped IMU bound, speed within 10 x the encoder bound plus the unmeasured vy
    est, p = o["est"], o["plant"]
    assert np.median(np.abs(est[:, 3] - p[:, 0])) < 10 * 0.5 * std["x_std"]
    assert np.median(np.abs(est[:, 4] - p[:, 1])) < 10 * 0.5 * std["y_std"]
    assert np.median(np.abs(est[:, 5] - p[:, 6])) < 10 * 0.5 * std["psi_std"]
    assert np.median(np.abs(est[:, 0] - p[:, 2])) < 10 * 0.5 * std["v_std"] + 0.05


def test_observer_removed_runs_like_a_handle_that_never_had_one(fx):
    eng, _ = fleet_engine()
    _, plant0 = fleet_start(eng, 16, seed=4)
    eng.close()
    a = run_fleet(fx, plant0, 15, None)
    b = run_fleet(fx, plant0, 15, None, setup_then_remove=True)
    for key in ("plant", "local", "cmd", "iters", "status"):
        assert np.array_equal(a[key], b[key]), key
    # and the estimator does change the loop
    c = run_fleet(fx, plant0, 15, {})
    assert not np.array_equal(a["plant"], c["plant"])


def test_device_noise_and_gps_hold_match_the_documented_generator(fx):
    """Per key, the draws the fleet adds (latest measurement minus the plant) equal the numpy restatement of the generator to
    1e-12, and the GPS reading is refreshed exactly on the steps the reference's publish counter allows."""
    eng, _ = fleet_engine()
    _, plant0 = fleet_start(eng, 48, seed=12)
    eng.close()
    std = dict(psi_std=0.02, psiDot_std=0.05, x_std=0.01, y_std=0.01, v_std=0.03)
    seed, voff, nb = 4242, 1000, 0.5
    eng, mp = fleet_engine()
    eng.observer_setup(cfg_of(fx, seed=seed, vehicle_offset=voff, n_bound=nb, **std))
    eng.cl_init(plant0, mp.halfWidth, mp.slack, q9_swap=True, n_sub=N_SUB)
    # the reference counter (SIM:296-305) with thUpdate = (1 / 1000) / 0.005: published on these steps
    cnt, th, pub_steps = 0, (1.0 / 1000.0) / 0.005, set()
    for k in range(1, 6 * N_SUB + 1):
        if cnt > th:
            cnt = 0; pub_steps.add(k)
        else:
            cnt += 1
    assert pub_steps == set(range(2, 6 * N_SUB + 1, 2))
    for t in range(1, 7):
        eng.cl_tick(1)
        o = eng.cl_read()
        _, meas = eng.observer_read()
        p, k = o["plant"], t * N_SUB
        vids = voff + np.arange(len(p))
        want = {ch: np.array([R.noise(std[R.CHANNELS[ch] + "_std"], nb, seed, int(v), k, ch) for v in vids]) for ch in range(5)}
        assert np.max(np.abs((meas[:, 4] - p[:, 6]) - want[0])) <= 1e-12
        assert np.max(np.abs((meas[:, 1] - p[:, 7]) - want[1])) <= 1e-12
        assert np.max(np.abs((meas[:, 0] - np.sqrt(p[:, 2] ** 2 + p[:, 3] ** 2)) - want[4])) <= 1e-12
        for ch, col, pc in ((2, 2, 0), (3, 3, 1)):
            d = meas[:, col] - p[:, pc]
            if k in pub_steps:                           # refreshed on this step: plant + this step's draw
                assert np.max(np.abs(d - want[ch])) <= 1e-12
            else:                                        # held from the previous step
                assert np.min(np.abs(d - want[ch])) > 1e-9
        for ch in range(5):
            lim = nb * std[R.CHANNELS[ch] + "_std"]
            assert np.all(np.abs(want[ch]) <= lim)
    eng.close()


class ObservedCascadeRef(object):
    """The oracle cascade (oracle/cascade_ref.py) with the restated sensors + estimator in the loop: both nodes measure the
    estimate in the plant's layout, the plant advances under the command with one sensor + observer step per plant step."""

    def __init__(self, g, *a, **k):
        from oracle import cascade_ref as CR
        self.ref = CR.CascadeRef(*a, **k)
        self.true = self.ref.plant.copy()
        self.veh = [R.Vehicle(g, p, est0=[p[2], p[3], p[7], p[0], p[1], p[6]]) for p in self.true]
        self.ref.plant = self.view()

    def view(self):
        return np.array([[v.est[3], v.est[4], v.est[0], v.est[1], 0.0, 0.0, v.est[5], v.est[2]] for v in self.veh])

    def tick(self):
        from oracle import osqp_ref, plant_ref as PR
        r = self.ref
        B, Nc = r.B, r.Nc
        while r.plan_ticks < (2 * r.k) // 3 + 1:
            r.planner_tick()
        vel = np.empty((B, Nc + 1)); curv = np.empty((B, Nc))
        for b in range(B):
            r.local[b], v, c = r.glue[b].measure(r.plant[b], r.refs[b])
            vel[b, :Nc] = v; vel[b, Nc] = v[-1]; curv[b] = c
        w = dict(N=Nc, dt=r.dtc, Q=r.Qc, R=r.Rc, dR=r.dRc, track=r.track, x0=r.local.copy(), u_prev=r.uPred,
                 vel_ref=vel, curv_s=curv, u_old=r.cmd.copy(), cf_new=60.0, lap=1)
        r.ctrl = osqp_ref.ctrl_tick_batch(w, nthreads=r.nthreads)
        r.uPred = r.ctrl["uPred"]
        r.cmd = r.uPred[:, 0, :].copy()
        for b in range(B):
            st = self.true[b]
            for _ in range(r.n_sub[r.k % 3]):
                st = PR.simulator_f(st, [r.cmd[b, 1], r.cmd[b, 0]])
                self.veh[b].substep(st, r.cmd[b, 0], r.cmd[b, 1])
            self.true[b] = st
        r.plant = self.view()
        r.k += 1


def test_cascade_with_observer_vs_oracle_cascade(fx):
    """8 vehicles, 24 controller ticks of the racing cascade with the estimator in the loop against the oracle cascade with the
    restated estimator; the bars of tests/test_gpu_cascade.py::test_cascade_fleet_vs_oracle."""
    import lpvmpc
    from lpvmpc import workloads as W
    from tests._golden import load
    c = load("cascade")
    B = 8
    rng = np.random.default_rng(11)
    plant0 = np.tile(c["plant0"], (B, 1))
    plant0[:, 1] += rng.normal(0, 0.015, B); plant0[:, 2] += rng.uniform(-0.05, 0.3, B); plant0[:, 6] += rng.normal(0, 0.015, B)
    cmd0 = np.tile(c["cmd0"], (B, 1)); uPred0 = np.tile(c["uPred0"], (B, 1, 1))
    mp = lpvmpc.Map("L_shape", 0.2)
    plan = lpvmpc.BatchedSolver("planner", 40, 0.05, W.PLAN_Q, W.PLAN_R, W.PLAN_dR, L_cf=W.PLAN_L, track=mp.PointAndTangent)
    plan.handoff_setup()
    Q, Rm, dR = W.CTRL_TUNINGS["race"]
    ctrl = lpvmpc.BatchedSolver("controller", 20, 1 / 30.0, Q, Rm, dR, track=mp.PointAndTangent)
    ctrl.observer_setup(cfg_of(fx))
    ctrl.cascade_init(plan, plant0, cmd0, uPred0, lap0=1, half_width=mp.halfWidth, slack=mp.slack, plan_max_ey=0.2, q9_swap=True)
    ref = ObservedCascadeRef(gains(fx), mp.PointAndTangent, W.CTRL_TUNINGS["race"], (W.PLAN_Q, W.PLAN_R, W.PLAN_dR, W.PLAN_L), plant0,
                             cmd0, uPred0, half_width=mp.halfWidth, slack=mp.slack, plan_max_ey=0.2, nthreads=4)
    same_iters = 0
    for k in range(24):
        ctrl.cascade_tick(1); ref.tick()
        o = ctrl.cascade_read(full=False)
        est, _ = ctrl.observer_read()
        assert np.max(np.abs(o["plant"] - ref.true)) <= 1e-5, k
        assert np.max(np.abs(est - np.array([v.est for v in ref.veh]))) <= 1e-5, k
        assert np.max(np.abs(o["local"] - ref.ref.local)) <= 1e-5, k
        assert np.max(np.abs(o["cmd"] - ref.ref.cmd)) <= 1e-4, k
        assert np.array_equal(o["status"], ref.ref.ctrl["status"])
        same_iters += int(np.sum(o["iters"] == ref.ref.ctrl["iters"]))
    assert same_iters >= 0.95 * 24 * B
    # the controller measured the estimate, not the plant
    assert np.max(np.abs(est[:, 1] - o["plant"][:, 3])) > 0
    ctrl.close(); plan.close()
    # closing a cascade with an estimator leaves no pending HIP error behind: the next handle's launches succeed
    eng, _ = fleet_engine()
    w = W.controller_batch(4, N=20, seed=1)
    eng.lpv(w["x0"], w["u_prev"], w["vel_ref"], w["curv_s"], w["cf_new"], w["lap"])
    eng.close()
