"""GPU: sensor faults (lpvmpc_set_sensor_faults, lpvmpc_sensor_faults_read, lpvmpc_sensor_step_batch).  All-off rows change no word of
a lap-0 fleet or a race (the faulted kernels restate the fused observe kernels: this holds the two together); the stand-alone step
matches the numpy restatement (tests/_sensor_faults_ref.py) under the bar tests/test_gpu_observer.py holds the device step to (1e-12,
relative), counters and stuck / zero readings exactly; the random loss draws the restatement's pattern; draws are independent of
sharding; faulted fleets and races match the host replay under the bars of the tyre model's tests; snapshot, restore, clone; refusals."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import _race_observer_ref as RO
from tests import _sensor_faults_ref as F
from tests import _tyre_ref as T
from tests.test_gpu_delayed_fleets import STD, close, ctrl, engines, lshape, obs_cfg, same
from tests.test_gpu_plant_params import RACE_KEYS, _race_same

pytestmark = pytest.mark.gpu

STDS = (0.01, 0.05, 0.01, 0.01, 0.02)          # STD in the restatement's channel order
STEP_BAR = 1e-12                               # tests/test_gpu_observer.py: the device step against _observer_ref, relative to max(1, |x|)
DT = 0.005


def bind_estimator(e, rows):
    """Per-vehicle estimator rows with gain tables designed on the device (lpvmpc_set_observer_vehicles)."""
    from lpvmpc.api import observer_design_config
    g = RO.estimator_gains()
    e.set_observer_vehicles(rows, design=observer_design_config(g["lim_ls"], g["lim_hs"]))


# ---- 1. all-off rows attached against nothing attached ------------------------------------------------------------------------
def cl_run(mp, plant0, n_ticks, est, faults=None, attach_tick=0, obsveh=None, **kw):
    e = ctrl(mp)
    e.observer_setup(est)
    if obsveh is not None:
        bind_estimator(e, obsveh)
    e.cl_init(plant0, mp.halfWidth, mp.slack, q9_swap=True, n_sub=7, **kw)
    out = []
    for t in range(n_ticks):
        if faults is not None and t == attach_tick:
            e.set_sensor_faults(**faults)
        e.cl_tick(1)
        o = e.cl_read()
        o["est"], o["meas"] = e.observer_read()
        o.update(e.actuator_read())
        out.append(o)
    e.close()
    return out


CL_KEYS = ("plant", "local", "cmd", "iters", "status", "act_state", "path", "est", "meas")


@pytest.mark.parametrize("obsveh", [False, True], ids=["config", "per_vehicle"])
def test_all_off_lap0_fleet_is_the_healthy_fleet(obsveh):
    """B = 67 (a ragged second wavefront), estimator with noise, 12 ticks: every word the reads return is equal."""
    import lpvmpc
    mp = lshape()
    B, n = 67, 12
    plant0 = RO.grid_fleet(B, 3)
    prow = lpvmpc.sample_plant_params(B, 5)
    kw = dict(plant_params=prow, tyre_params=lpvmpc.sample_tyre_params(B, 5), est=obs_cfg(**dict(STD, seed=5)), obsveh=prow if obsveh else None)
    a = cl_run(mp, plant0, n, **kw)
    b = cl_run(mp, plant0, n, faults=dict(rows=F.off(B), seed=11), **kw)
    for t in range(n):
        for k in CL_KEYS:
            assert same(a[t][k], b[t][k]), (t, k)
    assert not same(a[n - 1]["est"][:, 3], a[n - 1]["plant"][:, 0])         # the sensors are noisy


def race_run(mp, plant0, n_ticks, est, faults=None, obsveh=None, **kw):
    path, tt, plan = engines(mp)
    if obsveh is not None:
        bind_estimator(path, obsveh)
    path.race_init(tt, plan, plant0, laps=2, half_width=mp.halfWidth, slack=mp.slack, estimator=est, **kw)
    if faults is not None:
        path.set_sensor_faults(**faults)
    out = []
    for _ in range(n_ticks):
        path.race_tick(1)
        o = path.race_read()
        o["est"], o["meas"] = path.observer_read()
        o.update(path.actuator_read())
        out.append(o)
    last = dict(zip(("path_uPred", "tt_uPred"), path.race_predictions()))
    last.update(zip(("lap_step", "alive"), path.race_laps()))
    out.append(last)
    close(path, tt, plan)
    return out


@pytest.mark.parametrize("obsveh", [False, True], ids=["config", "per_vehicle"])
def test_all_off_race_is_the_healthy_race(obsveh):
    import lpvmpc
    mp = lshape()
    B, n = 5, 30
    plant0 = RO.start_line_fleet(mp.PointAndTangent, B, 7, 0.975, 0.985)
    prow = lpvmpc.sample_plant_params(B, 4)
    kw = dict(half_track0=1, plant_params=prow, tyre_params=lpvmpc.tyre_params(B), est=obs_cfg(**dict(STD, seed=9)), obsveh=prow if obsveh else None)
    a = race_run(mp, plant0, n, **kw)
    b = race_run(mp, plant0, n, faults=dict(rows=F.off(B), seed=3), **kw)
    _race_same(a, b, n, RACE_KEYS + ("est", "meas", "act_state", "path", "tt"))
    assert np.any(a[n - 1]["phase"] == 1)                                   # through a lap event


# ---- 2. the stand-alone step against the restatement ---------------------------------------------------------------------------
ENC_WIN, GPS_OUT, JUMP_WIN = (7.0, 45.0), (10.0, 9.0), (12.0, 6.0)


def component_rows(B):
    """Vehicle b carries fault b % 8: none, the GPS outage, the jump, the bias, the drift, the scale, the stuck encoder, all of them."""
    rows = F.off(B)
    q = np.arange(B) % 8
    al = q == 7
    rows[(q == 1) | al, 0:2] = GPS_OUT
    rows[(q == 2) | al, 3:7] = JUMP_WIN + (0.4, -0.3)
    rows[(q == 3) | al, 7] = 0.07
    rows[(q == 4) | al, 8] = 0.3
    rows[(q == 5) | al, 9] = 0.9
    rows[(q == 6) | al, 10:12] = ENC_WIN
    return rows, q


def plant_path(B, steps, seed):
    """[steps + 1, B, 8]: the oracle plant from the grid under a held command per vehicle."""
    from oracle import plant_ref as PR
    st = RO.grid_fleet(B, seed)
    u = np.column_stack([np.full(B, 0.6), np.where(np.arange(B) % 2, 0.15, -0.15)])
    out = [st.copy()]
    for _ in range(steps):
        st = np.array([PR.simulator_f(st[b], u[b]) for b in range(B)])
        out.append(st)
    return np.array(out), u


@pytest.mark.parametrize("noisy", [False, True], ids=["launch_file", "noisy"])
def test_step_matches_the_restatement(noisy):
    """B = 65, 70 chained device steps; per step the restatement starts from the device's state before the step.  The launch file's
    sensor settings (every std 0, GPS at 1000 Hz, n_bound 0.5): y, the GPS hold, the encoder words and the counters are exact, the
    estimate within 1e-12.  With noise: y and the hold within 1e-12 too (libm's log / cos), counters, stuck and zero readings exact."""
    mp = lshape()
    B, steps = 65, 70
    rows, q = component_rows(B)
    path_, u = plant_path(B, steps, 6)
    okw = dict(STD, seed=31, vehicle_offset=4) if noisy else {}
    cfg = obs_cfg(**okw)
    g = RO.estimator_gains()
    veh = [F.FaultedVehicle(g, path_[0][b], stds=STDS if noisy else (0, 0, 0, 0, 0), seed=okw.get("seed", 0), vid=okw.get("vehicle_offset", 0) + b,
                            row=rows[b], fault_seed=77, fault_vid=9 + b) for b in range(B)]
    state = np.array([v.state() for v in veh])
    e = ctrl(mp)
    worst = 0.0
    seen_zero, seen_stuck, held = set(), set(), {}
    for k in range(1, steps + 1):
        new = e.sensor_step(cfg, state, path_[k], u[:, 1], u[:, 0], rows=rows, seed=77, vehicle_offset=9)
        for b in range(B):
            v = veh[b]
            v.load(state[b])
            v.substep(path_[k][b], u[b, 1], u[b, 0])
            want = v.state()
            assert np.array_equal(new[b, 15:18], want[15:18]), (k, b)                        # GPS counter, encoder counter, k
            assert (new[b, 14] == 0.0) == (want[14] == 0.0), (k, b)
            if not noisy:
                assert same(new[b, 6:15], want[6:15]), (k, b, new[b, 6:15] - want[6:15])
            err = np.abs(new[b, :15] - want[:15]) / np.maximum(1.0, np.abs(want[:15]))
            worst = max(worst, float(err.max()))
        stuck = (q == 6) | (q == 7)
        if ENC_WIN[0] <= k < sum(ENC_WIN):
            assert np.array_equal(new[stuck, 13], state[stuck, 13]), k                       # the previous reading, delivered again
            assert np.all(new[stuck, 16] == k - ENC_WIN[0] + 1)
            assert np.all((new[stuck, 14] == 0.0) == (k - ENC_WIN[0] + 1 >= 41)), k          # reads 0 from the 41st stuck step on
            seen_zero |= {k} if np.all(new[stuck, 14] == 0.0) else set()
        elif k >= sum(ENC_WIN):
            assert np.all(new[stuck, 14] != 0.0) and np.all(new[stuck, 16] == 0), k          # the first step after the window reads again
        out = (q == 1) | (q == 7)
        if k == GPS_OUT[0] - 1:
            held = new[out, 11:13].copy()
        if GPS_OUT[0] <= k < sum(GPS_OUT):
            assert same(new[out, 11:13], held), k
            seen_stuck.add(k)
        if k == sum(GPS_OUT) + 1:                                                            # step 20 publishes
            assert not np.any(new[out, 11:13] == held)
        if not noisy and k in (12, 14, 16):                                                  # publications inside the jump window
            assert same(new[q == 2, 11], path_[k][q == 2, 0] + 0.0 + 0.4) and same(new[q == 2, 12], path_[k][q == 2, 1] + 0.0 - 0.3)
        if not noisy and k > 4:
            assert same(new[q == 3, 7], path_[k][q == 3, 7] + 0.0 + 0.07)
            assert same(new[q == 4, 10], path_[k][q == 4, 6] + 0.0 + 0.3 * (k * DT))
        state = new
    print("sensor step (%s): worst relative deviation %.3e over %d steps" % ("noisy" if noisy else "launch file", worst, steps))
    assert worst <= STEP_BAR
    assert seen_zero == set(range(47, 52)) and seen_stuck == set(range(10, 19))
    # healthy rows == NULL, and the per-vehicle estimator form on off rows
    a = e.sensor_step(cfg, state, path_[steps], u[:, 1], u[:, 0])
    b = e.sensor_step(cfg, state, path_[steps], u[:, 1], u[:, 0], rows=F.off(B), seed=5)
    assert same(a, b)
    e.close()
    import lpvmpc
    e = ctrl(mp)
    bind_estimator(e, lpvmpc.sample_plant_params(B, 8))
    a = e.sensor_step(cfg, state, path_[steps], u[:, 1], u[:, 0])
    b = e.sensor_step(cfg, state, path_[steps], u[:, 1], u[:, 0], rows=F.off(B), seed=5)
    c = e.sensor_step(cfg, state, path_[steps], u[:, 1], u[:, 0], rows=rows, seed=77, vehicle_offset=9)
    assert same(a, b) and not same(a, c)
    with pytest.raises(lpvmpc.LpvMpcError):
        e.sensor_step(cfg, state[:8], path_[steps][:8], u[:8, 1], u[:8, 0])             # another B than the binding's
    e.close()


# ---- 3. random loss ------------------------------------------------------------------------------------------------------------
LOSS_B, LOSS_PUBS, LOSS_P, LOSS_VOFF = 4096, 40, 0.3, 1000


def loss_reference():
    """The restatement's loss pattern [LOSS_PUBS, LOSS_B] for the first seed under which no draw lies within 1e-9 of z."""
    from lpvmpc.sensor_faults import loss_z
    z = loss_z(LOSS_P)
    for seed in range(1, 20):
        g = np.array([[F.loss_gauss(seed, LOSS_VOFF + b, 2 * j) for b in range(LOSS_B)] for j in range(1, LOSS_PUBS + 1)])
        excluded = int(np.sum(np.abs(g - z) < 1e-9))
        if excluded == 0:
            return seed, z, g > z, excluded
    raise AssertionError("no seed without a draw within 1e-9 of z")


def test_random_loss_draws_the_restatements_pattern():
    """4096 vehicles x 40 publishing steps at p = 0.3 on the launch file's sensors (publications on the even steps): a publication is
    taken exactly when the hold equals this step's plant position.  The seed is chosen on the CPU so that no draw is excluded."""
    seed, z, want, excluded = loss_reference()
    assert excluded == 0
    mp = lshape()
    B = LOSS_B
    rows = F.off(B); rows[:, 2] = z
    cfg = obs_cfg()
    g = RO.estimator_gains()
    st0 = np.tile([0.0, 0.2, 1.0, 0.0, 0.0, 0.0, 0.1, 0.0], (B, 1)); st0[:, 0] = 1e-5 * np.arange(B)
    state = np.array([F.FaultedVehicle(g, st0[b]).state() for b in range(B)])
    e = ctrl(mp)
    got = np.zeros_like(want)
    for k in range(1, 2 * LOSS_PUBS + 1):
        st = st0.copy(); st[:, 0] += 0.01 * k
        state = e.sensor_step(cfg, state, st, 0.0, 0.3, rows=rows, seed=seed, vehicle_offset=LOSS_VOFF)
        taken = state[:, 11] == st[:, 0]
        if k % 2:
            assert not np.any(taken), k                                     # silent steps
        else:
            got[k // 2 - 1] = ~taken
    e.close()
    assert np.array_equal(got, want), int(np.sum(got != want))
    share, n = float(got.mean()), got.size
    bar = 5.0 * math.sqrt(LOSS_P * (1.0 - LOSS_P) / n)
    print("random loss: seed %d, z %.6f, lost share %.5f (p %.2f, bar %.5f), excluded %d" % (seed, z, share, LOSS_P, bar, excluded))
    assert abs(share - LOSS_P) <= bar


# ---- 4. sharding ---------------------------------------------------------------------------------------------------------------
def test_faults_do_not_depend_on_sharding():
    """A 64-vehicle lap-0 fleet with sampled faults and a random loss over 12 ticks equals its two 32-vehicle shards with
    vehicle_offset 0 / 32 bit for bit."""
    import lpvmpc
    mp = lshape()
    B, n, h = 64, 12, 32
    plant0 = RO.grid_fleet(B, 6)
    rows = lpvmpc.sample_faults(B, 4, spread=dict(gps_outage_t0=(0.05, 0.2), gps_outage_len=(0.05, 0.2), imu_w_bias=(-0.05, 0.05), gps_loss_p=(0.2, 0.5)))
    prow, tyres = lpvmpc.sample_plant_params(B, 4), lpvmpc.sample_tyre_params(B, 4)

    def run(lo, hi, faults=True):
        return cl_run(mp, plant0[lo:hi], n, obs_cfg(**dict(STD, seed=13, vehicle_offset=lo)), plant_params=prow[lo:hi], tyre_params=tyres[lo:hi],
                      faults=dict(rows=rows[lo:hi], seed=21, vehicle_offset=lo) if faults else None)

    whole, a, b = run(0, B), run(0, h), run(h, B)
    for t in range(n):
        for k in CL_KEYS:
            assert same(whole[t][k], np.concatenate([a[t][k], b[t][k]])), (t, k)
    quiet = run(0, B, faults=False)
    assert np.all(np.any(whole[n - 1]["est"] != quiet[n - 1]["est"], axis=1))


# ---- 5. lap-0 fleet against the host replay ------------------------------------------------------------------------------------
def test_faulted_lap0_fleet_matches_the_replay():
    """8 vehicles, 30 ticks (210 observer steps), a 1 s GPS outage (steps 5 .. 204) and a biased gyro against the host replay (the
    oracle plant + the restatement): plant, measurement, command and estimate within 2e-6, identical iteration counts and statuses
    (test_pacejka_lap0_fleet_matches_the_replay's rule).  After tick 28 (observer step 203, inside the outage's last steps) the position estimate is further
    from the plant than in the healthy run, on the device and in the replay."""
    import lpvmpc
    mp = lshape()
    B, n = 8, 30
    plant0 = RO.grid_fleet(B, 21)
    prow, tyres = lpvmpc.sample_plant_params(B, 17), lpvmpc.sample_tyre_params(B, 17)
    rows = lpvmpc.fault_rows(B, DT, gps_outage=(0.025, 1.0), imu_w_bias=0.05)
    assert rows[:, 0:2].tolist() == [[5.0, 200.0]] * B
    oc = obs_cfg(**dict(STD, seed=3))
    e, h = ctrl(mp), ctrl(mp)
    for x in (e, h):
        x.observer_setup(oc)
        x.cl_init(plant0, mp.halfWidth, mp.slack, q9_swap=True, n_sub=7, plant_params=prow, tyre_params=tyres)
    e.set_sensor_faults(rows, seed=41, vehicle_offset=3)
    assert same(e.sensor_faults(), rows) and h.sensor_faults() is None
    rkw = dict(plant_params=prow, tyre_params=tyres, half_track0=0, laps=1, half_width=mp.halfWidth, slack=mp.slack, gains=RO.estimator_gains(),
               stds=STDS, seed=3)
    ref = F.FaultedRaceRef(mp.PointAndTangent, plant0, rows, fault_seed=41, fault_offset=3, **rkw)
    quiet = T.TyreRaceRef(mp.PointAndTangent, plant0, **rkw)
    def pos_err(est, plant):
        return np.hypot(est[:, 3] - plant[:, 0], est[:, 4] - plant[:, 1])

    worst = 0.0
    for t in range(n):
        e.cl_tick(1); h.cl_tick(1); ref.tick(); quiet.tick()
        o = e.cl_read()
        assert np.all(ref.phase == 0), t
        assert np.array_equal(o["iters"], ref.iters) and np.array_equal(o["status"], ref.status), t
        worst = max(worst, *(float(np.max(np.abs(o[k] - v))) for k, v in (("plant", ref.plant), ("local", ref.local), ("cmd", ref.cmd))))
        worst = max(worst, float(np.max(np.abs(e.observer_read()[0] - ref.estimate()))))
        if t == 28:                                                         # observer step 203: the outage's last steps
            d_f, d_h = pos_err(e.observer_read()[0], o["plant"]), pos_err(h.observer_read()[0], h.cl_read()["plant"])
            r_f, r_h = pos_err(ref.estimate(), ref.plant), pos_err(quiet.estimate(), quiet.plant)
    print("faulted lap-0 fleet: vs replay %.2e over %d ticks; position error at the end of the outage: device %.3g (healthy %.3g), replay %.3g "
          "(healthy %.3g)" % (worst, n, d_f.min(), d_h.max(), r_f.min(), r_h.max()))
    assert worst <= 2e-6
    assert np.all(d_f > d_h) and np.all(r_f > r_h)
    assert all(v.k == 210 for v in ref.veh)
    close(e, h)


# ---- 6. race against the host replay -------------------------------------------------------------------------------------------
RACE_SEED = 17


def race_rows(B):
    import lpvmpc
    return lpvmpc.fault_rows(B, DT, gps_outage=(0.6, 0.25), imu_w_bias=0.03, gps_loss_p=0.2, enc_scale=0.98)


def test_faulted_race_matches_the_replay():
    """8 vehicles on the launch file's Pacejka tyre with the estimator through their lap events, faults attached at tick 10, against the
    host replay under test_pacejka_race_matches_the_replay's rule: lap 0 within 2e-6, the same event ticks, the same vehicles lost, and
    in each survivor's first 24 racing ticks two thirds within 1e-5 / 1e-4, all within 2e-2, >= 95 % equal iteration counts, equal
    statuses (its vehicle counts, 8 of 12, are two thirds of the fleet: here 5 of 8)."""
    import lpvmpc
    mp = lshape()
    B, W_, attach = 8, 24, 10
    plant0 = RO.start_line_fleet(mp.PointAndTangent, B, RACE_SEED, 0.90, 0.975)
    prow, tyres = lpvmpc.sample_plant_params(B, 23), lpvmpc.tyre_params(B)
    rows = race_rows(B)
    path, tt, plan = engines(mp)
    path.race_init(tt, plan, plant0, half_track0=1, laps=3, half_width=mp.halfWidth, slack=mp.slack, plant_params=prow, tyre_params=tyres,
                   estimator=obs_cfg(**dict(STD, seed=7)))
    ref = F.FaultedRaceRef(mp.PointAndTangent, plant0, rows, fault_seed=5, attach_tick=attach, tyre_params=tyres, plant_params=prow, half_track0=1,
                           laps=3, half_width=mp.halfWidth, slack=mp.slack, gains=RO.estimator_gains(), stds=STDS, seed=7)
    racing = np.zeros(B, int)
    ev_dev = np.full(B, -1)
    w_state = np.zeros(B); w_cmd = np.zeros(B); same_it = n_it = 0
    lost_dev, lost_ref, st_diff = {}, {}, []
    err0 = np.zeros(B)
    t = 0
    while np.any(racing < W_) and t < 200:
        if t == attach:
            path.set_sensor_faults(rows, seed=5)
        ph_before = ref.phase.copy()
        path.race_tick(1); ref.tick()
        o = path.race_read()
        ev_dev[(ev_dev < 0) & (o["phase"] == 1)] = t
        lap0 = (o["phase"] == 0) & (ref.phase == 0)
        assert np.array_equal(o["phase"] == 0, ref.phase == 0), t
        lost0 = (ph_before == 0) & (o["phase"] == 3)
        assert np.array_equal(lost0, (ph_before == 0) & (ref.phase == 3)), t
        if np.any(lap0):
            est = path.observer_read()[0]
            for a_, b_ in ((o["plant"], ref.plant), (o["local"], ref.local), (o["cmd"], ref.cmd), (est, ref.estimate())):
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
    n_lost_pubs = sum(1 for v in ref.veh for _, lost in v.lost if lost)
    print("faulted race vs replay: %d ticks, events %s, lap 0 worst %.3g, survivors within 1e-5 / 1e-4: %d of %d, worst survivor %.3g / %.3g, "
          "lost %s, iterations %d / %d, lost publications %d" % (t, sorted(ref.event_tick.tolist()), err0[kept].max(), strict.sum(), surv.sum(),
                                                                 w_state[surv].max(), w_cmd[surv].max(), lost_dev, same_it, n_it, n_lost_pubs))
    assert surv_ref.sum() >= need                                                           # the replay alone, on the CPU
    assert np.all((racing >= W_) | (ev_dev < 0)) and n_it > 0 and np.sum(ev_dev >= 0) >= need
    assert np.array_equal(ev_dev, ref.event_tick) and len(set(ev_dev[ev_dev >= 0].tolist())) >= 4
    assert kept.sum() >= need and np.all(err0[kept] <= 2e-6)
    assert lost_dev == lost_ref
    assert not st_diff, st_diff
    assert same_it >= 0.95 * n_it
    assert strict.sum() >= 2 * surv.sum() // 3
    assert np.all(w_state[surv] <= 2e-2) and np.all(w_cmd[surv] <= 2e-2)
    assert n_lost_pubs > 0 and np.all(ev_dev[ev_dev >= 0] > attach)
    assert same(path.sensor_faults(), rows)
    close(path, tt, plan)


def faulted_fleet(B, rows=None, stds=STD, laps=2, plant0=None, **kw):
    import lpvmpc
    mp = lshape()
    if plant0 is None:
        plant0 = RO.start_line_fleet(mp.PointAndTangent, B, 7, 0.97, 0.985)
    return lpvmpc.RaceFleet(mp, plant0, laps=laps, half_track0=1, kernel_variant=0, tyre_params=lpvmpc.tyre_params(B),
                            estimator=obs_cfg(init_vx=1.0, **dict(stds, seed=5)), sensor_faults=None if rows is None else dict(rows=rows, seed=9), **kw)


def race_reads(f, n):
    out = []
    for _ in range(n):
        f.run(1)
        o = f.state()
        o["est"], o["meas"] = f.estimate()
        o["act_state"] = f.actuator()["act_state"]
        out.append(o)
    return out


def reads_equal(a, b, what):
    for t, (x, y) in enumerate(zip(a, b)):
        for k in x:
            if k != "ticks":
                assert same(x[k], y[k]), (what, t, k)


def test_detach_mid_race_gives_the_healthy_kernels_words():
    """A race with faults through tick 24, snapshot, detach, 6 ticks, against a race that never had a binding restored to that
    snapshot (the rows are a binding, not state: the blobs are interchangeable): bit for bit, through lap events.  Attached, the same 6
    ticks differ."""
    B = 8
    f, g = faulted_fleet(B, race_rows(B)), faulted_fleet(B)
    assert g.faults() is None and same(f.faults(), race_rows(B))
    f.run(24); g.run(3)
    snap = f.snapshot()
    assert snap.to_bytes()[:8] == g.snapshot().to_bytes()[:8] and len(snap.to_bytes()) == len(g.snapshot().to_bytes())
    attached = race_reads(f, 6)
    f.restore(snap)
    f.fault(None)
    assert f.faults() is None
    detached = race_reads(f, 6)
    g.restore(snap)
    healthy = race_reads(g, 6)
    reads_equal(detached, healthy, "detached vs never attached")
    assert not same(attached[-1]["est"], detached[-1]["est"])
    assert np.any(detached[-1]["phase"] == 1)
    f.close(); g.close()


# ---- 7. snapshot and clone -----------------------------------------------------------------------------------------------------
def test_snapshot_restore_and_clone_with_faults_attached():
    """With faults attached a race restored to its snapshot repeats its next 20 ticks bit for bit.  A clone keeps its slot's own row:
    with noiseless sensors, slot 1 (the same loss row as slot 0, another vid) draws its own losses, and slot 2's biased gyro reads the
    plant's rate plus its bias while slot 0's reads the plant's."""
    B = 8
    rows = race_rows(B)
    f = faulted_fleet(B, rows)
    f.run(15)
    snap = f.snapshot()
    first = race_reads(f, 20)
    f.restore(snap)
    again = race_reads(f, 20)
    reads_equal(first, again, "restored")
    assert np.any(first[-1]["phase"] == 1) and same(f.faults(), rows)
    f.close()
    import lpvmpc
    rows = lpvmpc.fault_rows(B, DT, gps_loss_p=0.5)
    rows[2, 7] = 0.05
    quiet = dict(psi_std=0.0, psiDot_std=0.0, x_std=0.0, y_std=0.0, v_std=0.0)
    f = faulted_fleet(B, rows, stds=quiet, plant0=RO.grid_fleet(B, 4))
    f.run(5)
    src = np.arange(B, dtype=np.int32); src[1] = 0; src[2] = 0
    assert f.clone(src) == 2
    o = f.state(); est, meas = f.estimate()
    assert same(o["plant"][1], o["plant"][0]) and same(est[2], est[0]) and same(meas[1], meas[0])
    differs = False
    for _ in range(6):
        f.run(1)
        o = f.state(); est, meas = f.estimate()
        differs = differs or not same(meas[1, 2:4], meas[0, 2:4])
        assert meas[0, 1] == o["plant"][0, 7] and meas[2, 1] == o["plant"][2, 7] + 0.0 + 0.05
    assert differs                                                          # the clone in slot 1 drew its own losses
    assert same(f.faults(), rows)
    f.close()


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_a_running_fleet_untouched():
    """Every refusal returns LPVMPC_E_ARG, and the fleet it was tried on runs on word for word like one that was never asked."""
    import lpvmpc
    from lpvmpc import _ffi
    mp = lshape()
    B = 8
    plant0 = RO.grid_fleet(B, 2)
    prow, tyres = lpvmpc.sample_plant_params(B, 3), lpvmpc.sample_tyre_params(B, 3, kind=[0, 1] * 4)
    rows = lpvmpc.fault_rows(B, DT, gps_outage=(0.05, 0.1), imu_w_bias=0.02, enc_outage=(0.1, 0.3), gps_loss_p=0.2)
    oc = obs_cfg(**dict(STD, seed=5))
    cfg = _ffi.default_sensor_fault_config()

    def refused(x, r, n=B):
        return x._lib.lpvmpc_set_sensor_faults(x._h, n, C.byref(cfg), _ffi.ptr(np.ascontiguousarray(r))) == _ffi.E_ARG

    e, f = ctrl(mp), ctrl(mp)
    assert refused(e, rows)                                                 # no fleet or race on the handle
    assert e.sensor_faults() is None
    for x in (e, f):
        x.observer_setup(oc)
        x.cl_init(plant0, mp.halfWidth, mp.slack, plant_params=prow, tyre_params=tyres)
        x.set_sensor_faults(rows, seed=7)
        x.cl_tick(3)
    bad_words = [(i, v) for i in range(12) for v in (np.nan, np.inf)] + \
                [(i, v) for i in (0, 1, 3, 4, 10, 11) for v in (2.5, -1.0, 2.0 ** 31)] + [(9, 0.0), (9, -0.5)]
    for i, v in bad_words:
        bad = rows.copy(); bad[B - 1, i] = v
        assert refused(e, bad), (i, v)
    assert refused(e, rows[:B - 1], B - 1)                                  # another B than the fleet's
    os_ = np.zeros((B, 18)); st = np.tile(plant0[:1], (B, 1)); z = np.zeros(B)
    rc = e._lib.lpvmpc_sensor_step_batch(e._h, B, C.byref(oc), 0.005, C.byref(cfg), None, _ffi.ptr(os_), _ffi.ptr(st), _ffi.ptr(z), _ffi.ptr(z))
    assert rc == _ffi.E_ARG                                                 # a batch call on a handle that runs a fleet
    assert same(e.sensor_faults(), rows)
    e.cl_tick(5); f.cl_tick(5)
    a, b = e.cl_read(), f.cl_read()
    for k in ("plant", "local", "cmd", "iters", "status"):
        assert same(a[k], b[k]), k
    assert same(e.observer_read()[0], f.observer_read()[0])
    # a release frees the binding; a new fleet starts healthy
    e.cl_release()
    assert e.sensor_faults() is None
    e.cl_init(plant0, mp.halfWidth, mp.slack, plant_params=prow, tyre_params=tyres)
    assert e.sensor_faults() is None
    # fleets without an estimator, without the tables, or with a track binding
    g = ctrl(mp)
    g.cl_init(plant0, mp.halfWidth, mp.slack, plant_params=prow, tyre_params=tyres)                # ground truth
    assert refused(g, rows)
    g.observer_setup(oc)
    for kw in (dict(), dict(plant_params=prow)):
        g.cl_init(plant0, mp.halfWidth, mp.slack, **kw)
        assert refused(g, rows)
        g.cl_tick(1)
    g.cl_release()
    g.set_tracks([mp, lpvmpc.Map("oval", 0.2)], np.zeros(B, np.int32))
    g.cl_init(plant0, mp.halfWidth, mp.slack, plant_params=prow, tyre_params=tyres)
    assert refused(g, rows)                                                 # a lap-0 fleet with tracks bound
    g.cl_tick(1)
    close(e, f, g)
    # the stand-alone step refuses bad rows and counters
    s = ctrl(mp)
    for i, v in ((9, 0.0), (0, 1.5), (7, np.nan)):
        bad = rows.copy(); bad[0, i] = v
        rc = s._lib.lpvmpc_sensor_step_batch(s._h, B, C.byref(oc), 0.005, C.byref(cfg), _ffi.ptr(bad), _ffi.ptr(os_), _ffi.ptr(st), _ffi.ptr(z), _ffi.ptr(z))
        assert rc == _ffi.E_ARG, (i, v)
    for i, v in ((15, -1.0), (16, 0.5), (17, np.nan)):
        bad = os_.copy(); bad[1, i] = v
        rc = s._lib.lpvmpc_sensor_step_batch(s._h, B, C.byref(oc), 0.005, C.byref(cfg), _ffi.ptr(rows), _ffi.ptr(bad), _ffi.ptr(st), _ffi.ptr(z), _ffi.ptr(z))
        assert rc == _ffi.E_ARG, (i, v)
    s.close()
    # races: without an estimator, without tyre rows, not the path handle; a race with tracks is served
    path, tt, plan = engines(mp)
    path.race_init(tt, plan, plant0, half_width=mp.halfWidth, slack=mp.slack, plant_params=prow, tyre_params=tyres)
    assert refused(path, rows)                                              # on ground truth
    path.cl_release()
    path.race_init(tt, plan, plant0, half_width=mp.halfWidth, slack=mp.slack, plant_params=prow, estimator=oc)
    assert refused(path, rows)                                              # no tyre rows
    path.cl_release()
    path.race_init(tt, plan, plant0, half_width=mp.halfWidth, slack=mp.slack, plant_params=prow, tyre_params=tyres, estimator=oc)
    assert refused(tt, rows)                                                # not the path handle
    path.set_sensor_faults(rows, seed=7)
    path.race_tick(2)
    bad = rows.copy(); bad[0, 9] = -1.0
    assert refused(path, bad)
    assert same(path.sensor_faults(), rows)
    close(path, tt, plan)
    f2 = lpvmpc.RaceFleet([mp, lpvmpc.Map("oval", 0.2)], np.tile(plant0[:1], (4, 1)), track_of=[0, 1, 0, 1], estimator=oc, kernel_variant=0,
                          sensor_faults=rows[:4])
    f2.run(2)
    assert same(f2.faults(), rows[:4]) and np.all(np.isfinite(f2.state()["plant"]))
    f2.close()
