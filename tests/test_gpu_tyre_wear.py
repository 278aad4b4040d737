"""GPU: tyre wear and temperature (lpvmpc_set_tyre_wear, lpvmpc_tyre_wear_read, lpvmpc_tyre_wear_fit, lpvmpc_plant_step_worn_batch).
The stand-alone step equals the numpy restatement (tests/_tyre_wear_ref.py) bit for bit in all six state words, and its plant is the
tyre step on the live rows the restatement computes, word for word; all-off rows change no word of a step, a lap-0 fleet or a race;
frozen and finished vehicles are not touched; the state does not depend on sharding; a worn race matches the host replay under
test_disturbed_race_matches_the_replay's rule; wear and disturbances compose as g * (gamma * base) and detach in either order; the
tyre change; snapshot, restore and clone carry the tyre sets; read-back and refusals."""
import ctypes as C

import numpy as np
import pytest

from tests import _disturbance_ref as D
from tests import _race_observer_ref as RO
from tests import _race_snapshot as S
from tests import _tyre_wear_ref as WR
from tests.test_gpu_delayed_fleets import close, ctrl, engines, lshape, same
from tests.test_gpu_disturbance import HW0, SLACK0, around, local_s, off
from tests.test_gpu_plant_params import RACE_KEYS, _race_same

pytestmark = pytest.mark.gpu

N_SUB, DT = 7, 0.005
E_ARG = -1


def wear_off(B):
    return np.tile(WR.ALL_OFF, (B, 1))


def biting(B, seed=0):
    """Rows that act from the first tick on whatever the car does: the sets start 15 .. 25 K under T_opt and relax towards an ambient
    above it, so g < 1 at once and moves every tick; wear, heat and the cliff act as soon as the car slides."""
    import lpvmpc
    rng = np.random.default_rng([seed, 77])
    return lpvmpc.tyre_wear_rows(B, k_wear=rng.uniform(20, 60, B), k_hot=0.05, k_heat=rng.uniform(200, 600, B), k_cool=rng.uniform(0.5, 2.0, B),
                                 T_amb=45.0, T_opt=40.0, k_temp=rng.uniform(3e-4, 6e-4, B), wear_slope=0.5, cliff_at=0.2, cliff_slope=1.0,
                                 g_min=0.3, T_start=rng.uniform(15, 25, B))


# ---- 1. the stand-alone step against the restatement, exact ---------------------------------------------------------------------------
def step_case(B, seed):
    """Random rows over all twelve words, pre-tick plant states and carried wear states; vehicle b takes the edge case b % 8:
    1, 2: |vx| on either side of the plant's gate 0.2; 3: ay == 0; 4, 5: W just below / above cliff_at; 6: W about to saturate at 1;
    7: g clamped at g_min; 0: none -- and every 16th vehicle a row whose g is 1."""
    rng = np.random.default_rng([seed, B])
    rows = np.column_stack([rng.uniform(0, 5, B), rng.uniform(0, 0.2, B), rng.uniform(0, 50, B), rng.uniform(0, 5, B), rng.uniform(0, 40, B),
                            rng.uniform(10, 60, B), rng.uniform(0, 1e-3, B), rng.uniform(0, 0.8, B), rng.uniform(0.05, 0.95, B),
                            rng.uniform(0, 4, B), rng.uniform(1e-3, 0.6, B), rng.uniform(0, 80, B)])
    ws = WR.fresh(rows)
    ws[:, 0] = rng.uniform(0, 0.5, B); ws[:, 1] = rng.uniform(0, 80, B); ws[:, 4] = rng.integers(0, 50, B); ws[:, 5] = rng.uniform(0, 10, B)
    mp = lshape()
    st = around(mp, B, seed)
    st[:, 3] = rng.normal(0, 0.15, B); st[:, 5] = rng.normal(0, 3.0, B); st[:, 7] = rng.normal(0, 1.0, B)
    k = np.arange(B) % 8
    st[k == 1, 2] = 0.2; st[k == 2, 2] = np.nextafter(0.2, 1.0); st[k == 3, 5] = 0.0
    ws[k == 4, 0] = rows[k == 4, 8] - 1e-12; ws[k == 5, 0] = rows[k == 5, 8] + 1e-12
    ws[k == 6, 0] = 1.0 - 1e-9; rows[k == 6, 0] = 5.0
    rows[k == 7, 7] = 1.5; ws[k == 7, 0] = 0.9; rows[k == 7, 10] = 0.4
    one = np.arange(B) % 16 == 8
    rows[one, 6] = 0.0; rows[one, 7] = 0.0; rows[one, 9] = 0.0
    u = np.column_stack([np.full(B, 0.6), np.where(np.arange(B) % 2, 0.25, -0.25)])
    return mp, rows, ws, st, u


@pytest.mark.parametrize("disturbed", [False, True], ids=["wear", "wear+disturbances"])
@pytest.mark.parametrize("B", [1, 64, 65])
def test_step_matches_the_restatement_exactly(B, disturbed):
    """Three chained ticks of 7 steps carrying every state.  All six wear words equal the restatement bit for bit; the plant and the
    actuator state equal lpvmpc_plant_step_tyres_batch on the live rows g * base that the restatement computed, word for word: the
    same plant kernel on a scaled table.  With disturbance rows -- a kick inside the second tick and a patch under every other vehicle;
    no gusts, whose draws the host restates to 1e-11 only -- they equal lpvmpc_plant_step_disturbed_batch on the live rows
    g * (gamma * base) with the patches' gamma set to 1, and gamma is the disturbances' own word."""
    import lpvmpc
    mp, rows, ws0, st0, u = step_case(B, 5)
    tr = mp.PointAndTangent
    prow = lpvmpc.sample_plant_params(B, 6)
    tyres = lpvmpc.sample_tyre_params(B, 6, kind=(np.arange(B) % 2).astype(float))
    drows = flat = None
    dist = None
    if disturbed:
        drows = off(B)
        drows[:, 4:7] = (10.0, 0.15, -0.6)                                                     # in the second of the three calls
        s = local_s(mp, st0, HW0, SLACK0)
        p = np.arange(B) % 2 == 0
        drows[p, 7] = np.mod(s[p] - 0.5, D.lap_length(tr)); drows[p, 8] = 3.0; drows[p, 9] = 0.45
        flat = drows.copy(); flat[:, 9] = 1.0
        dist = D.Model(drows)
    model = WR.Model(rows, state=ws0)
    e = ctrl(mp)
    st, act, ds, ws = st0, None, None, ws0
    seen_g, seen_W, gated = set(), set(), 0
    for c in range(3):
        lp, lt = prow.copy(), tyres.copy()
        for b in range(B):
            pre, gamma = st[b], None
            if disturbed:
                pre, gamma = dist.apply(b, st[b], N_SUB * c, N_SUB, DT, tr, HW0, SLACK0)
            g = model.apply(b, pre, prow[b, 1], prow[b, 2], N_SUB, DT)
            lp[b], lt[b] = WR.live_rows(prow[b], tyres[b], g, gamma)
            gated += int(abs(pre[2]) <= 0.2 and model.state[b, 2] == 0.0)
        got = e.plant_step_worn(st, u, rows, ws, rows=drows, dist_state=ds, plant_params=prow, tyre_params=tyres, act_state=act, n_sub=N_SUB)
        if disturbed:
            want = e.plant_step_disturbed(st, u, flat, ds, plant_params=lp, tyre_params=lt, act_state=act, n_sub=N_SUB)
            assert same(got[2][:, :4], want[2][:, :4]) and same(got[2][:, 4], dist.state[:, 4]), c
        else:
            want = e.plant_step_vehicles(st, u, lp, act, n_sub=N_SUB, tyre_params=lt)
            assert got[2] is None
        bad = np.nonzero(np.any(got[3].view(np.uint64) != model.state.view(np.uint64), axis=1))[0]
        assert bad.size == 0, (c, bad[:4].tolist(), got[3][bad[:2]].tolist(), model.state[bad[:2]].tolist())
        assert same(got[0], want[0]) and same(got[1], want[1]), c
        st, act, ds, ws = got
        seen_g |= set(np.where(ws[:, 3] == rows[:, 10], -1.0, ws[:, 3]).tolist()); seen_W |= set(ws[:, 0].tolist())
    assert np.all(ws[:, 4] == ws0[:, 4] + 3) and np.all(act[:, -1] == 3 * N_SUB) and np.all(np.isfinite(st))
    if B >= 64:                                                                                # every clamp and the gate were met
        assert -1.0 in seen_g and 1.0 in seen_g and 1.0 in seen_W and gated >= B // 8, (sorted(seen_g)[:3], gated)
        if disturbed:
            assert set(ds[:, 4].tolist()) == {1.0, 0.45}
    e.close()


# ---- 2. all-off rows attached against nothing attached --------------------------------------------------------------------------------
def test_all_off_step_is_the_tyre_step():
    import lpvmpc
    mp = lshape()
    B = 16
    st0 = around(mp, B, 1); st0[:, 5] = 2.0; st0[:, 7] = 0.5
    u = np.column_stack([np.full(B, 0.8), np.where(np.arange(B) % 2, 0.2, -0.2)])
    prow, tyres = lpvmpc.sample_plant_params(B, 2), lpvmpc.sample_tyre_params(B, 2, kind=(np.arange(B) % 2).astype(float))
    e = ctrl(mp)
    a = e.plant_step_vehicles(st0, u, prow, None, n_sub=N_SUB, tyre_params=tyres)
    b = e.plant_step_worn(st0, u, wear_off(B), plant_params=prow, tyre_params=tyres, n_sub=N_SUB)
    assert same(a[0], b[0]) and same(a[1], b[1]) and b[2] is None
    assert np.all(b[3][:, [0, 1, 3, 4]] == [0.0, 20.0, 1.0, 1.0])                             # W, T, g, ticks
    assert np.all(b[3][:, 2] > 0) and same(b[3][:, 5], b[3][:, 2] * (N_SUB * DT))             # P and E are the car's, not the row's
    e.close()


CL_KEYS = ("plant", "local", "cmd", "iters", "status", "act_state", "path")


def cl_run(mp, plant0, n_ticks, wear=None, attach_tick=0, **kw):
    e = ctrl(mp)
    e.cl_init(plant0, mp.halfWidth, mp.slack, q9_swap=True, n_sub=N_SUB, **kw)
    out = []
    for t in range(n_ticks):
        if wear is not None and t == attach_tick:
            e.set_tyre_wear(wear)
        e.cl_tick(1)
        o = e.cl_read()
        o.update(e.actuator_read())
        out.append(o)
    if wear is not None:
        out.append(e.tyre_wear_read()[1])
    e.close()
    return out


def test_all_off_lap0_fleet_is_the_unattached_fleet():
    import lpvmpc
    mp = lshape()
    B, n = 8, 30
    plant0 = RO.grid_fleet(B, 3)
    kw = dict(plant_params=lpvmpc.sample_plant_params(B, 5), tyre_params=lpvmpc.sample_tyre_params(B, 5))
    a = cl_run(mp, plant0, n, **kw)
    b = cl_run(mp, plant0, n, wear=wear_off(B), **kw)
    for t in range(n):
        for k in CL_KEYS:
            assert np.array_equal(a[t][k], b[t][k]), (t, k)
    assert np.all(b[n][:, [0, 1, 3, 4]] == [0.0, 20.0, 1.0, float(n)])


def race_run(mp, plant0, n_ticks, wear=None, **kw):
    path, tt, plan = engines(mp)
    path.race_init(tt, plan, plant0, laps=2, half_width=mp.halfWidth, slack=mp.slack, **kw)
    if wear is not None:
        path.set_tyre_wear(wear)
    out = []
    for _ in range(n_ticks):
        path.race_tick(1)
        o = path.race_read()
        o.update(path.actuator_read())
        out.append(o)
    last = dict(zip(("path_uPred", "tt_uPred"), path.race_predictions()))
    last.update(zip(("lap_step", "alive"), path.race_laps()))
    if wear is not None:
        last["wear"] = path.tyre_wear_read()[1]
    out.append(last)
    close(path, tt, plan)
    return out


def test_all_off_race_is_the_unattached_race():
    import lpvmpc
    mp = lshape()
    B, n = 8, 30
    plant0 = RO.start_line_fleet(mp.PointAndTangent, B, 7, 0.975, 0.985)
    kw = dict(half_track0=1, plant_params=lpvmpc.sample_plant_params(B, 4), tyre_params=lpvmpc.tyre_params(B))
    a = race_run(mp, plant0, n, **kw)
    b = race_run(mp, plant0, n, wear=wear_off(B), **kw)
    _race_same(a, b, n, RACE_KEYS + ("act_state", "path", "tt"))
    assert np.any(a[n - 1]["phase"] == 1)                                                     # through a lap event
    assert np.all(b[n]["wear"][:, [0, 1, 3, 4]] == [0.0, 20.0, 1.0, float(n)])


# ---- 3. frozen and finished vehicles --------------------------------------------------------------------------------------------------
def test_frozen_race_vehicle_is_not_touched():
    """A race vehicle that takes no plant step because it is lost (on the first tick) keeps the state its set started with, tick count
    0; the others count three ticks and their sets move."""
    mp = lshape()
    B = 8
    plant0 = RO.start_line_fleet(mp.PointAndTangent, B, 5)
    plant0[2, 2] = np.inf
    rows = biting(B)
    path, tt, plan = engines(mp)
    path.race_init(tt, plan, plant0, half_track0=1, half_width=mp.halfWidth, slack=mp.slack, tyre_params="linear")
    path.set_tyre_wear(rows)
    path.race_tick(3)
    o, (r, state) = path.race_read(), path.tyre_wear_read()
    live = np.arange(B) != 2
    assert same(r, rows) and o["phase"][2] == 3 and same(o["plant"][2], plant0[2])
    assert same(state[2], WR.fresh(rows)[2])
    assert np.all(state[live, 4] == 3) and np.all(state[live, 1] != rows[live, 11]) and np.all(state[live, 3] < 1) and np.all(o["phase"][live] < 2)
    close(path, tt, plan)


def test_finished_race_vehicle_is_not_touched():
    """test_gpu_disturbance's one-lap race: four vehicles finish while four are still in lap 0.  Wear attached then leaves the finished
    vehicles' sets and tick count alone and reaches the others."""
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
    assert np.any(done[:4]) and np.all(before["phase"][4:] == 0)
    rows = biting(B)
    base = path.plant_params_read(), path.tyre_params_read()
    path.set_tyre_wear(rows)
    path.race_tick(3)
    o, (_, state) = path.race_read(), path.tyre_wear_read()
    assert same(o["plant"][done], before["plant"][done]) and np.all(o["phase"][done] == 2)
    assert same(state[done], WR.fresh(rows)[done])
    assert np.all(state[4:, 4] == 3) and np.all(state[4:, 3] < 1) and np.all(state[4:, 1] != rows[4:, 11])
    assert same(path.plant_params_read(), base[0]) and same(path.tyre_params_read(), base[1])     # the base rows while attached
    path.set_tyre_wear(None)                                                                   # and in the live tables after the detach
    assert same(path.plant_params_read(), base[0]) and same(path.tyre_params_read(), base[1])
    close(path, tt, plan)


# ---- 4. sharding ----------------------------------------------------------------------------------------------------------------------
def test_wear_does_not_depend_on_sharding():
    """A lap-0 fleet of 8 over 15 ticks equals its two halves of 4, word for word, wear state included: a set has its own history."""
    import lpvmpc
    mp = lshape()
    B, n, h = 8, 15, 4
    plant0 = RO.grid_fleet(B, 6)
    plant0[:, 7] = np.where(np.arange(B) % 2, 0.5, -0.5)
    rows = biting(B, 4)
    prow, tyres = lpvmpc.sample_plant_params(B, 4), lpvmpc.sample_tyre_params(B, 4)

    def run(lo, hi):
        return cl_run(mp, plant0[lo:hi], n, plant_params=prow[lo:hi], tyre_params=tyres[lo:hi], wear=rows[lo:hi])

    whole, a, b = run(0, B), run(0, h), run(h, B)
    for t in range(n):
        for k in CL_KEYS:
            assert same(whole[t][k], np.concatenate([a[t][k], b[t][k]])), (t, k)
    assert same(whole[n], np.concatenate([a[n], b[n]]))
    quiet = cl_run(mp, plant0, n, plant_params=prow, tyre_params=tyres)
    assert np.max(np.abs(whole[n - 1]["plant"] - quiet[n - 1]["plant"])) > 1e-6 and np.all(whole[n][:, 3] < 1) and np.all(whole[n][:, 4] == n)


# ---- 5. the worn race against the host replay ------------------------------------------------------------------------------------------
def test_worn_race_matches_the_replay():
    """tests/_tyre_wear_ref.race_case: 8 vehicles on the launch file's Pacejka tyre, laps = 3, wear attached at tick 10, against the
    host replay under test_disturbed_race_matches_the_replay's rule, taken over unchanged: lap 0 within 2e-6, the same event ticks, the
    same vehicles lost, equal statuses, and in each survivor's first 24 racing ticks two thirds within 1e-5 / 1e-4, all within 2e-2,
    >= 95 % equal iteration counts.  W, T and g of the strict survivors agree with the replay within 1e-5 as well; on the replay g
    falls below 0.9 for at least half the fleet inside its window (tests/test_tyre_wear_host.py asserts the replay's side alone)."""
    B, W_, attach = WR.RACE_B, WR.RACE_WINDOW, WR.RACE_ATTACH
    mp, plant0, prow, tyres, rows, ref = WR.race_case()
    path, tt, plan = engines(mp)
    path.race_init(tt, plan, plant0, half_track0=1, laps=WR.RACE_LAPS, half_width=mp.halfWidth, slack=mp.slack, plant_params=prow, tyre_params=tyres)
    racing = np.zeros(B, int)
    ev_dev = np.full(B, -1)
    w_state = np.zeros(B); w_cmd = np.zeros(B); w_wear = np.zeros(B); same_it = n_it = 0
    lost_dev, lost_ref, st_diff = {}, {}, []
    err0 = np.zeros(B)
    g_low = np.ones(B)
    t = 0
    while np.any(racing < W_) and t < 200:
        if t == attach:
            path.set_tyre_wear(rows)
        ph_before = ref.phase.copy()
        path.race_tick(1); ref.tick()
        o = path.race_read()
        ws = path.tyre_wear_read()[1] if t >= attach else None
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
            w_wear[v] = max(w_wear[v], float(np.max(np.abs(ws[v, [0, 1, 3]] - ref.wear.state[v, [0, 1, 3]]))))
            g_low[v] = min(g_low[v], float(ref.wear.state[v, 3]))
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
    print("worn race vs replay: %d ticks, events %s, lap 0 worst %.3g, survivors within 1e-5 / 1e-4: %d of %d, worst survivor %.3g / %.3g, "
          "worst W / T / g of the strict survivors %.3g, lost %s, iterations %d / %d, lowest g %s"
          % (t, sorted(ref.event_tick.tolist()), err0[kept].max(), strict.sum(), surv.sum(), w_state[surv].max(), w_cmd[surv].max(),
             w_wear[strict].max() if strict.any() else -1.0, lost_dev, same_it, n_it, np.round(g_low, 3).tolist()))
    assert surv_ref.sum() >= need                                                             # the replay alone, on the CPU
    assert np.sum(g_low < 0.9) >= B // 2                                                      # the wear bit inside the windows
    assert np.all((racing >= W_) | (ev_dev < 0)) and n_it > 0 and np.sum(ev_dev >= 0) >= need
    assert np.array_equal(ev_dev, ref.event_tick) and len(set(ev_dev[ev_dev >= 0].tolist())) >= 4
    assert kept.sum() >= need and np.all(err0[kept] <= 2e-6)
    assert lost_dev == lost_ref
    assert not st_diff, st_diff
    assert same_it >= 0.95 * n_it
    assert strict.sum() >= 2 * surv.sum() // 3
    assert np.all(w_state[surv] <= 2e-2) and np.all(w_cmd[surv] <= 2e-2)
    assert np.all(w_wear[strict] <= 1e-5)
    assert np.all(ev_dev[ev_dev >= 0] > attach)
    assert same(path.plant_params_read(), prow) and same(path.tyre_params_read(), tyres)      # the base rows while attached
    path.set_tyre_wear(None)
    assert same(path.plant_params_read(), prow) and same(path.tyre_params_read(), tyres)      # and the live tables after the detach
    import lpvmpc
    with pytest.raises(lpvmpc.LpvMpcError):
        path.tyre_wear_read()
    close(path, tt, plan)


# ---- 6. composition with the disturbances, 7. the tyre change --------------------------------------------------------------------------
class Probe(object):
    """A lap-0 fleet read through one-tick probes: the plant after a tick against the stand-alone tyre step (another handle) from the
    plant, the actuator state and the command of that tick on candidate live rows.  Both are the device's plant on a table, so the
    right candidate matches word for word."""

    def __init__(self, B, seed):
        import lpvmpc
        self.mp = lshape()
        self.B = B
        self.plant0 = RO.grid_fleet(B, seed)
        self.plant0[:, 7] = np.where(np.arange(B) % 2, 0.5, -0.5)
        self.prow, self.tyres = lpvmpc.sample_plant_params(B, seed), lpvmpc.sample_tyre_params(B, seed, kind=(np.arange(B) % 2).astype(float))
        self.e, self.f = ctrl(self.mp), ctrl(self.mp)
        self.e.cl_init(self.plant0, self.mp.halfWidth, self.mp.slack, q9_swap=True, n_sub=N_SUB, plant_params=self.prow, tyre_params=self.tyres)

    def tick(self):
        """One tick; returns (the plant before, the function candidate rows -> matches word for word)."""
        before, act = self.e.cl_read()["plant"], self.e.actuator_read()["act_state"]
        self.e.cl_tick(1)
        o = self.e.cl_read()

        def matches(lp, lt):
            got = self.f.plant_step_vehicles(before, o["cmd"][:, ::-1], lp, act, n_sub=N_SUB, tyre_params=lt)[0]
            return np.array([same(got[b], o["plant"][b]) for b in range(self.B)])
        return before, matches

    def live(self, g=None, gamma=None):
        lp, lt = self.prow.copy(), self.tyres.copy()
        for b in range(self.B):
            if g is not None:
                lp[b], lt[b] = WR.live_rows(self.prow[b], self.tyres[b], g[b], None if gamma is None else gamma[b])
            elif gamma is not None:
                lp[b], lt[b] = D.scaled(self.prow[b], self.tyres[b], gamma[b])
        return lp, lt

    def worn(self, model, before):
        return np.array([model.apply(b, before[b], self.prow[b, 1], self.prow[b, 2], N_SUB, DT) for b in range(self.B)])

    def close(self):
        close(self.e, self.f)


def test_wear_and_disturbances_compose_and_detach_in_either_order():
    """A whole-lap patch (gamma 0.7 / 0.45) and biting wear on a lap-0 fleet of 8.  Both attached: the tick is the tyre step on
    g * (gamma * base), not on g * base, gamma * base or base.  Disturbances detached: g * base on the next tick.  Attached again,
    then wear detached: gamma * base.  Both detached: the base rows bit for bit, read back from the live tables, and the tick on them."""
    B = 8
    p = Probe(B, 9)
    L = D.lap_length(p.mp.PointAndTangent)
    drows = off(B); drows[:, 7:10] = (0.0, L, 0.7); drows[B // 2:, 9] = 0.45
    gamma = drows[:, 9].copy()
    rows = biting(B, 2)
    model = WR.Model(rows)
    e = p.e
    e.set_disturbances(drows)
    e.set_tyre_wear(rows)
    for t in range(3):                                                                         # both
        before, matches = p.tick()
        g = p.worn(model, before)
        assert np.all(matches(*p.live(g, gamma))), t
        assert same(e.tyre_wear_read()[1], model.state) and same(e.disturbances_read()[1][:, 4], gamma), t
        for other in (p.live(g), p.live(None, gamma), p.live()):
            assert not np.any(matches(*other)), t
        assert np.all(g < 1) and same(e.plant_params_read(), p.prow) and same(e.tyre_params_read(), p.tyres)
    e.set_disturbances(None)                                                                   # wear alone
    before, matches = p.tick()
    g = p.worn(model, before)
    assert np.all(matches(*p.live(g))) and not np.any(matches(*p.live(g, gamma))) and same(e.tyre_wear_read()[1], model.state)
    e.set_disturbances(drows)                                                                  # both again: the wear's state went on
    before, matches = p.tick()
    g = p.worn(model, before)
    assert np.all(matches(*p.live(g, gamma))) and same(e.tyre_wear_read()[1], model.state)
    e.set_tyre_wear(None)                                                                      # the disturbances alone
    before, matches = p.tick()
    assert np.all(matches(*p.live(None, gamma))) and not np.any(matches(*p.live()))
    import lpvmpc
    with pytest.raises(lpvmpc.LpvMpcError):
        e.tyre_wear_read()
    e.set_tyre_wear(rows)                                                                      # wear detached last: the other order
    model = WR.Model(rows)
    before, matches = p.tick()
    g = p.worn(model, before)
    assert np.all(matches(*p.live(g, gamma)))
    e.set_disturbances(None)
    e.set_tyre_wear(None)
    assert same(e.plant_params_read(), p.prow) and same(e.tyre_params_read(), p.tyres)        # read from the live tables now
    before, matches = p.tick()
    assert np.all(matches(*p.live()))
    p.close()


def test_tyre_change_resets_the_masked_sets():
    """fit_tyres on a mask resets exactly the masked vehicles' W, T, P and g and keeps their tick count and energy; the others are not
    touched; the next tick's state and live words follow from the fresh sets.  Refused without a binding."""
    import lpvmpc
    B = 8
    p = Probe(B, 12)
    rows = biting(B, 3)
    model = WR.Model(rows)
    e = p.e
    with pytest.raises(lpvmpc.LpvMpcError):
        e.tyre_wear_fit(np.ones(B, bool))
    e.set_tyre_wear(rows)
    for _ in range(5):
        before, matches = p.tick()
        g = p.worn(model, before)
    assert np.all(matches(*p.live(g))) and same(e.tyre_wear_read()[1], model.state)
    mask = np.arange(B) % 3 == 0
    old = e.tyre_wear_read()[1]
    e.tyre_wear_fit(mask)
    new = e.tyre_wear_read()[1]
    assert same(new[~mask], old[~mask])
    assert same(new[mask, :4], np.column_stack([np.zeros(mask.sum()), rows[mask, 11], np.zeros(mask.sum()), np.ones(mask.sum())]))
    assert same(new[mask, 4:], old[mask, 4:]) and np.all(new[mask, 4] == 5) and np.all(old[mask, 3] < 1)
    model.fit(mask)
    assert same(new, model.state)
    before, matches = p.tick()
    g = p.worn(model, before)
    assert np.all(matches(*p.live(g))) and same(e.tyre_wear_read()[1], model.state)
    p.close()
    f = S.fleet("C1", B)                                                                       # the same through RaceFleet
    f.wear(rows)
    f.run(4)
    f.fit_tyres(mask)
    r, s = f.tyre_wear()
    assert same(r, rows) and same(s[mask, :4], new[mask, :4]) and np.all(s[:, 4] == 4) and np.all(s[~mask, 3] < 1)
    f.close()


# ---- 8. snapshot, restore and clone ----------------------------------------------------------------------------------------------------
def worn_fleet(B):
    f = S.fleet("C1", B)
    f.wear(biting(B, 6))
    return f


def test_restore_repeats_a_worn_race():
    """A race with wear (and C1's estimator, actuator and disturbances), snapshotted at tick 14, run on for 12 ticks with the wear
    state read after each, restored and run again, equals its first future word for word."""
    B, after = 8, 12
    f = worn_fleet(B)
    f.run(S.T0)
    snap = f.snapshot()
    assert snap.header["features"] & 16 and list(snap.arrays)[-2:] == ["wear.state", "wear.rows"]
    assert same(snap.arrays["wear.state"], f.tyre_wear()[1]) and same(snap.arrays["wear.rows"], biting(B, 6))

    def future():
        out, wear = [], []
        for _ in range(after):
            out += S.run_reading(f, "C1", 1)
            wear.append(f.tyre_wear()[1])
        return out, wear

    first, wear1 = future()
    f.restore(snap)
    assert same(f.tyre_wear()[1], snap.arrays["wear.state"])
    again, wear2 = future()
    S.assert_reads_equal(first, again, "worn race")
    for t in range(after):
        assert same(wear1[t], wear2[t]), t
    assert not same(wear1[-1], snap.arrays["wear.state"]) and np.all(wear1[-1][:, 4] == S.T0 + after)
    f.close()


@pytest.mark.parametrize("name", ["swap", "all from the first"])
def test_clone_moves_the_tyre_set(name):
    B = 8
    src = np.arange(B, dtype=np.int32)
    if name == "swap":
        src[0], src[B - 1] = B - 1, 0
    else:
        src[:] = 0
    f = worn_fleet(B)
    f.run(S.T0)
    before = f.snapshot()
    rows0, state0 = f.tyre_wear()
    assert f.clone(src) == int(np.sum(src != np.arange(B)))
    after = f.snapshot()
    S.snaps_equal(after, before.take(src), name)
    rows1, state1 = f.tyre_wear()
    assert same(state1, state0[src]) and same(rows1, rows0[src]) and not same(state0[0], state0[B - 1])
    f.run(2)                                                                                   # the race goes on, every set on its own rows
    s2 = f.tyre_wear()[1]
    assert np.all(s2[:, 4] == S.T0 + 2) and np.all(np.isfinite(s2))
    if name == "all from the first":
        assert not same(s2[0], s2[1])                                                          # (other slots draw other gusts)
    f.close()


def test_blob_without_the_binding_knows_nothing_of_it():
    """A race without wear: the blob's size is the header, the directory and the arrays of its own directory, no entry and no feature
    bit names the wear.  Attaching adds exactly the two arrays; detaching gives the first blob back byte for byte."""
    from lpvmpc.snapshot import ENTRY_BYTES, HEADER_BYTES, RaceSnapshot
    B = 5
    f = S.fleet("C1", B)
    f.run(3)
    p = f.path

    def size():
        n = C.c_int64(0)
        assert p._lib.lpvmpc_race_snapshot_size(p._h, C.byref(n)) == 0
        return n.value

    blob = p.race_snapshot(raw=True)
    snap = RaceSnapshot.from_bytes(blob)
    own = HEADER_BYTES + ENTRY_BYTES * len(snap.directory) + sum((B * W * (4 if typ else 8) + 7) // 8 * 8 for typ, W, _ in snap.directory.values())
    assert size() == len(blob) == own
    assert not any(k.startswith("wear") for k in snap.directory) and snap.header["features"] == 1 | 2 | 4
    assert snap.to_bytes() == bytes(blob)
    f.wear(biting(B))
    assert size() == own + 2 * ENTRY_BYTES + B * (6 + 12) * 8
    worn = f.snapshot()
    assert worn.header["features"] == 1 | 2 | 4 | 16 and list(worn.directory)[:len(snap.directory)] == list(snap.directory)
    with pytest.raises(Exception):
        f.restore(snap)                                                                        # another feature word: refused
    f.wear(None)
    assert size() == own and bytes(p.race_snapshot(raw=True)) == bytes(blob)
    f.restore(snap)
    f.close()


# ---- 9. read-back and refusals --------------------------------------------------------------------------------------------------------
def test_read_back_and_refusals_leave_a_running_fleet_untouched():
    """tyre_wear_read returns the rows given; each refusal gives LPVMPC_E_ARG and the fleet it was tried on runs on, equal word for
    word to one that was never asked; fleets without the tables, a release and a new fleet carry no binding."""
    import lpvmpc
    from lpvmpc import _ffi
    mp = lshape()
    B = 8
    plant0 = RO.grid_fleet(B, 2)
    plant0[:, 7] = 0.4
    prow, tyres = lpvmpc.sample_plant_params(B, 3), lpvmpc.sample_tyre_params(B, 3, kind=[0, 1] * 4)
    rows = biting(B, 8)
    e, f = ctrl(mp), ctrl(mp)
    with pytest.raises(lpvmpc.LpvMpcError):
        e.tyre_wear_read()                                                                     # no fleet
    lib = e._lib
    assert lib.lpvmpc_set_tyre_wear(e._h, B, _ffi.ptr(rows)) == E_ARG                          # no fleet
    assert lib.lpvmpc_set_tyre_wear(None, B, _ffi.ptr(rows)) == E_ARG                          # no handle
    for x in (e, f):
        x.cl_init(plant0, mp.halfWidth, mp.slack, plant_params=prow, tyre_params=tyres)
        x.set_tyre_wear(rows)
        x.cl_tick(3)
    r, state = e.tyre_wear_read()
    assert same(r, rows) and np.all(state[:, 4] == 3) and np.all(state[:, 3] < 1)
    assert lib.lpvmpc_tyre_wear_read(e._h, None, None) == 0
    assert lib.lpvmpc_tyre_wear_fit(e._h, None) == E_ARG
    bad_words = [(0, -0.1), (1, -1.0), (2, -1e-9), (3, -2.0), (6, -1e-6), (7, -0.5), (9, -0.1), (8, -0.01), (8, 1.5), (10, 0.0), (10, -1.0), (10, 1.01),
                 (3, 1.0 / (N_SUB * DT)), (3, 100.0)] + [(i, v) for i in range(12) for v in (np.nan, np.inf)]
    e2 = ctrl(mp)
    for i, v in bad_words:
        bad = rows.copy(); bad[B - 1, i] = v
        assert lib.lpvmpc_set_tyre_wear(e._h, B, _ffi.ptr(bad)) == E_ARG, (i, v)
        st = np.tile(plant0[:1], (B, 1)); u = np.zeros((B, 2))
        rc = e2._lib.lpvmpc_plant_step_worn_batch(e2._h, B, _ffi.ptr(st), None, _ffi.ptr(u), N_SUB, DT, 0.05, None, None, None, None, None, None, None,
                                                 None, _ffi.ptr(bad), None)
        assert rc == E_ARG and same(st, np.tile(plant0[:1], (B, 1))), (i, v)
    ok = rows.copy(); ok[:, 3] = 0.99 / (N_SUB * DT)                                           # just inside the Euler bound
    st = np.tile(plant0[:1], (B, 1)); u = np.zeros((B, 2))
    assert e2._lib.lpvmpc_plant_step_worn_batch(e2._h, B, _ffi.ptr(st), None, _ffi.ptr(u), N_SUB, DT, 0.05, None, None, None, None, None, None, None,
                                                None, _ffi.ptr(ok), None) == 0
    for i, v in ((0, np.nan), (1, np.inf), (4, 2.5), (4, -1.0), (5, -np.inf)):                # the carried state's words
        st = np.tile(plant0[:1], (B, 1)); ws = WR.fresh(rows); ws[B - 1, i] = v
        rc = e2._lib.lpvmpc_plant_step_worn_batch(e2._h, B, _ffi.ptr(st), None, _ffi.ptr(u), N_SUB, DT, 0.05, None, None, None, None, None, None, None,
                                                 None, _ffi.ptr(rows), _ffi.ptr(ws))
        assert rc == E_ARG and same(st, np.tile(plant0[:1], (B, 1))), (i, v)
    rc = e2._lib.lpvmpc_plant_step_worn_batch(e2._h, B, _ffi.ptr(st), None, _ffi.ptr(u), N_SUB, DT, 0.05, None, None, None, None, None, None, None,
                                             None, None, None)
    assert rc == E_ARG                                                                         # no wear rows
    e2.close()
    assert lib.lpvmpc_set_tyre_wear(e._h, B - 1, _ffi.ptr(rows)) == E_ARG                      # B mismatch
    st = np.tile(plant0[:1], (B, 1))
    rc = lib.lpvmpc_plant_step_worn_batch(e._h, B, _ffi.ptr(st), None, _ffi.ptr(u), 1, DT, 0.05, None, None, None, None, None, None, None, None,
                                          _ffi.ptr(rows), None)
    assert rc == E_ARG                                                                         # a batch call on a handle that runs a fleet
    assert same(e.tyre_wear_read()[0], rows) and same(e.plant_params_read(), prow) and same(e.tyre_params_read(), tyres)
    e.cl_tick(5); f.cl_tick(5)
    a, b = e.cl_read(), f.cl_read()
    for k in ("plant", "local", "cmd", "iters", "status"):
        assert same(a[k], b[k]), k
    assert same(e.tyre_wear_read()[1], f.tyre_wear_read()[1])
    # attaching again starts the sets over; a release frees the binding; a new fleet starts unworn; no tables, nothing to scale
    e.set_tyre_wear(rows)
    assert same(e.tyre_wear_read()[1], WR.fresh(rows))
    e.cl_release()
    with pytest.raises(lpvmpc.LpvMpcError):
        e.tyre_wear_read()
    e.cl_init(plant0, mp.halfWidth, mp.slack, plant_params=prow, tyre_params=tyres)
    with pytest.raises(lpvmpc.LpvMpcError):
        e.tyre_wear_read()
    g = ctrl(mp)
    g.cl_init(plant0, mp.halfWidth, mp.slack, plant_params=prow, tyre_params=tyres)
    e.cl_tick(4); g.cl_tick(4)
    assert same(e.cl_read()["plant"], g.cl_read()["plant"])
    for kw in (dict(), dict(plant_params=prow)):
        g.cl_init(plant0, mp.halfWidth, mp.slack, **kw)
        assert g._lib.lpvmpc_set_tyre_wear(g._h, B, _ffi.ptr(rows)) == E_ARG
        g.cl_tick(1)
    close(e, f, g)
    path, tt, plan = engines(mp)
    path.race_init(tt, plan, plant0, half_width=mp.halfWidth, slack=mp.slack, plant_params=prow)
    assert path._lib.lpvmpc_set_tyre_wear(path._h, B, _ffi.ptr(rows)) == E_ARG                 # a race without tyre rows
    path.cl_release()
    path.race_init(tt, plan, plant0, half_width=mp.halfWidth, slack=mp.slack, plant_params=prow, tyre_params=tyres)
    assert tt._lib.lpvmpc_set_tyre_wear(tt._h, B, _ffi.ptr(rows)) == E_ARG                     # not the path handle
    path.set_tyre_wear(rows)
    path.race_tick(2)
    bad = rows.copy(); bad[0, 10] = 0.0
    assert path._lib.lpvmpc_set_tyre_wear(path._h, B, _ffi.ptr(bad)) == E_ARG
    hot = rows.copy(); hot[0, 3] = 0.99 / (N_SUB * DT)                                         # the race's n_max is 7 as well
    path.set_tyre_wear(hot)
    path.set_tyre_wear(rows); path.race_tick(2)
    r, state = path.tyre_wear_read()
    assert same(r, rows) and np.all(state[:, 4] == 2)
    assert same(path.plant_params_read(), prow) and same(path.tyre_params_read(), tyres)
    close(path, tt, plan)
