"""GPU: the walls (lpvmpc_race_walls / _read, lpvmpc_wall_step_batch; BatchedSolver.race_walls / race_walls_read / wall_step,
RaceFleet.wall / walls) against the numpy restatement tests/_walls_ref.py: the crafted single ticks at B = 1, 3, 63, 64, 65 and 257
without tracks bound and with a two-track binding, a scripted sequence with the carry handed over between two handles, a race with
walls against the host replay, the far-margin and detached races, restore and clone, the attach orders with disturbances and
interactions, reruns, the refusals, and one physical check.  Decisions, counters and who was written are held exactly, values to 1e-11
relative to max(1, |value|) -- the bar the device plant and transforms hold against their oracle -- and word for word for the vehicle
whose heading and whose wall's track heading are exactly 0.  tests/test_walls_host.py asserts the decision margins that make the exact
comparisons meaningful."""
import ctypes as C

import numpy as np
import pytest

from tests import _walls_cases as K
from tests import _walls_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-11
B = K.RACE_B


def batch_engine(mp=None):
    import lpvmpc
    mp = mp or lpvmpc.Map("L_shape", 0.2)
    return lpvmpc.BatchedSolver("controller", 20, 1 / 30.0, np.eye(6), np.eye(2), np.ones(2), track=mp.PointAndTangent)


def engines(mp):
    from tests.test_gpu_race_record import engines as E
    return E(mp)


def close(*es):
    for e in es:
        e.close()


def same(a, b):
    return np.asarray(a).shape == np.asarray(b).shape and np.asarray(a).tobytes() == np.asarray(b).tobytes()


def close_to(a, b, what):
    a, b = np.asarray(a, float), np.asarray(b, float)
    assert np.array_equal(np.isnan(a), np.isnan(b)), what
    ok = ~np.isnan(a)
    err = float(np.max(np.abs(a[ok] - b[ok]) / np.maximum(1.0, np.abs(b[ok])))) if ok.any() else 0.0
    assert err <= TOL, (what, err)
    return err


def compare(plant, out, carry, before, ref, exact=(), rows=None):
    """A device tick against the restatement's: decisions, counters and who was written exactly; values to TOL; the vehicles ``exact``
    (heading and track heading exactly 0, so cos / sin are exact and the normal is (0, -+1)) word for word: every word of the response
    that does not pass through the located ey -- x, vx, vy, psiDot, the impulses -- equals the restatement's, and DEPTH and y, which do
    (ey = |p - S| * sin(atan2(..)) of the row arithmetic, where the device's and the host's libraries may round differently in the
    last place), are held to TOL above and word for word against each other: y is the response to the device's own DEPTH."""
    from lpvmpc import _ffi
    for k in R.I32_NAMES:
        assert np.array_equal(out[k], ref[k]), (k, np.nonzero(out[k] != ref[k])[0][:8])
    assert same(plant[~ref["written"]], before[~ref["written"]])                # untouched vehicles keep their rows bit for bit
    assert same(plant[:, [4, 5, 6]], before[:, [4, 5, 6]])                      # ax, ay, yaw are nobody's to write
    worst = close_to(plant, ref["plant"], "plant")
    for k in R.F64_NAMES:
        worst = max(worst, close_to(out[k], ref[k], k))
    for c, k in enumerate(_ffi.WALL_CARRY_I32_NAMES):
        assert np.array_equal(carry["i32"][c], ref["carry"][k]), k
    for c, k in enumerate(_ffi.WALL_CARRY_F64_NAMES):
        close_to(carry["f64"][c], ref["carry"][k], "carried " + k)
    for b in exact:
        assert ref["hit"][b] == 1 and before[b, 6] == 0.0 and abs(ref["detail"][b]["n"][1]) == 1.0 and ref["detail"][b]["n"][0] == 0.0
        assert same(plant[b, [0, 2, 3, 4, 5, 6, 7]], ref["plant"][b, [0, 2, 3, 4, 5, 6, 7]]), (b, plant[b] - ref["plant"][b])
        for k in ("impulse", "impulse_total", "max_impulse"):
            assert same(out[k][b], ref[k][b]), (b, k)
        redo, _, _ = R.respond(before[b], rows[b], ref["detail"][b]["r"], ref["detail"][b]["n"], out["depth"][b], R.config())
        assert same(plant[b], redo), (b, plant[b] - redo)
    return worst


@pytest.mark.parametrize("bound", (False, True), ids=("own_track", "two_tracks"))
@pytest.mark.parametrize("n", K.SIZES)
def test_one_tick_of_crafted_geometry(n, bound):
    """Every kind of contact on a straight, a left arc, a right arc and across a seam, as many as fit in n vehicles (all of them from
    45 on), a frozen and a non-finite vehicle among them; vehicle 1 (n >= 3) is the exact one."""
    sc, ref = K.case(n, bound)
    e = batch_engine()
    if bound:
        e.set_tracks(K.tracks(), sc["track_of"])
    plant, out, carry = e.wall_step(sc["plant"], sc["rows"], 5, nstep=sc["nstep"], half_width=K.HALF_WIDTH)
    again = e.wall_step(sc["plant"], sc["rows"], 5, nstep=sc["nstep"], half_width=K.HALF_WIDTH)
    e.close()
    exact = [b for b in range(n) if sc["names"][b] == "exact"]
    worst = compare(plant, out, carry, sc["plant"], ref, exact=exact, rows=sc["rows"])
    print("wall tick, B = %d, %s: margin %.3g, %d hit, %d outside, worst relative error %.3g" %
          (n, "two tracks" if bound else "own track", ref["margin"], int(ref["hit"].sum()), int(ref["outside"].sum()), worst))
    assert same(again[0], plant) and same(again[1]["f64"], out["f64"]) and same(again[1]["i32"], out["i32"])   # reruns: bit for bit
    if n >= 3:
        assert exact == [1] + ([46] if n > 46 else []) + ([91, 136, 181, 226] if n > 226 else [])
    if n >= 45:
        assert ref["hit"].sum() >= 28 * (n // 45) and ref["outside"].sum() >= 8 * (n // 45)
        assert set(ref["side"].tolist()) == {-1, 0, 1} and set(ref["corner"].tolist()) == {-1, 0, 1, 2, 3}


def test_the_words_of_the_configuration_reach_the_kernel():
    """yaw_response 0, no friction, no push, another footprint and margin: each against the restatement with the same words."""
    sc, _ = K.case(45)
    e = batch_engine()
    for words in (dict(yaw_response=0), dict(friction=0.0, restitution=1.0), dict(push=0.0), dict(push=1.0, friction=2.0),
                  dict(half_length=0.35, half_width_car=0.15, margin=0.12, reach=0.3)):
        _, ref = K.case(45, cfg=words)
        plant, out, carry = e.wall_step(sc["plant"], sc["rows"], 5, cfg=words, nstep=sc["nstep"], half_width=K.HALF_WIDTH)
        assert ref["margin"] >= K.MARGIN, (words, ref["margins"])
        compare(plant, out, carry, sc["plant"], ref)
        if words.get("yaw_response") == 0:
            assert same(plant[:, 7], sc["plant"][:, 7])
    e.close()


def test_carry_through_a_scripted_sequence():
    """12 ticks of 3 cars: a hit starts, lasts and ends twice; every counter exact on every tick, and the run split over two handles,
    the carry handed over, equals the one run."""
    rows = K.plant_rows(3)
    tab = np.asarray(K.tracks()[0].PointAndTangent, float)
    e, e2 = batch_engine(), batch_engine()
    carry = carry2 = ref_carry = None
    for t in range(K.SCRIPT_TICKS):
        p = K.script(t)
        ref = R.tick(p, rows, tab, K.HALF_WIDTH, R.config(), t=t, carry=ref_carry)
        ref_carry = ref["carry"]
        plant, out, carry = e.wall_step(p, rows, t, carry=carry, half_width=K.HALF_WIDTH)
        compare(plant, out, carry, p, ref)
        if t == 5:
            carry2 = dict(f64=carry["f64"].copy(), i32=carry["i32"].copy())
        if t > 5:
            plant2, out2, carry2 = e2.wall_step(p, rows, t, carry=carry2, half_width=K.HALF_WIDTH)
            assert same(plant2, plant) and same(out2["f64"], out["f64"]) and same(out2["i32"], out["i32"])
            assert same(carry2["f64"], carry["f64"]) and same(carry2["i32"], carry["i32"])
    close(e, e2)
    assert out["hit_ticks"].tolist() == [5, 0, 8] and out["first_hit_tick"].tolist() == [2, -1, 4]
    assert out["max_impulse"][0] > 0 and out["impulse_total"][0] >= out["max_impulse"][0]


# ---- in a race ---------------------------------------------------------------------------------------------------------------------
def start(mp, plant0, prow, tyres, walls=None):
    path, tt, plan = engines(mp)
    path.race_init(tt, plan, plant0, half_track0=0, laps=3, half_width=mp.halfWidth, slack=mp.slack, plant_params=prow, tyre_params=tyres)
    if walls is not None:
        path.race_walls(walls)
    return path, tt, plan


def run(path, n, walls=False):
    out = []
    for _ in range(n):
        path.race_tick(1)
        o = path.race_read()
        if walls:
            o["walls"] = path.race_walls_read()
        out.append(o)
    return out


RACE_KEYS = ("plant", "local", "cmd", "phase", "lap", "iters", "status", "plan_iters", "plan_status")


def races_equal(a, b):
    assert len(a) == len(b)
    for t, (x, y) in enumerate(zip(a, b)):
        for k in RACE_KEYS:
            assert same(x[k], y[k]), (t, k)


def test_race_with_walls_matches_the_host_replay():
    """A _tyres race of 8 cars aimed at the walls, 30 lap-0 ticks against the host replay: the tyre race's bar, states within 2e-6,
    equal statuses and iteration counts; the walls' decisions follow the replay's exactly; hits start and end."""
    mp, plant0, prow, tyres = K.race_setup()
    ticks, margin = K.race_replay()
    path, tt, plan = start(mp, plant0, prow, tyres, walls=K.RACE_CFG)
    worst = worst_out = 0.0
    hits = []
    for t, ref in enumerate(ticks):
        path.race_tick(1)
        o, w = path.race_read(), path.race_walls_read()
        assert np.all(o["phase"] == 0), t
        for k in ("plant", "local", "cmd"):
            worst = max(worst, float(np.max(np.abs(o[k] - ref[k]))))
        assert np.array_equal(o["iters"], ref["iters"]) and np.array_equal(o["status"], ref["status"]), t
        for k in R.I32_NAMES:
            assert np.array_equal(w[k], ref["wall"][k]), (t, k)
        for k in R.F64_NAMES:
            worst_out = max(worst_out, float(np.max(np.abs(w[k] - ref["wall"][k]))))
        hits.append(w["hit"].copy())
    close(path, tt, plan)
    hits = np.array(hits)
    print("race with walls vs replay: %d ticks, worst state / command error %.3g, worst output error %.3g, %d hits by %d cars, smallest "
          "decision margin of the replay %.3g" % (len(ticks), worst, worst_out, int(hits.sum()), int(hits.any(axis=0).sum()), margin))
    assert worst <= 2e-6 and worst_out <= 2e-6
    assert hits.any(axis=0).sum() >= 3 and not hits[0].any() and not hits[-1].any()


def test_far_margin_detached_restored_and_reruns():
    """A far-margin attachment equals nothing attached, every word; a rerun of the attached race is bit-identical; a race detached at
    tick 10 equals, from the same snapshot, one that never had the binding; a restore while attached replays the same ticks."""
    mp, plant0, prow, tyres = K.race_setup()
    n = 20
    path, tt, plan = start(mp, plant0, prow, tyres)
    plain = run(path, n)
    close(path, tt, plan)
    path, tt, plan = start(mp, plant0, prow, tyres, walls=dict(margin=50.0))
    far = run(path, n)
    w = path.race_walls_read()
    assert not w["hit_ticks"].any() and not w["outside"].any() and not w["f64"].any() and np.all(w["corner"] == -1)
    close(path, tt, plan)
    races_equal(plain, far)
    first = None
    for _ in range(2):
        path, tt, plan = start(mp, plant0, prow, tyres, walls=K.RACE_CFG)
        on = run(path, n, walls=True)
        if first is not None:
            races_equal(first, on)
            for x, y in zip(first, on):
                assert same(x["walls"]["f64"], y["walls"]["f64"]) and same(x["walls"]["i32"], y["walls"]["i32"])
        else:
            close(path, tt, plan)
        first = first or on
    assert not same(first[-1]["plant"], plain[-1]["plant"])                     # the attached race is another race
    # restore while attached (the second of the two races is still open, at tick 20): back to its own snapshot, the same ticks again
    snap = path.race_snapshot()
    a = run(path, 5, walls=True)
    path.race_restore(snap)
    b = run(path, 5, walls=True)
    races_equal(a, b)
    assert same(a[-1]["walls"]["i32"][:3], b[-1]["walls"]["i32"][:3])           # per-tick words alike; the counters are the binding's
    close(path, tt, plan)
    # detached at tick 10: from there on the race that never had the binding, started from the same snapshot
    path, tt, plan = start(mp, plant0, prow, tyres, walls=K.RACE_CFG)
    run(path, 10)
    assert path.race_walls_read()["hit_ticks"].sum() > 0
    path.race_walls(detach=True)
    snap = path.race_snapshot()
    a = run(path, 10)
    close(path, tt, plan)
    path, tt, plan = start(mp, plant0, prow, tyres)
    path.race_restore(snap)
    b = run(path, 10)
    close(path, tt, plan)
    races_equal(a, b)


def test_clone_with_walls_attached():
    mp, plant0, prow, tyres = K.race_setup()
    path, tt, plan = start(mp, plant0, prow, tyres, walls=K.RACE_CFG)
    run(path, 6)
    before = path.race_walls_read()
    src = np.arange(B); src[0] = 5
    assert path.race_clone(src) == 1
    o = path.race_read()
    assert same(o["plant"][0], o["plant"][5])
    after = path.race_walls_read()
    assert same(before["i32"], after["i32"]) and same(before["f64"], after["f64"])   # the counters belong to the binding's slots
    path.race_tick(1)
    w = path.race_walls_read()
    for k in ("depth", "hit", "side", "corner", "outside"):                    # the same pose in front of the same wall
        assert same(w[k][0], w[k][5]), k
    assert w["hit"][5] == 1 and w["hit_ticks"][0] == before["hit_ticks"][0] + 1
    close(path, tt, plan)


def test_walls_disturbances_and_interactions_in_each_attach_order():
    """Walls, disturbances (a grip patch and a kick) and interactions (heats of 4) attached in three orders give the same race, word
    for word; plant_params_read returns the caller's rows throughout; detaching the walls alone leaves the other two attached."""
    import lpvmpc
    from lpvmpc import disturbance as D
    mp, plant0, prow, tyres = K.race_setup()
    rows = D.disturbance_rows(B, patch0=(0.0, float(mp.TrackLength), 0.8), kick_step=np.full(B, 10.0), kick_vy=np.where(np.arange(B) % 2 == 0, 0.8, -0.8))
    heat = np.array([0] * 4 + [1] * 4)
    steps = dict(walls=lambda p: p.race_walls(K.RACE_CFG), dist=lambda p: p.set_disturbances(rows),
                 inter=lambda p: (p.race_heats(heat, half_length=0.2, half_width=0.1), p.race_interactions(dict(draft_gain=0.5))))
    got = []
    for order in (("walls", "dist", "inter"), ("inter", "dist", "walls"), ("dist", "walls", "inter")):
        path, tt, plan = start(mp, plant0, prow, tyres)
        for s in order:
            steps[s](path)
            assert same(path.plant_params_read(), prow), (order, s)
        got.append(run(path, 8, walls=True))
        if order[0] == "walls":
            path.race_walls(detach=True)
            path.race_tick(1)
            assert path.race_interactions_read()["draft_ticks"].max() >= 0 and same(path.plant_params_read(), prow)
            with pytest.raises(lpvmpc.LpvMpcError):
                path.race_walls_read()
        close(path, tt, plan)
    for other in got[1:]:
        races_equal(got[0], other)
        assert same(got[0][-1]["walls"]["f64"], other[-1]["walls"]["f64"]) and same(got[0][-1]["walls"]["i32"], other[-1]["walls"]["i32"])
    assert got[0][-1]["walls"]["hit_ticks"].sum() > 0


def test_refusals_and_lifetime():
    import lpvmpc
    from lpvmpc import _ffi
    mp, plant0, prow, tyres = K.race_setup()
    e = batch_engine()
    assert e._lib.lpvmpc_race_walls(e._h, None) == -1 and e._lib.lpvmpc_race_walls_read(e._h, None, None) == -1   # no race
    with pytest.raises(lpvmpc.LpvMpcError):
        e.race_walls()
    sc, _ = K.case(3)
    with pytest.raises(ValueError):
        e.wall_step(sc["plant"], sc["rows"], 0, cfg=dict(push=2.0))
    bad = sc["rows"].copy(); bad[0, 3] = 0.0
    with pytest.raises(lpvmpc.LpvMpcError):
        e.wall_step(sc["plant"], bad, 0)                                        # Iz = 0
    with pytest.raises(lpvmpc.LpvMpcError):
        e.wall_step(sc["plant"], sc["rows"], 0, half_width=float("nan"))
    e.set_tracks(K.tracks(), [0, 1])
    with pytest.raises(lpvmpc.LpvMpcError):
        e.wall_step(sc["plant"], sc["rows"], 0)                                 # tracks bound for 2 vehicles, 3 given
    e.close()
    # no plant table
    path, tt, plan = engines(mp)
    path.race_init(tt, plan, plant0, half_track0=0, laps=3, half_width=mp.halfWidth, slack=mp.slack)
    with pytest.raises(lpvmpc.LpvMpcError, match="plant table"):
        path.race_walls()
    path.race_tick(1)
    with pytest.raises(lpvmpc.LpvMpcError):
        tt.wall_step(sc["plant"], sc["rows"], 0)                                # a handle that runs a race
    close(path, tt, plan)
    path, tt, plan = start(mp, plant0, prow, tyres)
    with pytest.raises(lpvmpc.LpvMpcError):
        path.race_walls_read()                                                  # nothing attached
    path.race_walls(detach=True)                                                # detaching nothing is no error
    path.race_walls(K.RACE_CFG)
    path.race_tick(12)
    before = path.race_walls_read()
    assert before["hit_ticks"].sum() > 0
    for word, v in (("margin", -0.1), ("margin", float("nan")), ("reach", 0.0), ("half_length", 0.0), ("half_width_car", float("inf")),
                    ("restitution", 1.5), ("friction", -1.0), ("push", -0.5), ("yaw_response", 2), ("reserved", 1)):
        c = _ffi.default_wall_config()
        setattr(c, word, v)
        assert path._lib.lpvmpc_race_walls(path._h, C.byref(c)) == -1, word     # LPVMPC_E_ARG, past the Python checks
    after = path.race_walls_read()
    assert same(before["f64"], after["f64"]) and same(before["i32"], after["i32"])   # a refused call leaves the binding as it was
    path.race_walls()                                                           # attaching again: the counters start anew
    w = path.race_walls_read()
    assert not w["hit_ticks"].any() and np.all(w["first_hit_tick"] == -1) and not w["f64"].any()
    path.race_tick(1)
    close(path, tt, plan)


def test_the_fleet_interface():
    import lpvmpc
    mp, plant0, prow, tyres = K.race_setup()
    fleet = lpvmpc.RaceFleet(mp, plant0, laps=3, half_track0=0, plant_params=prow, tyre_params=tyres, kernel_variant=0, walls=K.RACE_CFG)
    fleet.run(12)
    w = fleet.walls()
    ticks, _ = K.race_replay()
    assert np.array_equal(w["hit_ticks"], ticks[11]["wall"]["hit_ticks"]) and w["hit_ticks"].sum() > 0
    fleet.wall(detach=True)
    with pytest.raises(lpvmpc.LpvMpcError):
        fleet.walls()
    fleet.wall()
    fleet.run(1)
    assert fleet.walls()["first_hit_tick"].max() <= 12
    fleet.close()
    fleet = lpvmpc.RaceFleet(mp, plant0, laps=3, half_track0=0, walls=True)     # selects the start with a plant table
    fleet.run(2)
    assert not fleet.walls()["outside"].any()
    fleet.close()


def test_a_kicked_car_is_lost_without_walls_and_races_on_with_them():
    """A calm fleet; a disturbance row kicks car 2 sideways at 4 m/s in tick 5.  Without walls it leaves the track and is frozen as
    phase 3 within 45 ticks; with the default walls it is still racing, with hits counted.  (The kick was picked on the host replay:
    tests/test_walls_host.py holds both outcomes there.)"""
    from lpvmpc import disturbance as D
    mp, _, prow, tyres = K.race_setup()
    plant0, kicks = K.kick_setup()
    rows = D.disturbance_rows(B, kick_step=kicks[:, 0], kick_vy=kicks[:, 1], kick_w=kicks[:, 2])
    phase = {}
    for name, walls in (("open", None), ("walls", {})):
        path, tt, plan = start(mp, plant0, prow, tyres, walls=walls)
        path.set_disturbances(rows)
        path.race_tick(K.KICK_TICKS)
        phase[name] = path.race_read()["phase"].copy()
        if walls is not None:
            w = path.race_walls_read()
        close(path, tt, plan)
    print("kicked car: phase without walls %d, with walls %d; hit ticks %d, largest impulse %.3g" %
          (phase["open"][K.KICK_CAR], phase["walls"][K.KICK_CAR], w["hit_ticks"][K.KICK_CAR], w["max_impulse"][K.KICK_CAR]))
    assert phase["open"][K.KICK_CAR] == 3 and np.all(np.delete(phase["open"], K.KICK_CAR) == 0)
    assert np.all(phase["walls"] == 0) and w["hit_ticks"][K.KICK_CAR] > 0 and not np.delete(w["hit_ticks"], K.KICK_CAR).any()
