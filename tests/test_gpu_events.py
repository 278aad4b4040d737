"""GPU: the race event log (lpvmpc_race_events / _read, lpvmpc_event_step_batch; RaceFleet.log / events) against the numpy restatement
tests/_events_ref.py.  Every comparison is exact on integers and bitwise on doubles (a NaN matching a NaN): the log copies or
subtracts words the device already wrote, so there is no tolerance to choose.  The batch form at B = 1, 65, 300 (a reversing heat of
256: 32 640 events on a tick) and one past the scanning workgroup's width, the carry through scripted spells and sources that come
and go, max_events and the kinds masks; on a race the ring, a real race run twice from the same start (one multi-tick call with the
log against a tick-at-a-time replay of the reference without it), and the attachment rules."""
import ctypes as C

import numpy as np
import pytest

from tests import _events_cases as K
from tests import _events_ref as R

pytestmark = pytest.mark.gpu


def batch_engine():
    import lpvmpc
    mp = lpvmpc.Map("L_shape", 0.2)
    return lpvmpc.BatchedSolver("controller", 20, 1 / 30.0, np.eye(6), np.eye(2), np.ones(2), track=mp.PointAndTangent)


def engines(mp):
    from tests.test_gpu_race_record import engines as E
    return E(mp)


def close(*es):
    for e in es:
        e.close()


def same(a, b):
    return np.asarray(a).shape == np.asarray(b).shape and np.asarray(a).tobytes() == np.asarray(b).tobytes()


def run_script(e, script, kinds=None, max_events=None):
    """A script through the batch form, the carry passed from tick to tick, against the reference: every tick's events, n_events,
    COUNT / COUNT_TOTAL and the carried total.  Returns each tick's count."""
    heat, ticks = script
    B = ticks[0]["phase"].shape[0]
    ref = R.EventsRef(B, R.ALL_KINDS if kinds is None else kinds)
    carry = None
    counts = []
    for k in ticks:
        hp = k["heats"]
        want = ref.step(k["t"], k["phase"], k["lap"], k["lap_value"], hp, heat if hp is not None else None, k["walls"])
        tab, n, out, carry = e.event_step(k["t"], k["phase"], k["lap"], k["lap_value"], heats=hp, heat=heat if hp is not None else None,
                                          walls=k["walls"], kinds=kinds, carry=carry, max_events=max_events)
        assert n == len(want), (k["t"], n, len(want))
        R.assert_same(tab, want if max_events is None else want[:max_events], "tick %d" % k["t"])
        assert np.array_equal(out["count"], ref.count) and np.array_equal(out["count_total"], ref.count_total), k["t"]
        assert carry["total"] == ref.total
        counts.append(n)
    return counts


@pytest.fixture(scope="module")
def eng():
    e = batch_engine()
    yield e
    e.close()


def test_one_vehicle_without_heats_or_walls(eng):
    B = 1
    ticks = [K.tick(0, B), K.tick(1, B, [1], [1], [70.0]), K.tick(2, B, [1], [1], [70.0]), K.tick(3, B, [2], [2], [150.0]),
             K.tick(4, B, [2], [2], [150.0])]
    assert run_script(eng, (None, ticks)) == [0, 1, 0, 2, 0]
    ticks = [K.tick(0, B), K.tick(1, B, [3], [0])]
    assert run_script(eng, (None, ticks)) == [0, 1]


def test_one_past_a_wavefront(eng):
    counts = run_script(eng, K.random_script(65, K.interleaved_heats(65, 8), 6, 11))
    assert counts[0] == 0 and min(counts[1:]) > 65


def test_a_heat_of_256_reverses_its_order(eng):
    assert run_script(eng, K.reversal()) == [0, 32640, 0]


def test_one_past_the_scanning_workgroup(eng):
    B = K.SCAN_WIDTH + 1
    assert B >= 1025
    heat = K.interleaved_heats(B, 16)
    assert (heat[::3] == -1).all() and (heat[1::3] >= 0).all()                  # vehicles in no heat interleaved
    counts = run_script(eng, K.random_script(B, heat, 4, 3))
    assert counts[0] == 0 and min(counts[1:]) > B
    # the last vehicle alone emits: its slot is behind the first chunk's 1024 silent vehicles
    lap = np.zeros(B, np.int32); lap[-1] = 1
    assert run_script(eng, (None, [K.tick(0, B), K.tick(1, B, lap=lap, lap_value=np.full(B, 9.0))])) == [0, 1]


@pytest.mark.parametrize("B", [64, 300, 2049])
def test_every_vehicle_emits_and_then_none_does(eng, B):
    assert run_script(eng, K.all_and_none(B)) == [0, B, 0]


def test_spells_through_the_carry(eng):
    """The crafted six ticks: begin, hold, end, with the lengths and the extrema (tests/test_events_host.py pins the reference's words);
    every kind, and every kind that can share a tick on one vehicle."""
    assert run_script(eng, K.crafted()) == [0, 10, 0, 0, 4, 0]


def test_a_source_that_appears_and_disappears(eng):
    """Heats and walls absent on tick 0, present on tick 1 (first sight: nothing from them), absent on tick 2 (open spells are dropped
    without an END), present again on ticks 3 and 4 (first sight again, then events)."""
    on = lambda t: t in (1, 3, 4)
    script = K.random_script(40, K.interleaved_heats(40, 8), 5, 17, heats_on=on, walls_on=on)
    heat, ticks = script
    counts = run_script(eng, script)
    per_tick, _ = K.run_ref(script)
    assert [len(p) for p in per_tick] == counts
    for t in (1, 2, 3):
        assert all(e[1] <= R.LOST for e in per_tick[t]), t                      # the race's own kinds only
    assert any(e[1] >= R.PASS for e in per_tick[4])
    assert ticks[1]["heats"]["i32"][R.H_CONTACT].any() and ticks[1]["walls"]["i32"][R.W_HIT].any()     # spells were open on tick 1


def test_max_events_and_kinds_masks(eng):
    script = K.random_script(65, K.interleaved_heats(65, 8), 4, 23)
    full = run_script(eng, script)
    assert run_script(eng, script, max_events=10) == full and run_script(eng, script, max_events=0) == full and min(full[1:]) > 10
    per_kind = []
    for kind in range(1, 9):
        per_kind.append(sum(run_script(eng, K.crafted(), kinds=1 << kind)))
    assert per_kind == [1, 1, 1, 3, 2, 2, 2, 2]
    assert sum(run_script(eng, K.crafted(), kinds=0)) == 0


# ---- on a race ----------------------------------------------------------------------------------------------------------------------
def feed(ref, path, t, heat=None, walls=False, fresh=(False, False)):
    """One tick's reads of a race into the reference; returns (events, everything that was read)."""
    o = path.race_read()
    ls, alive = path.race_laps()
    lv = ls[np.arange(ls.shape[0]), np.clip(o["lap"], 0, ls.shape[1] - 1)].astype(float)
    st = path.race_standings() if heat is not None else None
    w = path.race_walls_read() if walls else None
    evs = ref.step(t, o["phase"], o["lap"], lv, st, heat, w, heats_fresh=fresh[0], walls_fresh=fresh[1])
    return evs, dict(race=o, lap_step=ls, alive=alive, standings=st, walls=w)


def test_the_ring_on_a_race():
    """23 identical cars in two packs (20 and 3 clones) short of the line, no heats, no walls: each pack has its lap event on one
    tick, so the race has ticks of 0, 3 and 20 events.  The same ticks (from one snapshot) with capacity 1, 7 (smaller than a tick),
    5 (no divisor of the total) and 64: total, kept and the oldest-first order against the ring model."""
    import lpvmpc
    from oracle import plant_ref as PR
    mp = lpvmpc.Map("L_shape", 0.2)
    tab = np.asarray(mp.PointAndTangent, float)
    L = float(mp.TrackLength)
    n = 24
    plant0 = np.zeros((23, 8))
    for b in range(23):                                                         # the pack of 20 in front, the pack of 3 behind it
        x, y, th = PR.get_global_position(tab, L - (0.15 if b < 20 else 0.4), 0.0)
        plant0[b] = [x, y, 1.0, 0.0, 0.0, 0.0, th, 0.0]
    path, tt, plan = engines(mp)
    path.race_init(tt, plan, plant0, half_track0=1, laps=3, half_width=mp.halfWidth, slack=mp.slack)
    snap = path.race_snapshot()
    ref = R.EventsRef(23)
    per_tick = []
    for t in range(n):
        path.race_tick(1)
        per_tick.append(feed(ref, path, t)[0])
    counts = sorted(set(len(p) for p in per_tick))
    print("ring race: events per tick", [len(p) for p in per_tick])
    assert counts == [0, 3, 20] and per_tick[0] == []
    flat = [e for p in per_tick for e in p]
    for cap in (1, 7, 5, 64):
        path.race_restore(snap)
        path.race_events(dict(capacity=cap))
        path.race_tick(n)
        ring = R.Ring(cap)
        for p in per_tick:
            ring.push_tick(p)
        r = path.race_events_read()
        assert (r["total"], r["kept"]) == (ring.total, ring.kept) == (len(flat), min(cap, len(flat)))
        R.assert_same(r["events"], ring.read(), "capacity %d" % cap)
        R.assert_same(path.race_events_read(3)["events"], ring.read(3), "capacity %d, last 3" % cap)
        assert np.array_equal(r["count_total"], ref.count_total) and r["count"].sum() == len(per_tick[-1])
        path.race_events(detach=True)
    assert len(flat) % 5 != 0
    close(path, tt, plan)


def start(log=None, heats=True, walls=True):
    mp, plant0, prow, tyres = K.race_setup()
    path, tt, plan = engines(mp)
    path.race_init(tt, plan, plant0, half_track0=0, laps=3, half_width=mp.halfWidth, slack=mp.slack, plant_params=prow, tyre_params=tyres)
    if heats:
        path.race_heats(K.RACE_HEAT, **K.RACE_FOOTPRINT)
    if walls:
        path.race_walls(K.RACE_WALLS)
    if log is not None:
        path.race_events(log)
    return path, tt, plan


def reads_equal(a, b):
    for k in a["race"]:
        assert same(a["race"][k], b["race"][k]), k
    assert same(a["lap_step"], b["lap_step"]) and same(a["alive"], b["alive"])
    for name in ("standings", "walls"):
        for k in ("f64", "i32"):
            assert same(a[name][k], b[name][k]), (name, k)
    assert same(a["standings"]["line_tick"], b["standings"]["line_tick"]) and same(a["standings"]["line_pos"], b["standings"]["line_pos"])


def test_a_real_race_twice_from_the_same_start():
    """(b) without the log, a tick at a time, every tick's reads fed to the reference; (a) with the log, all ticks in one call.  The
    two event lists are equal, every plane of the last tick is (a)'s bit for bit (the log only observes), and the run holds a lap
    event, a pass, a contact that begins and ends and a wall hit that begins and clears."""
    n = K.RACE_TICKS
    path, tt, plan = start()
    ref = R.EventsRef(K.RACE_B)
    want = []
    for t in range(n):
        path.race_tick(1)
        evs, last_b = feed(ref, path, t, K.RACE_HEAT, True)
        want += evs
    close(path, tt, plan)
    path, tt, plan = start(log={})
    path.race_tick(n)
    r = path.race_events_read()
    _, last_a = feed(R.EventsRef(K.RACE_B), path, n - 1, K.RACE_HEAT, True)
    close(path, tt, plan)
    kinds = sorted(set(e[1] for e in want))
    print("real race: %d events, per kind %s" % (len(want), {k: sum(1 for e in want if e[1] == k) for k in kinds}))
    assert r["total"] == len(want) == r["kept"]
    R.assert_same(r["events"], want, "race")
    assert np.array_equal(r["count_total"], ref.count_total)
    reads_equal(last_a, last_b)
    assert {R.LAP, R.PASS, R.CONTACT_BEGIN, R.CONTACT_END, R.WALL_HIT, R.WALL_CLEAR} <= set(kinds)


def test_heats_and_walls_come_and_go_under_the_log():
    """The log stays attached while heats and walls are attached, replaced and detached, and meets each new attachment at first
    sight: the race a tick at a time, the reference told what was done between the ticks."""
    path, tt, plan = start(log=dict(capacity=4096), heats=False, walls=False)
    ref = R.EventsRef(K.RACE_B)
    want = []
    heat = None; walls = False
    for t in range(24):
        fresh = [False, False]
        if t == 2:
            path.race_walls(K.RACE_WALLS); walls = True
        if t == 4:
            path.race_heats(K.RACE_HEAT, **K.RACE_FOOTPRINT); heat = K.RACE_HEAT
        if t == 9:
            path.race_walls(K.RACE_WALLS); fresh[1] = True                      # replaced between two ticks
        if t == 12:
            heat = np.array([0, 1] * 4, np.int32)
            path.race_heats(heat, **K.RACE_FOOTPRINT); fresh[0] = True          # replaced, with other members
        if t == 16:
            path.race_walls(detach=True); walls = False
        if t == 18:
            path.race_heats(None); heat = None
        if t == 20:
            path.race_walls(K.RACE_WALLS); walls = True
        path.race_tick(1)
        want += feed(ref, path, t, heat, walls, fresh)[0]
        assert path.race_events_read(0)["total"] == len(want), t               # still attached, and in step
    r = path.race_events_read()
    R.assert_same(r["events"], want, "come and go")
    assert len(want) > 0
    close(path, tt, plan)


def test_attachment_rules():
    import lpvmpc
    from lpvmpc import _ffi
    path, tt, plan = start(log=dict(capacity=50))
    lib = path._lib
    path.race_tick(12)
    before = path.race_events_read()
    assert before["total"] > 0
    # refusals leave the attached log bit for bit
    e = batch_engine()
    cfg = _ffi.default_event_config()
    assert lib.lpvmpc_race_events(e._h, C.byref(cfg)) == _ffi.E_ARG            # no race on the handle
    assert lib.lpvmpc_race_events_read(e._h, 0, None, None, None, None, None) == _ffi.E_ARG
    for bad in (_ffi.EventConfig(0, _ffi.EVENT_ALL_KINDS, (0, 0)), _ffi.EventConfig(-3, _ffi.EVENT_ALL_KINDS, (0, 0)),
                _ffi.EventConfig(8, 1, (0, 0)), _ffi.EventConfig(8, 0x200, (0, 0)), _ffi.EventConfig(8, 2, (0, 1)), _ffi.EventConfig(8, 2, (1, 0))):
        assert lib.lpvmpc_race_events(path._h, C.byref(bad)) == _ffi.E_ARG
        after = path.race_events_read()
        assert after["total"] == before["total"] and same(after["events"], before["events"]) and same(after["i32"], before["i32"])
    with pytest.raises(ValueError):
        path.race_events(dict(capacity=0))
    with pytest.raises(ValueError):
        path.race_events_read(-1)
    assert lib.lpvmpc_race_events_read(path._h, -1, None, None, None, None, None) == _ffi.E_ARG
    # restore and clone are refused while it is attached; a snapshot is not
    snap = path.race_snapshot()
    with pytest.raises(lpvmpc.LpvMpcError):
        path.race_restore(snap)
    with pytest.raises(lpvmpc.LpvMpcError):
        path.race_clone(np.arange(K.RACE_B))
    after = path.race_events_read()
    assert after["total"] == before["total"] and same(after["events"], before["events"])
    # replace restarts the count, and the first tick of the new binding is first sight
    path.race_events(dict(capacity=50, kinds=["wall_hit", "wall_clear"]))
    assert path.race_events_read()["total"] == 0
    path.race_tick(1)
    r = path.race_events_read()
    assert r["total"] == 0 and not r["i32"].any()
    path.race_tick(10)
    r = path.race_events_read()
    assert set(r["events"]["kind"].tolist()) <= {R.WALL_HIT, R.WALL_CLEAR}
    # detached: reads are refused, restore and clone work, the heats and the walls are still there
    path.race_events(detach=True)
    path.race_events(detach=True)                                               # nothing attached: nothing to do
    with pytest.raises(lpvmpc.LpvMpcError):
        path.race_events_read()
    path.race_standings(); path.race_walls_read()
    path.race_heats(None)
    path.race_restore(snap)
    assert path.race_clone(np.arange(K.RACE_B)) == 0
    close(path, tt, plan)
    # the batch form: a busy handle, B = 0, a NULL argument, half a heats side, a bad kinds word
    path, tt, plan = start(heats=False, walls=False)
    z = np.zeros(4, np.int32); zf = np.zeros(4); cf = np.zeros((2, 4)); ci = np.zeros((11, 4), np.int32); out = np.zeros((2, 4), np.int32)
    tot = C.c_int64(0); n = _ffi._i(0)
    p = _ffi.ptr

    def call(h, B, phase=z, kinds=_ffi.EVENT_ALL_KINDS, heat=None, hf=None, hi=None, total=tot):
        return lib.lpvmpc_event_step_batch(h, B, 0, p(phase), p(z), p(zf), 1, p(heat), p(hf), p(hi), None, None, kinds, p(cf), p(ci),
                                           C.byref(total) if total is not None else None, 0, None, None, C.byref(n), p(out))
    assert call(path._h, 4) == _ffi.E_ARG and b"batch calls" in lib.lpvmpc_last_error(path._h)     # busy
    assert call(e._h, 0) == 0                                                   # nothing to do
    assert call(e._h, 4) == 0
    assert call(e._h, 4, phase=None) == _ffi.E_ARG and call(e._h, 4, total=None) == _ffi.E_ARG and call(e._h, -1) == _ffi.E_ARG
    assert call(e._h, 4, heat=z) == _ffi.E_ARG and call(e._h, 4, kinds=1) == _ffi.E_ARG
    close(path, tt, plan, e)


def test_the_fleet_interface():
    import lpvmpc
    from lpvmpc import events as E
    mp, plant0, prow, tyres = K.race_setup()
    fleet = lpvmpc.RaceFleet(mp, plant0, laps=3, half_track0=0, plant_params=prow, tyre_params=tyres, kernel_variant=0,
                             heats=dict(heat=K.RACE_HEAT, **K.RACE_FOOTPRINT), walls=K.RACE_WALLS, events=dict(capacity=256))
    fleet.run(20)
    tab, total = fleet.events()
    assert total == tab.shape[0] > 0 and tab.dtype == E.DTYPE
    keys = list(zip(tab["tick"].tolist(), tab["vehicle"].tolist(), tab["kind"].tolist(), tab["other"].tolist()))
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    last, _ = fleet.events(2)
    assert same(last, tab[-2:])
    fleet.log(detach=True)
    with pytest.raises(lpvmpc.LpvMpcError):
        fleet.events()
    fleet.log()
    assert fleet.events()[1] == 0
    for e in (fleet.path, fleet.tt, fleet.planner):
        e.close()
