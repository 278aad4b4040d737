"""GPU: the heats (lpvmpc_race_heats / _standings, lpvmpc_heat_step_batch; BatchedSolver.race_heats / race_standings / heat_step,
RaceFleet.heats / standings) against the numpy restatement tests/_heats_ref.py: one tick of crafted geometry, scripted sequences
with the carry passed back in, heats attached to a race and stepped on the recorder's channels, per-vehicle tracks, lifetime and
refusals.  The order, progress, gaps, passes and line tables are held word for word, the clearances to the reference's band."""
import ctypes as C

import numpy as np
import pytest

from tests import _heats_cases as HC
from tests import _heats_ref as R
from tests import _race_observer_ref as RO

pytestmark = pytest.mark.gpu

KV = 0          # kernel_variant fixed on every handle: kernel routes may depend on B


def lshape():
    import lpvmpc
    return lpvmpc.Map("L_shape", 0.2)


def batch_engine():
    import lpvmpc
    return lpvmpc.BatchedSolver("controller", 20, 1 / 30.0, np.eye(6), np.eye(2), np.ones(2), track=lshape().PointAndTangent)


def engines(mp):
    from tests.test_gpu_race_record import engines as E
    return E(mp)


def close(*es):
    for e in es:
        e.close()


def same(a, b):
    return np.asarray(a).shape == np.asarray(b).shape and np.asarray(a).tobytes() == np.asarray(b).tobytes()


@pytest.mark.parametrize("case", ("three_heats", "one_of_256"))
def test_one_tick_of_crafted_geometry(case):
    from lpvmpc import heats as H
    c = HC.crafted() if case == "three_heats" else HC.crafted_256()
    B = c["heat"].shape[0]
    eng = batch_engine()
    dev, carry = eng.heat_step(c["heat"], c["L"], c["pose"], c["s"], c["inside"], c["phase"], 5,
                               carry=H.new_carry(B, c["turns0"], c["phase0"]), half_length=c["hl"], half_width=c["hw"])
    eng.close()
    ref = R.HeatsRef(c["heat"], c["L"], c["turns0"], c["phase0"], c["hl"], c["hw"]).step(5, c["pose"], c["s"], c["inside"], c["phase"])
    m = c["heat"] >= 0
    fin = m & np.isfinite(ref["clearance"])
    err = np.abs(dev["clearance"][fin] - ref["clearance"][fin])
    print(case, "max |clearance - reference| = %.3e, largest band %.3e; contacts %d; touching pairs read %s" %
          (err.max(), ref["band"].max(), int(dev["contact"].sum()), [(float(dev["clearance"][a]), int(dev["contact"][a])) for a, _ in c["touching"]]))
    R.compare(dev, ref, case)
    assert np.array_equal(dev["first_contact_tick"][m & (dev["contact"] == 1)], np.full(int((m & (dev["contact"] == 1)).sum()), 5))
    # the same word on both sides of every mutual nearest pair
    near = dev["nearest"]
    mutual = [b for b in range(B) if near[b] >= 0 and near[near[b]] == b]
    assert len(mutual) >= 10
    for b in mutual:
        assert dev["clearance"][b].tobytes() == dev["clearance"][near[b]].tobytes(), (b, near[b])
    # a vehicle in no heat
    out = ~m
    assert np.all(dev["position"][out] == -1) and np.all(np.isnan(dev["f64"][:, out])) and np.all(dev["class"][out] == -1)
    assert np.all(dev["nearest"][out] == -1) and np.all(dev["ahead"][out] == -1) and np.all(dev["first_contact_tick"][out] == -1)
    assert np.all(dev["i32"][[3, 4, 6, 7, 8]][:, out] == 0)
    assert np.array_equal(carry["i32"][0][m], 1 + 2 * ~np.isnan(ref["progress"][m]))      # the flag word: ticked, located


@pytest.mark.parametrize("name", list(HC.SEQUENCES))
def test_scripted_sequences(name):
    from lpvmpc import heats as H
    static, ticks = HC.sequence(HC.SEQUENCES[name])
    B = static["heat"].shape[0]
    eng = batch_engine()
    ref = R.HeatsRef(static["heat"], static["L"], static["turns0"], None, HC.SEQ_HL, HC.SEQ_HW, lines=3)
    carry = H.new_carry(B, static["turns0"], lines=3)
    for t, k in enumerate(ticks):
        dev, carry = eng.heat_step(static["heat"], static["L"], k["pose"], k["s"], k["inside"], k["phase"], t, carry=carry,
                                   half_length=HC.SEQ_HL, half_width=HC.SEQ_HW)
        want = ref.step(t, k["pose"], k["s"], k["inside"], k["phase"])
        want["ambiguous"][:] = False                             # every sep of a sequence is exact in float64: nothing may differ
        R.compare(dev, want, "%s tick %d" % (name, t), exact_sep=True)
        for key in ("nearest", "contact", "contact_ticks", "first_contact_tick"):
            assert np.array_equal(dev[key], want[key]), (name, t, key)
        # the batch form keeps no line tables (K = 0): the device's word is the carried crossing count, from which heat_step fills the
        # tables on the host.  The kernel's own line-table write is checked in the race tests below
        assert np.array_equal(carry["i32"][3][static["heat"] >= 0], ref.crossings[static["heat"] >= 0]), (name, t)
    eng.close()
    assert dev["passes"].sum() >= 4 and dev["line_tick"][0, 0] == 8 and dev["line_tick"][7, 0] == 8


def race_plant0(mp):
    """8 vehicles near the end of the L shape's lap, two heats of 4 (even / odd indices).  Heat 0: vehicles 0 and 2 at one pose
    (contact from the first tick).  Heat 1: vehicle 1 at 1.4 m/s starts 0.1 m behind vehicle 3 at 0.5 m/s, offset 0.05 m to the side."""
    from oracle import plant_ref as PR
    tab = np.asarray(mp.PointAndTangent, float)
    L = float(tab[-1, 3] + tab[-1, 4])
    s0 = L - 0.6
    spec = [(s0, 0.0, 1.0), (s0 - 0.1, 0.05, 1.4), (s0, 0.0, 1.0), (s0, 0.0, 0.5), (s0 - 1.5, 0.02, 1.0), (s0 - 2.0, -0.03, 0.95),
            (s0 - 3.0, -0.02, 1.05), (s0 - 4.0, 0.03, 1.0)]
    plant0 = np.zeros((8, 8))
    for b, (s, ey, vx) in enumerate(spec):
        x, y, th = PR.get_global_position(tab, s, ey)
        plant0[b] = [x, y, vx, 0, 0, 0, th, 0]
    return plant0, L


def test_heats_attached_to_a_race():
    mp = lshape()
    plant0, L = race_plant0(mp)
    B, T = 8, 40
    heat = np.arange(B) % 2
    turns0 = np.full(B, -1)
    kw = dict(half_track0=1, laps=2, half_width=mp.halfWidth, slack=mp.slack)
    path, tt, plan = engines(mp)
    path.race_init(tt, plan, plant0, **kw)
    path.race_record(T, 1)
    path.race_heats(heat, turns0=turns0)
    before = path.race_standings()
    assert np.all(before["position"] == -1) and np.all(before["turns"] == -1) and np.all(np.isnan(before["f64"]))
    ref = R.HeatsRef(heat, L, turns0, None, 0.4, 0.2, lines=4)
    skip = np.zeros(B, bool)
    worst = 0.0
    for t in range(T):
        path.race_tick(1)
        dev = path.race_standings()
        rec = path.race_record_read(last=1)
        assert rec["tick"][0] == t
        pose = np.stack([rec["x"][0], rec["y"][0], rec["yaw"][0]], axis=1)
        want = ref.step(t, pose, rec["track_s"][0], rec["inside"][0], rec["phase"][0])
        R.compare(dev, want, "tick %d" % t, skip_contact=skip)
        skip |= want["ambiguous"]
        fin = np.isfinite(want["clearance"])
        worst = max(worst, float(np.max(np.abs(dev["clearance"] - want["clearance"])[fin] / want["band"][fin])))
    from lpvmpc import telemetry
    tab = telemetry.standings_table(dev, heat)
    print("race: passes %s, contact ticks %s, turns %s, line ticks %s, worst |clearance error| / band %.3f, ambiguous %s" %
          (dev["passes"].tolist(), dev["contact_ticks"].tolist(), dev["turns"].tolist(), dev["line_tick"][:, 0].tolist(), worst, skip.tolist()))
    print("heat 1 order", tab[1]["vehicle"].tolist(), "gaps", tab[1]["gap_ahead"].tolist())
    assert want["passes"].sum() >= 1 and want["passes"][1] >= 1, want["passes"]          # the reference replay shows the pass
    assert want["contact_ticks"].sum() >= 1 and want["contact_ticks"][0] >= 1 and want["first_contact_tick"][0] == 0
    assert np.any(want["line_tick"][:, 0] >= 0)
    final = dict(path.race_read()); final["lap_step"], final["alive"] = path.race_laps(); final["pu"], final["tu"] = path.race_predictions()
    close(path, tt, plan)
    # the same race without heats and without the recorder
    path, tt, plan = engines(mp)
    path.race_init(tt, plan, plant0, **kw)
    path.race_tick(T)
    plain = dict(path.race_read()); plain["lap_step"], plain["alive"] = path.race_laps(); plain["pu"], plain["tu"] = path.race_predictions()
    close(path, tt, plan)
    for k in final:                                              # every word: the race's start zeroes the planner's report too
        assert same(final[k], plain[k]), k
    assert np.all(final["plan_iters"][final["phase"] == 0] == 0) and np.any(final["plan_iters"] > 0)


def test_per_vehicle_tracks():
    from tests import _tracks as TK
    from tests.test_gpu_tracks import race_engines
    from lpvmpc import LpvMpcError
    maps, of = TK.race_palette(), TK.cycle(TK.RACE_B, 4)
    plant0 = TK.race_starts(maps, of)
    B, T = TK.RACE_B, 24
    heat = np.where(of == 0, 0, np.where(of == 1, 1, -1))
    Lb = np.array([float(maps[k].PointAndTangent[-1, 3] + maps[k].PointAndTangent[-1, 4]) for k in of])
    path, tt, plan = race_engines(None, (maps, of))
    path.race_init(tt, plan, plant0, half_track0=1, laps=2, tyre_params="linear", half_width=123.0, slack=456.0)
    with pytest.raises(LpvMpcError) as e:                        # one heat spanning two tracks
        path.race_heats(np.zeros(B, int))
    assert "track" in str(e.value)
    path.race_record(T, 1)
    path.race_heats(heat, turns0=np.full(B, -1))
    ref = R.HeatsRef(heat, Lb, np.full(B, -1), None, 0.4, 0.2, lines=4)
    skip = np.zeros(B, bool)
    for t in range(T):
        path.race_tick(1)
        dev = path.race_standings()
        rec = path.race_record_read(last=1)
        pose = np.stack([rec["x"][0], rec["y"][0], rec["yaw"][0]], axis=1)
        want = ref.step(t, pose, rec["track_s"][0], rec["inside"][0], rec["phase"][0])
        R.compare(dev, want, "tick %d" % t, skip_contact=skip)
        skip |= want["ambiguous"]
    print("tracks: turns %s progress %s" % (dev["turns"].tolist(), dev["progress"].tolist()))
    assert np.any(dev["turns"][heat >= 0] == 0) and len(set(Lb[heat >= 0].tolist())) == 2       # line crossings, each heat with its own L
    close(path, tt, plan)


def test_lifetime_and_refusals():
    import lpvmpc
    from lpvmpc import _ffi, LpvMpcError
    mp = lshape()
    lib = _ffi.load()
    plant0, L = race_plant0(mp)
    B = 8
    path, tt, plan = engines(mp)
    cfg = _ffi.HeatsConfig()
    lib.lpvmpc_heats_default_config(C.byref(cfg))
    assert (cfg.half_length, cfg.half_width_car) == (0.4, 0.2)

    def attach(heat, hl=0.4, hw=0.2, h=None):
        c = _ffi.HeatsConfig(hl, hw)
        a = np.ascontiguousarray(heat, np.int32)
        return lib.lpvmpc_race_heats(h or path._h, C.byref(c), a.ctypes.data_as(C.c_void_p), None)

    two = np.arange(B) % 2
    assert attach(two) == _ffi.E_ARG                                        # no race on the handle
    assert lib.lpvmpc_race_standings(path._h, None, None, None, None) == _ffi.E_ARG
    kw = dict(half_track0=1, laps=2, half_width=mp.halfWidth, slack=mp.slack)
    path.race_init(tt, plan, plant0, **kw)
    assert lib.lpvmpc_race_standings(path._h, None, None, None, None) == _ffi.E_ARG      # detached
    assert "lpvmpc_race_heats" in lib.lpvmpc_last_error(path._h).decode()
    assert attach(two, h=tt._h) == _ffi.E_ARG                               # the race belongs to the path handle
    bad = two.copy(); bad[3] = -2
    assert attach(bad) == _ffi.E_ARG
    assert attach(two, 0.0, 0.2) == _ffi.E_ARG and attach(two, 0.4, float("nan")) == _ffi.E_ARG and attach(two, -0.4, 0.2) == _ffi.E_ARG
    assert lib.lpvmpc_race_heats(path._h, None, two.astype(np.int32).ctypes.data_as(C.c_void_p), None) == _ffi.E_ARG
    assert lib.lpvmpc_race_standings(path._h, None, None, None, None) == _ffi.E_ARG      # every refusal left it detached
    assert attach(np.array([7, 7, 1000000, -1, 7, 1000000, 7, -1])) == 0                  # indices need not be dense
    path.race_tick(3)
    s = path.race_standings()
    assert sorted(s["position"][[0, 1, 4, 6]].tolist()) == [0, 1, 2, 3] and sorted(s["position"][[2, 5]].tolist()) == [0, 1]
    assert np.all(s["position"][[3, 7]] == -1)
    # snapshot allowed, restore and clone refused while attached, and working after the detach
    path.race_heats(two)
    path.race_tick(4)
    first = path.race_standings()
    assert first["contact_ticks"][0] == 4 and first["first_contact_tick"][0] == 3
    snap = path.race_snapshot()
    for call in (lambda: path.race_restore(snap), lambda: path.race_clone(np.arange(B)[::-1].copy())):
        with pytest.raises(LpvMpcError) as e:
            call()
        assert "lpvmpc_race_heats(path, cfg, NULL, NULL)" in str(e.value)
    path.race_tick(2)
    # re-attach resets the counters
    path.race_heats(two)
    blank = path.race_standings()
    assert np.all(blank["position"] == -1) and np.all(blank["contact_ticks"] == 0)
    path.race_tick(1)
    again = path.race_standings()
    assert again["contact_ticks"][0] == 1 and again["first_contact_tick"][0] == 9 and np.all(again["passes"] == 0)
    path.race_heats(None)
    with pytest.raises(LpvMpcError):
        path.race_standings()
    path.race_restore(snap)
    assert path.race_read()["ticks"] == 7
    assert path.race_clone(np.array([1, 1, 2, 3, 4, 5, 6, 7])) == 1
    # a heat of 257 members
    close(path, tt, plan)
    big, _ = race_plant0(mp)
    big = np.tile(big, (33, 1))[:257]
    path, tt, plan = engines(mp)
    path.race_init(tt, plan, big, **kw)
    assert attach(np.zeros(257, np.int32)) == _ffi.E_ARG and "256" in lib.lpvmpc_last_error(path._h).decode()
    h256 = np.zeros(257, np.int32); h256[100] = -1
    assert attach(h256) == 0
    path.race_tick(1)
    s = path.race_standings()
    assert sorted(s["position"][h256 == 0].tolist()) == list(range(256)) and s["position"][100] == -1
    # release frees; a new race on the same handles starts without heats
    path.cl_release()
    path.race_init(tt, plan, big, **kw)
    assert lib.lpvmpc_race_standings(path._h, None, None, None, None) == _ffi.E_ARG
    path.race_tick(1)
    assert attach(h256) == 0
    close(tt)                                                   # destroying a handle of the race ends it, heats included
    assert attach(h256) == _ffi.E_ARG
    close(path, plan)
    # the batch form's refusals
    eng = batch_engine()
    c = HC.crafted()
    with pytest.raises(LpvMpcError):
        eng.heat_step(c["heat"], c["L"], c["pose"], c["s"], c["inside"], c["phase"], 0, n_heats=2)       # heat 2 of 2
    with pytest.raises(LpvMpcError):
        eng.heat_step(c["heat"], 0.0, c["pose"], c["s"], c["inside"], c["phase"], 0)
    eng.close()


def test_race_fleet_interface():
    import lpvmpc
    from lpvmpc import telemetry
    mp = lshape()
    plant0 = RO.start_line_fleet(mp.PointAndTangent, 16, 5, 0.9, 0.97)
    f = lpvmpc.RaceFleet(mp, plant0, laps=2, half_track0=1, kernel_variant=KV)
    heat = np.arange(16) // 8
    f.heats(heat)
    f.run(30)
    s = f.standings()
    tab = telemetry.standings_table(s, heat)
    assert sorted(tab) == [0, 1] and s["line_tick"].shape == (16, 4) and len(tab[0]["vehicle"]) == 8
    f.heats(None)
    with pytest.raises(lpvmpc.LpvMpcError):
        f.standings()
    f.close()
