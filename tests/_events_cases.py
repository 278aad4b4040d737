"""Inputs of the race event log's tests: scripted ticks (the race's rows and the heats' / the walls' output planes of each tick, written
directly: the log copies and compares words, it does not care where they came from), and the start of the real race of
tests/test_gpu_events.py.  A script is (heat [B] or None, [tick dicts]); a tick dict holds t, phase, lap, lap_value and heats /
walls (planes dict(f64=, i32=) or None)."""
from __future__ import annotations

import numpy as np

from tests import _events_ref as R

HEAT_F64, HEAT_I32, WALL_F64, WALL_I32 = 5, 10, 4, 6
SCAN_WIDTH = 1024                   # the scanning workgroup's width (csrc/events.hpp: kEventBlock)


def blank_heats(B, heat):
    """The standings' planes with nobody in contact: positions in member order, class 1, progress descending with the position."""
    f = np.full((HEAT_F64, B), np.nan); i = np.zeros((HEAT_I32, B), np.int32)
    i[[R.H_POSITION, 1, R.H_NEAREST, 5, R.H_CLASS]] = -1
    for g in np.unique(heat[heat >= 0]):
        mem = np.nonzero(heat == g)[0]
        i[R.H_POSITION, mem] = np.arange(mem.size)
        i[R.H_CLASS, mem] = 1
        f[R.H_PROGRESS, mem] = 100.0 - 0.37 * np.arange(mem.size)
        f[R.H_CLEARANCE, mem] = 1.5
    return dict(f64=f, i32=i)


def blank_walls(B):
    f = np.zeros((WALL_F64, B)); i = np.zeros((WALL_I32, B), np.int32)
    i[R.W_CORNER] = -1
    return dict(f64=f, i32=i)


def copy_planes(p):
    return None if p is None else dict(f64=p["f64"].copy(), i32=p["i32"].copy())


def tick(t, B, phase=None, lap=None, lap_value=None, heats=None, walls=None):
    return dict(t=t, phase=np.zeros(B, np.int32) if phase is None else np.asarray(phase, np.int32).copy(),
                lap=np.zeros(B, np.int32) if lap is None else np.asarray(lap, np.int32).copy(),
                lap_value=np.full(B, -1.0) if lap_value is None else np.asarray(lap_value, float).copy(), heats=heats, walls=walls)


def random_script(B, heat, n_ticks, seed, heats_on=lambda t: True, walls_on=lambda t: True, t0=0):
    """n_ticks of random but well-formed words: positions a permutation within each heat, most members class 1, contacts and wall hits
    that come and go, laps that grow, phases that end in 2 or 3."""
    rng = np.random.default_rng(seed)
    heat = None if heat is None else np.asarray(heat, np.int32)
    phase = rng.integers(0, 2, B).astype(np.int32); lap = phase.copy()
    ticks = []
    for k in range(n_ticks):
        t = t0 + k
        up = (rng.random(B) < 0.15) & (phase < 2)
        lap = lap + up
        phase = np.where(up & (phase == 0), 1, phase)
        phase = np.where((phase < 2) & (rng.random(B) < 0.04), 2, phase)
        phase = np.where((phase < 2) & (rng.random(B) < 0.04), 3, phase).astype(np.int32)
        hp = wp = None
        if heat is not None and heats_on(t):
            hp = blank_heats(B, heat)
            for g in np.unique(heat[heat >= 0]):
                mem = np.nonzero(heat == g)[0]
                hp["i32"][R.H_POSITION, mem] = rng.permutation(mem.size)
                hp["i32"][R.H_CLASS, mem] = np.where(rng.random(mem.size) < 0.85, 1, rng.integers(0, 4, mem.size))
                hp["i32"][R.H_NEAREST, mem] = np.where(rng.random(mem.size) < 0.9, rng.choice(mem, mem.size), -1)
                con = rng.random(mem.size) < 0.4
                hp["i32"][R.H_CONTACT, mem] = con
                hp["f64"][R.H_CLEARANCE, mem] = np.where(con, -rng.random(mem.size), rng.random(mem.size))
                hp["f64"][R.H_PROGRESS, mem] = np.where(rng.random(mem.size) < 0.95, 50.0 * rng.standard_normal(mem.size), np.nan)
        if walls_on(t):
            wp = blank_walls(B)
            hit = rng.random(B) < 0.4
            wp["i32"][R.W_HIT] = hit
            wp["i32"][R.W_SIDE] = np.where(hit, rng.choice([-1, 1], B), 0)
            wp["i32"][R.W_CORNER] = np.where(hit, rng.integers(0, 4, B), -1)
            wp["f64"][R.W_DEPTH] = np.where(hit, rng.random(B) * 0.1, 0.0)
            wp["f64"][R.W_IMPULSE] = np.where(hit, rng.random(B) * 3.0, 0.0)
        ticks.append(tick(t, B, phase, lap, np.floor(rng.random(B) * 5000.0), hp, wp))
    return heat, ticks


def interleaved_heats(B, size, every=3):
    """Heats of ``size`` over the vehicles whose index is no multiple of ``every`` (those are in no heat), members interleaved: vehicle
    k of them is in heat k % n_heats, so the members of a heat are spread over the whole index range."""
    heat = np.full(B, -1, np.int32)
    idx = np.nonzero(np.arange(B) % every != 0)[0]
    n = max(1, (idx.size + size - 1) // size)
    heat[idx] = np.arange(idx.size) % n
    return heat


def reversal():
    """B = 300: a heat of 256 (vehicles 0 .. 255) and one of 44.  Tick 0 is first sight; on tick 1 the 256-heat reverses its order:
    every pair flips, 32 640 PASS events, 255 of them by vehicle 255; tick 2 repeats tick 1: nothing."""
    B = 300
    heat = np.array([0] * 256 + [1] * 44, np.int32)
    a = blank_heats(B, heat)
    b = copy_planes(a)
    b["i32"][R.H_POSITION, :256] = 255 - np.arange(256)
    b["f64"][R.H_PROGRESS, :256] = a["f64"][R.H_PROGRESS, :256][::-1]
    return heat, [tick(0, B, heats=a), tick(1, B, heats=b), tick(2, B, heats=copy_planes(b))]


def all_and_none(B):
    """Tick 0 stores; on tick 1 every vehicle's lap counter grows (every vehicle emits); tick 2 repeats tick 1 (none does)."""
    lap1 = np.ones(B, np.int32)
    v = np.arange(B) * 7.0
    return None, [tick(0, B), tick(1, B, np.ones(B), lap1, v), tick(2, B, np.ones(B), lap1, v)]


def crafted():
    """B = 6, one heat of 4 (vehicles 0 .. 3), vehicles 4 and 5 in none; six ticks that contain every kind, a tick on which vehicle 2
    has every kind that can share a tick (LAP, FINISH, three PASSes, CONTACT_BEGIN, WALL_HIT), spells that begin, hold and end with
    their lengths and extrema, and a last tick with no event."""
    B = 6
    heat = np.array([0, 0, 0, 0, -1, -1], np.int32)
    out = []
    h = blank_heats(B, heat); w = blank_walls(B)
    h["i32"][R.H_POSITION, :4] = [0, 1, 3, 2]                                   # vehicle 2 is last
    out.append(tick(0, B, heats=copy_planes(h), walls=copy_planes(w)))         # t = 0: first sight of everything
    # t = 1: vehicle 2 finishes its lap, passes all three, touches vehicle 0 and the wall; vehicle 5 is lost; vehicle 4 hits the wall
    phase = np.array([0, 0, 2, 0, 0, 3]); lap = np.array([0, 0, 1, 0, 0, 0]); lv = np.array([-1.0, -1.0, 231.0, -1.0, -1.0, -1.0])
    h["i32"][R.H_POSITION, :4] = [1, 2, 0, 3]
    h["f64"][R.H_PROGRESS, :4] = [10.0, 9.5, 10.25, 9.0]
    h["i32"][R.H_CONTACT, [0, 2]] = 1; h["i32"][R.H_NEAREST, [0, 2]] = [2, 0]; h["f64"][R.H_CLEARANCE, [0, 2]] = -0.01
    w["i32"][R.W_HIT, [2, 4]] = 1; w["i32"][R.W_SIDE, [2, 4]] = [1, -1]; w["i32"][R.W_CORNER, [2, 4]] = [0, 3]
    w["f64"][R.W_DEPTH, [2, 4]] = [0.02, 0.03]; w["f64"][R.W_IMPULSE, [2, 4]] = [0.5, 0.75]
    out.append(tick(1, B, phase, lap, lv, copy_planes(h), copy_planes(w)))
    # t = 2: the contact deepens and its nearest changes for vehicle 0; the wall spell of vehicle 4 peaks
    h["f64"][R.H_CLEARANCE, [0, 2]] = [-0.04, -0.03]; h["i32"][R.H_NEAREST, 0] = 1
    w["f64"][R.W_IMPULSE, 4] = 1.25; w["f64"][R.W_IMPULSE, 2] = 0.25
    out.append(tick(2, B, phase, lap, lv, copy_planes(h), copy_planes(w)))
    # t = 3: both spells hold, shallower
    h["f64"][R.H_CLEARANCE, [0, 2]] = [-0.02, -0.02]; w["f64"][R.W_IMPULSE, [2, 4]] = [0.125, 0.5]
    out.append(tick(3, B, phase, lap, lv, copy_planes(h), copy_planes(w)))
    # t = 4: everything ends: CONTACT_END of 0 and 2 (length 3), WALL_CLEAR of 2 and 4 (length 3)
    h["i32"][R.H_CONTACT, [0, 2]] = 0; h["f64"][R.H_CLEARANCE, [0, 2]] = 0.3
    w["i32"][R.W_HIT, [2, 4]] = 0; w["i32"][R.W_SIDE, [2, 4]] = 0; w["i32"][R.W_CORNER, [2, 4]] = -1; w["f64"][:2, [2, 4]] = 0.0
    out.append(tick(4, B, phase, lap, lv, copy_planes(h), copy_planes(w)))
    out.append(tick(5, B, phase, lap, lv, copy_planes(h), copy_planes(w)))     # t = 5: nothing
    return heat, out


def run_ref(script, kinds=R.ALL_KINDS):
    """The reference over a script: the list of each tick's events, and the reference itself."""
    heat, ticks = script
    ref = R.EventsRef(ticks[0]["phase"].shape[0], kinds)
    return [ref.step(k["t"], k["phase"], k["lap"], k["lap_value"], k["heats"], heat if k["heats"] is not None else None, k["walls"])
            for k in ticks], ref


# ---- the real race: 8 cars on the L-shaped track in two heats of 4, walls on --------------------------------------------------------
RACE_B, RACE_TICKS = 8, 40
RACE_HEAT = np.array([0] * 4 + [1] * 4, np.int32)
RACE_FOOTPRINT = dict(half_length=0.1, half_width=0.05)
RACE_WALLS = dict(restitution=0.3)


def race_setup():
    """(map, plant0 [8, 8], plant rows, tyre rows).  Cars 0 .. 3 and 7 are tests/_walls_cases.race_setup's: left and right of the centre
    line in turn, each aimed at the wall of its side at 1.4 m/s, so that a front corner meets the wall within the first ticks and
    leaves it again while the controller steers back (WALL_HIT, WALL_CLEAR).  Car 4 starts 0.4 m in front of the line and has its lap
    event within the first dozen ticks (LAP).  Car 6 starts 0.3 m behind car 5 on the long straight at three times its speed and
    drives through it (no interactions are attached): with footprints of 0.2 m the two touch within a few ticks and part again
    (CONTACT_BEGIN, CONTACT_END, and a PASS)."""
    import lpvmpc
    from oracle import plant_ref as PR
    mp = lpvmpc.Map("L_shape", 0.2)
    tab = np.asarray(mp.PointAndTangent, float)
    L = float(mp.TrackLength)
    plant0 = np.zeros((RACE_B, 8))
    for k, slot in ((0, 0), (1, 1), (2, 2), (3, 3), (7, 4)):
        sg = 1.0 if slot % 2 == 0 else -1.0
        x, y, th = PR.get_global_position(tab, 1.2 + 1.6 * slot, sg * 0.12)
        plant0[k] = [x, y, 1.4, 0.0, 0.0, 0.0, th + sg * (0.4 + 0.04 * slot), 0.0]
    x, y, th = PR.get_global_position(tab, L - 0.4, 0.0)
    plant0[4] = [x, y, 1.4, 0.0, 0.0, 0.0, th, 0.0]
    for k, s, ey, v in ((5, 13.3, 0.0, 0.8), (6, 13.0, 0.02, 2.4)):
        x, y, th = PR.get_global_position(tab, s, ey)
        plant0[k] = [x, y, v, 0.0, 0.0, 0.0, th, 0.0]
    return mp, plant0, lpvmpc.sample_plant_params(RACE_B, 23), lpvmpc.tyre_params(RACE_B)
