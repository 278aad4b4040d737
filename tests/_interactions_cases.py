"""Crafted scenes of the interactions' GPU tests (tests/test_gpu_interactions.py), built and checked on the host: every scene's wake
and overlap decisions hold by a margin of at least 1e-6 in long double (asserted here), so the device and the restatement decide
alike and only values are compared to a tolerance."""
import numpy as np

from tests import _interactions_ref as R

SIZES = (1, 2, 5, 65, 256)          # no partner; the smallest pair; an odd tail in the unrolled loop; one lane in the second wavefront; a full block
MARGIN = 1e-6

# local frame, heading +x, the drawn car's footprint 0.8 x 0.4: (x, y, vx, vy, what)
PILE = [(0.0, 0.0, 1.0, 0.0, "pile centre: hits the car ahead, is hit from the side -- two contacts"),
        (0.7, 0.03, 0.6, 0.0, "ahead of the centre and slower: nose to tail"),
        (0.1, 0.35, 1.0, -0.2, "beside the centre, drifting into it: side by side (and across the car ahead)")]
FROZEN = (-0.7, 0.0, 1.5, 0.0, "frozen (nstep 0) on top of the pile's tail: neither touched nor seen")
POSELESS = (-1.3, 0.0, 1.0, 0.0, "x = NaN: neither touched nor seen")
NOSE_TAIL = [(5.0, 2.0, 1.4, 0.0, "rear car, faster"), (5.75, 2.0, 0.8, 0.0, "front car")]
SIDE = [(10.0, -2.0, 1.0, 0.1, "drifting left into its neighbour"), (10.05, -1.65, 1.0, -0.1, "drifting right")]


def template(n):
    """n members in member order with what each one is: (cars [n, 4], frozen index or -1, pose-less index or -1)."""
    if n == 1:
        return np.array([PILE[0][:4]]), -1, -1
    if n == 2:
        return np.array([PILE[0][:4], PILE[1][:4]]), -1, -1
    cars = [c[:4] for c in PILE] + [FROZEN[:4], POSELESS[:4]]
    frozen, poseless = 3, 4
    if n > 5:
        cars += [c[:4] for c in NOSE_TAIL + SIDE]
        k = 0
        while len(cars) < n:                                               # the drafting train behind the pile, 0.9 m apart, staggered
            cars.append((-2.05 - 0.9 * k, 0.04 * (k % 2), 1.0 + 0.01 * (k % 3), 0.0))
            k += 1
    return np.array(cars[:n]), frozen, poseless


def scene(n, yaw=0.0, wobble=0.0, heats=2, loose=3):
    """``heats`` heats of n members each, every heat the same template at the same place (they must not see each other), and ``loose``
    vehicles in no heat on top of the pile, interleaved in vehicle order.  yaw: the heading of the whole scene; wobble: a per-car
    heading offset of that size.  Returns dict(plant, rows, heat, nstep) -- checked: the margin of every decision is >= 1e-6."""
    cars, frozen, poseless = template(n)
    c0, s0 = np.cos(yaw), np.sin(yaw)
    B = heats * n + loose
    plant = np.zeros((B, 8)); rows = np.zeros((B, 7)); heat = np.full(B, -1); nstep = np.ones(B, int)
    order = []
    for k in range(n):                                                     # vehicle order: member k of heat 0, of heat 1, ..., then maybe a loose one
        for g in range(heats):
            order.append((g, k))
        if k < loose:
            order.append((-1, k))
    for k in range(max(0, loose - n)):
        order.append((-1, n + k))
    assert len(order) == B
    for b, (g, k) in enumerate(order):
        x, y, vx, vy = cars[k] if g >= 0 else (0.05 * k, 0.02, 1.0, 0.0)
        th = yaw + (wobble * np.sin(1.0 + k) if g >= 0 else 0.0)
        plant[b] = [c0 * x - s0 * y, s0 * x + c0 * y, vx, vy, 0.1 * (k % 3), -0.05 * (k % 2), th, 0.02 * (k % 5)]
        rows[b] = [0.125, 0.125, 1.5 + 0.1 * (k % 7), 0.03, 60.0, 60.0, 0.05 + 0.001 * (k % 5)]
        heat[b] = g
        if g >= 0 and k == frozen:
            nstep[b] = 0
        if g >= 0 and k == poseless:
            plant[b, 0] = np.nan
    return dict(plant=plant, rows=rows, heat=heat, nstep=nstep)


_cache = {}


def case(n, kind):
    """(scene, restatement's tick of it), computed once: kind "general" (heading 0.7, headings wobbling by 0.03) or "aligned" (every
    heading exactly 0: cos = 1, sin = 0 on both sides)."""
    key = (n, kind)
    if key not in _cache:
        sc = scene(n, yaw=0.7, wobble=0.03) if kind == "general" else scene(n)
        ref = R.tick(sc["plant"], sc["rows"], sc["heat"], R.config(), t=5, nstep=sc["nstep"])
        assert ref["margin"] >= MARGIN, (n, kind, ref["margin"])
        _cache[key] = (sc, ref)
    return _cache[key]


def script(t):
    """Tick t of the scripted 12-tick sequence of 4 cars in one heat (car 3 joins no heat): car 1 closes on car 0 and overlaps on ticks
    3-5 and again on 8-9; car 2 picks up car 0's draft on ticks 1-6 and loses it sideways."""
    gap01 = [1.5, 1.2, 0.95, 0.75, 0.7, 0.78, 0.9, 0.85, 0.76, 0.72, 0.9, 1.3][t]
    lat2 = [0.5, 0.1, 0.1, 0.05, 0.0, 0.1, 0.2, 0.45, 0.6, 0.6, 0.6, 0.6][t]
    plant = np.zeros((4, 8))
    plant[0] = [0.0, 0.0, 1.0, 0.0, 0, 0, 0.0, 0]
    plant[1] = [-gap01, 0.02, 1.3, 0.0, 0, 0, 0.0, 0]
    plant[2] = [-2.6, lat2, 1.0, 0.0, 0, 0, 0.0, 0]
    plant[3] = [-0.3, 0.0, 1.0, 0.0, 0, 0, 0.0, 0]
    return plant


SCRIPT_HEAT = np.array([0, 0, 0, -1])
SCRIPT_TICKS = 12
