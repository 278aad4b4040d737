"""Crafted scenes of the contact model's tests (tests/test_contact_host.py, tests/test_gpu_contact.py), built and checked on the host.
The scenes of tests/_interactions_cases.py are reused as they are (two co-located heats of n members and three loose vehicles; they
carry non-zero psiDot and Iz); a third heat, far away, holds the kinds the corner form is about: a T-bone ahead of and one behind the
struck car's centre, an angled corner into a side, a laterally offset nose-to-tail hit, two cars rubbing side by side and a three-car
pile-up of cars at different headings.  With n >= 65 seventy lone cars come first in that heat, so that its contacts sit in the second
wavefront of a 256-thread block.  Every hard decision of every scene holds by at least 1e-6 in long double, every clip by as much
unless it sits on its threshold (tests/_contact_ref.py), and no pair reaches the rule for an empty contact interval: asserted here."""
import numpy as np

from tests import _contact_ref as CR
from tests import _interactions_cases as K
from tests import _interactions_ref as R

SIZES = K.SIZES
MARGIN = K.MARGIN
PAD = 70

# local frame, the drawn car's footprint 0.8 x 0.4: name -> [(x, y, heading, vx, vy, psiDot)]
KINDS = dict(
    tbone_fore=[(0.0, 0.0, 0.0, 1.0, 0.0, 0.0), (0.17, -0.56, 1.45, 1.5, 0.0, 0.05)],        # the striker's nose in the right side, ahead of the centre
    tbone_aft=[(0.0, 0.0, 0.0, 1.0, 0.0, 0.0), (-0.23, -0.56, 1.45, 1.5, 0.0, -0.05)],       # ... behind the centre
    corner=[(0.0, 0.0, 0.0, 1.0, 0.0, 0.1), (-0.1552, -0.5373, 0.5, 1.3, 0.0, -0.1)],        # a front corner driven into the right side
    offset_tail=[(0.0, 0.0, 0.0, 1.4, 0.0, 0.0), (0.75, 0.1, 0.0, 0.8, 0.0, 0.0)],           # nose to tail, the front car 0.1 to the left
    rubbing=[(0.0, 0.0, 0.0, 1.2, 0.0, 0.02), (0.1, 0.37, 0.0, 0.8, -0.1, -0.02)],           # side by side, different speeds, drifting together
    pile=[(0.0, 0.0, 0.0, 1.0, 0.0, 0.1), (0.7, 0.05, 0.1, 0.6, 0.0, -0.1), (0.1, 0.35, -0.15, 1.0, -0.2, 0.05)])
ORDER = ("tbone_fore", "tbone_aft", "corner", "offset_tail", "rubbing", "pile")
ORIGIN = (40.0, 30.0)               # of the third heat; the kinds 6 m apart in y, out of each other's wakes
ROW = [0.125, 0.125, 1.5, 0.03, 60.0, 60.0, 0.05]


def kinds_heat(yaw=0.0, wobble=0.0, pad=0, aligned_only=False):
    """The third heat's vehicles in member order: (plant [m, 8], rows [m, 7], where: kind -> indices into them).  aligned_only: the
    kinds every heading of which is exactly 0."""
    c0, s0 = np.cos(yaw), np.sin(yaw)
    plant, rows, where = [], [], {}
    for k in range(pad):                                                   # lone cars, 2 m apart in x, seen by nobody
        x, y = ORIGIN[0] + 2.0 * k, ORIGIN[1] - 8.0
        plant.append([c0 * x - s0 * y, s0 * x + c0 * y, 1.0, 0.0, 0.0, 0.0, yaw, 0.01])
        rows.append(ROW)
    for q, kind in enumerate(ORDER):
        cars = KINDS[kind]
        if aligned_only and any(c[2] != 0.0 for c in cars):
            continue
        where[kind] = list(range(len(plant), len(plant) + len(cars)))
        for j, (x, y, th, vx, vy, w) in enumerate(cars):
            x, y = ORIGIN[0] + x, ORIGIN[1] + 6.0 * q + y
            plant.append([c0 * x - s0 * y, s0 * x + c0 * y, vx, vy, 0.05, -0.05, yaw + th + wobble * np.sin(2.0 + q + j), w])
            r = list(ROW); r[2] = 1.5 + 0.2 * j + 0.1 * q; r[3] = 0.03 + 0.004 * j
            rows.append(r)
    return np.array(plant), np.array(rows), where


def scene(n, yaw=0.0, wobble=0.0):
    """K.scene(n, yaw, wobble) with the third heat appended: dict(plant, rows, heat, nstep, where: kind -> vehicle indices)."""
    sc = K.scene(n, yaw=yaw, wobble=wobble)
    p, r, where = kinds_heat(yaw, wobble, pad=PAD if n >= 65 else 0)
    B0 = sc["plant"].shape[0]
    return dict(plant=np.vstack([sc["plant"], p]), rows=np.vstack([sc["rows"], r]), heat=np.concatenate([sc["heat"], np.full(len(p), 2)]),
                nstep=np.concatenate([sc["nstep"], np.ones(len(p), int)]), where={k: [B0 + i for i in v] for k, v in where.items()})


def checked(ref, what):
    assert ref["margin"] >= MARGIN and ref["clip_margin"] >= MARGIN and ref["empty"] == 0, (what, ref["margin"], ref["clip_margin"], ref["empty"])
    return ref


_cache = {}


def case(n, kind, ccfg=None):
    """(scene, restatement's tick of it at t = 5 under the default configurations), computed once: kind "general" (heading 0.7,
    headings wobbling by 0.03) or "aligned" (the frame's heading exactly 0, no wobble: every car of the reused scenes, of the offset
    nose-to-tail hit and of the rubbing pair has heading exactly 0)."""
    key = (n, kind)
    if key not in _cache:
        sc = scene(n, yaw=0.7, wobble=0.03) if kind == "general" else scene(n)
        ref = checked(CR.tick(sc["plant"], sc["rows"], sc["heat"], R.config(), CR.config(), t=5, nstep=sc["nstep"]), key)
        _cache[key] = (sc, ref)
    return _cache[key]


def exact_vehicles(sc):
    """Vehicles whose own heading and whose heat-mates' headings within reach are exactly 0 in an "aligned" scene: every vehicle of the
    reused scenes and of the kinds without a turned car."""
    ok = np.ones(sc["plant"].shape[0], bool)
    for kind, idx in sc["where"].items():
        if any(c[2] != 0.0 for c in KINDS[kind]):
            ok[idx] = False
    return ok


def pair_scene(kind, yaw=0.0):
    """One kind alone in one heat: (plant, rows, heat)."""
    p, r, where = kinds_heat(yaw)
    idx = where[kind]
    return p[idx], r[idx], np.zeros(len(idx), int)


def script(t):
    """Tick t of the scripted 12-tick sequence: K.script's four cars, car 1 closing on car 0 with a lateral offset that changes sign,
    so that the yaw kicks of the two hits (ticks 3-5 and 8-9) differ in sign."""
    p = K.script(t)
    p[1, 1] = 0.06 if t < 7 else -0.05
    p[:, 7] = [0.0, 0.02, 0.0, 0.0]
    return p


SCRIPT_HEAT, SCRIPT_TICKS = K.SCRIPT_HEAT, K.SCRIPT_TICKS
