"""Crafted single ticks of the walls' tests (tests/test_walls_host.py, tests/test_gpu_walls.py), built on the host from track
coordinates: each kind of contact on a straight, on a left arc, on a right arc and across a seam of the L-shaped track, and one vehicle
whose heading and whose wall's track heading are exactly 0.  test_walls_host.py asserts that every decision of every scene holds by a
margin of at least 1e-6 in long double, so the device and the restatement decide alike and only values are compared to a tolerance."""
import numpy as np

from tests import _walls_ref as R

SIZES = (1, 3, 63, 64, 65, 257)     # one quad; a quad tail; both sides of the 64-vehicle workgroup edge; more than four workgroups
MARGIN = 1e-6
HALF_WIDTH = 0.3                    # of the tracks below: the wall stands at |ey| = 0.55, a corner is located to |ey| = 1.05

# (name, ey of the centre, heading offset, vx, vy, psiDot, side): ey, heading offset, vy and psiDot are multiplied by the site's sign
# for that side (SITES below), so that every kind meets the same kind of wall on every site
KINDS = (
    ("nose", 0.25, 0.6, 1.5, 0.0, 0.1, "in"),             # nose-first: the front corner on the wall's side goes deep
    ("glance", 0.33, 0.08, 1.5, 0.0, 0.0, "in"),          # a glancing front corner, 12 mm deep
    ("slide", 0.42, 0.01, 1.0, 0.3, 0.0, "in"),           # both corners of a side beyond the wall, sliding into it
    ("separating", 0.42, 0.02, 1.0, -0.5, 0.0, "in"),     # beyond the wall and moving away: the push and no impulse
    ("beyond_reach", 0.9, 0.05, 1.0, 0.1, 0.0, "out"),    # the wall-side corners beyond reach: the contact is one of the other two
    ("centre_outside", 1.2, 0.05, 1.0, 0.1, 0.0, "out"),  # the centre beyond reach (OUTSIDE) and a far-side corner still located
    ("lost", 2.0, 0.0, 1.0, 0.0, 0.0, "out"),             # nothing located: OUTSIDE, no contact
    ("frozen", 0.25, 0.6, 1.5, 0.0, 0.1, "in"),           # the nose-first car with nstep = 0: neither touched nor counted
    ("not_finite", 0.25, 0.6, 1.5, np.nan, 0.1, "in"),    # vy = NaN: neither touched nor counted
    ("clear", 0.05, 0.02, 1.2, 0.05, 0.02, "in"),         # clear of everything: every word kept
    ("nose_other", -0.25, -0.6, 1.5, 0.0, -0.1, "in"),    # nose-first into the other wall (the inside of a bend)
)
# (name, s of the centre, sign of "in", sign of "out") on the L-shaped track: row 4 (straight), row 1 (left arc), row 2 (right arc) and
# the seam between row 3 (left arc, to s = 12.25) and row 4, the front corners on the straight and the rear ones on the arc.  On the
# bends both signs point to the outside, where a footprint sticks out (towards the inside its corners are nearer the centre line than
# its centre); "nose_other" meets the inside wall
SITES = (("straight", 13.7, 1.0, -1.0), ("left_arc", 3.2, -1.0, -1.0), ("right_arc", 6.6, 1.0, 1.0), ("seam", 12.32, 1.0, -1.0))
# the exact vehicle: heading exactly 0 at the seam between row 5 (left arc) and row 6 (straight, heading exactly 0), sliding into the
# left wall.  Its rear corners are located on the arc, where they are less deep: the front left corner wins on the straight, th = 0
EXACT_X, EXACT_EY = -1.8647889756541158 + 0.3, 0.42


def tracks():
    """The palette of the bound runs: the L-shaped track and its mirror image, both of half width 0.3."""
    import lpvmpc
    from lpvmpc.track import mirrored
    a = lpvmpc.Map("L_shape", 0.2)
    return [a, mirrored(a)]


def templates(tab, mirror=False):
    """The plant rows [45, 8], nstep [45] and names of every kind on every site and the exact vehicle (index 1), placed on the table
    ``tab``; mirror: the scene's mirror image (for the mirrored track)."""
    from oracle import plant_ref as PR
    tab = np.asarray(tab, float)
    flip = -1.0 if mirror else 1.0
    out, nstep, names = [], [], []
    for site, s0, s_in, s_out in SITES:
        for kind, ey, dpsi, vx, vy, w, side in KINDS:
            sg = flip * (s_in if side == "in" else s_out)
            x, y, th = PR.get_global_position(tab, s0, sg * ey)
            out.append([x, y, vx, sg * vy, 0.3, -0.2, th + sg * dpsi, sg * w])
            nstep.append(0 if kind == "frozen" else 7)
            names.append(site + "/" + kind)
    exact = [EXACT_X, flip * EXACT_EY, 1.0, flip * 0.3, 0.1, 0.2, 0.0, 0.0]
    out.insert(1, exact); nstep.insert(1, 7); names.insert(1, "exact")
    return np.array(out), np.array(nstep), names


def plant_rows(B):
    """Plant rows [B, 7] with masses and yaw inertias that differ from vehicle to vehicle."""
    b = np.arange(B)
    rows = np.tile([0.125, 0.125, 1.98, 0.03, 60.0, 60.0, 0.05], (B, 1))
    rows[:, 2] = 1.5 + 0.1 * (b % 7)
    rows[:, 3] = 0.02 + 0.004 * (b % 5)
    return rows


_cache = {}


def case(B, bound=False, cfg=None):
    """The scene of B vehicles: vehicle b is template b % 45, on track b % 2 of tracks() when bound.  Returns (scene, ref): scene a dict
    of plant, rows, nstep, names, track_of (None unbound) and tables / half_width as _walls_ref.tick takes them; ref its result.  Built
    once per (B, bound) and shared; neither is to be changed."""
    key = (B, bound)
    if cfg is None and key in _cache:
        return _cache[key]
    pal = [np.asarray(t.PointAndTangent, float) for t in tracks()]
    t0, n0, names = templates(pal[0])
    t1, _, _ = templates(pal[1], mirror=True)
    n = t0.shape[0]
    idx = np.arange(B) % n
    of = (np.arange(B) % 2) if bound else None
    plant = np.where((of if bound else np.zeros(B, int))[:, None] == 1, t1[idx], t0[idx])
    sc = dict(plant=plant, rows=plant_rows(B), nstep=n0[idx], names=[names[i] for i in idx], track_of=of,
              track=pal if bound else pal[0], half_width=[HALF_WIDTH, HALF_WIDTH] if bound else HALF_WIDTH)
    ref = R.tick(plant, sc["rows"], sc["track"], sc["half_width"], R.config(**(cfg or {})), t=5, nstep=sc["nstep"], track_of=of)
    if cfg is None:
        _cache[key] = (sc, ref)
    return sc, ref


# ---- a scripted 12-tick sequence of 3 cars on the straight (row 4): a hit that starts, lasts and ends twice; a car that stays clear;
# a car beyond the wall on the other side from tick 4 on
SCRIPT_TICKS = 12
_EY0 = [0.1, 0.2, 0.38, 0.45, 0.40, 0.2, 0.1, 0.36, 0.5, 0.2, 0.1, 0.0]


def script(t):
    """Plant rows [3, 8] of tick t of the scripted sequence."""
    from oracle import plant_ref as PR
    import lpvmpc
    tab = np.asarray(lpvmpc.Map("L_shape", 0.2).PointAndTangent, float)
    p = np.zeros((3, 8))
    for b, (ey, dpsi, vy) in enumerate(((_EY0[t], 0.05, 0.2), (0.0, 0.0, 0.0), (-0.2 if t < 4 else -0.45, -0.03, -0.1 * (t % 3)))):
        x, y, th = PR.get_global_position(tab, 13.0 + 0.1 * t, ey)
        p[b] = [x, y, 1.0, vy, 0.0, 0.0, th + dpsi, 0.0]
    return p


# ---- in a race: 8 cars on the L-shaped track, aimed at the walls ----------------------------------------------------------------------
RACE_B, RACE_TICKS = 8, 30
RACE_CFG = dict(restitution=0.3)


def race_setup():
    """(map, plant0 [8, 8], plant rows, tyre rows): the cars 1.6 m apart from s = 1.2 on, left and right of the centre line in turn,
    each aimed at the wall of its side by 0.4 to 0.68 rad at 1.4 m/s, so that a front corner meets the wall within the first ticks while the
    controller steers back; no car reaches its lap event within RACE_TICKS (half_track0 = 0)."""
    import lpvmpc
    from oracle import plant_ref as PR
    mp = lpvmpc.Map("L_shape", 0.2)
    tab = np.asarray(mp.PointAndTangent, float)
    plant0 = np.zeros((RACE_B, 8))
    for k in range(RACE_B):
        sg = 1.0 if k % 2 == 0 else -1.0
        x, y, th = PR.get_global_position(tab, 1.2 + 1.6 * k, sg * 0.12)
        plant0[k] = [x, y, 1.4, 0.0, 0.0, 0.0, th + sg * (0.4 + 0.04 * k), 0.0]
    return mp, plant0, lpvmpc.sample_plant_params(RACE_B, 23), lpvmpc.tyre_params(RACE_B)


def race_ref(wall_cfg=RACE_CFG, kicks=None, plant0=None):
    """A fresh host replay of the race of race_setup() (tests/_walls_ref.walled_race_ref)."""
    mp, p0, prow, tyres = race_setup()
    Ref = R.walled_race_ref()
    return Ref(np.asarray(mp.PointAndTangent, float), p0 if plant0 is None else plant0, None if wall_cfg is None else R.config(**wall_cfg),
               kicks=kicks, tyre_params=tyres, plant_params=prow, half_track0=0, laps=3, half_width=mp.halfWidth, slack=mp.slack)


_replay = {}


def race_replay():
    """The replay of RACE_TICKS ticks, run once and shared: a list of per-tick dicts (plant, local, cmd, phase, iters, status, wall) and
    the replay's smallest decision margin."""
    if not _replay:
        ref = race_ref()
        ticks = []
        for _ in range(RACE_TICKS):
            ref.tick()
            ticks.append(dict(plant=ref.plant.copy(), local=ref.local.copy(), cmd=ref.cmd.copy(), phase=ref.phase.copy(), iters=ref.iters.copy(),
                              status=ref.status.copy(), wall={k: np.array(ref.wall[k]) for k in R.F64_NAMES + R.I32_NAMES}))
        _replay.update(ticks=ticks, margin=ref.margin)
    return _replay["ticks"], _replay["margin"]


# ---- the physical check: a calm fleet, car 2 kicked sideways by a disturbance row at plant step 38 (tick 5) -------------------------------
KICK_CAR, KICK_STEP, KICK_VY, KICK_TICKS = 2, 38, 4.0, 45


def kick_setup():
    """(plant0 [8, 8] on the centre line at 1 m/s, kicks [8, 3] = (kick_step, kick_vy, kick_w), -1: none)."""
    import lpvmpc
    from oracle import plant_ref as PR
    tab = np.asarray(lpvmpc.Map("L_shape", 0.2).PointAndTangent, float)
    plant0 = np.zeros((RACE_B, 8))
    for k in range(RACE_B):
        x, y, th = PR.get_global_position(tab, 1.2 + 1.6 * k, 0.0)
        plant0[k] = [x, y, 1.0, 0.0, 0.0, 0.0, th, 0.0]
    kicks = np.zeros((RACE_B, 3)); kicks[:, 0] = -1
    kicks[KICK_CAR] = [KICK_STEP, KICK_VY, 0.0]
    return plant0, kicks
