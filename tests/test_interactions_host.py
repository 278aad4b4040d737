"""The interactions' model on the host (include/lpvmpc.h, "Interactions"): physical invariants of the numpy restatement
(tests/_interactions_ref.py), the Python helpers' checks, grid() and the channel constants.  No GPU."""
import os
import re

import numpy as np
import pytest

from tests import _heats_ref as HR
from tests import _interactions_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52


def rows_of(B, m=None, mu=0.05):
    rows = np.tile([0.125, 0.125, 1.98, 0.03, 60.0, 60.0, mu], (B, 1))
    if m is not None:
        rows[:, 2] = m
    return rows


def car(x, y, yaw=0.0, vx=1.0, vy=0.0):
    return [x, y, vx, vy, 0.0, 0.0, yaw, 0.0]


def world_u(p):
    c, s = np.cos(p[6]), np.sin(p[6])
    return np.array([c * p[2] - s * p[3], s * p[2] + c * p[3]])


def random_scene(rng, n, box=1.2):
    plant = np.zeros((n, 8))
    plant[:, 0] = rng.uniform(0, box, n); plant[:, 1] = rng.uniform(0, box, n)
    plant[:, 2] = rng.uniform(0.8, 2.0, n); plant[:, 3] = rng.uniform(-0.2, 0.2, n)
    plant[:, 6] = rng.uniform(-np.pi, np.pi, n)
    return plant, rows_of(n, m=rng.uniform(1.0, 3.0, n))


def test_momentum_is_kept_where_no_clamp_fires():
    """sum m u over a heat's participants is unchanged by a tick to 64 * 2^-52 * sum m |u|: every pair's two impulses are one J times
    +-n, so only the round-off of the world -> body -> world round trip is left."""
    rng = np.random.default_rng(7)
    checked = hits = 0
    for trial in range(60):
        n = int(rng.integers(2, 9))
        plant, rows = random_scene(rng, n)
        o = R.tick(plant, rows, np.zeros(n, int), R.config(restitution=float(rng.uniform(0, 1))))
        c, s = np.cos(plant[:, 6]), np.sin(plant[:, 6])
        if np.any(o["written"] & (o["plant"][:, 2] == 0.0)):
            continue                                                       # a vx clamp fired
        p0, scale = R.world_momentum(plant, rows, np.arange(n))
        p1, _ = R.world_momentum(o["plant"], rows, np.arange(n))
        assert np.all(np.abs(p1 - p0) <= 64 * EPS * scale), (trial, p1 - p0, scale)
        checked += 1; hits += int(o["hit"].sum())
    assert checked >= 20 and hits >= 20


@pytest.mark.parametrize("e", [0.0, 0.3, 1.0])
def test_restitution_of_a_single_pair(e):
    """The normal relative velocity afterwards is -restitution times the one before; restitution 1 keeps the pair's translational
    kinetic energy, restitution 0 leaves a closing speed of 0."""
    plant = np.array([car(0.0, 0.0, 0.1, 1.5), car(0.7, 0.05, -0.2, 0.6)])   # nose to tail, the rear car faster
    rows = rows_of(2, m=[1.5, 2.5])
    o = R.tick(plant, rows, [0, 0], R.config(restitution=e, push=0.0))
    assert o["hit"].tolist() == [1, 1] and o["impulse"][0] > 0 and o["impulse"][0] == o["impulse"][1]
    # the normal, from the impulse itself
    du0 = world_u(o["plant"][0]) - world_u(plant[0])
    nrm = -du0 / np.linalg.norm(du0)
    vn0 = (world_u(plant[1]) - world_u(plant[0])) @ nrm
    vn1 = (world_u(o["plant"][1]) - world_u(o["plant"][0])) @ nrm
    assert vn0 < 0 and abs(vn1 + e * vn0) <= 1e-14
    ke = lambda P: 0.5 * sum(rows[b, 2] * world_u(P[b]) @ world_u(P[b]) for b in range(2))
    if e == 1.0:
        assert abs(ke(o["plant"]) - ke(plant)) <= 1e-14 * ke(plant)
    else:
        assert ke(o["plant"]) < ke(plant)
    if e == 0.0:
        assert abs(vn1) <= 1e-15


def test_relabelling_a_pair_mirrors_the_impulses():
    plant = np.array([car(0.0, 0.0, 0.1, 1.5, 0.1), car(0.6, 0.1, 0.4, 0.6, -0.05)])
    rows = rows_of(2, m=[1.5, 2.5])
    a = R.tick(plant, rows, [0, 0], R.config())
    b = R.tick(plant[::-1], rows[::-1], [0, 0], R.config())
    assert a["hit"].tolist() == [1, 1]
    np.testing.assert_allclose(a["plant"], b["plant"][::-1], rtol=0, atol=1e-14)
    np.testing.assert_allclose(a["impulse"], b["impulse"][::-1], rtol=0, atol=1e-14)
    np.testing.assert_allclose(a["shelter"], b["shelter"][::-1], rtol=0, atol=1e-14)


def test_a_rigid_motion_moves_the_result_with_it():
    rng = np.random.default_rng(3)
    plant, rows = random_scene(rng, 6, box=1.0)
    th, tx, ty = 0.83, -2.0, 5.0
    Rm = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])

    def move(P):
        Q = P.copy()
        Q[:, :2] = P[:, :2] @ Rm.T + [tx, ty]
        Q[:, 6] = P[:, 6] + th
        return Q
    a = R.tick(plant, rows, np.zeros(6, int), R.config())
    b = R.tick(move(plant), rows, np.zeros(6, int), R.config())
    assert a["hit"].sum() >= 2 and min(a["margin"], b["margin"]) > 1e-9
    assert np.array_equal(a["hit"], b["hit"]) and np.array_equal(a["leader"], b["leader"])
    np.testing.assert_allclose(move(a["plant"]), b["plant"], rtol=0, atol=1e-13)
    np.testing.assert_allclose(a["shelter"], b["shelter"], rtol=0, atol=1e-13)
    np.testing.assert_allclose(a["impulse"], b["impulse"], rtol=0, atol=1e-13)


def test_a_separating_pair_is_pushed_but_gets_no_impulse():
    plant = np.array([car(0.0, 0.0, 0.0, 0.5), car(0.7, 0.0, 0.0, 1.5)])     # overlapping, the front car faster
    o = R.tick(plant, rows_of(2), [0, 0], R.config(push=0.5))
    assert o["hit"].tolist() == [1, 1] and o["impulse"].tolist() == [0.0, 0.0]
    assert np.array_equal(o["plant"][:, 2:], plant[:, 2:])                   # velocities word for word (heading 0: no round-off)
    assert o["plant"][0, 0] < 0.0 and o["plant"][1, 0] > 0.7                 # pushed apart along x
    assert abs((o["plant"][1, 0] - o["plant"][0, 0]) - (0.7 + 0.5 * 0.1)) <= 1e-15


@pytest.mark.parametrize("pos, yaw, inside", [
    ((-1.0, 0.0), 0.0, True),            # behind the leader, on its axis
    ((-3.0, 0.0), 0.0, False),           # on the wake's far edge (lon == wake_length)
    ((-3.5, 0.0), 0.0, False),           # beyond it
    ((-1.0, 0.3), 0.0, False),           # on the side edge (|lat| == wake_half_width)
    ((-1.0, -0.5), 0.0, False),          # outside it
    ((1.0, 0.0), 0.0, False),            # ahead of the leader
    ((0.0, 0.25), 0.0, False),           # level with it (lon == 0)
    ((-1.0, 0.0), np.pi, False),         # facing the other way
    ((-1.0, 0.0), np.pi / 2, False),     # across (align == cos(pi / 2) > 0 by 6e-17 only in float64 -- contact off, no margin asked)
])
def test_shelter_is_zero_outside_the_wake(pos, yaw, inside):
    plant = np.array([car(0.0, 0.0), car(pos[0], pos[1], yaw)])
    if yaw == np.pi / 2:
        plant[1, 6] = 1.6                                                   # clearly past the quarter turn
    o = R.tick(plant, rows_of(2), [0, 0], R.config(contact=0))
    ahead = pos == (1.0, 0.0)                                               # then car 0 is the one in a wake: car 1's
    assert (o["shelter"][0] > 0) == ahead and o["leader"][0] == (1 if ahead else -1)
    assert (o["shelter"][1] > 0) == inside and (o["leader"][1] == 0) == inside
    if inside:
        assert abs(o["shelter"][1] - (1 - 1.0 / 3.0)) <= 1e-15
        assert o["mu_live"][1] == 0.05 * (1.0 - 0.3 * o["shelter"][1]) and o["mu_live"][0] == 0.05
    else:
        assert o["mu_live"][1] == 0.05 and (o["mu_live"][0] == 0.05) != ahead
    assert np.array_equal(o["plant"], plant)


def test_max_picks_the_lowest_index_on_a_tie():
    """Two leaders side by side, the follower centred behind them: both shelters are the same word, the lower index leads."""
    plant = np.array([car(0.0, 0.25), car(0.0, -0.25), car(-1.0, 0.0)])
    o = R.tick(plant, rows_of(3), [0, 0, 0], R.config(contact=0, wake_half_width=0.5))
    assert o["shelter"][2] > 0 and o["leader"][2] == 0
    o = R.tick(plant[[1, 0, 2]], rows_of(3), [0, 0, 0], R.config(contact=0, wake_half_width=0.5))
    assert o["leader"][2] == 0


def test_all_off_changes_no_word():
    rng = np.random.default_rng(11)
    plant, rows = random_scene(rng, 8, box=0.8)
    o = R.tick(plant, rows, np.zeros(8, int), R.config(draft_gain=0.0, contact=0))
    assert np.array_equal(o["plant"], plant) and np.array_equal(o["mu_live"], rows[:, 6]) and not o["written"].any()
    assert o["hit"].sum() == 0 and o["impulse_total"].sum() == 0


def test_frozen_and_pose_less_members_are_neither_touched_nor_seen():
    plant = np.array([car(0.0, 0.0), car(-0.7, 0.0, vx=1.5), car(-0.7, 0.05, vx=1.5), car(-1.5, 0.0)])
    plant[2, 6] = np.nan
    o = R.tick(plant, rows_of(4), [0, 0, 0, 0], R.config(), nstep=[1, 0, 1, 1])
    assert o["part"].tolist() == [True, False, False, True]
    assert o["hit"].tolist() == [0, 0, 0, 0] and o["leader"].tolist() == [-1, -1, -1, 0]
    assert np.array_equal(o["plant"][:, :6], plant[:, :6])


def test_config_validators():
    from lpvmpc import _ffi, interactions as I
    c = I.interaction_config()
    assert {k: getattr(c, k) for k in I.DEFAULTS} == I.DEFAULTS == R.DEFAULTS
    c = I.interaction_config(draft_gain=0, wake_length=1.5, contact=False, restitution=1, push=0)
    assert (c.draft_gain, c.wake_length, c.contact, c.restitution, c.push) == (0.0, 1.5, 0, 1.0, 0.0)
    for bad in (dict(draft_gain=-0.1), dict(draft_gain=1.1), dict(draft_gain=float("nan")), dict(wake_length=0.0), dict(wake_length=float("inf")),
                dict(wake_half_width=-1.0), dict(wake_half_width=0), dict(contact=2), dict(contact=0.5), dict(restitution=-1e-9),
                dict(restitution=1.5), dict(push=2.0), dict(push=float("nan")), dict(gain=0.1)):
        with pytest.raises(ValueError):
            I.interaction_config(**bad)
    assert I.as_config(dict(push=0.25)).push == 0.25 and I.as_config(None).push == 0.5 and I.as_config(c).wake_length == 1.5
    k = I.new_carry(5)
    assert k["f64"].shape == (_ffi.INTER_CARRY_F64, 5) and k["i32"].shape == (_ffi.INTER_CARRY_I32, 5) and k["i32"].dtype == np.int32
    assert k["i32"][_ffi.INTER_CARRY_I32_NAMES.index("first_hit_tick")].tolist() == [-1] * 5 and k["i32"].sum() == -5 and not k["f64"].any()
    f = np.arange(4 * 3, dtype=float).reshape(4, 3); i = np.arange(5 * 3, dtype=np.int32).reshape(5, 3)
    d = I.interactions_dict(f, i)
    assert d["mu"] is not None and np.array_equal(d["mu"], f[1]) and np.array_equal(d["draft_ticks"], i[4]) and d["f64"] is f


def test_python_channel_constants_equal_the_headers():
    from lpvmpc import _ffi
    text = open(os.path.join(ROOT, "include", "lpvmpc.h")).read()
    H = {k: int(v) for k, v in re.findall(r"#define\s+LPVMPC_INTER_(\w+)\s+(\d+)", text)}
    assert (H["F64"], H["I32"], H["CARRY_F64"], H["CARRY_I32"]) == (_ffi.INTER_F64, _ffi.INTER_I32, _ffi.INTER_CARRY_F64, _ffi.INTER_CARRY_I32)
    for names, prefix in ((_ffi.INTER_F64_NAMES, ""), (_ffi.INTER_I32_NAMES, ""), (_ffi.INTER_CARRY_F64_NAMES, "CARRY_"),
                          (_ffi.INTER_CARRY_I32_NAMES, "CARRY_")):
        for c, k in enumerate(names):
            assert H[prefix + k.upper()] == c, (prefix, k)
    assert len(_ffi.INTER_F64_NAMES) == H["F64"] and len(_ffi.INTER_I32_NAMES) == H["I32"]
    assert len(_ffi.INTER_CARRY_F64_NAMES) == H["CARRY_F64"] and len(_ffi.INTER_CARRY_I32_NAMES) == H["CARRY_I32"]
    assert _ffi.INTER_F64_NAMES == R.F64_NAMES and _ffi.INTER_I32_NAMES == R.I32_NAMES
    # the struct, field by field, against the header's declaration order
    body = re.search(r"typedef struct lpvmpc_interaction_config \{(.*?)\} lpvmpc_interaction_config;", text, re.S).group(1)
    fields = re.findall(r"^\s*(double|int32_t)\s+(\w+);", body, re.M)
    assert [(n, "double" if t is _ffi._d else "int32_t") for n, t in _ffi.InteractionConfig._fields_] == [(n, t) for t, n in fields]
    for name in ("lpvmpc_interaction_default_config", "lpvmpc_race_interactions", "lpvmpc_race_interactions_read", "lpvmpc_interaction_step_batch"):
        assert name in _ffi.EXPORTS and re.search(r"\b%s\(" % name, text)


def test_grid_places_footprints_with_positive_clearance_on_every_track():
    """On each of the package's tracks: n cars behind the line, gap metres apart along the centre line, alternating +-stagger, every
    pair of footprints clear (the drawn car in line, half-size footprints where cars stand side by side), every car inside the track and heading along it.  (The transform is passed in: the package's own is a
    device kernel.)"""
    from lpvmpc import interactions as I
    from lpvmpc.track import palette
    from oracle import plant_ref as PR
    for mp in palette():
        tab = np.asarray(mp.PointAndTangent, float)
        where = lambda s, ey: PR.get_global_position(tab, s, ey)
        for n, gap, stagger, hl, hw in ((8, 1.0, 0.0, 0.4, 0.2), (8, 0.6, 0.12, 0.2, 0.1), (3, 1.0, -0.1, 0.4, 0.2)):
            plant0, turns0 = I.grid(mp, n, gap, stagger, position=where)
            assert plant0.shape == (n, 8) and turns0.tolist() == [-1] * n and np.all(plant0[:, 2] == 1.0)
            sep, _ = HR.sep_matrix(plant0[:, [0, 1, 6]], hl, hw)
            assert float(sep[~np.eye(n, dtype=bool)].min()) > 0, (mp.shape, n, gap, stagger)
            for k in range(n):
                s, ey, epsi, inside = PR.get_local_position(tab, mp.halfWidth, mp.slack, *plant0[k, [0, 1, 6]])
                want = stagger if k % 2 == 0 else -stagger
                assert inside and abs(s - (mp.TrackLength - (k + 1) * gap)) <= 1e-9 and abs(ey - want) <= 1e-9 and abs(epsi) <= 1e-9
    mp = palette()[0]
    for bad in ((0, 0.9, 0.0), (4, 0.0, 0.0), (4, 0.9, 5.0), (100, 0.9, 0.0), (4, float("nan"), 0.0)):
        with pytest.raises(ValueError):
            I.grid(mp, *bad, position=lambda s, ey: (0.0, 0.0, 0.0))
