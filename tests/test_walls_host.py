"""The walls' model on the host (include/lpvmpc.h, "Walls"): physical properties of the numpy restatement (tests/_walls_ref.py), the
Python helpers' checks, corners(), the channel constants and exported symbols, and the gate that makes the GPU comparison meaningful:
the decision margins of the crafted scenes and of the race replay.  No GPU."""
import os
import re

import numpy as np
import pytest

from tests import _walls_cases as K
from tests import _walls_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52


def lshape_table():
    import lpvmpc
    return np.asarray(lpvmpc.Map("L_shape", 0.2).PointAndTangent, float)


def random_hits(n, seed, **words):
    """n cars on the straight (row 4) with a corner beyond the left or right wall, random headings, velocities and yaw rates."""
    from oracle import plant_ref as PR
    rng = np.random.default_rng(seed)
    tab = lshape_table()
    plant = np.zeros((n, 8))
    for b in range(n):
        sg = 1.0 if b % 2 == 0 else -1.0
        x, y, th = PR.get_global_position(tab, 13.2 + rng.uniform(0, 1.0), sg * rng.uniform(0.3, 0.5))
        plant[b] = [x, y, rng.uniform(0.3, 2.0), rng.uniform(-1, 1), 0.1, -0.1, th + rng.uniform(-0.5, 0.5), rng.uniform(-2, 2)]
    rows = K.plant_rows(n)
    return tab, plant, rows, R.tick(plant, rows, tab, K.HALF_WIDTH, R.config(**words))


@pytest.mark.parametrize("words", (dict(), dict(restitution=1.0, friction=0.0), dict(restitution=0.0, friction=5.0), dict(yaw_response=0),
                                   dict(restitution=1.0, friction=0.7, push=1.0)))
def test_kinetic_energy_does_not_rise(words):
    """m |u|^2 / 2 + Iz w^2 / 2 after a hit is at most the energy before, up to 64 * 2^-52 of it: the response is some twenty rounded
    operations on words of the energy's scale, each within 2^-53 relative, and vx, vy and w each enter the energy squared (a factor of
    two), so 64 units bounds the rounding of a step that keeps the energy exactly (restitution 1, no friction).  With yaw_response = 0
    the yaw term is left out on both sides: psiDot is not the response's to change."""
    tab, plant, rows, o = random_hits(200, 11, **words)
    assert o["hit"].sum() >= 150 and (o["impulse"] > 0).sum() >= 50
    worst = -np.inf
    for b in np.nonzero(o["written"])[0]:
        e0, e1 = R.kinetic_energy(plant[b], rows[b]), R.kinetic_energy(o["plant"][b], rows[b])
        worst = max(worst, (e1 - e0) / e0)
        assert e1 <= e0 * (1.0 + 64 * EPS), (b, e0, e1)
    print("kinetic energy, %s: largest relative change %.3g over %d hits" % (words, worst, int(o["written"].sum())))


def test_restitution_without_friction():
    """friction = 0: the corner's normal velocity after the hit is -restitution * vn, to a few units of rounding of the speeds."""
    for e in (0.0, 0.2, 1.0):
        tab, plant, rows, o = random_hits(100, 5, restitution=e, friction=0.0)
        seen = 0
        for b in np.nonzero(o["written"])[0]:
            d = o["detail"][b]
            if not d["vn"] < 0:
                continue
            rx, ry = d["r"]
            ux, uy = d["u2"]
            vn1 = (ux + d["w2"] * -ry) * d["n"][0] + (uy + d["w2"] * rx) * d["n"][1]
            scale = abs(plant[b, 2]) + abs(plant[b, 3]) + abs(plant[b, 7])
            assert abs(vn1 - (-e * d["vn"])) <= 32 * EPS * scale, (e, b, vn1, d["vn"])
            seen += 1
        assert seen >= 30


def test_yaw_response_off_never_changes_psidot_and_untouched_rows_are_kept():
    tab, plant, rows, o = random_hits(100, 7, yaw_response=0)
    assert o["written"].sum() >= 60
    assert np.array_equal(o["plant"][:, 7], plant[:, 7])
    assert np.array_equal(o["plant"][:, [4, 5, 6]], plant[:, [4, 5, 6]])            # ax, ay, yaw are never written
    tab, plant, rows, o = random_hits(100, 7)
    assert np.any(o["plant"][:, 7] != plant[:, 7])
    assert np.array_equal(o["plant"][:, [4, 5, 6]], plant[:, [4, 5, 6]])
    sc, ref = K.case(45)
    keep = ~ref["written"]
    assert keep.sum() >= 16 and sc["plant"][keep].tobytes() == ref["plant"][keep].tobytes()   # bit for bit, NaN included


def test_the_push_removes_its_share_of_the_depth():
    """After the tick the contact corner's depth, measured again at the vehicle's new position with the old heading, is
    (1 - push) * depth on a straight, where the normal does not turn."""
    tab = lshape_table()
    for push in (0.0, 0.5, 1.0):
        _, plant, rows, o = random_hits(60, 3, push=push)
        for b in np.nonzero(o["written"])[0]:
            q = o["corner"][b]
            after = plant[b].copy(); after[[0, 1]] = o["plant"][b, [0, 1]]
            _, pts = R.corners(after[None], R.config())
            ok, ey, _ = R.locate(tab, pts[0, q, 0], pts[0, q, 1], 1.05, lambda k, m: None)
            assert ok and abs((abs(ey) - 0.55) - (1.0 - push) * o["depth"][b]) <= 1e-12, (push, b)


def test_mirror_symmetry_left_wall_against_right_wall():
    """A scene and its mirror image in the centre line of a straight that runs along +x exactly (a table of two straights and two
    half circles): the same depths, impulses and corners of the other hand, vx equal, vy and psiDot negated."""
    r = 1.5
    tab = np.array([[2.0, 0.0, 0.0, 0.0, 2.0, 0.0], [2.0, 2 * r, np.pi, 2.0, np.pi * r, 1 / r], [0.0, 2 * r, np.pi, 2.0 + np.pi * r, 2.0, 0.0],
                    [0.0, 0.0, 0.0, 4.0 + np.pi * r, np.pi * r, 1 / r]])
    rng = np.random.default_rng(2)
    n = 40
    plant = np.zeros((n, 8))
    for b in range(n):
        plant[b] = [rng.uniform(0.6, 1.4), rng.uniform(0.3, 0.5), rng.uniform(0.5, 2), rng.uniform(-1, 1), 0, 0, rng.uniform(-0.4, 0.4), rng.uniform(-1, 1)]
    mirror = plant * np.array([1, -1, 1, -1, 1, -1, -1, -1.0])
    rows = K.plant_rows(n)
    a, b_ = R.tick(plant, rows, tab, 0.3, R.config()), R.tick(mirror, rows, tab, 0.3, R.config())
    assert a["hit"].sum() >= 30 and np.array_equal(a["hit"], b_["hit"]) and np.array_equal(a["side"], -b_["side"])
    swap = np.array([1, 0, 3, 2, -1])
    assert np.array_equal(swap[a["corner"]], b_["corner"])
    assert np.allclose(a["depth"], b_["depth"], rtol=0, atol=1e-14) and np.allclose(a["impulse"], b_["impulse"], rtol=0, atol=1e-13)
    assert np.allclose(a["plant"] * np.array([1, -1, 1, -1, 1, -1, -1, -1.0]), b_["plant"], rtol=0, atol=1e-13)


def test_the_nearest_stretch_of_track_wins_not_the_first_row():
    """Two straights 1.2 m apart running in opposite directions (a narrow hairpin of half circles r = 0.6): a corner between them,
    0.45 m from the second and 0.75 m from the first, is located on the second although the first row accepts it too."""
    r = 0.6
    tab = np.array([[3.0, 0.0, 0.0, 0.0, 3.0, 0.0], [3.0, 2 * r, np.pi, 3.0, np.pi * r, 1 / r], [0.0, 2 * r, np.pi, 3.0 + np.pi * r, 3.0, 0.0],
                    [0.0, 0.0, 0.0, 6.0 + np.pi * r, np.pi * r, 1 / r]])
    margins = {}
    ok, ey, th = R.locate(tab, 1.5, 0.75, 1.05, lambda k, m: margins.__setitem__(k, min(m, margins.get(k, np.inf))))
    assert ok and abs(ey - 0.45) < 1e-12 and abs(abs(th) - np.pi) < 1e-12 and abs(margins["row"] - 0.3) < 1e-12


def test_python_helpers_and_validators():
    from lpvmpc import _ffi, walls as W
    c = W.wall_config(margin=0.1, friction=0.0, yaw_response=False)
    assert (c.margin, c.reach, c.friction, c.yaw_response, c.reserved) == (0.1, 0.5, 0.0, 0, 0)
    for bad in (dict(margin=-0.1), dict(margin=float("nan")), dict(reach=0.0), dict(half_length=0.0), dict(half_width_car=-1.0), dict(restitution=1.5),
                dict(restitution=-0.1), dict(friction=-0.1), dict(friction=float("inf")), dict(push=2.0), dict(yaw_response=2), dict(yaw_response=0.5),
                dict(reserved=0), dict(wake=1.0)):
        with pytest.raises(ValueError):
            W.wall_config(**bad)
    raw = _ffi.WallConfig(0.25, 0.5, 0.4, 0.2, 0.2, 0.3, 0.5, 1, 1)
    with pytest.raises(ValueError):
        W.as_config(raw)                                                        # reserved != 0
    assert W.as_config(dict(push=0.25)).push == 0.25 and W.as_config(None).push == 0.5 and W.as_config(c).margin == 0.1
    assert {k: getattr(W.as_config(None), k) for k in W.DEFAULTS} == R.DEFAULTS == W.DEFAULTS
    k = W.new_carry(5)
    assert k["f64"].shape == (_ffi.WALL_CARRY_F64, 5) and k["i32"].shape == (_ffi.WALL_CARRY_I32, 5) and k["i32"].dtype == np.int32
    assert k["i32"][_ffi.WALL_CARRY_I32_NAMES.index("first_hit_tick")].tolist() == [-1] * 5 and k["i32"].sum() == -5 and not k["f64"].any()
    f = np.arange(4 * 3, dtype=float).reshape(4, 3); i = np.arange(6 * 3, dtype=np.int32).reshape(6, 3)
    d = W.walls_dict(f, i)
    assert np.array_equal(d["impulse"], f[1]) and np.array_equal(d["outside"], i[5]) and d["f64"] is f and d["i32"] is i


def test_corners_are_the_headers():
    from lpvmpc import walls as W
    sc, _ = K.case(45)
    p = sc["plant"][np.isfinite(sc["plant"]).all(axis=1)]
    got = W.corners(p)
    _, want = R.corners(p, R.config())
    assert got.shape == (p.shape[0], 4, 2) and got.tobytes() == want.tobytes()
    one = W.corners([[1.0, 2.0, 0, 0, 0, 0, 0.0, 0]], dict(half_length=0.5, half_width_car=0.25))[0]
    assert one.tolist() == [[1.5, 2.25], [1.5, 1.75], [0.5, 2.25], [0.5, 1.75]]        # front left, front right, rear left, rear right
    with pytest.raises(ValueError):
        W.corners(np.zeros((3, 7)))


def test_python_channel_constants_and_symbols_equal_the_headers():
    from lpvmpc import _ffi
    text = open(os.path.join(ROOT, "include", "lpvmpc.h")).read()
    H = {k: int(v) for k, v in re.findall(r"#define\s+LPVMPC_WALL_(\w+)\s+(\d+)", text)}
    assert (H["F64"], H["I32"], H["CARRY_F64"], H["CARRY_I32"]) == (_ffi.WALL_F64, _ffi.WALL_I32, _ffi.WALL_CARRY_F64, _ffi.WALL_CARRY_I32)
    for names, prefix in ((_ffi.WALL_F64_NAMES, ""), (_ffi.WALL_I32_NAMES, ""), (_ffi.WALL_CARRY_F64_NAMES, "CARRY_"),
                          (_ffi.WALL_CARRY_I32_NAMES, "CARRY_")):
        assert len(names) == H[prefix + ("F64" if names[0] in ("depth", "impulse_total") else "I32")]
        for c, k in enumerate(names):
            assert H[prefix + k.upper()] == c, (prefix, k)
    assert _ffi.WALL_F64_NAMES == R.F64_NAMES and _ffi.WALL_I32_NAMES == R.I32_NAMES
    # the struct, field by field, against the header's declaration order
    body = re.search(r"typedef struct lpvmpc_wall_config \{(.*?)\} lpvmpc_wall_config;", text, re.S).group(1)
    fields = re.findall(r"^\s*(double|int32_t)\s+(\w+);", body, re.M)
    assert [(n, "double" if t is _ffi._d else "int32_t") for n, t in _ffi.WallConfig._fields_] == [(n, t) for t, n in fields]
    # every function the header declares is in _ffi.EXPORTS, and the other way round
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(lpvmpc_\w+)\s*\(", code))
    assert declared == set(_ffi.EXPORTS), sorted(declared ^ set(_ffi.EXPORTS))
    for name in ("lpvmpc_wall_default_config", "lpvmpc_race_walls", "lpvmpc_race_walls_read", "lpvmpc_wall_step_batch"):
        assert name in declared


# ---- the gate of the GPU comparison ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bound", (False, True))
def test_every_decision_of_the_crafted_scenes_holds_by_1e_6(bound):
    sc, ref = K.case(90, bound)
    print("crafted scenes, bound=%s: margins %s" % (bound, {k: "%.3g" % v for k, v in ref["margins"].items()}))
    assert ref["margin"] >= K.MARGIN
    by = dict(zip(sc["names"], range(len(sc["names"]))))
    for site, _, _, _ in K.SITES:
        g = lambda kind, word: ref[word][by[site + "/" + kind]]
        assert g("nose", "hit") == 1 and g("nose", "impulse") > 0 and g("nose", "corner") in (0, 1)
        assert g("glance", "hit") == 1 and 0 < g("glance", "depth") < 0.06
        assert g("slide", "hit") == 1 and g("slide", "impulse") > 0
        assert g("separating", "hit") == 1 and g("separating", "impulse") == 0 and g("separating", "depth") > 0
        assert g("beyond_reach", "hit") == 1 and g("beyond_reach", "outside") == 0
        assert g("centre_outside", "hit") == 1 and g("centre_outside", "outside") == 1
        assert g("lost", "hit") == 0 and g("lost", "outside") == 1
        for kind in ("frozen", "not_finite", "clear"):
            assert g(kind, "hit") == 0 and g(kind, "outside") == 0 and g(kind, "corner") == -1 and g(kind, "hit_ticks") == 0
        assert g("nose_other", "hit") == 1
        if not bound:                                                          # (bound: the two stand on tracks that mirror each other)
            assert g("nose_other", "side") == -g("nose", "side")
    e = by["exact"]
    assert ref["hit"][e] == 1 and ref["corner"][e] in (0, 1) and sc["plant"][e, 6] == 0.0
    assert R.config()["margin"] + K.HALF_WIDTH == 0.55


def test_the_scripted_sequence_and_the_race_replay_hold_their_margins():
    rows = K.plant_rows(3)
    carry, seen = None, []
    tab = lshape_table()
    for t in range(K.SCRIPT_TICKS):
        o = R.tick(K.script(t), rows, tab, K.HALF_WIDTH, R.config(), t=t, carry=carry)
        carry = o["carry"]
        assert o["margin"] >= K.MARGIN, (t, o["margins"])
        seen.append(o["hit"].tolist())
    assert [h[0] for h in seen] == [0, 0, 1, 1, 1, 0, 0, 1, 1, 0, 0, 0] and not any(h[1] for h in seen)
    assert [h[2] for h in seen] == [0] * 4 + [1] * 8
    assert o["hit_ticks"].tolist() == [5, 0, 8] and o["first_hit_tick"].tolist() == [2, -1, 4]
    ticks, margin = K.race_replay()
    hit = np.array([o["wall"]["hit"] for o in ticks])
    print("race replay: smallest decision margin %.3g, hit ticks %s" % (margin, ticks[-1]["wall"]["hit_ticks"].tolist()))
    assert margin >= 1e-9
    assert (ticks[-1]["wall"]["hit_ticks"] > 0).sum() >= 3 and not hit[0].any() and not hit[-1].any()   # hits start and end
    assert all(np.all(o["phase"] == 0) for o in ticks)


def test_the_kick_loses_the_car_without_walls_and_not_with_them():
    """On the host replay: the kicked car is lost (phase 3) within the run without walls, and still racing with hits counted with them;
    the GPU test runs the same two races on the device."""
    plant0, kicks = K.kick_setup()
    out = {}
    for name, cfg in (("open", None), ("walls", {})):
        ref = K.race_ref(wall_cfg=cfg, kicks=kicks, plant0=plant0)
        for _ in range(K.KICK_TICKS):
            ref.tick()
        out[name] = ref
    assert out["open"].phase[K.KICK_CAR] == 3 and np.all(np.delete(out["open"].phase, K.KICK_CAR) == 0)
    assert np.all(out["walls"].phase == 0) and out["walls"].wall["hit_ticks"][K.KICK_CAR] > 0 and out["walls"].margin >= 1e-9
