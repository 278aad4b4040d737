"""The contact model on the host (include/lpvmpc.h, "Contact model"): physical invariants and scene properties of the numpy
restatement (tests/_contact_ref.py), the crafted scenes' decision margins, the Python helpers' checks and the channel constants.
No GPU."""
import os
import re

import numpy as np
import pytest

from tests import _contact_cases as C
from tests import _contact_ref as CR
from tests import _interactions_cases as K
from tests import _interactions_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52


def rows_of(B, m=None, iz=None):
    rows = np.tile([0.125, 0.125, 1.98, 0.03, 60.0, 60.0, 0.05], (B, 1))
    if m is not None:
        rows[:, 2] = m
    if iz is not None:
        rows[:, 3] = iz
    return rows


def car(x, y, yaw=0.0, vx=1.0, vy=0.0, w=0.0):
    return [x, y, vx, vy, 0.0, 0.0, yaw, w]


def tick(plant, rows, cfg=None, ccfg=None):
    return CR.tick(plant, rows, np.zeros(len(plant), int), R.config(**(cfg or {})), CR.config(**(ccfg or {})))


def world_u(p):
    c, s = np.cos(p[6]), np.sin(p[6])
    return np.array([c * p[2] - s * p[3], s * p[2] + c * p[3]])


def test_an_isolated_pair_keeps_both_momenta_and_gains_no_energy():
    """Seeded random pairs on which no vx clamp acts: linear momentum is kept to 64 * 2^-52 * sum m |u| (the interactions' bound),
    angular momentum about the origin, sum m (c x u) + Iz w at the positions before the push, to the same bound scaled by the lever
    arms, and the kinetic energy, rotation included, never rises beyond 64 * 2^-52 of itself; no pair reaches the rule for an empty
    contact interval."""
    rng = np.random.default_rng(1)
    checked = 0
    worst = [0.0, 0.0, -np.inf]
    for trial in range(1500):
        plant = np.zeros((2, 8))
        plant[0, :2] = rng.uniform(-0.5, 0.5, 2); plant[1, :2] = plant[0, :2] + rng.uniform(-1, 1, 2)
        plant[:, 6] = rng.uniform(-np.pi, np.pi, 2)
        plant[:, 2] = rng.uniform(0.8, 2.0, 2); plant[:, 3] = rng.uniform(-0.3, 0.3, 2); plant[:, 7] = rng.normal(size=2) * 2
        rows = rows_of(2, m=rng.uniform(1.0, 3.0, 2), iz=rng.uniform(0.02, 0.06, 2))
        o = tick(plant, rows, dict(restitution=float(rng.uniform(0, 1))), dict(friction=float(rng.uniform(0, 1.5))))
        if not o["hit"].any():
            continue
        assert o["empty"] == 0 and o["hit"].tolist() == [1, 1] and o["partners"].tolist() == [1, 1]
        if np.any(o["plant"][:, 2] == 0.0):
            continue                                                       # a vx clamp fired
        sel = np.arange(2)
        p0, scale = R.world_momentum(plant, rows, sel)
        p1, _ = R.world_momentum(o["plant"], rows, sel)
        assert np.all(np.abs(p1 - p0) <= 64 * EPS * scale), (trial, p1 - p0, scale)
        L0, lscale = CR.angular_momentum(plant, rows, sel, plant)
        L1, _ = CR.angular_momentum(o["plant"], rows, sel, plant)
        assert abs(L1 - L0) <= 64 * EPS * lscale, (trial, L1 - L0, lscale)
        E0, E1 = CR.energy(plant, rows, sel), CR.energy(o["plant"], rows, sel)
        assert E1 <= E0 * (1 + 64 * EPS), (trial, E1 - E0)
        worst = [max(worst[0], float(np.abs(p1 - p0).max())), max(worst[1], abs(L1 - L0)), max(worst[2], (E1 - E0) / E0)]
        checked += 1
    print("pairs %d: worst momentum drift %.3g, angular %.3g, relative energy change %.3g" % (checked, *worst))
    assert checked >= 300


@pytest.mark.parametrize("kind", ("general", "aligned"))
@pytest.mark.parametrize("n", K.SIZES)
def test_without_friction_and_yaw_it_is_the_interactions_word_for_word(n, kind):
    sc, ref = K.case(n, kind)
    o = CR.tick(sc["plant"], sc["rows"], sc["heat"], R.config(), CR.config(friction=0.0, yaw_response=0), t=5, nstep=sc["nstep"])
    for k in R.F64_NAMES + R.I32_NAMES + ("plant", "mu_live", "written", "part"):
        assert np.asarray(o[k]).tobytes() == np.asarray(ref[k]).tobytes(), k
    assert not np.nansum(np.abs(o["yaw_kick"])) and not np.nansum(o["friction_impulse"])


@pytest.mark.parametrize("kind", ("general", "aligned"))
@pytest.mark.parametrize("n", C.SIZES)
def test_crafted_scenes_hold_their_margins(n, kind):
    sc, ref = C.case(n, kind)                                              # asserts the margins and that no interval is empty
    for name, idx in sc["where"].items():
        assert ref["hit"][idx].all() and np.all(ref["partners"][idx] == (2 if name == "pile" else 1)), name
        assert np.all(ref["friction_impulse"][idx] > 0) and np.all(ref["yaw_kick"][idx] != 0), name
    assert ref["max_partners"].max() == 2


def test_a_centred_nose_to_tail_hit_spins_nobody_and_an_offset_one_spins_both():
    o = tick(np.array([car(0, 0, vx=1.4), car(0.75, 0.0, vx=0.8)]), rows_of(2))
    assert o["hit"].tolist() == [1, 1] and o["impulse"][0] > 0
    assert o["yaw_kick"].tolist() == [0.0, 0.0] and o["plant"][:, 7].tolist() == [0.0, 0.0] and o["friction_impulse"].tolist() == [0.0, 0.0]
    # the front car 0.1 to the left: the contact point is left of the rear car's centre and right of the front car's, the impulse on
    # the rear car points backwards (a left lever arm and a backward force turn it to the left, +), on the front car forwards
    # (a right lever arm and a forward force: + as well)
    o = tick(np.array([car(0, 0, vx=1.4), car(0.75, 0.1, vx=0.8)]), rows_of(2), ccfg=dict(friction=0.0))
    assert o["yaw_kick"][0] > 0 and o["yaw_kick"][1] > 0
    o = tick(np.array([car(0, 0, vx=1.4), car(0.75, -0.1, vx=0.8)]), rows_of(2), ccfg=dict(friction=0.0))
    assert o["yaw_kick"][0] < 0 and o["yaw_kick"][1] < 0


def test_a_t_bone_turns_the_struck_car_by_where_it_is_hit():
    fore = tick(*C.pair_scene("tbone_fore")[:2])
    aft = tick(*C.pair_scene("tbone_aft")[:2])
    # struck in its right side by a car going left: ahead of the centre it is turned to the left (+), behind it to the right (-)
    assert fore["yaw_kick"][0] > 0.5 and aft["yaw_kick"][0] < -0.5
    off = tick(*C.pair_scene("tbone_fore")[:2], ccfg=dict(yaw_response=0))
    assert off["yaw_kick"].tolist() == [0.0, 0.0] and np.array_equal(off["plant"][:, 7], C.pair_scene("tbone_fore")[0][:, 7])


def mirrored(plant):
    q = np.array(plant, float)
    q[:, [1, 3, 5, 6, 7]] *= -1.0
    return q


@pytest.mark.parametrize("kind", C.ORDER)
def test_mirror_rigid_motion_and_relabelling_symmetry(kind):
    plant, rows, heat = C.pair_scene(kind)
    o = tick(plant, rows)
    m = tick(mirrored(plant), rows)
    np.testing.assert_allclose(m["plant"], mirrored(o["plant"]), rtol=0, atol=1e-13)
    np.testing.assert_allclose(m["yaw_kick"], -o["yaw_kick"], rtol=0, atol=1e-12)
    th, sh = 1.1, np.array([3.0, -2.0])
    c, s = np.cos(th), np.sin(th)
    q = plant.copy()
    q[:, 0], q[:, 1] = c * plant[:, 0] - s * plant[:, 1] + sh[0], s * plant[:, 0] + c * plant[:, 1] + sh[1]
    q[:, 6] += th
    r = tick(q, rows)
    np.testing.assert_allclose(r["plant"][:, [2, 3, 7]], o["plant"][:, [2, 3, 7]], rtol=0, atol=1e-12)
    np.testing.assert_allclose(r["plant"][:, 0], c * o["plant"][:, 0] - s * o["plant"][:, 1] + sh[0], rtol=0, atol=1e-12)
    np.testing.assert_allclose(r["plant"][:, 1], s * o["plant"][:, 0] + c * o["plant"][:, 1] + sh[1], rtol=0, atol=1e-12)
    for k in ("impulse", "friction_impulse", "yaw_kick"):
        np.testing.assert_allclose(r[k], o[k], rtol=0, atol=1e-12)
    # relabelling.  Between parallel cars two axes tie and the lower index owns the axis, so P moves by the depth along n with the
    # labels: that changes the friction's lever arms and nothing else, and those kinds are relabelled without friction
    parallel = len({c[2] for c in C.KINDS[kind]}) == 1
    ccfg = dict(friction=0.0) if parallel else {}
    o, b = tick(plant, rows, ccfg=ccfg), tick(plant[::-1], rows[::-1], ccfg=ccfg)
    np.testing.assert_allclose(b["plant"][::-1], o["plant"], rtol=0, atol=1e-12)
    for k in ("impulse", "friction_impulse", "yaw_kick"):
        np.testing.assert_allclose(b[k][::-1], o[k], rtol=0, atol=1e-12)


def test_rubbing_loses_tangential_speed_only_with_friction():
    plant, rows, _ = C.pair_scene("rubbing")
    plant[:, 7] = 0.0
    before = abs(world_u(plant[1])[0] - world_u(plant[0])[0])              # the cars head along x and touch along y: x is the tangent
    rub = tick(plant, rows, ccfg=dict(yaw_response=0))
    slip = tick(plant, rows, ccfg=dict(friction=0.0, yaw_response=0))
    assert rub["friction_impulse"][0] > 0 and abs(world_u(rub["plant"][1])[0] - world_u(rub["plant"][0])[0]) < before - 1e-3
    assert slip["friction_impulse"].tolist() == [0.0, 0.0] and abs(world_u(slip["plant"][1])[0] - world_u(slip["plant"][0])[0]) == before


def test_a_member_with_a_psidot_that_is_not_finite_takes_no_part():
    plant = np.array([car(0, 0, vx=1.4), car(0.75, 0.05, vx=0.8, w=np.inf), car(0.1, 0.37, vx=1.0, vy=-0.1)])
    o = tick(plant, rows_of(3))
    assert o["part"].tolist() == [True, False, True] and o["hit"].tolist() == [1, 0, 1] and o["partners"].tolist() == [1, 0, 1]
    assert np.array_equal(o["plant"][1], plant[1])


def test_config_validators():
    from lpvmpc import _ffi, contact as Kc
    c = Kc.contact_config()
    assert {k: getattr(c, k) for k in Kc.DEFAULTS} == Kc.DEFAULTS == CR.DEFAULTS and c.reserved == 0
    c = Kc.contact_config(friction=0, yaw_response=False)
    assert (c.friction, c.yaw_response) == (0.0, 0)
    for bad in (dict(friction=-0.1), dict(friction=float("nan")), dict(friction=float("inf")), dict(yaw_response=2), dict(yaw_response=0.5),
                dict(yaw_response=-1), dict(reserved=0), dict(mu=0.3)):
        with pytest.raises(ValueError):
            Kc.contact_config(**bad)
    assert Kc.as_config(dict(friction=0.5)).friction == 0.5 and Kc.as_config(None).friction == 0.3 and Kc.as_config(c).yaw_response == 0
    k = Kc.new_contact_carry(5)
    assert k["f64"].shape == (_ffi.CONTACT_CARRY_F64, 5) and k["i32"].shape == (_ffi.CONTACT_CARRY_I32, 5) and k["i32"].dtype == np.int32
    assert not k["f64"].any() and not k["i32"].any()
    f = np.arange(3 * 4, dtype=float).reshape(3, 4); i = np.arange(2 * 4, dtype=np.int32).reshape(2, 4)
    d = Kc.contact_dict(f, i)
    assert np.array_equal(d["yaw_kick"], f[1]) and np.array_equal(d["max_partners"], i[1]) and d["f64"] is f and d["i32"] is i


def test_python_channel_constants_and_symbols_equal_the_headers():
    from lpvmpc import _ffi
    text = open(os.path.join(ROOT, "include", "lpvmpc.h")).read()
    H = {k: int(v) for k, v in re.findall(r"#define\s+LPVMPC_CONTACT_(\w+)\s+(\d+)", text)}
    assert (H["F64"], H["I32"], H["CARRY_F64"], H["CARRY_I32"]) == (_ffi.CONTACT_F64, _ffi.CONTACT_I32, _ffi.CONTACT_CARRY_F64, _ffi.CONTACT_CARRY_I32)
    for names, prefix in ((_ffi.CONTACT_F64_NAMES, ""), (_ffi.CONTACT_I32_NAMES, ""), (_ffi.CONTACT_CARRY_F64_NAMES, "CARRY_"),
                          (_ffi.CONTACT_CARRY_I32_NAMES, "CARRY_")):
        for c, k in enumerate(names):
            assert H[prefix + k.upper()] == c, (prefix, k)
    assert len(_ffi.CONTACT_F64_NAMES) == H["F64"] and len(_ffi.CONTACT_I32_NAMES) == H["I32"]
    assert len(_ffi.CONTACT_CARRY_F64_NAMES) == H["CARRY_F64"] and len(_ffi.CONTACT_CARRY_I32_NAMES) == H["CARRY_I32"]
    assert _ffi.CONTACT_F64_NAMES == CR.F64_NAMES and _ffi.CONTACT_I32_NAMES == CR.I32_NAMES
    body = re.search(r"typedef struct lpvmpc_contact_config \{(.*?)\} lpvmpc_contact_config;", text, re.S).group(1)
    fields = re.findall(r"^\s*(double|int32_t)\s+(\w+);", body, re.M)
    assert [(n, "double" if t is _ffi._d else "int32_t") for n, t in _ffi.ContactConfig._fields_] == [(n, t) for t, n in fields]
    # every function the header declares is an export and the other way round
    declared = set(re.findall(r"^[A-Za-z_][\w \*]*?\b(lpvmpc_\w+)\(", text, re.M))
    assert declared == set(_ffi.EXPORTS), (sorted(declared - set(_ffi.EXPORTS)), sorted(set(_ffi.EXPORTS) - declared))
    for name in ("lpvmpc_contact_default_config", "lpvmpc_race_contact", "lpvmpc_race_contact_read", "lpvmpc_contact_step_batch"):
        assert name in declared
