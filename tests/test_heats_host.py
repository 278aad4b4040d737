"""CPU: the heats' reference (tests/_heats_ref.py) against its own definitions, the conditions on the GPU tests' inputs
(tests/_heats_cases.py), and the Python-side refusals and the standings table, which need no device."""
import numpy as np
import pytest

from tests import _heats_cases as HC
from tests import _heats_ref as R


def run_crafted(c):
    ref = R.HeatsRef(c["heat"], c["L"], c["turns0"], c["phase0"], c["hl"], c["hw"])
    return ref.step(0, c["pose"], c["s"], c["inside"], c["phase"])


def test_positions_are_a_permutation_with_ties():
    rng = np.random.default_rng(3)
    for trial in range(20):
        B = 60
        heat = rng.integers(-1, 4, B)
        s = rng.integers(0, 4, B).astype(float)                             # many equal progresses
        inside = (rng.uniform(size=B) > 0.2).astype(int)
        phase = rng.integers(0, 4, B)
        ref = R.HeatsRef(heat, 10.0, phase0=rng.integers(0, 3, B))
        for t in range(3):
            o = ref.step(t, rng.uniform(-1, 1, (B, 3)), s, inside, phase)
            for g in range(4):
                m = heat == g
                assert sorted(o["position"][m].tolist()) == list(range(int(m.sum()))), (trial, t, g)
                lead = o["position"][m] == 0
                assert np.all(o["ahead"][m][lead] == -1) and np.all(o["ahead"][m][~lead] >= 0)
            assert np.all(o["position"][heat < 0] == -1)


def test_sep_sign_agrees_with_polygon_intersection():
    rng = np.random.default_rng(17)
    checked = overlapping = 0
    for _ in range(2000):
        a = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-np.pi, np.pi)])
        b = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-np.pi, np.pi)])
        sep, band = R.sep_pair(a, b, HC.HL, HC.HW)
        if abs(sep) <= band:
            continue
        hit = R.polygons_intersect(R.corners(a, HC.HL, HC.HW), R.corners(b, HC.HL, HC.HW))
        assert hit == bool(sep < 0), (a, b, float(sep))
        checked += 1; overlapping += hit
    assert checked > 1900 and 200 < overlapping < checked - 200, (checked, overlapping)


def test_wrap_backward_wrap_and_hold():
    L = 10.0
    ref = R.HeatsRef([0, 0, 0], L, turns0=[0, 0, -1])
    pose = np.zeros((3, 3)); pose[:, 1] = [0, 5, 10]
    ph = np.ones(3, int)
    o = ref.step(0, pose, [9.5, 0.25, 9.0], [1, 1, 1], ph)
    assert o["turns"].tolist() == [0, 0, -1] and o["progress"].tolist() == [9.5, 0.25, -1.0]
    o = ref.step(1, pose, [0.5, 9.75, 10000.0], [1, 1, 0], ph)              # forward wrap, backward wrap, hold
    assert o["turns"].tolist() == [1, -1, -1] and o["progress"].tolist() == [10.5, -0.25, -1.0]
    o = ref.step(2, pose, [0.75, 9.5, 0.5], [1, 1, 1], ph)                   # the held car comes back beyond the line
    assert o["turns"].tolist() == [1, -1, 0] and o["progress"].tolist() == [10.75, -0.5, 0.5]
    never = R.HeatsRef([0], L)
    o = never.step(0, np.zeros((1, 3)), [10000.0], [0], [1])
    assert np.isnan(o["progress"][0]) and o["class"][0] == 2


def test_crafted_inputs_are_outside_the_band_except_the_touching_pairs():
    for c in (HC.crafted(), HC.crafted_256()):
        o = run_crafted(c)
        touching = sorted(b for pair in c["touching"] for b in pair)
        assert sorted(np.nonzero(o["ambiguous"])[0].tolist()) == touching, (np.nonzero(o["ambiguous"])[0], touching)
        for a, b in c["touching"]:
            assert o["nearest"][a] == b and o["nearest"][b] == a and abs(o["clearance"][a]) <= o["band"][a]
        assert o["contact"].sum() >= 4 and set(np.unique(o["class"][c["heat"] >= 0])) == {0, 1, 2, 3}
    c = HC.crafted()
    o = run_crafted(c)
    n = c["named"]
    assert abs(o["clearance"][n["side_by_side"][0]] - 0.13) < 1e-12 and abs(o["clearance"][n["nose_to_tail"][1]] - 0.05) < 1e-12
    assert abs(o["clearance"][n["t_bone"][0]] + 0.03) < 1e-12 and o["nearest"][n["identical"][2]] == n["identical"][0]
    assert np.isinf(o["clearance"][n["nan_pose"][0]]) and o["nearest"][n["nan_pose"][0]] == -1
    assert o["clearance"][n["far"][0]] > 100 and 0 < o["clearance"][n["corners_45"][0]] < 0.3
    sizes = np.bincount(c["heat"][c["heat"] >= 0]).tolist()
    assert sizes == [1, 5, 65] and np.sum(c["heat"] < 0) == 9


@pytest.mark.parametrize("name", list(HC.SEQUENCES))
def test_every_sequence_has_its_events(name):
    static, ticks = HC.sequence(HC.SEQUENCES[name])
    ref = R.HeatsRef(static["heat"], static["L"], static["turns0"], None, HC.SEQ_HL, HC.SEQ_HW, lines=3)
    outs = [ref.step(t, k["pose"], k["s"], k["inside"], k["phase"]) for t, k in enumerate(ticks)]
    passes = np.array([o["passes"] for o in outs]); turns = np.array([o["turns"] for o in outs])
    assert passes[5][1] == 1 and passes[4][1] == 0 and passes[9][0] == 1 and passes[8][0] == 0          # the overtake and the re-pass
    assert outs[9]["passed"][1] == 2 or outs[9]["passed"][1] == 1
    assert turns[8][0] == 1 and turns[7][0] == 0 and turns[3][2] == -1 and turns[2][2] == 0             # a wrap, a backward wrap
    assert outs[-1]["line_tick"][0, 0] == 8 and outs[-1]["line_tick"][1, 0] == 7 and outs[-1]["line_tick"][7, 0] == 8
    assert outs[-1]["line_pos"][1, 0] == outs[7]["position"][1]
    held = [o["progress"][4] for o in outs[2:6]]
    assert len(set(held)) == 1 and ticks[4]["inside"][4] == 0 and outs[4]["class"][4] == 1               # a hold
    assert passes[4][5] == 1 and passes[6][4] == 1
    assert outs[9]["class"][5] == 0 and outs[8]["class"][5] == 1 and outs[11]["class"][1] == 0           # two finishers
    assert outs[11]["position"][5] == 0 and outs[11]["position"][1] == 1
    assert outs[10]["class"][7] == 3 and outs[9]["class"][7] == 1                                        # a loss
    assert outs[0]["class"][3] == 2 and outs[2]["class"][3] == 1
    assert max(o["contact"].sum() for o in outs) >= 2 and outs[-1]["contact_ticks"][0] > 0
    if name == "unit":                                                                                   # exactly touching is no contact
        assert outs[0]["clearance"][0] == 0.0 and outs[0]["contact"][0] == 0


def test_python_refusals_need_no_device():
    from lpvmpc import heats as H
    assert H.check_heats([0, -1, 5, 5], 4).dtype == np.int32
    with pytest.raises(ValueError):
        H.check_heats([0, 1], 3)
    with pytest.raises(ValueError):
        H.check_heats([0, -2, 1], 3)
    with pytest.raises(ValueError):
        H.check_heats([0.5, 1, 1], 3)
    with pytest.raises(ValueError):
        H.check_heats(np.zeros(257, int), 257)
    assert H.check_heats(np.zeros(256, int), 256).shape == (256,)
    with pytest.raises(ValueError):
        H.check_heats([0, 0, 1], 3, track_of=[0, 1, 1])
    assert H.check_heats([0, 0, 1], 3, track_of=[1, 1, 0]).tolist() == [0, 0, 1]
    for bad in ((0.0, 0.2), (0.4, -1.0), (np.nan, 0.2), (np.inf, 0.2)):
        with pytest.raises(ValueError):
            H.check_extents(*bad)
    c = H.new_carry(3, turns0=[0, -1, 2], lines=2)
    assert c["i32"].shape == (10, 3) and c["i32"][1].tolist() == [0, -1, 2] and c["i32"][0].tolist() == [0, 0, 0]
    assert c["line_tick"].tolist() == [[-1, -1]] * 3 and c["f64"].shape == (3, 3)


def test_standings_table():
    from lpvmpc import telemetry
    c = HC.crafted()
    o = run_crafted(c)
    tab = telemetry.standings_table(o, c["heat"])
    assert sorted(tab) == [0, 1, 2]
    for g, row in tab.items():
        assert row["position"].tolist() == list(range(len(row["vehicle"]))) and np.all(c["heat"][row["vehicle"]] == g)
        assert np.all(np.diff(row["cls"]) >= 0)                                  # finishers first, lost last
        run = row["cls"] == 1
        assert np.all(np.diff(row["progress"][run]) <= 0)
        gl = row["gap_leader"][run]
        if row["cls"][0] == 1:
            assert np.isnan(gl[0]) and np.all(np.diff(gl[1:]) >= 0)
    bad = dict(o); bad["position"] = o["position"].copy(); bad["position"][c["heat"] == 1] = 0
    with pytest.raises(ValueError):
        telemetry.standings_table(bad, c["heat"])
