"""CPU: the tyre model (include/lpvmpc.h, "Tyre model").  lpvmpc.plant.pacejka reproduces the reference's own Simulator.pacejka (the
fixture's curve) and, inside the restated Simulator.f recursion, the fixture's trajectories; with kind 0 rows the restatement and the
fleet replay are the per-vehicle ones word for word.  The new translation unit instantiates only the tyre forms; the C ABI declares and
exports the new calls; the Python helpers build, sample and check rows."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "autonomous-racing-lpv-mpp-mpc_amd", "csrc")
GOLD = os.path.join(ROOT, "tests", "golden", "tyre", "tyre.npz")
NEW = ("lpvmpc_plant_step_tyres_batch", "lpvmpc_cl_init_tyres", "lpvmpc_race_init_tyres", "lpvmpc_tyre_params_read",
       "lpvmpc_tyre_force_batch")
FIVE = ("plant_kernel", "cl_command_plant_measure_kernel", "cl_command_plant_observe_kernel", "race_command_plant_kernel",
        "race_command_plant_observe_kernel")
KEYS = ("plant", "local", "cmd", "phase", "lap", "iters", "status", "half", "event_tick")


def test_pacejka_is_the_reference_curve():
    """1e-12: the project's bar for numpy restatements against reference fixtures."""
    from lpvmpc import plant
    g = np.load(GOLD)
    assert g["curve_force"].shape == (len(g["curve_sets"]), 257) and len(g["curve_sets"]) >= 4
    assert np.array_equal(g["curve_sets"][0], [1.98, 6.0, 1.6, 0.8])                   # the launch file's
    for (m, B, C, cf), f in zip(g["curve_sets"], g["curve_force"]):
        assert np.max(np.abs(plant.pacejka(g["curve_alpha"], m, (1.0, B, C, cf)) - f)) <= 1e-12
        assert np.max(np.abs([float(plant.pacejka(a, m, (1.0, B, C, cf))) for a in g["curve_alpha"][::16]] - f[::16])) <= 1e-12
    # the launch file's curve: stiffer than 60 N/rad at the origin, peak near 0.249 rad, falling beyond it
    a = np.linspace(0.0, 1.0, 100001)
    f = plant.pacejka(a, 1.98)
    assert abs(a[np.argmax(f)] - 0.249) < 1e-3 and f[-1] < 0.9 * f.max()
    assert abs(plant.pacejka(1e-6, 1.98) / 1e-6 - 0.8 * 1.98 * 9.81 / 2 * 1.6 * 6.0) < 1e-6 and plant.pacejka(1e-6, 1.98) / 1e-6 > 60


def test_restatement_reproduces_the_fixture_trajectories():
    from tests import _tyre_ref as T
    g = np.load(GOLD)
    assert g["state"].shape == (8, 300, 8)
    beyond = 0
    for c in range(8):
        st, ap, slip = T.simulate(g["plant0"], g["cmd"][c], g["params"][c], T.pacejka_forces(g["tyre"][c]), int(g["La"][c]), int(g["Ld"][c]),
                                  bool(g["lld"][c]), float(g["dt"]))
        assert np.max(np.abs(ap - g["applied"][c])) <= 1e-12, c
        assert np.max(np.abs(st - g["state"][c])) <= 1e-12, c
        assert np.max(np.abs(slip - g["slip"][c])) <= 1e-12, c
        lin = T.simulate(g["plant0"], g["cmd"][c], g["params"][c], T.linear_forces, int(g["La"][c]), int(g["Ld"][c]), bool(g["lld"][c]))[0]
        if g["tyre"][c, 0]:
            assert np.max(np.abs(lin[:, 7] - g["state"][c][:, 7])) > 1e-3, c           # a restatement that ignored the tyre row fails
            beyond += np.max(np.abs(g["slip"][c])) > 0.3
        else:
            assert np.array_equal(lin, st)
    assert beyond >= 2 and np.sum(g["tyre"][:, 0] == 0) == 1
    assert np.sum((g["La"] > 0) | (g["Ld"] > 0) | (g["lld"] > 0)) >= 2


def test_kind0_step_is_the_per_vehicle_step_word_for_word():
    from tests import _plant_params_ref as P
    from tests import _tyre_ref as T
    rng = np.random.default_rng(5)
    for _ in range(300):
        st = rng.normal(0, 1, 8); st[2] = rng.choice([0.1, rng.uniform(-3, 3)])
        u = rng.normal(0, 0.5, 2)
        row = P.nominal_row() * rng.uniform(0.7, 1.3, 7)
        assert np.array_equal(T.simulator_f_forces(st, u, row, T.pacejka_forces([0.0, 6.0, 1.6, 0.8])), P.simulator_f_row(st, u, row))
        assert not np.array_equal(T.simulator_f_forces(st, u, row, T.pacejka_forces(T.LAUNCH_FILE)), P.simulator_f_row(st, u, row)) or abs(st[2]) <= 0.2


@pytest.mark.parametrize("observed", [False, True])
def test_kind0_replay_is_the_per_vehicle_replay(observed):
    import lpvmpc
    from tests._plant_params_ref import VehicleRaceRef
    from tests._race_observer_ref import estimator_gains, start_line_fleet
    from tests._tyre_ref import TyreRaceRef
    mp = lpvmpc.Map("L_shape", 0.2)
    plant0 = start_line_fleet(mp.PointAndTangent, 4, 3, 0.93, 0.975)
    rows = lpvmpc.sample_plant_params(4, 6)
    kw = dict(half_track0=1, laps=1, half_width=mp.halfWidth, slack=mp.slack, steering_delay=2, delay_a=3, delay_df=5, low_level_dyn=True,
              plant_params=rows)
    if observed:
        kw.update(gains=estimator_gains(), stds=(0.01, 0.05, 0.01, 0.01, 0.02), seed=7)
    a = VehicleRaceRef(mp.PointAndTangent, plant0, **kw)
    b = TyreRaceRef(mp.PointAndTangent, plant0, **kw)
    c = TyreRaceRef(mp.PointAndTangent, plant0, tyre_params=lpvmpc.tyre_params(4, kind=[0, 1, 0, 0]), **kw)
    for t in range(36):
        a.tick(); b.tick(); c.tick()
        for key in KEYS:
            assert np.array_equal(getattr(a, key), getattr(b, key), equal_nan=True), (t, key)
        if observed:
            assert np.array_equal(a.estimate(), b.estimate()), t
    # a tyre row reaches the plant of its vehicle only
    assert np.array_equal(c.plant[[0, 2, 3]], a.plant[[0, 2, 3]], equal_nan=True) and not np.array_equal(c.plant[1], a.plant[1])


def _source(fname):
    s = open(os.path.join(CSRC, fname)).read()
    return re.sub(r"//.*", "", re.sub(r"/\*.*?\*/", "", s, flags=re.S))


def test_new_unit_instantiates_the_tyre_forms_only():
    from tests.test_fleet_kernel_instances import KERNELS
    s = _source("tyre.hip")
    inst = set(re.findall(r"\b(%s)\s*<\s*([^<>]*?)\s*>" % "|".join(KERNELS + ("tyre_force_kernel",)), s))
    assert inst == {(k, "true, true, true") for k in FIVE} | {("tyre_force_kernel", "true")}
    assert "__global__" not in s
    # the other units keep their forms
    for f, forms in (("closed_loop.hip", {"false"}), ("observer.hip", {"false"}), ("race.hip", {"false"}), ("actuator.hip", {"true"}),
                     ("plant_params.hip", {"true, true"})):
        assert {a for _, a in re.findall(r"\b(%s)\s*<\s*([^<>]*?)\s*>" % "|".join(KERNELS), _source(f))} == forms, f
    mk = open(os.path.join(CSRC, "Makefile")).read()
    rule = [ln for ln in mk.split("\n") if ln.startswith("\tmkdir") and "../$<" in ln and "tyre-hip" in ln]
    assert "tyre.o" in mk and len(rule) == 1 and "-ffp-contract=off" in rule[0] and "$(RESCHK) tyre-hip" in rule[0]


def test_new_calls_are_declared_and_exported():
    from lpvmpc import _ffi
    h = open(os.path.join(ROOT, "include", "lpvmpc.h")).read()
    assert "Tyre model" in h
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, h), name
        assert name in _ffi.EXPORTS, name
    assert re.search(r"#define\s+LPVMPC_TYRE_WORDS\s+4\b", h) and _ffi.TYRE_WORDS == 4
    if os.path.exists(_ffi.LIB_PATH):
        lib = _ffi.load()
        assert all(hasattr(lib, n) for n in NEW)


def test_helpers_build_rows_and_sample_them():
    import lpvmpc
    from lpvmpc import plant
    assert np.array_equal(lpvmpc.tyre_params(2), [[1.0, 6.0, 1.6, 0.8]] * 2)
    r = lpvmpc.tyre_params(3, kind=[0, 1, 1], B_=5.0, c_f=[0.5, 0.6, 0.7])
    assert np.array_equal(r, [[0, 5.0, 1.6, 0.5], [1, 5.0, 1.6, 0.6], [1, 5.0, 1.6, 0.7]])
    with pytest.raises(ValueError):
        lpvmpc.tyre_params(3, C=[1.0, 2.0])
    a = lpvmpc.sample_tyre_params(64, 11)
    assert np.array_equal(a, lpvmpc.sample_tyre_params(64, 11)) and not np.array_equal(a, lpvmpc.sample_tyre_params(64, 12))
    assert np.array_equal(a[40:], lpvmpc.sample_tyre_params(24, 11, offset=40))
    f = a / np.array(plant.PACEJKA)
    assert np.all(a[:, 0] == 1)
    for i, s in ((1, 0.20), (2, 0.10), (3, 0.25)):
        assert np.all(np.abs(f[:, i] - 1) <= s + 1e-12) and np.std(f[:, i]) > s / 4, i
    b = lpvmpc.sample_tyre_params(8, 11, spread=dict(c_f=0.1), kind=0)
    assert np.array_equal(b[:, :3], lpvmpc.tyre_params(8, kind=0)[:, :3]) and np.all(b[:, 3] != 0.8)
    with pytest.raises(ValueError):
        lpvmpc.sample_tyre_params(8, 1, spread=dict(B=1.5))
    with pytest.raises(TypeError):
        lpvmpc.sample_tyre_params(8, 1, spread=dict(kind=0.5))


def test_rows_with_bad_shapes_or_values_are_refused_before_the_library():
    from lpvmpc import plant
    from lpvmpc.api import _tyre_rows
    good = plant.tyre_params(4)
    for a in (good[:3], good[:, :3], good.reshape(-1), np.zeros((4, 4, 1))):
        with pytest.raises(ValueError):
            plant.check_tyre_params(a, 4)
    for (b, i, v) in ((0, 0, 2.0), (1, 0, 0.5), (2, 0, -1.0), (3, 0, np.nan), (0, 1, np.nan), (1, 2, np.inf), (2, 3, -0.1), (3, 1, -1e-9)):
        x = good.copy(); x[b, i] = v
        with pytest.raises(ValueError):
            plant.check_tyre_params(x, 4)
    x = good.copy(); x[:, 1:] = 0.0
    assert np.array_equal(plant.check_tyre_params(x, 4), x)                          # B = C = c_f = 0 are allowed
    assert np.array_equal(_tyre_rows("pacejka", 3), plant.tyre_params(3))
    with pytest.raises(ValueError):
        _tyre_rows("magic", 3)
    with pytest.raises(ValueError):
        plant.check_tyre_params(np.array([["a"] * 4] * 4), 4)
