"""CPU: the race with the estimator in the loop -- its C ABI and Python entry points, and its host replay
(tests/_race_observer_ref.py), whose schedule is pinned to the race's host replay without an estimator (tests/_race_ref.py)."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOISE = dict(stds=(0.01, 0.05, 0.01, 0.01, 0.02), seed=7)


def test_observed_race_is_declared_and_exported():
    import inspect

    import lpvmpc
    from lpvmpc import _ffi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lpvmpc.h")).read(), flags=re.S)
    assert re.search(r"int\s+lpvmpc_race_init_observed\s*\(", text)
    assert "lpvmpc_race_init_observed" in _ffi.EXPORTS and hasattr(_ffi.load(), "lpvmpc_race_init_observed")
    assert len(_ffi.load().lpvmpc_race_init_observed.argtypes) == 8
    assert inspect.signature(lpvmpc.BatchedSolver.race_init).parameters["estimator"].default is None
    assert inspect.signature(lpvmpc.RaceFleet).parameters["estimator"].default is None
    assert callable(lpvmpc.RaceFleet.estimate)


def _fleet():
    import lpvmpc
    from tests._race_observer_ref import start_line_fleet
    mp = lpvmpc.Map("L_shape", 0.2)
    return mp, start_line_fleet(mp.PointAndTangent, 4, 3, 0.93, 0.975)


def test_replay_measuring_the_plant_is_the_race_replay():
    """With the estimate replaced by the plant in every measurement, the replay is RaceRef word for word: lap 0, the lap events,
    the racing ticks, the finish.  The observer still runs alongside and is carried through the event."""
    from tests._race_observer_ref import ObservedRaceRef, estimator_gains
    from tests._race_ref import RaceRef
    mp, plant0 = _fleet()
    kw = dict(half_track0=1, laps=1, half_width=mp.halfWidth, slack=mp.slack)
    a = RaceRef(mp.PointAndTangent, plant0, **kw)
    b = ObservedRaceRef(estimator_gains(), mp.PointAndTangent, plant0, measure_plant=True, **NOISE, **kw)
    steps = np.zeros(4, int)
    for t in range(45):
        ph, k = b.phase.copy(), [c.k if c is not None else 0 for c in b.casc]
        a.tick(); b.tick()
        for key in ("plant", "local", "cmd", "phase", "lap", "iters", "status", "half", "event_tick"):
            assert np.array_equal(getattr(a, key), getattr(b, key), equal_nan=True), (t, key)
        for v in range(4):              # plant steps of this tick: none for a vehicle frozen or lost on entry
            if ph[v] == 0 and b.phase[v] != 3:
                steps[v] += b.n_sub_lap0
            elif ph[v] == 1 and b.phase[v] == 1:
                steps[v] += b.n_sub[k[v] % 3]
        # one estimator per vehicle for the whole race: its step counter counts every plant step since the start
        assert [v.k for v in b.veh] == steps.tolist(), t
    print("events", b.event_tick.tolist(), "phases", b.phase.tolist())
    assert np.all(b.phase >= 1) and len(set(b.event_tick.tolist())) >= 2 and np.all(b.event_tick >= 9)


def test_replay_measures_the_estimate():
    """Measuring the estimate changes the race: lap 0 and the racing ticks read it, and the lap events follow it."""
    from tests._race_observer_ref import ObservedRaceRef, estimator_gains
    mp, plant0 = _fleet()
    kw = dict(half_track0=1, laps=1, half_width=mp.halfWidth, slack=mp.slack)
    g = estimator_gains()
    a = ObservedRaceRef(g, mp.PointAndTangent, plant0, measure_plant=True, **NOISE, **kw)
    b = ObservedRaceRef(g, mp.PointAndTangent, plant0, **NOISE, **kw)
    for t in range(40):
        e0 = b.estimate().copy()
        a.tick(); b.tick()
        lap0 = (b.phase == 0)
        if t == 0:          # the first measurement is made from the start estimate [init_vx, 0, 0, x0, y0, yaw0]
            assert np.array_equal(b.local[:, :3], np.column_stack([np.full(4, 0.2), np.zeros(4), np.zeros(4)]))
        assert np.array_equal(b.local[lap0, 0], np.maximum(e0[lap0, 0], 0.01))
    assert not np.array_equal(a.plant, b.plant)
    assert np.all(b.phase == 1) and np.all(np.abs(b.estimate()[:, 3:5] - b.plant[:, :2]) < 0.05)
