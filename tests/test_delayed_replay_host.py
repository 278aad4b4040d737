"""CPU: the host replay of the delayed fleets (tests/_delayed_race_ref.py).  With steering delay 0 and the actuator all off it is
the race replay without (RaceRef) and with the estimator (ObservedRaceRef) word for word: lap 0, the lap events, the racing ticks,
the finish.  With delays its plant runs through the reference's actuator FIFOs, and the controllers' histories step as the
reference's lists do, `tt` taking the command only from its event tick on."""
import numpy as np

NOISE = dict(stds=(0.01, 0.05, 0.01, 0.01, 0.02), seed=7)
KEYS = ("plant", "local", "cmd", "phase", "lap", "iters", "status", "half", "event_tick")


def _fleet():
    import lpvmpc
    from tests._race_observer_ref import start_line_fleet
    mp = lpvmpc.Map("L_shape", 0.2)
    return mp, start_line_fleet(mp.PointAndTangent, 4, 3, 0.93, 0.975)


def test_zero_delay_replay_is_the_race_replay():
    from tests._delayed_race_ref import DelayedRaceRef
    from tests._race_ref import RaceRef
    mp, plant0 = _fleet()
    kw = dict(half_track0=1, laps=1, half_width=mp.halfWidth, slack=mp.slack)
    a = RaceRef(mp.PointAndTangent, plant0, **kw)
    b = DelayedRaceRef(mp.PointAndTangent, plant0, **kw)
    for t in range(45):
        a.tick(); b.tick()
        for key in KEYS:
            assert np.array_equal(getattr(a, key), getattr(b, key), equal_nan=True), (t, key)
    assert np.all(b.phase >= 1) and len(set(b.event_tick.tolist())) >= 2


def test_zero_delay_replay_is_the_observed_race_replay():
    from tests._delayed_race_ref import DelayedRaceRef
    from tests._race_observer_ref import ObservedRaceRef, estimator_gains
    mp, plant0 = _fleet()
    kw = dict(half_track0=1, laps=1, half_width=mp.halfWidth, slack=mp.slack, **NOISE)
    g = estimator_gains()
    a = ObservedRaceRef(g, mp.PointAndTangent, plant0, **kw)
    b = DelayedRaceRef(mp.PointAndTangent, plant0, gains=g, **kw)
    for t in range(40):
        a.tick(); b.tick()
        for key in KEYS:
            assert np.array_equal(getattr(a, key), getattr(b, key), equal_nan=True), (t, key)
        assert np.array_equal(a.estimate(), b.estimate()), t
    assert np.all(b.phase >= 1)


def test_delayed_replay_histories_and_pins():
    """steeringDelay 3, La = 6 / Ld = 4 steps with the servo lag: the path history is the list recursion of the commands; on each
    vehicle's event tick tt's history is [0, .., 0, last servo] with OldAccelera = last motor; the replay's own solves honour the
    pins (uPred[i, steer] = OldSteering[i + 1], i < d) on solved ticks; the plant is the actuated one, not the direct one."""
    from tests import _actuator_ref as AR
    from tests._delayed_race_ref import DelayedRaceRef
    mp, plant0 = _fleet()
    d = 3
    r = DelayedRaceRef(mp.PointAndTangent, plant0, steering_delay=d, delay_a=6, delay_df=4, low_level_dyn=True, half_track0=1, laps=1,
                       half_width=mp.halfWidth, slack=mp.slack)
    hist = np.zeros((4, 2 + d))
    seen = 0
    for t in range(40):
        prev_cmd, prev_phase = r.cmd.copy(), r.phase.copy()
        r.tick()
        for b in range(4):
            if prev_phase[b] == 0 and r.phase[b] == 0:
                hist[b] = AR.uold_push(hist[b], prev_cmd[b, 0], prev_cmd[b, 1])
                assert np.array_equal(r.p_hist[b], hist[b]), (t, b)
                if r.status[b] == 1 and t >= 9:
                    assert np.max(np.abs(r.uPred_path[b][:d, 0] - r.p_hist[b][2:])) < 1e-6, (t, b)
            if prev_phase[b] == 0 and r.phase[b] == 1 and t >= 9:
                assert np.array_equal(r.t_hist[b], [0.0, prev_cmd[b, 1]] + [0.0] * (d - 1) + [prev_cmd[b, 0]]), (t, b)
                seen += 1
    assert seen >= 2 and all(a.k > 0 for a in r.act)
