"""GPU: a race's start zeroes the iteration, status and polish rows of its three handles (include/lpvmpc.h, lpvmpc_race_read: the
planner's report reads 0 before a vehicle's first planner tick).  The rows are carried state -- a masked launch leaves the rows of the
vehicles it does not run -- so without the zeroing a second race on the same handles, or one on a recycled allocation, starts with
another race's words in them."""
import numpy as np
import pytest

from tests import _race_observer_ref as RO

pytestmark = pytest.mark.gpu

ROWS = ("iters", "status", "polish")


def test_a_second_race_on_the_same_handles_starts_with_zero_rows():
    import lpvmpc
    from tests.test_gpu_race_record import engines
    mp = lpvmpc.Map("L_shape", 0.2)
    B = 8
    plant0 = RO.start_line_fleet(mp.PointAndTangent, B, 5, 0.95, 0.97)
    kw = dict(half_track0=1, laps=2, half_width=mp.halfWidth, slack=mp.slack)
    path, tt, plan = engines(mp)
    path.race_init(tt, plan, plant0, **kw)
    path.race_tick(60)
    o = path.race_read()
    snap = path.race_snapshot()
    print("first race: phases %s plan_iters %s" % (o["phase"].tolist(), o["plan_iters"].tolist()))
    assert np.any(o["plan_status"] != 0) and np.any(o["plan_iters"] > 0)             # the handles' rows now hold the first race's words
    for e in ("path", "tt", "plan"):
        assert np.any(snap.arrays["%s.iters" % e] != 0), e
    path.cl_release()
    path.race_init(tt, plan, plant0, **kw)
    o = path.race_read()
    assert o["ticks"] == 0 and np.all(o["plan_iters"] == 0) and np.all(o["plan_status"] == 0)
    assert np.all(o["iters"] == 0) and np.all(o["status"] == 0)
    snap = path.race_snapshot()
    for e in ("path", "tt", "plan"):
        for k in ROWS:
            assert np.all(snap.arrays["%s.%s" % (e, k)] == 0), (e, k)
    path.race_tick(5)                                                                 # lap 0: no vehicle has planned yet
    o = path.race_read()
    assert np.all(o["phase"] == 0) and np.all(o["plan_iters"] == 0) and np.all(o["plan_status"] == 0) and np.all(o["iters"] > 0)
    for e in (path, tt, plan):
        e.close()
