"""GPU: the race engine (lpvmpc_race_*) -- lap 0, per-vehicle lap events and racing for one fleet -- against the reference
trace (tests/golden/cascade.npz), against the two existing engines it composes (lpvmpc_cl_*, lpvmpc_cascade_*), against the
host replay (tests/_race_ref.py), and the active-instance mask of the solve kernel (lpvmpc_solve_batch_masked)."""
import numpy as np
import pytest

from tests._golden import load

pytestmark = pytest.mark.gpu

KV = 0          # kernel_variant fixed on every handle: kernel routes may depend on B


def engines(mp, kv=KV):
    import lpvmpc
    from lpvmpc import workloads as W
    Qp, Rp, dRp = W.CTRL_TUNINGS["path"]; Qr, Rr, dRr = W.CTRL_TUNINGS["race"]
    path = lpvmpc.BatchedSolver("controller", 20, 1 / 30.0, Qp, Rp, dRp, track=mp.PointAndTangent)
    tt = lpvmpc.BatchedSolver("controller", 20, 1 / 30.0, Qr, Rr, dRr, track=mp.PointAndTangent)
    plan = lpvmpc.BatchedSolver("planner", 40, 0.05, W.PLAN_Q, W.PLAN_R, W.PLAN_dR, L_cf=W.PLAN_L, track=mp.PointAndTangent)
    for e in (path, tt, plan):
        e.set_option("kernel_variant", kv)
    plan.handoff_setup()
    return path, tt, plan


def lshape():
    import lpvmpc
    return lpvmpc.Map("L_shape", 0.2)


def start_line_fleet(mp, B, seed, s_lo=0.8, s_hi=0.97):
    """B vehicles on the last quarter of the lap (HalfTrack = 1), so that their lap events are spread over many ticks."""
    rng = np.random.default_rng(seed)
    L = mp.TrackLength
    plant0 = np.zeros((B, 8))
    from oracle import plant_ref as PR
    for b in range(B):
        s = rng.uniform(s_lo, s_hi) * L
        ey = rng.normal(0, 0.02)
        x, y, th = PR.get_global_position(mp.PointAndTangent, s, ey)
        plant0[b] = [x, y, rng.uniform(0.9, 1.1), 0.0, 0.0, 0.0, th + rng.normal(0, 0.02), 0.0]
    return plant0


def test_race_reproduces_the_reference_trace():
    """One vehicle from cascade.npz's pre_plant[0] with HalfTrack = 1: the 17 lap-0 ticks with the lap event, then 60 racing
    ticks, to the bars of test_gpu_dropin.py (lap 0) and of test_cascade_matches_reference_trace (racing)."""
    c = load("cascade")
    mp = lshape()
    path, tt, plan = engines(mp)
    path.race_init(tt, plan, c["pre_plant"][0][None], half_track0=1, laps=5, half_width=mp.halfWidth, slack=mp.slack)
    P = int(c["pre_ticks"])
    for t in range(P):
        assert np.max(np.abs(path.race_read()["plant"][0] - c["pre_plant"][t])) <= 2e-6, t
        path.race_tick(1)
        o = path.race_read()
        assert np.max(np.abs(o["local"][0] - c["pre_local"][t])) <= 2e-6, t
        assert np.max(np.abs(o["cmd"][0] - c["pre_cmd"][t])) <= 2e-5, t
        assert o["lap"][0] == c["pre_lap"][t] and o["phase"][0] == (1 if c["pre_lap"][t] else 0), t
    strict = dict(plant=0.0, local=0.0, cmd=0.0); loose = dict(strict)
    split = None
    for k in range(60):
        before = path.race_read()
        path.race_tick(1)
        o = path.race_read()
        j = int(c["ctrl_plan_ticks"][k]) - 1
        assert o["status"][0] == c["ctrl_status"][k] and o["plan_status"][0] == c["plan_status"][j], k
        assert o["lap"][0] == c["ctrl_lap"][k]
        if split is None and o["plan_iters"][0] != c["plan_iters"][j]:
            split = (k, j)
        if split is None:
            assert o["iters"][0] == c["ctrl_iters"][k], k
        w = strict if split is None else loose
        w["plant"] = max(w["plant"], float(np.max(np.abs(before["plant"][0] - c["ctrl_plant"][k]))))
        w["local"] = max(w["local"], float(np.max(np.abs(o["local"][0] - c["ctrl_local"][k]))))
        w["cmd"] = max(w["cmd"], float(np.max(np.abs(o["cmd"][0] - c["ctrl_cmd"][k]))))
    print("race trace: strict until", split, strict, "after:", loose)
    assert split is None or (split[0] >= 51 and split[1] >= 34), split
    assert strict["plant"] <= 1e-5 and strict["local"] <= 1e-5 and strict["cmd"] <= 1e-4
    assert max(loose.values()) <= 2e-2
    ls, alive = path.race_laps()
    assert ls[0, 0] == 0 and ls[0, 1] == 7 * (P - 1) and alive[0] == P + 60        # lap 1 starts with the event tick's plant steps
    for e in (path, tt, plan):
        e.close()


def test_lap0_fleet_equals_the_closed_loop_engine_bit_for_bit():
    """Before any lap event the race is lpvmpc_cl_tick on the same vehicles, word for word."""
    import lpvmpc
    from lpvmpc import workloads as W
    mp = lshape()
    B = 24
    rng = np.random.default_rng(4)
    plant0 = np.zeros((B, 8)); plant0[:, 1] = rng.normal(0, 0.03, B); plant0[:, 2] = rng.uniform(0.8, 1.2, B); plant0[:, 6] = rng.normal(0, 0.03, B)
    path, tt, plan = engines(mp)
    path.race_init(tt, plan, plant0, laps=1, half_width=mp.halfWidth, slack=mp.slack)
    Qp, Rp, dRp = W.CTRL_TUNINGS["path"]
    cl = lpvmpc.BatchedSolver("controller", 20, 1 / 30.0, Qp, Rp, dRp, track=mp.PointAndTangent)
    cl.set_option("kernel_variant", KV)
    cl.cl_init(plant0, mp.halfWidth, mp.slack, q9_swap=True, n_sub=7)
    for t in range(40):
        path.race_tick(1); cl.cl_tick(1)
        a, b = path.race_read(), cl.cl_read()
        assert np.all(a["phase"] == 0)
        for k in ("plant", "local", "cmd", "iters", "status"):
            assert np.array_equal(a[k], b[k]), (t, k)
    for e in (path, tt, plan, cl):
        e.close()


def test_racing_ticks_equal_single_vehicle_cascades_bit_for_bit():
    """8 vehicles whose events fire on different ticks: from its event on, every racing tick of a vehicle equals a B = 1
    lpvmpc_cascade_* (prefetch 0) started from that vehicle's post-event state read from the race."""
    import lpvmpc
    from lpvmpc import workloads as W
    mp = lshape()
    B, T = 8, 70
    plant0 = start_line_fleet(mp, B, 21, 0.88, 0.99)
    path, tt, plan = engines(mp)
    path.race_init(tt, plan, plant0, half_track0=1, laps=3, half_width=mp.halfWidth, slack=mp.slack)
    Qr, Rr, dRr = W.CTRL_TUNINGS["race"]
    cas, events = {}, {}
    prev = path.race_read()
    compared = 0
    for t in range(T):
        path.race_tick(1)
        o = path.race_read()
        for b, (c, q) in cas.items():
            if o["phase"][b] != 1:
                continue
            c.cascade_tick(1)
            r = c.cascade_read(full=False)
            for k in ("plant", "local", "cmd", "iters", "status", "lap", "plan_iters", "plan_status"):
                assert np.array_equal(o[k][b], r[k][0]), (t, b, k)
            compared += 1
        for b in np.nonzero((prev["phase"] == 0) & (o["phase"] == 1))[0]:
            b = int(b); events[b] = t
            if t < 9:
                continue
            _pu, tu = path.race_predictions()
            c = lpvmpc.BatchedSolver("controller", 20, 1 / 30.0, Qr, Rr, dRr, track=mp.PointAndTangent)
            q = lpvmpc.BatchedSolver("planner", 40, 0.05, W.PLAN_Q, W.PLAN_R, W.PLAN_dR, L_cf=W.PLAN_L, track=mp.PointAndTangent)
            for e in (c, q):
                e.set_option("kernel_variant", KV)
            c.set_option("cascade_prefetch", 0)
            q.handoff_setup()
            c.cascade_init(q, o["plant"][b][None], o["cmd"][b][None], tu[b][None], lap0=1, half_width=mp.halfWidth, slack=mp.slack,
                           plan_max_ey=0.2, q9_swap=True)
            cas[b] = (c, q)
        prev = o
    print("events:", events, "racing vehicle-ticks compared:", compared)
    assert len(set(events.values())) >= 4 and len(cas) >= 6 and compared >= 150
    for c, q in cas.values():
        c.close(); q.close()
    for e in (path, tt, plan):
        e.close()


def test_mixed_fleet_matches_the_host_replay():
    """Vehicles spread over the last quarter of the lap, so that their events are spread over tens of ticks: every vehicle's
    event tick equals the host replay's, and so does its phase sequence for as long as the two trajectories agree to the loose
    bar of the cascade trace.  Beyond that the planner's open-loop recursion has amplified eps-level differences of its QPs
    (configs[4] is a survival experiment): which tick a vehicle is lost on is then chaotic on both sides."""
    from tests._race_ref import RaceRef
    mp = lshape()
    B, T = 48, 120
    plant0 = start_line_fleet(mp, B, 7)
    path, tt, plan = engines(mp)
    path.race_init(tt, plan, plant0, half_track0=1, laps=3, half_width=mp.halfWidth, slack=mp.slack)
    ref = RaceRef(mp.PointAndTangent, plant0, half_track0=1, laps=3, half_width=mp.halfWidth, slack=mp.slack)
    dev_phase, ref_phase = [], []
    worst = np.zeros(B); it_diff = 0; st_diff = 0
    apart = np.zeros(B, bool)                  # the two trajectories of a vehicle have parted beyond the loose bar
    for t in range(T):
        path.race_tick(1); ref.tick()
        o = path.race_read()
        alive = (o["phase"] <= 1) & (ref.phase <= 1)
        d = np.max(np.abs(o["plant"] - ref.plant), axis=1)
        both_lost = (o["phase"] == 3) & (ref.phase == 3)
        apart |= ~both_lost & ~(d <= 2e-2)
        assert np.array_equal(o["phase"][~apart], ref.phase[~apart]), t
        dev_phase.append(o["phase"].copy()); ref_phase.append(ref.phase.copy())
        worst[alive] = np.maximum(worst[alive], d[alive])
        it_diff += int(np.sum(o["iters"][alive] != ref.iters[alive])); st_diff += int(np.sum(o["status"][alive] != ref.status[alive]))
    dev_phase, ref_phase = np.array(dev_phase), np.array(ref_phase)
    ev_dev = [int(np.argmax(dev_phase[:, b] >= 1)) if np.any(dev_phase[:, b] >= 1) else -1 for b in range(B)]
    ev_ref = [int(ref.event_tick[b]) for b in range(B)]
    # classes: A round-off (the strict bar of the cascade trace), B the eps-level divergence of the planner's open-loop
    # recursion (the loose bar), C beyond
    cls = ["A" if w <= 1e-5 else "B" if w <= 2e-2 else "C" for w in worst]
    cls = [c if not a else "C" for c, a in zip(cls, apart)]
    print("mixed fleet: events", sorted(ev_dev), "classes", {c: cls.count(c) for c in set(cls)}, "iteration / status differences",
          it_diff, st_diff, "worst plant difference", float(worst.max()))
    assert ev_dev == ev_ref
    assert len(set(ev_dev)) >= 10
    assert np.sum(~apart) >= B // 4, int(np.sum(~apart))
    for e in (path, tt, plan):
        e.close()


def test_from_the_grid_to_the_finish():
    """32 vehicles near the origin, HalfTrack = 0, one racing lap, 900 ticks: lap 0 at 1 m/s is about 580 ticks."""
    mp = lshape()
    B, T = 32, 900
    rng = np.random.default_rng(12)
    plant0 = np.zeros((B, 8)); plant0[:, 1] = rng.normal(0, 0.02, B); plant0[:, 2] = rng.uniform(0.9, 1.1, B)
    path, tt, plan = engines(mp)
    path.race_init(tt, plan, plant0, laps=1, half_width=mp.halfWidth, slack=mp.slack)
    prev = path.race_read()
    frozen = {}
    for t in range(T):
        path.race_tick(1)
        o = path.race_read()
        assert np.all(o["phase"] >= prev["phase"]), t                        # phases never go backwards
        for b in np.nonzero(o["phase"] >= 2)[0]:
            b = int(b)
            assert o["iters"][b] == 0
            if b in frozen:
                assert np.array_equal(o["plant"][b], frozen[b][0], equal_nan=True) and np.array_equal(o["cmd"][b], frozen[b][1], equal_nan=True)
            else:
                frozen[b] = (o["plant"][b].copy(), o["cmd"][b].copy())
        prev = o
    ls, alive = path.race_laps()
    ph = prev["phase"]
    print("grid: phases", np.bincount(ph, minlength=4).tolist(), "lap-0 events (steps)", sorted(ls[:, 1].tolist()))
    assert np.sum(ph >= 1) >= B // 2
    for b in range(B):
        reached = ls[b][ls[b] >= 0]
        assert np.all(np.diff(reached) > 0) and ls[b, 0] == 0
        assert np.all(ls[b][len(reached):] == -1)
        if ph[b] == 2:
            assert ls[b, 2] > ls[b, 1] > 0
    lt = (ls[:, 1:] - ls[:, :-1]) * 0.005
    assert np.all(lt[ls[:, 1] > 0, 0] > 15.0)                                # lap 0 at ~1 m/s on a 19.2 m track
    assert np.all(alive <= T) and np.all(alive[ph == 0] == T)
    for e in (path, tt, plan):
        e.close()


def test_masked_solve():
    """Active rows equal the unmasked solve bit for bit, inactive rows are untouched byte for byte, an all-zero mask does nothing."""
    from lpvmpc import workloads
    B = 256
    w = workloads.controller_batch(B, N=20, seed=5)
    eng = workloads.make_solver(w)
    eng.set_option("kernel_variant", KV)
    args = (w["x0"], w["u_prev"], w["vel_ref"], w["curv_s"], w["u_old"], None, w["cf_new"], w["lap"])
    full = eng.solve(*args)
    rng = np.random.default_rng(1)
    act = (rng.random(B) < 0.4).astype(np.int32)
    sentinel = {k: np.full_like(v, 7) for k, v in full.items()}
    out = {k: v.copy() for k, v in sentinel.items()}
    eng.solve_batch_masked(act, *args[:5], cf_new=w["cf_new"], lap=w["lap"], out=out)
    on = act != 0
    for k in full:
        assert np.array_equal(out[k][on], full[k][on]), k
        assert out[k][~on].tobytes() == sentinel[k][~on].tobytes(), k
    out2 = {k: v.copy() for k, v in sentinel.items()}
    eng.solve_batch_masked(np.zeros(B, np.int32), *args[:5], cf_new=w["cf_new"], lap=w["lap"], out=out2)
    for k in full:
        assert out2[k].tobytes() == sentinel[k].tobytes(), k
    eng.close()


def test_race_refusals():
    import lpvmpc
    from lpvmpc import workloads as W
    mp = lshape()
    p0 = np.zeros((2, 8)); p0[:, 2] = 1.0
    kw = dict(half_width=mp.halfWidth, slack=mp.slack)
    Qp, Rp, dRp = W.CTRL_TUNINGS["path"]
    path, tt, plan = engines(mp)

    def refused(fn, *a, **k):
        with pytest.raises(lpvmpc.LpvMpcError) as e:
            fn(*a, **k)
        return str(e.value)

    bare = lpvmpc.BatchedSolver("planner", 40, 0.05, W.PLAN_Q, W.PLAN_R, W.PLAN_dR, L_cf=W.PLAN_L, track=mp.PointAndTangent)
    assert "handoff_setup" in refused(path.race_init, tt, bare, p0, **kw)
    short = lpvmpc.BatchedSolver("controller", 10, 1 / 30.0, Qp, Rp, dRp, track=mp.PointAndTangent)
    refused(path.race_init, short, plan, p0, **kw)                                   # different N
    other_dt = lpvmpc.BatchedSolver("controller", 20, 1 / 20.0, Qp, Rp, dRp, track=mp.PointAndTangent)
    refused(path.race_init, other_dt, plan, p0, **kw)                                # different dt
    long_ = lpvmpc.BatchedSolver("controller", 24, 1 / 30.0, Qp, Rp, dRp, track=mp.PointAndTangent)
    long_tt = lpvmpc.BatchedSolver("controller", 24, 1 / 30.0, Qp, Rp, dRp, track=mp.PointAndTangent)
    assert "N <= 20" in refused(long_.race_init, long_tt, plan, p0, **kw)
    delayed = lpvmpc.BatchedSolver("controller", 20, 1 / 30.0, Qp, Rp, dRp, track=mp.PointAndTangent, steering_delay=1)
    assert "steeringDelay" in refused(delayed.race_init, tt, plan, p0, **kw)
    assert "steeringDelay" in refused(path.race_init, delayed, plan, p0, **kw)
    tt.set_option("warm_start", 1)
    assert "warm_start" in refused(path.race_init, tt, plan, p0, **kw)
    tt.set_option("warm_start", 0)
    from lpvmpc import _ffi
    path.observer_setup(_ffi.default_observer_config())
    assert "estimator" in refused(path.race_init, tt, plan, p0, **kw)
    path.observer_setup(None)
    refused(path.race_init, tt, plan, p0, laps=0, **kw)
    refused(plan.race_init, tt, path, p0, **kw)                                      # roles swapped
    refused(path.race_tick, 1)                                                       # not initialised
    # batch calls on all three handles while the race runs
    path.race_init(tt, plan, p0, **kw)
    path.race_tick(2)
    w = W.controller_batch(2, N=20, seed=1)
    for e in (path, tt):
        assert "race" in refused(e.solve, w["x0"], w["u_prev"], w["vel_ref"], w["curv_s"], w["u_old"], None, w["cf_new"], w["lap"])
    pw = W.planner_batch(2, N=40, seed=1)
    assert "race" in refused(plan.solve, pw["x0"], pw["u_prev"], None, pw["curv_s"], pw["u_old"], pw["max_ey"])
    refused(tt.cl_init, p0, mp.halfWidth, mp.slack)
    refused(tt.race_init, path, plan, p0, **kw)
    path.cl_release()                                                                # ends the race: batch calls work again
    tt.solve(w["x0"], w["u_prev"], w["vel_ref"], w["curv_s"], w["u_old"], None, w["cf_new"], w["lap"])
    # destroying a handle the race drives ends the race
    path.race_init(tt, plan, p0, **kw)
    plan.close()
    refused(path.race_tick, 1)
    for e in (path, tt, bare, short, other_dt, long_, long_tt, delayed):
        e.close()


def same_words(a, b, what=""):
    """Word for word, where a NaN matches a NaN (its payload is not specified)."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    if a.dtype.kind == "f":
        na, nb = np.isnan(a), np.isnan(b)
        diff = (na != nb) | (~na & (a.view(np.int64) != b.view(np.int64)))
    else:
        diff = a != b
    assert not diff.any(), "%s: %d words differ" % (what, int(diff.sum()))


def test_failed_race_init_leaves_the_three_handles_idle():
    """A race_init whose lap_step table ([256][laps + 2] int32 with laps = 2e9: ~2 TB) hipMalloc refuses, after the smaller buffers
    before it were allocated: the call fails, none of the three engines is left in a race, no HIP error stays pending, and a second
    race on the same engines equals one on fresh engines.  (No tick between the failed call and the second init: harmless on any build.)
    No vehicle reaches its planner in 12 ticks, and race_read's plan_iters / plan_status of a vehicle that never planned are what the
    planner's workspace held (docs/HISTORY.md, "Race recorder"): each planner first solves one 256-instance batch, so that every
    word compared is defined."""
    import lpvmpc
    from lpvmpc import _ffi, workloads as W
    mp = lshape()
    B = 256
    plant0 = start_line_fleet(mp, B, 11)
    kw = dict(half_track0=1, half_width=mp.halfWidth, slack=mp.slack)
    pw = W.planner_batch(B, N=40, seed=7)
    path, tt, plan = engines(mp)
    fresh = engines(mp)
    for q in (plan, fresh[2]):
        q.solve(pw["x0"], pw["u_prev"], None, pw["curv_s"], pw["u_old"], pw["max_ey"])
    with pytest.raises(lpvmpc.LpvMpcError):                                          # (a)
        path.race_init(tt, plan, plant0, laps=2_000_000_000, **kw)

    def run(p, t, q, first_tick):
        p.race_init(t, q, plant0, laps=1, **kw)                                      # (b): accepted on the same three engines
        first_tick(p)
        p.race_tick(11)                                                              # 9 seed ticks + 3 on the LPV branch
        ls, al = p.race_laps()
        pu, tu = p.race_predictions()
        out = dict(p.race_read(), lap_step=ls, alive=al, path_uPred=pu, tt_uPred=tu)
        p.cl_release()
        sol = q.solve(pw["x0"], pw["u_prev"], None, pw["curv_s"], pw["u_old"], pw["max_ey"])   # (c): the planner is free again
        return out, sol

    def checked_tick(p):                                                             # (d): the first launches after the failed call
        lib = _ffi.load()
        assert lib.lpvmpc_race_tick(p._h, 1) == 0, lib.lpvmpc_last_error(p._h).decode()

    a, sa = run(path, tt, plan, checked_tick)
    b, sb = run(*fresh, lambda p: p.race_tick(1))
    assert a["ticks"] == b["ticks"] == 12
    for k in a:
        same_words(a[k], b[k], k)
    for k in sa:
        same_words(sa[k], sb[k], "planner solve " + k)
    for e in (path, tt, plan) + tuple(fresh):
        e.close()
