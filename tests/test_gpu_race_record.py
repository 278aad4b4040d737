"""GPU: the race recorder (lpvmpc_race_record / _record_read / _lap_stats; BatchedSolver.race_record*, RaceFleet.record / trace /
lap_stats) against per-tick lpvmpc_race_read of an identical race, lpvmpc_local_position_batch, the host replay (tests/_race_ref.py)
and its numpy restatement (telemetry.lap_stats); its ring, sharding, refusals and lifetime."""
import ctypes as C

import numpy as np
import pytest

from tests import _race_observer_ref as RO

pytestmark = pytest.mark.gpu

KV = 0          # kernel_variant fixed on every handle: kernel routes may depend on B
STD = dict(psi_std=0.01, psiDot_std=0.05, x_std=0.01, y_std=0.01, v_std=0.02)
BASE = ("plant", "local", "cmd", "phase", "lap", "iters", "status")


def lshape():
    import lpvmpc
    return lpvmpc.Map("L_shape", 0.2)


def obs_cfg(**kw):
    from lpvmpc.observer import observer_config
    g = RO.estimator_gains()
    return observer_config(g["L_ls"], g["lim_ls"], g["L_hs"], g["lim_hs"], **kw)


def act_cfg():
    import lpvmpc
    c = lpvmpc.actuator_config(low_level_dyn=True)
    c.delay_a, c.delay_df = 4, 6
    return c


def engines(mp, sd=0):
    import lpvmpc
    from lpvmpc import workloads as W
    Qp, Rp, dRp = W.CTRL_TUNINGS["path"]; Qr, Rr, dRr = W.CTRL_TUNINGS["race"]
    kw = {"steering_delay": sd} if sd else {}
    path = lpvmpc.BatchedSolver("controller", 20, 1 / 30.0, Qp, Rp, dRp, track=mp.PointAndTangent, **kw)
    tt = lpvmpc.BatchedSolver("controller", 20, 1 / 30.0, Qr, Rr, dRr, track=mp.PointAndTangent, **kw)
    plan = lpvmpc.BatchedSolver("planner", 40, 0.05, W.PLAN_Q, W.PLAN_R, W.PLAN_dR, L_cf=W.PLAN_L, track=mp.PointAndTangent)
    for e in (path, tt, plan):
        e.set_option("kernel_variant", KV)
    plan.handoff_setup()
    return path, tt, plan


def close(*es):
    for e in es:
        e.close()


VARIANTS = dict(truth=dict(), estimator=dict(est=True), actuator=dict(act=True))


def start(mp, plant0, v, laps=3, half=1):
    sd = 3 if v.get("act") else 0
    path, tt, plan = engines(mp, sd)
    kw = dict(half_track0=half, laps=laps, half_width=mp.halfWidth, slack=mp.slack)
    if v.get("est"):
        kw["estimator"] = obs_cfg(seed=5, **v.get("obs", {}), **STD)
    if v.get("act"):
        kw["actuator"] = act_cfg()
    path.race_init(tt, plan, plant0, **kw)
    return path, tt, plan


def final(path):
    o = path.race_read()
    ls, al = path.race_laps()
    pu, tu = path.race_predictions()
    return dict(o, lap_step=ls, alive=al, path_uPred=pu, tt_uPred=tu)


def same(a, b):
    return np.asarray(a).shape == np.asarray(b).shape and np.asarray(a).tobytes() == np.asarray(b).tobytes()


def same_words(a, b, what=""):
    """Word for word, where a NaN matches a NaN (its payload is not specified); the first differing word is reported."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    if a.dtype.kind == "f":
        na, nb = np.isnan(a), np.isnan(b)
        diff = (na != nb) | (~na & (a.view(np.int64 if a.itemsize == 8 else np.int32) != b.view(np.int64 if b.itemsize == 8 else np.int32)))
    else:
        diff = a != b
    if diff.any():
        i = tuple(int(x[0]) for x in np.nonzero(diff))
        raise AssertionError("%s: %d words differ, first at %s: %r vs %r" % (what, int(diff.sum()), i, a[i], b[i]))


def same_stats(st, want, what=""):
    for k in ("f64", "i32", "end_tick"):
        same_words(st[k], want[k], "%s %s" % (what, k))


def per_tick(mp, plant0, T, v, laps=3):
    """The unrecorded race, read after every tick."""
    path, tt, plan = start(mp, plant0, v, laps)
    out = []
    for _ in range(T):
        path.race_tick(1)
        o = path.race_read()
        if v.get("est"):
            o["est"] = path.observer_read()[0]
        out.append(o)
    f = final(path)
    if v.get("est"):
        f["est"] = path.observer_read()
    if v.get("act"):
        f["act"] = path.actuator_read()
    close(path, tt, plan)
    return out, f


def recorded(mp, plant0, T, v, laps=3, chunks=(100, 140)):
    """The recorded race (stride 1, ring of T), enqueued in a few race_tick calls."""
    path, tt, plan = start(mp, plant0, v, laps)
    path.race_record(T, 1)
    done = 0
    for c in chunks:
        n = min(c, T - done)
        if n > 0:
            path.race_tick(n)
            done += n
    if done < T:
        path.race_tick(T - done)
    tr = path.race_record_read()
    st = path.race_lap_stats()
    f = final(path)
    if v.get("est"):
        f["est"] = path.observer_read()
    if v.get("act"):
        f["act"] = path.actuator_read()
    close(path, tt, plan)
    return tr, st, f


@pytest.fixture(scope="module")
def runs():
    """48 vehicles whose lap events are spread over the first ~90 ticks, 240 ticks, per variant."""
    mp = lshape()
    plant0 = RO.start_line_fleet(mp.PointAndTangent, 48, 7, 0.8, 0.97)
    out = {}
    for name, v in VARIANTS.items():
        out[name] = (recorded(mp, plant0, 240, v), per_tick(mp, plant0, 240, v))
    return mp, plant0, out


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_trace_equals_per_tick_reads(runs, variant):
    mp, plant0, out = runs
    (tr, _st, fr), (ref, fref) = out[variant]
    T = len(ref)
    assert tr["total"] == T and np.array_equal(tr["tick"], np.arange(T))
    ev = [int(np.argmax([o["phase"][b] >= 1 for o in ref])) for b in range(len(plant0)) if any(o["phase"][b] >= 1 for o in ref)]
    print(variant, "event ticks", sorted(ev))
    assert len(set(ev)) >= 10
    planned = 0
    B = len(plant0)
    k_rac = np.zeros(B, int); done = np.zeros(B, int)            # racing ticks entered, planner ticks run (per-tick reads only)
    for t in range(T):
        for k in BASE:
            assert same(tr[k][t], ref[t][k]), (variant, t, k)
        # the planner schedule, from the per-tick reads: a vehicle entering racing tick k with a finite plant (and estimate)
        # runs planner ticks 0 .. floor(2k/3) before it (race_plan_start_kernel)
        prev_ph = ref[t - 1]["phase"] if t else np.zeros(B, int)
        prev_pl = ref[t - 1]["plant"] if t else plant0
        fin = np.all(np.isfinite(prev_pl), axis=1)
        if variant == "estimator" and t:
            fin &= np.all(np.isfinite(ref[t - 1]["est"]), axis=1)
        racing = prev_ph == 1
        want = racing & fin & (done <= (2 * k_rac) // 3)
        done += want; k_rac += racing
        m = tr["plan_iters"][t] >= 0
        assert np.array_equal(m, want), (variant, t, np.nonzero(m != want)[0])
        planned += int(m.sum())
        assert np.array_equal(tr["plan_iters"][t][m], ref[t]["plan_iters"][m]), t
        assert np.array_equal(tr["plan_status"][t][m], ref[t]["plan_status"][m]), t
        assert np.all(tr["plan_status"][t][~m] == -1)
        if variant == "estimator":
            assert same(tr["est"][t], ref[t]["est"]), t
        else:
            assert np.all(np.isnan(tr["est"][t]))
    assert planned > 0
    for k in ("plant", "local", "cmd", "phase", "lap", "iters", "status", "lap_step", "alive", "path_uPred", "tt_uPred"):
        assert same(fr[k], fref[k]), k
    ran = np.any(tr["plan_iters"] >= 0, axis=0)        # (the planner words of a vehicle that never planned are not the race's)
    for k in ("plan_iters", "plan_status"):
        assert same(fr[k][ran], fref[k][ran]), k
    if variant == "estimator":
        assert same(fr["est"][0], fref["est"][0]) and same(fr["est"][1], fref["est"][1])
    if variant == "actuator":
        for a, b in zip(fr["act"], fref["act"]):
            assert same(a, b)


def test_lap0_statistics_measure_the_lateral_error(runs):
    """On ground truth the lap-0 branch measures local_position of the plant as it enters the tick, and the track channels are
    local_position of the plant after the tick: the measurement of tick t is the track frame of tick t - 1 (of plant0 on tick 0).
    With q9_swap the lap-0 branch stores that ey in local slot 3, and the lap-0 statistics must be of it, not of the heading error."""
    import lpvmpc
    mp, plant0, out = runs
    tr, st, _f = out["truth"][0]
    eng = lpvmpc.BatchedSolver("controller", 20, 1 / 30.0, np.eye(6), np.eye(2), np.ones(2), track=mp.PointAndTangent)
    lp0 = eng.local_position(plant0[:, [0, 1, 6]], mp.halfWidth, mp.slack)
    eng.close()
    B, T = plant0.shape[0], len(tr["tick"])
    ey_in = np.vstack([lp0[None, :, 1], tr["track_ey"][:-1]])             # [T, B]: ey of the plant each tick measures
    prev = np.vstack([np.zeros((1, B), np.int32), tr["phase"][:-1]])
    lap0_branch = (tr["phase"] == 0) | ((tr["phase"] == 1) & (prev == 0))
    solved = tr["src"] >= 0
    m = lap0_branch & solved
    assert m.sum() > 1000
    assert np.array_equal(tr["local_epsi"][m], ey_in[m])                    # slot 3 holds ey (quirk Q9)
    sse = np.zeros(B); mx = np.zeros(B)
    for t in range(T):
        c = m[t] & (tr["lap"][t] == 0)
        e = ey_in[t]
        sse = np.where(c, sse + e * e, sse)
        mx = np.where(c & (np.abs(e) > mx), np.abs(e), mx)
    assert same(st["sse_ey"][:, 0], sse) and same(st["max_ey"][:, 0], mx)
    print("lap 0: max |ey| over the fleet", float(mx.max()), "max |epsi| read from slot 5", float(np.abs(tr["local_ey"][m]).max()))


def test_track_frame_channels(runs):
    import lpvmpc
    mp, plant0, out = runs
    tr = out["truth"][0][0]
    eng = lpvmpc.BatchedSolver("controller", 20, 1 / 30.0, np.eye(6), np.eye(2), np.ones(2), track=mp.PointAndTangent)
    worst = 0.0
    for t in range(len(tr["tick"])):
        xyp = np.stack([tr["x"][t], tr["y"][t], tr["yaw"][t]], axis=1)
        lp = eng.local_position(xyp, mp.halfWidth, mp.slack)
        assert np.array_equal(tr["inside"][t], lp[:, 3].astype(np.int32)), t
        worst = max(worst, float(np.max(np.abs(tr["track"][t] - lp[:, :3]))))
        assert same(tr["track"][t], lp[:, :3]), (t, worst)
    eng.close()
    print("track frame: max |recorder - lpvmpc_local_position_batch| =", worst)


def test_reference_channels():
    """Lap-0-branch ticks (the event tick included) carry [0 0 0 1]; racing ticks the host replay's window point."""
    from tests._race_ref import RaceRef
    mp = lshape()
    B, T = 48, 120
    plant0 = RO.start_line_fleet(mp.PointAndTangent, B, 7, 0.8, 0.97)
    path, tt, plan = start(mp, plant0, {})
    path.race_record(T, 1)
    path.race_tick(T)
    tr = path.race_record_read()
    close(path, tt, plan)
    ref = RaceRef(mp.PointAndTangent, plant0, half_track0=1, laps=3, half_width=mp.halfWidth, slack=mp.slack)
    prev = np.zeros(B, int)
    apart = np.zeros(B, bool)
    lap0_ticks = racing = strict = 0
    worst = 0.0
    for t in range(T):
        ref.tick()
        ph = tr["phase"][t]
        d = np.max(np.abs(tr["plant"][t] - ref.plant), axis=1)
        apart |= ~((ph == 3) & (ref.phase == 3)) & ~(d <= 2e-2)
        l0 = (prev == 0) & (ph <= 1)
        assert np.all(tr["ref"][t][l0] == np.array([0.0, 0.0, 0.0, 1.0])), t
        lap0_ticks += int(l0.sum())
        for b in np.nonzero((prev == 1) & (ph == 1) & (ref.phase == 1) & ~apart)[0]:
            w = ref.casc[b].glue[0].win
            e = float(np.max(np.abs(tr["ref"][t][b] - w[:4, 0])))
            worst = max(worst, e)
            strict += e <= 1e-5
            racing += 1
            assert e <= 2e-2, (t, b, e)
        prev = ph
    print("reference channels: lap-0-branch vehicle-ticks", lap0_ticks, "racing", racing, "within 1e-5", strict, "worst", worst)
    assert lap0_ticks > 0 and racing > 100


def test_lap_stats_equal_the_numpy_restatement(runs):
    import lpvmpc
    from lpvmpc import telemetry
    mp, plant0, out = runs
    for name in VARIANTS:
        (tr, st, fr), _ = out[name]
        want = telemetry.lap_stats(tr, 3)
        print(name, "lap statistics: NaN words", int(np.isnan(st["f64"]).sum()))
        same_stats(st, want, name)
        ended = fr["phase"] >= 2
        assert np.all((st["end_tick"] >= 0) == ended)
        finished = fr["phase"] == 2
        assert np.array_equal(st["ticks"].sum(axis=1), fr["alive"] - finished), name     # alive ticks from 0 (recording from tick 0)
        assert np.all(st["ticks"][:, 0] > 0)
        s = telemetry.add_rmse(st)
        n = st["ticks"] > 0
        assert np.all(np.isnan(s["rmse_ey"][~n])) and np.array_equal(s["rmse_ey"][n], np.sqrt(st["sse_ey"][n] / st["ticks"][n]), equal_nan=True)
    assert lpvmpc.RaceFleet is not None


def test_stride_and_ring():
    mp = lshape()
    B = 24
    plant0 = RO.start_line_fleet(mp.PointAndTangent, B, 11, 0.85, 0.97)
    path, tt, plan = start(mp, plant0, {})
    path.race_record(43, 1)
    path.race_tick(43)
    full = path.race_record_read()
    close(path, tt, plan)
    path, tt, plan = start(mp, plant0, {})
    path.race_record(7, 3)
    path.race_tick(25); path.race_tick(15)
    r = path.race_record_read()
    assert r["total"] == 14 and np.array_equal(r["tick"], np.arange(21, 40, 3))
    for k in ("plant", "local", "cmd", "ref", "track", "est", "phase", "lap", "src", "iters", "status", "plan_iters", "plan_status", "inside"):
        assert same(r[k], full[k][21:40:3]), k
    last = path.race_record_read(last=2)
    assert np.array_equal(last["tick"], [36, 39]) and same(last["plant"], full["plant"][[36, 39]])
    # stop: nothing kept, statistics refused
    path.race_record(0)
    r0 = path.race_record_read()
    assert r0["total"] == 0 and r0["tick"].shape == (0,)
    from lpvmpc import LpvMpcError, telemetry
    with pytest.raises(LpvMpcError):
        path.race_lap_stats()
    # restart at tick 40: ring and statistics start afresh
    path.race_record(5, 1)
    path.race_tick(3)
    r1 = path.race_record_read()
    assert r1["total"] == 3 and np.array_equal(r1["tick"], [40, 41, 42])
    for k in ("plant", "local", "phase", "src", "iters"):
        assert same(r1[k], full[k][40:43]), k
    st = path.race_lap_stats()
    sub = {k: (v[40:43] if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == 43 else v) for k, v in full.items()}
    want = telemetry.lap_stats(sub, 3, phase0=full["phase"][39])
    same_stats(st, want, "restart")
    close(path, tt, plan)


def test_sharding():
    mp = lshape()
    B, T = 64, 90
    plant0 = RO.start_line_fleet(mp.PointAndTangent, B, 9)

    def run(p0, off):
        v = dict(est=True, obs=dict(vehicle_offset=off))
        path, tt, plan = start(mp, p0, v)
        path.race_record(T, 1)
        path.race_tick(T)
        tr, st = path.race_record_read(), path.race_lap_stats()
        close(path, tt, plan)
        return tr, st

    a, sa = run(plant0, 0)
    lo, slo = run(plant0[:32], 0)
    hi, shi = run(plant0[32:], 32)
    from lpvmpc import _ffi
    for k in _ffi.REC_F64_NAMES + _ffi.REC_I32_NAMES:
        assert same(a[k], np.concatenate([lo[k], hi[k]], axis=1)), k
    same_stats(sa, {k: np.concatenate([slo[k], shi[k]]) for k in ("f64", "i32", "end_tick")}, "shards")
    assert np.sum(a["phase"][-1] >= 1) >= B // 2


def test_refusals_and_lifetime():
    import lpvmpc
    from lpvmpc import _ffi
    mp = lshape()
    lib = _ffi.load()
    B = 48
    plant0 = RO.start_line_fleet(mp.PointAndTangent, B, 3, 0.85, 0.97)
    path, tt, plan = engines(mp)

    def rc(cap, stride, h=None):
        cfg = _ffi.RaceRecordConfig(cap, stride)
        return lib.lpvmpc_race_record(h or path._h, C.byref(cfg))

    assert rc(4, 1) == _ffi.E_ARG                                            # no race on the handle
    assert lib.lpvmpc_race_record_read(path._h, 1, None, None, None, None) == _ffi.E_ARG
    assert lib.lpvmpc_race_lap_stats(path._h, None, None, None) == _ffi.E_ARG
    assert lib.lpvmpc_race_record(path._h, None) == _ffi.E_ARG
    path.race_init(tt, plan, plant0, half_track0=1, laps=3, half_width=mp.halfWidth, slack=mp.slack)
    assert rc(4, 1, tt._h) == _ffi.E_ARG                                     # the race belongs to the path handle
    assert rc(-1, 1) == _ffi.E_ARG and rc(4, 0) == _ffi.E_ARG and rc(4, -2) == _ffi.E_ARG
    assert lib.lpvmpc_race_record_read(path._h, -1, None, None, None, None) == _ffi.E_ARG
    # a ring of ~22 TB: hipMalloc refuses it at once; the race runs on unrecorded and equal to an unrecorded race
    path.race_tick(10)
    assert rc(2_000_000_000, 1) == _ffi.E_NOMEM
    assert "hipMalloc" in lib.lpvmpc_last_error(path._h).decode()
    assert lib.lpvmpc_race_lap_stats(path._h, None, None, None) == _ffi.E_ARG
    path.race_tick(30)
    p2, t2, q2 = engines(mp)
    p2.race_init(t2, q2, plant0, half_track0=1, laps=3, half_width=mp.halfWidth, slack=mp.slack)
    p2.race_tick(40)
    a, b = final(path), final(p2)
    for k in a:
        if k not in ("plan_iters", "plan_status"):       # (compared below, in the traces)
            assert same(a[k], b[k]), k
    # the recorder works after the refusal: both races recorded for 20 more ticks, trace for trace
    path.race_record(20, 1); p2.race_record(20, 1)
    path.race_tick(20); p2.race_tick(20)
    ta, tb = path.race_record_read(), p2.race_record_read()
    for k in _ffi.REC_F64_NAMES + _ffi.REC_I32_NAMES:
        assert same(ta[k], tb[k]), k
    same_stats(path.race_lap_stats(), p2.race_lap_stats(), "after E_NOMEM")
    path.race_record(0)
    close(p2, t2, q2)
    # a refused argument leaves a running recorder as it was
    path.race_record(5, 2)
    path.race_tick(4)
    assert rc(5, 0) == _ffi.E_ARG
    path.race_tick(2)
    assert path.race_record_read()["total"] == 3
    # cl_release frees the recorder; the next race starts unrecorded
    path.cl_release()
    path.race_init(tt, plan, plant0, half_track0=1, laps=3, half_width=mp.halfWidth, slack=mp.slack)
    tot = np.zeros(1, np.int32)
    assert lib.lpvmpc_race_record_read(path._h, 8, tot.ctypes.data_as(C.c_void_p), None, None, None) == 0 and tot[0] == 0
    assert lib.lpvmpc_race_lap_stats(path._h, None, None, None) == _ffi.E_ARG
    path.race_record(4, 1)
    path.race_tick(2)
    assert path.race_record_read()["total"] == 2
    close(tt)                                               # destroying a handle of the race ends it, recorder included
    assert rc(4, 1) == _ffi.E_ARG
    close(path, plan)
    assert lpvmpc.RaceFleet is not None


def test_race_fleet_interface():
    import lpvmpc
    mp = lshape()
    plant0 = RO.start_line_fleet(mp.PointAndTangent, 16, 5, 0.9, 0.97)
    f = lpvmpc.RaceFleet(mp, plant0, laps=2, half_track0=1, kernel_variant=KV)
    f.record(20, 2)
    f.run(40)
    tr = f.trace()
    assert tr["total"] == 20 and tr["plant"].shape == (20, 16, 8) and tr["x"].shape == (20, 16)
    s = f.lap_stats()
    assert s["rmse_v"].shape == (16, 3) and np.all(np.isfinite(s["rmse_v"][:, 0]))
    f.close()


def test_full_size():
    mp = lshape()
    B, T = 8192, 300
    rng = np.random.default_rng(1)
    plant0 = RO.start_line_fleet(mp.PointAndTangent, 64, 13, 0.85, 0.99)[rng.integers(0, 64, B)]
    plant0[:, 2] += rng.uniform(-0.05, 0.05, B)
    path, tt, plan = start(mp, plant0, {}, laps=1)
    path.race_record(30, 10)
    path.race_tick(T)
    tr = path.race_record_read()
    st = path.race_lap_stats()
    o = path.race_read()
    close(path, tt, plan)
    assert tr["total"] == 30 and np.array_equal(tr["tick"], np.arange(0, 300, 10))
    assert tr["plant"].shape == (30, B, 8) and tr["phase"].shape == (30, B) and st["ticks"].shape == (B, 2)
    alive_end = o["phase"] <= 1                # (a vehicle whose plant diverges on a tick is lost on the next one)
    for t in range(30):
        alive = (tr["phase"][t] <= 1) & alive_end
        for k in ("plant", "local", "cmd", "ref", "track"):
            assert np.all(np.isfinite(tr[k][t][alive])), (t, k)
    assert np.all(np.isnan(tr["est"]))
    ended = 0
    for b in np.nonzero(tr["phase"][-1] >= 2)[0]:
        t0 = int(np.argmax(tr["phase"][:, b] >= 2))
        ended += 1
        for t in range(t0 + 1, 30):
            for k in ("plant", "local", "cmd", "ref", "track", "phase", "lap", "inside"):
                assert same(tr[k][t][b], tr[k][t0][b]), (b, t, k)
            assert tr["src"][t][b] == -1 and tr["iters"][t][b] == 0
    print("full size: phases at the end", np.bincount(o["phase"], minlength=4).tolist(), "vehicles ended in the window", ended)
    assert np.sum(o["phase"] >= 1) >= B // 2
