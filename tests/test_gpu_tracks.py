"""GPU: per-vehicle tracks (lpvmpc_set_tracks, lpvmpc_tracks_read; include/lpvmpc.h, "Per-vehicle tracks").  A handle with a track
palette bound transforms and linearises vehicle b on track track_of[b]:
  * word for word against the per-handle path that exists without a binding -- one plain handle per palette entry, created with that
    entry's table and called with its half width and slack -- for the transforms, lpv, estimate_abc and the solves (plain and
    masked), with and without model rows bound beside the tracks;
  * against the oracle (oracle/plant_ref.py at 1e-11; oracle/lpv_ref.py at the bars of tests/test_gpu_horizons.py: 1e-11 of each
    array's largest magnitude for lpv, 1e-12 for the seed-mode linearisation);
  * the lap-0 fleet, started through lpvmpc_cl_init_tyres: every vehicle of a mixed fleet bit for bit the same vehicle of a
    homogeneous fleet on a handle of its track (plain, with plant and tyre rows, with the estimator behind noisy sensors, with the
    per-vehicle estimator), and the plain one against the host replay (2e-6, equal iteration counts);
  * the race, started through lpvmpc_race_init_tyres on three handles with equal bindings: a mixed 12-vehicle race through its lap
    events bit for bit the homogeneous races, the event ticks those of the host replay; the hand-off on a bound planner handle;
  * a one-entry palette of the handle's own track changes no word; refusals, lifetime and the read-back.
NaN compares as NaN.  Palette and batches: tests/_tracks.py."""
import ctypes as C

import numpy as np
import pytest

from oracle import lpv_ref as L, plant_ref as PR
from tests import _model_params as M
from tests import _tracks as TK
from tests.test_gpu_horizons import relclose

pytestmark = pytest.mark.gpu

P = dict(L.DEFAULT_PARAMS)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def engine(w, track=None, **kw):
    import lpvmpc
    return lpvmpc.BatchedSolver(w["kind"], w["N"], w["dt"], w["Q"], w["R"], w["dR"], L_cf=w["L_cf"], track=track, **kw)


def plain_engine(track=None):
    import lpvmpc
    return lpvmpc.BatchedSolver("controller", 8, 1.0 / 30.0, np.eye(6), np.eye(2), np.ones(2), track=track)


def lpv(e, w):
    return e.lpv(w["x0"], w["u_prev"], w["vel_ref"], w["curv_s"], cf_new=w["cf_new"], lap=w["lap"])


def solve(e, w, active=None):
    a = (w["x0"], w["u_prev"], w["vel_ref"], w["curv_s"], w["u_old"], w["max_ey"], w["cf_new"], w["lap"])
    return e.solve(*a) if active is None else e.solve_batch_masked(active, *a)


# ---- 1. transforms ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", TK.SIZES)
def test_transforms_on_a_mixed_batch(B):
    """local_position / global_position of a bound handle (created without a table of its own): every instance equals, word for
    word, the plain handle of its track called with that track's half width and slack -- the bound call's own half width and slack
    (here 123, 456) are ignored -- and the whole batch is within 1e-11 of oracle/plant_ref.py, the sentinels and inside flags equal."""
    maps, of = TK.palette(), TK.cycle(B)
    sey, pts = TK.transform_points(B, 7000 + B, maps, of)
    e = plain_engine()
    e.set_tracks(maps, of)
    loc, glob = e.local_position(pts, 123.0, 456.0), e.global_position(sey)
    e.close()
    for t, idx in TK.groups(of):
        p = plain_engine(maps[t].PointAndTangent)
        assert same(loc[idx], p.local_position(pts[idx], maps[t].halfWidth, maps[t].slack)), ("local", B, t)
        assert same(glob[idx], p.global_position(sey[idx])), ("global", B, t)
        p.close()
    ref_l = np.array([PR.get_local_position(maps[of[b]].PointAndTangent, maps[of[b]].halfWidth, maps[of[b]].slack, *pts[b]) for b in range(B)], float)
    ref_g = np.array([PR.get_global_position(maps[of[b]].PointAndTangent, *sey[b]) for b in range(B)], float)
    assert np.array_equal(loc[:, 3], ref_l[:, 3])
    el, eg = float(np.max(np.abs(loc - ref_l))), float(np.max(np.abs(glob - ref_g)))
    print("B=%d: local max err %.2e, global max err %.2e, %d of %d inside" % (B, el, eg, int(loc[:, 3].sum()), B))
    assert el <= 1e-11 and eg <= 1e-11
    if B >= 5:
        assert np.any(loc[:, 3] == 0) and np.any(loc[:, 3] == 1) and np.all(loc[loc[:, 3] == 0, :3] == 10000)


# ---- 2. linearisation -------------------------------------------------------------------------------------------------------
CASES = {"ctrl20_lap0": ("controller", 20, TK.ctrl_lap0, 8200), "plan40": ("planner", 40, TK.plan, 8300)}


def oracle_lpv(kind, w, j, tab, p, cf):
    if kind == "controller":
        return L.ctrl_lpv_prediction(p, w["dt"], w["N"], tab, w["x0"][j], w["u_prev"][j], w["vel_ref"][j], None, cf, 0)
    return L.plan_lpv_prediction(p, w["dt"], w["N"], tab, w["x0"][j], w["curv_s"][j], w["u_prev"][j])


def oracle_abc(kind, w, xx, delta, j, tab, p):
    if kind == "controller":
        return L.ctrl_estimate_abc(p, w["dt"], w["N"], tab, xx[j], np.stack([delta[j], np.zeros(w["N"])], axis=1))
    return L.plan_estimate_abc(p, w["dt"], w["N"], tab, xx[j], delta[j])


@pytest.mark.parametrize("B", (5, 67))
@pytest.mark.parametrize("model", (False, True))
@pytest.mark.parametrize("name", sorted(CASES))
def test_lpv_and_seed_mode_on_a_mixed_batch(name, model, B):
    """lpv() states and [A | B] and the seed-mode [A | B] of a bound handle, word for word those of the per-track handles, and
    against the oracle on each vehicle's table.  model: ROWS of tests/_model_params.py bound beside the tracks (the per-track
    handles then bind their vehicles' rows too, and the oracle takes each vehicle's row with its Cf for both axles of the controller
    roll-out); without model rows the controller roll-out takes the call's cf_new, here 57.5 != the handle's Cf."""
    kind, N, make, seed = CASES[name]
    maps, of = TK.palette(), TK.cycle(B)
    w = dict(make(B, N, seed + B, maps, of), cf_new=57.5)
    xx, delta = TK.seed_inputs(B, N, kind, seed + 50 + B, maps, of)
    rows = M.interleaved(B) if model else None
    e = engine(w)
    e.set_tracks(maps, of)
    if model:
        e.set_model_params(rows)
    S, A, Bm = lpv(e, w)
    Ae, Be = e.estimate_abc(xx, delta)
    e.close()
    for t, idx in TK.groups(of):
        p = engine(w, maps[t].PointAndTangent)
        if model:
            p.set_model_params(rows[idx])
        Sg, Ag, Bg = lpv(p, TK.sub(w, idx))
        Aeg, Beg = p.estimate_abc(xx[idx], delta[idx])
        p.close()
        for got, want, what in ((S, Sg, "states"), (A, Ag, "A"), (Bm, Bg, "B"), (Ae, Aeg, "abc A"), (Be, Beg, "abc B")):
            assert same(got[idx], want), (name, model, B, t, what)
    worst = 0.0
    for j in range(B):
        tab = maps[of[j]].PointAndTangent
        p = dict(P, **M.params_of(rows[j])) if model else P
        Sr, Ar, Br = oracle_lpv(kind, w, j, tab, p, float(rows[j, 4]) if model else w["cf_new"])
        Aer, Ber = oracle_abc(kind, w, xx, delta, j, tab, p)
        for got, want, tol, what in ((S[j], Sr, 1e-11, "states"), (A[j], Ar, 1e-11, "A"), (Bm[j], Br, 1e-11, "B"),
                                     (Ae[j], Aer, 1e-12, "abc A"), (Be[j], Ber, 1e-12, "abc B")):
            worst = max(worst, relclose(got, want, tol, "%s #%d %s" % (name, j, what)))
    print("%s model=%s B=%d: word for word; against the oracle max rel err %.2e" % (name, model, B, worst))


# ---- 3. solves --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_solves_on_a_mixed_batch(name):
    """B = 67, plain and masked (every third instance left out: its rows keep the caller's NaN): status, iteration count, xPred and
    uPred are word for word those of the per-track handles on their sub-batches."""
    kind, N, make, seed = CASES[name]
    B = 67
    maps, of = TK.palette(), TK.cycle(B)
    w = make(B, N, seed + B, maps, of)
    active = (np.arange(B) % 3 != 0).astype(np.int32)
    e = engine(w)
    e.set_tracks(maps, of)
    got = [solve(e, w), solve(e, w, active)]
    from tests.test_gpu_model_params import _dev_solve
    dev = _dev_solve(e, w)                                        # lpvmpc_solve_batch_dev on the bound handle: the plain call's words
    for k in ("status", "iters", "polish", "xPred", "uPred", "resid"):
        assert same(dev[k], got[0][k]), (name, "dev", k)
    e.close()
    assert np.all(np.isin(got[0]["status"], (1, 2, -2, -3, 3))) and np.mean(got[0]["status"] == 1) > 0.5
    for t, idx in TK.groups(of):
        p = engine(w, maps[t].PointAndTangent)
        g = TK.sub(w, idx)
        ref = [solve(p, g), solve(p, g, active[idx])]
        p.close()
        for a, r, how in zip(got, ref, ("plain", "masked")):
            for k in ("status", "iters", "xPred", "uPred"):
                assert same(a[k][idx], r[k]), (name, how, t, k)
    print("%s: B = 67, plain and masked, word for word; iters %d..%d" % (name, got[0]["iters"].min(), got[0]["iters"].max()))


# ---- 4. identity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_one_entry_palette_of_the_own_track_changes_no_word(name):
    """T = 1, the handle's own table, half width and slack: lpv, estimate_abc, solve and the transforms equal the unbound handle's,
    word for word; after unbinding the handle is unbound again."""
    import lpvmpc
    kind, N, make, seed = CASES[name]
    B = 67
    mp = lpvmpc.Map("L_shape", 0.2)
    of = np.zeros(B, np.int32)
    w = make(B, N, seed + 1, [mp], of)
    xx, delta = TK.seed_inputs(B, N, kind, seed + 2, [mp], of)
    sey, pts = TK.transform_points(B, seed + 3, [mp], of)

    def everything(e):
        return (list(lpv(e, w)) + list(e.estimate_abc(xx, delta)) + [v for _, v in sorted(solve(e, w).items())] +
                [e.local_position(pts, mp.halfWidth, mp.slack), e.global_position(sey)])

    e = engine(w, mp.PointAndTangent)
    want = everything(e)
    assert e.tracks_read() is None
    e.set_tracks([mp], of)
    r = e.tracks_read()
    assert same(r["tables"][0], mp.PointAndTangent) and same(r["track_of"], of) and r["half_width"][0] == mp.halfWidth and r["slack"][0] == mp.slack
    for a, b in zip(everything(e), want):
        assert same(a, b), name
    e.set_tracks(None, None)
    assert e.tracks_read() is None
    for a, b in zip(everything(e), want):
        assert same(a, b), name
    e.close()


# ---- 4. - 6. the lap-0 fleet ------------------------------------------------------------------------------------------------
FLEET_B, FLEET_T = 67, 10
VARIANTS = ("plain", "rows", "estimator", "estimator_vehicles")
_FLEET = {}


def path_engine(track=None):
    import lpvmpc
    from lpvmpc import workloads as W
    Q, R, dR = W.CTRL_TUNINGS["path"]
    return lpvmpc.BatchedSolver("controller", 20, 1 / 30.0, Q, R, dR, track=track)


def fleet_run(variant, plant0, mp=None, bind=None):
    """T ticks of a 67-vehicle lap-0 fleet, every word read back per tick.  mp: a homogeneous fleet on a handle of that track; bind =
    (maps, track_of): a handle without a table of its own, the tracks bound.  plain: an unbound handle starts through lpvmpc_cl_init
    (the plain kernels), a bound one through lpvmpc_cl_init_tyres with NULL rows; rows: sampled plant rows, every other vehicle on
    the Pacejka tyre; estimator: the gain-scheduled estimator behind noisy sensors (noise keyed by vehicle id);
    estimator_vehicles: the same with the per-vehicle estimator bound (nominal rows, the configuration's tables per vehicle)."""
    import lpvmpc
    from tests import _race_observer_ref as RO
    from tests.test_gpu_delayed_fleets import STD, obs_cfg
    B = plant0.shape[0]
    e = path_engine(None if mp is None else mp.PointAndTangent)
    kw = {}
    if bind is not None:
        e.set_tracks(*bind)
        kw = dict(tyre_params="linear")
    if variant == "rows":
        tyres = lpvmpc.tyre_params(B)
        tyres[::2, 0] = 0.0
        kw = dict(plant_params=lpvmpc.sample_plant_params(B, 31), tyre_params=tyres)
    if variant.startswith("estimator"):
        e.observer_setup(obs_cfg(**dict(STD, seed=11)))
    if variant == "estimator_vehicles":
        g = RO.estimator_gains()
        e.set_observer_vehicles(np.tile([0.125, 0.125, 1.98, 0.03, 60.0, 60.0, 0.05], (B, 1)), np.tile(g["L_ls"], (B, 1, 1, 1)),
                                np.tile(g["L_hs"], (B, 1, 1, 1)))
        kw = dict(kw, plant_params="nominal")
    hw, sl = (123.0, 456.0) if mp is None else (mp.halfWidth, mp.slack)      # bound: the call's half width and slack are ignored
    e.cl_init(plant0, hw, sl, q9_swap=True, n_sub=7, **kw)
    out = []
    for _ in range(FLEET_T):
        e.cl_tick(1)
        o = e.cl_read()
        if variant.startswith("estimator"):
            o["est"], o["meas"] = e.observer_read()
        out.append(o)
    e.close()
    return out


def mixed_fleet(variant):
    """The mixed fleet of a variant, run once and shared."""
    if variant not in _FLEET:
        maps, of = TK.palette(), TK.cycle(FLEET_B)
        plant0 = TK.fleet_starts(FLEET_B, 8400, maps, of)
        _FLEET[variant] = (maps, of, plant0, fleet_run(variant, plant0, bind=(maps, of)))
    return _FLEET[variant]


@pytest.mark.parametrize("variant", VARIANTS)
def test_one_entry_palette_changes_no_word_of_a_fleet(variant):
    """T = 1, the handle's own track, half width and slack: every word of 10 ticks of a 67-vehicle fleet equals the unbound run's."""
    import lpvmpc
    mp = lpvmpc.Map("L_shape", 0.2)
    of = np.zeros(FLEET_B, np.int32)
    plant0 = TK.fleet_starts(FLEET_B, 8401, [mp], of)
    a, b = fleet_run(variant, plant0, mp=mp), fleet_run(variant, plant0, bind=([mp], of))
    for t in range(FLEET_T):
        assert sorted(a[t]) == sorted(b[t])
        for k in a[t]:
            assert same(a[t][k], b[t][k]), (variant, t, k)
    assert np.all(np.isfinite(a[-1]["plant"])) and np.mean(a[-1]["local"][:, 4] < 9999) >= 0.9


@pytest.mark.parametrize("variant", VARIANTS)
def test_mixed_fleet_equals_the_homogeneous_fleets(variant):
    """Every vehicle of the mixed fleet equals, bit for bit and on every tick, the same vehicle of a homogeneous 67-vehicle fleet on a
    handle of its track (one run per palette entry; only the vehicles of that entry are compared -- the others are off that track)."""
    maps, of, plant0, got = mixed_fleet(variant)
    for t_, idx in TK.groups(of):
        ref = fleet_run(variant, plant0, mp=maps[t_])
        for t in range(FLEET_T):
            for k in got[t]:
                assert same(got[t][k][idx], ref[t][k][idx]), (variant, t_, t, k)
    last = got[-1]                                                # (not an empty comparison: the fleet drives, on its tracks)
    assert np.all(np.isfinite(last["plant"])) and np.mean(last["local"][:, 4] < 9999) >= 0.9 and np.mean(np.isin(last["status"], (1, 2))) >= 0.9


def test_mixed_fleet_against_the_host_replay():
    """The mixed plain fleet against the host replay, vehicle by vehicle on its own table with its own half width and slack: nothing
    of the device on the other side, so a mistake shared by the bound and the unbound forms -- a wrong width, a wrong table -- cannot
    hide behind the comparison above.  The existing fleet bar: plant, measurement and command within 2e-6, equal iteration counts
    and statuses, on each of the 10 ticks (nine seed-mode ticks and the first LPV tick)."""
    maps, of, plant0, got = mixed_fleet("plain")
    ref = TK.lap0_replay(maps, of, plant0, FLEET_T)
    worst = 0.0
    for t in range(FLEET_T):
        assert np.array_equal(got[t]["iters"], ref[t]["iters"]) and np.array_equal(got[t]["status"], ref[t]["status"]), t
        for k in ("plant", "local", "cmd"):
            worst = max(worst, float(np.max(np.abs(got[t][k] - ref[t][k]))))
    print("mixed fleet against the host replay: max difference %.2e over %d ticks" % (worst, FLEET_T))
    assert worst <= 2e-6


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------
def _raw_set(e, T, rows, tab, hw, sl, B, of):
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return e._lib.lpvmpc_set_tracks(e._h, T, ptr(rows), ptr(tab), ptr(hw), ptr(sl), B, ptr(of))


def test_refusals_leave_the_binding_unchanged():
    import lpvmpc
    from lpvmpc.track import pack_tracks
    E_ARG = lpvmpc._ffi.E_ARG
    maps, B = TK.palette(), 5
    of = TK.cycle(B)
    rows, tab, hw, sl, of32 = pack_tracks(maps, of)
    e = plain_engine()
    e.set_tracks(maps[:2], np.array([0, 1, 1, 0, 1]))
    before = e.tracks_read()

    def refused(T=6, rows=rows, tab=tab, hw=hw, sl=sl, B=B, of=of32):
        assert _raw_set(e, T, rows, tab, hw, sl, B, of) == E_ARG
        after = e.tracks_read()
        assert all(same(a, b) for a, b in zip(after["tables"], before["tables"])) and len(after["tables"]) == 2
        assert all(same(after[k], before[k]) for k in ("half_width", "slack", "track_of"))

    big = np.zeros((65, 16, 6)); big[:, :, 4] = 1.0
    refused(T=65, rows=np.full(65, 2, np.int32), tab=big, hw=np.ones(65), sl=np.ones(65), of=np.zeros(B, np.int32))
    refused(T=-1)
    for bad in (1, 17, 0, -3):
        r = rows.copy(); r[2] = bad
        refused(rows=r)
    for word in (np.nan, np.inf, -np.inf):
        t = tab.copy(); t[3, 2, 1] = word
        refused(tab=t)
    for length in (0.0, -0.5):
        t = tab.copy(); t[1, 3, 4] = length
        refused(tab=t)
    for v in (np.nan, np.inf, -0.1):
        a = hw.copy(); a[4] = v
        refused(hw=a)
        a = sl.copy(); a[0] = v
        refused(sl=a)
    for v in (-1, 6):
        o = of32.copy(); o[3] = v
        refused(of=o)
    refused(B=-2)
    for k in ("rows", "tab", "hw", "sl", "of"):
        refused(**{k: None})
    # a non-finite word beyond the rows in use is ignored and reads back as zero
    t = tab.copy(); t[0, 15, 0] = np.nan
    assert _raw_set(e, 6, rows, t, hw, sl, B, of32) == 0
    r = e.tracks_read()
    assert len(r["tables"]) == 6 and all(same(a, m.PointAndTangent) for a, m in zip(r["tables"], maps)) and same(r["track_of"], of32)
    # another B than the binding's is refused before anything is launched
    sey, pts = TK.transform_points(7, 1, maps, TK.cycle(7))
    for call in (lambda: e.local_position(pts, 0.3, 0.15), lambda: e.global_position(sey),
                 lambda: e.lpv(np.ones((7, 6)), np.zeros((7, 8, 2)), np.ones((7, 9)), None, lap=0),
                 lambda: e.estimate_abc(np.ones((7, 8, 6)), np.zeros((7, 8))),
                 lambda: e.solve(np.ones((7, 6)), np.zeros((7, 8, 2)), np.ones((7, 9)), None, np.zeros((7, 2)), None, 60.0, 0),
                 lambda: e.solve_batch_masked(np.ones(7, np.int32), np.ones((7, 6)), np.zeros((7, 8, 2)), np.ones((7, 9)), None, np.zeros((7, 2)),
                                              None, 60.0, 0)):
        with pytest.raises(lpvmpc.LpvMpcError) as err:
            call()
        assert err.value.code == E_ARG and "lpvmpc_set_tracks" in str(err.value)
    e.close()


# ---- 4. / 7. the race and the hand-off ----------------------------------------------------------------------------------------
def race_engines(mp=None, bind=None):
    """(path, tt, planner) with the reference's tunings on the track of mp, or without a table of their own and bind = (maps,
    track_of) bound to all three."""
    import lpvmpc
    from lpvmpc import workloads as W
    tab = None if mp is None else mp.PointAndTangent
    Qr, Rr, dRr = W.CTRL_TUNINGS["race"]
    path = path_engine(tab)
    tt = lpvmpc.BatchedSolver("controller", 20, 1 / 30.0, Qr, Rr, dRr, track=tab)
    plan = lpvmpc.BatchedSolver("planner", 40, 0.05, W.PLAN_Q, W.PLAN_R, W.PLAN_dR, L_cf=W.PLAN_L, track=tab)
    for e in (path, tt, plan):
        e.set_option("kernel_variant", 0)                         # (kernel routes may depend on B)
        if bind is not None:
            e.set_tracks(*bind)
    plan.handoff_setup()
    return path, tt, plan


def race_run(plant0, T, mp=None, bind=None, est=False, laps=2):
    """T ticks of a race with the recorder on, every word read back per tick, the lap table, the kept records and the lap
    statistics at the end.  An unbound race starts through lpvmpc_race_init (or _observed), a bound one through lpvmpc_race_init_tyres
    with NULL rows and the call's half width and slack set to values no track has."""
    from tests.test_gpu_delayed_fleets import STD, obs_cfg
    path, tt, plan = race_engines(mp, bind)
    kw = dict(estimator=obs_cfg(**dict(STD, seed=13))) if est else {}
    if bind is not None:
        kw.update(tyre_params="linear", half_width=123.0, slack=456.0)
    else:
        kw.update(half_width=mp.halfWidth, slack=mp.slack)
    path.race_init(tt, plan, plant0, half_track0=1, laps=laps, **kw)
    path.race_record(T)
    ticks = []
    for _ in range(T):
        path.race_tick(1)
        o = path.race_read()
        o["path_uPred"], o["tt_uPred"] = path.race_predictions()
        if est:
            o["est"], o["meas"] = path.observer_read()
        ticks.append(o)
    ls, alive = path.race_laps()
    rec = path.race_record_read()
    stats = path.race_lap_stats()
    out = dict(ticks=ticks, lap_step=ls, alive=alive, rec={k: v for k, v in rec.items() if isinstance(v, np.ndarray) and v.ndim >= 2},
               stats=dict(f64=stats["f64"], i32=stats["i32"], end_tick=stats["end_tick"]))
    for e in (path, tt, plan):
        e.close()
    return out


def race_same(a, b, idx, what):
    """Every word of the vehicles idx of two race_run results."""
    for t, (x, y) in enumerate(zip(a["ticks"], b["ticks"])):
        assert sorted(x) == sorted(y)
        ran = a["ticks"][t - 1]["phase"][idx] == 1 if t else np.zeros(len(idx), bool)      # the planner runs from the tick after the event
        for k in x:
            if k in ("plan_iters", "plan_status"):                # (before a vehicle's first planner tick: whatever the workspace held)
                assert same(x[k][idx][ran], y[k][idx][ran]), (what, t, k)
            elif k != "ticks":
                assert same(x[k][idx], y[k][idx]), (what, t, k)
    assert same(a["lap_step"][idx], b["lap_step"][idx]) and same(a["alive"][idx], b["alive"][idx]), what
    for k in a["rec"]:
        assert same(a["rec"][k][:, idx], b["rec"][k][:, idx]), (what, "record", k)         # [records, B, ...]
    for k in a["stats"]:
        assert same(a["stats"][k][idx], b["stats"][k][idx]), (what, "lap statistics", k)


@pytest.mark.parametrize("est", (False, True))
def test_one_entry_palette_changes_no_word_of_a_race(est):
    """T = 1, the handles' own track, half width and slack bound to path, tt and planner: every word of 6 ticks of a 67-vehicle race
    equals the unbound run's, the recorder's records and lap statistics included (on ground truth and with the estimator)."""
    from tests.test_gpu_race import lshape, start_line_fleet
    mp = lshape()
    B = 67
    plant0 = start_line_fleet(mp, B, 21)
    a = race_run(plant0, 6, mp=mp, est=est)
    b = race_run(plant0, 6, bind=([mp], np.zeros(B, np.int32)), est=est)
    race_same(a, b, np.arange(B), "T = 1, est=%s" % est)
    assert np.all(a["ticks"][-1]["phase"] < 2) and np.all(np.isfinite(a["ticks"][-1]["plant"]))


RACE_EVENT_TICKS = TK.RACE_EVENT_TICKS                                   # the host replay's: 12 14 11 17 13 15 13 18 11 14 12 17
RACE_T = 18 + 1 + 6                                                      # 6 racing ticks beyond the last event


def test_mixed_race_through_the_lap_events():
    """12 vehicles on four tracks of different lengths (oval 13 m, L shape 19.23 m, 3110 19.27 m, oval x 1.3 16.9 m; vehicle b on
    entry b mod 4), started RACE_DIST[b] = 0.40 0.46 0.52 0.58 0.43 0.49 0.56 0.61 0.38 0.47 0.53 0.59 m before the end of their
    own lap with HalfTrack = 1.  The starts were chosen beforehand with the host replay (tests/_race_ref.py, per track), whose lap
    events fall on ticks RACE_EVENT_TICKS: after the 9 seed ticks, seven different ticks, three vehicles per track.  The race runs 6
    racing ticks beyond the last event.  Every vehicle equals, bit for bit, the same vehicle of a 12-vehicle race on handles of its
    track: plant, commands, measurement, phase, lap, lap steps, controller and planner statuses and iteration counts, both
    controllers' predictions, the recorder's records and lap statistics.  Asserted, so that it cannot pass empty: the device's
    event ticks are the replay's, and every track has at least two vehicles that passed their event inside the window and are alive at
    the end."""
    maps, of = TK.race_palette(), TK.cycle(TK.RACE_B, 4)
    plant0 = TK.race_starts(maps, of)
    got = race_run(plant0, RACE_T, bind=(maps, of))
    phase = np.array([o["phase"] for o in got["ticks"]])                    # [T, B]
    event = np.array([int(np.argmax(phase[:, b] == 1)) if np.any(phase[:, b] == 1) else -1 for b in range(TK.RACE_B)])
    print("event ticks: device %s, replay %s" % (event.tolist(), list(RACE_EVENT_TICKS)))
    assert np.array_equal(event, RACE_EVENT_TICKS)
    for t_, idx in TK.groups(of):
        ref = race_run(plant0, RACE_T, mp=maps[t_])
        race_same(got, ref, idx, "track %d" % t_)
    last = got["ticks"][-1]
    alive = (last["phase"] == 1) & np.all(np.isfinite(last["plant"]), axis=1) & (last["lap"] == 1)
    for t_, idx in TK.groups(of):
        assert alive[idx].sum() >= 2, (t_, last["phase"][idx])
    assert len(set(event.tolist())) >= 2 and np.all(got["lap_step"][:, 1] == 7 * event)
    assert np.all(last["plan_iters"] > 0)                                   # the planner has run for every vehicle


def test_handoff_on_a_bound_planner():
    """lpvmpc_handoff_batch on a bound planner handle (plan_pose: curvature and centre-line pose from each vehicle's track) over 3
    ticks, B = 67: SS, pose, the planner-rate signals and the resampled references are word for word those of the per-track
    handles; another B than the binding's is refused."""
    import lpvmpc
    from lpvmpc import workloads as W
    B = 67
    maps, of = TK.palette(), TK.cycle(B)
    w = TK.plan(B, 40, 8600, maps, of)
    mk = lambda tab: lpvmpc.BatchedSolver("planner", 40, 0.05, W.PLAN_Q, W.PLAN_R, W.PLAN_dR, L_cf=W.PLAN_L, track=tab)
    rng = np.random.default_rng(8601)
    xPred = np.concatenate([w["x0"][:, None, :], w["x0"][:, None, :] + rng.normal(0, 0.01, (B, 40, 5))], axis=1)
    SS0, pose0 = w["curv_s"].copy(), np.zeros((B, 3))
    for b in range(B):
        pose0[b] = PR.get_global_position(maps[of[b]].PointAndTangent, SS0[b, 0] % TK.lengths(maps)[of[b]], 0.0)

    def run(e, idx):
        SS, pose, out = SS0[idx].copy(), pose0[idx].copy(), []
        for _ in range(3):
            o = e.handoff(xPred[idx], SS, pose, want_sig=True)
            SS, pose = o["SS"], o["pose"]
            out.append(o)
        return out

    e = mk(None)
    e.set_tracks(maps, of)
    e.handoff_setup()
    got = run(e, np.arange(B))
    with pytest.raises(lpvmpc.LpvMpcError) as err:
        e.handoff(xPred[:5], SS0[:5], pose0[:5])
    assert err.value.code == lpvmpc._ffi.E_ARG and "lpvmpc_set_tracks" in str(err.value)
    e.close()
    assert np.all(np.isfinite(got[-1]["refs"]))
    for t_, idx in TK.groups(of):
        p = mk(maps[t_].PointAndTangent)
        p.handoff_setup()
        ref = run(p, idx)
        p.close()
        for a, r in zip(got, ref):
            for k in ("SS", "pose", "sig", "refs"):
                assert same(a[k][idx], r[k]), (t_, k)


def test_engine_starts_on_a_bound_handle():
    """The lap-0 fleet and the race start on bound handles through the most general entries only: lpvmpc_cl_init, _actuated and
    _vehicles and lpvmpc_race_init, _observed, _actuated and _vehicles refuse them with a message that names lpvmpc_cl_init_tyres /
    lpvmpc_race_init_tyres, which refuse another B than the binding's.  A race needs equal bindings on path, tt and planner: one or
    two bound handles, or bindings that differ in a table word, a width, a slack or an index, are refused.  The cascade refuses a
    bound handle.  Every refused start leaves the handles idle; lpvmpc_set_tracks is refused while the handle runs a fleet or race."""
    import lpvmpc
    from lpvmpc import workloads as W
    from tests.test_gpu_delayed_fleets import obs_cfg
    E_ARG = lpvmpc._ffi.E_ARG
    mp = lpvmpc.Map("L_shape", 0.2)
    B = 5
    of = np.zeros(B, np.int32)
    path, tt, plan = race_engines(mp)
    plant0 = np.tile(np.array([0.01, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0]), (B, 1))

    def refused(call, word="lpvmpc_set_tracks"):
        with pytest.raises(lpvmpc.LpvMpcError) as err:
            call()
        assert err.value.code == E_ARG and word in str(err.value), str(err.value)

    path.set_tracks([mp], of)
    refused(lambda: path.cl_init(plant0, mp.halfWidth, mp.slack), "lpvmpc_cl_init_tyres")
    refused(lambda: path.cl_init(plant0, mp.halfWidth, mp.slack, actuator=lpvmpc._ffi.default_actuator_config()), "lpvmpc_cl_init_tyres")
    refused(lambda: path.cl_init(plant0, mp.halfWidth, mp.slack, plant_params="nominal"), "lpvmpc_cl_init_tyres")
    refused(lambda: path.cl_init(plant0[:4], mp.halfWidth, mp.slack, tyre_params="linear"))          # another B than the binding's
    refused(lambda: path.cascade_init(plan, plant0, np.zeros((B, 2)), np.zeros((B, 20, 2))))
    refused(lambda: path.race_init(tt, plan, plant0, tyre_params="linear"), "or none")               # one of three bound
    tt.set_tracks([mp], of)
    refused(lambda: path.race_init(tt, plan, plant0, tyre_params="linear"), "or none")               # two of three
    plan.set_tracks([mp], of)
    act = lpvmpc._ffi.default_actuator_config()
    for kw in ({}, dict(estimator=obs_cfg()), dict(actuator=act), dict(plant_params="nominal")):      # all three, not the general entry
        refused(lambda: path.race_init(tt, plan, plant0, **kw), "lpvmpc_race_init_tyres")
    refused(lambda: path.race_init(tt, plan, plant0[:4], tyre_params="linear"))                      # another B than the binding's
    refused(lambda: path.cascade_init(plan, plant0, np.zeros((B, 2)), np.zeros((B, 20, 2))))
    # unequal bindings: a table word, a half width, a slack, an index, the palette size
    segs = lpvmpc.track.TRACK_SPECS["L_shape"][0]
    moved = lpvmpc.Map.from_segments(segs, mp.halfWidth, mp.slack)
    moved.PointAndTangent[2, 0] += 1e-9
    of2 = of.copy(); of2[3] = 1
    pair = [mp, lpvmpc.Map("oval", 0.2)]
    for what, common, odd in (("table", ([mp], of), ([moved], of)),
                              ("width", ([mp], of), ([lpvmpc.Map.from_segments(segs, mp.halfWidth + 0.01, mp.slack)], of)),
                              ("slack", ([mp], of), ([lpvmpc.Map.from_segments(segs, mp.halfWidth, mp.slack + 0.01)], of)),
                              ("index", (pair, of), (pair, of2)), ("size", ([mp], of), (pair, of))):
        for k in range(3):
            for j, e in enumerate((path, tt, plan)):
                e.set_tracks(*(odd if j == k else common))
            refused(lambda: path.race_init(tt, plan, plant0, tyre_params="linear"), "differ")
    for e in (path, tt, plan):
        e.set_tracks([mp], of)
    with pytest.raises(lpvmpc.LpvMpcError):
        path.race_tick(1)                                         # nothing was started
    path.race_init(tt, plan, plant0, tyre_params="linear")        # equal bindings, the general entry: the race starts
    for e in (path, tt, plan):
        refused(lambda: e.set_tracks([mp, mp], of), "race")
    path.race_tick(2)
    assert np.all(np.isfinite(path.race_read()["plant"]))
    path.cl_release()
    for e in (tt, plan):
        e.set_tracks(None, None)
    path.cl_init(plant0, 0.0, 0.0, tyre_params="linear")          # the general entry starts the bound fleet, which refuses a new binding
    refused(lambda: path.set_tracks([mp, mp], of), "fleet")
    path.cl_tick(2)
    assert np.all(np.isin(path.cl_read()["status"], (1, 2))) and np.all(path.cl_read()["local"][:, 4] < 9999)
    path.cl_release()
    path.set_tracks(None, None)
    assert path.tracks_read() is None
    for e in (path, tt, plan):
        e.close()
