"""GPU: per-vehicle tunings (lpvmpc_set_tunings, lpvmpc_tunings_read; include/lpvmpc.h, "Per-vehicle tunings").  A handle with
tuning rows bound builds instance b's QP with row b:
  1. against the oracle with each instance's row (tests/_tunings.py: rows, batches, per-row oracle), on every kernel family;
  2. word for word against the per-handle path that exists without a binding -- one plain handle per row, created with the row's
     weights and limits -- on every solve route, deferral included: a parked instance finishes with its own row;
  3. the handle's own row bound to every instance changes no output word (stand-alone calls, lap-0 fleet, cascade, race);
  4. interleaved rows in a fleet and a race equal, bit for bit, the uniform fleets and races of handles created with each row,
     and a race split in two halves with the rows split likewise equals the whole;
  5. weight-only rows against the host replay with per-vehicle weights (tests/_tuned_race_ref.py);
  6. refusals; 7. lifecycle and two handles on two threads; 8. a 1024-vehicle recorded race of sampled tt tunings."""
import ctypes as C
import threading

import numpy as np
import pytest

from tests import _race_observer_ref as RO
from tests import _tunings as TU
from tests.test_gpu_delayed_fleets import KV, close, ctrl, engines, lshape, same
from tests.test_gpu_model_params import _dev_solve
from tests.test_gpu_plant_params import RACE_KEYS, _race_same

pytestmark = pytest.mark.gpu

OUT_KEYS = ("status", "iters", "polish", "xPred", "uPred", "resid")


def engine(w, variant=0, **settings):
    import lpvmpc
    e = lpvmpc.BatchedSolver(w["kind"], w["N"], w["dt"], w["Q"], w["R"], w["dR"], L_cf=w["L_cf"], track=w["track"], steering_delay=TU.delay_of(w),
                             **settings)
    e.set_option("kernel_variant", variant)
    return e


def plain(w, row, variant=0):
    e = TU.plain_engine(w, row)
    e.set_option("kernel_variant", variant)
    return e


def mixed_rows(name, shift=0):
    return TU.interleaved(TU.batch(name)[1]["x0"].shape[0], TU.rows4(name), shift)


# ---- 1. against the per-row oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,variant", [("ctrl8", 0), ("ctrl13", 0), ("ctrl20", 0), ("ctrl20", 3), ("ctrl20", 9), ("ctrl20d3", 0), ("plan20", 0),
                                          ("plan20", 9), ("plan30", 0), ("plan30", 4), ("plan40", 0), ("plan40", 6)])
def test_interleaved_rows_against_the_per_row_oracle(name, variant):
    """The four rows of the batch interleaved and bound: statuses, iteration counts and solutions against tick_batch_qp with each
    instance's weights and limits, under tests/_tolerance.py check_batch as it stands (per row group, with the group's limits)."""
    kind, w = TU.batch(name)
    rows = mixed_rows(name)
    e = engine(w, variant)
    e.set_tunings(rows)
    out = TU.solve(e, w)
    e.close()
    ref = TU.oracle(name)
    assert not np.any(ref["status"] == -10)                       # (tests/test_tunings_host.py: the oracle answers every instance)
    total = TU.check_interleaved(name, out)
    print("%s variant %d: iters %d..%d statuses %s %s" % (name, variant, out["iters"].min(), out["iters"].max(),
                                                          dict(zip(*map(list, np.unique(out["status"], return_counts=True)))), total))
    assert set(total) == {"A", "B", "C", "D", "no_solution", "flips"}


# ---- 2. word for word against one plain handle per row ----------------------------------------------------------------------------
def with_seed_inputs(w, seed=9400):
    """The batch with trajectories and steering angles for the seed-mode linearisation (drawn once for the whole batch: a
    sub-batch takes its instances' slices)."""
    from tests.test_gpu_model_params import seed_inputs
    xx, delta = seed_inputs(w, w["kind"], seed)
    return dict(w, seed_xx=xx, seed_delta=delta)


def run_route(e, w, route):
    """Every output of one route as a list of dicts (one per tick)."""
    if route == "AB":
        _, A, Bm = e.lpv(w["x0"], w["u_prev"], w["vel_ref"], w["curv_s"], cf_new=w["cf_new"], lap=w["lap"])
        return [e.solve_AB(w["x0"], A, Bm, w["vel_ref"], w["u_old"], w["max_ey"])]
    if route == "seed":
        A, Bm = e.estimate_abc(w["seed_xx"], w["seed_delta"])
        return [e.solve_AB(w["x0"], A, Bm, w["vel_ref"], w["u_old"], w["max_ey"])]
    if route == "masked":
        return [e.solve_batch_masked(w["active"], w["x0"], w["u_prev"], w["vel_ref"], w["curv_s"], w["u_old"], w["max_ey"], w["cf_new"], w["lap"])]
    if route == "dev":
        return [_dev_solve(e, w)]
    if route == "warm":
        e.set_option("warm_start", 1)
        return [TU.solve(e, w) for _ in range(2)]
    if route in ("defer", "tail"):
        B = w["x0"].shape[0]
        e.reserve(B)
        e.set_option("defer_after", 50); e.set_option("defer_budget", -1); e.set_option("defer_pool", 2 * B)
        e.set_option("defer_tail", 0 if route == "defer" else 1)
        return [TU.solve(e, w)]
    return [TU.solve(e, w)]


def compare_routes(name, route, variant=0):
    """The bound handle on one route against the plain handles of its rows on their sub-batches.  "defer" (defer_tail 0: the same
    kernel continues a parked instance from its image) is held, word for word, to the plain handles' UNDEFERRED solves; "tail" (the
    whole-CU tail kernel finishes them) to the plain handles on the same route at the deferred path's own bar
    (tests/test_gpu_model_params.py: status, iterations and polish equal, polished points 1e-7, others 1e-6)."""
    kind, w = TU.batch(name)
    B = w["x0"].shape[0]
    rows = mixed_rows(name)
    w = dict(with_seed_inputs(w), active=(np.arange(B) % 3 != 0).astype(np.int32))
    e = engine(w, variant)
    e.set_tunings(rows)
    got = run_route(e, w, route)
    if route in ("defer", "tail"):
        assert e.defer_stats()[0] >= 1, (name, route)                 # (every batch has instances beyond 50 iterations)
    e.close()
    worst = 0.0
    for row, idx in TU.groups(rows):
        g = TU.sub_batch(w, idx)
        p = plain(g, row, variant)
        ref = run_route(p, g, "plain" if route == "defer" else route)
        p.close()
        for a, r in zip(got, ref):
            on = g["active"] != 0 if route == "masked" else np.ones(len(idx), bool)
            for k in ("status", "iters", "polish"):
                assert np.array_equal(a[k][idx][on], r[k][on]), (name, route, variant, k)
            if route == "tail":
                pol = (r["status"] == 1) & (r["polish"] == 1)
                for k in ("xPred", "uPred"):
                    assert np.array_equal(np.isnan(a[k][idx]), np.isnan(r[k])), (name, k)
                    d = np.nan_to_num(np.abs(a[k][idx] - r[k]).reshape(len(idx), -1)).max(axis=1)
                    assert np.all(d[pol] <= 1e-7) and np.all(d[~pol] <= 1e-6), (name, k, float(d.max()))
                    worst = max(worst, float(d.max()))
            else:
                for k in ("xPred", "uPred", "resid"):
                    assert same(a[k][idx][on], r[k][on]), (name, route, variant, k)
    return worst


@pytest.mark.parametrize("name", TU.NAMES)
def test_bound_handle_equals_one_handle_per_row(name):
    """xPred, uPred, status, iterations, polish flag and residuals of the bound handle equal, word for word, those of the plain
    handles BatchedSolver(Q=, R=, dR=, L_cf=, ctrl_* / plan_* = the row's) on their sub-batches: solve, solve_AB with the LPV blocks
    and with the seed-mode blocks, the device-pointer call, a masked call, warm start 1 over two ticks, deferral at 50 iterations
    with defer_tail 0; with the tail kernel the deferred path's own bar."""
    for route in ("plain", "AB", "seed", "dev", "masked", "warm", "defer"):
        compare_routes(name, route)
    worst = compare_routes(name, "tail")
    print("%s: every route word for word; tail kernel max difference %.2e" % (name, worst))


@pytest.mark.parametrize("name", ["ctrl20", "plan20"])
def test_parked_instances_finish_with_their_own_rows_as_riders(name):
    """The recipe of tests/test_gpu_deferral_riders.py (defer_after 50, defer_budget 50, defer_tail 0; two device-pointer calls on one
    stream, then the join) on a bound handle: call 1's parked instances continue as riders of call 2's launch -- whose new instances
    read OTHER rows of the table at the same time (the batch rolled by one instance, so instance b carries the data of b + 1 under
    row b) -- and every word of both calls equals the plain handles' undeferred solves: that file's bar, bit for bit."""
    import torch
    from tests.test_gpu_deferral_riders import PENDING, _dev_call, _host
    kind, w = TU.batch(name)
    B = w["x0"].shape[0]
    rows = mixed_rows(name)
    w2 = {k: (np.roll(v, -1, axis=0) if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == B and k != "track" else v) for k, v in w.items()}
    e = engine(w); e.reserve(B)
    e.set_tunings(rows)
    e.set_option("defer_pool", 2 * B); e.set_option("defer_after", 50); e.set_option("defer_budget", 50); e.set_option("defer_tail", 0)
    st = torch.cuda.Stream()
    keep1, o1 = _dev_call(torch, e, w, B, kind == "planner", stream=st)
    torch.cuda.synchronize()
    pending = _host(o1)["status"] == PENDING
    assert len({int(b) % 4 for b in np.nonzero(pending)[0]}) >= 2, np.nonzero(pending)[0]      # parked instances of more than one row
    keep2, o2 = _dev_call(torch, e, w2, B, kind == "planner", stream=st)
    e.join(st.cuda_stream); torch.cuda.synchronize()
    h1, h2 = _host(o1), _host(o2)
    parked = e.defer_stats()[0]
    e.close()
    assert parked >= int(pending.sum())
    for row, idx in TU.groups(rows):
        for ww, h in ((w, h1), (w2, h2)):
            g = TU.sub_batch(ww, idx)
            p = plain(g, row)
            r = _dev_solve(p, g)
            p.close()
            for k in OUT_KEYS:
                assert np.array_equal(h[k][idx], r[k], equal_nan=True), (name, k)


# ---- 3. the handle's own row changes nothing --------------------------------------------------------------------------------------
def own_rows(e, B):
    from lpvmpc import tuning
    return tuning.tuning_rows(B, e)


@pytest.mark.parametrize("name", TU.NAMES)
def test_own_row_changes_no_stand_alone_call(name):
    """The handle's own row bound to every instance: every word of solve and solve_AB equals the unbound handle's; other rows in
    between change them; after unbinding the handle equals a fresh one again."""
    kind, w = TU.batch(name)
    B = w["x0"].shape[0]
    w = with_seed_inputs(w)

    def everything(e):
        return [v for _, v in sorted(TU.solve(e, w).items())] + [v for r in run_route(e, w, "AB") + run_route(e, w, "seed") for _, v in sorted(r.items())]

    fresh = engine(w)
    want = everything(fresh)
    fresh.close()
    e = engine(w)
    assert e.tunings_read() is None
    rows = own_rows(e, B)
    assert same(rows, np.tile(TU.rows4(name)[0], (B, 1)))
    e.set_tunings(rows)
    assert same(e.tunings_read(), rows)
    for a, b in zip(everything(e), want):
        assert same(a, b), name
    e.set_tunings(mixed_rows(name))
    assert any(not same(a, b) for a, b in zip(everything(e), want))
    e.set_tunings(None)
    assert e.tunings_read() is None
    for a, b in zip(everything(e), want):
        assert same(a, b), name
    e.close()


def cl_run(mp, plant0, T, tun=None, row=None):
    """A lap-0 fleet of the path controller (or of the plain handle of ``row``) with ``tun`` bound; its read-back of every tick."""
    e = ctrl(mp) if row is None else fleet_engine(mp, "path", row)
    if tun is not None:
        e.set_tunings(tun if not isinstance(tun, str) else own_rows(e, plant0.shape[0]))
    e.cl_init(plant0, mp.halfWidth, mp.slack, q9_swap=True, n_sub=7)
    out = []
    for _ in range(T):
        e.cl_tick(1)
        out.append(e.cl_read())
    e.close()
    return out


def test_own_row_changes_no_lap0_fleet():
    mp = lshape()
    B, T = 32, 30
    plant0 = RO.grid_fleet(B, 3)
    a, b = cl_run(mp, plant0, T), cl_run(mp, plant0, T, tun="own")
    for t in range(T):
        for k in ("plant", "local", "cmd", "iters", "status"):
            assert same(a[t][k], b[t][k]), (t, k)


def test_own_row_changes_no_cascade():
    from tests._golden import load
    from tests.test_gpu_cascade import controller_tt, fleet_start, planner
    c = load("cascade")
    B, K = 8, 24
    plant0 = fleet_start(c, 5, B)
    runs = []
    for bind in (False, True):
        plan, mp = planner()
        plan.handoff_setup()
        e = controller_tt(mp)
        if bind:
            e.set_tunings(own_rows(e, B)); plan.set_tunings(own_rows(plan, B))
        e.cascade_init(plan, plant0, np.tile(c["cmd0"], (B, 1)), np.tile(c["uPred0"], (B, 1, 1)), lap0=1, half_width=mp.halfWidth,
                       slack=mp.slack, plan_max_ey=0.2, q9_swap=True)
        out = []
        for _ in range(K):
            e.cascade_tick(1)
            out.append(e.cascade_read())
        runs.append(out)
        close(e, plan)
    for t in range(K):
        assert sorted(runs[0][t]) == sorted(runs[1][t])
        for k in runs[0][t]:
            assert same(runs[0][t][k], runs[1][t][k]), (t, k)


# the three handles of a race (tests/test_gpu_delayed_fleets.py engines): role -> (kind, N, dt, weights)
def _roles():
    from lpvmpc import workloads as W
    return {"path": ("controller", 20, 1 / 30.0, W.CTRL_TUNINGS["path"] + (None,)), "tt": ("controller", 20, 1 / 30.0, W.CTRL_TUNINGS["race"] + (None,)),
            "plan": ("planner", 40, 0.05, (W.PLAN_Q, W.PLAN_R, W.PLAN_dR, W.PLAN_L))}


def host_engine(mp, role):
    """kind and configuration of a race handle, without a handle (for tuning.tuning_rows / sample_tunings)."""
    from lpvmpc.api import build_config
    kind, N, dt, (Q, R, dR, Lc) = _roles()[role]
    e = TU.HostEngine.__new__(TU.HostEngine)
    e.cfg = build_config(kind, N, dt, Q, R, dR, L_cf=Lc, track=mp.PointAndTangent)
    e.kind = e.cfg.kind
    return e


def fleet_engine(mp, role, row):
    """The plain handle of a race role created with ``row``."""
    import lpvmpc
    from lpvmpc import tuning
    kind, N, dt, _ = _roles()[role]
    e = lpvmpc.BatchedSolver(kind, N, dt, track=mp.PointAndTangent, **tuning.engine_kwargs(kind, row))
    e.set_option("kernel_variant", KV)
    if kind == "planner":
        e.handoff_setup()
    return e


def fleet_rows(mp, role, weights_only=False):
    """[4, 64] rows of a race handle: its own; every diagonal weight scaled (Q x 1.2, R x 0.9, dR x 0.8, L_cf x 1.1); tighter limits
    that the lap-0 speed of 1 m/s and the racing speeds leave feasible (controller delta_max 0.2, a_max 1.5, a_min_abs 0.8; planner
    epsi box +-0.6, input boxes [-0.2, -0.6] .. [0.2, 1.6]), or with weights_only dR x 1.25; a sampled row (tuning.sample_tunings,
    seed 17: weights +-30 %, and without weights_only delta_max / umax +-10 %)."""
    from lpvmpc import tuning
    h = host_engine(mp, role)
    own = tuning.tuning_rows(1, h)[0]
    d = tuning.split_row(h.kind, own)
    planner = role == "plan"
    scaled = dict(Q=d["Q"] * 1.2, R=d["R"] * 0.9, dR=d["dR"] * 0.8)
    if planner:
        scaled["L_cf"] = d["L_cf"] * 1.1
    if weights_only:
        lim, spread = dict(dR=d["dR"] * 1.25), None
    elif planner:
        xmin, xmax = d["xmin"].copy(), d["xmax"].copy()
        xmin[4], xmax[4] = -0.6, 0.6
        lim, spread = dict(xmin=xmin, xmax=xmax, umin=[-0.2, -0.6], umax=[0.2, 1.6]), dict(tuning.DEFAULT_SPREAD, umax=0.1)
    else:
        lim = dict(delta_max=0.2, a_max=1.5, a_min_abs=0.8)
        spread = dict({k: v for k, v in tuning.DEFAULT_SPREAD.items() if k != "L_cf"}, delta_max=0.1)
    return np.stack([own, tuning.tuning_rows(1, h, **scaled)[0], tuning.tuning_rows(1, h, **lim)[0], tuning.sample_tunings(1, 17, spread, h)[0]])


def race_run(mp, plant0, T, tun=None, rows=None, laps=2, **kw):
    """tun: tables for (path, tt, planner) or "own"; rows: one row per role -- the three handles are CREATED with them."""
    if rows is None:
        es = engines(mp)
    else:
        es = tuple(fleet_engine(mp, role, r) for role, r in zip(("path", "tt", "plan"), rows))
    if tun is not None:
        for e, r in zip(es, (None,) * 3 if tun == "own" else tun):
            e.set_tunings(own_rows(e, plant0.shape[0]) if r is None else r)
    path, tt, plan = es
    path.race_init(tt, plan, plant0, laps=laps, half_width=mp.halfWidth, slack=mp.slack, **kw)
    out = []
    for _ in range(T):
        path.race_tick(1)
        out.append(path.race_read())
    last = dict(zip(("path_uPred", "tt_uPred"), path.race_predictions()))
    last.update(zip(("lap_step", "alive"), path.race_laps()))
    out.append(last)
    close(path, tt, plan)
    return out


def test_own_row_changes_no_race():
    """24 vehicles, 90 ticks from the start line, through the lap event: every word read back equals the unbound race's."""
    mp = lshape()
    B, T = 24, 90
    plant0 = RO.start_line_fleet(mp.PointAndTangent, B, 7)
    a = race_run(mp, plant0, T, half_track0=1)
    b = race_run(mp, plant0, T, tun="own", half_track0=1)
    _race_same(a, b, T, RACE_KEYS)
    assert np.any(a[T - 1]["phase"] >= 1)


# ---- 4. interleaved rows in a fleet and a race ------------------------------------------------------------------------------------
def test_interleaved_rows_equal_uniform_lap0_fleets():
    """A lap-0 fleet (40 ticks) with four rows interleaved on the path handle equals, vehicle for vehicle and bit for bit, the four
    fleets of a handle CREATED with that row (nothing bound)."""
    mp = lshape()
    B, T = 16, 40
    plant0 = RO.grid_fleet(B, 8)
    uni = fleet_rows(mp, "path")
    m = cl_run(mp, plant0, T, tun=TU.interleaved(B, uni))
    for k in range(4):
        u = cl_run(mp, plant0, T, row=uni[k])
        v = np.arange(B) % 4 == k
        for t in range(T):
            for key in ("plant", "local", "cmd", "iters", "status"):
                assert same(m[t][key][v], u[t][key][v]), (k, t, key)
    assert not same(m[T - 1]["cmd"][0], m[T - 1]["cmd"][1])


def test_interleaved_rows_equal_uniform_races_and_halves():
    """A race of 24 vehicles over 120 ticks, lap events spread out, rows interleaved on the path, tt and planner handles: equal, per
    vehicle and bit for bit, to the four uniform races whose three handles were created with those rows (nothing bound) -- through the
    lap event and the racing phase; the race split into two halves with the rows sliced likewise equals the whole; RaceFleet binds
    the same tables."""
    import lpvmpc
    mp = lshape()
    B, T = 24, 120
    plant0 = RO.start_line_fleet(mp.PointAndTangent, B, 13, 0.8, 0.97)
    uni = [fleet_rows(mp, role) for role in ("path", "tt", "plan")]
    tun = tuple(TU.interleaved(B, u) for u in uni)
    f = lpvmpc.RaceFleet(mp, plant0, laps=2, half_track0=1, path_tunings=tun[0], tt_tunings=tun[1], plan_tunings=tun[2])
    for got, want in zip(f.tunings(), tun):
        assert same(got, want)
    f.close()
    whole = race_run(mp, plant0, T, tun=tun, half_track0=1)
    ev = [int(np.argmax([r["phase"][v] >= 1 for r in whole[:T]])) for v in range(B)]
    assert len(set(ev)) >= 4, ev
    assert np.sum(np.isin(whole[T - 1]["phase"], (1, 2))) >= 4                    # the racing phase is compared, not only lost cars
    for k in range(4):
        u = race_run(mp, plant0, T, rows=[x[k] for x in uni], half_track0=1)
        _race_same(whole, u, T, RACE_KEYS, np.arange(B) % 4 == k)
    h = B // 2
    lo = race_run(mp, plant0[:h], T, tun=tuple(x[:h] for x in tun), half_track0=1)
    hi = race_run(mp, plant0[h:], T, tun=tuple(x[h:] for x in tun), half_track0=1)
    for t in range(T):
        for key in RACE_KEYS:
            assert same(whole[t][key], np.concatenate([lo[t][key], hi[t][key]])), (t, key)


# ---- 5. weight-only rows against the host replay ----------------------------------------------------------------------------------
def _weights(role, row):
    from lpvmpc import tuning
    d = tuning.split_row("planner" if role == "plan" else "controller", row)
    return (d["Q"], d["R"], d["dR"]) + ((d["L_cf"],) if role == "plan" else ())


def test_weight_rows_in_a_lap0_fleet_match_the_tuned_host_replay():
    """8 vehicles, weight-only rows interleaved on the path handle, against TunedRaceRef with each vehicle's weights over 40 ticks:
    the bars of the existing lap-0 replays (2e-6, identical iteration counts and statuses)."""
    from tests._tuned_race_ref import TunedRaceRef
    mp = lshape()
    B, T = 8, 40
    plant0 = RO.grid_fleet(B, 41)
    rows = TU.interleaved(B, fleet_rows(mp, "path", weights_only=True))
    e = ctrl(mp)
    e.set_tunings(rows)
    e.cl_init(plant0, mp.halfWidth, mp.slack, q9_swap=True, n_sub=7)
    ref = TunedRaceRef(mp.PointAndTangent, plant0, path_weights=[_weights("path", r) for r in rows], laps=1, half_width=mp.halfWidth, slack=mp.slack)
    worst = 0.0
    for t in range(T):
        e.cl_tick(1); ref.tick()
        o = e.cl_read()
        assert np.all(ref.phase == 0), t
        assert np.array_equal(o["status"], ref.status) and np.array_equal(o["iters"], ref.iters), t
        worst = max(worst, float(np.max(np.abs(o["plant"] - ref.plant))), float(np.max(np.abs(o["local"] - ref.local))),
                    float(np.max(np.abs(o["cmd"] - ref.cmd))))
    e.close()
    print("weight rows, lap-0 fleet against the tuned host replay: B=%d, %d ticks, max difference %.2e" % (B, T, worst))
    assert worst <= 2e-6
    assert len({tuple(c) for c in np.round(o["cmd"][:4], 9)}) == 4             # the four rows drive differently


def test_weight_rows_in_a_race_match_the_tuned_host_replay():
    """12 vehicles from the start line, weight-only rows on all three handles, 60 ticks through the lap event, against TunedRaceRef:
    the bars of test_gpu_race.py test_mixed_fleet_matches_the_host_replay -- every vehicle's event tick equals the replay's, and its
    phase for as long as the two trajectories agree to 2e-2 (on at least a quarter of the fleet to the end)."""
    from tests._tuned_race_ref import TunedRaceRef
    mp = lshape()
    B, T = 12, 60
    plant0 = RO.start_line_fleet(mp.PointAndTangent, B, 7)
    tun = tuple(TU.interleaved(B, fleet_rows(mp, role, weights_only=True)) for role in ("path", "tt", "plan"))
    path, tt, plan = engines(mp)
    for e, r in zip((path, tt, plan), tun):
        e.set_tunings(r)
    path.race_init(tt, plan, plant0, half_track0=1, laps=3, half_width=mp.halfWidth, slack=mp.slack)
    ref = TunedRaceRef(mp.PointAndTangent, plant0, path_weights=[_weights("path", r) for r in tun[0]], tt_weights=[_weights("tt", r) for r in tun[1]],
                       plan_weights=[_weights("plan", r) for r in tun[2]], half_track0=1, laps=3, half_width=mp.halfWidth, slack=mp.slack)
    apart = np.zeros(B, bool)
    dev_phase = []
    for t in range(T):
        path.race_tick(1); ref.tick()
        o = path.race_read()
        d = np.max(np.abs(o["plant"] - ref.plant), axis=1)
        apart |= ~((o["phase"] == 3) & (ref.phase == 3)) & ~(d <= 2e-2)
        assert np.array_equal(o["phase"][~apart], ref.phase[~apart]), t
        dev_phase.append(o["phase"].copy())
    close(path, tt, plan)
    dev_phase = np.array(dev_phase)
    ev_dev = [int(np.argmax(dev_phase[:, b] >= 1)) if np.any(dev_phase[:, b] >= 1) else -1 for b in range(B)]
    print("weight rows, race against the tuned host replay: events", ev_dev, "apart", int(apart.sum()))
    assert ev_dev == [int(x) for x in ref.event_tick]
    assert sum(x >= 0 for x in ev_dev) >= 4
    assert np.sum(~apart) >= B // 4, int(np.sum(~apart))


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals():
    """Each refused call returns LPVMPC_E_ARG and leaves the binding and the next solve unchanged."""
    import lpvmpc
    from lpvmpc import _ffi
    for name, bad_words in (("ctrl20", ((0, 7, np.nan, "Q"), (1, 37, np.inf, "R"), (2, 50, np.nan, "NaN limit"), (3, 48, 6.0, "vx_min > max_vel"),
                                        (4, 50, -0.1, "delta_max < 0"), (5, 51, -2.0, "a_max < -a_min_abs"))),
                            ("plan30", ((0, 43, np.nan, "L_cf"), (1, 58, 0.3, "umin > umax"), (2, 50, 3.0, "xmin > xmax"), (3, 61, np.nan, "NaN limit")))):
        kind, w = TU.batch(name)
        B = w["x0"].shape[0]
        rows = mixed_rows(name)
        e = engine(w)
        lib = e._lib
        e.set_tunings(rows)
        before = TU.solve(e, w)

        def refused(rc):
            assert rc == _ffi.E_ARG, rc
            assert same(e.tunings_read(), rows)
            after = TU.solve(e, w)
            for k in before:
                assert same(before[k], after[k]), k

        for b, i, v, what in bad_words:
            bad = rows.copy(); bad[b, i] = v
            refused(lib.lpvmpc_set_tunings(e._h, B, _ffi.ptr(bad)))
            msg = lib.lpvmpc_last_error(e._h).decode()
            assert "row %d" % b in msg and what in msg, msg
        refused(lib.lpvmpc_set_tunings(e._h, -1, _ffi.ptr(rows)))
        refused(lib.lpvmpc_set_tunings(e._h, B, None))
        ok = rows.copy(); ok[0, 63] = np.nan; ok[1, 51 if kind == "planner" else 47] = np.nan       # ignored words are stored as set
        e.set_tunings(ok)
        assert same(e.tunings_read(), ok)
        after = TU.solve(e, w)
        for k in before:
            assert same(before[k], after[k]), k
        e.set_tunings(rows)
        # another batch size: refused before anything is launched, no output word written, whatever the route
        sub = TU.sub_batch(w, np.arange(B - 3))
        _, A, Bm = e.lpv(sub["x0"], sub["u_prev"], sub["vel_ref"], sub["curv_s"], cf_new=sub["cf_new"], lap=sub["lap"])
        for call in (lambda: TU.solve(e, sub), lambda: e.solve_AB(sub["x0"], A, Bm, sub["vel_ref"], sub["u_old"], sub["max_ey"]),
                     lambda: e.solve_batch_masked(np.ones(B - 3, np.int32), sub["x0"], sub["u_prev"], sub["vel_ref"], sub["curv_s"], sub["u_old"], sub["max_ey"]),
                     lambda: _dev_solve(e, sub)):
            with pytest.raises(lpvmpc.LpvMpcError) as err:
                call()
            assert err.value.code == _ffi.E_ARG
        n = B - 3
        N, nx = int(w["N"]), (6 if kind == "controller" else 5)
        xP, uP = np.full((n, N + 1, nx), -7.0), np.full((n, N, 2), -7.0)
        st, it = np.full(n, 99, np.int32), np.full(n, 99, np.int32)
        p = lambda a: None if a is None else _ffi.ptr(np.ascontiguousarray(a, np.float64))
        rc = lib.lpvmpc_solve_batch(e._h, n, p(sub["x0"]), p(sub["u_prev"]), p(sub["vel_ref"]), p(sub["curv_s"]), p(sub["u_old"]), p(sub["max_ey"]),
                                    C.c_double(sub["cf_new"]), int(sub["lap"]), _ffi.ptr(xP), _ffi.ptr(uP), _ffi.ptr(st), _ffi.ptr(it), None, None)
        assert rc == _ffi.E_ARG and np.all(xP == -7.0) and np.all(uP == -7.0) and np.all(st == 99) and np.all(it == 99)
        refused(_ffi.E_ARG)
        e.close()
    # binding during a fleet; the engines check B at init
    mp = lshape()
    Bf = 8
    plant0 = RO.grid_fleet(Bf, 2)
    uni = fleet_rows(mp, "path")
    f = ctrl(mp)
    f.set_tunings(TU.interleaved(Bf + 1, uni))
    with pytest.raises(lpvmpc.LpvMpcError) as err:
        f.cl_init(plant0, mp.halfWidth, mp.slack)
    assert err.value.code == _ffi.E_ARG
    f.set_tunings(TU.interleaved(Bf, uni))
    f.cl_init(plant0, mp.halfWidth, mp.slack)
    f.cl_tick(12)
    for r in (TU.interleaved(Bf, uni, 1), None):
        with pytest.raises(lpvmpc.LpvMpcError) as err:
            f.set_tunings(r)
        assert err.value.code == _ffi.E_ARG
    assert same(f.tunings_read(), TU.interleaved(Bf, uni))
    f.cl_tick(1)
    f.cl_release()
    f.set_tunings(None)
    f.close()
    for i, role in enumerate(("path", "tt", "plan")):
        es = engines(mp)
        es[i].set_tunings(TU.interleaved(Bf + 2, fleet_rows(mp, role)))
        with pytest.raises(lpvmpc.LpvMpcError) as err:
            es[0].race_init(es[1], es[2], plant0, half_width=mp.halfWidth, slack=mp.slack)
        assert err.value.code == _ffi.E_ARG, role
        es[i].set_tunings(TU.interleaved(Bf, fleet_rows(mp, role)))
        es[0].race_init(es[1], es[2], plant0, half_width=mp.halfWidth, slack=mp.slack)
        es[0].race_tick(3)
        for x in es:                                                  # all three take part in the race: binding refused
            with pytest.raises(lpvmpc.LpvMpcError):
                x.set_tunings(None)
        close(*es)


# ---- 7. lifecycle and concurrency -------------------------------------------------------------------------------------------------
def test_lifecycle():
    """Read-back (NULL table: the batch size only); rebinding with another B; unbinding restores the unbound words; destroy after
    bind."""
    kind, w = TU.batch("ctrl8")
    B = w["x0"].shape[0]
    e = engine(w)
    n = C.c_int32(-1)
    assert e._lib.lpvmpc_tunings_read(e._h, C.byref(n), None) == 0 and n.value == 0
    unbound = TU.solve(e, w)
    rows = mixed_rows("ctrl8")
    e.set_tunings(rows)
    assert e._lib.lpvmpc_tunings_read(e._h, C.byref(n), None) == 0 and n.value == B
    assert same(e.tunings_read(), rows)
    full = TU.solve(e, w)
    assert not same(full["uPred"], unbound["uPred"])
    idx = np.arange(20, 20 + 4 * 9)                                   # a sub-batch that starts on row 0 again: 36 instances
    sub = TU.sub_batch(w, idx)
    e.set_tunings(rows[idx])
    assert e.tunings_read().shape == (36, 64)
    part = TU.solve(e, sub)
    for k in OUT_KEYS:
        assert same(part[k], full[k][idx]), k
    e.set_tunings(None)
    again = TU.solve(e, w)
    for k in OUT_KEYS:
        assert same(again[k], unbound[k]), k
    e.set_tunings(rows)
    e.close()                                                         # destroy after bind frees the table


def test_two_bound_handles_on_two_host_threads():
    """Two handles with different bindings, each on its own host thread: every result equals the serial run's, word for word."""
    kind, w = TU.batch("ctrl20")
    tables = (mixed_rows("ctrl20"), mixed_rows("ctrl20", shift=2))

    def run(rows):
        e = engine(w)
        e.set_tunings(rows)
        out = [TU.solve(e, w) for _ in range(3)]
        assert same(e.tunings_read(), rows)
        e.close()
        return out

    serial = [run(r) for r in tables]
    assert not same(serial[0][0]["uPred"], serial[1][0]["uPred"])
    results, errors = [None, None], []

    def worker(i):
        try:
            results[i] = run(tables[i])
        except Exception as e:          # noqa: BLE001 -- reported by the main thread
            errors.append(repr(e))

    th = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors
    for i in range(2):
        for a, b in zip(results[i], serial[i]):
            for k in a:
                assert same(a[k], b[k]), (i, k)


# ---- 8. a recorded race of sampled tunings ----------------------------------------------------------------------------------------
def test_recorded_race_of_sampled_tt_tunings_properties():
    """1024 vehicles, each with a sampled tt tuning (weights +-30 %, delta_max +-10 %), recorded, 30 ticks in three blocks: statuses
    are valid, a lost vehicle stays lost, a vehicle is alive as long as its plant state is finite, and the lap statistics of the
    vehicles still driving are finite."""
    import lpvmpc
    from lpvmpc import tuning
    mp = lshape()
    B = 1024
    plant0 = RO.start_line_fleet(mp.PointAndTangent, B, 3, 0.9, 0.97)
    rows = tuning.sample_tunings(B, 5, dict(Q=0.3, R=0.3, dR=0.3, delta_max=0.1), host_engine(mp, "tt"))
    f = lpvmpc.RaceFleet(mp, plant0, laps=2, half_track0=1, tt_tunings=rows)
    assert same(f.tunings()[1], rows) and f.tunings()[0] is None and f.tunings()[2] is None
    f.record(8)
    valid = {0} | (set(lpvmpc._ffi.STATUS_TEXT) - {-11})
    lost_prev, racing_prev = np.zeros(B, bool), np.zeros(B, bool)
    for block in range(3):
        f.run(10)
        o = f.state()
        finite = np.all(np.isfinite(o["plant"]), axis=1)
        lost = o["phase"] == 3
        assert not np.any(finite[lost]) and not np.any(~finite & ~lost & lost_prev)
        assert not np.any(lost_prev & ~lost)
        assert set(np.unique(o["status"]).tolist()) <= valid
        planned = racing_prev & np.isin(o["phase"], (1, 2))               # (the planner's report of a vehicle is written from its first planner tick on)
        assert set(np.unique(o["plan_status"][planned]).tolist()) <= valid
        lost_prev, racing_prev = lost, o["phase"] >= 1
    ls = f.lap_stats()
    driving = o["phase"] <= 1
    for k in ("sse_v", "sse_ey", "sse_epsi", "sum_vx"):
        assert np.all(np.isfinite(ls[k][driving])), k
    print("recorded race of sampled tt tunings: phases after 30 ticks %s, racing %d" %
          (dict(zip(*map(list, np.unique(o["phase"], return_counts=True)))), int(np.sum(o["phase"] == 1))))
    assert np.sum(o["phase"] == 1) >= 16                                  # the tt rows are in use
    f.close()
