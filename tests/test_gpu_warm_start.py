"""GPU: the opt-in warm start (lpvmpc_set_option "warm_start" 1 | 2) against the CPU oracle's warm-started run, on
every solve route of tests/test_gpu_settings.py (ROUTES: kernel variants, the tiled batch-size-selected forms, the deferral through
the host-array call), and the rule of whose state is valid.

Every other warm test of the suite compares the device with the device (variant 9 against 0, bound against plain handles, deferred
against plain): a shift rule wrong the same way in Solver::warm_start, which every kernel form shares, passes them all.  Here:

  a. three ticks per route and mode.  Both sides are fed identical inputs, derived from the ORACLE's previous tick
     (tests/_warm_ref.py next_inputs), so mode 1 is always tested on a new QP.  Tick 1 equals the cold oracle (check_batch).  On
     ticks 2 and 3 the ROBUST instances (tests/golden/warm_start/robust.npz: the oracle itself decides them the same way under both
     elimination orders and under warm starts perturbed by 1e-6) have the oracle's status, iteration count and polish flag and a
     solution in classes A-C of tests/_tolerance.py; the others are counted per route and held to "finite where the oracle is";
     the controllers once more on their default route with termination checked on every iteration and the polish off: iteration
     counts that resolve single iterations, and the ADMM iterate's reported residuals against the oracle's (check_resid);
  b. the warm ticks take fewer iterations than the cold oracle on the same data, on a controller and a planner workload;
  c. whose state is valid (include/lpvmpc.h, "warm_start"): an instance warm-starts from its own most recent solve since the option
     was last set, the workspace was (re)allocated or a fleet, cascade or race was initialised on the handle, and starts cold
     otherwise -- a masked call behind a reset, a masked call that leaves older state, a changed batch size, a previous tick without
     a solution.  "Cold" is word for word the result of a handle with warm_start 0.

Out of scope: warm starts inside the cascade (lpvmpc_cascade_init accepts them, nothing tests them) and in races (refused by
design, tests/test_gpu_race.py).  Class counts are printed per case (run with -s)."""
import numpy as np
import pytest

from oracle import osqp_ref as O
from tests import _tolerance as T
from tests import _warm_ref as WR
from tests import test_gpu_settings as G

pytestmark = pytest.mark.gpu

OUT_KEYS = ("xPred", "uPred", "status", "iters", "polish", "resid")


def engine(w, variant=0, defer=0, mode=0, **settings):
    import lpvmpc
    eng = lpvmpc.BatchedSolver(w["kind"], w["N"], w["dt"], w["Q"], w["R"], w["dR"], L_cf=w["L_cf"], track=w["track"],
                               steering_delay=WR.delay_of(w, w["kind"]), **settings)
    eng.set_option("kernel_variant", variant)
    if defer:
        B = w["x0"].shape[0]
        eng.reserve(B)
        eng.set_option("defer_after", defer); eng.set_option("defer_budget", -1); eng.set_option("defer_pool", B)
    if mode:
        eng.set_option("warm_start", mode)
    return eng


def run(eng, w, active=None, out=None):
    args = (w["x0"], w["u_prev"], w["vel_ref"], w["curv_s"], w["u_old"], w["max_ey"], w["cf_new"], w["lap"])
    return eng.solve(*args) if active is None else eng.solve_batch_masked(active, *args, out=out)


def rows(d, idx):
    """The instances ``idx`` (a bool mask) of a workload or result dict."""
    B = idx.size
    return {k: (v[idx] if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == B and k != "track" else v) for k, v in d.items()}


def same(a, b, idx=None):
    """Every output word of the instances ``idx`` equal (NaN equal to NaN); the first differing array's name, or None."""
    for k in OUT_KEYS:
        x, y = (a[k], b[k]) if idx is None else (a[k][idx], b[k][idx])
        if not np.array_equal(x, y, equal_nan=x.dtype.kind == "f"):
            return k
    return None


def check_warm_tick(tag, w, kind, out, ref, robust, settings=None):
    """Rule a. of a warm tick; returns the class counts of the robust instances."""
    ko, kr = WR.key(out), WR.key(ref)
    bad = np.nonzero(robust & (ko != kr).any(axis=1))[0]
    print("%s: %d robust, %d outside (of which %d differ from the oracle)" % (tag, int(robust.sum()), int((~robust).sum()),
                                                                             int((~robust & (ko != kr).any(axis=1)).sum())))
    assert bad.size == 0, (tag, "robust instances off the oracle's (status, iterations, polish)", [(int(j), ko[j].tolist(), kr[j].tolist()) for j in bad[:8]])
    for j in np.nonzero(~robust)[0]:
        if np.isfinite(ref["uPred"][j]).all() and np.isfinite(ref["xPred"][j]).all():
            assert np.isfinite(out["uPred"][j]).all() and np.isfinite(out["xPred"][j]).all(), (tag, int(j))
    return T.check_batch(rows(w, robust), kind, rows(out, robust), rows(ref, robust), allow_status_flip_at_max_iter=False, settings=settings)


# ---- a. every route, both modes, three ticks ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", WR.MODES)
@pytest.mark.parametrize("route", G.ROUTES, ids=lambda r: "%s-v%d%s%s" % (r[0], r[1], "-tiled" if r[2] else "", "-defer%d" % r[3] if r[3] else ""))
def test_warm_ticks_match_the_oracle_on_every_route(route, mode):
    name, variant, tile, defer = route
    eng = None
    try:
        for tick in (1, 2, 3):
            kind, w = WR.scenario_workload(name, mode, tick)
            ref = WR.scenario_ref(name, mode, tick)
            robust = WR.robust(name, mode, tick) if tick > 1 else None
            if tile:
                w, ref = G.tiled(w, G.TILE), G.tiled_ref(ref, G.TILE)
                robust = None if robust is None else np.concatenate([robust] * G.TILE)
            if eng is None:
                eng = engine(w, variant, defer, mode)
            out = run(eng, w)
            tag = "%s variant=%d tiled=%d defer=%d mode=%d tick %d" % (name, variant, tile, defer, mode, tick)
            if tick == 1:
                counts = T.check_batch(w, kind, out, ref)
            else:
                assert int((~robust).sum()) == (G.TILE if tile else 1) * int((~WR.robust(name, mode, tick)).sum())
                counts = check_warm_tick(tag, w, kind, out, ref, robust)
            G._report(tag, counts, out)
        if defer:
            assert eng.defer_stats()[0] >= 1, name
    finally:
        if eng is not None:
            eng.close()


@pytest.mark.parametrize("mode", WR.MODES)
@pytest.mark.parametrize("name", WR.FINE_NAMES)
def test_warm_ticks_at_single_iteration_resolution(name, mode):
    """The same three ticks on the default route of every controller workload with termination checked on EVERY iteration and the
    polish off (tests/_warm_ref.py FINE_SETTINGS), against the oracle under the same settings.  At the defaults an iteration count
    moves in blocks of 25 and the polish puts both sides on the optimum: a controller QP that a right and a wrong start both solve by
    the first check tells them apart on no instance -- with the dynamics duals left unshifted the matrix above still passes at
    N = 8, 10 and 13.  Here one iteration more or less shows, and the returned ADMM iterate's residuals (the resid words, which
    depend on the start continuously) are held to the oracle's at the bounds of tests/_tolerance.py check_resid."""
    st = WR.FINE_SETTINGS
    eng = None
    try:
        for tick in (1, 2, 3):
            kind, w = WR.scenario_workload(name, mode, tick, WR.FINE_CASE)
            ref = WR.scenario_ref(name, mode, tick, case=WR.FINE_CASE)
            if eng is None:
                eng = engine(w, 0, 0, mode, **st)
            out = run(eng, w)
            tag = "%s fine mode=%d tick %d" % (name, mode, tick)
            if tick == 1:
                counts = T.check_batch(w, kind, out, ref, settings=st)
            else:
                counts = check_warm_tick(tag, w, kind, out, ref, WR.robust(name, mode, tick, WR.FINE_CASE), settings=st)
                assert len(np.unique(ref["iters"])) >= 4, np.unique(ref["iters"])           # the counts do resolve single iterations
            rep = T.check_resid(w, kind, out, ref, yard=T.RESID_BOUNDS, settings=st, qps=WR.scenario_qps(name, mode, tick, WR.FINE_CASE))
            if tick > 1:
                assert not set(rep["left_out"]) & set(np.nonzero(WR.robust(name, mode, tick, WR.FINE_CASE))[0].tolist())
            G._report(tag, counts, out)
            print("%s resid: %s worst %s" % (tag, rep["counts"], {"%s/%s" % k: "%.1e" % v for k, v in rep["worst"].items()}))
    finally:
        if eng is not None:
            eng.close()


# ---- b. the state is used -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", WR.MODES)
def test_warm_ticks_take_fewer_iterations_than_cold(mode):
    """Summed over the two warm ticks, the device's mean iteration count on the robust instances with a solution is below the cold
    oracle's on the same data, on at least one controller and one planner workload.  (Not on every one: a planner QP that runs
    hundreds of iterations from the previous solution gains little, and shifted -- mode 2 -- most planner workloads lose; the
    figures are printed.)"""
    fewer = {"controller": 0, "planner": 0}
    for name in ("ctrl20", "ctrl20d3", "plan20", "plan25"):
        eng = None
        warm = cold = 0.0
        try:
            for tick in (1, 2, 3):
                kind, w = WR.scenario_workload(name, mode, tick)
                if eng is None:
                    eng = engine(w, 0, 0, mode)
                out = run(eng, w)
                if tick > 1:
                    c = WR.scenario_ref(name, mode, tick, cold=True)
                    idx = WR.robust(name, mode, tick) & WR.has_solution(out) & WR.has_solution(c)
                    warm += float(out["iters"][idx].mean()); cold += float(c["iters"][idx].mean())
        finally:
            if eng is not None:
                eng.close()
        print("%s mode %d: mean iterations over ticks 2 + 3, warm device %.1f, cold oracle %.1f" % (name, mode, warm, cold))
        fewer[kind] += warm < cold
    assert fewer["controller"] >= 1 and fewer["planner"] >= 1, fewer


# ---- c. whose state is valid ----------------------------------------------------------------------------------------------------
def _mask(B):
    """Every third instance inactive."""
    return (np.arange(B) % 3 != 2).astype(np.int32)


@pytest.mark.parametrize("mode", WR.MODES)
def test_reset_then_masked_call_starts_the_inactive_instances_cold(mode):
    """Warm on; plain call A; set_option("warm_start") again -- a fresh start; masked call B (every third instance inactive); plain
    call C.  B is cold on its instances.  In C the instances inactive in B are COLD, word for word a warm_start 0 handle's (not
    started from A's state, which the reset discarded), and the active ones follow the oracle warm-started from its B."""
    name = "ctrl20"
    kind, w1 = WR.scenario_workload(name, mode, 1)
    _, w2 = WR.scenario_workload(name, mode, 2)
    N, d, B = int(w1["N"]), WR.delay_of(w1, kind), w1["x0"].shape[0]
    rB = WR.scenario_ref(name, mode, 2, cold=True)
    w3 = WR.next_inputs(w2, kind, rB)
    active = _mask(B); on = active != 0
    eng, plain = engine(w1, mode=mode), engine(w1, mode=0)
    try:
        run(eng, w1)
        eng.set_option("warm_start", mode)
        oB = run(eng, w2, active)
        oC = run(eng, w3)
        cB, cC = run(plain, w2), run(plain, w3)
    finally:
        eng.close(); plain.close()
    assert same(oB, cB, on) is None, same(oB, cB, on)
    z, y = WR.warm_state(rB, kind, N, d, mode)
    z[~on] = 0.0; y[~on] = 0.0
    rC = O.tick_batch_qp(w3, kind, nthreads=WR.NTHREADS, warm=(z, y))
    # the test can tell: started from A's state, some inactive instance takes another number of iterations
    stale = O.tick_batch_qp(w3, kind, nthreads=WR.NTHREADS, warm=WR.warm_state(WR.scenario_ref(name, mode, 1), kind, N, d, mode))
    assert np.any(stale["iters"][~on] != rC["iters"][~on])
    assert np.any(rC["iters"][on] != cC["iters"][on])                  # and the active ones do start warm
    assert same(oC, cC, ~on) is None, ("inactive instances are not cold", same(oC, cC, ~on), oC["iters"][~on], cC["iters"][~on])
    assert np.array_equal(WR.key(oC), WR.key(rC)), np.nonzero((WR.key(oC) != WR.key(rC)).any(axis=1))[0]
    print("reset, masked, plain (mode %d): %s" % (mode, T.check_batch(w3, kind, oC, rC)))


def test_inactive_instances_keep_their_outputs_and_older_state():
    """Plain call A, masked call B, plain call C without a reset (mode 2): B leaves the inactive instances' output rows as they
    were, and in C such an instance starts from A's state, shifted once; the active ones from B's.  Pinned to the oracle run so."""
    name, mode = "ctrl20", 2
    kind, w1 = WR.scenario_workload(name, mode, 1)
    _, w2 = WR.scenario_workload(name, mode, 2)
    _, w3 = WR.scenario_workload(name, mode, 3)
    N, d, B = int(w1["N"]), WR.delay_of(w1, kind), w1["x0"].shape[0]
    r1, r2 = WR.scenario_ref(name, mode, 1), WR.scenario_ref(name, mode, 2)
    active = _mask(B); on = active != 0
    eng = engine(w1, mode=mode)
    try:
        oA = run(eng, w1)
        oB = run(eng, w2, active, out={k: v.copy() for k, v in oA.items()})
        oC = run(eng, w3)
    finally:
        eng.close()
    assert same(oB, oA, ~on) is None, same(oB, oA, ~on)
    assert np.array_equal(WR.key(oB)[on], WR.key(r2)[on])
    zB, yB = WR.warm_state(r2, kind, N, d, mode)
    zA, yA = WR.warm_state(r1, kind, N, d, mode)
    zB[~on] = zA[~on]; yB[~on] = yA[~on]
    rC = O.tick_batch_qp(w3, kind, nthreads=WR.NTHREADS, warm=(zB, yB))
    cold = WR.scenario_ref(name, mode, 3, cold=True)
    assert np.any(rC["iters"][~on] != cold["iters"][~on])              # the test can tell an instance that lost its state
    assert np.array_equal(WR.key(oC), WR.key(rC)), np.nonzero((WR.key(oC) != WR.key(rC)).any(axis=1))[0]
    print("plain, masked, plain: %s" % T.check_batch(w3, kind, oC, rC))


def test_a_changed_batch_size_starts_cold():
    """Sizes 71 -> 40 -> 71 with warm_start 2: the second and the third call are both cold, word for word a warm_start 0 handle's."""
    name, mode = "ctrl20", 2
    kind, w1 = WR.scenario_workload(name, mode, 1)
    _, w2 = WR.scenario_workload(name, mode, 2)
    B = w1["x0"].shape[0]
    first = np.arange(B) < 40
    w2s = rows(w2, first)
    eng, plain = engine(w1, mode=mode), engine(w1, mode=0)
    try:
        run(eng, w1)
        o40, o71 = run(eng, w2s), run(eng, w2)
        c40, c71 = run(plain, w2s), run(plain, w2)
    finally:
        eng.close(); plain.close()
    assert same(o40, c40) is None, same(o40, c40)
    assert same(o71, c71) is None, same(o71, c71)
    cold, warm = WR.scenario_ref(name, mode, 2, cold=True), WR.scenario_ref(name, mode, 2)
    assert np.any(warm["iters"] != cold["iters"]) and np.any(warm["iters"][first] != cold["iters"][first])
    print("71 -> 40 -> 71: %s %s" % (T.check_batch(w2s, kind, o40, rows(cold, first)), T.check_batch(w2, kind, o71, cold)))


@pytest.mark.parametrize("mode", WR.MODES)
def test_an_infeasible_previous_tick_starts_cold(mode):
    """An instance whose previous tick had no solution (PRIMAL INFEASIBLE instances of the planner workload) starts cold: word
    for word a warm_start 0 handle's second tick, and the cold oracle's under check_batch."""
    name = "plan20"
    kind, w1 = WR.scenario_workload(name, mode, 1)
    _, w2 = WR.scenario_workload(name, mode, 2)
    r1 = WR.scenario_ref(name, mode, 1)
    none = ~WR.has_solution(r1)
    assert none.sum() >= 3, none.sum()
    eng, plain = engine(w1, mode=mode), engine(w1, mode=0)
    try:
        o1 = run(eng, w1)
        o2 = run(eng, w2)
        c2 = run(plain, w2)
    finally:
        eng.close(); plain.close()
    assert np.array_equal(~WR.has_solution(o1), none)
    assert same(o2, c2, none) is None, (same(o2, c2, none), o2["iters"][none], c2["iters"][none])
    assert same(o2, c2, ~none) is not None                             # the others did start warm
    cold = WR.scenario_ref(name, mode, 2, cold=True)
    print("no solution, then cold (mode %d): %s" % (mode, T.check_batch(rows(w2, none), kind, rows(o2, none), rows(cold, none))))
