"""GPU: the loop schedule of the solve -- check_termination, adaptive_rho, adaptive_rho_interval, max_iter, polish -- against the
CPU oracle (oracle/osqp_ref.py tick_batch_qp under the same settings) on every solve route of tests/test_gpu_settings.py.

Every other comparison with the oracle runs 25 / 25 / 4000 / on / on, where the check grid, the rho grid and the cap coincide.  The
cases of SCHEDULES (tests/test_gpu_settings.py) take them apart: checks without rho updates and rho updates without checks (the
register-state kernels file their state on either, the other forms are told of the check only), a cap off both grids and no
check inside the loop (OSQP's closing update_info / check_termination: here the last iteration's own check, the counter to the
next check never reaching past max_iter), one iteration, a check on the first iteration, no adaptation, no polish.
  a. the schedule matrix on every route: statuses and iteration counts equal to the oracle's, solutions to tests/_tolerance.py, no
     class D, the parking of the deferred routes as the settings say, the polish flags of nopolish, adp0 and norho the same run;
  b. polished device solutions against the active-set optimum under the schedule cases that have polished points;
  c. park and restore under schedules whose two intervals differ: a deferred call equals the plain call bit for bit, with a pass
     to completion behind the call and with riders in the next call.
Class counts are printed per case and route (run with -s)."""
import numpy as np
import pytest

from tests import _tolerance as T
from tests import test_gpu_deferral_riders as R
from tests import test_gpu_settings as G
from tests.test_gpu_horizons import ctrl_workload, plan_workload
from tests.test_gpu_settings import ROUTES, SCHEDULES, TILE, device_solve, oracle, tiled, tiled_ref, workload

pytestmark = pytest.mark.gpu

PENDING = -11


def _chk(st):
    return int(st.get("check_termination", 25))


def _adp(st):
    return int(st.get("adaptive_rho_interval", 25)) if st.get("adaptive_rho", 1) else 0


def _cap(st):
    return int(st.get("max_iter", 4000))


def park_check(st, defer_after):
    """The iteration at which an instance that is still unsolved parks: the first termination check inside the loop at or beyond
    defer_after and before the cap (an instance at max_iter is finished, not parked).  None: the schedule has no such check."""
    chk = _chk(st)
    if chk <= 0:
        return None
    p = -(-defer_after // chk) * chk
    return p if p < _cap(st) else None


def counters_at(st, p):
    """The down-counters (to_chk, to_adp) of the loop behind iteration p: iterations to the next check / rho update (p at least a
    check interval in front of the cap, where the check counter is cut to the iterations left)."""
    chk, adp = _chk(st), _adp(st)
    return (chk - p % chk if chk > 0 else 0), (adp - p % adp if adp > 0 else 0)


# ---- a. the schedule matrix on every route -----------------------------------------------------------------------------------
# One more deferred route per workload for max100: defer_after at the cap itself.  The check of iteration 100 is the last
# iteration's, so nothing parks there.
EXTRA_ROUTES = {"max100": [("ctrl20", 0, False, 100), ("plan20", 0, False, 100)]}
# (case, workload): instances beyond their class's bar with status and iteration count equal to the oracle's, each under a rule of
# tests/test_gpu_settings.py _beyond_bars (at most one per (case, workload); a status or count disagreement is never listed)
BEYOND_BARS = {}


@pytest.mark.parametrize("case", list(SCHEDULES))
def test_schedule_on_every_route(case):
    """Every route of the solve under one loop schedule: statuses and iteration counts equal to the oracle's, solutions in classes
    A-C.  No class D (the oracle's two elimination orders agree on every instance under these cases).  At most one status flip at
    the cap per (case, workload).  The deferred routes park where the settings leave a check in [defer_after, max_iter) and park
    nothing otherwise; either way the call returns the oracle's results.  nopolish: no polish flag set.  Every route runs: a route
    that misses a rule is listed with what it missed, and the routes behind it are still held to theirs."""
    flipped, failed = {}, []
    for route in ROUTES + EXTRA_ROUTES.get(case, []):
        try:
            _one_route(case, route, flipped)
        except AssertionError as e:
            failed.append((route, str(e)[:400]))
    for name, js in flipped.items():
        if len(js) > 1:
            failed.append((name, "flips", sorted(js)))
    assert not failed, failed


def _one_route(case, route, flipped):
    st = SCHEDULES[case]
    name, variant, tile, defer = route
    kind, w = workload(name)
    ref = oracle(name, case)
    B0 = w["x0"].shape[0]
    if tile:
        w, ref = tiled(w, TILE), tiled_ref(ref, TILE)
    out, parked = device_solve(w, variant, defer, **st)
    tag = "%s %s B=%d variant=%d defer=%d parked=%d" % (case, name, w["x0"].shape[0], variant, defer, parked)
    if defer:
        p = park_check(st, defer)
        if p is None:
            assert parked == 0, (tag, parked)
        else:
            n_late = int(np.sum(ref["iters"] > p))                 # the oracle's instances that pass that check unsolved
            assert n_late >= 1 and 1 <= parked <= n_late, (tag, p, n_late)
    if case == "nopolish":
        assert not np.any(ref["polish"]) and not np.any(out["polish"]), (tag, np.nonzero(out["polish"])[0][:8])
    flipped.setdefault(name, set()).update(int(j) % B0 for j in np.nonzero(out["status"] != ref["status"])[0])
    skip, rule = BEYOND_BARS.get((case, name), ([], None)) if not tile else ([], None)
    if skip:
        assert len(skip) <= 1
        G._beyond_bars(case, name, kind, w, out, ref, skip, rule)
        B = w["x0"].shape[0]
        w, out, ref = G._drop(w, skip, B), G._drop(out, skip, B), G._drop(ref, skip, B)
    counts = T.check_batch(w, kind, out, ref, settings=st)
    G._report(tag, counts, out)
    assert counts["D"] == 0, (tag, counts)


def test_interval_zero_and_adaptive_rho_off_are_the_same_run():
    """adaptive_rho_interval = 0 and adaptive_rho = 0 both mean no adaptation (include/lpvmpc.h; the oracle returns identical
    results for the two, tests/test_settings_host.py): every output word of the two device runs is equal on every route."""
    for name, variant, tile, defer in ROUTES:
        kind, w = workload(name)
        if tile:
            w = tiled(w, TILE)
        # (a pool entry for every request -- 2 B: instances younger than twice defer_after may take three quarters of a pool -- so that
        # which instances the tail kernel finishes does not depend on timing)
        pool = 2 * w["x0"].shape[0]
        a, pa = device_solve(w, variant, defer, defer_pool=pool, **SCHEDULES["adp0"])
        b, pb = device_solve(w, variant, defer, defer_pool=pool, **SCHEDULES["norho"])
        assert pa == pb, (name, variant, defer, pa, pb)
        assert set(a) == set(b)
        for k in a:
            assert np.array_equal(a[k], b[k], equal_nan=True), (name, variant, defer, k)


# ---- b. polished solutions against the active-set optimum --------------------------------------------------------------------
# Polished points of the oracle alone that are the active-set optimum, of up to 12 per workload (CPU, counted before this list
# was written): chk1 99, chk7_adp10 99, chk10_adp7 100, adp40 103, chk40_adp15_max130 94, chk0_max90 93, max60 92, max100 93,
# adp0 100, norho 100.  max1 (every instance at the cap after one iteration) and nopolish have none and fall out.
CERTIFIED = [c for c in SCHEDULES if c not in ("max1", "nopolish")]


@pytest.mark.parametrize("case", CERTIFIED)
def test_polished_solutions_are_the_active_set_optimum(case):
    """tests/test_gpu_settings.py's certificate test under the schedule cases with at least 30 such points on the oracle side
    (CERTIFIED): wherever the oracle's polished point is the active-set optimum, the device's is too, to 1e-6, on at least 30
    instances.  Left out: max1 and nopolish, which polish nothing."""
    G.test_polished_solutions_are_the_active_set_optimum(case)


# ---- c. park and restore keep the counters -----------------------------------------------------------------------------------
PARK_WORKLOADS = ["ctrl20", "plan20", "plan30"]        # (plan30: deferred handles use the four-wavefront form)
PARK_CASES = ["chk7_adp10", "chk40_adp15_max130", "adp40"]
# (first, second) batch of a workload: call 1, whose instances park and are followed, and call 2.  The planners take the matrix's
# batch first and one more of the same builder and size second.  The controller takes them the other way round: of the matrix's 71
# instances only two pass the first check of chk40_adp15_max130 (iteration 40) unsolved, of seed 8134's five do, two up to the cap.
BATCHES = {"ctrl20": (lambda: ctrl_workload(71, 20, seed=8134), lambda: workload("ctrl20")[1]),
           "plan20": (lambda: workload("plan20")[1], lambda: plan_workload(67, 20, seed=8211)),
           "plan30": (lambda: workload("plan30")[1], lambda: plan_workload(67, 30, seed=8213))}
_BATCH, _PLAIN = {}, {}


def _batch(name, second):
    if (name, second) not in _BATCH:
        _BATCH[(name, second)] = BATCHES[name][int(second)]()
    return _BATCH[(name, second)]


def _engine(w, st, B):
    import lpvmpc
    eng = lpvmpc.BatchedSolver(w["kind"], w["N"], w["dt"], w["Q"], w["R"], w["dR"], L_cf=w["L_cf"], track=w["track"], **st)
    eng.reserve(B)
    return eng


def _dev_call(torch, eng, w, stream=None):
    return R._dev_call(torch, eng, w, w["x0"].shape[0], w["kind"] == "planner", stream=stream)


def _plain(torch, name, case, second=False):
    """The plain call of a batch under a case, run once and shared (never written to)."""
    if (name, case, second) not in _PLAIN:
        w = _batch(name, second)
        eng = _engine(w, SCHEDULES[case], w["x0"].shape[0])
        _, o = _dev_call(torch, eng, w); torch.cuda.synchronize()
        _PLAIN[(name, case, second)] = R._host(o)
        eng.close()
    return _PLAIN[(name, case, second)]


def choose_defer_after(st, iters):
    """defer_after from the plain run's iteration counts: a check iteration K inside the loop behind which the two down-counters
    differ and which at least three instances pass unsolved -- the first that at most half of the batch passes, or, where every
    check has more (a low cap), the first of all.  Returns (K, number of instances beyond K)."""
    chk = _chk(st)
    cands = []
    for p in range(chk, min(_cap(st), int(iters.max())), chk):
        c = counters_at(st, p)
        if c[0] != c[1] and int(np.sum(iters > p)) >= 3:
            cands.append(p)
    assert cands, "no check iteration with three instances beyond it"
    few = [p for p in cands if np.sum(iters > p) <= len(iters) // 2]
    K = few[0] if few else cands[0]
    return K, int(np.sum(iters > K))


@pytest.mark.parametrize("case", PARK_CASES)
@pytest.mark.parametrize("name", PARK_WORKLOADS)
def test_pass_behind_the_call_restores_the_counters(name, case):
    """defer_tail 0, defer_pool B, defer_budget 0: a deferred call (the same kernel's pass to completion behind it) and the join
    equal the plain call of the same settings bit for bit (include/lpvmpc.h).  At least three instances park, the first of them at
    the check of iteration K with to_chk != to_adp: a restore that mixed the two counters up, or reset them to their intervals,
    moves the next rho update or check and with it every word behind it."""
    import torch
    st = SCHEDULES[case]
    w = _batch(name, False)
    B = w["x0"].shape[0]
    ref = _plain(torch, name, case)
    K, n_late = choose_defer_after(st, ref["iters"])
    to_chk, to_adp = counters_at(st, K)
    assert n_late >= 3 and to_chk != to_adp and park_check(st, K) == K
    eng = _engine(w, st, B)
    eng.set_option("defer_pool", B); eng.set_option("defer_after", K); eng.set_option("defer_budget", 0); eng.set_option("defer_tail", 0)
    _, o = _dev_call(torch, eng, w)
    eng.join(0); torch.cuda.synchronize()
    parked, refused = eng.defer_stats()
    print("%s %s: defer_after %d (to_chk %d, to_adp %d), %d of %d beyond it, %d parked, %d refused" % (name, case, K, to_chk, to_adp, n_late, B, parked, refused))
    # (the first 3 B / 4 requests of the check at K get a pool entry -- the share of instances younger than 2 K -- so min(n_late, that) park there)
    assert parked >= 3, (parked, refused)
    R._same(R._host(o), ref)
    eng.close()


@pytest.mark.parametrize("case", PARK_CASES)
@pytest.mark.parametrize("name", PARK_WORKLOADS)
def test_riders_restore_the_counters(name, case):
    """Riders (defer_budget > 0, defer_tail 0) under a schedule whose intervals differ, by the rule of
    tests/test_gpu_deferral_riders.py test_parked_instances_ride_in_the_next_call: after call 1 alone every instance beyond K is
    LPVMPC_PENDING at K; call 2 (another batch) carries them one budget (a multiple of the check interval) further: finished, or
    parked again exactly there; after the join every word of both calls equals the plain calls'.  At least three instances park, at
    least one of them with to_chk != to_adp (from the iteration it is pending at)."""
    import torch
    st = SCHEDULES[case]
    w1, w2 = _batch(name, False), _batch(name, True)
    B = w1["x0"].shape[0]
    ref1, ref2 = _plain(torch, name, case), _plain(torch, name, case, True)
    K, n_late = choose_defer_after(st, ref1["iters"])
    budget = 2 * _chk(st)
    eng = _engine(w1, st, B)
    eng.set_option("defer_pool", 4 * B)        # the stragglers of both calls, all of them young: three quarters of it must hold them ("defer_pool")
    eng.set_option("defer_after", K); eng.set_option("defer_budget", budget); eng.set_option("defer_tail", 0)
    s = torch.cuda.Stream()
    keep1, o1 = _dev_call(torch, eng, w1, stream=s)
    torch.cuda.synchronize()
    h1 = R._host(o1)
    late = ref1["iters"] > K
    assert np.all(h1["status"][late] == PENDING) and np.all(h1["iters"][late] == K), (h1["status"][late], h1["iters"][late])
    assert not np.any(h1["status"][~late] == PENDING)
    for k in ("status", "iters", "uPred"):
        assert np.array_equal(h1[k][~late], ref1[k][~late], equal_nan=True), k
    parked1, refused1 = eng.defer_stats()
    assert parked1 == int(late.sum()) >= 3 and refused1 == 0, (parked1, refused1)
    differ = [counters_at(st, int(p)) for p in h1["iters"][late]]
    assert any(c[0] != c[1] for c in differ), differ[:4]
    keep2, o2 = _dev_call(torch, eng, w2, stream=s)
    torch.cuda.synchronize()
    h1b, h2 = R._host(o1), R._host(o2)
    refused2 = eng.defer_stats()[1] - refused1
    idx = np.nonzero(late)[0]
    still = idx[h1b["status"][idx] == PENDING]
    done = idx[h1b["status"][idx] != PENDING]
    print("%s %s: defer_after %d budget %d: %d parked by call 1, %d finished as riders of call 2, %d parked again; %d refusals in call 2"
          % (name, case, K, budget, len(idx), len(done), len(still), refused2))
    if refused2 == 0:
        assert np.array_equal(h1b["iters"][still], h1["iters"][still] + budget), (h1["iters"][still], h1b["iters"][still])
        assert np.all(ref1["iters"][done] <= h1["iters"][done] + budget)    # finished within the budget, not beyond it
        # which of the two happens follows from the plain run: parked again iff unsolved at K + budget, a check before the cap
        again = (ref1["iters"] > K + budget) & (K + budget < _cap(st))
        assert np.array_equal(np.sort(still), np.nonzero(again)[0]), (still, np.nonzero(again)[0])
    else:
        assert np.all(h1b["iters"][still] >= h1["iters"][still] + budget)
    assert np.all(ref1["iters"][still] > h1["iters"][still] + budget)
    for k in ("status", "iters", "polish", "xPred", "uPred", "resid"):
        assert np.array_equal(h1b[k][done], ref1[k][done], equal_nan=True), k
    late2 = ref2["iters"] > K
    assert np.all(h2["status"][late2] == PENDING) and np.all(h2["iters"][late2] <= K) and not np.any(h2["status"][~late2] == PENDING)
    eng.join(s.cuda_stream); torch.cuda.synchronize()
    R._same(R._host(o1), ref1)
    R._same(R._host(o2), ref2)
    eng.close()
