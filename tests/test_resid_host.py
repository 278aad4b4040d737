"""CPU: the oracle side of tests/test_gpu_resid.py -- the yardsticks of the reported words resid = (pri_res, dua_res, obj_val, rho_final).

  * The oracle's own words can be recomputed from the point it returns, in long double, with no ADMM involved (ORACLE_DEV_* of
    tests/_tolerance.py): the device's words are held to 100 x these figures at the device's own point.
  * The oracle under its two elimination orders of the same KKT matrix (the stage-wise order of tick_batch_qp, solve_qp's RCM order)
    differs by round-off alone: no status, iteration count or polish flag differs on more than 5 % of a workload, and the spread of
    each word per class is ORDER_DEV_*: the device's words are held to 100 x these against the oracle's.
  Every constant is asserted from both sides: never exceeded, and not more than twice the measured figure, so a stale one fails.
  * Non-vacuity of the GPU module: the classes are populated, the cases change the words, rho_final is the configured rho where no
    update can run, and the late rho update (tests/_tolerance.py late_rho) changes the oracle's rho_final where the rule says so.
Nine workloads, thirteen cases and the module's own (tests/_tolerance.py RESID_CASES, RESID_OWN_CASES)."""
import numpy as np
import pytest

from oracle import osqp_ref as O
from tests import _tolerance as T
from tests import test_gpu_settings as G

CASES = T.RESID_CASES + list(T.RESID_OWN_CASES)
_RCM, _STAGE, _REP = {}, {}, {}


def settings_of(case):
    return T.RESID_OWN_CASES[case] if case in T.RESID_OWN_CASES else G.settings_of(case)


def stage(name, case):
    if case not in T.RESID_OWN_CASES:
        return G.oracle(name, case)
    if (name, case) not in _STAGE:
        kind, w = G.workload(name)
        _STAGE[(name, case)] = O.tick_batch_qp(w, kind, settings=settings_of(case), nthreads=G.NTHREADS, qps=G._QPS[name])
    return _STAGE[(name, case)]


def rcm(name, case):
    if (name, case) not in _RCM:
        kind, w = G.workload(name)
        _RCM[(name, case)] = O.tick_batch_qp(w, kind, settings=settings_of(case), nthreads=G.NTHREADS, qps=G._QPS[name], order="rcm")
    return _RCM[(name, case)]


def reports(case):
    """Per workload: check_resid of the stage-wise oracle against itself (its own-point figures) and of the RCM oracle against it."""
    if case not in _REP:
        _REP[case] = {}
        for name in G.WORKLOADS:
            kind, w = G.workload(name)
            a, b = stage(name, case), rcm(name, case)
            kw = dict(settings=settings_of(case), qps=G._QPS[name], named=T.RESID_NAMED.get((case, name), ()), late_rule=False)
            _REP[case][name] = (T.check_resid(w, kind, a, a, None, **kw), T.check_resid(w, kind, b, a, None, **kw))
    return _REP[case]


def _own(k):
    return k[0].endswith("_own") or k[0] == "pri_excess"


def _held(measured, recorded, what):
    for k, c in recorded.items():
        m = measured.get(k, 0.0)
        print("%s %s/%s: measured %.3e, recorded %.3e" % (what, k[0], k[1], m, c))
        assert m <= c, (what, k, m, c)
        assert m >= 0.5 * c, (what, k, m, c, "the recorded figure is stale")


def test_oracle_words_are_recomputed_from_its_point():
    """ORACLE_DEV_*: obj_val, pri_res (polished: against the violation; unpolished: never below it) and dua_res of both orders
    against the long double evaluation at the returned (z, y)."""
    worst = {}
    for case in CASES:
        for name, (r0, r1) in reports(case).items():
            for r in (r0, r1):
                for k, v in r["worst"].items():
                    if _own(k):
                        worst[k] = max(worst.get(k, 0.0), v)
    _held(worst, T.RESID_ORACLE_DEV, "own point")


def test_order_to_order_yardstick():
    """ORDER_DEV_*: the RCM order against the stage-wise order, per word and class; obj_val of class D word for word."""
    worst = {}
    for case in CASES:
        for name, (r0, r1) in reports(case).items():
            for k, v in r1["worst"].items():
                if not _own(k):
                    worst[k] = max(worst.get(k, 0.0), v)
    assert worst[("obj", "D")] == 0.0
    _held({k: v for k, v in worst.items() if k != ("obj", "D")}, {k: v for k, v in T.RESID_ORDER_DEV.items() if k != ("obj", "D")}, "orders")
    assert set(T.RESID_BOUNDS) == set(T.RESID_ORACLE_DEV) | set(T.RESID_ORDER_DEV) | {("dua_floor", "A")}
    assert all(T.RESID_BOUNDS[k] == 100.0 * v for d in (T.RESID_ORACLE_DEV, T.RESID_ORDER_DEV) for k, v in d.items())


@pytest.mark.parametrize("case", CASES, ids=lambda c: str(c))
def test_orders_agree_in_status_iterations_and_polish(case):
    """The share of instances left out of the comparison because the two orders decide differently: at most 5 % per workload."""
    for name, (r0, r1) in reports(case).items():
        B = stage(name, case)["status"].shape[0]
        print("%s %s: %s left out %s" % (case, name, r1["counts"], r1["left_out"]))
        assert not r0["left_out"] or all(stage(name, case)["status"][j] == -10 for j in r0["left_out"]), (name, r0["left_out"])
        assert len(r1["left_out"]) <= 0.05 * B, (case, name, r1["left_out"])
        c = r1["counts"]
        assert c["A"] + c["B"] + c["C"] + c["D"] + c["unsolved"] + len(r1["left_out"]) == B


def test_classes_are_populated():
    """The defaults populate all four classes (planner N = 25: A 33, B 23, C 5, D 6); max60 puts at least 60 planner instances in
    class C; nopolish has no class A; max1 ends every instance at the cap."""
    c = reports(None)["plan25"][0]["counts"]
    assert (c["A"], c["B"], c["C"], c["D"]) == (33, 23, 5, 6), c
    tot = T.merge_resid_reports([r0 for r0, _ in reports(None).values()])["counts"]
    assert min(tot["A"], tot["B"], tot["C"], tot["D"]) >= 10, tot
    n = sum(reports("max60")[name][0]["counts"]["C"] for name in G.WORKLOADS if G.WORKLOADS[name][0] == "planner")
    assert n >= 60, n
    assert all(r0["counts"]["A"] == 0 for r0, _ in reports("nopolish").values())
    c1 = T.merge_resid_reports([r0 for r0, _ in reports("max1").values()])["counts"]
    assert c1["A"] == c1["B"] == c1["D"] == 0 and c1["C"] >= 600, c1


@pytest.mark.parametrize("case", ["adp0", "norho", "max1"])
def test_rho_final_is_the_configured_rho_where_no_update_runs(case):
    assert T.rho_is_fixed(settings_of(case)) and not T.rho_is_fixed(None) and not T.rho_is_fixed(settings_of("max60"))
    for name in G.WORKLOADS:
        for o in (stage(name, case), rcm(name, case)):
            ok = o["status"] != -10
            assert ok.sum() >= 60 and np.all(o["resid"][ok, 3] == 0.1), name


@pytest.mark.parametrize("case", [c for c in CASES if c is not None], ids=str)
def test_each_case_changes_the_words(case):
    """Against the defaults, each case changes resid on at least a third of the instances of one workload."""
    best = 0.0
    for name in G.WORKLOADS:
        a, b = stage(name, None)["resid"], stage(name, case)["resid"]
        diff = ~np.all((a == b) | (np.isnan(a) & np.isnan(b)), axis=1)
        best = max(best, float(diff.mean()))
    print("%s: resid differs from the defaults' on %.0f %% of the instances of its most changed workload" % (case, 100 * best))
    assert best >= 1.0 / 3.0, (case, best)


def test_resid_of_an_instance_without_an_answer_is_nan():
    """tick_batch_qp: NaN x 4 on an instance it gives up on (-10), finite words elsewhere; the existing keys are unchanged."""
    kind, w = G.workload("plan25")
    qps = list(G._QPS["plan25"]); qps[3] = None
    o = O.tick_batch_qp(dict(w), kind, nthreads=G.NTHREADS, qps=qps)
    assert set(o) == {"xPred", "uPred", "z", "y", "status", "iters", "polish", "resid"} and o["resid"].shape == (67, 4)
    assert o["status"][3] == -10 and np.isnan(o["resid"][3]).all()
    rest = np.arange(67) != 3
    assert np.isfinite(o["resid"][rest]).all()
    assert np.array_equal(o["resid"][rest], stage("plan25", None)["resid"][rest])
    with pytest.raises(ValueError):
        O.tick_batch_qp(dict(w), kind, qps=qps, order="amd")


def test_the_late_rho_update():
    """Where max_iter is off the check grid and on the rho grid, the oracle updates rho on the last iteration before its closing
    check (osqp_ref.c: the update sits inside the loop); the device's closing check comes first, so a run it ends reports the rho
    of iteration max_iter - 1 (tests/_tolerance.py late_rho).  None of RESID_CASES has such an iteration; under the module's own
    case the rule takes instances on most workloads, and on some of them the oracle's rho_final is NOT the rho one iteration
    earlier -- so the rule states a difference, and the GPU test would fail without it."""
    for case in T.RESID_CASES:
        st = settings_of(case)
        cap = (st or {}).get("max_iter", 4000)
        assert not any(T.late_rho(s, cap, st) for s in (1, -3, -4)), case
    case, = T.RESID_OWN_CASES
    st = settings_of(case)
    assert T.late_rho(1, 75, st) and T.late_rho(-3, 75, st) and not T.late_rho(-2, 75, st) and not T.late_rho(2, 75, st) and not T.late_rho(1, 40, st)
    n = moved = 0
    for name in ("ctrl20", "plan20", "plan30"):
        kind, w = G.workload(name)
        o = stage(name, case)
        perm = O.ctrl_delay_ordering(int(w["N"]), 0) if kind == "controller" else O.plan_ordering(int(w["N"]))
        for j in np.nonzero(o["status"] != -10)[0]:
            if T.late_rho(int(o["status"][j]), int(o["iters"][j]), st):
                qp = G._QPS[name][j]
                r = O.solve_qp(qp.P, qp.q, qp.A, qp.l, qp.u, perm=perm, **dict(st, max_iter=74))
                n += 1
                moved += int(abs(r.info.rho_final - o["resid"][j, 3]) > 0.5 * r.info.rho_final)
    print("late rho update: %d instances under the rule, the oracle's rho_final moved on the last iteration on %d of them" % (n, moved))
    assert n >= 10 and moved >= 1, (n, moved)
