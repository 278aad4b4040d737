"""GPU: the words a solve reports about itself -- resid[B][4] = (pri_res, dua_res, obj_val, rho_final), include/lpvmpc.h -- against
the CPU oracle and against a long double recomputation from the point the device returns.

Every other GPU test compares resid device against device (variants, deferral, riders, masked calls, bound handles, the bitwise
golden fixture); the code that writes the words feeds no decision, so statuses and iteration counts do not pin it either: a
value that is wrong on every route passed them all.  Here, on the 24 solve routes of tests/test_gpu_settings.py and under thirteen
settings cases (tests/_tolerance.py RESID_CASES) plus one of this module's own (LATE_RHO):
  * obj_val against 1/2 z'Pz + q'z of the device's own point in long double (needs no oracle solve; classes A, B, C), against the
    oracle's obj_val (A, B), and word for word +-1e30 where there is no solution (D);
  * pri_res against the long double constraint violation of the device's point (A; an upper bound of it in B and C), pri_res
    and dua_res against the oracle's (A in units of the termination threshold, B, C, D relative);
  * rho_final relative to the oracle's, word for word the configured rho where no update can run (adp0, norho, max1), and on the
    instances of the late rho update (tests/_tolerance.py late_rho) against the oracle's rho one iteration earlier;
  * NaN x 4 on a row without an answer, the neighbours' words unchanged bit for bit.
Rules and bounds: tests/_tolerance.py (check_resid, RESID_BOUNDS: 100 x the oracle's own figure of each quantity and class,
measured by tests/test_resid_host.py).  Class counts and worst figures are printed per case (run with -s)."""
import numpy as np
import pytest

from oracle import osqp_ref as O
from tests import _tolerance as T
from tests import test_gpu_settings as G
from tests.test_gpu_schedule import park_check

pytestmark = pytest.mark.gpu

# max_iter off the check grid (40) and on the rho grid (15): the closing check of iteration 75 ends runs that the oracle's rho update
# of the same iteration precedes (tests/_tolerance.py late_rho).  None of the cases of RESID_CASES has such an iteration.
OWN_CASES = T.RESID_OWN_CASES
LATE_RHO, = OWN_CASES
CASES = T.RESID_CASES + [LATE_RHO]
LEFT_OUT_SHARE = 0.05

_ORC = {}


def settings_of(case):
    return OWN_CASES[case] if case in OWN_CASES else G.settings_of(case)


def oracle(name, case):
    if case not in OWN_CASES:
        return G.oracle(name, case)
    if (name, case) not in _ORC:
        kind, w = G.workload(name)
        _ORC[(name, case)] = O.tick_batch_qp(w, kind, settings=OWN_CASES[case], nthreads=G.NTHREADS, qps=G._QPS[name])
    return _ORC[(name, case)]


def accepted_by_check_batch(case, name, kind, w, out, ref, j, st):
    """An instance whose status, iteration count or polish flag differs from the oracle's is left out of check_resid; it must be
    one check_batch accepts: a status flip at the cap, class D (the certificate one check apart), a named instance of
    BEYOND_BARS, or one outside its ``sane`` mask (the oracle gives up on it: scaling3, planner N = 25 #63, whose KKT factorisation
    breaks down under the stage-wise order)."""
    so, sr = int(out["status"][j]), int(ref["status"][j])
    if sr == -10 or (sr == 1 and np.isnan(ref["uPred"][j]).any()):
        return "no oracle answer"
    if {so, sr} <= {T.SOLVED_INACC, T.MAX_ITER} and so != sr and int(out["iters"][j]) == int(ref["iters"][j]):
        return "flip"
    if int(out["iters"][j]) != int(ref["iters"][j]) and T.class_d(w, kind, j, out, ref, st):
        return "D"
    if j % len(G._QPS[name]) in G.BEYOND_BARS.get((case, name), ([], None))[0]:
        return "beyond"
    return None


def run_route(case, route, bounds=None):
    """One route under one case through check_resid; returns (tag, report, out)."""
    name, variant, tile, defer = route
    st = settings_of(case) or {}
    kind, w = G.workload(name)
    ref = oracle(name, case)
    if tile:
        w, ref = G.tiled(w, G.TILE), G.tiled_ref(ref, G.TILE)
    out, parked = G.device_solve(w, variant, defer, **st)
    B = w["x0"].shape[0]
    tag = "%s %s B=%d variant=%d defer=%d parked=%d" % (case, name, B, variant, defer, parked)
    if defer:       # the tail kernel's read-back of the residual words runs on parked instances (none parks without a check inside the loop)
        if park_check(st, defer) is None:
            assert parked == 0, tag
        else:
            assert parked >= 1, tag
    rep = T.check_resid(w, kind, out, ref, bounds, st, G._QPS[name], named=T.RESID_NAMED.get((case, name), ()),
                        polish_floor=T.RESID_POLISH_FLOOR.get((case, name), ()))
    for j in rep["left_out"]:
        why = accepted_by_check_batch(case, name, kind, w, out, ref, j, st)
        assert why, (tag, j, "left out", int(out["status"][j]), int(ref["status"][j]), int(out["iters"][j]), int(ref["iters"][j]),
                     int(out["polish"][j]), int(ref["polish"][j]))
    assert len(rep["left_out"]) <= LEFT_OUT_SHARE * B, (tag, rep["left_out"])
    c = rep["counts"]
    assert c["A"] + c["B"] + c["C"] + c["D"] + c["unsolved"] + len(rep["left_out"]) == B, (tag, c)
    return tag, rep, out


def _fmt(worst):
    return ", ".join("%s/%s %.2e" % (k[0], k[1], v) for k, v in sorted(worst.items()))


@pytest.mark.parametrize("case", CASES, ids=lambda c: str(c))
def test_resid_on_every_route(case):
    """All 24 routes under one settings case: every instance lands in a class (or is one check_batch accepts: at most 5 % of a
    route), every word of resid within its bound.  The deferred routes park (where the schedule has a check to park at): the
    tail kernel finishes those instances and reads the residual words back from its checker's verdict."""
    reports = []
    for route in G.ROUTES:
        tag, rep, out = run_route(case, route, T.RESID_BOUNDS)
        reports.append(rep)
        print("%s iters %d..%d %s left out %s" % (tag, int(np.min(out["iters"])), int(np.max(out["iters"])), rep["counts"], rep["left_out"]))
    tot = T.merge_resid_reports(reports)
    print("%s: %s, left out %d; worst: %s" % (case, tot["counts"], tot["left_out"], _fmt(tot["worst"])))
    c = tot["counts"]
    if case == "nopolish":
        assert c["A"] == 0, c
    if case == LATE_RHO:
        assert c["late_rho"] >= 24, c                 # (at least one instance per route takes the rule)
    else:
        assert c["late_rho"] == 0, c
    if case is None:
        assert min(c["A"], c["B"], c["C"], c["D"]) >= 24, c


def test_rows_without_an_answer_report_nan():
    """Three rows with non-finite inputs (the batch of tests/test_gpu_parity.py test_non_finite_inputs_yield_nan_and_unsolved):
    four NaN each; the neighbours' resid equals the clean run's bit for bit, on three kernel variants."""
    from lpvmpc import workloads
    w = workloads.controller_batch(6, N=20, seed=4)
    for variant in (0, 1, 2):
        eng = workloads.make_solver(w)
        eng.set_option("kernel_variant", variant)
        clean = eng.solve(w["x0"], w["u_prev"], w["vel_ref"], w["curv_s"], w["u_old"], None, w["cf_new"], w["lap"])
        x0 = w["x0"].copy(); vel = w["vel_ref"].copy(); uold = w["u_old"].copy()
        x0[1, 3] = np.nan; vel[3, 7] = np.inf; uold[4, 1] = np.nan
        out = eng.solve(x0, w["u_prev"], vel, w["curv_s"], uold, None, w["cf_new"], w["lap"])
        eng.close()
        cr, br = np.asarray(clean["resid"]), np.asarray(out["resid"])
        assert cr.shape == br.shape == (6, 4)
        for b in (1, 3, 4):
            assert out["status"][b] == -10 and np.isnan(br[b]).all(), (variant, b, br[b])
        for b in (0, 2, 5):
            assert np.isfinite(cr[b]).all() and cr[b].tobytes() == br[b].tobytes(), (variant, b, cr[b], br[b])
