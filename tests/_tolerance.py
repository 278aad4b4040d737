"""Test infrastructure: the stated float tolerance of the QP stage (include/lpvmpc.h) as code.

Against the CPU oracle on identical data, status and iteration count are EQUAL, with two documented exceptions:
  (1) a run that ends at max_iter, where OSQP's "solved inaccurate" test -- 10 eps -- is decided by round-off: MAX_ITER_REACHED on
      one side, SOLVED_INACCURATE on the other, same iteration count (one instance of the 110 202 of the wide sweep: oval, sweep
      seed 0, planner N = 20);
  (2) class D below: a PRIMAL INFEASIBLE planner QP whose certificate fires one termination check (25 iterations) apart (one
      instance of 110 202: Euge_Track, sweep seed 4, planner N = 40, #393 -- device 50, batch oracle 75).
The solution falls in one of three classes:

  A  polished (status SOLVED, polish flag 1): both sit on the active-set optimum            -> |dx|, |du| <= 1e-6
  B  un-polished, converged (SOLVED without a successful polish, SOLVED_INACCURATE before the cap): the two implementations run
     the same ADMM recursion and differ by the round-off of equivalent KKT factorisations   -> <= 2e-4 (observed <= 1e-6)
  C  ran to the iteration cap (max_iter = 4000: MAX_ITER_REACHED, or SOLVED_INACCURATE by the 10 eps test at the cap): the returned
     point is an UNCONVERGED ADMM iterate of an ill-conditioned planner QP (P has 31 near-zero eigenvalues; the
     forward-Euler model grows like 2^N); 4000 iterations amplify the round-off difference of the two implementations.  OSQP
     guarantees nothing for such a point and the reference uses it as it comes (CTRL:322-324, PLAN:214-216).  Held: same iteration
     count (the cap), statuses within {MAX_ITER_REACHED, SOLVED_INACCURATE}, |du| <= 2e-2 (observed over 110 202 instances: 42 in
     this class, |du| <= 1.01e-2, 40 of them with the objective within 1e-3 and the primal residual inside the status's tolerance;
     profiles/r06_parity_sweep.txt lists every one).  The class carries NO objective bound: two of the 42 (3110, sweep seed 1,
     planner N = 20 / 30, #63) differ from the oracle's point by 1.8e-2 / 2.8e-4 in the objective.
Every instance of the wide sweep (tests/diagnostics/seed_sweep.py) beyond 1e-6 is in class C.

  D  no solution on either side (PRIMAL / DUAL INFEASIBLE, exact or inaccurate: NaN outputs, equal statuses): the iterates of an
     infeasible QP diverge, K is as ill-conditioned as it gets (forward-Euler growth 1.7^40 at N = 40) and the certificate's third
     test, |A' dy| < eps |dy|, is then decided by the round-off of the KKT solve -- THE ORACLE ITSELF stops one check apart under its
     two elimination orders of the same KKT matrix (oracle/lpv_ref.c hands osqp_ref.c the stage-wise order, oracle/osqp_ref.py's
     solve_qp the RCM order of the assembled matrices: 75 against 50 iterations on the named instance, |dy| 12 037 against 567 at the
     check of iteration 25; tests/diagnostics/certificate_margin.py prints the margins).  Held: equal statuses, no solution on either
     side, and the device's iteration count equals the oracle's under ONE of its two elimination orders.  The reference discards
     such a result whatever its iteration count (feasible = 0: CTRL:320-324, PLAN:214-216).
"""
import numpy as np

from oracle import lpv_ref as L

P = dict(L.DEFAULT_PARAMS)
SOLVED, SOLVED_INACC, MAX_ITER = 1, 2, -2
NO_SOLUTION = (-3, 3, -4, 4)        # primal / dual infeasible, exact or inaccurate
CLASS_C_DU = 2e-2                   # (round 6: 5e-2 -> 2e-2; observed <= 1.01e-2)


def class_d(w, kind, j, out, ref, settings=None, params=None, limits=None):
    """Class D: an infeasible QP whose certificate fires one check apart.  True iff statuses are equal, neither side returns a
    solution and the device's iteration count is the oracle's under its OTHER elimination order (solve_qp: RCM) of the same data,
    solved under the same settings."""
    from oracle import osqp_ref as O
    st, sr = int(out["status"][j]), int(ref["status"][j])
    if st != sr or st not in NO_SOLUTION:
        return False
    if np.isfinite(out["uPred"][j]).any() or np.isfinite(ref["uPred"][j]).any():
        return False
    qp = instance_qp(w, kind, j, params, limits)
    r = O.solve_qp(qp.P, qp.q, qp.A, qp.l, qp.u, **O.osqp_settings(settings))
    return r.info.status_val == st and int(r.info.iter) == int(out["iters"][j])


def instance_qp(w, kind, j, params=None, limits=None):
    """(P, q, A, l, u) of instance j of a workload dict, assembled on the host as the reference does (oracle/osqp_ref.py
    instance_qp: vehicle ``params``, QP ``limits``)."""
    from oracle import osqp_ref as O
    return O.instance_qp(w, kind, j, params, limits)


def primal_residual(qp, z, eps=1e-3):
    """OSQP's unscaled primal residual of the point z (with its own z_c = clip(Az)) and the tolerance eps (1 + max(|Az|, |z_c|))."""
    A = np.asarray(qp.A.todense() if hasattr(qp.A, "todense") else qp.A, float)
    Az = A @ z
    zc = np.clip(Az, qp.l, qp.u)
    inf = lambda v: float(np.max(np.abs(v), initial=0.0))
    return inf(Az - zc), eps + eps * max(inf(Az), inf(zc))


def objective(qp, z):
    Pm = np.asarray(qp.P.todense() if hasattr(qp.P, "todense") else qp.P, float)
    return float(0.5 * z @ Pm @ z + np.asarray(qp.q, float) @ z)


def outlier_report(w, kind, j, out, ref, settings=None, params=None, limits=None):
    """Class-C evidence for instance j: a dict with the fields the sweep prints and `class` in {"C", "FAIL: ..."}."""
    st, st_ref = int(out["status"][j]), int(ref["status"][j])
    pol = int(out["polish"][j]) if "polish" in out else 0
    du = float(np.max(np.abs(out["uPred"][j] - ref["uPred"][j])))
    qp = instance_qp(w, kind, j, params, limits)
    zd = np.concatenate([out["xPred"][j].reshape(-1), out["uPred"][j].reshape(-1)])
    zr = np.concatenate([ref["xPred"][j].reshape(-1), ref["uPred"][j].reshape(-1)])
    fd, fr = objective(qp, zd), objective(qp, zr)
    gap = abs(fd - fr) / max(1.0, abs(fr))
    pri, tol = primal_residual(qp, zd)
    pri_ref, _ = primal_residual(qp, zr)
    capped = int(out["iters"][j]) == int(ref["iters"][j]) == int((settings or {}).get("max_iter", w.get("max_iter", 4000)))
    why = []
    if not ({st, st_ref} <= {SOLVED_INACC, MAX_ITER}):
        why.append("status (only runs that end at the cap may differ beyond class B)")
    if not capped:
        why.append("iterations (not at the cap)")
    if du > CLASS_C_DU:
        why.append("|du|")
    lim = tol if st == SOLVED else (10.0 * tol if st == SOLVED_INACC else float("inf"))      # (informative: a MAX_ITER point met no rule)
    return dict(status=st, status_ref=st_ref, polish=pol, iters=int(out["iters"][j]), iters_ref=int(ref["iters"][j]), du=du, obj_gap=gap,
                pri=pri, pri_tol=lim, pri_ref=pri_ref, **{"class": "C" if not why else "FAIL: " + ", ".join(why)})


def check_batch(w, kind, out, ref, allow_status_flip_at_max_iter=True, settings=None, params=None, limits=None):
    """The whole rule set on a batch; returns counts per class and raises AssertionError on the first violation.  ``settings``,
    ``params`` and ``limits``: those of the handle (BatchedSolver settings, vehicle parameters, QP limits as for
    oracle/osqp_ref.py tick_batch_qp), for the host's own solves of classes C and D."""
    sane = (ref["status"] != -10) & ~(np.isnan(ref["uPred"]).any(axis=(1, 2)) & (ref["status"] == 1))
    counts = dict(A=0, B=0, C=0, D=0, no_solution=0, flips=0)
    for j in np.nonzero(sane)[0]:
        st, sr = int(out["status"][j]), int(ref["status"][j])
        if st != sr:
            assert allow_status_flip_at_max_iter and {st, sr} <= {SOLVED_INACC, MAX_ITER} and int(out["iters"][j]) == int(ref["iters"][j]), (int(j), st, sr)
            counts["flips"] += 1
        if int(out["iters"][j]) != int(ref["iters"][j]):
            assert class_d(w, kind, int(j), out, ref, settings, params, limits), (int(j), st, sr, int(out["iters"][j]), int(ref["iters"][j]))
            counts["D"] += 1
        fo, fr = np.isfinite(out["uPred"][j]).all(), np.isfinite(ref["uPred"][j]).all()
        assert fo == fr, (int(j), "finite", fo, fr)
        if not fo:
            counts["no_solution"] += 1
            continue
        d = max(float(np.max(np.abs(out["uPred"][j] - ref["uPred"][j]))), float(np.max(np.abs(out["xPred"][j] - ref["xPred"][j])) / max(1.0, float(np.max(np.abs(ref["xPred"][j]))))))
        polished = st == SOLVED and "polish" in out and int(out["polish"][j]) == 1
        if d <= 1e-6:
            counts["A" if polished else "B"] += 1
        elif not polished and d <= 2e-4:
            counts["B"] += 1
        else:
            r = outlier_report(w, kind, int(j), out, ref, settings, params, limits)
            assert r["class"] == "C", (int(j), r)
            counts["C"] += 1
    return counts


# ---- the reported words: resid[B][4] = (pri_res, dua_res, obj_val, rho_final) -------------------------------------------------
# Classes of check_resid, decided by status, polish flag and iteration count alone (those are equal to the oracle's on every
# instance compared, so both sides fall in the same class):
#   A  SOLVED with an accepted polish: the words are the polished point's;
#   B  a solution that is the ADMM iterate of a run that ended before the cap (SOLVED with the polish off or rejected -- flag 0 /
#      -1 --, SOLVED_INACCURATE): the words are the iterate's;
#   C  ran to the cap (iterations = max_iter, MAX_ITER_REACHED or SOLVED_INACCURATE): an unconverged iterate;
#   D  no solution (PRIMAL / DUAL INFEASIBLE, exact or inaccurate): obj_val is +-1e30, the residuals are the last iterate's.
#
# The figures.  ORACLE_DEV_*: the oracle's reported words against the long double recomputation from the point it returns (no
# ADMM involved).  ORDER_DEV_*: the oracle against itself under its two elimination orders of the same KKT matrix (the stage-wise
# order of tick_batch_qp against solve_qp's RCM order), the round-off yardstick of each word.  Each is the maximum over the nine
# workloads of tests/test_gpu_settings.py, RESID_CASES and RESID_OWN_CASES, measured by tests/test_resid_host.py, which holds every constant
# between the measured value (beside it) and twice that.  A device bound is 100 x the oracle's own figure (RESID_MARGIN), as for the
# observer design and the track edges.
RESID_MARGIN = 100.0
RESID_CASES = [None, "scaling0", "scaling3", "combined", "nopolish", "delta1e-4", "eps_a1e-2_r1e-4", "max60", "chk40_adp15_max130",
               "chk0_max90", "adp0", "norho", "max1"]
# a case of this rule set's own, beside those of tests/test_gpu_settings.py: max_iter off the check grid and ON the rho grid (late_rho)
RESID_OWN_CASES = {"chk40_adp15_max75": dict(check_termination=40, adaptive_rho_interval=15, max_iter=75)}
# (case, workload) -> instances under a rule of their own: the oracle-free figures only, no comparison with the oracle's words.
#   scaling0 / planner N = 25 #63: BEYOND_BARS "capped" of tests/test_gpu_settings.py -- unscaled, at the cap, the oracle's own iterate
#   has a primal residual of 8 and carries nothing: its two elimination orders differ by 0.97 / 0.98 / 1.0 relative in pri_res /
#   dua_res / rho_final (and its own dua_res by 9 % from the long double one: |Pz|, |A'y| ~ 1e6 cancel).
RESID_NAMED = {("scaling0", "plan25"): [63]}
# (case, workload) -> polished instances whose DEVICE dua_res is beyond ("dua", "A") and held to the rule "dua_floor" instead.
#   combined (polish_refine_iter = 1) / controller N = 10 #10, #52, planner N = 30 #0 (the two-wave MFMA kernel, variant 2, alone):
#   the device's polish solves K_pol = P + delta I + A_act' A_act / delta (admm_solve.hip, polish), the oracle the reduced KKT system
#   with a -delta I block.  The two are equal in exact arithmetic; the weights 1 / delta = 1e6 leave a round-off of eps64 / delta times
#   the terms of the dual residual in the unrefined solve, which each refinement step shrinks: with OSQP's three steps the two sides
#   agree to 3e-11 of the threshold under every other case, with the single step of "combined" the remainder shows (891 polished
#   instances per pass over the routes: all others within the bar, these at 8.0e-8 .. 1.4e-7 of the threshold against 7.5e-8).  The rule:
#   |dua_res - oracle's| <= (eps64 / delta) max(|Pz|, |A'y|, |q|) -- one rounding error of the weighted system -- and every other word
#   of the instance at the class's bars.
RESID_POLISH_FLOOR = {("combined", "ctrl10"): [10, 52], ("combined", "plan30"): [0]}
OSQP_INFTY = 1e30
LD = np.longdouble

# the oracle's words against the long double recomputation from its own point (key of resid_figures -> figure, measured beside it)
ORACLE_DEV_OBJ_A = 2.5e-15          # 2.408e-15  relative, max(1, |obj|)
ORACLE_DEV_OBJ_B = 3.1e-15          # 2.972e-15
ORACLE_DEV_OBJ_C = 2.5e-14          # 2.417e-14  (chk40_adp15_max130, planner N = 30 #44)
ORACLE_DEV_PRI_A = 2.7e-6           # 2.641e-06  |pri_res - violation| / max(1, |Az|): OSQP's polished pri_res is |Az - clip(Az + y)|, which
#                                     exceeds the violation wherever an active row sits a regularisation step inside its bound (adp0,
#                                     controller N = 20 #40; 8e-16 on most instances).  The tight pin of a polished pri_res is ("pri", "A").
ORACLE_DEV_PRI_EXCESS_B = 2.3e-16   # 2.254e-16  max(0, violation - pri_res) / max(1, |Az|): the round-off of A z alone (z_ADMM is inside the
ORACLE_DEV_PRI_EXCESS_C = 8.8e-16   # 8.708e-16  bounds, so the violation cannot exceed pri_res in exact arithmetic)
ORACLE_DEV_DUA_A = 6.6e-12          # 6.482e-12  absolute (host only: the device returns no duals)
ORACLE_DEV_DUA_B = 1.1e-6           # 1.079e-06  relative (nopolish, controller N = 8 #9: dua_res 1e-9 of |Pz|)
ORACLE_DEV_DUA_C = 1.7e-9           # 1.595e-09  relative
# the oracle under its two elimination orders
ORDER_DEV_OBJ_A = 4.0e-10           # 3.915e-10  relative, max(1, |obj|) (combined, planner N = 30 #14)
ORDER_DEV_OBJ_B = 3.9e-10           # 3.822e-10
ORDER_DEV_PRI_A = 7.4e-9            # 7.288e-09  in units of the instance's termination threshold
ORDER_DEV_DUA_A = 7.5e-10           # 7.410e-10
ORDER_DEV_PRI_B = 1.6e-6            # 1.531e-06  relative to the reference's
ORDER_DEV_DUA_B = 1.4e-5            # 1.330e-05
ORDER_DEV_PRI_C = 2.0e-4            # 1.913e-04  (adp0, planner N = 25 #63, at the cap)
ORDER_DEV_DUA_C = 1.4e-5            # 1.354e-05
ORDER_DEV_PRI_D = 1.3e-10           # 1.267e-10
ORDER_DEV_DUA_D = 6.7e-7            # 6.575e-07
ORDER_DEV_RHO_A = 1.4e-5            # 1.317e-05  (chk0_max90, controller N = 8 #28)
ORDER_DEV_RHO_B = 3.0e-7            # 2.969e-07
ORDER_DEV_RHO_C = 9.0e-7            # 8.977e-07
ORDER_DEV_RHO_D = 5.2e-7            # 5.166e-07
RESID_ORACLE_DEV = {("obj_own", "A"): ORACLE_DEV_OBJ_A, ("obj_own", "B"): ORACLE_DEV_OBJ_B, ("obj_own", "C"): ORACLE_DEV_OBJ_C,
                    ("pri_own", "A"): ORACLE_DEV_PRI_A, ("pri_excess", "B"): ORACLE_DEV_PRI_EXCESS_B, ("pri_excess", "C"): ORACLE_DEV_PRI_EXCESS_C,
                    ("dua_own", "A"): ORACLE_DEV_DUA_A, ("dua_own", "B"): ORACLE_DEV_DUA_B, ("dua_own", "C"): ORACLE_DEV_DUA_C}
RESID_ORDER_DEV = {("obj", "A"): ORDER_DEV_OBJ_A, ("obj", "B"): ORDER_DEV_OBJ_B, ("obj", "D"): 0.0,
                   ("pri", "A"): ORDER_DEV_PRI_A, ("pri", "B"): ORDER_DEV_PRI_B, ("pri", "C"): ORDER_DEV_PRI_C, ("pri", "D"): ORDER_DEV_PRI_D,
                   ("dua", "A"): ORDER_DEV_DUA_A, ("dua", "B"): ORDER_DEV_DUA_B, ("dua", "C"): ORDER_DEV_DUA_C, ("dua", "D"): ORDER_DEV_DUA_D,
                   ("rho", "A"): ORDER_DEV_RHO_A, ("rho", "B"): ORDER_DEV_RHO_B, ("rho", "C"): ORDER_DEV_RHO_C, ("rho", "D"): ORDER_DEV_RHO_D}
# the device's bounds: obj of class D is word for word (0), as is rho where no update can run (check_resid)
RESID_BOUNDS = {k: RESID_MARGIN * v for d in (RESID_ORACLE_DEV, RESID_ORDER_DEV) for k, v in d.items()}
RESID_BOUNDS[("dua_floor", "A")] = 1.0      # (in units of the rule's own allowance: RESID_POLISH_FLOOR)


def _ld(a):
    return np.asarray(a.todense() if hasattr(a, "todense") else a, float).astype(LD)


def resid_class(status, polish, iters, max_iter):
    if status in NO_SOLUTION:
        return "D"
    if status == SOLVED and polish == 1:
        return "A"
    if iters == max_iter and status in (MAX_ITER, SOLVED_INACC):
        return "C"
    return "B"


def recomputed(qp, z, y=None):
    """In long double, from a point alone: the objective 1/2 z'Pz + q'z, the violation |Az - clip(Az, l, u)|_inf, max(1, |Az|_inf)
    (the scale of the violation's round-off) and, given the duals, |Pz + q + A'y|_inf."""
    Pm, Am, q, z = _ld(qp.P), _ld(qp.A), _ld(qp.q), np.asarray(z, float).astype(LD)
    Pz, Az = Pm @ z, Am @ z
    lo, hi = np.maximum(_ld(qp.l), -LD(OSQP_INFTY)), np.minimum(_ld(qp.u), LD(OSQP_INFTY))
    inf = lambda v: np.max(np.abs(v), initial=LD(0))
    out = dict(obj=LD(0.5) * (z @ Pz) + q @ z, viol=inf(Az - np.clip(Az, lo, hi)), scale=max(LD(1), inf(Az)))
    if y is not None:
        out["dua"] = inf(Pz + q + Am.T @ np.asarray(y, float).astype(LD))
    return out


def termination_thresholds(qp, z, y, settings=None):
    """OSQP's termination thresholds of an instance at the point (z, y): eps_abs + eps_rel max(|Az|, |clip(Az)|) for the primal
    residual, eps_abs + eps_rel max(|Pz|, |A'y|, |q|) for the dual one (float64: they only set a unit)."""
    s = dict(eps_abs=1e-3, eps_rel=1e-3); s.update({k: v for k, v in (settings or {}).items() if k in s})
    Pm = np.asarray(qp.P.todense() if hasattr(qp.P, "todense") else qp.P, float)
    Am = np.asarray(qp.A.todense() if hasattr(qp.A, "todense") else qp.A, float)
    inf = lambda v: float(np.max(np.abs(v), initial=0.0))
    Az = Am @ z
    return (s["eps_abs"] + s["eps_rel"] * max(inf(Az), inf(np.clip(Az, qp.l, qp.u))),
            s["eps_abs"] + s["eps_rel"] * max(inf(Pm @ z), inf(Am.T @ y), inf(qp.q)))


def _rel(a, b, floor=0.0):
    a, b = float(a), float(b)
    return 0.0 if a == b else abs(a - b) / max(abs(b), floor)


def rho_is_fixed(settings=None):
    """No rho update can run: adaptive_rho = 0, adaptive_rho_interval = 0, or a cap below the first update.  rho_final is then the
    configured rho, word for word."""
    s = dict(adaptive_rho=1, adaptive_rho_interval=25, max_iter=4000); s.update({k: v for k, v in (settings or {}).items() if k in s})
    return not s["adaptive_rho"] or s["adaptive_rho_interval"] <= 0 or s["max_iter"] < s["adaptive_rho_interval"]


def late_rho(status, iters, settings=None):
    """The device's one meant difference from OSQP in rho_final (docs/HISTORY.md, "Loop schedule against the oracle").  When max_iter
    is off the check grid but on the rho grid, OSQP updates rho on the last iteration BEFORE its closing check (osqp_ref.c: the
    update sits inside the loop, the closing update_info / check_termination behind it); the device's closing check is the loop's
    own and precedes the update, so a run that the closing check ENDS (SOLVED or an exact certificate at iters = max_iter) skips
    that update and reports the rho of iteration max_iter - 1.  A run the closing check leaves unsolved (MAX_ITER_REACHED, or
    SOLVED_INACCURATE by the 10 eps test behind it) performs the update on both sides.  None of RESID_CASES has max_iter on the rho
    grid (130 / 15, 60 / 25, 90 / 25); tests/test_gpu_resid.py adds a case that has (75 / 15, checks every 40)."""
    s = dict(adaptive_rho=1, adaptive_rho_interval=25, max_iter=4000, check_termination=25)
    s.update({k: v for k, v in (settings or {}).items() if k in s})
    chk, adp, cap = s["check_termination"], s["adaptive_rho_interval"], s["max_iter"]
    off_grid = chk <= 0 or cap % chk != 0
    return bool(s["adaptive_rho"] and adp > 0 and cap % adp == 0 and off_grid and iters == cap and status not in (MAX_ITER, SOLVED_INACC))


def resid_figures(qp, cls, z, y, resid, ref_resid=None, thr=None):
    """The deviations of one instance's four words, keyed (quantity, class).  Oracle-free ("own": from the point z, and y where
    the caller has the duals): obj_own relative to max(1, |obj|); pri_own (A) |pri_res - violation| and pri_excess (B, C)
    max(0, violation - pri_res), both over max(1, |Az|_inf); dua_own absolute (A) or relative (B, C).  Against ``ref_resid``:
    obj relative to max(1, |obj|) (A, B; D: 0 if the words are equal, else inf); pri / dua in units of the termination threshold
    ``thr`` (A: both sides are at round-off) or relative to the reference's (B, C, D); rho relative."""
    f = {}
    if cls != "D":
        r = recomputed(qp, z, y)
        f[("obj_own", cls)] = float(abs(LD(resid[2]) - r["obj"]) / max(LD(1), abs(r["obj"])))
        if cls == "A":
            f[("pri_own", cls)] = float(abs(LD(resid[0]) - r["viol"]) / r["scale"])
        else:
            f[("pri_excess", cls)] = float(max(LD(0), r["viol"] - LD(resid[0])) / r["scale"])
        if y is not None:
            f[("dua_own", cls)] = float(abs(LD(resid[1]) - r["dua"])) if cls == "A" else float(abs(LD(resid[1]) - r["dua"]) / max(r["dua"], LD(1e-300)))
    if ref_resid is not None:
        if cls == "D":
            f[("obj", cls)] = 0.0 if resid[2] == ref_resid[2] and abs(ref_resid[2]) == OSQP_INFTY else float("inf")
        elif cls != "C":
            f[("obj", cls)] = abs(resid[2] - ref_resid[2]) / max(1.0, abs(ref_resid[2]))
        for i, name in ((0, "pri"), (1, "dua")):
            f[(name, cls)] = abs(resid[i] - ref_resid[i]) / thr[i] if cls == "A" else _rel(resid[i], ref_resid[i], 1e-300)
        f[("rho", cls)] = _rel(resid[3], ref_resid[3])
    return f


def check_resid(w, kind, out, ref, yard=None, settings=None, qps=None, named=(), late_rule=True, polish_floor=()):
    """The rule set of the reported words on a batch: ``out["resid"]`` (B, 4) against the long double recomputation from ``out``'s own
    point and against ``ref["resid"]`` (oracle/osqp_ref.py tick_batch_qp under the same ``settings``).  ``yard``: the bound of every
    (quantity, class) of resid_figures (RESID_BOUNDS for the device); None measures without asserting (tests/test_resid_host.py: the
    oracle against itself).  ``qps``: the instances' QPs if the caller has them (indexed modulo their number: tiled batches).

    Compared: the instances of check_batch's ``sane`` mask whose status, iteration count and polish flag equal the reference's; the
    others are check_batch's business and are listed in ``left_out``.  A row without an answer on the ``out`` side (UNSOLVED) must
    hold four NaN.  rho_final: relative to the reference's; exactly the configured rho where no update can run (rho_is_fixed);
    on a late_rho instance against the reference's rho one iteration earlier (its own solve with max_iter - 1; ``late_rule`` False
    switches the rule off: the oracle against itself).  ``named``: instances under a rule of their own (RESID_NAMED) -- the
    oracle-free figures only; ``polish_floor``: polished instances whose dua_res takes the rule of RESID_POLISH_FLOOR.
    Returns dict(counts, worst, where, left_out): instances per class, worst figure and its instance per (quantity, class)."""
    from oracle import osqp_ref as O
    st = dict(settings or {})
    cap = int(st.get("max_iter", w.get("max_iter", 4000)))
    B = out["status"].shape[0]
    sane = (ref["status"] != -10) & ~(np.isnan(ref["uPred"]).any(axis=(1, 2)) & (ref["status"] == 1))
    rep = dict(counts=dict(A=0, B=0, C=0, D=0, unsolved=0, late_rho=0), worst={}, where={}, left_out=[])
    fixed, rho0 = rho_is_fixed(st), float(st.get("rho", 0.1))
    for j in range(B):
        if int(out["status"][j]) == -10:
            assert np.isnan(out["resid"][j]).all(), (j, "a row without an answer reports", out["resid"][j])
            rep["counts"]["unsolved"] += 1
            continue
        key = lambda d: (int(d["status"][j]), int(d["iters"][j]), int(d["polish"][j]))
        if not sane[j] or key(out) != key(ref):
            rep["left_out"].append(j)
            continue
        s_, it, pol = key(out)
        cls = resid_class(s_, pol, it, cap)
        rep["counts"][cls] += 1
        qp = qps[j % len(qps)] if qps is not None else instance_qp(w, kind, j)
        z = np.concatenate([out["xPred"][j].reshape(-1), out["uPred"][j].reshape(-1)])
        thr = termination_thresholds(qp, ref["z"][j], ref["y"][j], st) if cls == "A" else None
        rr = np.array(ref["resid"][j], float)
        if j % (len(qps) if qps is not None else B) in named:
            rr = None
        elif late_rule and late_rho(s_, it, st):
            N = int(w["N"])
            d = np.asarray(w["u_old"]).reshape(B, -1).shape[1] - 2 if kind == "controller" else 0
            perm = O.ctrl_delay_ordering(N, d) if kind == "controller" else O.plan_ordering(N)
            r = O.solve_qp(qp.P, qp.q, qp.A, qp.l, qp.u, perm=perm, **dict(O.osqp_settings(st), max_iter=cap - 1))
            assert r.info.iter == cap - 1, (j, r.info.iter)
            rr[3] = r.info.rho_final
            rep["counts"]["late_rho"] += 1
        f = resid_figures(qp, cls, z, out["y"][j] if "y" in out and rr is not None else None, out["resid"][j], rr, thr)
        if cls == "A" and j % (len(qps) if qps is not None else B) in polish_floor:
            s = dict(eps_abs=1e-3, eps_rel=1e-3, polish_delta=1e-6); s.update({k: v for k, v in st.items() if k in s})
            allow = np.finfo(float).eps / s["polish_delta"] * (thr[1] - s["eps_abs"]) / s["eps_rel"]
            del f[("dua", "A")]
            f[("dua_floor", "A")] = abs(out["resid"][j, 1] - rr[1]) / allow
        if fixed and rr is not None:
            f[("rho", cls)] = 0.0 if out["resid"][j, 3] == rho0 else float("inf")
        for k, v in f.items():
            if not v <= rep["worst"].get(k, -1.0):
                rep["worst"][k], rep["where"][k] = v, j
            if yard is not None:
                assert v <= yard[k], (j, k, v, yard[k], "device", list(out["resid"][j]), "oracle", list(ref["resid"][j]))
    return rep


def merge_resid_reports(reports):
    """Counts summed, worst figures maximised over check_resid reports."""
    tot = dict(counts={}, worst={}, left_out=0)
    for r in reports:
        for k, v in r["counts"].items():
            tot["counts"][k] = tot["counts"].get(k, 0) + v
        for k, v in r["worst"].items():
            tot["worst"][k] = max(tot["worst"].get(k, 0.0), v)
        tot["left_out"] += len(r["left_out"])
    return tot
