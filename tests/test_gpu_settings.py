"""GPU: what a user configures -- OSQP settings away from their defaults, an asymmetric vehicle, other QP limits -- against the
CPU oracle (oracle/osqp_ref.py tick_batch_qp: the reference's QP of every instance, solved by the OSQP restatement under the
same settings, with the C ticks' stage-wise elimination order).

Every other GPU test runs OSQP's defaults on the reference's symmetric vehicle (lf = lr, Cf = Cr): a setting hard-coded to its
default in one solve instantiation, two settings swapped, lf swapped with lr would pass them all.  Here:
  a. each single-axis departure of SETTINGS (and one combined case) on every solve route of DESIGN section 4 -- the compile-time
     kernels of the controller (N = 8, 10, 20 and its variants, a steering delay) and the planner (N = 20, 30, 40 and theirs, the
     batch-size-selected forms at N = 30), the run-time-horizon kernels and the whole-CU tail kernel through the deferral;
  b. non-vacuity on the oracle side: each departure changes iteration counts or solutions against the defaults, each swap-
     detecting pair changes statuses or iteration counts when swapped;
  c. polished device solutions under each departure against the active-set optimum (oracle/kkt_cert.py, no ADMM involved);
  d. the vehicle of tests/golden/params.npz: LPV / seed-mode / solves / plant / lap-0 fleet;
  e. other controller limits and planner boxes, active at the optimum.
Rules: tests/_tolerance.py (check_batch).  Batch sizes are ragged.  Class counts are printed per case (run with -s)."""
import numpy as np
import pytest

from oracle import kkt_cert, lpv_ref as L, osqp_ref as O, plant_ref as PR
from tests import _tolerance as T
from tests._golden import load
from tests.test_gpu_horizons import ctrl_workload, delay_workload, plan_workload, relclose

pytestmark = pytest.mark.gpu

NTHREADS = 16

SETTINGS = {
    "alpha1.0": dict(alpha=1.0), "alpha1.8": dict(alpha=1.8), "sigma1e-4": dict(sigma=1e-4),
    "rho0.01": dict(rho=0.01), "rho1": dict(rho=1.0),
    "eps_a1e-4_r1e-2": dict(eps_abs=1e-4, eps_rel=1e-2), "eps_a1e-2_r1e-4": dict(eps_abs=1e-2, eps_rel=1e-4),
    "inf_p1e-6_d1e-2": dict(eps_prim_inf=1e-6, eps_dual_inf=1e-2), "inf_p1e-2_d1e-6": dict(eps_prim_inf=1e-2, eps_dual_inf=1e-6),
    "delta1e-8": dict(polish_delta=1e-8), "delta1e-4": dict(polish_delta=1e-4),
    "refine0": dict(polish_refine_iter=0), "refine1": dict(polish_refine_iter=1), "refine7": dict(polish_refine_iter=7),
    "rhotol2": dict(adaptive_rho_tolerance=2.0), "rhotol10": dict(adaptive_rho_tolerance=10.0),
    "scaling0": dict(scaling=0), "scaling1": dict(scaling=1), "scaling3": dict(scaling=3), "scaling15": dict(scaling=15),
    "combined": dict(alpha=1.2, sigma=1e-5, scaling=5, polish_refine_iter=1, adaptive_rho_tolerance=3.0),
}
SWAPS = [("eps_a1e-4_r1e-2", "eps_a1e-2_r1e-4"), ("inf_p1e-6_d1e-2", "inf_p1e-2_d1e-6")]
# the loop schedule (tests/test_gpu_schedule.py): when Solver::run checks, adapts rho, stops and polishes.  At the defaults (25 / 25 /
# 4000 / on / on) the check grid, the rho grid and the cap coincide; each case here takes them apart another way.
SCHEDULES = {
    "chk1": dict(check_termination=1),
    "chk7_adp10": dict(check_termination=7, adaptive_rho_interval=10),
    "chk10_adp7": dict(check_termination=10, adaptive_rho_interval=7),
    "adp40": dict(adaptive_rho_interval=40),
    "chk40_adp15_max130": dict(check_termination=40, adaptive_rho_interval=15, max_iter=130),
    "chk0_max90": dict(check_termination=0, max_iter=90),
    "max60": dict(max_iter=60), "max100": dict(max_iter=100), "max1": dict(max_iter=1),
    "adp0": dict(adaptive_rho_interval=0), "norho": dict(adaptive_rho=0), "nopolish": dict(polish=0),
}
SCHEDULE_SWAPS = [("chk7_adp10", "chk10_adp7")]

# workload name -> (kind, builder); B ragged.  The planner N = 30 forms selected by batch size (two-wave MFMA at B >= 512, the
# global-scalings kernel of variant 7 at B > 512) run "plan30" tiled 8 times (536 instances, the tiled oracle).
WORKLOADS = {
    "ctrl8": ("controller", lambda: ctrl_workload(71, 8, seed=8101)),
    "ctrl10": ("controller", lambda: ctrl_workload(71, 10, seed=8102)),
    "ctrl13": ("controller", lambda: ctrl_workload(71, 13, seed=8103)),
    "ctrl20": ("controller", lambda: ctrl_workload(71, 20, seed=8104)),
    "ctrl20d3": ("controller", lambda: delay_workload(71, 20, 3, seed=8105)),
    "plan20": ("planner", lambda: plan_workload(67, 20, seed=8201)),
    "plan25": ("planner", lambda: plan_workload(67, 25, seed=8202)),
    "plan30": ("planner", lambda: plan_workload(67, 30, seed=8203)),
    "plan40": ("planner", lambda: plan_workload(67, 40, seed=8204)),
}
TILE = 8
# route: (workload, kernel_variant, tiled, deferral (defer_after) or 0)
ROUTES = [("ctrl8", 0, False, 0), ("ctrl10", 0, False, 0), ("ctrl13", 0, False, 0),
          ("ctrl20", 0, False, 0), ("ctrl20", 2, False, 0), ("ctrl20", 3, False, 0), ("ctrl20", 9, False, 0), ("ctrl20d3", 0, False, 0),
          ("ctrl20", 0, False, 25),
          ("plan20", 0, False, 0), ("plan20", 3, False, 0), ("plan20", 9, False, 0), ("plan20", 0, False, 25),
          ("plan25", 0, False, 0),
          ("plan30", 0, False, 0), ("plan30", 2, False, 0), ("plan30", 3, False, 0), ("plan30", 4, False, 0), ("plan30", 5, False, 0),
          ("plan30", 0, True, 0), ("plan30", 7, True, 0),
          ("plan40", 0, False, 0), ("plan40", 3, False, 0), ("plan40", 6, False, 0)]

_W, _QPS, _ORC = {}, {}, {}


def workload(name):
    if name not in _W:
        kind, make = WORKLOADS[name]
        w = make()
        _W[name] = w
        _QPS[name] = []
        for j in range(w["x0"].shape[0]):
            try:
                _QPS[name].append(O.instance_qp(w, kind, j))
            except ValueError:
                _QPS[name].append(None)
    return WORKLOADS[name][0], _W[name]


def settings_of(case):
    """The settings dict of a case of SETTINGS or SCHEDULES (None: the defaults)."""
    if case is None:
        return None
    return SETTINGS[case] if case in SETTINGS else SCHEDULES[case]


def oracle(name, case):
    """tick_batch_qp of one workload under one settings case (None: defaults), computed once and shared by every route."""
    if (name, case) not in _ORC:
        kind, w = workload(name)
        _ORC[(name, case)] = O.tick_batch_qp(w, kind, settings=settings_of(case), nthreads=NTHREADS, qps=_QPS[name])
    return _ORC[(name, case)]


def tiled(w, n):
    B = w["x0"].shape[0]
    return {k: (np.concatenate([v] * n) if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == B and k != "track" else v)
            for k, v in w.items()}


def tiled_ref(ref, n):
    return {k: np.concatenate([v] * n) for k, v in ref.items()}


def device_solve(w, variant=0, defer_after=0, params=None, defer_pool=None, **settings):
    import lpvmpc
    d = int(np.asarray(w["u_old"]).reshape(w["x0"].shape[0], -1).shape[1] - 2) if w["kind"] == "controller" else 0
    eng = lpvmpc.BatchedSolver(w["kind"], w["N"], w["dt"], w["Q"], w["R"], w["dR"], L_cf=w["L_cf"], track=w["track"], params=params,
                               steering_delay=d, **settings)
    eng.set_option("kernel_variant", variant)
    if defer_after:
        B = w["x0"].shape[0]
        eng.reserve(B)
        eng.set_option("defer_after", defer_after); eng.set_option("defer_budget", -1); eng.set_option("defer_pool", defer_pool or B)
    out = eng.solve(w["x0"], w["u_prev"], w["vel_ref"], w["curv_s"], w["u_old"], w["max_ey"], w["cf_new"], w["lap"])
    parked = eng.defer_stats()[0] if defer_after else 0
    eng.close()
    return out, parked


def _report(tag, counts, out):
    print("%s iters %d..%d %s" % (tag, int(np.min(out["iters"])), int(np.max(out["iters"])), counts))


# ---- a. the settings matrix on every route -----------------------------------------------------------------------------------
# (case, workload): instances beyond their class's bar while status and iteration count equal the oracle's, each held to a rule of
# its own that states why (every other instance of those batches, on every route, to check_batch):
#   rhotol2 / planner N = 40 #23  "converged": polish failed on both sides after 675 iterations, |du| 3.5e-4 (class B: 2e-4): both
#                                 points meet the termination tolerance and their objectives agree to 1e-4;
#   scaling0 / planner N = 25 #63 "capped": unscaled, both at the cap, |du| 1.9 (class C: 2e-2): the oracle's own iterate is far from
#                                 feasible (primal residual 8), the point carries nothing;
#   refine0 / controller N = 20 #31 "polish": polish_refine_iter = 0 -- the polished point is the unrefined delta-regularised solve,
#                                 and its acceptance test (residuals both smaller) is decided differently: the device's polish
#                                 fails (-1), the oracle's succeeds (1).  The device then returns its ADMM iterate: held to the
#                                 oracle's ADMM iterate (the same solve without polish) at class B's bar.  Open (docs/HISTORY.md);
#   refine0 / controller N = 13 #60 "polished": both polish without refinement; the unrefined points agree to class B's bar.
BEYOND_BARS = {("rhotol2", "plan40"): ([23], "converged"), ("scaling0", "plan25"): ([63], "capped"),
               ("refine0", "ctrl20"): ([31], "polish"), ("refine0", "ctrl13"): ([60], "polished")}


def _beyond_bars(case, name, kind, w, out, ref, js, rule):
    st = settings_of(case)
    for j in js:
        assert int(out["status"][j]) == int(ref["status"][j]) and int(out["iters"][j]) == int(ref["iters"][j]), (case, name, j)
        du = float(np.max(np.abs(out["uPred"][j] - ref["uPred"][j])))
        if rule == "converged":
            r = T.outlier_report(w, kind, j, out, ref, settings=st)
            assert r["status"] == T.SOLVED and r["obj_gap"] <= 1e-4 and r["pri"] <= r["pri_tol"], (case, name, j, r)
        elif rule == "capped":
            r = T.outlier_report(w, kind, j, out, ref, settings=st)
            assert r["status"] == T.MAX_ITER and r["iters"] == st.get("max_iter", 4000) and r["pri_ref"] > 1.0, (case, name, j, r)
        elif rule == "polish":
            assert int(out["polish"][j]) == -1 and int(ref["polish"][j]) == 1, (case, name, j)
            qp = _QPS[name][j]
            perm = O.ctrl_delay_ordering(int(w["N"]), 0) if kind == "controller" else O.plan_ordering(int(w["N"]))
            r = O.solve_qp(qp.P, qp.q, qp.A, qp.l, qp.u, perm=perm, **dict(O.osqp_settings(st), polish=0))
            _, u_admm, _ = L.unpack_solution(r.x, 6 if kind == "controller" else 5, 2, int(w["N"]))
            e = float(np.max(np.abs(out["uPred"][j] - u_admm)))
            assert r.info.iter == int(out["iters"][j]) and e <= 2e-4, (case, name, j, e)
        else:
            assert int(out["polish"][j]) == 1 and int(ref["polish"][j]) == 1 and du <= 2e-4, (case, name, j, du)


def _drop(d, idx, B):
    keep = np.setdiff1d(np.arange(B), idx)
    return {k: (v[keep] if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == B and k != "track" else v) for k, v in d.items()}


@pytest.mark.parametrize("case", list(SETTINGS))
def test_settings_on_every_route(case):
    """Every route of the solve under one departure from OSQP's defaults: statuses and iteration counts equal to the oracle's under
    the same settings, solutions in classes A-D (BEYOND_BARS: the named instances under their own rules).  The deferred routes park every instance past 25 iterations:
    the whole-CU tail kernel (controller and planner N = 20) finishes them with the handle's settings."""
    st = SETTINGS[case]
    for name, variant, tile, defer in ROUTES:
        kind, w = workload(name)
        ref = oracle(name, case)
        if tile:
            w, ref = tiled(w, TILE), tiled_ref(ref, TILE)
        out, parked = device_solve(w, variant, defer, **st)
        if defer:
            assert parked >= 1, (name, parked)
        skip, rule = BEYOND_BARS.get((case, name), ([], None)) if not tile else ([], None)
        if skip:
            _beyond_bars(case, name, kind, w, out, ref, skip, rule)
            B = w["x0"].shape[0]
            w, out, ref = _drop(w, skip, B), _drop(out, skip, B), _drop(ref, skip, B)
        counts = T.check_batch(w, kind, out, ref, settings=st)
        _report("%s %s B=%d variant=%d defer=%d parked=%d" % (case, name, w["x0"].shape[0], variant, defer, parked), counts, out)


# ---- b. non-vacuity: oracle only, in tests/test_settings_host.py -------------------------------------------------------------


# ---- c. polished solutions against the active-set optimum --------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in SETTINGS if SETTINGS[c].get("polish_refine_iter", 3) > 0])
def test_polished_solutions_are_the_active_set_optimum(case):
    """On the default route of each workload, polished device solutions (up to 12 per workload) against the optimum of the active
    set the oracle names (kkt_cert.active_set_optimum: dense solves, no ADMM code), to 1e-6.  OSQP accepts a polish that improves
    the residuals, not only the exact optimum: without refinement, at a loose eps_rel or a large delta a polished point can sit
    1e-5..1e-2 from it (so on both sides).  The rule: wherever the oracle's polished point is the optimum, the device's is too, on at
    least 30 instances per case; the others are counted.  Not run at polish_refine_iter = 0: there a polished point is the
    unrefined delta-regularised solve, never the optimum (none of 102 on the oracle side), and the matrix above covers it."""
    st = settings_of(case)
    n = worst = off = 0
    for name in WORKLOADS:
        kind, w = workload(name)
        out, _ = device_solve(w, 0, 0, **st)
        ref = oracle(name, case)
        pol = np.nonzero((out["status"] == 1) & (out["polish"] == 1))[0][:12]
        for j in pol:
            qp = _QPS[name][j]
            z = np.concatenate([out["xPred"][j].reshape(-1), out["uPred"][j].reshape(-1)])
            try:
                xs, _, _ = kkt_cert.active_set_optimum(qp.P, qp.q, qp.A, qp.l, qp.u, ref["z"][j], ref["y"][j])
            except RuntimeError:
                continue
            scale = max(1.0, float(np.max(np.abs(xs))))
            if float(np.max(np.abs(ref["z"][j] - xs))) / scale > 1e-6:
                off += 1
                continue
            e = float(np.max(np.abs(z - xs))) / scale
            assert e <= 1e-6, (case, name, int(j), e)
            worst = max(worst, e); n += 1
    print("%s: %d polished solutions certified, max rel err %.2e; %d polished points not the optimum on the oracle side" % (case, n, worst, off))
    assert n >= 30, n


# ---- d. an asymmetric vehicle (tests/golden/params.npz) ----------------------------------------------------------------------
def vehicle():
    g = load("params")
    return {k: float(g[k]) for k in ("lf", "lr", "m", "Iz", "Cf", "Cr", "mu")}


def swapped(p):
    return dict(p, lf=p["lr"], lr=p["lf"], Cf=p["Cr"], Cr=p["Cf"])


def test_vehicle_is_told_apart_from_its_mirror():
    """The oracle's solutions for the vehicle and for its lf <-> lr, Cf <-> Cr mirror differ by more than 1e-3: a swap on the
    device cannot pass the solve checks below."""
    veh = vehicle()
    for name in ("ctrl20", "plan30"):
        kind, w = workload(name)
        a = O.tick_batch_qp(w, kind, params=veh, nthreads=NTHREADS)
        b = O.tick_batch_qp(w, kind, params=swapped(veh), nthreads=NTHREADS)
        ok = np.isfinite(a["uPred"]).all(axis=(1, 2)) & np.isfinite(b["uPred"]).all(axis=(1, 2))
        d = float(np.max(np.abs(a["uPred"][ok] - b["uPred"][ok])))
        print("%s: vehicle against its mirror, max |du| %.3e" % (name, d))
        assert d > 1e-3, (name, d)


@pytest.mark.parametrize("kind,N", [("controller", 9), ("controller", 20), ("planner", 20), ("planner", 30)])
def test_vehicle_lpv_and_seed_mode(kind, N):
    """eng.lpv and eng.estimate_abc of a handle created with the vehicle against lpv_ref with it: 1e-12 of each array's largest
    magnitude; the mirror vehicle misses by far more."""
    import lpvmpc
    from lpvmpc import workloads
    veh = vehicle(); p = dict(L.DEFAULT_PARAMS, **veh); pm = dict(L.DEFAULT_PARAMS, **swapped(veh))
    B = 37
    w = ctrl_workload(B, N, seed=8300 + N, vary=True, vmin=1.2) if kind == "controller" else plan_workload(B, N, seed=8300 + N, vary=True)
    eng = workloads.make_solver(w, params=veh)
    if kind == "controller":
        S, A, Bm = eng.lpv(w["x0"], w["u_prev"], w["vel_ref"], w["curv_s"], cf_new=w["cf_new"], lap=w["lap"])
    else:
        S, A, Bm = eng.lpv(w["x0"], w["u_prev"], None, w["curv_s"])
    rng = np.random.default_rng(8400 + N)
    tab = w["track"]; Lt = float(tab[-1, 3] + tab[-1, 4])
    vx = rng.uniform(0.8, 3.0, (B, N)); vy = rng.normal(0, 0.05, (B, N)); wz = rng.normal(0, 0.3, (B, N))
    epsi = rng.normal(0, 0.1, (B, N)); ey = rng.normal(0, 0.1, (B, N)); s = rng.uniform(0.0, 0.99 * Lt, (B, N))
    delta = rng.uniform(-0.24, 0.24, (B, N))
    xx = np.stack([vx, vy, wz, epsi, s, ey], axis=2) if kind == "controller" else np.stack([vx, vy, wz, ey, epsi, s], axis=2)
    Ae, Be = eng.estimate_abc(xx, delta)
    eng.close()
    worst = mirror = 0.0
    for j in range(B):
        for pp, tol in ((p, 1e-12), (pm, None)):
            if kind == "controller":
                Sr, Ar, Br = L.ctrl_lpv_prediction(pp, w["dt"], N, tab, w["x0"][j], w["u_prev"][j], w["vel_ref"][j],
                                                   None if w["curv_s"] is None else w["curv_s"][j], w["cf_new"], w["lap"])
                Aer, Ber = L.ctrl_estimate_abc(pp, w["dt"], N, tab, xx[j], np.stack([delta[j], np.zeros(N)], axis=1))
            else:
                Sr, Ar, Br = L.plan_lpv_prediction(pp, w["dt"], N, tab, w["x0"][j], w["curv_s"][j], w["u_prev"][j])
                Aer, Ber = L.plan_estimate_abc(pp, w["dt"], N, tab, xx[j], delta[j])
            pairs = ((S[j], Sr, "states"), (A[j], Ar, "A"), (Bm[j], Br, "B"), (Ae[j], Aer, "abc A"), (Be[j], Ber, "abc B"))
            if tol is None:
                mirror = max(mirror, max(float(np.max(np.abs(g - r))) / max(1.0, float(np.max(np.abs(r)))) for g, r, _ in pairs))
            else:
                for got, want, what in pairs:
                    worst = max(worst, relclose(got, want, tol, "%s N=%d #%d %s" % (kind, N, j, what)))
    print("%s N=%d vehicle: lpv / seed-mode max rel err %.2e, against the mirror vehicle %.2e" % (kind, N, worst, mirror))
    assert mirror > 1e-3


@pytest.mark.parametrize("name,variant", [("ctrl8", 0), ("ctrl13", 0), ("ctrl20", 0), ("ctrl20", 9), ("ctrl20d3", 0),
                                          ("plan20", 0), ("plan25", 0), ("plan30", 0), ("plan40", 0)])
def test_vehicle_solves(name, variant):
    veh = vehicle()
    kind, w = workload(name)
    ref = O.tick_batch_qp(w, kind, params=veh, nthreads=NTHREADS)
    out, _ = device_solve(w, variant, 0, params=veh)
    counts = T.check_batch(w, kind, out, ref, params=veh)
    _report("vehicle %s variant=%d" % (name, variant), counts, out)


def test_vehicle_plant_step():
    """lpvmpc_plant_step_batch with the vehicle: the fixture's Simulator.f trajectory (the reference's own class), and 41 vehicles
    from random states under random inputs against plant_ref.simulator_f, 200 steps each, to 1e-11."""
    import lpvmpc
    g = load("params")
    veh = vehicle()
    sp = dict(PR.SIM_PARAMS, lf=veh["lf"], lr=veh["lr"], m=veh["m"], Iz=veh["Iz"], mu=float(g["sim_mu"]), dt=float(g["sim_dt"]))
    eng = lpvmpc.BatchedSolver("controller", 20, 1 / 30.0, np.eye(6), np.eye(2), np.ones(2), params=veh)
    B = 42
    rng = np.random.default_rng(8500)
    st = np.column_stack([rng.uniform(-3, 3, B), rng.uniform(-3, 3, B), rng.uniform(0.1, 3.0, B), rng.normal(0, 0.1, B),
                          rng.normal(0, 0.5, B), rng.normal(0, 0.5, B), rng.uniform(-3, 3, B), rng.normal(0, 0.5, B)])
    st[0] = g["sim_init"]
    ref = st.copy()
    worst = 0.0
    for k in range(200):
        u = np.column_stack([rng.uniform(-1.0, 2.0, B), rng.uniform(-0.25, 0.25, B)])
        u[0] = g["sim_u"][k]
        st = eng.plant_step(st, u, n_sub=1, dt_sim=sp["dt"], mu_sim=sp["mu"])
        ref = np.array([PR.simulator_f(ref[b], u[b], sp) for b in range(B)])
        for got, want in ((st, ref), (st[0], g["sim_states"][k])):
            e = float(np.max(np.abs(got - want)) / max(1.0, float(np.max(np.abs(want)))))
            assert e <= 1e-11, (k, e)
            worst = max(worst, e)
    eng.close()
    print("vehicle plant: 200 steps, max rel err %.2e" % worst)


def test_vehicle_lap0_fleet_matches_the_host_replay():
    """A lap-0 fleet (lpvmpc_cl_init / cl_tick: seed ticks, then LPV path following, 7 plant steps per tick) of the vehicle against
    the host replay (tests/_race_ref.py RaceRef with the vehicle), 60 ticks, at the bars of the reference trace of the closed loop
    (test_gpu_closed_loop.py): equal statuses and iteration counts, plant / local state / command within 2e-6."""
    import lpvmpc
    from lpvmpc import workloads as W
    from tests._race_ref import RaceRef
    veh = vehicle()
    mp = lpvmpc.Map("L_shape", 0.2)
    B = 69
    rng = np.random.default_rng(8600)
    plant0 = np.zeros((B, 8)); plant0[:, 1] = rng.normal(0, 0.03, B); plant0[:, 2] = rng.uniform(0.8, 1.2, B); plant0[:, 6] = rng.normal(0, 0.03, B)
    Qp, Rp, dRp = W.CTRL_TUNINGS["path"]
    eng = lpvmpc.BatchedSolver("controller", 20, 1 / 30.0, Qp, Rp, dRp, track=mp.PointAndTangent, params=veh)
    eng.cl_init(plant0, mp.halfWidth, mp.slack, q9_swap=True, n_sub=7)
    ref = RaceRef(mp.PointAndTangent, plant0, laps=1, half_width=mp.halfWidth, slack=mp.slack, params=veh)
    worst = 0.0
    for t in range(60):
        eng.cl_tick(1); ref.tick()
        o = eng.cl_read()
        assert np.all(ref.phase == 0), t
        assert np.array_equal(o["status"], ref.status), (t, np.nonzero(o["status"] != ref.status)[0])
        assert np.array_equal(o["iters"], ref.iters), (t, np.nonzero(o["iters"] != ref.iters)[0])
        d = max(float(np.max(np.abs(o["plant"] - ref.plant))), float(np.max(np.abs(o["local"] - ref.local))),
                float(np.max(np.abs(o["cmd"] - ref.cmd))))
        assert d <= 2e-6, (t, d)
        worst = max(worst, d)
    eng.close()
    print("vehicle lap-0 fleet: B=%d, 60 ticks, max difference %.2e" % (B, worst))


# ---- e. other limits ---------------------------------------------------------------------------------------------------------
CTRL_LIMITS = dict(vx_min=1.0, delta_max=0.2, a_max=0.7, a_min_abs=0.6)
PLAN_BOXES = dict(xmin=[0.9, -0.05, -1.2, -0.2, -0.3], xmax=[5.0, 0.04, 1.0, 0.2, 0.25], umin=[-0.2, -0.5], umax=[0.18, 1.5])


def _active(qp, z, rows, tol=1e-6):
    Az = np.asarray(qp.A, float)[rows] @ z
    return np.any((np.abs(Az - qp.u[rows]) <= tol) | (np.abs(Az - qp.l[rows]) <= tol))


@pytest.mark.parametrize("name,variant", [("ctrl13", 0), ("ctrl20", 0), ("ctrl20", 3), ("ctrl20d3", 0), ("plan20", 0), ("plan30", 0),
                                          ("plan40", 0)])
def test_limits(name, variant):
    """Controller limits (ctrl_vx_min / delta_max / a_max / a_min_abs) and planner boxes (plan_xmin / xmax / umin / umax) away
    from the reference's: the device against the oracle's QP with the same rows.  At the oracle's optimum one changed row kind is
    active on at least 10 % of the instances and every other kind but at most one on some instance (the run-time controller N = 13
    never brakes to -a_min_abs, the planners' tighter vy box keeps them off the steering box), so a device that kept a default
    there solves another QP."""
    kind, w = workload(name)
    N = int(w["N"])
    if kind == "controller":
        lim = CTRL_LIMITS
        st = dict(ctrl_vx_min=1.0, ctrl_delta_max=0.2, ctrl_a_max=0.7, ctrl_a_min_abs=0.6)
        groups = {"delta_max": [2 * N + 4 * k + r for k in range(N) for r in (0, 1)], "a_max": [2 * N + 4 * k + 2 for k in range(N)],
                  "a_min_abs": [2 * N + 4 * k + 3 for k in range(N)]}
    else:
        lim = PLAN_BOXES
        st = dict(plan_xmin=lim["xmin"], plan_xmax=lim["xmax"], plan_umin=lim["umin"], plan_umax=lim["umax"])
        me, nz = (N + 1) * 5, (N + 1) * 5 + 2 * N
        groups = {"vy": [me + k * 5 + 1 for k in range(1, N + 1)], "wz": [me + k * 5 + 2 for k in range(1, N + 1)],
                  "epsi": [me + k * 5 + 4 for k in range(1, N + 1)], "delta": [me + me + 2 * k for k in range(N)],
                  "a": [me + me + 2 * k + 1 for k in range(N)]}
        assert me + me + 2 * N == me + nz
    ref = O.tick_batch_qp(w, kind, limits=lim, nthreads=NTHREADS)
    share = {}
    for g, rows in groups.items():
        n = 0
        for j in np.nonzero(ref["status"] == 1)[0]:
            qp = O.instance_qp(w, kind, j, limits=lim)
            n += int(_active(qp, ref["z"][j], rows))
        share[g] = n / w["x0"].shape[0]
    if kind == "controller":
        # vx_min: the speeds follow vel_ref, so the rows bind on stage 0, pinned to x0: an instance starting below vx_min is
        # PRIMAL INFEASIBLE (a device that ignored ctrl_vx_min would solve it)
        ref0 = O.tick_batch_qp(w, kind, limits=dict(lim, vx_min=0.01), nthreads=NTHREADS)
        share["vx_min"] = float(np.mean((ref["status"] == -3) & (ref0["status"] == 1)))
    out, _ = device_solve(w, variant, 0, **st)
    counts = T.check_batch(w, kind, out, ref, limits=lim)
    _report("limits %s variant=%d active shares %s" % (name, variant, {k: round(v, 2) for k, v in share.items()}), counts, out)
    assert max(share.values()) >= 0.1 and sum(v > 0 for v in share.values()) >= len(share) - 1, share
