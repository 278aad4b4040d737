"""GPU: every horizon, steering delay and kernel route the library accepts, against the CPU oracle.

The parity tests (test_gpu_parity.py) sit on the horizons with a specialised kernel and on steeringDelay 0.  Here the
horizons without one run the run-time-horizon kernels <6,0,1> / <5,0,1> at odd and even N (stage parity: L_k kept transposed
for odd k, the two-sided elimination's join at N/2, the ping-pong passes of the equilibration), the steering delay is pinned
on every kernel_variant at delays up to 8, the batched LPV / seed-mode entry points on ragged B*N, and the straggler deferral
parks and restores the run-time kernel's LDS image.

Rules: tests/_tolerance.py (check_batch) -- equal status and iteration count, solutions in classes A / B / C / D.  Controller
QPs of these workloads are all solved.  Batch sizes are not multiples of 64, and neither is B*N.  Each sweep prints its class
counts (run with -s to see them)."""
import numpy as np
import pytest

from oracle import lpv_ref as L, osqp_ref as O
from tests import _tolerance as T

pytestmark = pytest.mark.gpu

P = dict(L.DEFAULT_PARAMS)
NTHREADS = 16

CTRL_N = [8, 9, 10, 11, 13, 19, 20, 21, 27, 51, 52]
PLAN_N = [8, 9, 19, 20, 21, 29, 30, 31, 39, 40, 41, 52]
DELAYS = [(8, 1), (8, 7), (9, 8), (10, 1), (10, 8), (13, 5), (20, 1), (20, 4), (20, 8), (21, 3), (52, 8)]


@pytest.fixture(scope="module")
def lpvmpc():
    import lpvmpc as m
    return m


def _track_length(tab):
    return float(tab[-1, 3] + tab[-1, 4])


def ctrl_workload(B, N, seed, shape="oval", lap=1, vary=False, vmin=0.8):
    """workloads.controller_batch (vx in [0.8, 3]; vmin > 0.8 maps it onto [vmin, 3]); lap 0: curvature from the map at the
    rolled-out s (curv_s None), and every third instance starts within one horizon's travel of the lap end so that its roll-out
    wraps.  vary: u_prev and vel_ref change from stage to stage (the LPV tests: a mix-up of stages or instances shows).
    Below vx = 1.04 the forward-Euler yaw mode, 1 - dt (lf^2 Cf + lr^2 Cr) / (Iz vx), is unstable (and the lateral one below 0.9):
    a long roll-out, or one driven off its steady inputs -- pinned or varied steering -- leaves the speed box (infeasible QPs),
    runs s below 0 (no curvature) or amplifies round-off into the QP's data, so those workloads take vmin = 1.2."""
    from lpvmpc import workloads
    w = workloads.controller_batch(B, N=N, seed=seed, shape=shape)
    rng = np.random.default_rng(seed + 7919)
    if vmin != 0.8:
        x0 = w["x0"].copy()
        x0[:, 0] = vmin + (x0[:, 0] - 0.8) * ((3.0 - vmin) / 2.2)
        w = dict(w, x0=x0, vel_ref=np.repeat(x0[:, :1], N + 1, axis=1))
    if lap == 0:
        x0 = w["x0"].copy()
        wrap = np.arange(B) % 3 == 0
        travel = x0[wrap, 0] * w["dt"] * N
        x0[wrap, 4] = _track_length(w["track"]) - rng.uniform(0.05, 0.95, int(wrap.sum())) * travel
        w = dict(w, x0=x0, curv_s=None, lap=0)
    if vary:
        w = dict(w, u_prev=w["u_prev"] + rng.normal(0.0, 0.02, w["u_prev"].shape),
                 vel_ref=w["vel_ref"] * rng.uniform(0.95, 1.05, w["vel_ref"].shape))
    return w


def plan_workload(B, N, seed, shape="L_shape", vary=False):
    """workloads.planner_batch with every third instance's SS starting within one horizon's travel of the lap end (SS crosses it)."""
    from lpvmpc import workloads
    w = workloads.planner_batch(B, N=N, seed=seed, shape=shape)
    rng = np.random.default_rng(seed + 7919)
    SS = w["curv_s"].copy()
    wrap = np.arange(B) % 3 == 0
    step = SS[:, 1] - SS[:, 0]
    s0 = _track_length(w["track"]) - rng.uniform(0.05, 0.95, int(wrap.sum())) * step[wrap] * N
    SS[wrap] = s0[:, None] + np.arange(N + 1)[None, :] * step[wrap, None]
    w = dict(w, curv_s=SS)
    if vary:
        w = dict(w, u_prev=w["u_prev"] + rng.normal(0.0, 0.02, w["u_prev"].shape))
    return w


def delay_workload(B, N, d, seed):
    """Controller batch (vx in [1.2, 3], see ctrl_workload) for a handle with steeringDelay = d: u_old = [OldSteering[0],
    OldAccelera[0], OldSteering[1..d]], the d pins drawn inside the steering box as a random walk from OldSteering[0]."""
    w = ctrl_workload(B, N, seed, vmin=1.2)
    rng = np.random.default_rng(seed + 104729)
    pins = np.clip(w["u_old"][:, :1] + np.cumsum(rng.normal(0.0, 0.06, (B, d)), axis=1), -0.24, 0.24)
    return dict(w, u_old=np.concatenate([w["u_old"], pins], axis=1))


def solve(w, variant=0, **settings):
    from lpvmpc import workloads
    eng = workloads.make_solver(w, **settings)
    eng.set_option("kernel_variant", variant)
    out = eng.solve(w["x0"], w["u_prev"], w["vel_ref"], w["curv_s"], w["u_old"], w["max_ey"], w["cf_new"], w["lap"])
    eng.close()
    return out


def relclose(a, b, tol, what):
    a = np.asarray(a, float); b = np.asarray(b, float)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(1.0, float(np.max(np.abs(b))))
    err = float(np.max(np.abs(a - b)))
    assert err <= tol * scale, "%s: max err %.3e > %.1e * %.3e" % (what, err, tol, scale)
    return err / scale


def _report(tag, counts, out):
    print("%s iters %d..%d %s" % (tag, int(np.min(out["iters"])), int(np.max(out["iters"])), counts))


# ---- a. controller horizon sweep ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lap", [1, 0])
@pytest.mark.parametrize("shape", ["oval", "L_shape"])
@pytest.mark.parametrize("N", CTRL_N)
def test_controller_horizon_sweep(lpvmpc, N, shape, lap):
    """The fused tick at every kind of horizon (compile-time N = 8 / 10 / 20, run-time kernel elsewhere; odd and even) on
    kernel_variant 0 and 1 (and 2, 3 at N = 20), lap 1 (caller's curvature) and lap 0 (the map's, rolled-out s wrapping).
    Every QP is solved, except where the roll-out leaves the track table (s < 0 behind a diverged low-speed roll-out: the
    reference raises, UTIL:44-48): there the device reports UNSOLVED with NaN outputs (lpvmpc.h) -- the C tick returns NaN.
    vx starts at 0.8 up to N = 27 and at 1.2 beyond (see ctrl_workload): at vx = 0.8 and N = 52 the roll-out grows ~1.6^52 and
    the QP's data is decided by its round-off -- the oracle's numpy and C assemblies of one instance differ by 0.2 in u."""
    w = ctrl_workload(97, N, seed=1000 + 10 * N + lap, shape=shape, lap=lap, vmin=0.8 if N <= 27 else 1.2)
    ref = O.ctrl_tick_batch(w, nthreads=NTHREADS)
    nocurv = ~np.isfinite(ref["uPred"]).all(axis=(1, 2))
    assert lap == 0 or not nocurv.any()
    assert np.all(ref["status"][~nocurv] == 1), np.unique(ref["status"], return_counts=True)
    for variant in ((0, 1, 2, 3) if N == 20 else (0, 1)):
        out = solve(w, variant)
        assert np.all(out["status"][~nocurv] == 1), (variant, np.unique(out["status"], return_counts=True))
        assert np.all(out["status"][nocurv] == -10) and np.isnan(out["uPred"][nocurv]).all(), (variant, np.nonzero(nocurv)[0])
        counts = T.check_batch(w, "controller", out, ref)
        assert counts["C"] == counts["D"] == counts["flips"] == 0, counts
        _report("ctrl N=%d %s lap=%d variant=%d no-curvature %d" % (N, shape, lap, variant, int(nocurv.sum())), counts, out)


# ---- b. planner horizon sweep ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", PLAN_N)
def test_planner_horizon_sweep(lpvmpc, N):
    """The planner tick at every kind of horizon (compile-time N = 20 / 30 / 40, run-time kernel elsewhere) on the default
    kernel and kernel_variant 1; a third of the instances' SS crosses the lap end."""
    w = plan_workload(65, N, seed=2000 + N)
    assert np.any(w["curv_s"][:, -1] > _track_length(w["track"]))
    ref = O.plan_tick_batch(w, nthreads=NTHREADS)
    for variant in (0, 1):
        out = solve(w, variant)
        counts = T.check_batch(w, "planner", out, ref)
        _report("plan N=%d variant=%d" % (N, variant), counts, out)


# ---- c. steering-delay matrix ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,d", DELAYS)
def test_steering_delay_matrix(lpvmpc, N, d):
    """steeringDelay = d (CTRL:518-527) on every kernel_variant in {0, 1, 2, 3, 9} against the delay oracle
    (osqp_ref.ctrl_tick_batch_delay); at N = 20 these reach <6,20,2>, <6,20,1>, the run-time kernel and the fall-back of
    variant 9, elsewhere they collapse onto the horizon's kernel.  A route that dropped a pinned-steering row solves another QP:
    the pins would not hold and the iterations would differ."""
    B = 48
    w = delay_workload(B, N, d, seed=3000 + 10 * N + d)
    ref = O.ctrl_tick_batch_delay(w, nthreads=NTHREADS)
    assert np.all(ref["status"] == 1), np.unique(ref["status"], return_counts=True)
    pins = w["u_old"][:, 2:]
    assert np.max(np.abs(ref["uPred"][:, :d, 0] - pins)) <= 2e-4
    for variant in (0, 1, 2, 3, 9):
        out = solve(w, variant, steering_delay=d)
        assert np.all(out["status"] == 1), (variant, np.unique(out["status"], return_counts=True))
        counts = T.check_batch(w, "controller", out, ref)
        assert counts["C"] == counts["D"] == counts["flips"] == 0, counts
        err = float(np.max(np.abs(out["uPred"][:, :d, 0] - pins)))
        assert err <= 2e-4, (variant, err)
        _report("delay N=%d d=%d variant=%d |pin| %.1e" % (N, d, variant, err), counts, out)


# ---- d. batched LPV and seed-mode entry points --------------------------------------------------------------------------------
@pytest.mark.parametrize("lap", [0, 1])
@pytest.mark.parametrize("N", [8, 9, 13, 21, 52])
def test_controller_lpv_batch(lpvmpc, N, lap):
    """eng.lpv (two launches: one thread per (instance, stage), then one lane per instance) against the serial host roll-out,
    instance by instance, at 1e-11 of each array's largest magnitude (the golden tolerance), B = 97, 65, 1 (B*N ragged)."""
    from lpvmpc import workloads
    worst = 0.0
    for B in (97, 65, 1):
        w = ctrl_workload(B, N, seed=4000 + 10 * N + B + lap, lap=lap, vary=True, vmin=1.2)
        eng = workloads.make_solver(w)
        S, A, Bm = eng.lpv(w["x0"], w["u_prev"], w["vel_ref"], w["curv_s"], cf_new=w["cf_new"], lap=w["lap"])
        eng.close()
        wrapped = 0
        for j in range(B):
            Sr, Ar, Br = L.ctrl_lpv_prediction(P, w["dt"], N, w["track"], w["x0"][j], w["u_prev"][j], w["vel_ref"][j],
                                               None if w["curv_s"] is None else w["curv_s"][j], w["cf_new"], w["lap"])
            wrapped += int(Sr[-1, 4] > _track_length(w["track"]))
            for got, want, what in ((S[j], Sr, "states"), (A[j], Ar, "A"), (Bm[j], Br, "B")):
                worst = max(worst, relclose(got, want, 1e-11, "N=%d lap=%d B=%d #%d %s" % (N, lap, B, j, what)))
        if lap == 0 and B > 1:
            assert wrapped >= B // 6, wrapped
    print("ctrl lpv N=%d lap=%d: max rel err %.2e" % (N, lap, worst))


@pytest.mark.parametrize("N", [9, 20, 31, 40])
def test_planner_lpv_batch(lpvmpc, N):
    """The planner's eng.lpv against the serial host roll-out, B = 97, 65, 1, SS crossing the lap end: 1e-11 of each array's
    largest magnitude (observed <= 1.5e-13; the golden test of the planner allows 1e-10)."""
    from lpvmpc import workloads
    worst = 0.0
    for B in (97, 65, 1):
        w = plan_workload(B, N, seed=5000 + 10 * N + B, vary=True)
        eng = workloads.make_solver(w)
        S, A, Bm = eng.lpv(w["x0"], w["u_prev"], None, w["curv_s"])
        eng.close()
        for j in range(B):
            Sr, Ar, Br = L.plan_lpv_prediction(P, w["dt"], N, w["track"], w["x0"][j], w["curv_s"][j], w["u_prev"][j])
            for got, want, what in ((S[j], Sr, "states"), (A[j], Ar, "A"), (Bm[j], Br, "B")):
                worst = max(worst, relclose(got, want, 1e-11, "N=%d B=%d #%d %s" % (N, B, j, what)))
    print("plan lpv N=%d: max rel err %.2e" % (N, worst))


@pytest.mark.parametrize("kind,N", [("controller", 9), ("controller", 20), ("planner", 13), ("planner", 30)])
def test_estimate_abc_batch(lpvmpc, kind, N):
    """eng.estimate_abc (seed-mode linearisation along a given trajectory, one thread per (instance, stage)) against
    ctrl_estimate_abc / plan_estimate_abc at 1e-12, B = 97, 65, 1; s runs past the lap end."""
    tab = lpvmpc.Map("oval" if kind == "controller" else "L_shape", 0.2).PointAndTangent
    Lt = _track_length(tab)
    worst = 0.0
    for B in (97, 65, 1):
        rng = np.random.default_rng(6000 + 10 * N + B)
        vx = rng.uniform(0.8, 3.0, (B, N)); vy = rng.normal(0, 0.05, (B, N)); wz = rng.normal(0, 0.3, (B, N))
        epsi = rng.normal(0, 0.1, (B, N)); ey = rng.normal(0, 0.1, (B, N)); s = rng.uniform(0.0, 1.5 * Lt, (B, N))
        delta = rng.uniform(-0.24, 0.24, (B, N))
        if kind == "controller":
            eng = lpvmpc.BatchedSolver("controller", N, 1 / 30.0, np.eye(6), np.eye(2), np.ones(2), track=tab)
            xx = np.stack([vx, vy, wz, epsi, s, ey], axis=2)
        else:
            eng = lpvmpc.BatchedSolver("planner", N, 0.05, np.eye(5), np.eye(2), np.ones(2), L_cf=np.zeros(5), track=tab)
            xx = np.stack([vx, vy, wz, ey, epsi, s], axis=2)
        A, Bm = eng.estimate_abc(xx, delta)
        eng.close()
        for j in range(B):
            if kind == "controller":
                Ar, Br = L.ctrl_estimate_abc(P, 1 / 30.0, N, tab, xx[j], np.stack([delta[j], np.zeros(N)], axis=1))
            else:
                Ar, Br = L.plan_estimate_abc(P, 0.05, N, tab, xx[j], delta[j])
            worst = max(worst, relclose(A[j], Ar, 1e-12, "%s N=%d B=%d #%d A" % (kind, N, B, j)))
            worst = max(worst, relclose(Bm[j], Br, 1e-12, "%s N=%d B=%d #%d B" % (kind, N, B, j)))
    print("%s estimate_abc N=%d: max rel err %.2e" % (kind, N, worst))


# ---- e. deferral on the run-time-horizon kernel -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,N,d", [("controller", 13, 2), ("controller", 21, 0), ("planner", 25, 0)])
def test_runtime_kernel_deferral_is_bit_identical(lpvmpc, kind, N, d):
    """Straggler deferral parks and restores the run-time kernel's LDS image (the largest, sized by N).  No tail kernel exists
    at these horizons, so with "defer_tail" 0 and 1 every output word equals the plain call's."""
    from lpvmpc import workloads
    B = 97
    w = delay_workload(B, N, d, seed=7000 + N) if kind == "controller" else plan_workload(B, N, seed=7000 + N)
    args = (w["x0"], w["u_prev"], w["vel_ref"], w["curv_s"], w["u_old"], w["max_ey"], w["cf_new"], w["lap"])
    plain = workloads.make_solver(w, steering_delay=d)
    ref = plain.solve(*args)
    plain.close()
    assert np.sum(ref["iters"] > 25) >= 8, ref["iters"]
    for tail in (0, 1):
        eng = workloads.make_solver(w, steering_delay=d)
        eng.reserve(B)
        eng.set_option("defer_pool", 2 * B); eng.set_option("defer_after", 25); eng.set_option("defer_tail", tail)
        got = eng.solve(*args)
        parked, refused = eng.defer_stats()
        eng.close()
        assert parked > 0, (tail, parked, refused)
        for k in ("status", "iters", "polish", "xPred", "uPred", "resid"):
            assert np.array_equal(np.asarray(got[k]), np.asarray(ref[k]), equal_nan=True), (tail, k)
        print("deferral %s N=%d d=%d tail=%d: parked %d, refused %d, %d of %d instances past 25 iterations"
              % (kind, N, d, tail, parked, refused, int(np.sum(ref["iters"] > 25)), B))
