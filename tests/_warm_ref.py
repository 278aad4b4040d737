"""Test infrastructure: the opt-in warm start (lpvmpc_set_option "warm_start") restated on the host, in plain numpy
on the oracle's (z, y) -- the reference's variable and row order (oracle/lpv_ref.py ctrl_build_qp / plan_build_qp):

  controller  z = [x_0 .. x_N (6 each) | u_0 .. u_N-1 (2 each)]
              y = [2 speed rows per stage k < N | 4 input rows per stage k < N | 6 dynamics rows per stage k <= N | d pins]
  planner     z = [x_0 .. x_N (5 each) | u_0 .. u_N-1 (2 each)]
              y = [5 dynamics rows per stage k <= N | 5 state-box rows per stage k <= N | 2 input-box rows per stage k < N]

The rule of mode 2 (shift_state; include/lpvmpc.h, "warm_start"): stage k takes stage k + 1 and the last stage that exists for a row
or variable is kept -- states, dynamics rows and the planner's state-box rows run to stage N, inputs, the planner's input-box rows
and the controller's box rows to stage N - 1.  Of the d pinned-steering rows of steeringDelay = d, row k < d - 1 takes row k + 1 and
the last one starts at 0: stage d has no pin.  Mode 1 takes (z, y) as they are.  An instance whose previous solve returned no
solution (PRIMAL / DUAL INFEASIBLE, exact or inaccurate, or UNSOLVED) starts from zeros, a cold start.

The scenario of tests/test_gpu_warm_start.py (three ticks, the inputs of a tick derived from the ORACLE's previous one) and the
robust set (tests/golden/warm_start/robust.npz: the instances whose warm tick the oracle itself decides the same way under both of
its elimination orders and under perturbed warm starts) are computed here, once per process."""
import os

import numpy as np

from oracle import osqp_ref as O

NTHREADS = 16
MODES = (1, 2)
WARM_TICKS = (2, 3)
NO_SOLUTION = (-3, 3, -4, 4, -10)
MAX_ITER = 4000
# relative size of the perturbed warm starts: the observed bound of classes A and B of tests/_tolerance.py (1e-6), the most the
# device's own state of the previous tick may differ from the oracle's
PERTURB = 1e-6
PERTURB_SEEDS = (9301, 9302)
ROBUST_SHARE = 0.75
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "warm_start", "robust.npz")


def dims(kind, N, d=0):
    """(nx, nz, m) of a QP of the kind."""
    nx = 6 if kind == "controller" else 5
    nz = (N + 1) * nx + N * 2
    return nx, nz, (6 * N + (N + 1) * 6 + d if kind == "controller" else (N + 1) * nx + nz)


def delay_of(w, kind):
    return int(np.asarray(w["u_old"]).reshape(np.asarray(w["x0"]).shape[0], -1).shape[1] - 2) if kind == "controller" else 0


def shift_state(kind, N, d, z, y):
    """(z, y) of shapes (B, nz), (B, m) shifted by one stage (module docstring)."""
    z = np.asarray(z, np.float64); y = np.asarray(y, np.float64)
    B = z.shape[0]
    nx, nz, m = dims(kind, N, d)
    assert z.shape == (B, nz) and y.shape == (B, m), (z.shape, y.shape)
    ns = (N + 1) * nx
    to_N = np.minimum(np.arange(N + 1) + 1, N)              # rows / variables that exist up to stage N
    to_N1 = np.minimum(np.arange(N) + 1, N - 1)             # ... up to stage N - 1
    per = lambda a, n, idx: a.reshape(B, -1, n)[:, idx].reshape(B, -1)
    z2 = np.concatenate([per(z[:, :ns], nx, to_N), per(z[:, ns:], 2, to_N1)], axis=1)
    if kind == "controller":
        mi = 6 * N
        pins = y[:, mi + ns:]
        y2 = np.concatenate([per(y[:, :2 * N], 2, to_N1), per(y[:, 2 * N:mi], 4, to_N1), per(y[:, mi:mi + ns], nx, to_N),
                             pins[:, 1:], np.zeros((B, 1 if d > 0 else 0))], axis=1)
    else:
        y2 = np.concatenate([per(y[:, :ns], nx, to_N), per(y[:, ns:2 * ns], nx, to_N), per(y[:, 2 * ns:], 2, to_N1)], axis=1)
    assert z2.shape == z.shape and y2.shape == y.shape
    return z2, y2


def saved_state(res):
    """(z, y) as a solve leaves them for the next one: the returned point and duals, zeros for an instance without a solution."""
    z = np.array(res["z"], np.float64); y = np.array(res["y"], np.float64)
    none = np.isin(res["status"], NO_SOLUTION) | ~np.isfinite(z).all(axis=1) | ~np.isfinite(y).all(axis=1)
    z[none] = 0.0; y[none] = 0.0
    return z, y


def warm_state(res, kind, N, d, mode):
    """The warm start that follows the result ``res`` under ``mode`` (1: as saved, 2: shifted by one stage)."""
    z, y = saved_state(res)
    return shift_state(kind, N, d, z, y) if mode == 2 else (z, y)


def has_solution(res):
    return np.isfinite(res["uPred"]).all(axis=(1, 2)) & np.isfinite(res["xPred"]).all(axis=(1, 2))


def next_inputs(w, kind, res):
    """The workload of the next tick: where ``res`` has a solution, x0 <- xPred[:, 1], u_prev <- uPred shifted by one stage (the
    last stage kept), u_old <- uPred[:, 0] -- with steeringDelay = d in the device's layout [steer, accel, pin_1 .. pin_d], the pins
    of the next tick being the steering of stages 1 .. d; elsewhere the instance keeps its inputs."""
    sol = has_solution(res)
    x0 = np.array(w["x0"], np.float64); u_prev = np.array(w["u_prev"], np.float64); u_old = np.array(w["u_old"], np.float64)
    xP, uP = res["xPred"], res["uPred"]
    x0[sol] = xP[sol, 1]
    u_prev[sol] = np.concatenate([uP[sol, 1:], uP[sol, -1:]], axis=1)
    u_old[sol, :2] = uP[sol, 0]
    d = delay_of(w, kind)
    if d:
        u_old[sol, 2:] = uP[sol, 1:d + 1, 0]
    return dict(w, x0=x0, u_prev=u_prev, u_old=u_old)


def perturbed(ws, seed):
    """The warm start with every word scaled by 1 + PERTURB * U(-1, 1)."""
    rng = np.random.default_rng(seed)
    return tuple(a * (1.0 + PERTURB * rng.uniform(-1.0, 1.0, a.shape)) for a in ws)


def key(res):
    """What the warm tick is compared by: (status, iterations, polish flag) per instance."""
    return np.stack([res["status"], res["iters"], res["polish"]], axis=1).astype(np.int64)


# ---- the scenario, cached -------------------------------------------------------------------------------------------------------
# ``case``: a settings case of tests/test_gpu_settings.py (None: the defaults), or FINE_CASE: termination checked on every iteration
# and no polish.  An iteration count then resolves single iterations, not blocks of 25, and every instance returns its ADMM iterate
# with that iterate's residuals (resid words), which depend on the start continuously: at the defaults a controller QP that is solved
# at its first or second check whatever the start, and polished onto the optimum, tells a wrong start from a right one on few
# instances, or none.
FINE_CASE = "fine"
FINE_SETTINGS = dict(check_termination=1, polish=0)
FINE_NAMES = ("ctrl8", "ctrl10", "ctrl13", "ctrl20", "ctrl20d3")
_W, _QPS, _REF = {}, {}, {}


def _base(name):
    from tests import test_gpu_settings as G
    return G.WORKLOADS[name][0], G.workload(name)[1]


def _settings(case):
    from tests import test_gpu_settings as G
    return FINE_SETTINGS if case == FINE_CASE else G.settings_of(case)


def scenario_workload(name, mode, tick, case=None):
    """(kind, w) of a tick (1, 2, 3) of the scenario of workload ``name``: tick 1 is the workload of tests/test_gpu_settings.py,
    tick t + 1 follows the oracle's tick t (next_inputs).  Tick 2 is the same under both modes (tick 1 is cold)."""
    kind, w1 = _base(name)
    k = (name, 0 if tick <= 2 else mode, tick, case)
    if k not in _W:
        _W[k] = w1 if tick == 1 else next_inputs(scenario_workload(name, mode, tick - 1, case)[1], kind, scenario_ref(name, mode, tick - 1, case=case))
    return kind, _W[k]


def scenario_qps(name, mode, tick, case=None):
    k = (name, 0 if tick <= 2 else mode, tick, case)
    if k not in _QPS:
        kind, w = scenario_workload(name, mode, tick, case)
        qps = []
        for j in range(w["x0"].shape[0]):
            try:
                qps.append(O.instance_qp(w, kind, j))
            except ValueError:
                qps.append(None)
        _QPS[k] = qps
    return _QPS[k]


def scenario_warm(name, mode, tick, case=None):
    """The warm start of a warm tick (2, 3): from the oracle's previous tick."""
    kind, w = scenario_workload(name, mode, tick, case)
    return warm_state(scenario_ref(name, mode, tick - 1, case=case), kind, int(w["N"]), delay_of(w, kind), mode)


def scenario_ref(name, mode, tick, cold=False, case=None):
    """The oracle's result of a tick of the scenario (stage-wise elimination order): tick 1 cold, ticks 2 and 3 warm-started from
    its own previous tick under ``mode``.  ``cold``: the same data from a cold start."""
    k = (name, 0 if tick == 1 or (cold and tick == 2) else mode, tick, bool(cold) or tick == 1, case)
    if k not in _REF:
        kind, w = scenario_workload(name, mode, tick, case)
        warm = None if k[3] else scenario_warm(name, mode, tick, case)
        _REF[k] = O.tick_batch_qp(w, kind, settings=_settings(case), nthreads=NTHREADS, qps=scenario_qps(name, mode, tick, case), warm=warm)
    return _REF[k]


def robust_mask(name, mode, tick, case=None):
    """The robust instances of a warm tick, measured on the oracle alone: (status, iterations, polish flag) equal under the stage-wise
    and the RCM elimination order and under the two perturbed warm starts, an answer on the oracle's side, and a previous tick that
    did not end at the iteration cap (such a point carries no bound: class C of tests/_tolerance.py)."""
    kind, w = scenario_workload(name, mode, tick, case)
    qps, warm = scenario_qps(name, mode, tick, case), scenario_warm(name, mode, tick, case)
    base, prev = scenario_ref(name, mode, tick, case=case), scenario_ref(name, mode, tick - 1, case=case)
    st = _settings(case)
    ok = (base["status"] != -10) & (prev["iters"] < int((st or {}).get("max_iter", MAX_ITER)))
    runs = [O.tick_batch_qp(w, kind, settings=st, nthreads=NTHREADS, qps=qps, warm=warm, order="rcm")]
    runs += [O.tick_batch_qp(w, kind, settings=st, nthreads=NTHREADS, qps=qps, warm=perturbed(warm, s)) for s in PERTURB_SEEDS]
    for r in runs:
        ok &= (key(r) == key(base)).all(axis=1)
    return ok


def fixture_key(name, mode, tick, case=None):
    return "%s%s_m%d_t%d" % (name, "_" + case if case else "", mode, tick)


def compute_robust():
    """Fixture key -> bool mask: every workload of tests/test_gpu_settings.py at the defaults, the controllers also under FINE_CASE."""
    from tests import test_gpu_settings as G
    cases = [(n, None) for n in G.WORKLOADS] + [(n, FINE_CASE) for n in FINE_NAMES]
    return {fixture_key(n, m, t, c): robust_mask(n, m, t, c) for n, c in cases for m in MODES for t in WARM_TICKS}


_FIX = None


def robust(name, mode, tick, case=None):
    """The committed mask of a warm tick."""
    global _FIX
    if _FIX is None:
        with np.load(FIXTURE) as f:
            _FIX = {k: f[k].astype(bool) for k in f.files}
    return _FIX[fixture_key(name, mode, tick, case)]
