"""Oracle (TEST INFRASTRUCTURE): ctypes front end of ``osqp_ref.c``.

Builds ``oracle/_build/liboracle.so`` with gcc on first use (or through
``oracle/Makefile``).  See the header of ``osqp_ref.c`` for what is restated
and why parity with the real OSQP binary is *unpinned*.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import reverse_cuthill_mckee

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "_build", "liboracle.so")
_SRCS = ["osqp_ref.c", "lpv_ref.c"]

STATUS = {1: "solved", 2: "solved inaccurate", 3: "primal infeasible inaccurate",
          4: "dual infeasible inaccurate", -2: "maximum iterations reached",
          -3: "primal infeasible", -4: "dual infeasible", -7: "problem non convex",
          -10: "unsolved"}


class Settings(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("rho", "sigma", "alpha", "eps_abs", "eps_rel",
                                           "eps_prim_inf", "eps_dual_inf", "delta",
                                           "adaptive_rho_tolerance")] + \
               [(k, C.c_int) for k in ("max_iter", "check_termination", "scaling", "adaptive_rho",
                                        "adaptive_rho_interval", "polish", "polish_refine_iter",
                                        "scaled_termination")]


class Info(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("iter", "status_val", "status_polish", "rho_updates")] + \
               [(k, C.c_double) for k in ("obj_val", "pri_res", "dua_res", "rho_estimate", "rho_final")]


def build(force=False):
    srcs = [os.path.join(_HERE, s) for s in _SRCS if os.path.exists(os.path.join(_HERE, s))]
    if not force and os.path.exists(_LIB) and all(
            os.path.getmtime(_LIB) >= os.path.getmtime(s) for s in srcs):
        return _LIB
    os.makedirs(os.path.dirname(_LIB), exist_ok=True)
    cmd = ["gcc", "-O2", "-fPIC", "-shared", "-fopenmp", "-o", _LIB] + srcs + ["-lm"]
    subprocess.run(cmd, check=True)
    return _LIB


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.osqp_ref_default_settings.argtypes = [C.POINTER(Settings)]
        _lib.osqp_ref_solve.restype = C.c_int
        _lib.osqp_ref_solve_ws.restype = C.c_int
    return _lib


def default_settings(**over):
    s = Settings()
    lib().osqp_ref_default_settings(C.byref(s))
    for k, v in over.items():
        if not hasattr(s, k):
            raise KeyError(k)
        setattr(s, k, v)
    return s


def kkt_ordering(P, A):
    """Fill-reducing ordering of the (n+m) KKT unknowns (stand-in for OSQP's AMD;
    the ordering only changes round-off)."""
    n = P.shape[0]
    m = A.shape[0]
    Pb = (abs(sp.csr_matrix(P)) > 0).astype(np.int8)
    Ab = (abs(sp.csr_matrix(A)) > 0).astype(np.int8)
    K = sp.bmat([[Pb + Pb.T + sp.eye(n, dtype=np.int8), Ab.T],
                 [Ab, sp.eye(m, dtype=np.int8)]], format="csr")
    return np.ascontiguousarray(reverse_cuthill_mckee(K, symmetric_mode=True), dtype=np.int32)


def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def solve_qp(P, q, A, l, u, perm="rcm", x_ws=None, y_ws=None, **settings):
    """Solve min 1/2 x'Px + q'x s.t. l <= Ax <= u with the OSQP restatement.

    ``P`` (n,n) symmetric, ``A`` (m,n): dense arrays or scipy sparse.  Returns a
    namespace ``x, y, info`` where ``info`` carries iter / status_val / status /
    status_polish / obj_val / pri_res / dua_res / rho_updates / rho_estimate.
    ``x_ws`` (n,), ``y_ws`` (m,): an unscaled warm start as osqp_warm_start takes it
    (osqp_ref_solve_ws: x <- D^-1 x_ws, y <- c E^-1 y_ws, z <- A x); None: cold."""
    P = sp.csc_matrix(P)
    A = sp.csc_matrix(A)
    n, m = P.shape[0], A.shape[0]
    Pu = sp.triu(P, format="csc")
    Pu.sort_indices(); A.sort_indices()
    Pu.eliminate_zeros(); A.eliminate_zeros()
    q = np.ascontiguousarray(q, dtype=np.float64)
    l = np.ascontiguousarray(l, dtype=np.float64)
    u = np.ascontiguousarray(u, dtype=np.float64)
    if isinstance(perm, str):
        perm = kkt_ordering(P, A) if perm == "rcm" else None
    s = settings.pop("settings", None) or default_settings(**settings)
    x = np.empty(n); y = np.empty(m)
    info = Info()
    if x_ws is not None:
        x_ws = np.ascontiguousarray(x_ws, dtype=np.float64).reshape(n)
    if y_ws is not None:
        y_ws = np.ascontiguousarray(y_ws, dtype=np.float64).reshape(m)
    Pp = Pu.indptr.astype(np.int32); Pi = Pu.indices.astype(np.int32); Px = Pu.data.astype(np.float64)
    Ap = A.indptr.astype(np.int32); Ai = A.indices.astype(np.int32); Ax = A.data.astype(np.float64)
    rc = lib().osqp_ref_solve_ws(
        C.c_int(n), C.c_int(m), _ptr(Pp, C.c_int), _ptr(Pi, C.c_int), _ptr(Px, C.c_double), _ptr(q, C.c_double),
        _ptr(Ap, C.c_int), _ptr(Ai, C.c_int), _ptr(Ax, C.c_double), _ptr(l, C.c_double), _ptr(u, C.c_double),
        _ptr(perm, C.c_int) if perm is not None else None, C.byref(s),
        _ptr(x_ws, C.c_double) if x_ws is not None else None, _ptr(y_ws, C.c_double) if y_ws is not None else None,
        _ptr(x, C.c_double), _ptr(y, C.c_double), C.byref(info))
    if rc != 0:
        raise RuntimeError("osqp_ref_solve failed (KKT factorisation), rc=%d" % rc)
    return SimpleNamespace(
        x=x, y=y,
        info=SimpleNamespace(iter=info.iter, status_val=info.status_val,
                             status=STATUS.get(info.status_val, "?"), status_polish=info.status_polish,
                             obj_val=info.obj_val, pri_res=info.pri_res, dua_res=info.dua_res,
                             rho_updates=info.rho_updates, rho_estimate=info.rho_estimate,
                             rho_final=info.rho_final))


def ctrl_tick_batch(w, nthreads=1, params=None, warm=None, shift=True):
    """Whole controller tick (LPV roll-out + QP assembly + OSQP restatement) for a batch, in C
    (oracle/lpv_ref.c).  ``w`` is a workload dict (keys N, dt, Q, R, dR, track, x0, u_prev, vel_ref,
    curv_s, u_old, cf_new, lap).  Returns dict(xPred, uPred, status, iters, z, y); ``warm`` = a previous result
    dict whose (z, y) warm-start this tick (shifted by one stage when ``shift``)."""
    from .lpv_ref import DEFAULT_PARAMS
    p = dict(DEFAULT_PARAMS)
    if params:
        p.update(params)
    pv = np.array([p["lf"], p["lr"], p["m"], p["Iz"], p["Cf"], p["Cr"], p["mu"], p["max_vel"]], dtype=np.float64)
    N = int(w["N"])
    x0 = np.ascontiguousarray(w["x0"], np.float64); B = x0.shape[0]
    arrs = dict(Q=np.ascontiguousarray(w["Q"], np.float64), R=np.ascontiguousarray(w["R"], np.float64),
                dR=np.ascontiguousarray(w["dR"], np.float64), track=np.ascontiguousarray(w["track"], np.float64),
                u_prev=np.ascontiguousarray(w["u_prev"], np.float64), vel_ref=np.ascontiguousarray(w["vel_ref"], np.float64),
                curv=np.ascontiguousarray(w["curv_s"] if w["curv_s"] is not None else np.zeros((B, N)), np.float64),
                u_old=np.ascontiguousarray(w["u_old"], np.float64))
    xPred = np.empty((B, N + 1, 6)); uPred = np.empty((B, N, 2))
    status = np.empty(B, np.int32); iters = np.empty(B, np.int32)
    nz = (N + 1) * 6 + N * 2; m = 6 * N + (N + 1) * 6
    z = np.empty((B, nz)); y = np.empty((B, m))
    zw = yw = None
    if warm is not None:
        zw = np.ascontiguousarray(warm["z"], np.float64); yw = np.ascontiguousarray(warm["y"], np.float64)
    d = C.c_double
    f = lib().oracle_ctrl_tick_batch
    f.restype = C.c_int
    f(C.c_int(B), C.c_int(N), d(float(w["dt"])), _ptr(pv, d), _ptr(arrs["Q"], d), _ptr(arrs["R"], d), _ptr(arrs["dR"], d),
      _ptr(arrs["track"], d), C.c_int(arrs["track"].shape[0]), _ptr(x0, d), _ptr(arrs["u_prev"], d), _ptr(arrs["vel_ref"], d),
      _ptr(arrs["curv"], d), _ptr(arrs["u_old"], d), d(float(w["cf_new"])), C.c_int(int(w["lap"])),
      _ptr(xPred, d), _ptr(uPred, d), _ptr(status, C.c_int), _ptr(iters, C.c_int), C.c_int(int(nthreads)),
      _ptr(zw, d) if zw is not None else None, _ptr(yw, d) if yw is not None else None, C.c_int(1 if shift else 0),
      _ptr(z, d), _ptr(y, d))
    return dict(xPred=xPred, uPred=uPred, status=status, iters=iters, z=z, y=y)


def ctrl_delay_ordering(N, delay, nx=6, nu=2):
    """Stage-wise KKT ordering of a controller QP with ``delay`` pinned-steering rows: the order oracle/lpv_ref.c hands the
    solver for delay 0 (x_0 rows, then per stage its variables, box rows and the dynamics rows into the next stage), with
    the pin of stage k (row 6N + (N+1)nx + k of ctrl_build_qp) placed after stage k's box rows."""
    nz = (N + 1) * nx + N * nu
    mi = 6 * N
    perm = [nz + mi + r for r in range(nx)]
    for k in range(N + 1):
        perm += [k * nx + a for a in range(nx)]
        if k < N:
            perm += [(N + 1) * nx + k * nu + j for j in range(nu)]
            perm += [nz + 2 * k, nz + 2 * k + 1] + [nz + 2 * N + 4 * k + t for t in range(4)]
            if k < delay:
                perm.append(nz + mi + (N + 1) * nx + k)
            perm += [nz + mi + (k + 1) * nx + r for r in range(nx)]
    return np.array(perm, dtype=np.int32)


def plan_ordering(N, nx=5, nu=2):
    """Stage-wise KKT ordering of a planner QP: the order oracle/lpv_ref.c hands the solver (oracle_plan_tick_batch): the
    x_0 equality rows, then per stage each state with its box row, each input with its box row and the dynamics rows into
    the next stage."""
    nz = (N + 1) * nx + N * nu
    me = (N + 1) * nx
    perm = [nz + r for r in range(nx)]
    for k in range(N + 1):
        for a in range(nx):
            perm += [k * nx + a, nz + me + k * nx + a]
        if k < N:
            for j in range(nu):
                v = (N + 1) * nx + k * nu + j
                perm += [v, nz + me + v]
            perm += [nz + (k + 1) * nx + r for r in range(nx)]
    return np.array(perm, dtype=np.int32)


def osqp_settings(settings=None):
    """The OSQP part of a BatchedSolver settings dict as keyword arguments of solve_qp (polish_delta -> delta); the
    controller limits, the planner boxes and steering_delay are not solver settings and are dropped."""
    out = {}
    for k, v in (settings or {}).items():
        if k == "polish_delta":
            out["delta"] = v
        elif hasattr(Settings, k):
            out[k] = v
    return out


def instance_qp(w, kind, j, params=None, limits=None):
    """(P, q, A, l, u) of instance j of a workload dict, assembled on the host as the reference does, for the vehicle
    ``params`` (DEFAULT_PARAMS updated by it) and the QP ``limits`` (keywords of ctrl_build_qp: vx_min / delta_max / a_max /
    a_min_abs; of plan_build_qp: xmin / xmax / umin / umax).  A controller u_old with more than two columns is the device's
    layout of a handle with steeringDelay = d, [OldSteering[0], OldAccelera[0], OldSteering[1..d]]: the QP then carries
    the d pinned-steering rows (CTRL:518-527)."""
    from . import lpv_ref as L
    p = dict(L.DEFAULT_PARAMS)
    if params:
        p.update(params)
    N = int(w["N"])
    lim = dict(limits or {})
    if kind == "controller":
        S, A, B = L.ctrl_lpv_prediction(p, w["dt"], N, w["track"], w["x0"][j], w["u_prev"][j], w["vel_ref"][j],
                                        None if w["curv_s"] is None else w["curv_s"][j], w["cf_new"], w["lap"])
        u_old = np.asarray(w["u_old"][j], float).reshape(-1)
        return L.ctrl_build_qp(w["Q"], w["R"], w["dR"], N, A, B, w["x0"][j], u_old[:2], w["vel_ref"][j], p["max_vel"],
                               steer_hist=u_old[2:], **lim)
    S, A, B = L.plan_lpv_prediction(p, w["dt"], N, w["track"], w["x0"][j], w["curv_s"][j], w["u_prev"][j])
    mey = float(np.broadcast_to(w["max_ey"], (np.asarray(w["x0"]).shape[0],))[j])
    return L.plan_build_qp(w["Q"], w["R"], w["dR"], w["L_cf"], N, A, B, w["x0"][j], w["u_old"][j], mey, p["max_vel"],
                           p["min_vel"], **lim)


def tick_batch_qp(w, kind, settings=None, params=None, limits=None, nthreads=16, qps=None, order="stage", warm=None):
    """One tick of a batch, instance by instance: the LPV roll-out and the reference's QP (instance_qp: vehicle ``params``,
    QP ``limits``) solved by the OSQP restatement under ``settings`` (a BatchedSolver settings dict, see osqp_settings).
    ``kind`` "controller" (``u_old`` (B, 2 + d): d = steeringDelay pinned-steering rows) or "planner".  Elimination order:
    the stage-wise one of the C ticks (ctrl_delay_ordering, plan_ordering): at default arguments the statuses and iteration
    counts equal ctrl_tick_batch / plan_tick_batch's; the solutions differ by the round-off of the C ticks' own LPV / QP assembly
    (polished within 1e-10, tests/test_settings_host.py).  Returns dict(xPred, uPred, status, iters, polish, z, y, resid);
    ``resid`` (B, 4) holds the solver's own (pri_res, dua_res, obj_val, rho_final) in the order of the device's resid words, NaN
    for an instance without an answer (-10).  ``nthreads`` (<= 16) solves run at a time (the solver releases the GIL).  ``qps``: the instances' QPs (a list of instance_qp results
    or None entries for a roll-out that left the track) when the caller solves the same batch under several settings.
    ``order`` "rcm": solve_qp's default elimination order instead of the stage-wise one (the same KKT matrix: the two results
    differ by round-off alone, the yardstick of tests/_tolerance.py check_resid).  ``warm``: (z, y) of shapes (B, nz) and (B, m), the
    warm start of every instance as solve_qp takes it, already shifted by the caller (tests/_warm_ref.py shift_state); a row of
    zeros is a cold start."""
    from concurrent.futures import ThreadPoolExecutor
    N = int(w["N"])
    x0 = np.asarray(w["x0"], np.float64); B = x0.shape[0]
    ctrl = kind == "controller"
    nx = 6 if ctrl else 5
    nz = (N + 1) * nx + N * 2
    if ctrl:
        d = np.asarray(w["u_old"], np.float64).reshape(B, -1).shape[1] - 2
        perm, m = ctrl_delay_ordering(N, d), 6 * N + (N + 1) * 6 + d
    else:
        perm, m = plan_ordering(N), (N + 1) * nx + nz
    kw = osqp_settings(settings)
    if order == "rcm":
        perm = "rcm"
    elif order != "stage":
        raise ValueError(order)

    def one(j):
        # no answer (NaN, UNSOLVED -10): a roll-out that leaves the track table (the reference raises, UTIL:44-48) or a KKT
        # factorisation that breaks down
        try:
            qp = instance_qp(w, kind, j, params, limits) if qps is None else qps[j]
            if qp is None:
                raise ValueError("no QP")
            ws = {} if warm is None else dict(x_ws=warm[0][j], y_ws=warm[1][j])
            r = solve_qp(qp.P, qp.q, qp.A, qp.l, qp.u, perm=perm, **ws, **kw)
        except (ValueError, RuntimeError):
            return np.full(nz, np.nan), np.full(m, np.nan), -10, 0, 0, (np.nan,) * 4
        return r.x, r.y, r.info.status_val, r.info.iter, r.info.status_polish, (r.info.pri_res, r.info.dua_res, r.info.obj_val, r.info.rho_final)

    with ThreadPoolExecutor(max_workers=max(1, min(16, int(nthreads)))) as ex:
        res = list(ex.map(one, range(B)))
    z = np.array([r[0] for r in res]).reshape(B, nz)
    return dict(xPred=z[:, :(N + 1) * nx].reshape(B, N + 1, nx).copy(), uPred=z[:, (N + 1) * nx:].reshape(B, N, 2).copy(), z=z,
                y=np.array([r[1] for r in res]).reshape(B, m), status=np.array([r[2] for r in res], np.int32).reshape(B),
                iters=np.array([r[3] for r in res], np.int32).reshape(B), polish=np.array([r[4] for r in res], np.int32).reshape(B),
                resid=np.array([r[5] for r in res], np.float64).reshape(B, 4))


def ctrl_tick_batch_delay(w, nthreads=1, params=None):
    """Controller tick with steeringDelay = d = u_old.shape[1] - 2 for a batch: per instance the LPV roll-out
    (lpv_ref.ctrl_lpv_prediction), the reference's QP with d pinned-steering rows (lpv_ref.ctrl_build_qp, CTRL:518-527) and
    the OSQP restatement.  ``w`` is a workload dict as for ctrl_tick_batch, with ``u_old`` in the device's layout
    [OldSteering[0], OldAccelera[0], OldSteering[1..d]] (B, 2 + d).  Elimination order: the stage-wise one of
    ctrl_delay_ordering (the C tick's order at d = 0); on tests/golden/ctrl_n20_delay.npz it reproduces the reference's
    status, iteration count and polish flag of every case (as does solve_qp's RCM order, which the class-D rule of
    tests/_tolerance.py takes as the other order).  Returns dict(xPred, uPred, status, iters, z, y, polish); ``nthreads``
    solves run at a time (the solver releases the GIL).  tick_batch_qp at default settings and limits."""
    return tick_batch_qp(w, "controller", params=params, nthreads=nthreads)


def plan_tick_batch(w, nthreads=1, params=None):
    """Whole planner tick for a batch in C (oracle/lpv_ref.c); ``w`` as produced by workloads.planner_batch."""
    from .lpv_ref import DEFAULT_PARAMS
    p = dict(DEFAULT_PARAMS)
    if params:
        p.update(params)
    pv = np.array([p["lf"], p["lr"], p["m"], p["Iz"], p["Cf"], p["Cr"], p["mu"], p["max_vel"], p["min_vel"]], dtype=np.float64)
    N = int(w["N"])
    c = lambda a: np.ascontiguousarray(a, np.float64)
    x0 = c(w["x0"]); B = x0.shape[0]
    Q, R, dR, Lcf, track = c(w["Q"]), c(w["R"]), c(w["dR"]), c(w["L_cf"]), c(w["track"])
    u_prev, SS, u_old, mey = c(w["u_prev"]), c(w["curv_s"]), c(w["u_old"]), c(np.broadcast_to(w["max_ey"], (B,)))
    xPred = np.empty((B, N + 1, 5)); uPred = np.empty((B, N, 2))
    status = np.empty(B, np.int32); iters = np.empty(B, np.int32)
    d = C.c_double
    f = lib().oracle_plan_tick_batch
    f.restype = C.c_int
    f(C.c_int(B), C.c_int(N), d(float(w["dt"])), _ptr(pv, d), _ptr(Q, d), _ptr(R, d), _ptr(dR, d), _ptr(Lcf, d),
      _ptr(track, d), C.c_int(track.shape[0]), _ptr(x0, d), _ptr(u_prev, d), _ptr(SS, d), _ptr(u_old, d), _ptr(mey, d),
      _ptr(xPred, d), _ptr(uPred, d), _ptr(status, C.c_int), _ptr(iters, C.c_int), C.c_int(int(nthreads)))
    return dict(xPred=xPred, uPred=uPred, status=status, iters=iters)
