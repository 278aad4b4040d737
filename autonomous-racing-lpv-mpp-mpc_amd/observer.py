"""Gain-scheduled LPV state estimator (reference stateEstimator.py, EST): configuration helpers, a host-side synthesis of
usable vertex gains, and the drop-in ``GainScheduledLPVObserver`` computed on the device (lpvmpc_observer_step_batch).

The estimator's recipe, its sensors and its noise generator are written down in include/lpvmpc.h ("Gain-scheduled LPV state
estimator").  The gain tables are the caller's, in the reference's shapes: ``Llmi`` [6, 5, 16] and ``SchedVars_Limits`` [6, 2]
for the low-speed and the high-speed polytope (Estimator_Gains_LS.mat / Estimator_Gains_HS.mat, EST:230-235).
"""
from __future__ import annotations

import numpy as np

from . import _ffi

# the observer's own model constants (EST:404-410), independent of the controller's configuration
OBS_PARAMS = dict(lf=0.125, lr=0.125, m=1.98, I=0.03, Cf=60.0, Cr=60.0, mu=0.05)
C_OBS = np.array([[1., 0., 0., 0., 0., 0.],     # vx        (EST:248-252)
                  [0., 0., 1., 0., 0., 0.],     # omega
                  [0., 0., 0., 1., 0., 0.],     # x
                  [0., 0., 0., 0., 1., 0.],     # y
                  [0., 0., 0., 0., 0., 1.]])    # yaw


def _obs_params(params):
    """params None: OBS_PARAMS; a dict with OBS_PARAMS' keys; or a row [lf, lr, m, Iz, Cf, Cr, mu] (the plant rows' order)."""
    if params is None:
        return OBS_PARAMS
    if isinstance(params, dict):
        return params
    lf, lr, m, I, Cf, Cr, mu = (float(v) for v in np.asarray(params, float).ravel())
    return dict(lf=lf, lr=lr, m=m, I=I, Cf=Cf, Cr=Cr, mu=mu)


def observer_ab(vx, vy, theta, steer, params=None):
    """Continuous_AB_Comp (EST:402-436): (A_obs [6,6], B_obs [6,2]) of the observer model, with the observer's own constants or
    a vehicle's ``params`` (see ``_obs_params``)."""
    p = _obs_params(params)
    lf, lr, m, I, Cf, Cr, mu = p["lf"], p["lr"], p["m"], p["I"], p["Cf"], p["Cr"], p["mu"]
    B = np.array([[-(np.sin(steer) * Cf) / m, 1.], [(np.cos(steer) * Cf) / m, 0.], [(lf * Cf * np.cos(steer)) / I, 0.],
                  [0., 0.], [0., 0.], [0., 0.]])
    A = np.zeros((6, 6))
    A[0, 0] = -mu
    A[0, 1] = (np.sin(steer) * Cf) / (m * vx)
    A[0, 2] = (np.sin(steer) * Cf * lf) / (m * vx) + vy
    A[1, 1] = -(Cr + Cf * np.cos(steer)) / (m * vx)
    A[1, 2] = -(lf * Cf * np.cos(steer) - lr * Cr) / (m * vx) - vx
    A[2, 1] = -(lf * Cf * np.cos(steer) - lr * Cr) / (I * vx)
    A[2, 2] = -(lf * lf * Cf * np.cos(steer) + lr * lr * Cr) / (I * vx)
    A[3, 0], A[3, 1] = np.cos(theta), -np.sin(theta)
    A[4, 0], A[4, 1] = np.sin(theta), np.cos(theta)
    A[5, 2] = 1.
    return A, B


def polytope_vertices(limits):
    """The 16 vertices (vx, vy, theta, steer) of a SchedVars_Limits table [6, 2], in the order of EST:475-491's weights:
    vertex i takes the maximum of vx / vy / steer / theta where bit 3 / 2 / 1 / 0 of i is set, else the minimum."""
    lim = np.asarray(limits, float)
    out = []
    for i in range(16):
        vx = lim[0, 1] if i & 8 else lim[0, 0]
        vy = lim[1, 1] if i & 4 else lim[1, 0]
        st = lim[3, 1] if i & 2 else lim[3, 0]
        th = lim[5, 1] if i & 1 else lim[5, 0]
        out.append((vx, vy, th, st))
    return out


def observer_vertex_gains(limits, Qo=None, Ro=None, params=None):
    """``Llmi`` [6, 5, 16] for a polytope with the given SchedVars_Limits [6, 2]: at each of the 16 vertices the steady-state
    Kalman gain of (A_obs, C) from scipy's ``solve_continuous_are``, with the reference's sign convention L = -P C^T Ro^-1
    (GS_LPV_Est adds L C, so A + L C = A - P C^T Ro^-1 C is Hurwitz at every vertex).

    These are per-vertex stabilising gains, NOT the reference's LMI design (its MATLAB synthesis and the .mat files it wrote
    are not available): they make the estimator usable for tests, tools and users without those files.  Between vertices the
    blended gain is not guaranteed to stabilise; with the reference's own tables, pass those instead.  ``params``: the model
    row the vertices are built on (``observer_ab``); ``BatchedSolver.observer_design`` is the device form for whole fleets."""
    from scipy.linalg import solve_continuous_are
    Qo = np.diag([1.0, 1.0, 1.0, 1.0, 1.0, 1.0]) if Qo is None else np.asarray(Qo, float)
    Ro = np.diag([0.1, 0.1, 0.01, 0.01, 0.01]) if Ro is None else np.asarray(Ro, float)
    Ri = np.linalg.inv(Ro)
    L = np.zeros((6, 5, 16))
    for i, (vx, vy, th, st) in enumerate(polytope_vertices(limits)):
        A, _ = observer_ab(vx, vy, th, st, params)
        P = solve_continuous_are(A.T, C_OBS.T, Qo, Ro)
        L[:, :, i] = -P @ C_OBS.T @ Ri
    return L


def observer_config(Est_Gains_LS, SchedVars_Limits_LS, Est_Gains_HS, SchedVars_Limits_HS, loop_rate=200.0, init_vx=0.2,
                    psi_std=0.0, psiDot_std=0.0, x_std=0.0, y_std=0.0, v_std=0.0, n_bound=0.5, gps_freq=1000.0, seed=0,
                    vehicle_offset=0):
    """An ``lpvmpc_observer_config`` from the reference's tables and the launch file's sensor parameters (defaults:
    MAIN_LAUNCH.launch's values)."""
    cfg = _ffi.default_observer_config()
    for name, a, shape in (("L_ls", Est_Gains_LS, (6, 5, 16)), ("lim_ls", SchedVars_Limits_LS, (6, 2)),
                           ("L_hs", Est_Gains_HS, (6, 5, 16)), ("lim_hs", SchedVars_Limits_HS, (6, 2))):
        a = _ffi.f64(a, shape, name).ravel()
        getattr(cfg, name)[:] = a.tolist()
    cfg.loop_rate, cfg.init_vx = float(loop_rate), float(init_vx)
    cfg.psi_std, cfg.psiDot_std, cfg.x_std, cfg.y_std, cfg.v_std = map(float, (psi_std, psiDot_std, x_std, y_std, v_std))
    cfg.n_bound, cfg.gps_freq = float(n_bound), float(gps_freq)
    cfg.seed, cfg.vehicle_offset = int(seed) & (2 ** 64 - 1), int(vehicle_offset)
    return cfg


class GainScheduledLPVObserver(object):
    """Drop-in for the reference Estimator's observer (EST:349-492): ``GS_LPV_Est(states_est, y_meas, u)`` advances
    ``states_est`` by one step with the semantics of the reference, on the device.  Like the reference it ignores the
    ``states_est`` argument in favour of its own state, and accepts (and ignores) the AB / L callables the reference passes.
    The reference's ``curr_time > 0.02`` start-up test uses t = k / loop_rate with k the number of steps taken including the
    current one (the reference reads the ROS clock).  Attributes: states_est, vx_est, vy_est, psiDot_est, x_est, y_est,
    yaw_est, L_gain [6, 5], A_obs [6, 6], B_obs [6, 2], index (steps taken), dt."""

    def __init__(self, Est_Gains_LS, SchedVars_Limits_LS, Est_Gains_HS, SchedVars_Limits_HS, loop_rate=200.0, init_vx=0.2,
                 device=0):
        from .api import BatchedSolver
        self._cfg = observer_config(Est_Gains_LS, SchedVars_Limits_LS, Est_Gains_HS, SchedVars_Limits_HS, loop_rate=loop_rate,
                                    init_vx=init_vx)
        self._eng = BatchedSolver("controller", 8, 0.033, np.eye(6), np.eye(2), np.ones(2), device=device)
        self.dt = 1.0 / loop_rate
        self.n_states, self.n_meas = 6, 5
        self.C_obs = C_OBS.copy()
        self.index = 0
        self.L_gain = np.zeros((6, 5))
        self.A_obs = np.zeros((6, 6))
        self.B_obs = np.zeros((6, 2))
        self._set(np.array([float(init_vx), 0.0, 0.0, 0.0, 0.0, 0.0]))

    def _set(self, x):
        self.states_est = x
        self.vx_est, self.vy_est, self.psiDot_est, self.x_est, self.y_est, self.yaw_est = (float(v) for v in x)

    def GS_LPV_Est(self, states_est=None, y_meas=None, u=None, *callables):
        est, (L, A, B) = self._eng.observer_step(self._cfg, self.states_est[None, :], np.asarray(y_meas, float)[None, :],
                                                 np.asarray(u, float)[None, :], self.index + 1, want_aux=True)
        self.L_gain, self.A_obs, self.B_obs = L[0].copy(), A[0].copy(), B[0].copy()
        self._set(est[0].copy())
        self.index += 1

    def close(self):
        self._eng.close()
