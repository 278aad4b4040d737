"""Numpy restatement (test infrastructure) of the device gain design of csrc/observer_design.hip and of the per-vehicle
observer step: the same algorithm with the same pivot rule, not the same summation order.

Design, per (vehicle row, polytope, vertex): A = A_obs at the vertex from the row's seven words, Hamiltonian
Z = [[A^T, -C^T Ro^-1 C], [-Qo, -A]], matrix-sign Newton iteration Z <- (c Z + Z^-1 / c) / 2 with c = sqrt(|Z^-1|_F / |Z|_F),
the inverse by Gauss-Jordan with partial pivoting (largest magnitude, lowest row on a tie), stop at |dZ|_F <= 1e-13 |Z|_F within
40 iterations, P from the normal equations of [W12; W22 + I] P = -[W11 + I; W21] by a 6 x 6 Cholesky, symmetrised, and
L = -P C^T Ro^-1.  A problem that does not stop within the cap gives NaN gains and iteration count -1."""
import math

import numpy as np

import _observer_ref as R

NOMINAL_ROW = np.array([0.125, 0.125, 1.98, 0.03, 60.0, 60.0, 0.05])
C_OBS = np.zeros((5, 6)); C_OBS[0, 0] = C_OBS[1, 2] = C_OBS[2, 3] = C_OBS[3, 4] = C_OBS[4, 5] = 1.0
QO_DEFAULT = np.eye(6)
RO_DEFAULT = np.diag([0.1, 0.1, 0.01, 0.01, 0.01])
STOP, CAP = 1e-13, 40


def vertices(lim):
    """polytope_vertices' order: bit 3 / 2 / 1 / 0 of i takes the maximum of vx / vy / steer / theta."""
    lim = np.asarray(lim, float).reshape(6, 2)
    return [(lim[0, (i >> 3) & 1], lim[1, (i >> 2) & 1], lim[5, i & 1], lim[3, (i >> 1) & 1]) for i in range(16)]


def a_obs(row, vx, vy, th, steer):
    """Continuous_AB_Comp as obs_step writes it, the seven constants from the row."""
    lf, lr, m, I, Cf, Cr, mu = (float(v) for v in row)
    s, c = math.sin(steer), math.cos(steer)
    B = np.array([[-(s * Cf) / m, 1.], [(c * Cf) / m, 0.], [(lf * Cf * c) / I, 0.], [0., 0.], [0., 0.], [0., 0.]])
    A = np.zeros((6, 6))
    A[0, 0] = -mu; A[0, 1] = (s * Cf) / (m * vx); A[0, 2] = (s * Cf * lf) / (m * vx) + vy
    A[1, 1] = -(Cr + Cf * c) / (m * vx); A[1, 2] = -(lf * Cf * c - lr * Cr) / (m * vx) - vx
    A[2, 1] = -(lf * Cf * c - lr * Cr) / (I * vx); A[2, 2] = -(lf * lf * Cf * c + lr * lr * Cr) / (I * vx)
    A[3, 0], A[3, 1] = math.cos(th), -math.sin(th)
    A[4, 0], A[4, 1] = math.sin(th), math.cos(th)
    A[5, 2] = 1.0
    return A, B


def gj_inverse(Z):
    """Batched Gauss-Jordan inverse [n, 12, 12] without row exchanges: step p takes the unused row with the largest |a[., p]|."""
    n, d, _ = Z.shape
    a = np.concatenate([Z, np.broadcast_to(np.eye(d), (n, d, d))], axis=2).copy()
    used = np.zeros((n, d), bool)
    src = np.zeros((n, d), int)
    ar = np.arange(n)
    for p in range(d):
        cand = np.where(used, -1.0, np.abs(a[:, :, p]))
        piv = np.argmax(cand, axis=1)                                  # first (lowest row) of the largest
        prow = a[ar, piv, :].copy()                                    # [n, 2d]
        with np.errstate(all="ignore"):
            f = a[:, :, p] / prow[:, None, p]                          # [n, d]
            upd = a - f[:, :, None] * prow[:, None, :]
            upd[ar, piv, :] = prow / prow[:, None, p]
        a = upd
        a[:, :, p] = 0.0
        a[ar, piv, p] = 1.0
        used[ar, piv] = True
        src[:, p] = piv
    return np.take_along_axis(a[:, :, d:], src[:, :, None], axis=1)


def design(rows, lim_ls, lim_hs, Qo=None, Ro=None):
    """(L_ls [B, 6, 5, 16], L_hs, iters [B, 2, 16], P [B, 2, 16, 6, 6]) for rows [B, 7]."""
    rows = np.asarray(rows, float).reshape(-1, 7)
    Qo = QO_DEFAULT if Qo is None else np.asarray(Qo, float)
    Ro = RO_DEFAULT if Ro is None else np.asarray(Ro, float)
    Ri = np.linalg.inv(Ro)
    G = C_OBS.T @ Ri @ C_OBS
    B = rows.shape[0]
    Z = np.zeros((B, 2, 16, 12, 12))
    for b in range(B):
        for p, lim in enumerate((lim_ls, lim_hs)):
            for i, (vx, vy, th, st) in enumerate(vertices(lim)):
                A = a_obs(rows[b], vx, vy, th, st)[0]
                Z[b, p, i] = np.block([[A.T, -G], [-Qo, -A]])
    Z = Z.reshape(-1, 12, 12)
    n = Z.shape[0]
    iters = np.full(n, -1)
    W = np.full_like(Z, np.nan)
    live = np.arange(n)
    Zc = Z.copy()
    for k in range(1, CAP + 1):
        Zi = gj_inverse(Zc)
        with np.errstate(all="ignore"):
            c = np.sqrt(np.sqrt((Zi ** 2).sum((1, 2))) / np.sqrt((Zc ** 2).sum((1, 2))))[:, None, None]
            Zn = 0.5 * (c * Zc + Zi / c)
            done = np.sqrt(((Zn - Zc) ** 2).sum((1, 2))) <= STOP * np.sqrt((Zn ** 2).sum((1, 2)))
        W[live[done]] = Zn[done]
        iters[live[done]] = k
        live, Zc = live[~done], Zn[~done]
        if live.size == 0:
            break
    I6 = np.eye(6)
    P = np.full((n, 6, 6), np.nan)
    for q in np.nonzero(iters > 0)[0]:
        M = np.vstack([W[q, :6, 6:], W[q, 6:, 6:] + I6])
        N = -np.vstack([W[q, :6, :6] + I6, W[q, 6:, :6]])
        S, T = M.T @ M, M.T @ N
        try:
            Lc = np.linalg.cholesky(S)
        except np.linalg.LinAlgError:
            iters[q] = -1
            continue
        X = np.linalg.solve(Lc.T, np.linalg.solve(Lc, T))
        P[q] = 0.5 * (X + X.T)
    L = (-P @ C_OBS.T @ Ri).reshape(B, 2, 16, 6, 5)
    L = np.moveaxis(L, 2, 4)                                           # [B, 2, 6, 5, 16]
    return np.ascontiguousarray(L[:, 0]), np.ascontiguousarray(L[:, 1]), iters.reshape(B, 2, 16), P.reshape(B, 2, 16, 6, 6)


def care_residual(A, P, Qo=None, Ro=None):
    """max |A P + P A^T - P C^T Ro^-1 C P + Qo| / max(1, |P|_inf) of the filter equation."""
    Qo = QO_DEFAULT if Qo is None else np.asarray(Qo, float)
    Ro = RO_DEFAULT if Ro is None else np.asarray(Ro, float)
    G = C_OBS.T @ np.linalg.inv(Ro) @ C_OBS
    Rm = A @ P + P @ A.T - P @ G @ P + Qo
    return float(np.max(np.abs(Rm)) / max(1.0, np.max(np.abs(P))))


def p_of_gain(A, L, Qo=None, Ro=None):
    """The P behind a gain L [6, 5] = -P C^T Ro^-1 at A: five of its columns are -L Ro; the unmeasured state's row / column
    follows from symmetry, and P[1][1] from row 1 of the filter equation (its (1, 1) entry is linear in P[1][1])."""
    Qo = QO_DEFAULT if Qo is None else np.asarray(Qo, float)
    Ro = RO_DEFAULT if Ro is None else np.asarray(Ro, float)
    G = C_OBS.T @ np.linalg.inv(Ro) @ C_OBS
    P = np.zeros((6, 6))
    P[:, [0, 2, 3, 4, 5]] = -np.asarray(L, float) @ Ro
    P[[0, 2, 3, 4, 5], 1] = P[1, [0, 2, 3, 4, 5]]
    # entry (1, 1) of A P + P A^T - P G P + Qo with P[1][1] = t: G has no row / column 1, so P G P's (1, 1) entry does not hold t
    R0 = A @ P + P @ A.T - P @ G @ P + Qo
    P[1, 1] = -R0[1, 1] / (2.0 * A[1, 1])
    return P


def observer_step(row, L_ls, L_hs, lim_ls, lim_hs, x, y, u, k, dt):
    """One GS_LPV_Est step of a vehicle with its own model row and gain tables; limits as the configuration's.  The operations
    and their order are _observer_ref.observer_step's.  Returns (x_new, L, A, B)."""
    x = np.asarray(x, float); y = np.asarray(y, float)
    lim_ls, lim_hs = np.asarray(lim_ls, float).reshape(6, 2), np.asarray(lim_hs, float).reshape(6, 2)
    steer = u[0]
    if k * dt > 0.02:
        vx, vy, th = x[0], x[1], x[5]
    else:
        vx, vy, th = y[0], 0.0, y[4]
    A, B = a_obs(row, vx, vy, th, steer)
    if vx > lim_ls[0][1]:
        lim, G = lim_hs, np.asarray(L_hs)
    else:
        lim, G = lim_ls, np.asarray(L_ls)
    M = [(lim[0, 1] - vx) / (lim[0, 1] - lim[0, 0]), (lim[1, 1] - vy) / (lim[1, 1] - lim[1, 0]),
         (lim[3, 1] - steer) / (lim[3, 1] - lim[3, 0]), (lim[5, 1] - th) / (lim[5, 1] - lim[5, 0])]
    L = np.zeros((6, 5))
    for i in range(16):
        f = [1 - M[j] if i & (8 >> j) else M[j] for j in range(4)]
        L = L + f[0] * f[1] * f[2] * f[3] * G[:, :, i]
    xn = x + (dt * (A + L @ C_OBS) @ x + dt * B @ np.asarray(u, float) - dt * L @ y)
    return xn, L, A, B


class Vehicle(R.Vehicle):
    """_observer_ref.Vehicle whose observer step takes the vehicle's model row and its own gain tables."""

    def __init__(self, row, L_ls, L_hs, lim_ls, lim_hs, plant0, **kw):
        g = dict(L_ls=np.asarray(L_ls), L_hs=np.asarray(L_hs), lim_ls=np.asarray(lim_ls).reshape(6, 2),
                 lim_hs=np.asarray(lim_hs).reshape(6, 2))
        R.Vehicle.__init__(self, g, plant0, **kw)
        self.row = np.asarray(row, float)

    def substep(self, st, servo, motor):
        g = self.g
        # the parent's sensors, then the per-vehicle step in place of its observer_step
        real = R.observer_step
        R.observer_step = lambda g_, x, y, u, k, dt: observer_step(self.row, g["L_ls"], g["L_hs"], g["lim_ls"], g["lim_hs"], x, y, u, k, dt)
        try:
            return R.Vehicle.substep(self, st, servo, motor)
        finally:
            R.observer_step = real


# ---- the fixture and the yardstick that the device design is held to ---------------------------------------------------------
def fixture():
    import os
    return dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "estimator_vehicles", "design.npz")))


def gain_error(L, want):
    """Worst over vehicles and vertices of max |L - want| / max |want| per vertex table [6, 5]; L, want [B, 6, 5, 16]."""
    n = L.shape[0]
    return float((np.abs(L - want).reshape(n, 30, 16).max(1) / np.abs(want).reshape(n, 30, 16).max(1)).max())


def residual_of_gains(rows, lim, L, Qo=None, Ro=None):
    """Worst relative residual of the filter equation over vehicles and vertices, from the gains alone (p_of_gain); also the
    largest real part of an eigenvalue of A + L C."""
    worst, re = 0.0, -np.inf
    for b in range(len(rows)):
        for i, (vx, vy, th, st) in enumerate(vertices(lim)):
            A = a_obs(rows[b], vx, vy, th, st)[0]
            worst = max(worst, care_residual(A, p_of_gain(A, L[b, :, :, i], Qo, Ro), Qo, Ro))
            re = max(re, float(np.max(np.linalg.eigvals(A + L[b, :, :, i] @ C_OBS).real)))
    return worst, re


_YARD = {}


def yardstick():
    """The restatement against the fixture's scipy gains on all 1280 problems of set 1: dict(gain=worst relative gain error,
    resid=worst relative residual from the gains, iters=(min, max), L_ls, L_hs).  Computed once per process."""
    if not _YARD:
        f = fixture()
        L_ls, L_hs, it, _ = design(f["rows"], f["lim_ls"], f["lim_hs"])
        _YARD.update(gain=max(gain_error(L_ls, f["L_ls"]), gain_error(L_hs, f["L_hs"])),
                     resid=max(residual_of_gains(f["rows"], f["lim_ls"], L_ls)[0], residual_of_gains(f["rows"], f["lim_hs"], L_hs)[0]),
                     iters=(int(it.min()), int(it.max())), L_ls=L_ls, L_hs=L_hs)
    return _YARD
