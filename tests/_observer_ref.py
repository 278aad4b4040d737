"""Numpy restatement (test infrastructure) of the gain-scheduled LPV estimator, its sensors and its noise generator as
include/lpvmpc.h documents them.  Pinned against the reference by tests/golden/estimator/estimator.npz."""
import math

import numpy as np

MASK = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
CHANNELS = ("psi", "psiDot", "x", "y", "v")


def mix(z):
    z &= MASK
    z ^= z >> 30; z = (z * 0xBF58476D1CE4E5B9) & MASK
    z ^= z >> 27; z = (z * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def uniforms(seed, vid, step, ch):
    key = mix(mix(seed + GOLDEN * (vid + 1)) ^ (8 * step + ch))
    u1 = ((mix(key + GOLDEN) >> 11) + 1) * 2.0 ** -53
    u2 = (mix(key + 2 * GOLDEN) >> 11) * 2.0 ** -53
    return u1, u2


def gauss(seed, vid, step, ch):
    u1, u2 = uniforms(seed, vid, step, ch)
    return math.sqrt(-2.0 * math.log(u1)) * math.cos(2.0 * math.pi * u2)


def noise(std, n_bound, seed, vid, step, ch):
    if std == 0.0:
        return 0.0
    n, lim = std * gauss(seed, vid, step, ch), std * n_bound
    return max(-lim, min(n, lim))


def observer_step(g, x, y, u, k, dt):
    """One GS_LPV_Est step.  g: dict(L_ls, lim_ls, L_hs, lim_hs); returns (x_new, L, A, B)."""
    x = np.asarray(x, float); y = np.asarray(y, float)
    steer = u[0]
    if k * dt > 0.02:
        vx, vy, th = x[0], x[1], x[5]
    else:
        vx, vy, th = y[0], 0.0, y[4]
    lf = lr = 0.125; m = 1.98; I = 0.03; Cf = Cr = 60.0; mu = 0.05
    s, c = math.sin(steer), math.cos(steer)
    B = np.array([[-(s * Cf) / m, 1.], [(c * Cf) / m, 0.], [(lf * Cf * c) / I, 0.], [0., 0.], [0., 0.], [0., 0.]])
    A = np.zeros((6, 6))
    A[0, 0] = -mu; A[0, 1] = (s * Cf) / (m * vx); A[0, 2] = (s * Cf * lf) / (m * vx) + vy
    A[1, 1] = -(Cr + Cf * c) / (m * vx); A[1, 2] = -(lf * Cf * c - lr * Cr) / (m * vx) - vx
    A[2, 1] = -(lf * Cf * c - lr * Cr) / (I * vx); A[2, 2] = -(lf * lf * Cf * c + lr * lr * Cr) / (I * vx)
    A[3, 0], A[3, 1] = math.cos(th), -math.sin(th)
    A[4, 0], A[4, 1] = math.sin(th), math.cos(th)
    A[5, 2] = 1.0
    if vx > g["lim_ls"][0][1]:
        lim, G = np.asarray(g["lim_hs"]), np.asarray(g["L_hs"])
    else:
        lim, G = np.asarray(g["lim_ls"]), np.asarray(g["L_ls"])
    M = [(lim[0, 1] - vx) / (lim[0, 1] - lim[0, 0]), (lim[1, 1] - vy) / (lim[1, 1] - lim[1, 0]),
         (lim[3, 1] - steer) / (lim[3, 1] - lim[3, 0]), (lim[5, 1] - th) / (lim[5, 1] - lim[5, 0])]
    L = np.zeros((6, 5))
    for i in range(16):
        f = [1 - M[j] if i & (8 >> j) else M[j] for j in range(4)]
        L = L + f[0] * f[1] * f[2] * f[3] * G[:, :, i]
    Cm = np.zeros((5, 6)); Cm[0, 0] = Cm[1, 2] = Cm[2, 3] = Cm[3, 4] = Cm[4, 5] = 1.0
    xn = x + (dt * (A + L @ Cm) @ x + dt * B @ np.asarray(u, float) - dt * L @ y)
    return xn, L, A, B


class Vehicle(object):
    """Sensors + observer of one vehicle, in the fleet's convention (estimate [init_vx, 0, 0, x0, y0, yaw0], GPS hold at the
    start position) unless est0 / gps0 are given."""

    def __init__(self, g, plant0, init_vx=0.2, dt=0.005, dt_sim=0.005, gps_freq=1000.0, stds=(0, 0, 0, 0, 0), n_bound=0.5,
                 seed=0, vid=0, est0=None, gps0=None):
        self.g, self.dt, self.stds, self.n_bound, self.seed, self.vid = g, dt, [float(s) for s in stds], n_bound, seed, vid
        self.th = (1.0 / gps_freq) / dt_sim
        self.est = (np.array(est0, float) if est0 is not None
                    else np.array([init_vx, 0, 0, plant0[0], plant0[1], plant0[6]], float))
        self.gps = list(gps0) if gps0 is not None else [plant0[0], plant0[1]]
        self.gps_cnt = 0.0; self.enc_prev = 0.0; self.enc_meas = 0.0; self.enc_cnt = 0.0
        self.k = 0
        self.y = np.zeros(5)
        self.draws = []

    def n(self, step, ch):
        v = noise(self.stds[ch], self.n_bound, self.seed, self.vid, step, ch)
        self.draws.append(v)
        return v

    def substep(self, st, servo, motor):
        self.k += 1
        k = self.k
        imu_yaw = st[6] + self.n(k, 0); imu_w = st[7] + self.n(k, 1)
        gx = st[0] + self.n(k, 2); gy = st[1] + self.n(k, 3)
        if self.gps_cnt > self.th:
            self.gps_cnt = 0.0; self.gps = [gx, gy]
        else:
            self.gps_cnt += 1.0
        v = math.sqrt(st[2] * st[2] + st[3] * st[3]) + self.n(k, 4)
        if v != self.enc_prev:
            self.enc_meas = v; self.enc_cnt = 0.0
        else:
            self.enc_cnt += 1.0
            if self.enc_cnt > 40:
                self.enc_meas = 0.0
        self.enc_prev = v
        if k * self.dt > 0.02:
            y = [self.enc_meas, imu_w, self.gps[0], self.gps[1], imu_yaw]
        else:
            y = [self.est[0], imu_w, self.gps[0], self.gps[1], st[6]]
        self.y = np.array(y)
        self.est = observer_step(self.g, self.est, self.y, [servo, motor], k, self.dt)[0]
        return self.y
