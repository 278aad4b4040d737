"""Numpy restatement of the plant disturbances (include/lpvmpc.h, "Plant disturbances") and the host replay of the fleets that carry
them: gusts on tests/_observer_ref.gauss, grip patches on oracle.plant_ref.get_local_position, the plant on tests/_tyre_ref.

  * Model: the rows, the configuration and the state [B, 5] = (d_ax, d_ay, d_aw, ticks, gamma).  Model.apply(b, st, k0, n, ...) is one
    vehicle's disturbed tick in front of its n plant steps: it returns the plant state the steps start from and the tick's gamma.
  * step_tick: the stand-alone step (lpvmpc_plant_step_disturbed_batch) for one vehicle with the actuator all off.
  * DisturbedRaceRef: tests/_tyre_ref.TyreRaceRef whose vehicle b is disturbed in front of every advance, from tick ``attach_tick`` on
    (detached again from ``detach_tick`` on).  With all-off rows it is TyreRaceRef word for word.
"""
from __future__ import annotations

import math

import numpy as np

from oracle import plant_ref as PR
from tests import _observer_ref as OR
from tests import _tyre_ref as T

DIST_STREAM = 0xD157A2B3C4D5E6F7                       # LPVMPC_DIST_STREAM
WORDS = ("sigma_ax", "sigma_ay", "sigma_aw", "rho", "kick_step", "kick_vy", "kick_w", "p0_s0", "p0_len", "p0_gamma", "p1_s0", "p1_len",
         "p1_gamma")
ALL_OFF = np.array([0, 0, 0, 0, -1, 0, 0, 0, 0, 1, 0, 0, 1], float)


def lap_length(track):
    track = np.asarray(track, float)
    return float(track[-1, 3] + track[-1, 4])


def patch_gamma(row, s, inside, L):
    """gamma of one vehicle at arc length s: the product of the patches that contain s; 1 off the map."""
    g = 1.0
    if not inside:
        return g
    for p in (0, 1):
        s0, ln, gp = row[7 + 3 * p], row[8 + 3 * p], row[9 + 3 * p]
        d = s - s0
        if d < 0:
            d += L
        if d < ln:
            g *= gp
    return g


def kick_applies(kick_step, k0, n):
    """The tick whose plant steps are k0 .. k0 + n - 1 holds kick_step."""
    return k0 <= kick_step < k0 + n


class Model(object):
    def __init__(self, rows, seed=0, vehicle_offset=0, n_bound=3.0, state=None):
        self.rows = np.array(rows, float)
        self.B = self.rows.shape[0]
        assert self.rows.shape == (self.B, 13)
        self.seed = (int(seed) ^ DIST_STREAM) & OR.MASK
        self.voff, self.n_bound = int(vehicle_offset), float(n_bound)
        self.q = np.array([math.sqrt(1.0 - r * r) for r in self.rows[:, 3]])
        if state is None:
            self.state = np.zeros((self.B, 5)); self.state[:, 4] = 1.0
        else:
            self.state = np.array(state, float)

    def gust(self, b, ch):
        """The channel's next value (its state is advanced), or None where sigma is 0."""
        r, stt = self.rows[b], self.state[b]
        sigma = r[ch]
        if sigma == 0.0:
            return None
        j = int(stt[3])
        g = OR.gauss(self.seed, self.voff + b, j, ch)
        g = max(-self.n_bound, min(g, self.n_bound))
        d = sigma * g if j == 0 else r[3] * stt[ch] + sigma * self.q[b] * g
        stt[ch] = d
        return d

    def apply(self, b, st, k0, n, dt_sim, track, hw, slack):
        """One disturbed tick of vehicle b whose plant is about to take n steps from its step counter k0.  Returns (st, gamma)."""
        if n <= 0:
            return st, self.state[b, 4]
        st = np.array(st, float)
        r = self.rows[b]
        s, _ey, _epsi, inside = PR.get_local_position(track, hw, slack, st[0], st[1], st[6])
        gamma = patch_gamma(r, s, inside, lap_length(track))
        T_ = float(n) * dt_sim
        d = self.gust(b, 0)
        if d is not None:
            st[2] = abs(st[2] + d * T_)
        d = self.gust(b, 1)
        if d is not None:
            st[3] = st[3] + d * T_
        d = self.gust(b, 2)
        if d is not None:
            st[7] = st[7] + d * T_
        if kick_applies(r[4], k0, n):
            st[3] = st[3] + r[5]; st[7] = st[7] + r[6]
        self.state[b, 3] += 1.0
        self.state[b, 4] = gamma
        return st, gamma


def scaled(row, tyre, gamma):
    """The live plant and tyre rows of a tick: Cf, Cr and c_f times gamma."""
    row, tyre = np.array(row, float), np.array(tyre, float)
    row[4] = gamma * row[4]; row[5] = gamma * row[5]; tyre[3] = gamma * tyre[3]
    return row, tyre


def step_tick(model, b, st, k0, u, row, tyre, n, dt_sim, track, hw, slack, ignore_rows=False):
    """lpvmpc_plant_step_disturbed_batch for vehicle b with the actuator all off: u = (motor, servo) held n steps.  ignore_rows: the
    plant alone (the guard of the tests: a restatement that ignores the rows)."""
    st = np.array(st, float)
    if not ignore_rows:
        st, gamma = model.apply(b, st, k0, n, dt_sim, track, hw, slack)
        row, tyre = scaled(row, tyre, gamma)
    hook = T.pacejka_forces(tyre)
    for _ in range(n):
        st = T.simulator_f_forces(st, u, row, hook, dt_sim)
    return st


class DisturbedRaceRef(T.TyreRaceRef):
    """TyreRaceRef with disturbance rows [B, 13] attached from tick attach_tick on (until detach_tick, None: never detached)."""

    def __init__(self, track, plant0, rows, dist_seed=0, dist_offset=0, dist_n_bound=3.0, attach_tick=0, detach_tick=None, **kw):
        T.TyreRaceRef.__init__(self, track, plant0, **kw)                 # (seed, vehicle_offset, n_bound in kw are the estimator's)
        self.model = Model(rows, dist_seed, dist_offset, dist_n_bound)
        self.attach_tick, self.detach_tick = attach_tick, detach_tick

    def _advance(self, b, st, n):
        on = self.t >= self.attach_tick and (self.detach_tick is None or self.t < self.detach_tick)
        if not on:
            return T.TyreRaceRef._advance(self, b, st, n)
        base_row, base_hook = self.rows[b].copy(), self.hooks[b]
        st, gamma = self.model.apply(b, st, self.act[b].k, n, self.dt_sim, self.track, self.hw, self.slack)
        row, tyre = scaled(base_row, self.tyres[b], gamma)
        self.rows[b], self.hooks[b] = row, T.pacejka_forces(tyre)
        try:
            return T.TyreRaceRef._advance(self, b, st, n)
        finally:
            self.rows[b], self.hooks[b] = base_row, base_hook


def gust_bars(B, rho):
    """Five standard errors of the sample standard deviation, mean and lag-1 correlation of B independent unit-variance draws."""
    return 5.0 / math.sqrt(2.0 * B), 5.0 / math.sqrt(B), 5.0 * (1.0 - rho * rho) / math.sqrt(B)


def gust_stats(d_a, d_b):
    """(std, mean) of d_a and the correlation of d_a with d_b, across vehicles."""
    d_a, d_b = np.asarray(d_a, float), np.asarray(d_b, float)
    return float(np.std(d_a)), float(np.mean(d_a)), float(np.corrcoef(d_a, d_b)[0, 1])


GUST_CASE = dict(B=4096, sigma=1.0, rho=0.8, n_bound=10.0, seed=20261, calls=22)   # tick 20 against tick 21 (0-based)
