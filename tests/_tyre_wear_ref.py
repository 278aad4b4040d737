"""Numpy restatement of the tyre wear and temperature (include/lpvmpc.h, "Tyre wear and temperature") and the host replay of the races
that carry it, built on tests/_disturbance_ref.DisturbedRaceRef.

  * wear_tick: the model's expressions, one per line of the header, on Python floats (IEEE float64, every product and sum rounded on
    its own): the device words equal it bit for bit.
  * Model: the rows and the state [B, 6] = (W, T, P, g, ticks, E).  Model.apply(b, st, lr, m, n, dt_sim) is one vehicle's worn tick in
    front of its n plant steps and returns the tick's g; Model.fit(mask) is the tyre change.
  * live_rows: the live plant and tyre rows of a tick, Cf, Cr and c_f = g * (gamma * base), or g * base without disturbances.
  * step_tick: the stand-alone step (lpvmpc_plant_step_worn_batch) for one vehicle with the actuator all off.
  * WornRaceRef: DisturbedRaceRef whose vehicle b is worn in front of every advance, behind its disturbances, from tick
    ``wear_attach`` on.  With all-off wear rows it is DisturbedRaceRef word for word.
"""
from __future__ import annotations

import numpy as np

from tests import _disturbance_ref as D
from tests import _tyre_ref as T

WORDS = ("k_wear", "k_hot", "k_heat", "k_cool", "T_amb", "T_opt", "k_temp", "wear_slope", "cliff_at", "cliff_slope", "g_min", "T_start")
ALL_OFF = np.array([0, 0, 0, 0, 20, 20, 0, 0, 1, 0, 1e-3, 20], float)


def _min(a, b):
    return a if a < b else b


def _max(a, b):
    return a if a > b else b


def fresh(rows):
    """The state a binding starts from: {0, T_start, 0, 1, 0, 0} per vehicle."""
    rows = np.asarray(rows, float)
    s = np.zeros((rows.shape[0], 6))
    s[:, 1] = rows[:, 11]; s[:, 3] = 1.0
    return s


def wear_tick(row, state, st, lr, m, n, dt_sim):
    """One worn tick of a vehicle about to take n > 0 plant steps from the plant state st.  Returns the new state [6]."""
    k_wear, k_hot, k_heat, k_cool, T_amb, T_opt, k_temp, wear_slope, cliff_at, cliff_slope, g_min, _ = (float(v) for v in row)
    W, Tt, _P, _g, j, E = (float(v) for v in state)
    vx, vy, ay, w = float(st[2]), float(st[3]), float(st[5]), float(st[7])
    lr, m = float(lr), float(m)
    dl = float(n) * float(dt_sim)
    vs = abs(-vy + lr * w) if abs(vx) > 0.2 else 0.0
    F = m * abs(ay)
    P = F * vs
    E = E + P * dl
    hot = _max(0.0, Tt - T_opt)
    W = _min(1.0, W + ((k_wear * P) * dl) * (1.0 + k_hot * hot))
    Tt = Tt + dl * (k_heat * P - k_cool * (Tt - T_amb))
    d = Tt - T_opt
    gT = 1.0 - (k_temp * d) * d
    gW = (1.0 - wear_slope * W) - cliff_slope * _max(0.0, W - cliff_at)
    g = _min(1.0, _max(g_min, gW * gT))
    return np.array([W, Tt, P, g, j + 1.0, E])


class Model(object):
    def __init__(self, rows, state=None):
        self.rows = np.array(rows, float)
        self.B = self.rows.shape[0]
        assert self.rows.shape == (self.B, 12)
        self.state = fresh(self.rows) if state is None else np.array(state, float)

    def apply(self, b, st, lr, m, n, dt_sim):
        """One worn tick of vehicle b; a frozen vehicle (n <= 0) is not touched.  Returns g."""
        if n > 0:
            self.state[b] = wear_tick(self.rows[b], self.state[b], st, lr, m, n, dt_sim)
        return float(self.state[b, 3])

    def fit(self, mask):
        mask = np.asarray(mask, bool)
        self.state[mask, 0] = 0.0; self.state[mask, 1] = self.rows[mask, 11]; self.state[mask, 2] = 0.0; self.state[mask, 3] = 1.0


def live_rows(row, tyre, g, gamma=None):
    """The live plant and tyre rows of a tick: Cf, Cr and c_f = g * (gamma * base); gamma None: g * base."""
    row, tyre = np.array(row, float), np.array(tyre, float)
    for a, i in ((row, 4), (row, 5), (tyre, 3)):
        a[i] = g * a[i] if gamma is None else g * (gamma * a[i])
    return row, tyre


def step_tick(model, b, st, u, row, tyre, n, dt_sim, dist=None, k0=0, track=None, hw=0.3, slack=0.15):
    """lpvmpc_plant_step_worn_batch for vehicle b with the actuator all off.  dist: a _disturbance_ref.Model applied first (None: no
    disturbance model).  Returns (st, live_row, live_tyre)."""
    st = np.array(st, float)
    gamma = None
    if dist is not None:
        st, gamma = dist.apply(b, st, k0, n, dt_sim, track, hw, slack)
    g = model.apply(b, st, row[1], row[2], n, dt_sim)
    lrow, ltyre = live_rows(row, tyre, g, gamma)
    hook = T.pacejka_forces(ltyre)
    for _ in range(n):
        st = T.simulator_f_forces(st, u, lrow, hook, dt_sim)
    return st, lrow, ltyre


class WornRaceRef(D.DisturbedRaceRef):
    """DisturbedRaceRef (rows None: never disturbed) with wear rows [B, 12] attached from tick wear_attach on."""

    def __init__(self, track, plant0, wear_rows, rows=None, wear_attach=0, **kw):
        B = np.asarray(plant0).shape[0]
        self.disturbed = rows is not None
        D.DisturbedRaceRef.__init__(self, track, plant0, np.tile(D.ALL_OFF, (B, 1)) if rows is None else rows, **kw)
        self.wear = Model(wear_rows)
        self.wear_attach = wear_attach

    def _advance(self, b, st, n):
        if self.t < self.wear_attach or n <= 0:
            return D.DisturbedRaceRef._advance(self, b, st, n)
        dist_on = self.disturbed and self.t >= self.attach_tick and (self.detach_tick is None or self.t < self.detach_tick)
        base_row, base_hook = self.rows[b].copy(), self.hooks[b]
        gamma = None
        if dist_on:
            st, gamma = self.model.apply(b, st, self.act[b].k, n, self.dt_sim, self.track, self.hw, self.slack)
        g = self.wear.apply(b, st, base_row[1], base_row[2], n, self.dt_sim)
        row, tyre = live_rows(base_row, self.tyres[b], g, gamma)
        self.rows[b], self.hooks[b] = row, T.pacejka_forces(tyre)
        try:
            return T.TyreRaceRef._advance(self, b, st, n)
        finally:
            self.rows[b], self.hooks[b] = base_row, base_hook


# ---- the worn race of tests/test_tyre_wear_host.py and tests/test_gpu_tyre_wear.py --------------------------------------------------
# test_disturbed_race_matches_the_replay's fleet (seed 17, B = 8, the launch file's Pacejka tyre, laps = 3) with wear attached at tick
# 10.  The rows were chosen on the replay alone: the sliding power of these cars is 0.005 .. 0.03 W in a vehicle's first 24 racing
# ticks, so k_wear = 150 takes most of them over cliff_at = 0.3 inside their window, two of them down to g_min, and k_heat = 1500
# warms the sets by 1 .. 6 K towards and past T_opt.
RACE_B, RACE_WINDOW, RACE_ATTACH, RACE_LAPS, RACE_SEED = 8, 24, 10, 3, 17
RACE_WEAR = dict(k_wear=150.0, k_hot=0.05, k_heat=1500.0, k_cool=0.5, T_amb=20.0, T_opt=28.0, k_temp=4e-4, wear_slope=0.6, cliff_at=0.3,
                 cliff_slope=1.5, g_min=0.5, T_start=22.0)


def race_case():
    """(map, plant0, plant rows, tyre rows, wear rows, replay) of the worn race."""
    import lpvmpc
    from tests import _race_observer_ref as RO
    mp = lpvmpc.Map("L_shape", 0.2)
    B = RACE_B
    plant0 = RO.start_line_fleet(mp.PointAndTangent, B, RACE_SEED, 0.90, 0.975)
    prow, tyres = lpvmpc.sample_plant_params(B, 23), lpvmpc.tyre_params(B)
    rows = lpvmpc.tyre_wear_rows(B, **RACE_WEAR)
    ref = WornRaceRef(mp.PointAndTangent, plant0, rows, wear_attach=RACE_ATTACH, tyre_params=tyres, plant_params=prow, half_track0=1,
                      laps=RACE_LAPS, half_width=mp.halfWidth, slack=mp.slack)
    return mp, plant0, prow, tyres, rows, ref
