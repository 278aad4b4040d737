"""Numpy restatement of the device plant with per-vehicle parameters (include/lpvmpc.h, "Per-vehicle plant parameters") and the
host replay of the fleets that use it (lpvmpc_cl_init_vehicles, lpvmpc_race_init_vehicles).

  * simulator_f_row: oracle.plant_ref.simulator_f with a row [lf, lr, m, Iz, Cf, Cr, mu] -- the same expressions, with the tyre
    stiffnesses Cf, Cr where Simulator.f has 60, so that the nominal row gives simulator_f's words.  Pinned for lf, lr, m, Iz and mu
    by tests/golden/plant_params/plant_params.npz (the reference's own main loop, whose tyre is the constant 60); Cf and Cr are
    pinned by this restatement alone.
  * VehicleRaceRef: tests/_delayed_race_ref.DelayedRaceRef whose vehicle b steps its plant with its own row; the controllers, the
    planner and the estimator keep the nominal model.  With nominal rows it is DelayedRaceRef word for word.
"""
from __future__ import annotations

import numpy as np

from oracle import plant_ref as PR
from tests import _actuator_ref as AR
from tests._delayed_race_ref import DelayedRaceRef

WORDS = ("lf", "lr", "m", "Iz", "Cf", "Cr", "mu")


def nominal_row(mu=0.05, lf=0.125, lr=0.125, m=1.98, Iz=0.03):
    """The nominal row of the reference's launch file: Simulator.f's tyre 60, mu = simulator/mu."""
    return np.array([lf, lr, m, Iz, 60.0, 60.0, mu])


def simulator_f_row(st, u, row, dt=0.005):
    """One Euler step of Simulator.f with the vehicle's row.  st = [x y vx vy ax ay yaw psiDot], u = [a, delta]."""
    x, y, vx, vy, ax, ay, yaw, w = st
    lf, lr, m, Iz, Cf, Cr, mu = (float(v) for v in row)
    aF = aR = 0.0
    if abs(vx) > 0.2:
        aF = u[1] - np.arctan((vy + lf * w) / abs(vx))
        aR = np.arctan((-vy + lr * w) / abs(vx))
    FyF, FyR = Cf * aF, Cr * aR
    nx_ = x + dt * (np.cos(yaw) * vx - np.sin(yaw) * vy)
    ny_ = y + dt * (np.sin(yaw) * vx + np.cos(yaw) * vy)
    nvx = vx + dt * (ax + w * vy)
    nvy = vy + dt * (ay - w * vx)
    nax = u[0] - mu * vx - FyF / m * np.sin(u[1])
    nay = 1.0 / m * (FyF * np.cos(u[1]) + FyR)
    nyaw = yaw + dt * w
    nw = w + dt * (1.0 / Iz * (lf * FyF * np.cos(u[1]) - lr * FyR))
    return np.array([nx_, ny_, abs(nvx), nvy, nax, nay, nyaw, nw])


def simulate(plant0, cmd, row, La=0, Ld=0, lld=False, dt=0.005):
    """tests/_actuator_ref.simulate with the vehicle's row: per step k, u = actuator(cmd[k] = (motor, servo)),
    state = simulator_f_row(state, u).  Returns (states [K,8], applied [K,2])."""
    act = AR.Actuator(La, Ld, lld, dt)
    st = np.array(plant0, float)
    states, applied = [], []
    for m, s in np.asarray(cmd, float):
        u = act.step(float(m), float(s))
        st = simulator_f_row(st, u, row, dt)
        states.append(st); applied.append(u)
    return np.array(states), np.array(applied)


class VehicleRaceRef(DelayedRaceRef):
    """DelayedRaceRef with plant_params [B, 7] (None: the nominal row with mu = mu_sim for every vehicle)."""

    def __init__(self, track, plant0, plant_params=None, mu_sim=0.05, dt_sim=0.005, **kw):
        DelayedRaceRef.__init__(self, track, plant0, dt_sim=dt_sim, **kw)
        B = self.B
        rows = np.broadcast_to(nominal_row(mu_sim), (B, 7)) if plant_params is None else np.asarray(plant_params, float)
        assert rows.shape == (B, 7), rows.shape
        self.rows = np.array(rows)
        self.dt_sim = dt_sim

    def _advance(self, b, st, n):
        servo, motor = self.cmd[b]
        row = self.rows[b]
        for _ in range(n):
            st = simulator_f_row(st, self.act[b].step(motor, servo), row, self.dt_sim)
            if self.veh is not None:
                self.veh[b].substep(st, servo, motor)              # the estimator reads `ecu`: the commanded input
        return st


def vehicle_lap0_replay(track, plant0, **kw):
    """The per-vehicle lap-0 fleet (lpvmpc_cl_init_vehicles, path tuning, vel_ref = 1): the race replay from HalfTrack = 0, valid
    while no vehicle reaches its lap event (as tests/_delayed_race_ref.delayed_lap0_replay)."""
    return VehicleRaceRef(track, plant0, half_track0=0, **kw)
