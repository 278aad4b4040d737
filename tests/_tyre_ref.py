"""Numpy restatement of the device plant with a tyre row per vehicle (include/lpvmpc.h, "Tyre model") and the host replay of the
fleets that use it (lpvmpc_cl_init_tyres, lpvmpc_race_init_tyres).

  * simulator_f_forces: tests/_plant_params_ref.simulator_f_row's expressions around a hook forces(aF, aR, row) -> (FyF, FyR).  With
    linear_forces it is simulator_f_row word for word (tests/test_tyre_host.py), and so pinned to the reference's own loop by
    tests/golden/plant_params/.
  * pacejka_forces(tyre): the hook of a tyre row [kind, B, C, c_f] -- kind 0 the linear tyre of the plant row, kind 1
    lpvmpc.plant.pacejka on both axles with the row's mass.  The curve is pinned by tests/golden/tyre/tyre.npz, whose generator
    calls the reference's own Simulator.pacejka through this module's hook; the two calls in Simulator.f are commented out in the
    reference (vehicleSimulator.py:172-173), so the curve is the reference's and the recursion around it this restatement.
  * TyreRaceRef: tests/_plant_params_ref.VehicleRaceRef whose vehicle b steps with its own tyre row; the controllers, the planner
    and the estimator keep the nominal, linear-tyre model.  With kind 0 rows it is VehicleRaceRef word for word.
"""
from __future__ import annotations

import numpy as np

from tests import _actuator_ref as AR
from tests._plant_params_ref import VehicleRaceRef

LAUNCH_FILE = (1.0, 6.0, 1.6, 0.8)                       # kind 1, simulator/B, simulator/C, simulator/c_f
SOFT = (1.0, 4.0, 1.3, 0.5)


def linear_forces(aF, aR, row):
    return row[4] * aF, row[5] * aR


def pacejka_forces(tyre):
    """The force hook of the tyre row [kind, B, C, c_f]."""
    from lpvmpc.plant import pacejka
    tyre = np.asarray(tyre, float)
    if tyre[0] == 0.0:
        return linear_forces
    return lambda aF, aR, row: (float(pacejka(aF, row[2], tyre)), float(pacejka(aR, row[2], tyre)))


def slip_angles(st, u, row):
    vx, vy, w = st[2], st[3], st[7]
    aF = aR = 0.0
    if abs(vx) > 0.2:
        aF = u[1] - np.arctan((vy + row[0] * w) / abs(vx))
        aR = np.arctan((-vy + row[1] * w) / abs(vx))
    return aF, aR


def simulator_f_forces(st, u, row, forces, dt=0.005):
    """One Euler step of Simulator.f with the vehicle's row and the lateral forces of ``forces``.  st = [x y vx vy ax ay yaw psiDot],
    u = [a, delta]."""
    x, y, vx, vy, ax, ay, yaw, w = st
    row = [float(v) for v in row]
    lf, lr, m, Iz, _Cf, _Cr, mu = row
    aF, aR = slip_angles(st, u, row)
    FyF, FyR = forces(aF, aR, row)
    nx_ = x + dt * (np.cos(yaw) * vx - np.sin(yaw) * vy)
    ny_ = y + dt * (np.sin(yaw) * vx + np.cos(yaw) * vy)
    nvx = vx + dt * (ax + w * vy)
    nvy = vy + dt * (ay - w * vx)
    nax = u[0] - mu * vx - FyF / m * np.sin(u[1])
    nay = 1.0 / m * (FyF * np.cos(u[1]) + FyR)
    nyaw = yaw + dt * w
    nw = w + dt * (1.0 / Iz * (lf * FyF * np.cos(u[1]) - lr * FyR))
    return np.array([nx_, ny_, abs(nvx), nvy, nax, nay, nyaw, nw])


def simulate(plant0, cmd, row, forces, La=0, Ld=0, lld=False, dt=0.005):
    """tests/_plant_params_ref.simulate with the force hook.  Returns (states [K,8], applied [K,2], slip [K,2] = the slip angles
    each step saw)."""
    act = AR.Actuator(La, Ld, lld, dt)
    st = np.array(plant0, float)
    states, applied, slip = [], [], []
    for m, s in np.asarray(cmd, float):
        u = act.step(float(m), float(s))
        slip.append(slip_angles(st, u, row))
        st = simulator_f_forces(st, u, row, forces, dt)
        states.append(st); applied.append(u)
    return np.array(states), np.array(applied), np.array(slip)


class TyreRaceRef(VehicleRaceRef):
    """VehicleRaceRef with tyre_params [B, 4] (None: kind 0 for every vehicle)."""

    def __init__(self, track, plant0, tyre_params=None, **kw):
        VehicleRaceRef.__init__(self, track, plant0, **kw)
        rows = np.zeros((self.B, 4)) if tyre_params is None else np.array(tyre_params, float)
        assert rows.shape == (self.B, 4), rows.shape
        self.tyres = rows
        self.hooks = [pacejka_forces(r) for r in rows]

    def _advance(self, b, st, n):
        servo, motor = self.cmd[b]
        row = self.rows[b]
        for _ in range(n):
            st = simulator_f_forces(st, self.act[b].step(motor, servo), row, self.hooks[b], self.dt_sim)
            if self.veh is not None:
                self.veh[b].substep(st, servo, motor)              # the estimator reads `ecu`: the commanded input
        return st
