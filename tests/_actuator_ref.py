"""Numpy restatement of the reference simulator's actuator model (vehicleSimulator.py:53-78) over oracle.plant_ref.simulator_f, and
of a controller's OldSteering / OldAccelera history (controllerMain.py:289-298).  Pinned by tests/golden/actuator/actuator.npz,
which the reference's own main loop generated.  The ring form (act_words) is the host layout of the device's actuator state
(include/lpvmpc.h, "Actuator delay and servo lag")."""
from __future__ import annotations

import numpy as np

from oracle import plant_ref as PR

ACT_MAX_DELAY = 64
ACT_WORDS = 2 * ACT_MAX_DELAY + 2


class Actuator:
    """One vehicle's FIFOs and servo filter, as main() keeps them: a_his / df_his start as La / Ld zeros; every step appends the
    command and pops the oldest entry; with lowLevelDyn the filter runs on the popped steering."""

    def __init__(self, La, Ld, lld=False, dt=0.005, tf=0.07):
        self.a_his, self.df_his = [0.0] * int(La), [0.0] * int(Ld)
        self.lld, self.T, self.Tf = bool(lld), dt, tf
        self.servo_inp = 0.0
        self.k = 0
        self.log = []                     # every command received, for the ring form

    def step(self, motor, servo):
        self.a_his.append(motor); self.df_his.append(servo)
        self.log.append((motor, servo))
        self.k += 1
        if self.lld:
            T, Tf = self.T, self.Tf
            self.servo_inp = (1 - T / Tf) * self.servo_inp + (T / Tf) * self.df_his.pop(0)
            return [self.a_his.pop(0), self.servo_inp]
        return [self.a_his.pop(0), self.df_his.pop(0)]

    def words(self):
        return act_words(self.log, self.servo_inp)


def act_words(log, servo_inp):
    """Host layout of one vehicle's actuator state after the commands `log` (one per plant step): ring slot k % 64 holds the
    command of step k (zeros where no step wrote it), then servo_inp and the step count."""
    w = np.zeros(ACT_WORDS)
    for k, (m, s) in enumerate(log):
        w[k % ACT_MAX_DELAY] = m
        w[ACT_MAX_DELAY + k % ACT_MAX_DELAY] = s
    w[2 * ACT_MAX_DELAY] = servo_inp
    w[2 * ACT_MAX_DELAY + 1] = len(log)
    return w


def simulate(plant0, cmd, La, Ld, lld, dt=0.005, mu=0.05):
    """Per step k: u = actuator(cmd[k] = (motor, servo)), state = Simulator.f(state, u).  Returns (states [K,8], applied [K,2])."""
    p = dict(PR.SIM_PARAMS, dt=dt, mu=mu)
    act = Actuator(La, Ld, lld, dt)
    st = np.array(plant0, float)
    states, applied = [], []
    for m, s in np.asarray(cmd, float):
        u = act.step(float(m), float(s))
        st = PR.simulator_f(st, u, p)
        states.append(st); applied.append(u)
    return np.array(states), np.array(applied)


def uold_push(hist, servo, motor):
    """CMAIN:289-298 on the device layout u_old [2 + d] = [OldSteering[0], OldAccelera[0], OldSteering[1..d]]: OldSteering appends
    servo and drops its oldest entry, OldAccelera becomes [motor].  Returns the new row."""
    h = np.asarray(hist, float)
    d = h.size - 2
    steer = [h[0]] + list(h[2:])
    steer = steer[1:] + [servo]
    return np.array([steer[0], motor] + steer[1:1 + d])
