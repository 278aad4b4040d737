"""Host replay of the race engine with the state estimator in the loop (lpvmpc_race_init_observed): tests/_race_ref.RaceRef
composed with the restated sensors + observer of tests/_observer_ref.Vehicle.

Schedule (include/lpvmpc.h, race block): one Vehicle per vehicle for the whole race, started as the lap-0 fleet's (estimate
[init_vx, 0, 0, x0, y0, yaw0]) and carried on through the lap event; every plant step is followed by the vehicle's sensors and
one observer step; every measurement -- the lap-0 branch, the racing branch with both event rules, the planner's first state --
reads the estimate in the plant's layout [x y vx vy 0 0 yaw psiDot]; a vehicle entering a tick with a non-finite plant or estimate
is lost; finished and lost vehicles advance neither plant nor observer.  After its event a vehicle's racing ticks are those of
a B = 1 oracle.cascade_ref.CascadeRef whose `plant` is the estimate view, as ObservedCascadeRef in tests/test_gpu_observer.py.

measure_plant=True replaces the estimate by the plant in every measurement (the observer still runs): the replay is then
RaceRef's schedule, which tests/test_race_observer_host.py pins."""
from __future__ import annotations

import numpy as np

from oracle import cascade_ref as CR, osqp_ref, plant_ref as PR
from tests import _observer_ref as OR
from tests._race_ref import RaceRef


class ObservedRaceRef(RaceRef):
    def __init__(self, gains, track, plant0, init_vx=0.2, stds=(0, 0, 0, 0, 0), n_bound=0.5, seed=0, vehicle_offset=0,
                 gps_freq=1000.0, loop_rate=200.0, dt_sim=0.005, measure_plant=False, **kw):
        super().__init__(track, plant0, **kw)
        self.measure_plant = measure_plant
        self.veh = [OR.Vehicle(gains, self.plant[b], init_vx=init_vx, dt=1.0 / loop_rate, dt_sim=dt_sim, gps_freq=gps_freq,
                               stds=stds, n_bound=n_bound, seed=seed, vid=vehicle_offset + b) for b in range(self.B)]

    def view(self, b):
        """What vehicle b's measurements read: the estimate in the plant's layout (or the plant with measure_plant)."""
        if self.measure_plant:
            return self.plant[b].copy()
        e = self.veh[b].est
        return np.array([e[3], e[4], e[0], e[1], 0.0, 0.0, e[5], e[2]])

    def _advance(self, b, st, n):
        servo, motor = self.cmd[b]
        for _ in range(n):
            st = PR.simulator_f(st, [motor, servo])
            self.veh[b].substep(st, servo, motor)
        return st

    def _racing_tick(self, b):
        """One racing tick of vehicle b (ObservedCascadeRef.tick at B = 1); False when the vehicle finishes on it."""
        r = self.casc[b]
        r.plant = self.view(b)[None]
        while r.plan_ticks < (2 * r.k) // 3 + 1:
            r.planner_tick()
        lap_before = r.glue[0].lap
        r.local[0], v, c = r.glue[0].measure(r.plant[0], r.refs[0])
        if r.glue[0].lap != lap_before and r.glue[0].lap > self.laps:
            return False                                        # frozen before anything of this tick is applied
        Nc = r.Nc
        vel = np.empty((1, Nc + 1)); vel[0, :Nc] = v; vel[0, Nc] = v[-1]
        w = dict(N=Nc, dt=r.dtc, Q=r.Qc, R=r.Rc, dR=r.dRc, track=r.track, x0=r.local.copy(), u_prev=r.uPred,
                 vel_ref=vel, curv_s=np.asarray(c, float)[None], u_old=r.cmd.copy(), cf_new=60.0, lap=1)
        r.ctrl = osqp_ref.ctrl_tick_batch(w, nthreads=r.nthreads)
        r.uPred = r.ctrl["uPred"]
        r.cmd = r.uPred[:, 0, :].copy()
        self.cmd[b] = r.cmd[0]
        self.plant[b] = self._advance(b, self.plant[b].copy(), r.n_sub[r.k % 3])
        r.k += 1
        return True

    def tick(self):
        seed = self.t < 9
        for b in range(self.B):
            if self.phase[b] >= 2:
                self.iters[b] = 0
                continue
            m = self.view(b)
            if not (np.all(np.isfinite(self.plant[b])) and np.all(np.isfinite(m))):
                self.phase[b] = 3; self.iters[b] = 0
                continue
            if self.phase[b] == 1:
                c = self.casc[b]
                if not self._racing_tick(b):
                    self.phase[b] = 2; self.lap[b] = c.glue[0].lap; self.iters[b] = 0
                    continue
                self.local[b] = c.local[0]; self.lap[b] = c.glue[0].lap
                self.iters[b] = c.ctrl["iters"][0]; self.status[b] = c.ctrl["status"][0]
                continue
            s, ey, epsi, _ = PR.get_local_position(self.track, self.hw, self.slack, m[0], m[1], m[6])
            Lc = np.array([m[2] if m[2] >= 0.01 else 0.01, m[3], m[7], ey, s, epsi])         # CMAIN:183-188 (quirk Q9)
            self.local[b] = Lc
            if s >= 3 * self.TL / 4:
                self.half[b] = 1
            event = self.half[b] == 1 and s <= self.TL / 4
            if event and not seed:
                u, it, stt = self._solve_tt_event(b, Lc)
            else:
                u, it, stt = self._solve_path(b, Lc, seed)
                self.uPred_path[b] = u
            self.iters[b], self.status[b] = it, stt
            self.cmd[b] = u[0]
            self.plant[b] = self._advance(b, self.plant[b].copy(), self.n_sub_lap0)
            if event:
                self.half[b] = 0; self.lap[b] = 1; self.phase[b] = 1; self.event_tick[b] = self.t
                self.casc[b] = CR.CascadeRef(self.track, self.tt_tuning, self.plan_weights, self.view(b)[None], self.cmd[b][None], u[None],
                                             lap0=1, half_width=self.hw, slack=self.slack, plan_max_ey=self.max_ey, n_sub=self.n_sub)
        self.t += 1

    def estimate(self):
        return np.array([v.est for v in self.veh])


def estimator_gains():
    """The reference's gain and limit tables (tests/golden/estimator/estimator.npz) as _observer_ref.observer_step takes them."""
    import os
    f = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "estimator", "estimator.npz"))
    return {k: f[k] for k in ("L_ls", "lim_ls", "L_hs", "lim_hs")}


def start_line_fleet(track, B, seed, s_lo=0.8, s_hi=0.97):
    """B vehicles on the last part of the lap (to be started with HalfTrack = 1), so that their lap events spread over many ticks."""
    rng = np.random.default_rng(seed)
    track = np.asarray(track, float)
    L = float(track[-1, 3] + track[-1, 4])
    plant0 = np.zeros((B, 8))
    for b in range(B):
        s = rng.uniform(s_lo, s_hi) * L
        x, y, th = PR.get_global_position(track, s, rng.normal(0, 0.02))
        plant0[b] = [x, y, rng.uniform(0.9, 1.1), 0.0, 0.0, 0.0, th + rng.normal(0, 0.02), 0.0]
    return plant0


def grid_fleet(B, seed):
    """B vehicles near the origin (HalfTrack = 0): lap 0 from the grid."""
    rng = np.random.default_rng(seed)
    plant0 = np.zeros((B, 8))
    plant0[:, 1] = rng.normal(0, 0.02, B); plant0[:, 2] = rng.uniform(0.9, 1.1, B); plant0[:, 6] = rng.normal(0, 0.02, B)
    return plant0
