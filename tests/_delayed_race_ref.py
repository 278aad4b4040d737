"""Host replay of the delayed fleets (lpvmpc_cl_init_actuated, lpvmpc_race_init_actuated): tests/_race_ref.RaceRef and
tests/_race_observer_ref.ObservedRaceRef with

  * the actuator in the plant: per vehicle a tests/_actuator_ref.Actuator (the reference's FIFOs and servo filter) between the
    command and oracle.plant_ref.simulator_f; the observer, where it runs, is fed the commanded (servo, motor);
  * a steering delay d on both controllers: each keeps its u_old history [OldSteering[0], OldAccelera[0], OldSteering[1..d]]
    (zeros at the start); on each tick the controller of the vehicle's lap appends the last command and drops its oldest entry
    (CMAIN:289-298, after the lap logic: on the event tick that is `tt`), and its solve reads the history -- lap 0 and the event
    tick through oracle/lpv_ref.py's QP with the d pinned rows, racing ticks through osqp_ref.ctrl_tick_batch_delay.  Both use
    the stage-wise elimination order of osqp_ref.ctrl_delay_ordering.

With d = 0 the histories are the last command and every solve is the parent class's call, so with the actuator all off the
replay is RaceRef (gains None: ground truth) or ObservedRaceRef word for word; tests/test_delayed_replay_host.py pins that.
A fleet started with half_track0 = 0 and no lap event in the window is the delayed lap-0 fleet (lpvmpc_cl_init_actuated): the
race equals it word for word before any event (tests/test_gpu_delayed_fleets.py).  Not replayed: a lap event inside the 9
seed ticks (as RaceRef)."""
from __future__ import annotations

import numpy as np

from oracle import cascade_ref as CR, lpv_ref as L, osqp_ref, plant_ref as PR
from tests import _actuator_ref as AR
from tests._race_observer_ref import ObservedRaceRef
from tests._race_ref import RaceRef


class DelayedRaceRef(ObservedRaceRef):
    """gains None: the race on ground truth (RaceRef's measurements); else ObservedRaceRef's estimator (its keyword arguments)."""

    OBS_KEYS = ("init_vx", "stds", "n_bound", "seed", "vehicle_offset", "gps_freq", "loop_rate", "measure_plant")

    def __init__(self, track, plant0, steering_delay=0, delay_a=0, delay_df=0, low_level_dyn=False, gains=None, dt_sim=0.005, **kw):
        obs = {k: kw.pop(k) for k in self.OBS_KEYS if k in kw}
        if gains is None:
            RaceRef.__init__(self, track, plant0, **kw)
            self.veh, self.measure_plant = None, True
        else:
            ObservedRaceRef.__init__(self, gains, track, plant0, dt_sim=dt_sim, **obs, **kw)
        B, d = self.B, int(steering_delay)
        La = np.broadcast_to(np.asarray(delay_a, int), (B,)); Ld = np.broadcast_to(np.asarray(delay_df, int), (B,))
        self.act = [AR.Actuator(La[b], Ld[b], low_level_dyn, dt_sim) for b in range(B)]
        self.d = d
        self.p_hist = np.zeros((B, 2 + d))                      # path controller's history (device: the path handle's u_old)
        self.t_hist = np.zeros((B, 2 + d))                      # tt's
        self.perm = osqp_ref.ctrl_delay_ordering(self.N, d) if d else None

    # -- plant, measurement ------------------------------------------------------------------------------------------------
    def view(self, b):
        if self.veh is None:
            return self.plant[b].copy()
        return ObservedRaceRef.view(self, b)

    def _advance(self, b, st, n):
        servo, motor = self.cmd[b]
        for _ in range(n):
            st = PR.simulator_f(st, self.act[b].step(motor, servo))
            if self.veh is not None:
                self.veh[b].substep(st, servo, motor)              # the estimator reads `ecu`: the commanded input
        return st

    # -- solves --------------------------------------------------------------------------------------------------------------
    def _qp(self, tuning, A, Bm, x0, hist, b):
        p, N = L.DEFAULT_PARAMS, self.N
        Q, R, dR = tuning
        if self.d == 0:                                          # RaceRef's call
            qp = L.ctrl_build_qp(Q, R, dR, N, A, Bm, x0, self.cmd[b], np.ones(N + 1), p["max_vel"])
            r = osqp_ref.solve_qp(qp.P, qp.q, qp.A, qp.l, qp.u)
        else:
            qp = L.ctrl_build_qp(Q, R, dR, N, A, Bm, x0, hist[:2], np.ones(N + 1), p["max_vel"], steer_hist=hist[2:])
            r = osqp_ref.solve_qp(qp.P, qp.q, qp.A, qp.l, qp.u, perm=self.perm)
        _x, u, _ = L.unpack_solution(r.x, 6, 2, N)
        return u, r.info.iter, r.info.status_val

    def _solve_path_d(self, b, x_meas, seed):
        p, N = L.DEFAULT_PARAMS, self.N
        if seed:
            xx, uu = L.ctrl_seed_vectors(x_meas)
            A, Bm = L.ctrl_estimate_abc(p, self.dt, N, self.track, xx[:N], uu[:N])
            x0 = x_meas
        else:
            S, A, Bm = L.ctrl_lpv_prediction(p, self.dt, N, self.track, x_meas, self.uPred_path[b], np.ones(N + 1), np.zeros(N), 60.0, 0)
            x0 = S[0]
        return self._qp(self.path_tuning, A, Bm, x0, self.p_hist[b], b)

    def _solve_tt_event_d(self, b, x_meas):
        p, N = L.DEFAULT_PARAMS, self.N
        S, A, Bm = L.ctrl_lpv_prediction(p, self.dt, N, self.track, x_meas, self.uPred_path[b], np.ones(N + 1), np.zeros(N), 60.0, 1)
        return self._qp(self.tt_tuning, A, Bm, x_meas, self.t_hist[b], b)

    def _racing_tick(self, b):
        """ObservedRaceRef._racing_tick with tt's history step and its delayed solve."""
        r = self.casc[b]
        r.plant = self.view(b)[None]
        while r.plan_ticks < (2 * r.k) // 3 + 1:
            r.planner_tick()
        lap_before = r.glue[0].lap
        r.local[0], v, c = r.glue[0].measure(r.plant[0], r.refs[0])
        if r.glue[0].lap != lap_before and r.glue[0].lap > self.laps:
            return False                                        # frozen before anything of this tick is applied
        self.t_hist[b] = AR.uold_push(self.t_hist[b], self.cmd[b, 0], self.cmd[b, 1])
        Nc = r.Nc
        vel = np.empty((1, Nc + 1)); vel[0, :Nc] = v; vel[0, Nc] = v[-1]
        w = dict(N=Nc, dt=r.dtc, Q=r.Qc, R=r.Rc, dR=r.dRc, track=r.track, x0=r.local.copy(), u_prev=r.uPred,
                 vel_ref=vel, curv_s=np.asarray(c, float)[None], cf_new=60.0, lap=1)
        if self.d == 0:
            r.ctrl = osqp_ref.ctrl_tick_batch(dict(w, u_old=r.cmd.copy()), nthreads=r.nthreads)
        else:
            r.ctrl = osqp_ref.ctrl_tick_batch_delay(dict(w, u_old=self.t_hist[b][None].copy()), nthreads=r.nthreads)
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
            # CMAIN:289-298 after the lap logic: the event makes the vehicle's lap 1, so `tt` takes the command on that tick
            if event:
                self.t_hist[b] = AR.uold_push(self.t_hist[b], self.cmd[b, 0], self.cmd[b, 1])
            else:
                self.p_hist[b] = AR.uold_push(self.p_hist[b], self.cmd[b, 0], self.cmd[b, 1])
            if event and not seed:
                u, it, stt = self._solve_tt_event_d(b, Lc)
            else:
                u, it, stt = self._solve_path_d(b, Lc, seed)
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
        return None if self.veh is None else ObservedRaceRef.estimate(self)


def delayed_lap0_replay(track, plant0, **kw):
    """The delayed lap-0 fleet (lpvmpc_cl_init_actuated, path tuning, vel_ref = 1): the race replay from HalfTrack = 0, valid while
    no vehicle reaches its lap event."""
    return DelayedRaceRef(track, plant0, half_track0=0, **kw)
