"""Numpy restatement (test infrastructure) of the faulted sensor stage as include/lpvmpc.h documents it ("Sensor faults"), on top of
tests/_observer_ref.py: the healthy stage's words with a vehicle's fault row applied, then the shared observer step."""
import math

import numpy as np

from tests import _observer_ref as R
from tests import _tyre_ref as T

WORDS = ("gps_out_k0", "gps_out_len", "gps_loss_z", "gps_jump_k0", "gps_jump_len", "gps_jump_dx", "gps_jump_dy",
         "imu_w_bias", "imu_yaw_drift", "enc_scale", "enc_out_k0", "enc_out_len")
ALL_OFF = (0.0, 0.0, 9.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0)
FAULT_STREAM = 0x5E4507FA17C0FFEE
LOSS_CHANNEL = 5
STATE_WORDS = 18               # est [6], y [5], gps x y, enc_prev, enc_meas, gps_cnt, enc_cnt, k


def off(B):
    return np.tile(ALL_OFF, (B, 1))


def window(k, k0, n):
    return k0 <= k < k0 + n


def loss_gauss(seed, vid, k):
    return R.gauss((seed ^ FAULT_STREAM) & R.MASK, vid, k, LOSS_CHANNEL)


class FaultedVehicle(R.Vehicle):
    """R.Vehicle whose substep applies ``row`` (None: the healthy stage of R.Vehicle).  fault_seed / fault_vid: the fault
    configuration's seed and the vehicle's global index under its vehicle_offset.  ``lost`` lists, per publishing step, (k, lost);
    ``margin`` is the smallest |g - z| over the loss draws made."""

    def __init__(self, *a, row=None, fault_seed=0, fault_vid=0, **kw):
        R.Vehicle.__init__(self, *a, **kw)
        self.row = None if row is None else [float(x) for x in row]
        self.fault_seed, self.fault_vid = fault_seed, fault_vid
        self.lost, self.margin = [], math.inf

    @classmethod
    def adopt(cls, v, row, fault_seed, fault_vid):
        """The faulted twin of a running R.Vehicle: its whole state, by reference to nothing."""
        f = cls.__new__(cls)
        f.__dict__.update(v.__dict__)
        f.est, f.gps, f.y, f.draws = v.est.copy(), list(v.gps), v.y.copy(), list(v.draws)
        f.row = None if row is None else [float(x) for x in row]
        f.fault_seed, f.fault_vid = fault_seed, fault_vid
        f.lost, f.margin = [], math.inf
        return f

    def substep(self, st, servo, motor):
        if self.row is None:
            return R.Vehicle.substep(self, st, servo, motor)
        (out_k0, out_len, z, jump_k0, jump_len, dx, dy, w_bias, yaw_drift, enc_scale, enc_k0, enc_len) = self.row
        self.k += 1
        k = self.k
        imu_yaw = st[6] + self.n(k, 0) + yaw_drift * (k * self.dt)
        imu_w = st[7] + self.n(k, 1) + w_bias
        gx = st[0] + self.n(k, 2); gy = st[1] + self.n(k, 3)
        if window(k, jump_k0, jump_len):
            gx = gx + dx; gy = gy + dy
        pub = self.gps_cnt > self.th
        self.gps_cnt = 0.0 if pub else self.gps_cnt + 1.0
        if pub:
            lost = window(k, out_k0, out_len)
            if not lost and z < 9.0:
                g = loss_gauss(self.fault_seed, self.fault_vid, k)
                self.margin = min(self.margin, abs(g - z))
                lost = g > z
            self.lost.append((k, lost))
            if not lost:
                self.gps = [gx, gy]
        v = enc_scale * (math.sqrt(st[2] * st[2] + st[3] * st[3]) + self.n(k, 4))
        if window(k, enc_k0, enc_len):
            v = self.enc_prev
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
        self.est = R.observer_step(self.g, self.est, self.y, [servo, motor], k, self.dt)[0]
        return self.y

    # the device layout of the estimator's per-vehicle state (LPVMPC_OBS_STATE_WORDS)
    def state(self):
        return np.array(list(self.est) + list(self.y) + [self.gps[0], self.gps[1], self.enc_prev, self.enc_meas, self.gps_cnt, self.enc_cnt,
                                                         float(self.k)])

    def load(self, s):
        self.est, self.y = np.array(s[0:6], float), np.array(s[6:11], float)
        self.gps = [float(s[11]), float(s[12])]
        self.enc_prev, self.enc_meas, self.gps_cnt, self.enc_cnt, self.k = float(s[13]), float(s[14]), float(s[15]), float(s[16]), int(s[17])


class FaultedRaceRef(T.TyreRaceRef):
    """TyreRaceRef (with its estimator: pass gains) with fault rows [B, 12] attached from tick attach_tick on, until detach_tick
    (None: never detached)."""

    def __init__(self, track, plant0, rows, fault_seed=0, fault_offset=0, attach_tick=0, detach_tick=None, **kw):
        T.TyreRaceRef.__init__(self, track, plant0, **kw)
        self.fault_rows = np.asarray(rows, float)
        self.veh = [FaultedVehicle.adopt(v, None, fault_seed, fault_offset + b) for b, v in enumerate(self.veh)]
        self.attach_tick, self.detach_tick = attach_tick, detach_tick

    def _advance(self, b, st, n):
        on = self.t >= self.attach_tick and (self.detach_tick is None or self.t < self.detach_tick)
        self.veh[b].row = [float(x) for x in self.fault_rows[b]] if on else None
        return T.TyreRaceRef._advance(self, b, st, n)
