"""Sensor faults of a lap-0 fleet or a race with the estimator in the loop (include/lpvmpc.h, "Sensor faults"): per vehicle a GPS
outage window, a random GPS loss, a GPS jump window, a rate-gyro bias, a yaw drift, an encoder scale (a slipping wheel) and a stuck
encoder window.  Rows are [B, 12] = FAULT_WORD_NAMES per vehicle; windows count the vehicle's own observer steps k (the first step
is k = 1), the helpers take seconds (BatchedSolver.set_sensor_faults, RaceFleet(sensor_faults=...))."""
import math
from statistics import NormalDist

import numpy as np

from . import _ffi

FAULT_WORD_NAMES = ("gps_out_k0", "gps_out_len", "gps_loss_z", "gps_jump_k0", "gps_jump_len", "gps_jump_dx", "gps_jump_dy",
                    "imu_w_bias", "imu_yaw_drift", "enc_scale", "enc_out_k0", "enc_out_len")
OBS_STATE_NAMES = ("est_vx", "est_vy", "est_psiDot", "est_x", "est_y", "est_yaw", "y_vx", "y_psiDot", "y_x", "y_y", "y_yaw",
                   "gps_x", "gps_y", "enc_prev", "enc_meas", "gps_cnt", "enc_cnt", "k")
Z_OFF = 9.0                  # a loss threshold the generator cannot exceed (sqrt(-2 ln 2^-53) = 8.57): no draw
ALL_OFF = (0.0, 0.0, Z_OFF, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0)
_WINDOW_WORDS = (0, 1, 3, 4, 10, 11)


def loss_z(p):
    """The threshold z of a loss probability ``p`` per publication: P(gauss > z) = p, the standard normal's inverse CDF at 1 - p;
    p = 0 gives Z_OFF (nothing is drawn)."""
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError("loss probability %r is outside [0, 1)" % (p,))
    return Z_OFF if p == 0.0 else min(Z_OFF, NormalDist().inv_cdf(1.0 - p))


def steps(t_s, dt):
    """Seconds -> observer steps of ``dt`` seconds, rounded to the nearest step."""
    return float(math.floor(float(t_s) / float(dt) + 0.5))


def check_fault_rows(rows, B):
    """Validated float64 [B, 12] copy of ``rows`` with the library's refusals: every word finite, k0 and len integer-valued, >= 0
    and < 2^31, enc_scale > 0."""
    a = np.asarray(rows)
    if a.dtype.kind not in "fiu":
        raise ValueError("sensor fault rows must be numeric, got dtype %s" % a.dtype)
    a = np.array(a, dtype=np.float64)
    if a.shape != (B, _ffi.FAULT_WORDS):
        raise ValueError("sensor fault rows have shape %s, expected (%d, %d) = (B, [%s])" % (a.shape, B, _ffi.FAULT_WORDS, " ".join(FAULT_WORD_NAMES)))
    for b in range(B):
        for i, v in enumerate(a[b]):
            ok = math.isfinite(v)
            if ok and i in _WINDOW_WORDS:
                ok = v >= 0 and v == math.floor(v) and v < 2.0 ** 31
            elif ok and i == 9:
                ok = v > 0
            if not ok:
                raise ValueError("sensor fault rows: vehicle %d: %s = %g (every word finite; k0 and len integer-valued, >= 0 and < 2^31; "
                                 "enc_scale > 0)" % (b, FAULT_WORD_NAMES[i], v))
    return np.ascontiguousarray(a)


def _col(v, B):
    return np.broadcast_to(np.asarray(v, float), (B,))


def fault_rows(B, dt, gps_outage=None, gps_loss_p=None, gps_jump=None, imu_w_bias=None, imu_yaw_drift=None, enc_scale=None,
               enc_outage=None):
    """[B, 12] rows, all off unless given; every argument is a scalar (tuple of scalars) or [B] arrays.  ``dt`` is the observer step
    in seconds (1 / loop_rate); seconds are converted to observer steps, step k covering the time k * dt.
    ``gps_outage`` = (t0_s, len_s); ``gps_loss_p`` the probability that a publication is lost; ``gps_jump`` = (t0_s, len_s, dx, dy);
    ``imu_w_bias`` rad/s; ``imu_yaw_drift`` rad/s; ``enc_scale`` > 0; ``enc_outage`` = (t0_s, len_s)."""
    out = np.tile(np.array(ALL_OFF), (B, 1))
    to_steps = np.vectorize(lambda t: steps(t, dt), otypes=[float])
    if gps_outage is not None:
        out[:, 0] = to_steps(_col(gps_outage[0], B)); out[:, 1] = to_steps(_col(gps_outage[1], B))
    if gps_loss_p is not None:
        out[:, 2] = [loss_z(p) for p in _col(gps_loss_p, B)]
    if gps_jump is not None:
        out[:, 3] = to_steps(_col(gps_jump[0], B)); out[:, 4] = to_steps(_col(gps_jump[1], B))
        out[:, 5] = _col(gps_jump[2], B); out[:, 6] = _col(gps_jump[3], B)
    if imu_w_bias is not None:
        out[:, 7] = _col(imu_w_bias, B)
    if imu_yaw_drift is not None:
        out[:, 8] = _col(imu_yaw_drift, B)
    if enc_scale is not None:
        out[:, 9] = _col(enc_scale, B)
    if enc_outage is not None:
        out[:, 10] = to_steps(_col(enc_outage[0], B)); out[:, 11] = to_steps(_col(enc_outage[1], B))
    return check_fault_rows(out, B)


def sample_faults(B, seed, dt=0.005, spread=None, offset=0):
    """Monte-Carlo rows: each quantity of ``spread`` is uniform in its (lo, hi) per vehicle, drawn from a generator keyed
    (seed, offset + b), so that shard k of a sharded fleet takes sample_faults(n, seed, offset=k * n).  Keys: gps_outage_t0,
    gps_outage_len, enc_outage_t0, enc_outage_len (seconds), gps_loss_p, imu_w_bias, imu_yaw_drift, enc_scale.  Default: a GPS outage
    of 0.2 .. 1.0 s starting within 1 .. 3 s and a gyro bias of +-0.05 rad/s."""
    keys = ("gps_outage_t0", "gps_outage_len", "gps_loss_p", "imu_w_bias", "imu_yaw_drift", "enc_scale", "enc_outage_t0", "enc_outage_len")
    spread = dict(gps_outage_t0=(1.0, 3.0), gps_outage_len=(0.2, 1.0), imu_w_bias=(-0.05, 0.05)) if spread is None else dict(spread)
    unknown = set(spread) - set(keys)
    if unknown:
        raise TypeError("unknown sample_faults key(s) %s (keys: %s)" % (sorted(unknown), ", ".join(keys)))
    draw = {k: np.zeros(B) for k in keys}
    draw["enc_scale"] = np.ones(B)
    for b in range(B):
        u = np.random.default_rng([int(seed), int(offset) + b]).random(len(keys))
        for k, (lo, hi) in spread.items():
            draw[k][b] = lo + (hi - lo) * u[keys.index(k)]
    return fault_rows(B, dt, gps_outage=(draw["gps_outage_t0"], draw["gps_outage_len"]), gps_loss_p=draw["gps_loss_p"],
                      imu_w_bias=draw["imu_w_bias"], imu_yaw_drift=draw["imu_yaw_drift"], enc_scale=draw["enc_scale"],
                      enc_outage=(draw["enc_outage_t0"], draw["enc_outage_len"]))


def sensor_fault_config(seed=0, vehicle_offset=0):
    """A ``lpvmpc_sensor_fault_config`` (the library's defaults with the given fields)."""
    c = _ffi.default_sensor_fault_config()
    c.seed = int(seed) & ((1 << 64) - 1); c.vehicle_offset = int(vehicle_offset)
    return c


def parse_sensor_faults(spec, B, dt=0.005, t0=1.0):
    """Rows for the command-line tools' ``--sensor-faults`` flag, the same for every vehicle: ``gps_outage:LEN_S`` and
    ``enc_outage:LEN_S`` (windows that start ``t0`` seconds into the run), ``gps_loss:P``, ``imu_bias:RAD_PER_S``, ``imu_drift:RAD_PER_S``,
    ``enc_scale:S``; several may be joined with ``+``."""
    kw = {}
    for part in str(spec).split("+"):
        kind, _, arg = part.partition(":")
        try:
            v = float(arg)
        except ValueError:
            v = None
        if v is None or kind not in ("gps_outage", "enc_outage", "gps_loss", "imu_bias", "imu_drift", "enc_scale"):
            raise ValueError("--sensor-faults takes gps_outage:LEN_S, enc_outage:LEN_S, gps_loss:P, imu_bias:W, imu_drift:W or enc_scale:S "
                             "(joined with +), got %r" % (part,))
        if kind in ("gps_outage", "enc_outage"):
            kw[kind] = (t0, v)
        else:
            kw[{"gps_loss": "gps_loss_p", "imu_bias": "imu_w_bias", "imu_drift": "imu_yaw_drift", "enc_scale": "enc_scale"}[kind]] = v
    return fault_rows(B, dt, **kw)
