"""CPU: the sensor faults' restatement (tests/_sensor_faults_ref.py) against the healthy restatement and the header's text, the row
helpers (lpvmpc.sensor_faults), the header and the library's exports."""
import math
import os
import re

import numpy as np
import pytest

from tests import _observer_ref as R
from tests import _sensor_faults_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("lpvmpc_sensor_fault_default_config", "lpvmpc_set_sensor_faults", "lpvmpc_sensor_faults_read", "lpvmpc_sensor_step_batch")
STDS = (0.01, 0.05, 0.01, 0.01, 0.02)


def gains():
    from tests._race_observer_ref import estimator_gains
    return estimator_gains()


def drive(k):
    """A plant state that moves: something for every sensor to read on step k."""
    t = 0.005 * k
    return np.array([0.5 + 1.1 * t, -0.2 + 0.05 * math.sin(t), 1.1 + 0.1 * math.sin(3 * t), 0.02 * math.cos(2 * t), 0.0, 0.0,
                     0.1 + 0.3 * t, 0.3 * math.cos(t)])


def pair(row, seed=11, vid=3, stds=STDS, **kw):
    g, p0 = gains(), drive(0)
    a = R.Vehicle(g, p0, stds=stds, seed=seed, vid=vid, **kw)
    b = F.FaultedVehicle(g, p0, stds=stds, seed=seed, vid=vid, row=row, fault_seed=seed, fault_vid=vid, **kw)
    return a, b


def test_off_rows_are_the_healthy_stage_bit_for_bit():
    a, b = pair(F.ALL_OFF)
    for k in range(1, 101):
        st = drive(k)
        ya, yb = a.substep(st, 0.1, 0.4), b.substep(st, 0.1, 0.4)
        assert ya.tobytes() == yb.tobytes() and a.est.tobytes() == b.est.tobytes(), k
        assert (a.gps, a.gps_cnt, a.enc_prev, a.enc_meas, a.enc_cnt, a.k) == (b.gps, b.gps_cnt, b.enc_prev, b.enc_meas, b.enc_cnt, b.k), k
    assert b.margin == math.inf and all(not lost for _, lost in b.lost) and len(b.lost) == 50
    assert b.state().shape == (F.STATE_WORDS,)


def test_stuck_encoder_reads_zero_on_the_41st_stuck_step_and_recovers():
    row = list(F.ALL_OFF); row[10:12] = (7.0, 45.0)                         # stuck on steps 7 .. 51
    a, b = pair(row)
    for k in range(1, 60):
        st = drive(k)
        a.substep(st, 0.1, 0.4); b.substep(st, 0.1, 0.4)
        if k < 7:
            assert b.enc_meas == a.enc_meas and b.enc_cnt == 0
        elif k <= 51:
            n_stuck = k - 6
            assert b.enc_cnt == n_stuck and b.enc_prev == held, k
            assert b.enc_meas == (0.0 if n_stuck >= 41 else held), k           # exactly the 41st: step 47
            assert b.y[0] == b.enc_meas
        else:
            assert b.enc_meas == a.enc_meas and b.enc_cnt == 0 and b.y[0] == a.y[0], k   # the first step after the window reads again
        if k == 6:
            held = b.enc_prev
    assert held != 0.0


def test_gps_outage_from_a_publishing_and_from_a_silent_step():
    """thUpdate = 0.2: the counter publishes on every even step.  An outage (10, 9) begins on a publishing step and covers the
    publications 10 .. 18; an outage (11, 9) begins on a silent step and covers 12 .. 18: the hold keeps the last reading before it."""
    for k0, first_lost, held_from in ((10, 10, 8), (11, 12, 10)):
        row = list(F.ALL_OFF); row[0:2] = (float(k0), 9.0)
        a, b = pair(row)
        holds = {}
        for k in range(1, 26):
            st = drive(k)
            a.substep(st, 0.0, 0.3); b.substep(st, 0.0, 0.3)
            holds[k] = list(a.gps)
            assert b.gps_cnt == a.gps_cnt, k                                    # the beacon keeps its rhythm
            if k < first_lost or k >= 20:
                assert b.gps == a.gps, (k0, k)
            else:
                assert b.gps == holds[held_from] and b.gps != a.gps, (k0, k)
            assert b.y[2:4].tolist() == b.gps
        assert [k for k, lost in b.lost if lost] == list(range(first_lost, 19, 2))


def test_jump_bias_drift_and_scale():
    row = list(F.ALL_OFF)
    row[3:7] = (4.0, 4.0, 0.5, -0.25); row[7] = 0.07; row[8] = 0.3; row[9] = 0.9
    a, b = pair(row, stds=(0, 0, 0, 0, 0))
    for k in range(1, 13):
        st = drive(k)
        a.substep(st, 0.0, 0.3); b.substep(st, 0.0, 0.3)
        assert b.y[1] == st[7] + 0.0 + 0.07
        if k * 0.005 > 0.02:
            assert b.y[4] == st[6] + 0.0 + 0.3 * (k * 0.005)
            assert b.y[0] == 0.9 * (math.sqrt(st[2] ** 2 + st[3] ** 2) + 0.0)
        else:
            assert b.y[4] == st[6]                                          # the start-up branch is untouched
        if k in (4, 6):                                                     # publications inside the jump window 4 .. 7
            assert b.gps == [st[0] + 0.5, st[1] - 0.25]
        elif k in (2, 8, 10, 12):
            assert b.gps == [st[0], st[1]]


def test_random_loss_draws_its_own_stream_only_on_publishing_steps():
    z = 0.5
    row = list(F.ALL_OFF); row[2] = z
    a, b = pair(row, seed=21, vid=9)
    for k in range(1, 201):
        st = drive(k)
        a.substep(st, 0.0, 0.3); b.substep(st, 0.0, 0.3)
    assert [k for k, _ in b.lost] == list(range(2, 201, 2))
    want = [F.loss_gauss(21, 9, k) > z for k in range(2, 201, 2)]
    assert [lost for _, lost in b.lost] == want and 0 < sum(want) < 100
    assert F.loss_gauss(21, 9, 2) != R.gauss(21, 9, 2, 5)                  # the stream constant keeps it apart from the sensors' key
    assert len(b.draws) == len(a.draws)                                     # and it takes no draw from the sensors' channels


def test_fault_rows_convert_seconds_and_probabilities():
    from statistics import NormalDist
    import lpvmpc
    from lpvmpc import sensor_faults as S
    assert S.FAULT_WORD_NAMES == F.WORDS and S.ALL_OFF == F.ALL_OFF
    r = lpvmpc.fault_rows(3, 0.005)
    assert np.array_equal(r, F.off(3))
    r = lpvmpc.fault_rows(2, 0.005, gps_outage=(1.0, [1.0, 0.5]), gps_loss_p=[0.0, 0.3], gps_jump=(0.1, 0.05, 0.4, -0.2), imu_w_bias=0.05,
                          imu_yaw_drift=[0.0, 0.01], enc_scale=0.9, enc_outage=(0.035, 0.225))
    assert r[:, 0].tolist() == [200.0, 200.0] and r[:, 1].tolist() == [200.0, 100.0]
    assert r[0, 2] >= 9.0 and r[1, 2] == NormalDist().inv_cdf(0.7) and abs(r[1, 2] - 0.5244005127080407) < 1e-12
    assert r[:, 3:7].tolist() == [[20.0, 10.0, 0.4, -0.2]] * 2
    assert r[:, 7].tolist() == [0.05, 0.05] and r[:, 8].tolist() == [0.0, 0.01] and r[:, 9].tolist() == [0.9, 0.9]
    assert r[:, 10:12].tolist() == [[7.0, 45.0]] * 2
    assert S.loss_z(0.0) >= 9.0 and S.loss_z(0.5) == 0.0
    for bad in (dict(enc_scale=0.0), dict(enc_scale=-1.0), dict(imu_w_bias=np.nan), dict(gps_outage=(-1.0, 1.0)), dict(gps_loss_p=1.0),
                dict(gps_loss_p=-0.1), dict(enc_outage=(0.0, 2.0 ** 31 * 0.005))):
        with pytest.raises(ValueError):
            lpvmpc.fault_rows(2, 0.005, **bad)
    with pytest.raises(ValueError):
        S.check_fault_rows(np.zeros((2, 11)), 2)
    bad = F.off(2); bad[1, 4] = 2.5
    with pytest.raises(ValueError):
        S.check_fault_rows(bad, 2)
    a = lpvmpc.sample_faults(8, 4)
    lo, hi = lpvmpc.sample_faults(4, 4), lpvmpc.sample_faults(4, 4, offset=4)
    assert np.array_equal(a, np.concatenate([lo, hi])) and len({tuple(x) for x in a}) == 8
    assert np.all((a[:, 0] >= 200) & (a[:, 0] <= 600) & (a[:, 1] >= 40) & (a[:, 1] <= 200) & (np.abs(a[:, 7]) <= 0.05))
    assert np.array_equal(S.parse_sensor_faults("gps_outage:1.0+imu_bias:0.05", 2), lpvmpc.fault_rows(2, 0.005, gps_outage=(1.0, 1.0), imu_w_bias=0.05))
    assert np.array_equal(S.parse_sensor_faults("enc_outage:0.5+gps_loss:0.3", 1), lpvmpc.fault_rows(1, 0.005, enc_outage=(1.0, 0.5), gps_loss_p=0.3))
    with pytest.raises(ValueError):
        S.parse_sensor_faults("gps:1", 1)


def test_header_declares_and_library_exports_the_calls():
    import ctypes
    from lpvmpc import _ffi
    hdr = open(os.path.join(ROOT, "include", "lpvmpc.h")).read()
    for name in CALLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _ffi.EXPORTS
    assert re.search(r"#define\s+LPVMPC_FAULT_WORDS\s+12\b", hdr) and re.search(r"#define\s+LPVMPC_OBS_STATE_WORDS\s+18\b", hdr)
    m = re.search(r"#define\s+LPVMPC_FAULT_STREAM\s+(0x[0-9A-Fa-f]+)ull", hdr)
    assert m and int(m.group(1), 16) == F.FAULT_STREAM == _ffi.FAULT_STREAM != _ffi.DIST_STREAM
    assert re.search(r"typedef struct lpvmpc_sensor_fault_config \{\s*uint64_t seed;[^}]*int64_t\s+vehicle_offset;", hdr)
    words = re.search(r"rows \[B\]\[LPVMPC_FAULT_WORDS\] = \{([^}]*)\}", hdr).group(1)
    assert tuple(w.strip() for w in words.replace("*", " ").replace("\n", " ").split(",")) == F.WORDS
    assert (_ffi.FAULT_WORDS, _ffi.OBS_STATE_WORDS) == (12, 18) == (len(F.WORDS), F.STATE_WORDS)
    so = ctypes.CDLL(_ffi.LIB_PATH)
    for name in CALLS:
        assert hasattr(so, name), name
    c = _ffi.default_sensor_fault_config()
    assert (c.seed, c.vehicle_offset) == (0, 0)
