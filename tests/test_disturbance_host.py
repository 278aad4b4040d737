"""CPU: the plant disturbances' restatement (tests/_disturbance_ref.py), the row helpers (lpvmpc.disturbance), the header, the
library's exports and the rule that the feature lives in files of its own."""
import os
import re

import numpy as np
import pytest

from tests import _disturbance_ref as D
from tests import _tyre_ref as T
from tests._plant_params_ref import nominal_row

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "autonomous-racing-lpv-mpp-mpc_amd", "csrc")
CALLS = ("lpvmpc_disturbance_default_config", "lpvmpc_set_disturbances", "lpvmpc_disturbances_read", "lpvmpc_plant_step_disturbed_batch")
UNTOUCHED = ("fleet_kernels.hpp", "track_geometry.hpp", "observer_device.hpp", "track_view.hpp")
PLANT0 = np.array([0.4, 0.05, 1.1, 0.02, 0.0, 0.0, 0.03, 0.2])


def lshape():
    import lpvmpc
    return lpvmpc.Map("L_shape", 0.2)


@pytest.mark.parametrize("tyre", [(0.0, 6.0, 1.6, 0.8), T.LAUNCH_FILE])
def test_all_off_rows_are_the_tyre_restatement(tyre):
    """Five ticks of 7 steps with all-off rows equal tests/_tyre_ref.simulate over the same 35 steps, word for word, and leave the
    state at (0, 0, 0, ticks, 1)."""
    mp = lshape()
    row = nominal_row()
    cmd = np.tile([0.8, 0.15], (35, 1))
    ref = T.simulate(PLANT0, cmd, row, T.pacejka_forces(tyre))[0]
    m = D.Model(D.ALL_OFF[None])
    st = PLANT0.copy()
    for t in range(5):
        st = D.step_tick(m, 0, st, 7 * t, cmd[0], row, tyre, 7, 0.005, mp.PointAndTangent, mp.halfWidth, mp.slack)
        assert st.tobytes() == ref[7 * t + 6].tobytes(), t
    assert m.state[0].tolist() == [0.0, 0.0, 0.0, 5.0, 1.0]


def test_patch_membership():
    """Before, inside, after, across the start line, two overlapping patches (the product), off the map."""
    L = 10.0
    row = D.ALL_OFF.copy(); row[7:10] = (2.0, 3.0, 0.5)
    assert D.patch_gamma(row, 1.999, 1, L) == 1.0 and D.patch_gamma(row, 2.0, 1, L) == 0.5
    assert D.patch_gamma(row, 4.999, 1, L) == 0.5 and D.patch_gamma(row, 5.0, 1, L) == 1.0
    wrap = D.ALL_OFF.copy(); wrap[7:10] = (9.0, 2.0, 0.25)                 # 9 .. 10 and 0 .. 1
    assert [D.patch_gamma(wrap, s, 1, L) for s in (8.9, 9.0, 9.9, 0.0, 0.99, 1.0)] == [1.0, 0.25, 0.25, 0.25, 0.25, 1.0]
    two = row.copy(); two[10:13] = (4.0, 2.0, 0.5)                         # 4 .. 6 overlaps 2 .. 5 on 4 .. 5
    assert [D.patch_gamma(two, s, 1, L) for s in (3.0, 4.5, 5.5, 6.0)] == [0.5, 0.25, 0.5, 1.0]
    assert D.patch_gamma(two, 4.5, 0, L) == 1.0                            # off the map: the sentinels reach no patch
    whole = D.ALL_OFF.copy(); whole[7:10] = (3.0, L, 0.7)                  # len == L: the whole lap
    assert all(D.patch_gamma(whole, s, 1, L) == 0.7 for s in (0.0, 2.99, 3.0, 9.99))
    assert D.patch_gamma(D.ALL_OFF, 0.0, 1, L) == 1.0                      # len 0 contains nothing


def test_kick_window():
    assert [D.kick_applies(14.0, k0, 7) for k0 in (0, 7, 8, 14, 15)] == [False, False, True, True, False]
    assert not D.kick_applies(14.0, 7, 7) and D.kick_applies(14.0, 14, 6)   # kick_step == k0 + n belongs to the next tick
    assert not D.kick_applies(-1.0, 0, 7) and D.kick_applies(0.0, 0, 1)
    mp = lshape()
    rows = D.ALL_OFF[None].copy(); rows[0, 4:7] = (10, 0.3, -0.2)
    m = D.Model(rows)
    st, k, hits = PLANT0.copy(), 0, []
    for n in (7, 7, 6):
        before = st.copy()
        st, _ = m.apply(0, st, k, n, 0.005, mp.PointAndTangent, mp.halfWidth, mp.slack)
        hits.append(not np.array_equal(st, before))
        if hits[-1]:
            assert st[3] == before[3] + 0.3 and st[7] == before[7] - 0.2 and np.array_equal(np.delete(st, [3, 7]), np.delete(before, [3, 7]))
        k += n
    assert hits == [False, True, False]


def test_frozen_vehicle_and_silent_channels():
    """n == 0 touches nothing; a channel with sigma 0 performs no add (a -0.0 keeps its sign)."""
    mp = lshape()
    rows = D.ALL_OFF[None].copy(); rows[0, 1] = 0.5
    m = D.Model(rows, seed=3)
    st0 = PLANT0.copy(); st0[7] = -0.0
    st, _ = m.apply(0, st0, 0, 0, 0.005, mp.PointAndTangent, mp.halfWidth, mp.slack)
    assert st.tobytes() == st0.tobytes() and m.state[0].tolist() == [0, 0, 0, 0, 1]
    st, _ = m.apply(0, st0, 0, 7, 0.005, mp.PointAndTangent, mp.halfWidth, mp.slack)
    assert np.signbit(st[7]) and st[2] == st0[2] and st[3] != st0[3] and m.state[0, 3] == 1.0 and m.state[0, 0] == 0.0


def gust_run(B, sigma, rho, n_bound, seed, calls):
    rows = np.tile(D.ALL_OFF, (B, 1)); rows[:, :3] = sigma; rows[:, 3] = rho
    m = D.Model(rows, seed=seed, n_bound=n_bound)
    hist = []
    for _ in range(calls):
        for b in range(B):
            for ch in range(3):
                m.gust(b, ch)
            m.state[b, 3] += 1.0
        hist.append(m.state[:, :3].copy())
    return hist


def test_gust_statistics_of_the_restatement():
    """The case of the GPU test on the restatement alone: std, mean and lag-1 correlation across 4096 vehicles at tick 20, each
    channel, inside five standard errors; draws depend on (seed, vid, tick) only."""
    c = D.GUST_CASE
    hist = gust_run(**c)
    b_std, b_mean, b_rho = D.gust_bars(c["B"], c["rho"])
    for ch in range(3):
        sd, mean, r = D.gust_stats(hist[20][:, ch], hist[21][:, ch])
        print("channel %d: std %.4f (bar %.4f), mean %.4f (bar %.4f), lag-1 %.4f (bar %.4f)" % (ch, sd, b_std, mean, b_mean, r, b_rho))
        assert abs(sd - 1.0) <= b_std and abs(mean) <= b_mean and abs(r - c["rho"]) <= b_rho
    # sharding: vehicles 32 .. 63 of a fleet are vehicles 0 .. 31 of a shard with vehicle_offset 32
    rows = np.tile(D.ALL_OFF, (64, 1)); rows[:, :3] = 0.4; rows[:, 3] = 0.6
    whole, shard = D.Model(rows, seed=5), D.Model(rows[32:], seed=5, vehicle_offset=32)
    for _ in range(3):
        for b in range(32):
            assert whole.gust(32 + b, 1) == shard.gust(b, 1)
            whole.state[32 + b, 3] += 1; shard.state[b, 3] += 1
    other = D.Model(rows, seed=5 ^ D.DIST_STREAM)                             # the stream constant separates the sensors' seed
    assert other.seed == 5 and D.Model(rows, seed=5).seed != 5


def test_header_declares_and_library_exports_the_calls():
    from lpvmpc import _ffi
    hdr = open(os.path.join(ROOT, "include", "lpvmpc.h")).read()
    for name in CALLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _ffi.EXPORTS
    assert re.search(r"#define\s+LPVMPC_DIST_WORDS\s+13\b", hdr) and re.search(r"#define\s+LPVMPC_DIST_STATE\s+5\b", hdr)
    m = re.search(r"#define\s+LPVMPC_DIST_STREAM\s+(0x[0-9A-Fa-f]+)ull", hdr)
    assert m and int(m.group(1), 16) == D.DIST_STREAM == _ffi.DIST_STREAM
    assert re.search(r"typedef struct lpvmpc_disturbance_config \{\s*uint64_t seed;[^}]*int64_t\s+vehicle_offset;[^}]*double\s+n_bound;", hdr)
    assert (_ffi.DIST_WORDS, _ffi.DIST_STATE) == (13, 5) and len(D.WORDS) == 13
    import ctypes
    so = ctypes.CDLL(_ffi.LIB_PATH)
    for name in CALLS:
        assert hasattr(so, name), name
    c = _ffi.default_disturbance_config()
    assert (c.seed, c.vehicle_offset, c.n_bound) == (0, 0, 3.0)


def test_the_kernel_lives_in_its_own_file():
    """disturbance.hip defines disturbance_kernel and no other kernel; the shared headers of the fleet kernels know nothing of the
    feature; the Makefile gates the kernel's resources."""
    src = open(os.path.join(CSRC, "disturbance.hip")).read()
    kernels = set(re.findall(r"__global__\s+void\s+(?:__launch_bounds__\(\d+\)\s+)?(\w+)\s*\(", src))
    assert kernels == {"disturbance_kernel"}, kernels
    assert "__shared__" not in src
    for name in UNTOUCHED:
        text = open(os.path.join(CSRC, name)).read()
        assert not re.search(r"disturb|DistDev|kDist", text, re.I), name
    for name in os.listdir(CSRC):
        if name.endswith(".hip") and name != "disturbance.hip":
            assert "disturbance_kernel" not in open(os.path.join(CSRC, name)).read(), name
    mk = open(os.path.join(CSRC, "Makefile")).read()
    rule = re.search(r"^disturbance\.o:.*\n\t(.*)$", mk, re.M).group(1)
    assert "-ffp-contract=off" in rule and "$(RESCHK)" in rule and "disturbance_kernel" in rule and "--allow" not in rule


def test_row_helpers_validate_and_refuse():
    import lpvmpc
    from lpvmpc import disturbance as M
    B, L = 4, 13.0
    rows = lpvmpc.disturbance_rows(B, lap_length=L, sigma=0.3, rho=0.8, kick=(10, 0.2, -0.1), patch0=(12.0, 2.0, 0.5), p1_gamma=np.arange(B) * 0.25)
    assert rows.shape == (B, 13) and rows.dtype == np.float64 and rows.flags["C_CONTIGUOUS"]
    assert rows[2].tolist() == [0.3, 0.3, 0.3, 0.8, 10, 0.2, -0.1, 12.0, 2.0, 0.5, 0.0, 0.0, 0.5]
    assert np.array_equal(lpvmpc.disturbance_rows(2), np.tile(D.ALL_OFF, (2, 1))) and M.DIST_WORD_NAMES == D.WORDS
    bad = [(0, -0.1), (1, np.nan), (2, np.inf), (3, 1.0), (3, -0.01), (4, 2.5), (4, 2.0 ** 31), (5, np.nan), (6, -np.inf), (7, -0.1), (7, L),
           (8, -1.0), (8, L + 1e-9), (9, -0.5), (10, L), (11, 2 * L), (12, np.nan)]
    for i, v in bad:
        r = rows.copy(); r[1, i] = v
        with pytest.raises(ValueError):
            lpvmpc.check_disturbance_rows(r, B, L)
    ok = rows.copy(); ok[:, 4] = -7; ok[:, 8] = L; ok[:, 3] = 0.0
    assert np.array_equal(lpvmpc.check_disturbance_rows(ok, B, L), ok)
    for r, n in ((rows[:2], B), (rows[:, :12], B), (rows.astype(str), B)):
        with pytest.raises(ValueError):
            lpvmpc.check_disturbance_rows(r, n)
    with pytest.raises(TypeError):
        lpvmpc.disturbance_rows(B, sigma_az=1.0)
    a, b = lpvmpc.sample_disturbances(8, 3), lpvmpc.sample_disturbances(4, 3, offset=4)
    assert np.array_equal(a[4:], b) and np.all((a[:, :3] >= 0.2) & (a[:, :3] <= 1.0)) and np.all(a[:, 4] == -1)
    k = lpvmpc.sample_disturbances(8, 1, spread=dict(kick_step=(100, 200), kick_w=(-1, 1)))
    assert np.all(k[:, 4] == np.floor(k[:, 4])) and np.all(k[:, :4] == 0)
    assert lpvmpc.rho_from_tau(0.0, 1 / 30) == 0.0 and abs(lpvmpc.rho_from_tau(0.5, 1 / 30) - np.exp(-1 / 15)) < 1e-15
    with pytest.raises(ValueError):
        lpvmpc.rho_from_tau(-1.0, 0.1)
    import inspect
    assert "disturbance" in inspect.signature(lpvmpc.RaceFleet.__init__).parameters
    assert hasattr(lpvmpc.RaceFleet, "disturb") and hasattr(lpvmpc.RaceFleet, "disturbance")
    for name in ("set_disturbances", "disturbances_read", "plant_step_disturbed"):
        assert hasattr(lpvmpc.BatchedSolver, name)
