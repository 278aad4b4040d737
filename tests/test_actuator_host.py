"""CPU tests of the actuator model: the numpy restatement (tests/_actuator_ref.py) against the fixture the reference's own
simulator loop wrote (tests/golden/actuator/actuator.npz), the fixture's provenance, the seconds -> steps helpers and the ctypes
mirror of lpvmpc_actuator_config."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _actuator_ref as AR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GDIR = os.path.join(HERE, "golden", "actuator")
FIX = os.path.join(GDIR, "actuator.npz")
REF_TREE = "/root/reference/workspace/src/barc/src"


@pytest.fixture(scope="module")
def fx():
    return np.load(FIX)


def test_restatement_matches_the_reference_loop(fx):
    """Every case -- no delay, a few steps, 0.145 s (28 steps: int() truncation), the 64-step cap, servo lag on and off -- to 1e-12
    on the plant state and on the input the simulator applied."""
    assert len(fx["La"]) >= 6 and 28 in fx["La"] and 1 in fx["lld"] and 0 in fx["lld"]
    for c in range(len(fx["La"])):
        st, ap = AR.simulate(fx["plant0"], fx["cmd"][c], fx["La"][c], fx["Ld"][c], fx["lld"][c], float(fx["dt"]))
        assert np.max(np.abs(ap - fx["applied"][c])) <= 1e-12, c
        assert np.max(np.abs(st - fx["state"][c])) <= 1e-12, c
        if fx["La"][c] > 0:                           # the delay shows: zeros first, then the command La steps late
            La = fx["La"][c]
            assert np.all(fx["applied"][c][:La, 0] == 0) and np.array_equal(fx["applied"][c][La:, 0], fx["cmd"][c][:-La, 0])
        if fx["lld"][c]:
            assert not np.array_equal(fx["applied"][c][:, 1], fx["cmd"][c][:, 1])


def test_seconds_to_steps_reproduce_int():
    import lpvmpc
    from lpvmpc import _ffi
    for d in (0.0, 0.005, 0.015, 0.035, 0.1, 0.145, 0.3, 0.32):
        assert lpvmpc.delay_steps(d) == int(d / 0.005)
        c = lpvmpc.actuator_config(d, d, low_level_dyn=True)
        assert isinstance(c, _ffi.ActuatorConfig) and c.delay_a == c.delay_df == int(d / 0.005) and c.low_level_dyn == 1
        assert lpvmpc.controller_delay(d) == int(d / (1.0 / 30.0))
    assert lpvmpc.delay_steps(0.145) == 28 and lpvmpc.delay_steps(0.035) == 7
    assert lpvmpc.controller_delay(0.1) == 3 and lpvmpc.controller_delay(0.145) == 4
    c = lpvmpc.actuator_config()
    assert (c.delay_a, c.delay_df, c.low_level_dyn, c.servo_tf) == (0, 0, 0, 0.07)


def test_fixture_data_follows_its_generator(fx):
    """The fixture's inputs are what make_actuator_golden.py schedules, its FIFO lengths are int(delay / dt) of its delays, and its
    key set is the generator's manifest.  Where the reference tree is present the generator is run again and must reproduce the
    fixture bit for bit."""
    sys.path.insert(0, GDIR)
    try:
        import make_actuator_golden as G
    finally:
        sys.path.remove(GDIR)
    assert len(G.CASES) == len(fx["La"])
    for c, (da, dd, lld) in enumerate(G.CASES):
        assert (fx["delay_a"][c], fx["delay_df"][c], fx["lld"][c]) == (da, dd, int(lld))
        assert (fx["La"][c], fx["Ld"][c]) == (int(da / G.DT), int(dd / G.DT))
        s = G.schedule(c)
        assert np.array_equal(fx["cmd"][c][1:], s[1:]) and np.all(fx["cmd"][c][0] == 0)
    man = json.load(open(os.path.join(GDIR, "MANIFEST.json")))["actuator.npz"]
    assert sorted(man) == sorted(fx.files)
    for k in fx.files:
        assert [list(fx[k].shape), str(fx[k].dtype)] == [man[k]["shape"], man[k]["dtype"]], k
    if os.path.isdir(REF_TREE):
        out = os.path.join(os.environ.get("TMPDIR", "/tmp"), "actuator_regen_%d" % os.getpid())
        os.makedirs(out, exist_ok=True)
        subprocess.run([sys.executable, os.path.join(GDIR, "make_actuator_golden.py"), "--out", out], check=True, capture_output=True)
        new = np.load(os.path.join(out, "actuator.npz"))
        for k in fx.files:
            assert fx[k].tobytes() == new[k].tobytes(), k


def test_history_recursion():
    """OldSteering = [0] * (1 + d), OldAccelera = [0]: appending commands and dropping the oldest entry, in the device layout."""
    for d in (0, 1, 3, 8):
        steer, acc = [0.0] * (1 + d), [0.0]
        h = np.zeros(2 + d)
        for t in range(12):
            s, m = 0.1 * t + 0.01, -0.2 * t
            steer.append(s); steer.pop(0); acc.append(m); acc.pop(0)
            h = AR.uold_push(h, s, m)
            assert np.array_equal(h, [steer[0], acc[0]] + steer[1:]), (d, t)


def test_ring_words_follow_the_fifo():
    a = AR.Actuator(5, 3, True)
    for k in range(150):
        a.step(k * 1.0, -k * 1.0)
    w = a.words()
    assert w[-1] == 150 and w[-2] == a.servo_inp
    assert w[149 % 64] == 149 and w[64 + 149 % 64] == -149 and w[150 % 64] == 150 - 64


def test_actuator_config_layout(tmp_path):
    from lpvmpc import _ffi
    src = tmp_path / "a.c"
    src.write_text('#include "lpvmpc.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                   'int main(){printf("%zu %zu %zu %zu %zu %d %d\\n", sizeof(lpvmpc_actuator_config), offsetof(lpvmpc_actuator_config, delay_df),'
                   ' offsetof(lpvmpc_actuator_config, low_level_dyn), offsetof(lpvmpc_actuator_config, reserved),'
                   ' offsetof(lpvmpc_actuator_config, servo_tf), LPVMPC_ACT_MAX_DELAY, LPVMPC_ACT_WORDS); return 0;}\n')
    exe = tmp_path / "a"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, odf, olld, ores, otf, cap, words = map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    A = _ffi.ActuatorConfig
    assert (C.sizeof(A), A.delay_df.offset, A.low_level_dyn.offset, A.reserved.offset, A.servo_tf.offset) == (size, odf, olld, ores, otf)
    assert (_ffi.ACT_MAX_DELAY, _ffi.ACT_WORDS) == (cap, words) == (AR.ACT_MAX_DELAY, AR.ACT_WORDS)
