"""CPU tests of the gain-scheduled LPV estimator: the numpy restatement against the reference fixture, the synthesised
vertex gains, the C ABI of the new entry points and the documented noise generator."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import _observer_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIX = os.path.join(HERE, "golden", "estimator", "estimator.npz")


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(FIX))


def gains(fx):
    return {k: fx[k] for k in ("L_ls", "lim_ls", "L_hs", "lim_hs")}


def test_restated_step_matches_the_reference_grid(fx):
    g, dt = gains(fx), float(fx["dt"])
    n = len(fx["grid_k"])
    hs = ls = startup = outside = 0
    for i in range(n):
        xn, L, A, B = R.observer_step(g, fx["grid_est"][i], fx["grid_y"][i], fx["grid_u"][i], int(fx["grid_k"][i]), dt)
        for got, want in ((xn, fx["grid_new"][i]), (L, fx["grid_L"][i]), (A, fx["grid_A"][i]), (B, fx["grid_B"][i])):
            assert np.max(np.abs(got - want)) <= 1e-12 * max(1.0, np.max(np.abs(want))), i
        k = int(fx["grid_k"][i])
        vx = fx["grid_y"][i][0] if k * dt <= 0.02 else fx["grid_est"][i][0]
        startup += k * dt <= 0.02
        hs += vx > fx["lim_ls"][0, 1]; ls += vx <= fx["lim_ls"][0, 1]
        outside += vx > fx["lim_hs"][0, 1] or vx < fx["lim_ls"][0, 0]
    assert min(hs, ls, startup, outside) > 5


def test_restated_sensors_and_observer_match_the_reference_trace(fx):
    g = gains(fx)
    p0 = fx["trace_plant0"]
    v = R.Vehicle(g, p0, est0=fx["trace_est0"], gps0=(0.0, 0.0))      # the reference estimator's GPS starts at (0, 0)
    for k in range(len(fx["trace_u"])):
        st = fx["trace_plant"][k]
        y = v.substep(st, *fx["trace_u"][k])
        assert np.max(np.abs(y - fx["trace_y"][k])) <= 1e-12, k
        assert np.max(np.abs(v.est - fx["trace_est"][k])) <= 1e-10 * max(1.0, np.max(np.abs(fx["trace_est"][k]))), k
    # the trace exercises the GPS hold: the held position lags the plant on alternate steps
    held = np.abs(fx["trace_y"][:, 2] - fx["trace_plant"][:, 0]) > 0
    assert 150 < held.sum() < 250


def test_vertex_gains_are_hurwitz_at_every_vertex(fx):
    from lpvmpc import observer as O
    for lim, L in ((fx["lim_ls"], O.observer_vertex_gains(fx["lim_ls"])), (fx["lim_hs"], O.observer_vertex_gains(fx["lim_hs"]))):
        assert L.shape == (6, 5, 16)
        for i, vert in enumerate(O.polytope_vertices(lim)):
            A, _ = O.observer_ab(*vert)
            assert np.max(np.linalg.eigvals(A + L[:, :, i] @ O.C_OBS).real) < 0, i


def test_observer_abi_is_exported_and_mirrored(tmp_path):
    from lpvmpc import _ffi
    lib = _ffi.load()
    for name in ("lpvmpc_observer_default_config", "lpvmpc_observer_setup", "lpvmpc_observer_read", "lpvmpc_observer_step_batch"):
        assert hasattr(lib, name) and name in _ffi.EXPORTS
    src = tmp_path / "obs.c"
    src.write_text('#include "lpvmpc.h"\n#include <stdio.h>\n#include <stddef.h>\n'
                   'int main(){printf("%zu %zu %zu %zu %zu\\n", sizeof(lpvmpc_observer_config), offsetof(lpvmpc_observer_config, lim_hs),'
                   ' offsetof(lpvmpc_observer_config, loop_rate), offsetof(lpvmpc_observer_config, seed),'
                   ' offsetof(lpvmpc_observer_config, vehicle_offset)); return 0;}\n')
    exe = tmp_path / "obs"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    O = _ffi.ObserverConfig
    assert got == [C.sizeof(O), O.lim_hs.offset, O.loop_rate.offset, O.seed.offset, O.vehicle_offset.offset]
    cfg = _ffi.default_observer_config()
    assert (cfg.loop_rate, cfg.init_vx, cfg.n_bound, cfg.gps_freq, cfg.v_std, cfg.seed) == (200.0, 0.2, 0.5, 1000.0, 0.0, 0)
    assert all(v == 0.0 for v in cfg.L_ls)


def test_documented_generator_first_values():
    # splitmix64's finaliser of 0 is 0; the generator's published first draws for key (seed 1, vehicle 0, step 1)
    assert R.mix(0) == 0
    assert R.mix(1) == 0x5692161D100B05E5
    u = [R.uniforms(1, 0, 1, ch) for ch in range(5)]
    assert all(0.0 < a <= 1.0 and 0.0 <= b < 1.0 for a, b in u)
    g = np.array([R.gauss(1, 0, 1, ch) for ch in range(5)])
    np.testing.assert_allclose(g, FIRST_DRAWS, rtol=0, atol=1e-15)
    # a large sample is standard normal
    s = np.array([R.gauss(7, v, 3, 1) for v in range(4000)])
    assert abs(s.mean()) < 0.06 and abs(s.std() - 1.0) < 0.05
    # the documented formula in the header names these constants
    text = open(os.path.join(ROOT, "include", "lpvmpc.h")).read()
    for c in ("0xBF58476D1CE4E5B9", "0x94D049BB133111EB", "0x9E3779B97F4A7C15"):
        assert c in text


FIRST_DRAWS = [0.9431552654571836, -0.9322099338018945, 0.8276448885255477, 0.07884528385915293, 1.5405832337629908]
