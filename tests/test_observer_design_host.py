"""CPU: the per-vehicle estimator's host side -- the scipy fixture regenerates to itself, the numpy restatement of the device design
(tests/_observer_design_ref.py) against it (the figures it prints are the yardstick the GPU tests hold the device to), the
per-vehicle observer step against tests/_observer_ref.py, the new C ABI symbols and observer_vertex_gains' ``params``."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _observer_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _observer_design_ref as D  # noqa: E402  (it imports _observer_ref by its bare name)

GEN = os.path.join(HERE, "golden", "estimator_vehicles", "make_design_golden.py")
NEW = ("lpvmpc_observer_default_design", "lpvmpc_observer_design_batch", "lpvmpc_set_observer_vehicles", "lpvmpc_observer_vehicles_read",
       "lpvmpc_observer_step_vehicles_batch")


def test_fixture_layout_and_rows():
    f = D.fixture()
    est = np.load(os.path.join(HERE, "golden", "estimator", "estimator.npz"))
    assert np.array_equal(f["lim_ls"], est["lim_ls"]) and np.array_equal(f["lim_hs"], est["lim_hs"])
    assert f["rows"].shape == (40, 7) and np.array_equal(f["rows"][0], D.NOMINAL_ROW)
    assert np.all(np.abs(f["rows"] / D.NOMINAL_ROW - 1.0) <= 0.30 + 1e-12) and np.all(np.abs(f["rows"][1:] / D.NOMINAL_ROW - 1.0) > 0)
    assert f["L_ls"].shape == f["L_hs"].shape == (40, 6, 5, 16) and f["L2_ls"].shape == f["L2_hs"].shape == (8, 6, 5, 16)
    # the nominal row's tables are the ones the estimator fixture carries; the second set's weights are not diagonal
    assert np.array_equal(f["L_ls"][0], est["L_ls"]) and np.array_equal(f["L_hs"][0], est["L_hs"])
    for M in (f["Qo2"], f["Ro2"]):
        assert np.all(M[~np.eye(len(M), dtype=bool)] != 0) and np.array_equal(M, M.T) and np.all(np.linalg.eigvalsh(M) > 0)


def test_fixture_regenerates_to_itself(tmp_path):
    pytest.importorskip("scipy")
    out = tmp_path / "design.npz"
    subprocess.run([sys.executable, GEN, str(out)], check=True, capture_output=True)
    new, old = dict(np.load(out)), D.fixture()
    assert sorted(new) == sorted(old)
    for k in old:
        assert np.array_equal(new[k], old[k]), k


def test_vertex_gains_params_default_keeps_todays_words():
    pytest.importorskip("scipy")
    from lpvmpc.observer import OBS_PARAMS, observer_ab, observer_vertex_gains
    f = D.fixture()
    for lim in (f["lim_ls"], f["lim_hs"]):
        a, b, c = observer_vertex_gains(lim), observer_vertex_gains(lim, params=OBS_PARAMS), observer_vertex_gains(lim, params=D.NOMINAL_ROW)
        assert np.array_equal(a, b) and np.array_equal(a, c)
    for x, y in zip(observer_ab(0.7, 0.1, 0.3, -0.2), observer_ab(0.7, 0.1, 0.3, -0.2, params=OBS_PARAMS)):
        assert np.array_equal(x, y)
    # a row changes them, and the restatement builds the same A
    row = f["rows"][3]
    A, B = observer_ab(0.7, 0.1, 0.3, -0.2, params=row)
    assert not np.array_equal(A, observer_ab(0.7, 0.1, 0.3, -0.2)[0])
    A2, B2 = D.a_obs(row, 0.7, 0.1, 0.3, -0.2)
    assert np.allclose(A, A2, rtol=1e-15, atol=0) and np.allclose(B, B2, rtol=1e-15, atol=0)


def test_restatement_against_scipy_is_the_yardstick():
    """The figures printed here are what tests/test_gpu_observer_design.py multiplies by 100 for the device (trial run of the
    algorithm before it was written for the device: 1.1e-12 and 6.8e-13; this restatement: 1.2e-12 and 1.6e-13)."""
    f, y = D.fixture(), D.yardstick()
    print("restatement vs scipy, 1280 problems: worst relative gain error %.3e, worst relative residual %.3e, iterations %d..%d, "
          "largest gain word %.3f" % (y["gain"], y["resid"], y["iters"][0], y["iters"][1], max(np.abs(y["L_ls"]).max(), np.abs(y["L_hs"]).max())))
    # far inside what double precision gives an equation of this conditioning; never a bar taken from the device
    assert y["gain"] <= 1e-10 and y["resid"] <= 1e-10
    assert 1 <= y["iters"][0] and y["iters"][1] <= 12
    for lim, L in ((f["lim_ls"], y["L_ls"]), (f["lim_hs"], y["L_hs"])):
        assert D.residual_of_gains(f["rows"], lim, L)[1] < -1.0                  # every closed loop well inside the left half plane
    # the second set: weights with every off-diagonal word set
    L_ls, L_hs, it, _ = D.design(f["rows"][:8], f["lim_ls"], f["lim_hs"], f["Qo2"], f["Ro2"])
    e2 = max(D.gain_error(L_ls, f["L2_ls"]), D.gain_error(L_hs, f["L2_hs"]))
    print("second set (non-diagonal Qo, Ro), 256 problems: worst relative gain error %.3e, iterations %d..%d" % (e2, it.min(), it.max()))
    assert e2 <= 1e-10 and it.min() >= 1


def test_restatement_fails_loudly_without_a_stabilising_solution():
    """(A, C) not detectable -- here: no measurement weight at all on a marginally stable chain -- has no sign decomposition:
    NaN gains and iteration count -1, not a silent number."""
    f = D.fixture()
    Ro = np.diag([1e300] * 5)
    L_ls, _L_hs, it, _ = D.design(f["rows"][:1], f["lim_ls"], f["lim_hs"], np.zeros((6, 6)), Ro)
    assert np.all(it == -1) and np.all(np.isnan(L_ls))


def test_per_vehicle_step_with_the_nominal_row_is_the_observer_restatement():
    est = dict(np.load(os.path.join(HERE, "golden", "estimator", "estimator.npz")))
    g = {k: est[k] for k in ("L_ls", "lim_ls", "L_hs", "lim_hs")}
    dt = float(est["dt"])
    for i in range(len(est["grid_k"])):
        a = R.observer_step(g, est["grid_est"][i], est["grid_y"][i], est["grid_u"][i], int(est["grid_k"][i]), dt)
        b = D.observer_step(D.NOMINAL_ROW, g["L_ls"], g["L_hs"], g["lim_ls"], g["lim_hs"], est["grid_est"][i], est["grid_y"][i],
                            est["grid_u"][i], int(est["grid_k"][i]), dt)
        for x, y in zip(a, b):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), i
    # and the Vehicle: sensors + observer over the fixture's open-loop trace
    va = R.Vehicle(g, est["trace_plant0"], dt=dt)
    vb = D.Vehicle(D.NOMINAL_ROW, g["L_ls"], g["L_hs"], g["lim_ls"], g["lim_hs"], est["trace_plant0"], dt=dt)
    for k in range(60):
        servo, motor = est["trace_u"][k]
        ya, yb = va.substep(est["trace_plant"][k], servo, motor), vb.substep(est["trace_plant"][k], servo, motor)
        assert ya.tobytes() == yb.tobytes() and va.est.tobytes() == vb.est.tobytes(), k
    # another row or other tables change the step
    f = D.fixture()
    c = D.observer_step(f["rows"][5], g["L_ls"], g["L_hs"], g["lim_ls"], g["lim_hs"], est["grid_est"][0], est["grid_y"][0], est["grid_u"][0], 50, dt)
    d = D.observer_step(D.NOMINAL_ROW, f["L_ls"][5], f["L_hs"][5], g["lim_ls"], g["lim_hs"], est["grid_est"][0], est["grid_y"][0], est["grid_u"][0], 50, dt)
    a = R.observer_step(g, est["grid_est"][0], est["grid_y"][0], est["grid_u"][0], 50, dt)
    assert not np.array_equal(c[0], a[0]) and not np.array_equal(d[0], a[0])


def test_new_symbols_are_declared_exported_and_mirrored():
    import ctypes as C
    from lpvmpc import _ffi
    text = open(os.path.join(os.path.dirname(HERE), "include", "lpvmpc.h")).read()
    lib = _ffi.load()
    for n in NEW:
        assert n + "(" in text and n in _ffi.EXPORTS and hasattr(lib, n), n
    d = _ffi.default_observer_design()
    assert C.sizeof(_ffi.ObserverDesign) == 8 * (12 + 12 + 36 + 25)
    assert np.array_equal(np.array(d.Qo[:]).reshape(6, 6), np.eye(6)) and np.array_equal(np.array(d.Ro[:]).reshape(5, 5), D.RO_DEFAULT)
    assert not any(d.lim_ls[:]) and not any(d.lim_hs[:])
