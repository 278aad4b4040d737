"""GPU: the batched gain design of the per-vehicle estimator (csrc/observer_design.hip, lpvmpc_observer_design_batch) against the
scipy fixture tests/golden/estimator_vehicles/design.npz.  The bars are the numpy restatement's own worst figures on the same 1280
problems (tests/_observer_design_ref.yardstick, printed by tests/test_observer_design_host.py) times 100: the margin for the other
pivot ties and summation orders of a 16-lane elimination."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _observer_design_ref as D  # noqa: E402

pytestmark = pytest.mark.gpu
SIZES = (1, 5, 67)          # a lone vehicle; 16-lane groups that end mid-wavefront; a batch past a 64-lane boundary


def engine():
    import lpvmpc
    return lpvmpc.BatchedSolver("controller", 20, 1 / 30.0, np.eye(6), np.eye(2), np.ones(2))


@pytest.fixture(scope="module")
def runs():
    """The design at the three batch sizes (the fixture's rows, recycled), twice each, and the second weight set."""
    f = D.fixture()
    eng = engine()
    out = {"f": f}
    for B in SIZES:
        idx = np.arange(B) % 40
        out[B] = [eng.observer_design(f["rows"][idx], f["lim_ls"], f["lim_hs"], want_iters=True) for _ in range(2)]
    out["set2"] = eng.observer_design(f["rows"][:8], f["lim_ls"], f["lim_hs"], f["Qo2"], f["Ro2"], want_iters=True)
    eng.close()
    return out


@pytest.mark.parametrize("B", SIZES)
def test_gains_residual_stability_and_iterations(runs, B):
    f, y = runs["f"], D.yardstick()
    idx = np.arange(B) % 40
    L_ls, L_hs, it = runs[B][0]
    err = max(D.gain_error(L_ls, f["L_ls"][idx]), D.gain_error(L_hs, f["L_hs"][idx]))
    res_ls, re_ls = D.residual_of_gains(f["rows"][idx], f["lim_ls"], L_ls)
    res_hs, re_hs = D.residual_of_gains(f["rows"][idx], f["lim_hs"], L_hs)
    print("B = %d: device vs scipy worst relative gain error %.3e (restatement %.3e), worst relative residual %.3e (restatement %.3e), "
          "iterations %d..%d, max Re eig(A + L C) %.3f" % (B, err, y["gain"], max(res_ls, res_hs), y["resid"], it.min(), it.max(), max(re_ls, re_hs)))
    assert err <= 100 * y["gain"]
    assert max(res_ls, res_hs) <= 100 * y["resid"]
    assert max(re_ls, re_hs) < 0.0                                            # A + L C Hurwitz at every vertex
    assert it.shape == (B, 2, 16) and it.min() >= 1 and it.max() <= 40
    assert np.all(np.isfinite(L_ls)) and np.all(np.isfinite(L_hs))


def test_a_vehicles_tables_do_not_depend_on_the_batch_or_the_run(runs):
    big = runs[67][0]
    for B in SIZES:
        a, b = runs[B]
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes(), B                              # two runs
        for k in range(3):
            assert a[k].tobytes() == big[k][:B].tobytes(), (B, k)             # vehicle b's 960 words (and counts) at every size
    # rows 40..66 repeat rows 0..26: the same words wherever a problem lands in the grid
    for k in range(3):
        assert big[k][40:67].tobytes() == big[k][0:27].tobytes()


def test_non_diagonal_weights(runs):
    f, y = runs["f"], D.yardstick()
    L_ls, L_hs, it = runs["set2"]
    err = max(D.gain_error(L_ls, f["L2_ls"]), D.gain_error(L_hs, f["L2_hs"]))
    res = max(D.residual_of_gains(f["rows"][:8], f["lim_ls"], L_ls, f["Qo2"], f["Ro2"])[0],
              D.residual_of_gains(f["rows"][:8], f["lim_hs"], L_hs, f["Qo2"], f["Ro2"])[0])
    print("non-diagonal Qo, Ro: device vs scipy worst relative gain error %.3e, residual %.3e, iterations %d..%d" % (err, res, it.min(), it.max()))
    assert err <= 100 * y["gain"] and res <= 100 * y["resid"] and it.min() >= 1 and it.max() <= 40


def test_not_converged_gives_nan_and_minus_one():
    """No measurement weight worth the name and no process noise: the Hamiltonian has eigenvalues on the imaginary axis and the
    sign iteration has no limit."""
    f = D.fixture()
    eng = engine()
    L_ls, L_hs, it = eng.observer_design(f["rows"][:3], f["lim_ls"], f["lim_hs"], np.zeros((6, 6)), np.diag([1e300] * 5), want_iters=True)
    assert np.all(it == -1) and np.all(np.isnan(L_ls)) and np.all(np.isnan(L_hs))
    eng.close()


def test_refusals_leave_the_outputs_untouched():
    import lpvmpc
    from lpvmpc import _ffi
    from lpvmpc.api import observer_design_config
    f = D.fixture()
    eng = engine()
    B = 5
    rows = np.ascontiguousarray(f["rows"][:B])
    good = observer_design_config(f["lim_ls"], f["lim_hs"])

    def call(e, rows_, d):
        L_ls, L_hs, it = np.full((B, 6, 5, 16), 7.0), np.full((B, 6, 5, 16), 7.0), np.full((B, 2, 16), 7, np.int32)
        rc = e._lib.lpvmpc_observer_design_batch(e._h, B, _ffi.ptr(rows_), C.byref(d), _ffi.ptr(L_ls), _ffi.ptr(L_hs), _ffi.ptr(it))
        return rc, np.all(L_ls == 7.0) and np.all(L_hs == 7.0) and np.all(it == 7)

    assert call(eng, rows, good) == (0, False)
    bad_rows = []
    for col, v in ((2, -1.0), (0, 0.0), (4, -60.0), (6, np.nan), (3, np.inf)):
        r = rows.copy(); r[B - 1, col] = v
        bad_rows.append(r)
    for r in bad_rows:
        assert call(eng, r, good) == (_ffi.E_ARG, True)
    Ro_bad = [np.diag([0.1, 0.1, 0.01, 0.01, -0.01]), np.zeros((5, 5)), np.array(D.RO_DEFAULT) + np.triu(np.full((5, 5), 0.001), 1),
              np.full((5, 5), np.nan)]
    for Ro in Ro_bad:
        assert call(eng, rows, observer_design_config(f["lim_ls"], f["lim_hs"], Ro=Ro)) == (_ffi.E_ARG, True)
    Qn = np.eye(6); Qn[2, 2] = -1.0
    Qa = np.eye(6); Qa[0, 1] = 0.5
    Qf = np.eye(6); Qf[3, 3] = np.inf
    for Qo in (Qn, Qa, Qf):
        assert call(eng, rows, observer_design_config(f["lim_ls"], f["lim_hs"], Qo=Qo)) == (_ffi.E_ARG, True)
    assert call(eng, rows, observer_design_config(f["lim_ls"], f["lim_hs"], Qo=np.zeros((6, 6))))[0] == 0     # semidefinite is allowed
    for row in (0, 1, 3, 5):
        lim = f["lim_hs"].copy(); lim[row, 1] = lim[row, 0]
        assert call(eng, rows, observer_design_config(f["lim_ls"], lim)) == (_ffi.E_ARG, True)
        lim = f["lim_ls"].copy(); lim[row] = lim[row, ::-1]
        assert call(eng, rows, observer_design_config(lim, f["lim_hs"])) == (_ffi.E_ARG, True)
    lim = f["lim_ls"].copy(); lim[0, 0] = 0.0
    assert call(eng, rows, observer_design_config(lim, f["lim_hs"])) == (_ffi.E_ARG, True)
    assert "vx" in eng._lib.lpvmpc_last_error(eng._h).decode()
    eng.close()
    # refused while the handle runs a fleet, like the other batch calls
    from lpvmpc import workloads
    Q, Rm, dR = workloads.CTRL_TUNINGS["path"]
    mp = lpvmpc.Map("oval", 0.2)
    e = lpvmpc.BatchedSolver("controller", 20, 1 / 30.0, Q, Rm, dR, track=mp.PointAndTangent)
    p0 = np.zeros((4, 8)); p0[:, 2] = 1.0
    e.cl_init(p0, mp.halfWidth, mp.slack)
    assert call(e, rows, good) == (_ffi.E_ARG, True)
    e.cl_release()
    assert call(e, rows, good) == (0, False)
    e.close()
