"""GPU: the device actuator stage (lpvmpc_plant_step_actuated_batch) against the fixture of the reference's own simulator loop
(tests/golden/actuator/actuator.npz), step by step, with the actuator state carried across calls."""
import os

import numpy as np
import pytest

from tests import _actuator_ref as AR

pytestmark = pytest.mark.gpu

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "actuator", "actuator.npz")


def chunks(K, hold):
    """[start, stop) runs of a held command: holds of 7 / 7 / 6 steps from step 0, whose step 0 runs alone (EcuClass's initial
    [0, 0]; the schedule's first command arrives after it)."""
    out, k, h = [], 0, 0
    while k < K:
        n = int(hold[h % 3]); out.append((k, min(k + n, K))); k += n; h += 1
    return [(0, 1), (1, out[0][1])] + out[1:]


def engine():
    import lpvmpc
    from lpvmpc import workloads as W
    Qp, Rp, dRp = W.CTRL_TUNINGS["path"]
    return lpvmpc.BatchedSolver("controller", 20, 1 / 30.0, Qp, Rp, dRp)


@pytest.mark.parametrize("lld", [0, 1])
def test_plant_step_actuated_matches_the_reference_loop(lld):
    """All fixture cases of one lowLevelDyn setting in one batch, with their per-vehicle delays: one call per held command (n_sub =
    hold) matches the reference's states to 1e-11 after every call; the actuator state carries across calls, so per-step calls
    (n_sub = 1) give the same words; the final actuator state is the ring of the last 64 commands, servo_inp and the step count."""
    import lpvmpc
    fx = np.load(FIX)
    cases = np.nonzero(fx["lld"] == lld)[0]
    B, K = len(cases), fx["cmd"].shape[1]
    cfg = lpvmpc.actuator_config(low_level_dyn=bool(lld))
    La, Ld = fx["La"][cases], fx["Ld"][cases]
    e = engine()
    st, act = np.tile(fx["plant0"], (B, 1)), None
    st1, act1 = st.copy(), None
    worst = 0.0
    for a, b in chunks(K, fx["hold"]):
        u = fx["cmd"][cases, a]
        assert np.all(fx["cmd"][cases, a:b] == u[:, None, :])
        st, act = e.plant_step_actuated(st, act, u, n_sub=b - a, actuator=cfg, delay_a=La, delay_df=Ld)
        worst = max(worst, float(np.max(np.abs(st - fx["state"][cases, b - 1]))))
        for _ in range(a, b):
            st1, act1 = e.plant_step_actuated(st1, act1, u, n_sub=1, actuator=cfg, delay_a=La, delay_df=Ld)
    print("lld %d: max |device - reference| = %.3e over %d steps, %d vehicles" % (lld, worst, K, B))
    assert worst <= 1e-11
    assert st.tobytes() == st1.tobytes() and act.tobytes() == act1.tobytes()
    for i, c in enumerate(cases):
        ref = AR.Actuator(La[i], Ld[i], lld)
        for m, s in fx["cmd"][c]:
            ref.step(m, s)
        w = ref.words()
        assert np.array_equal(act[i, :-2], w[:-2]) and act[i, -1] == K
        assert abs(act[i, -2] - w[-2]) <= 1e-12
    e.close()


def test_uniform_config_and_refusals():
    """NULL delay arrays take the config's delay for every vehicle; delays above the cap or negative, a fractional step counter
    and arrays of the wrong length are refused."""
    import lpvmpc
    fx = np.load(FIX)
    c = int(np.nonzero((fx["La"] == 28) & (fx["lld"] == 0))[0][0])
    e = engine()
    cfg = lpvmpc.actuator_config(0.145, fx["delay_df"][c])
    st, act = fx["plant0"][None, :].copy(), None
    for a, b in chunks(120, fx["hold"]):
        st, act = e.plant_step_actuated(st, act, fx["cmd"][c:c + 1, a], n_sub=b - a, actuator=cfg)
    assert np.max(np.abs(st[0] - fx["state"][c, 119])) <= 1e-11
    from lpvmpc import _ffi
    for la in (65, -1):
        bad = _ffi.ActuatorConfig(); bad.delay_a = la; bad.servo_tf = 0.07
        with pytest.raises(lpvmpc.LpvMpcError):
            e.plant_step_actuated(st, None, [[0.0, 0.0]], actuator=bad)
    with pytest.raises(lpvmpc.LpvMpcError):
        e.plant_step_actuated(st, None, [[0.0, 0.0]], actuator=lpvmpc.actuator_config(), delay_df=[70])
    a2 = np.zeros((1, AR.ACT_WORDS)); a2[0, -1] = 2.5
    with pytest.raises(lpvmpc.LpvMpcError):
        e.plant_step_actuated(st, a2, [[0.0, 0.0]], actuator=lpvmpc.actuator_config())
    with pytest.raises(ValueError):
        e.plant_step_actuated(st, None, [[0.0, 0.0]], actuator=lpvmpc.actuator_config(), delay_a=[1, 2])
    e.close()
