"""GPU: the ADMM iteration of the controller's N = 20 kernel on every path of its element phases, against the CPU oracle.

The headline kernel (two wavefronts per instance, element state in registers) runs its update phase in two forms, chosen per wavefront:
wavefront 0 owns two elements per lane (elements 0 .. 127 and 128 .. 167 on its first 40 lanes, the others repeat their first
element), wavefront 1 one; each form exists for the first iteration of a launch and for the others, and each takes the ADMM weight of
its box rows from registers that only a rho update rewrites.  The riders entry runs the same text behind a restore, the closing pass
behind another.  The cases are the smallest batches that reach all of it:
  B = 1     one instance: both wavefront roles of one workgroup
  B = 5     an odd count, fewer instances than a compute unit holds twice over
  B = 130   more than one 128-entry pool's worth
  B = 130, three deferred calls (defer_after 25 / defer_budget 25) and a join: instances park at their first check, ride in the next
            call's launch, park again and finish in the closing pass
under both controller tunings of workloads.CTRL_TUNINGS.

Compared with oracle/osqp_ref.py tick_batch_qp on the same inputs: status, iteration count and polish flag exactly; xPred / uPred by
tests/_tolerance.py check_batch (1e-6 polished, 2e-4 otherwise: the bounds of tests/test_gpu_parity.py); the four residual words by
check_resid under RESID_BOUNDS.

Deferred case, oracle iteration counts of the three batches (seeds 16, 3, 103; 130 instances each; checks every 25 iterations):
  racing tuning   more than 25 iterations: 122 / 127 / 127,  more than 50: 18 / 24 / 20,  more than 75: 4 / 2 / 2
  path tuning     more than 25 iterations:  88 / 100 /  93,  more than 50: 19 / 21 / 24,  more than 75: 2 / 0 / 2
so call 1 has at least 88 candidates for its pool at iteration 25 (at least 64 are parked: asserted), at least 18 of them need call 2's
launch to go beyond iteration 50 (at least one is parked a second time: asserted), and two or more are left for call 3's launch and
the join."""
import numpy as np
import pytest

from oracle import osqp_ref as O
from tests import _tolerance as T
from tests import test_gpu_deferral_riders as R

pytestmark = pytest.mark.gpu

PENDING = -11
SEEDS = (16, 3, 103)
_CACHE = {}


def batch(tuning, B, seed):
    """The workload and the oracle's answer, computed once per (tuning, B, seed) and shared."""
    from lpvmpc import workloads
    key = (tuning, B, seed)
    if key not in _CACHE:
        w = dict(workloads.controller_batch(B, N=20, seed=seed))
        w["Q"], w["R"], w["dR"] = workloads.CTRL_TUNINGS[tuning]
        ref = O.tick_batch_qp(w, "controller", nthreads=8)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CACHE[key] = (w, ref)
    return _CACHE[key]


def against_oracle(w, out, ref, tag):
    B = w["x0"].shape[0]
    out = {k: np.asarray(v) for k, v in out.items() if isinstance(v, np.ndarray)}
    for k in ("status", "iters", "polish"):
        assert np.array_equal(out[k], ref[k]), (tag, k, np.nonzero(out[k] != ref[k])[0][:8], out[k][out[k] != ref[k]][:8], ref[k][out[k] != ref[k]][:8])
    counts = T.check_batch(w, "controller", out, ref, allow_status_flip_at_max_iter=False)
    rep = T.check_resid(w, "controller", out, ref, T.RESID_BOUNDS)
    assert rep["left_out"] == [], (tag, rep["left_out"])
    assert sum(rep["counts"][c] for c in "ABCD") == B, (tag, rep["counts"])
    print("%s: iters %d..%d, solution classes %s, resid classes %s" % (tag, int(out["iters"].min()), int(out["iters"].max()), counts, rep["counts"]))
    return out


@pytest.mark.parametrize("tuning", ["race", "path"])
@pytest.mark.parametrize("B", [1, 5, 130])
def test_plain_solve_matches_the_oracle(tuning, B):
    from lpvmpc import workloads
    w, ref = batch(tuning, B, SEEDS[0])
    eng = workloads.make_solver(w)
    out = eng.solve(w["x0"], w["u_prev"], w["vel_ref"], w["curv_s"], w["u_old"], None, w["cf_new"], w["lap"])
    eng.close()
    out = against_oracle(w, out, ref, "%s B=%d" % (tuning, B))
    if B == 130:
        assert (out["iters"] > 50).any() and (out["polish"] == 1).any()      # (rho updates and the polish ran)


@pytest.mark.parametrize("tuning", ["race", "path"])
def test_three_deferred_calls_and_a_join_match_the_oracle(tuning):
    """defer_after 25 / defer_budget 25 on one stream: see the module docstring for the counts that make instances park twice."""
    import torch
    B, K = 130, 25
    ws, refs = zip(*(batch(tuning, B, s) for s in SEEDS))
    # (from the oracle, on the CPU: parked at 25 by call 1, riders of call 2 that park again at 50, riders of call 3 left for the join)
    assert int((refs[0]["iters"] > K).sum()) >= 88 and int((refs[0]["iters"] > 2 * K).sum()) >= 18 and int((refs[0]["iters"] > 3 * K).sum()) >= 2
    # (pool admission is by age class -- first-time candidates may take three quarters of a pool -- so of more than 96 candidates
    # some are refused and finish inside their launch: which ones depends on timing, the results do not)
    eng = R._deferred(ws[0], B, K, K, pool=128)
    st = torch.cuda.Stream()
    calls, seen = [], []
    for j, w in enumerate(ws):
        calls.append(R._dev_call(torch, eng, w, B, False, stream=st))
        torch.cuda.synchronize()
        seen.append(R._host(calls[0][1]))          # call 1's outputs behind every call
    late = refs[0]["iters"] > K
    pend = [h["status"] == PENDING for h in seen]
    # call 1 alone: what is pending was parked at the first check; everything else is finished and final
    assert pend[0].sum() >= 64 and not np.any(pend[0] & ~late) and np.all(seen[0]["iters"][pend[0]] == K), (int(pend[0].sum()), seen[0]["iters"][pend[0]])
    for k in ("status", "iters", "polish"):
        assert np.array_equal(seen[0][k][~pend[0]], refs[0][k][~pend[0]]), k
    # call 2's launch carried them one budget further: at least one instance is parked a second time, at iteration 50 or beyond
    again = pend[0] & pend[1]
    assert again.any() and np.all(seen[1]["iters"][again] >= 2 * K) and np.all(refs[0]["iters"][again] > 2 * K), (seen[1]["iters"][pend[1]], refs[0]["iters"][pend[1]])
    # call 3's launch: whoever is still pending has passed iteration 75 through two restores
    third = again & pend[2]
    assert np.all(seen[2]["iters"][third] >= 3 * K)
    print("%s: parked / refused %s; call 1's instances pending behind calls 1, 2, 3: %d, %d, %d" % (tuning, eng.defer_stats(), int(pend[0].sum()), int(again.sum()), int(third.sum())))
    eng.join(st.cuda_stream); torch.cuda.synchronize()
    for j, (w, ref) in enumerate(zip(ws, refs)):
        against_oracle(w, R._host(calls[j][1]), ref, "%s deferred call %d" % (tuning, j + 1))
    eng.close()
