"""CPU: the host side of the warm-start tests (tests/test_gpu_warm_start.py).

  * tests/_warm_ref.py shift_state, the plain-numpy restatement of the documented shift rule, on labelled vectors (every row and
    variable kind, the pinned-steering rows) and against the C tick's own shift (oracle/lpv_ref.c oracle_ctrl_tick_batch).
  * oracle/osqp_ref.py tick_batch_qp(warm=...): the general path's warm start reproduces the C tick's on a controller batch, both
    modes; a zero warm start is the cold solve, word for word.
  * The robust set (tests/golden/warm_start/robust.npz): regenerates to itself, and at least three quarters of every (workload,
    mode, tick) are robust."""
import json
import os

import numpy as np
import pytest

from oracle import osqp_ref as O
from tests import _warm_ref as WR
from tests import test_gpu_settings as G


def _labels(kind, N, d):
    """z and y whose words name their (block, stage, component): 1000 block + 10 stage + component."""
    nx, nz, m = WR.dims(kind, N, d)
    blk = lambda b, n, c: (1000.0 * b + 10.0 * np.arange(n)[:, None] + np.arange(c)[None, :]).reshape(-1)
    z = np.concatenate([blk(1, N + 1, nx), blk(2, N, 2)])
    if kind == "controller":
        y = np.concatenate([blk(3, N, 2), blk(4, N, 4), blk(5, N + 1, nx), 6000.0 + 10.0 * np.arange(d)])
    else:
        y = np.concatenate([blk(5, N + 1, nx), blk(7, N + 1, nx), blk(8, N, 2)])
    assert z.size == nz and y.size == m
    return z[None], y[None]


@pytest.mark.parametrize("kind,N,d", [("controller", 8, 0), ("controller", 13, 0), ("controller", 20, 3), ("controller", 9, 8),
                                      ("controller", 10, 1), ("planner", 8, 0), ("planner", 25, 0), ("planner", 40, 0)])
def test_shift_state_moves_every_word_by_one_stage(kind, N, d):
    """Every word of the shifted state names the stage behind its own; the last stage that exists for its kind is kept: states,
    dynamics rows and the planner's state-box rows to N, inputs and every other box row to N - 1; the last pin starts at 0."""
    z, y = _labels(kind, N, d)
    z2, y2 = WR.shift_state(kind, N, d, z, y)
    n_pin = 0
    for a, a2 in ((z[0], z2[0]), (y[0], y2[0])):
        for v, v2 in zip(a, a2):
            b, k, c = int(v) // 1000, (int(v) % 1000) // 10, int(v) % 10
            if b == 6:                                             # pin of stage k: the pin of stage k + 1; stage d has none
                assert v2 == (v + 10.0 if k < d - 1 else 0.0), (v, v2)
                n_pin += 1
                continue
            last = N if b in (1, 5, 7) else N - 1
            assert v2 == 1000.0 * b + 10.0 * min(k + 1, last) + c, (v, v2)
    assert n_pin == d


def test_general_path_warm_start_matches_the_c_tick():
    """At d = 0 on a controller batch, tick_batch_qp(warm=shift_state(...)) has the status and iteration count of the C tick
    ctrl_tick_batch(warm=r0, shift=True) on every instance (mode 2), and the unshifted state those of shift=False (mode 1).  Both
    start from the C tick's own (z, y) of the first tick."""
    kind, w = G.workload("ctrl20")
    N = int(w["N"])
    r0 = O.ctrl_tick_batch(w, nthreads=WR.NTHREADS)
    r0["polish"] = np.zeros_like(r0["status"])
    w2 = WR.next_inputs(w, kind, r0)
    cold = O.ctrl_tick_batch(w2, nthreads=WR.NTHREADS)
    for mode in WR.MODES:
        c = O.ctrl_tick_batch(w2, nthreads=WR.NTHREADS, warm=r0, shift=mode == 2)
        p = O.tick_batch_qp(w2, kind, nthreads=WR.NTHREADS, warm=WR.warm_state(r0, kind, N, 0, mode))
        assert np.array_equal(p["status"], c["status"]) and np.array_equal(p["iters"], c["iters"]), (mode, np.nonzero(p["iters"] != c["iters"])[0])
        assert np.any(c["iters"] != cold["iters"]), mode           # the warm start is seen at all
    s1 = O.ctrl_tick_batch(w2, nthreads=WR.NTHREADS, warm=r0, shift=False)
    s2 = O.ctrl_tick_batch(w2, nthreads=WR.NTHREADS, warm=r0, shift=True)
    assert np.any(s1["iters"] != s2["iters"]) or float(np.max(np.abs(s1["z"] - s2["z"]))) > 0.0     # and so is the shift


@pytest.mark.parametrize("name", ["ctrl20d3", "plan20"])
def test_zero_warm_start_is_the_cold_solve(name):
    kind, w = G.workload(name)
    _, nz, m = WR.dims(kind, int(w["N"]), WR.delay_of(w, kind))
    B = w["x0"].shape[0]
    cold = G.oracle(name, None)
    zero = O.tick_batch_qp(w, kind, nthreads=WR.NTHREADS, qps=G._QPS[name], warm=(np.zeros((B, nz)), np.zeros((B, m))))
    for k in ("status", "iters", "polish", "z", "y", "resid"):
        assert np.array_equal(zero[k], cold[k], equal_nan=cold[k].dtype.kind == "f"), k


def test_an_instance_without_a_solution_leaves_zeros():
    """saved_state: a PRIMAL INFEASIBLE instance (the planner workloads have some) contributes zeros, every other one its point."""
    kind, w = G.workload("plan20")
    r = G.oracle("plan20", None)
    z, y = WR.saved_state(r)
    none = np.isin(r["status"], WR.NO_SOLUTION)
    assert none.sum() >= 1 and (~none).sum() >= 1
    assert not z[none].any() and not y[none].any()
    assert np.array_equal(z[~none], r["z"][~none]) and np.array_equal(y[~none], r["y"][~none])


@pytest.mark.parametrize("name", ["ctrl8", "ctrl13"])
def test_fine_settings_tell_an_unshifted_dual_apart(name):
    """What test_warm_ticks_at_single_iteration_resolution (tests/test_gpu_warm_start.py) can see, shown on the oracle: under
    FINE_SETTINGS the oracle's RCM order passes check_resid against its stage-wise order at the device's bounds, while a warm start
    whose dynamics duals were left unshifted -- which changes no status, iteration count or polish flag at these horizons -- does
    not."""
    from tests import _tolerance as T
    C, st, mode, tick = WR.FINE_CASE, WR.FINE_SETTINGS, 2, 2
    kind, w = WR.scenario_workload(name, mode, tick, C)
    N, d = int(w["N"]), WR.delay_of(w, kind)
    ref, qps = WR.scenario_ref(name, mode, tick, case=C), WR.scenario_qps(name, mode, tick, C)
    rcm = O.tick_batch_qp(w, kind, settings=st, nthreads=WR.NTHREADS, qps=qps, warm=WR.scenario_warm(name, mode, tick, C), order="rcm")
    rep = T.check_resid(w, kind, rcm, ref, yard=T.RESID_BOUNDS, settings=st, qps=qps, late_rule=False)
    assert rep["counts"]["B"] == w["x0"].shape[0] and not rep["left_out"], rep["counts"]
    z0, y0 = WR.saved_state(WR.scenario_ref(name, mode, tick - 1, case=C))
    z, y = WR.shift_state(kind, N, d, z0, y0)
    dyn = slice(6 * N, 6 * N + (N + 1) * 6)
    y[:, dyn] = y0[:, dyn]
    mut = O.tick_batch_qp(w, kind, settings=st, nthreads=WR.NTHREADS, qps=qps, warm=(z, y))
    print("%s: unshifted dynamics duals change (status, iterations, polish) on %d instances" % (name, int((WR.key(mut) != WR.key(ref)).any(axis=1).sum())))
    with pytest.raises(AssertionError):
        T.check_resid(w, kind, mut, ref, yard=T.RESID_BOUNDS, settings=st, qps=qps, late_rule=False)


def test_robust_set_regenerates_to_itself():
    """The committed masks are what tests/_warm_ref.py computes today, the key set is the manifest's, and at least three quarters
    of every (workload, mode, tick) are robust (measured shares: tests/golden/warm_start/make_robust.py)."""
    got = WR.compute_robust()
    with np.load(WR.FIXTURE) as f:
        have = {k: f[k] for k in f.files}
    man = json.load(open(os.path.join(os.path.dirname(WR.FIXTURE), "MANIFEST.json")))["robust.npz"]
    assert sorted(have) == sorted(got) == sorted(man)
    for k, v in got.items():
        assert have[k].dtype == np.uint8 and man[k] == {"dtype": "uint8", "shape": list(v.shape)}, k
        assert np.array_equal(have[k].astype(bool), v), (k, np.nonzero(have[k].astype(bool) != v)[0])
        print("%s: %d of %d robust" % (k, int(v.sum()), v.size))
        assert v.mean() >= WR.ROBUST_SHARE, (k, v.mean())
