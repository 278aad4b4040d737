"""GPU: straggler deferral with riders.  With "defer_budget" > 0 a deferred call enqueues no resume pass of its own: whatever the
handle's earlier calls left parked continues, one budget of iterations, in workgroups of the NEXT deferred call's main launch (the
riders; grid pool + B), and lpvmpc_join finishes what is left.  A parked instance therefore advances with the handle's next
deferred call or at the join -- and nothing about the results changes: every case here runs with "defer_tail" 0 (the same kernel
continues the entries) and compares every output word with the plain solve of the same batch, bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PENDING = -11


def _dev_call(torch, eng, w, B, planner, stream=None):
    dev = torch.device("cuda", 0)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    N, nx = w["N"], (5 if planner else 6)
    ins = dict(x0=t(w["x0"]), u_prev=t(w["u_prev"]), vel=t(w["vel_ref"]), curv=t(w["curv_s"]), u_old=t(w["u_old"]), mey=t(w["max_ey"]))
    with torch.cuda.stream(stream):              # the fills are ordered in front of the call on its own stream (None: the current one)
        o = dict(xPred=torch.full((B, N + 1, nx), -7.0, dtype=torch.float64, device=dev), uPred=torch.full((B, N, 2), -7.0, dtype=torch.float64, device=dev),
                 status=torch.zeros(B, dtype=torch.int32, device=dev), iters=torch.zeros(B, dtype=torch.int32, device=dev),
                 resid=torch.zeros((B, 4), dtype=torch.float64, device=dev), polish=torch.zeros(B, dtype=torch.int32, device=dev))
    eng.solve_dev(B, ins["x0"], ins["u_prev"], ins["vel"], ins["curv"], ins["u_old"], ins["mey"], o["xPred"], o["uPred"], o["status"], o["iters"],
                  o["resid"], o["polish"], cf_new=w["cf_new"], lap=w["lap"], stream=0 if stream is None else stream.cuda_stream)
    return ins, o


def _host(o):
    return {k: v.cpu().numpy() for k, v in o.items()}


def _same(a, b):
    for k in ("status", "iters", "polish"):
        assert np.array_equal(a[k], b[k]), (k, np.nonzero(a[k] != b[k])[0][:8])
    for k in ("xPred", "uPred", "resid"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def _plain(torch, w, B, planner=False):
    from lpvmpc import workloads
    eng = workloads.make_solver(w); eng.reserve(B)
    _, o = _dev_call(torch, eng, w, B, planner); torch.cuda.synchronize()
    ref = _host(o); eng.close()
    return ref


def _deferred(w, B, K=100, budget=100, pool=None):
    from lpvmpc import workloads
    eng = workloads.make_solver(w); eng.reserve(B)
    if pool is not None:
        eng.set_option("defer_pool", pool)
    eng.set_option("defer_after", K); eng.set_option("defer_budget", budget); eng.set_option("defer_tail", 0)
    return eng


@pytest.mark.parametrize("seed", [3, 16])
def test_parked_instances_ride_in_the_next_call(seed):
    """Calls 1 and 2 (two different batches) on one stream, defer_after 100 / defer_budget 100.  After call 1 alone nothing has
    continued: every instance beyond 100 iterations is LPVMPC_PENDING with iters <= 100.  Call 2's launch carries them: each has
    finished or is parked again exactly one budget further (the checks fall on multiples of 25; a rider that found the pool full
    at its check goes on in place and is further still).  After the join every word of both calls equals the plain solves."""
    import torch
    from lpvmpc import workloads
    B, K, budget = 1024, 100, 100
    w1 = workloads.controller_batch(B, N=20, seed=seed)
    w2 = workloads.controller_batch(B, N=20, seed=seed + 100)
    ref1, ref2 = _plain(torch, w1, B), _plain(torch, w2, B)
    assert ref1["iters"].max() >= 1000 and np.sum(ref1["iters"] > K) >= 4 and np.sum(ref2["iters"] > K) >= 4
    eng = _deferred(w1, B, K, budget)
    st = torch.cuda.Stream()
    keep1, o1 = _dev_call(torch, eng, w1, B, False, stream=st)
    torch.cuda.synchronize()
    h1 = _host(o1)
    late = ref1["iters"] > K
    assert np.all(h1["status"][late] == PENDING) and np.all(h1["iters"][late] <= K), (h1["status"][late], h1["iters"][late])
    assert not np.any(h1["status"][~late] == PENDING)
    for k in ("status", "iters", "uPred"):
        assert np.array_equal(h1[k][~late], ref1[k][~late], equal_nan=True), k
    parked1, refused1 = eng.defer_stats()
    assert parked1 == int(late.sum())
    keep2, o2 = _dev_call(torch, eng, w2, B, False, stream=st)
    torch.cuda.synchronize()
    h1b, h2 = _host(o1), _host(o2)
    refused2 = eng.defer_stats()[1] - refused1
    idx = np.nonzero(late)[0]
    still = idx[h1b["status"][idx] == PENDING]
    done = idx[h1b["status"][idx] != PENDING]
    print("seed %d: %d parked by call 1, %d finished as riders of call 2, %d parked again; %d refusals in call 2"
          % (seed, len(idx), len(done), len(still), refused2))
    assert len(still) >= 1 and len(done) >= 1                          # both outcomes occur in these batches
    if refused2 == 0:
        assert np.array_equal(h1b["iters"][still], h1["iters"][still] + budget), (h1["iters"][still], h1b["iters"][still])
        assert np.all(ref1["iters"][done] <= h1["iters"][done] + budget)    # finished within the budget, not beyond it
    else:
        assert np.all(h1b["iters"][still] >= h1["iters"][still] + budget)
    assert np.all(ref1["iters"][still] > h1["iters"][still] + budget)       # none of them was due within the budget
    for k in ("status", "iters", "polish", "xPred", "uPred", "resid"):
        assert np.array_equal(h1b[k][done], ref1[k][done], equal_nan=True), k
    late2 = ref2["iters"] > K
    assert np.all(h2["status"][late2] == PENDING) and np.all(h2["iters"][late2] <= K) and not np.any(h2["status"][~late2] == PENDING)
    eng.join(st.cuda_stream); torch.cuda.synchronize()
    _same(_host(o1), ref1)
    _same(_host(o2), ref2)
    eng.close()


def test_small_pool_with_riders_present():
    """A pool of 4 entries: launches 2 and 3 find riders in it and have many more candidates than room.  The surplus instances --
    new ones and riders whose entry could not be renewed -- finish inside the launch that holds them; results unchanged."""
    import torch
    from lpvmpc import workloads
    B = 1024
    ws = [workloads.controller_batch(B, N=20, seed=s) for s in (3, 16, 103)]
    refs = [_plain(torch, w, B) for w in ws]
    assert all(int(np.sum(r["iters"] > 100)) > 8 for r in refs)
    eng = _deferred(ws[0], B, 100, 100, pool=4)
    st = torch.cuda.Stream()
    outs = [_dev_call(torch, eng, w, B, False, stream=st) for w in ws]
    torch.cuda.synchronize()
    for (_, o), r in zip(outs, refs):
        assert int(np.sum(_host(o)["status"] == PENDING)) <= 4
    parked, refused = eng.defer_stats()
    assert parked >= 4 and refused > 0, (parked, refused)
    eng.join(st.cuda_stream); torch.cuda.synchronize()
    for (_, o), r in zip(outs, refs):
        _same(_host(o), r)
    eng.close()


def test_calls_alternating_between_two_streams():
    """The pools follow the handle from stream to stream through its hand-over event: launch j + 1, on the other stream, reads as
    riders what launch j parked, without any synchronisation by the caller."""
    import torch
    from lpvmpc import workloads
    B = 1024
    ws = [workloads.controller_batch(B, N=20, seed=s) for s in (3, 16)]
    refs = [_plain(torch, w, B) for w in ws]
    eng = _deferred(ws[0], B, 100, 100)
    sts = [torch.cuda.Stream(), torch.cuda.Stream()]
    keep = []
    for j in range(8):
        keep.append((j % 2, _dev_call(torch, eng, ws[j % 2], B, False, stream=sts[j % 2])))
        if j == 1:          # call 0's stragglers (stream 0) rode in call 1 (stream 1): finished, or parked one budget further
            sts[1].synchronize()
            h0 = _host(keep[0][1][1])
            late = refs[0]["iters"] > 100
            pend = h0["status"] == PENDING
            assert np.all(h0["iters"][late & pend] >= 200) and np.all(late[pend]), (h0["iters"][late], h0["status"][late])
            fin = late & ~pend
            assert fin.any() and np.array_equal(h0["iters"][fin], refs[0]["iters"][fin]) and np.array_equal(h0["uPred"][fin], refs[0]["uPred"][fin], equal_nan=True)
    eng.join(sts[0].cuda_stream); torch.cuda.synchronize()
    for i, (_, o) in keep:
        _same(_host(o), refs[i])
    eng.close()


def test_masked_call_with_parked_instances_present():
    """lpvmpc_solve_batch_masked on a handle that holds parked instances of an earlier deferred call: the mask applies to the new
    instances only -- masked-out rows untouched byte for byte, flagged rows equal to the plain solve -- and the earlier call's parked
    instances are continued to their end (the synchronous call joins)."""
    import torch
    from lpvmpc import workloads
    B = 1024
    w1 = workloads.controller_batch(B, N=20, seed=3)
    w2 = workloads.controller_batch(B, N=20, seed=16)
    ref1 = _plain(torch, w1, B)
    plain = workloads.make_solver(w2)
    args = (w2["x0"], w2["u_prev"], w2["vel_ref"], w2["curv_s"], w2["u_old"], None, w2["cf_new"], w2["lap"])
    full = plain.solve(*args); plain.close()
    eng = _deferred(w1, B, 100, 100)
    keep, o1 = _dev_call(torch, eng, w1, B, False)
    torch.cuda.synchronize()
    assert np.sum(_host(o1)["status"] == PENDING) == np.sum(ref1["iters"] > 100) > 0
    act = (np.random.default_rng(1).random(B) < 0.4).astype(np.int32)
    act[np.argmax(full["iters"])] = 1                                    # the batch's longest runner is among the flagged
    sentinel = {k: np.full_like(v, 7) for k, v in full.items()}
    out = {k: v.copy() for k, v in sentinel.items()}
    eng.solve_batch_masked(act, *args[:5], cf_new=w2["cf_new"], lap=w2["lap"], out=out)
    on = act != 0
    for k in full:
        assert np.array_equal(out[k][on], full[k][on], equal_nan=True), k
        assert out[k][~on].tobytes() == sentinel[k][~on].tobytes(), k
    torch.cuda.synchronize()
    _same(_host(o1), ref1)
    eng.close()


def test_planner_n20_with_riders():
    """The planner at N = 20 (mean 640 iterations, a fifth of the batch at max_iter): three calls whose long runners ride through
    the following launches, parked up to forty times each."""
    import torch
    from lpvmpc import workloads
    B = 512
    ws = [workloads.planner_batch(B, N=20, seed=s) for s in (2, 5)]
    refs = [_plain(torch, w, B, True) for w in ws]
    assert np.sum(refs[0]["iters"] > 300) > 50 and refs[0]["iters"].max() == 4000
    eng = _deferred(ws[0], B, 100, 100, pool=1024)
    st = torch.cuda.Stream()
    keep = [(j % 2, _dev_call(torch, eng, ws[j % 2], B, True, stream=st)) for j in range(3)]
    torch.cuda.synchronize()
    assert np.any(_host(keep[0][1][1])["status"] == PENDING)
    eng.join(st.cuda_stream); torch.cuda.synchronize()
    for i, (_, o) in keep:
        _same(_host(o), refs[i])
    eng.close()


@pytest.mark.parametrize("budget", [0, -1])
def test_budgets_zero_and_minus_one_behave_as_before(budget):
    """defer_budget 0: a pass to completion behind every call -- nothing is pending once the stream is idle, without a join.
    defer_budget -1: no pass and no riders -- what two calls parked stays exactly as they left it until lpvmpc_join.
    lpvmpc_defer_stats: every instance beyond defer_after iterations parked once, nothing refused (a pool entry for each)."""
    import torch
    from lpvmpc import workloads
    B, K = 1024, 100
    ws = [workloads.controller_batch(B, N=20, seed=s) for s in (3, 16)]
    refs = [_plain(torch, w, B) for w in ws]
    n_late = [int(np.sum(r["iters"] > K)) for r in refs]
    eng = _deferred(ws[0], B, K, budget, pool=1024)
    assert eng.defer_stats() == (0, 0)
    st = torch.cuda.Stream()
    outs = [_dev_call(torch, eng, w, B, False, stream=st) for w in ws]
    torch.cuda.synchronize()
    hs = [_host(o) for _, o in outs]
    assert eng.defer_stats() == (sum(n_late), 0)
    if budget == 0:
        for h, r in zip(hs, refs):
            _same(h, r)
    else:
        for h, r in zip(hs, refs):
            late = r["iters"] > K
            assert np.all(h["status"][late] == PENDING) and np.all(h["iters"][late] == K) and not np.any(h["status"][~late] == PENDING)
    eng.join(st.cuda_stream); torch.cuda.synchronize()
    for (_, o), r in zip(outs, refs):
        _same(_host(o), r)
    assert eng.defer_stats() == (sum(n_late), 0)
    eng.close()
