"""GPU: race snapshot, restore and clone (lpvmpc_race_snapshot / _restore / _clone; include/lpvmpc.h, "Race snapshot, restore and
clone").  Every comparison is bit for bit (integers exactly, doubles through their 64-bit patterns, NaN matching NaN).  Fleets,
configurations C0 / C1 / C2 and the read-backs compared: tests/_race_snapshot.py.  The fork tick T0 = 14 falls among the lap events,
so a snapshot holds lap-0 vehicles, vehicles on their event tick and racing vehicles at different planner phases; each test asserts
that at B = 67, and that three quarters of the fleet is alive when it ends.
  1. a race restored to its own snapshot repeats the 20 ticks it ran after it;
  2. a freshly initialised race of the same bindings but another history, restored from the blob, runs the source's future: the test
     that finds a state array missing from the inventory;
  3. taking snapshots changes nothing;
  4. clone(src) equals RaceSnapshot.take(src), the host definition, on every array;
  5. a clone lives its source's future (C0: homogeneous, no noise);
  6. a clone draws its own gusts, and a restore reproduces them;
  7. refusals leave the race as it was; a snapshot is allowed while recording and leaves the trace alone."""
import numpy as np
import pytest

from tests import _race_snapshot as S

pytestmark = pytest.mark.gpu

T0, AFTER = S.T0, 20
E_ARG = -1


def vacuity_at_fork(snap, B):
    n0, ne, nr = S.three_phases(snap)
    print("fork tick %d, B=%d: %d in lap 0, %d on their event tick, %d racing" % (snap.ticks, B, n0, ne, nr))
    if B == 67:
        assert n0 >= 1 and ne >= 1 and nr >= 1, (n0, ne, nr)


def vacuity_at_end(o, B):
    n = S.alive_count(o)
    print("end: %d of %d alive, phases %s" % (n, B, np.bincount(o["phase"], minlength=4).tolist()))
    if B == 67:
        assert 4 * n >= 3 * B, (n, B)


# ---- 1. restore into the same race ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,B", [("C0", 67), ("C1", 67), ("C2", 67), ("C1", 5), ("C0", 1)])
def test_restore_into_the_same_race(cfg, B):
    f = S.fleet(cfg, B)
    f.run(T0)
    snap = f.snapshot()
    assert snap.ticks == T0 and snap.B == B
    vacuity_at_fork(snap, B)
    first = S.run_reading(f, cfg, AFTER)
    f.restore(snap)
    assert f.state()["ticks"] == T0
    again = S.run_reading(f, cfg, AFTER)
    S.assert_reads_equal(first, again, (cfg, B))
    S.snaps_equal(snap, type(snap).from_bytes(snap.to_bytes()), "blob")
    vacuity_at_end(again[-1], B)
    f.close()


# ---- 2. restore into a fresh race ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["C0", "C1"])
def test_restore_into_a_fresh_race(cfg):
    B = 67
    a = S.fleet(cfg, B)
    a.run(T0)
    blob = a.path.race_snapshot(raw=True)
    vacuity_at_fork(a.snapshot(), B)
    want = S.run_reading(a, cfg, AFTER)
    a.close()
    maps, of = S.maps_of(cfg, B)
    b = S.fleet(cfg, B, plant0=S.other_starts(maps, of, B), half_track0=0)      # same bindings, another history
    b.run(3)
    before = S.reads(b, cfg)
    assert not S.same(before["plant"], want[0]["plant"])
    b.path.race_restore(blob)
    got = S.run_reading(b, cfg, AFTER)
    S.assert_reads_equal(want, got, cfg)
    vacuity_at_end(got[-1], B)
    b.close()


# ---- 3. snapshot is read-only --------------------------------------------------------------------------------------------------
def test_snapshot_changes_nothing():
    cfg, B, n = "C1", 67, T0 + AFTER
    a, b = S.fleet(cfg, B), S.fleet(cfg, B)
    ra, rb = [], []
    for t in range(n):
        ra += S.run_reading(a, cfg, 1)
        rb += S.run_reading(b, cfg, 1)
        if t % 5 == 4:
            s = b.snapshot()
            assert s.ticks == t + 1
            if t + 1 == 15:
                vacuity_at_fork(s, B)
    S.assert_reads_equal(ra, rb, "snapshotted every 5 ticks", other_race=True)
    vacuity_at_end(rb[-1], B)
    a.close(); b.close()


# ---- 4. clone against the host definition --------------------------------------------------------------------------------------
def src_maps(B, of):
    """identity, one swap, a 3-cycle, everything from vehicle 0, a random map; with tracks, kept inside each track."""
    ident = np.arange(B, dtype=np.int32)
    groups = [ident] if of is None else [ident[of == t] for t in np.unique(of)]
    out = [("identity", ident.copy())]
    swap, cyc, zero, rand = ident.copy(), ident.copy(), ident.copy(), ident.copy()
    rng = np.random.default_rng(B)
    for g in groups:
        if len(g) >= 2:
            swap[g[0]], swap[g[-1]] = g[-1], g[0]
        if len(g) >= 3:
            cyc[g[0]], cyc[g[1]], cyc[g[2]] = g[1], g[2], g[0]
        zero[g] = g[0]
        rand[g] = g[rng.integers(0, len(g), len(g))]
    return out + [("swap", swap), ("3-cycle", cyc), ("all from the first", zero), ("random", rand)]


@pytest.mark.parametrize("B", S.SIZES)
@pytest.mark.parametrize("cfg", ["C0", "C1", "C2"])
def test_clone_is_take(cfg, B):
    f = S.fleet(cfg, B)
    f.run(T0)
    _, of = S.maps_of(cfg, B)
    vacuity_at_fork(f.snapshot(), B)
    for name, src in src_maps(B, of):
        before = f.snapshot()
        moved = f.clone(src)
        assert moved == int(np.sum(src != np.arange(B))), name
        after = f.snapshot()
        S.snaps_equal(after, before.take(src), (cfg, B, name))
        assert after.ticks == before.ticks == T0
    f.restore(before)
    f.run(1)                                                   # the race goes on
    o = S.run_reading(f, cfg, 2)[-1]
    assert o["ticks"] == T0 + 3
    vacuity_at_end(o, B)
    f.close()


# ---- 5. a clone lives its source's future ---------------------------------------------------------------------------------------
def test_clone_lives_its_sources_future():
    cfg, B = "C0", 67
    rng = np.random.default_rng(3)
    src = rng.integers(0, B, B).astype(np.int32)
    src[:8] = np.arange(8)                                     # some stay
    a, twin = S.fleet(cfg, B), S.fleet(cfg, B)
    a.run(T0); twin.run(T0)
    vacuity_at_fork(a.snapshot(), B)
    assert a.clone(src) == int(np.sum(src != np.arange(B))) >= B // 2
    got, want = S.run_reading(a, cfg, 25), S.run_reading(twin, cfg, 25)
    S.assert_reads_equal(got, want, "clone vs twin", idx_a=np.arange(B), idx_b=src, other_race=True)
    vacuity_at_end(got[-1], B)
    a.close(); twin.close()


# ---- 6. a clone draws its own ---------------------------------------------------------------------------------------------------
def test_clone_draws_its_own():
    cfg, B = "C1", 67
    f = S.fleet(cfg, B)
    f.run(T0)
    vacuity_at_fork(f.snapshot(), B)
    assert f.clone(np.zeros(B, np.int32)) == B - 1
    start = f.snapshot()
    assert all(S.same(v, np.repeat(v[:1], B, axis=0)) for v in start.arrays.values())      # B copies of vehicle 0
    first = S.run_reading(f, cfg, 10)
    g = first[-1]["dist_state"]
    assert np.all(g[:, 3] == g[0, 3]) and g[0, 3] > 0                       # the same tick count ...
    differ = np.any(g[1:, 0:3] != g[0, 0:3], axis=1)
    print("clones whose gust words differ from vehicle 0's after 10 ticks: %d of %d" % (differ.sum(), B - 1))
    assert np.all(differ)                                                   # ... and other draws in every other slot
    f.restore(start)
    again = S.run_reading(f, cfg, 10)
    S.assert_reads_equal(first, again, "restored clones")
    vacuity_at_end(again[-1], B)
    f.close()


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------
def refused(call, *words):
    import lpvmpc
    with pytest.raises(lpvmpc.LpvMpcError) as e:
        call()
    assert e.value.code == E_ARG and all(w in str(e.value) for w in words), str(e.value)


def test_refusals_leave_the_race_as_it_was():
    import lpvmpc
    B = 67
    c2, c1, c0, small = S.fleet("C2", B), S.fleet("C1", B), S.fleet("C0", B), S.fleet("C1", 5)
    for f in (c2, c1, c0, small):
        f.run(T0)
    vacuity_at_fork(c1.snapshot(), B)
    blob0, blob5, blob1 = c0.path.race_snapshot(raw=True), small.path.race_snapshot(raw=True), c1.path.race_snapshot(raw=True)
    ident = np.arange(B, dtype=np.int32)

    def unchanged(f, call, *words):
        before = f.snapshot()
        refused(call, *words)
        S.snaps_equal(f.snapshot(), before, words)

    for bad in (B, -1):
        src = ident.copy(); src[3] = 5; src[40] = bad                       # a valid move in front of the bad index
        unchanged(c1, lambda: c1.clone(src), "lpvmpc_race_clone", "outside")
    src = ident.copy(); src[2] = 4; src[10] = 11                            # 10 and 11 are on different tracks
    unchanged(c2, lambda: c2.clone(src), "lpvmpc_race_clone", "track")
    unchanged(c1, lambda: c1.path.race_restore(blob0), "lpvmpc_race_restore", "snapshot's")      # (C0 differs in sd and in the feature word)
    small.disturb(None)                                                     # the same race without its disturbances: the feature word alone
    unchanged(small, lambda: small.path.race_restore(blob5), "lpvmpc_race_restore", "feature word")
    unchanged(c1, lambda: c1.path.race_restore(blob5), "lpvmpc_race_restore", "B = 5")
    for n in (0, 40, 64, len(blob1) // 2, len(blob1) - 1):
        unchanged(c1, lambda: c1.path.race_restore(blob1[:n]), "lpvmpc_race_restore")
    unchanged(c1, lambda: c1.path.race_restore(b"LPVRACF\0" + blob1[8:]), "magic")
    # an engine without a race
    e = lpvmpc.BatchedSolver("controller", 20, 1 / 30.0, np.eye(6), np.eye(2), np.ones(2), track=S.lshape().PointAndTangent)
    for call in (e.race_snapshot, lambda: e.race_restore(blob1), lambda: e.race_clone(ident)):
        refused(call, "race_init first")
    import ctypes as C
    n = C.c_int64(0)
    for rc in (e._lib.lpvmpc_race_snapshot_size(e._h, C.byref(n)), e._lib.lpvmpc_race_snapshot(e._h, None, 0),
               e._lib.lpvmpc_race_restore(e._h, None, 0), e._lib.lpvmpc_race_clone(e._h, None, None)):
        assert rc == E_ARG and b"call lpvmpc_race_init first" in e._lib.lpvmpc_last_error(e._h)
    e.close()
    # the recorder: restore and clone are refused while it is attached, a snapshot is not and leaves the trace alone
    twin = S.fleet("C1", B)
    twin.run(T0)
    c1.record(8); twin.record(8)
    c1.run(3); twin.run(3)
    unchanged(c1, lambda: c1.restore(c1.snapshot()), "lpvmpc_race_restore", "recorder", "capacity 0")
    unchanged(c1, lambda: c1.clone(np.zeros(B, np.int32)), "lpvmpc_race_clone", "recorder", "capacity 0")
    c1.run(3); twin.run(3)
    ta, tb = c1.trace(), twin.trace()
    assert ta["total"] == tb["total"] == 6
    for k, v in ta.items():
        if isinstance(v, np.ndarray):
            assert S.same(v, tb[k]), ("trace", k)
    c1.record(0)
    assert c1.clone(np.zeros(B, np.int32)) == B - 1                         # stopped: allowed again
    c1.restore(blob1)
    vacuity_at_end(S.run_reading(c1, "C1", 2)[-1], B)
    for f in (c2, c1, c0, small, twin):
        f.close()
