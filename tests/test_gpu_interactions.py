"""GPU: the interactions (lpvmpc_race_interactions / _read, lpvmpc_interaction_step_batch; BatchedSolver.race_interactions /
race_interactions_read / interaction_step, RaceFleet.interact / interactions) against the numpy restatement
tests/_interactions_ref.py: crafted single ticks in heats of 1, 2, 5, 65 and 256 members, a scripted sequence with the carry passed
back in, a race with the interactions attached against the host replay, the all-off and detached races, both orders of attaching
disturbances and interactions, reruns, the refusals, and one physical check of the slipstream.  Decisions, counters and who was
written are held exactly, values to 1e-11 relative to max(1, |value|) -- the bar the device plant and transforms hold against their
oracle -- and word for word where every heading is exactly 0."""
import numpy as np
import pytest

from tests import _interactions_cases as K
from tests import _interactions_ref as R

pytestmark = pytest.mark.gpu

KV = 0          # kernel_variant fixed on every handle: kernel routes may depend on B
TOL = 1e-11
SMALL = dict(half_length=0.2, half_width=0.1)      # footprints that fit side by side on a track of half width 0.3


def lshape():
    import lpvmpc
    return lpvmpc.Map("L_shape", 0.2)


def batch_engine():
    import lpvmpc
    return lpvmpc.BatchedSolver("controller", 20, 1 / 30.0, np.eye(6), np.eye(2), np.ones(2), track=lshape().PointAndTangent)


def engines(mp):
    from tests.test_gpu_race_record import engines as E
    return E(mp)


def close(*es):
    for e in es:
        e.close()


def same(a, b):
    return np.asarray(a).shape == np.asarray(b).shape and np.asarray(a).tobytes() == np.asarray(b).tobytes()


def close_to(a, b, what):
    a, b = np.asarray(a, float), np.asarray(b, float)
    assert np.array_equal(np.isnan(a), np.isnan(b)), what
    ok = ~np.isnan(a)
    err = float(np.max(np.abs(a[ok] - b[ok]) / np.maximum(1.0, np.abs(b[ok])))) if ok.any() else 0.0
    assert err <= TOL, (what, err)
    return err


def compare(plant, mu, out, carry, sc, ref, exact):
    """A device tick against the restatement's: decisions, counters and who was written exactly; values to TOL, or word for word."""
    from lpvmpc import _ffi
    for k in R.I32_NAMES:
        assert np.array_equal(out[k], ref[k]), k
    assert same(plant[~ref["written"]], sc["plant"][~ref["written"]])       # untouched vehicles keep their rows bit for bit
    assert same(plant[:, [4, 5, 6, 7]], sc["plant"][:, [4, 5, 6, 7]])        # ax, ay, yaw, psiDot are nobody's to write
    assert same(mu[~ref["part"]], sc["rows"][~ref["part"], 6])
    worst = 0.0
    if exact:
        assert same(plant, ref["plant"]) and same(mu, ref["mu_live"])
        for k in R.F64_NAMES:
            assert same(out[k], ref[k]), k
    else:
        worst = max(close_to(plant, ref["plant"], "plant"), close_to(mu, ref["mu_live"], "mu_live"))
        for k in R.F64_NAMES:
            worst = max(worst, close_to(out[k], ref[k], k))
    kf, ki = carry["f64"], carry["i32"]
    member = sc["heat"] >= 0
    for c, k in enumerate(_ffi.INTER_CARRY_I32_NAMES):
        assert np.array_equal(ki[c][member], ref["carry"][k][member]), k
    if exact:
        assert same(kf[0][member], ref["carry"]["impulse_total"][member])
    else:
        close_to(kf[0][member], ref["carry"]["impulse_total"][member], "carried impulse_total")
    return worst


@pytest.mark.parametrize("kind", ("general", "aligned"))
@pytest.mark.parametrize("n", K.SIZES)
def test_one_tick_of_crafted_geometry(n, kind):
    """Two heats of n members at the same place (they must not see each other) and three vehicles in no heat on top of them: a
    drafting train, a side-by-side overlap, a nose-to-tail hit, a three-car pile-up, a frozen member and one without a pose, as many
    as fit in n.  "aligned": every heading exactly 0, every output word equal."""
    sc, ref = K.case(n, kind)
    e = batch_engine()
    plant, mu, out, carry = e.interaction_step(sc["heat"], sc["plant"], sc["rows"], 5, nstep=sc["nstep"])
    e.close()
    worst = compare(plant, mu, out, carry, sc, ref, exact=(kind == "aligned"))
    print("interaction tick, heats of %d, %s: margin %.3g, %d hit, %d drafting, worst relative error %.3g" %
          (n, kind, ref["margin"], int(ref["hit"].sum()), int(np.nansum(ref["shelter"] > 0)), worst))
    if n >= 5:
        g0 = np.nonzero(sc["heat"] == 0)[0]
        assert ref["hit"][g0[:3]].tolist() == [1, 1, 1] and ref["hit"][g0[3:5]].tolist() == [0, 0]   # the pile; frozen and pose-less
        assert np.all(ref["impulse"][g0[:3]] > 0)                              # each car of the pile touches the two others
    if n >= 65:
        assert np.nansum(ref["shelter"] > 0) >= 2 * (n - 12) and ref["hit"].sum() == 14
    # the two heats read alike, and a vehicle in no heat reads NaN / -1 / 0
    a, b = np.nonzero(sc["heat"] == 0)[0], np.nonzero(sc["heat"] == 1)[0]
    for k in ("shelter", "mu", "impulse", "hit"):
        assert same(out[k][a], out[k][b]), k
    loose = sc["heat"] < 0
    assert np.all(np.isnan(out["f64"][:, loose])) and np.all(out["leader"][loose] == -1) and np.all(out["first_hit_tick"][loose] == -1)
    assert not out["hit"][loose].any() and not out["hit_ticks"][loose].any() and not out["draft_ticks"][loose].any()


def test_all_off_keeps_every_word():
    sc, _ = K.case(65, "general")
    e = batch_engine()
    plant, mu, out, _ = e.interaction_step(sc["heat"], sc["plant"], sc["rows"], 0, cfg=dict(draft_gain=0.0, contact=0), nstep=sc["nstep"])
    e.close()
    assert same(plant, sc["plant"]) and same(mu, sc["rows"][:, 6])
    assert not out["hit"].any() and np.nansum(out["impulse"]) == 0 and np.nansum(out["shelter"]) > 0


def test_carry_through_a_scripted_sequence():
    """12 ticks of 4 cars: hits start and end twice, a draft is picked up and lost; every counter exact on every tick, and the run
    split over two handles, the carry handed over, equals the one run."""
    rows = np.tile([0.125, 0.125, 1.98, 0.03, 60.0, 60.0, 0.05], (4, 1))
    e, e2 = batch_engine(), batch_engine()
    carry = carry2 = None
    ref_carry = None
    seen = []
    for t in range(K.SCRIPT_TICKS):
        p = K.script(t)
        ref = R.tick(p, rows, K.SCRIPT_HEAT, R.config(), t=t, carry=ref_carry)
        ref_carry = ref["carry"]
        assert ref["margin"] >= K.MARGIN
        plant, mu, out, carry = e.interaction_step(K.SCRIPT_HEAT, p, rows, t, carry=carry)
        compare(plant, mu, out, carry, dict(plant=p, rows=rows, heat=K.SCRIPT_HEAT), ref, exact=True)
        if t == 5:
            carry2 = dict(f64=carry["f64"].copy(), i32=carry["i32"].copy())
        if t > 5:
            plant2, mu2, out2, carry2 = e2.interaction_step(K.SCRIPT_HEAT, p, rows, t, carry=carry2)
            assert same(plant2, plant) and same(out2["f64"], out["f64"]) and same(out2["i32"], out["i32"])
            assert same(carry2["f64"], carry["f64"]) and same(carry2["i32"], carry["i32"])
        seen.append((int(out["hit"][1]), int(out["leader"][2])))
    close(e, e2)
    assert [h for h, _ in seen] == [0, 0, 0, 1, 1, 1, 0, 0, 1, 1, 0, 0]
    assert [l for _, l in seen] == [-1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1]
    assert out["hit_ticks"].tolist() == [5, 5, 0, 0] and out["first_hit_tick"].tolist() == [3, 3, -1, -1]
    assert out["draft_ticks"].tolist() == [0, 12, 6, 0]


# ---- in a race ---------------------------------------------------------------------------------------------------------------------
B, GAP, STAGGER = 8, 0.35, 0.095
HEAT = np.array([0] * 4 + [1] * 4)
CFG = dict(draft_gain=0.5)


def race_setup(mp, stagger=STAGGER, gap=GAP):
    """8 vehicles in two heats of 4, each heat the last four places of a grid of seven (so that 30 ticks pass before the first lap
    event), the rear cars faster; neighbours on the grid overlap sideways at the start."""
    import lpvmpc
    from lpvmpc import interactions as I
    p, _ = I.grid(mp, 7, gap, stagger)
    plant0 = np.vstack([p[3:], p[3:]])
    plant0[:, 2] = np.tile([1.0, 1.1, 1.2, 1.3], 2)
    return plant0, lpvmpc.sample_plant_params(B, 23), lpvmpc.tyre_params(B)


def start(mp, plant0, prow, tyres, heats=True, inter=None, **small):
    path, tt, plan = engines(mp)
    path.race_init(tt, plan, plant0, half_track0=1, laps=3, half_width=mp.halfWidth, slack=mp.slack, plant_params=prow, tyre_params=tyres)
    if heats:
        path.race_heats(HEAT, turns0=np.full(B, -1), **(small or SMALL))
    if inter is not None:
        path.race_interactions(inter)
    return path, tt, plan


def run(path, n, extra=()):
    out = []
    for _ in range(n):
        path.race_tick(1)
        o = path.race_read()
        for name in extra:
            o[name] = getattr(path, name)()
        out.append(o)
    return out


RACE_KEYS = ("plant", "local", "cmd", "phase", "lap", "iters", "status", "plan_iters", "plan_status")


def races_equal(a, b):
    for t, (x, y) in enumerate(zip(a, b)):
        for k in RACE_KEYS:
            assert same(x[k], y[k]), (t, k)


def test_race_with_interactions_matches_the_host_replay():
    """A _tyres race of 8 vehicles in two heats from grid(), the interactions attached at tick 0 with a draft and contact on, one pair
    and more overlapping at the start, 30 lap-0 ticks against the host replay (TyreRaceRef with the interaction applied in front of
    each vehicle's steps): the tyre race's bar, states within 2e-6, equal statuses and iteration counts; the interactions' outputs
    follow the replay's, decisions exactly."""
    mp = lshape()
    plant0, prow, tyres = race_setup(mp)
    T_ = 30
    Ref = R.interacting_race_ref()
    ref = Ref(np.asarray(mp.PointAndTangent, float), plant0, HEAT, R.config(**CFG), half_length=SMALL["half_length"],
              half_width_car=SMALL["half_width"], tyre_params=tyres, plant_params=prow, half_track0=1, laps=3, half_width=mp.halfWidth,
              slack=mp.slack)
    path, tt, plan = start(mp, plant0, prow, tyres, inter=CFG)
    worst = worst_out = 0.0
    hits = drafts = 0
    for t in range(T_):
        path.race_tick(1); ref.tick()
        o, io = path.race_read(), path.race_interactions_read()
        assert np.all(o["phase"] == 0) and np.all(ref.phase == 0), t           # the window: lap 0, nobody finishes or is lost
        for a_, b_ in ((o["plant"], ref.plant), (o["local"], ref.local), (o["cmd"], ref.cmd)):
            worst = max(worst, float(np.max(np.abs(a_ - b_))))
        assert np.array_equal(o["iters"], ref.iters) and np.array_equal(o["status"], ref.status), t
        for k in ("leader", "hit", "hit_ticks", "first_hit_tick", "draft_ticks"):
            assert np.array_equal(io[k], ref.inter[k]), (t, k)
        for k in ("shelter", "mu", "impulse", "impulse_total"):
            worst_out = max(worst_out, float(np.max(np.abs(io[k] - ref.inter[k]))))
        hits += int(io["hit"].sum()); drafts += int((io["shelter"] > 0).sum())
    print("race with interactions vs replay: %d ticks, worst state / command error %.3g, worst output error %.3g, %d hits, %d drafting, "
          "smallest decision margin of the replay %.3g" % (T_, worst, worst_out, hits, drafts, ref.margin))
    assert ref.margin >= 1e-5                                                    # the replay alone, on the CPU
    assert worst <= 2e-6 and worst_out <= 2e-6
    assert io["hit_ticks"].min() >= 4 and hits < B * T_ and drafts >= 3 * T_     # hits start and end; the train drafts
    assert same(path.plant_params_read(), prow)                                  # the caller's rows while attached
    close(path, tt, plan)


def test_all_off_detached_and_reruns():
    """All-off attached equals nothing attached, word for word; a rerun of the attached race is bit-identical; a race detached at tick
    10 equals, from the same snapshot, one that never had the binding; after the detach the live plant table is the started rows."""
    mp = lshape()
    plant0, prow, tyres = race_setup(mp)
    n = 20
    path, tt, plan = start(mp, plant0, prow, tyres)
    plain = run(path, n)
    close(path, tt, plan)
    path, tt, plan = start(mp, plant0, prow, tyres, inter=dict(draft_gain=0.0, contact=0))
    off = run(path, n)
    io = path.race_interactions_read()
    assert same(io["mu"], prow[:, 6]) and not io["hit_ticks"].any() and io["draft_ticks"].sum() > 0
    close(path, tt, plan)
    races_equal(plain, off)
    first = None
    for _ in range(2):
        path, tt, plan = start(mp, plant0, prow, tyres, inter=CFG)
        on = run(path, n, extra=("race_interactions_read",))
        close(path, tt, plan)
        if first is not None:
            races_equal(first, on)
            for x, y in zip(first, on):
                assert same(x["race_interactions_read"]["f64"], y["race_interactions_read"]["f64"])
                assert same(x["race_interactions_read"]["i32"], y["race_interactions_read"]["i32"])
        first = on
    assert not same(first[-1]["plant"], plain[-1]["plant"])                     # and the attached race is another race
    # detached at tick 10: from there on the race that never had the binding, started from the same snapshot
    path, tt, plan = start(mp, plant0, prow, tyres, inter=CFG)
    run(path, 10)
    assert not same(path.race_interactions_read()["mu"], prow[:, 6])            # sheltered words in the live table
    path.race_interactions(detach=True)
    snap = path.race_snapshot()
    assert same(path.plant_params_read(), prow)
    a = run(path, 10)
    close(path, tt, plan)
    path, tt, plan = start(mp, plant0, prow, tyres, heats=False)
    path.race_restore(snap)
    b = run(path, 10)
    close(path, tt, plan)
    races_equal(a, b)


def test_disturbances_and_interactions_in_both_orders():
    """Attach and detach disturbances and interactions in either order: plant_params_read returns the caller's rows throughout, each
    binding keeps the caller's words as its base, and with both detached the race runs on as one that never had either."""
    import lpvmpc
    from lpvmpc import disturbance as D
    mp = lshape()
    plant0, prow, tyres = race_setup(mp)
    rows = D.disturbance_rows(B, patch0=(0.0, float(mp.TrackLength), 0.6))         # a grip patch over the whole lap: Cf, Cr, c_f scaled on every tick
    path, tt, plan = start(mp, plant0, prow, tyres)
    want = run(path, 6)[-1]
    close(path, tt, plan)
    for order in ("dist_first", "inter_first"):
        path, tt, plan = start(mp, plant0, prow, tyres)
        snap = path.race_snapshot()

        def check():
            assert same(path.plant_params_read(), prow) and same(path.tyre_params_read(), tyres), order
        steps = ([lambda: path.set_disturbances(rows), lambda: path.race_interactions(CFG)] if order == "dist_first" else
                 [lambda: path.race_interactions(CFG), lambda: path.set_disturbances(rows)])
        for s in steps:
            s(); check(); path.race_tick(2); check()
        assert not same(path.race_interactions_read()["mu"], prow[:, 6])
        undo = [lambda: path.set_disturbances(None), lambda: path.race_interactions(detach=True)]
        for s in (undo if order == "dist_first" else undo[::-1]):
            s(); check(); path.race_tick(1); check()
        path.race_heats(None)
        path.race_restore(snap)                                                 # back to tick 0 on the live tables as they are now
        path.race_heats(HEAT, turns0=np.full(B, -1), **SMALL)
        got = run(path, 6)[-1]
        for k in RACE_KEYS:
            assert same(got[k], want[k]), (order, k)
        close(path, tt, plan)


def test_refusals_and_lifetime():
    import lpvmpc
    mp = lshape()
    plant0, prow, tyres = race_setup(mp)
    e = batch_engine()
    assert e._lib.lpvmpc_race_interactions(e._h, None) == -1 and e._lib.lpvmpc_race_interactions_read(e._h, None, None) == -1   # no race
    with pytest.raises(lpvmpc.LpvMpcError):
        e.race_interactions()
    e.close()
    # no plant table
    path, tt, plan = engines(mp)
    path.race_init(tt, plan, plant0, half_track0=1, laps=3, half_width=mp.halfWidth, slack=mp.slack)
    path.race_heats(HEAT, **SMALL)
    with pytest.raises(lpvmpc.LpvMpcError, match="plant table"):
        path.race_interactions(CFG)
    close(path, tt, plan)
    path, tt, plan = start(mp, plant0, prow, tyres, heats=False)
    with pytest.raises(lpvmpc.LpvMpcError, match="heats"):
        path.race_interactions(CFG)                                             # no heats
    with pytest.raises(lpvmpc.LpvMpcError):
        path.race_interactions_read()                                           # nothing attached
    path.race_heats(HEAT, turns0=np.full(B, -1), **SMALL)
    path.race_interactions(CFG)
    path.race_tick(3)
    before = path.race_interactions_read()
    from lpvmpc import _ffi
    import ctypes as C
    for word, v in (("draft_gain", 1.5), ("draft_gain", float("nan")), ("wake_length", 0.0), ("wake_half_width", -1.0), ("contact", 2),
                    ("restitution", -0.1), ("push", float("inf"))):
        c = _ffi.default_interaction_config()
        setattr(c, word, v)
        assert path._lib.lpvmpc_race_interactions(path._h, C.byref(c)) == -1, word      # LPVMPC_E_ARG, past the Python checks
    after = path.race_interactions_read()
    assert same(before["f64"], after["f64"]) and same(before["i32"], after["i32"])      # a refused call leaves the binding as it was
    path.race_tick(1)
    assert path.race_interactions_read()["draft_ticks"].max() == 4
    path.race_snapshot()                                                        # works while attached
    path.race_heats(HEAT, turns0=np.full(B, -1), **SMALL)                       # re-attaching the heats drops the interactions
    with pytest.raises(lpvmpc.LpvMpcError):
        path.race_interactions_read()
    assert same(path.plant_params_read(), prow)
    path.race_interactions(CFG)
    path.race_tick(2)
    path.race_heats(None)                                                       # and so does detaching them
    with pytest.raises(lpvmpc.LpvMpcError):
        path.race_interactions_read()
    assert same(path.plant_params_read(), prow)
    path.race_tick(1)
    close(path, tt, plan)
    e = batch_engine()                                                          # the batch form's refusals
    sc, _ = K.case(5, "aligned")
    with pytest.raises(ValueError):
        e.interaction_step(sc["heat"], sc["plant"], sc["rows"], 0, cfg=dict(push=2.0))
    bad = sc["rows"].copy(); bad[0, 2] = 0.0
    with pytest.raises(lpvmpc.LpvMpcError):
        e.interaction_step(sc["heat"], sc["plant"], bad, 0)
    with pytest.raises(ValueError):
        e.interaction_step(np.zeros(300, int), np.zeros((300, 8)), np.tile(sc["rows"][0], (300, 1)), 0)   # a heat of more than 256
    e.close()


def test_grid_on_the_device_transform_and_the_fleet_interface():
    """grid() through the package's own transform equals the host transform's grid; RaceFleet(heats=, interactions=) attaches both."""
    import lpvmpc
    from lpvmpc import interactions as I
    from oracle import plant_ref as PR
    mp = lshape()
    tab = np.asarray(mp.PointAndTangent, float)
    dev, t0 = I.grid(mp, 7, GAP, STAGGER)
    host, _ = I.grid(mp, 7, GAP, STAGGER, position=lambda s, ey: PR.get_global_position(tab, s, ey))
    assert np.max(np.abs(dev - host)) <= 1e-11 and t0.tolist() == [-1] * 7
    plant0, prow, tyres = race_setup(mp)
    fleet = lpvmpc.RaceFleet(mp, plant0, laps=3, half_track0=1, plant_params=prow, tyre_params=tyres, kernel_variant=KV,
                             heats=dict(heat=HEAT, turns0=np.full(B, -1), **SMALL), interactions=CFG)
    fleet.run(5)
    io = fleet.interactions()
    assert io["draft_ticks"].max() == 5 and io["hit_ticks"].max() >= 1 and fleet.standings()["contact_ticks"].max() >= 1
    fleet.interact(detach=True)
    with pytest.raises(lpvmpc.LpvMpcError):
        fleet.interactions()
    fleet.interact()
    fleet.run(1)
    assert fleet.interactions()["draft_ticks"].max() == 1
    fleet.close()
    with pytest.raises(ValueError):
        lpvmpc.RaceFleet(mp, plant0, laps=3, half_track0=1, interactions=True)


def test_the_second_car_of_a_train_is_faster_in_the_draft():
    """Contact off, four cars gridded in a line 0.9 m apart: after 20 ticks the second car of the train has a larger vx than the same
    car in the same race with draft_gain = 0."""
    import lpvmpc
    from lpvmpc import interactions as I
    mp = lshape()
    p, _ = I.grid(mp, 6, 0.9, 0.0)
    plant0 = np.vstack([p[2:], p[2:]])
    prow = lpvmpc.plant_params(B, mu_sim=0.4)                                      # a drag worth drafting out of
    tyres = lpvmpc.tyre_params(B)
    vx = {}
    for gain in (0.0, 0.8):
        path, tt, plan = start(mp, plant0, prow, tyres, inter=dict(draft_gain=gain, contact=0))
        o = run(path, 20)[-1]
        io = path.race_interactions_read()
        assert np.all(io["leader"][[1, 2, 3]] == [0, 1, 2]) and io["leader"][0] == -1 and not io["hit_ticks"].any()
        vx[gain] = o["plant"][:, 2].copy()
        close(path, tt, plan)
    print("vx after 20 ticks, draft_gain 0 / 0.8:", vx[0.0][:4], vx[0.8][:4])
    assert vx[0.8][1] > vx[0.0][1] + 1e-4 and same(vx[0.8][0], vx[0.0][0])     # the leader has nobody's wake
