"""GPU: the contact model (lpvmpc_race_contact / _read, lpvmpc_contact_step_batch; BatchedSolver.race_contact / race_contact_read /
contact_step, RaceFleet.contact / contacts) against the numpy restatement tests/_contact_ref.py: crafted single ticks in heats of 1, 2,
5, 65 and 256 members with a third heat of T-bones, a corner into a side, an offset nose-to-tail hit, a rubbing pair and a pile-up;
the equalities with the interactions alone; a scripted sequence with both carries passed back in; a race against the host replay;
attach orders, refusals and lifetime; and two physical checks.  Decisions, counters and who was written are held exactly, values to
1e-11 relative to max(1, |value|), and word for word for every vehicle whose own and whose partners' headings are exactly 0.
(Measured: the crafted ticks within 4.4e-16 of the restatement, 589 vehicles word for word at 256 members; the race within 7.2e-15 in
states and commands and 2.5e-14 in the planes over 30 ticks.)"""
import ctypes as C_

import numpy as np
import pytest

from tests import _contact_cases as C
from tests import _contact_ref as CR
from tests import _interactions_ref as R
from tests.test_gpu_interactions import B, CFG, HEAT, SMALL, batch_engine, close, lshape, race_setup, races_equal, run, same, start

pytestmark = pytest.mark.gpu

TOL = 1e-11


def err_of(a, b, what):
    a, b = np.asarray(a, float), np.asarray(b, float)
    assert np.array_equal(np.isnan(a), np.isnan(b)), what
    ok = ~np.isnan(a)
    return float(np.max(np.abs(a[ok] - b[ok]) / np.maximum(1.0, np.abs(b[ok])))) if ok.any() else 0.0


def compare(res, sc, ref, exact):
    """A device tick against the restatement's: decisions, counters and who was written exactly; values to TOL, and word for word for
    the vehicles exact [B] marks."""
    from lpvmpc import _ffi
    plant, mu, out, carry, cout, ccarry = res
    for k in R.I32_NAMES:
        assert np.array_equal(out[k], ref[k]), k
    for k in CR.I32_NAMES:
        assert np.array_equal(cout[k], ref[k]), k
    assert same(plant[~ref["written"]], sc["plant"][~ref["written"]])       # untouched vehicles keep their rows bit for bit
    assert same(plant[:, [4, 5, 6]], sc["plant"][:, [4, 5, 6]])              # ax, ay, yaw are nobody's to write
    assert same(mu[~ref["part"]], sc["rows"][~ref["part"], 6])
    member = sc["heat"] >= 0
    values = [("plant", plant, ref["plant"]), ("mu_live", mu, ref["mu_live"])]
    values += [(k, out[k], ref[k]) for k in R.F64_NAMES] + [(k, cout[k], ref[k]) for k in CR.F64_NAMES]
    values += [("carried impulse_total", np.where(member, carry["f64"][0], np.nan), np.where(member, ref["carry"]["impulse_total"], np.nan)),
               ("carried yaw_kick_total", np.where(member, ccarry["f64"][0], np.nan), np.where(member, ref["ccarry"]["yaw_kick_total"], np.nan))]
    worst = 0.0
    for what, got, want in values:
        e = err_of(got, want, what)
        assert e <= TOL, (what, e)
        worst = max(worst, e)
        assert same(np.asarray(got)[exact], np.asarray(want, float)[exact]), what
    for c, k in enumerate(_ffi.INTER_CARRY_I32_NAMES):
        assert np.array_equal(carry["i32"][c][member], ref["carry"][k][member]), k
    assert np.array_equal(ccarry["i32"][0][member], ref["ccarry"]["max_partners"][member])
    return worst


@pytest.mark.parametrize("kind", ("general", "aligned"))
@pytest.mark.parametrize("n", C.SIZES)
def test_one_tick_of_crafted_geometry(n, kind):
    """The interactions' scene of two co-located heats of n members (pile-up, nose-to-tail, side by side, the frozen and the pose-less
    member, the drafting train) and three loose vehicles, plus the third heat of the corner form's kinds.  "aligned": the frame's
    heading is exactly 0, and every vehicle without a turned car in reach is held word for word."""
    sc, ref = C.case(n, kind)
    e = batch_engine()
    res = e.contact_step(sc["heat"], sc["plant"], sc["rows"], 5, nstep=sc["nstep"])
    e.close()
    exact = C.exact_vehicles(sc) if kind == "aligned" else np.zeros(len(sc["heat"]), bool)
    worst = compare(res, sc, ref, exact)
    cout = res[4]
    print("contact tick, heats of %d, %s: margin %.3g, clip margin %.3g, %d hit, worst relative error %.3g, %d vehicles word for word" %
          (n, kind, ref["margin"], ref["clip_margin"], int(ref["hit"].sum()), worst, int(exact.sum())))
    for name, idx in sc["where"].items():
        assert np.all(cout["partners"][idx] == (2 if name == "pile" else 1)) and np.all(cout["yaw_kick"][idx] != 0), name
    assert not same(res[0][:, 7], sc["plant"][:, 7])                           # psiDot is written
    a, b = np.nonzero(sc["heat"] == 0)[0], np.nonzero(sc["heat"] == 1)[0]      # the two co-located heats read alike
    for k in ("friction_impulse", "yaw_kick", "partners"):
        assert same(cout[k][a], cout[k][b]), k
    loose = sc["heat"] < 0
    assert np.all(np.isnan(cout["f64"][:, loose])) and not cout["i32"][:, loose].any()


def test_without_friction_and_yaw_a_step_is_the_interactions_step():
    sc, _ = C.case(65, "general")
    e = batch_engine()
    plant, mu, out, carry = e.interaction_step(sc["heat"], sc["plant"], sc["rows"], 5, nstep=sc["nstep"])
    first = None
    for _ in range(2):                                                         # and a rerun is bit for bit
        res = e.contact_step(sc["heat"], sc["plant"], sc["rows"], 5, contact=dict(friction=0.0, yaw_response=0), nstep=sc["nstep"])
        assert same(res[0], plant) and same(res[1], mu) and same(res[2]["f64"], out["f64"]) and same(res[2]["i32"], out["i32"])
        assert same(res[3]["f64"], carry["f64"]) and same(res[3]["i32"], carry["i32"])
        assert not np.nansum(np.abs(res[4]["yaw_kick"])) and not np.nansum(res[4]["friction_impulse"]) and res[4]["partners"].sum() > 0
        full = e.contact_step(sc["heat"], sc["plant"], sc["rows"], 5, nstep=sc["nstep"])
        if first is not None:
            for x, y in zip(first[:2], full[:2]):
                assert same(x, y)
            for x, y in zip(first[2:], full[2:]):
                assert same(x["f64"], y["f64"]) and same(x["i32"], y["i32"])
        first = full
    e.close()
    assert not same(first[0], plant)


def test_both_carries_through_a_scripted_sequence():
    """12 ticks of 4 cars: two hits with lateral offsets of opposite sign; every counter exact on every tick, and the run split over two
    handles, both carries handed over, equals the one run."""
    rows = np.tile([0.125, 0.125, 1.98, 0.03, 60.0, 60.0, 0.05], (4, 1))
    e, e2 = batch_engine(), batch_engine()
    carry = ccarry = carry2 = ccarry2 = ref_carry = ref_ccarry = None
    kicks = []
    exact = np.ones(4, bool)
    for t in range(C.SCRIPT_TICKS):
        p = C.script(t)
        ref = C.checked(CR.tick(p, rows, C.SCRIPT_HEAT, R.config(), CR.config(), t=t, carry=ref_carry, ccarry=ref_ccarry), t)
        ref_carry, ref_ccarry = ref["carry"], ref["ccarry"]
        res = e.contact_step(C.SCRIPT_HEAT, p, rows, t, carry=carry, contact_carry=ccarry)
        carry, ccarry = res[3], res[5]
        compare(res, dict(plant=p, rows=rows, heat=C.SCRIPT_HEAT), ref, exact)
        if t == 5:
            carry2, ccarry2 = ({k: v.copy() for k, v in c.items()} for c in (carry, ccarry))
        if t > 5:
            res2 = e2.contact_step(C.SCRIPT_HEAT, p, rows, t, carry=carry2, contact_carry=ccarry2)
            carry2, ccarry2 = res2[3], res2[5]
            assert same(res2[0], res[0])
            for x, y in zip(res2[2:], res[2:]):
                assert same(x["f64"], y["f64"]) and same(x["i32"], y["i32"])
        kicks.append(float(res[4]["yaw_kick"][1]))
    close(e, e2)
    assert [k != 0 for k in kicks] == [False, False, False, True, True, True, False, False, True, True, False, False]
    assert kicks[3] * kicks[8] < 0
    assert res[4]["max_partners"].tolist() == [1, 1, 0, 0] and res[4]["yaw_kick_total"][1] > abs(kicks[8]) and np.isnan(res[4]["yaw_kick_total"][3])


# ---- in a race ---------------------------------------------------------------------------------------------------------------------
def start_contact(mp, plant0, prow, tyres, inter=CFG, contact=None):
    path, tt, plan = start(mp, plant0, prow, tyres, inter=inter)
    if contact is not None:
        path.race_contact(contact)
    return path, tt, plan


def test_race_with_the_contact_model_matches_the_host_replay():
    """The interactions' race of 8 vehicles in two heats from grid(), neighbours overlapping sideways at the start, with the contact
    model attached at tick 0: 30 lap-0 ticks against the host replay on tests/_contact_ref.py.  The tyre race's bar: states within 2e-6,
    equal statuses and iteration counts; the planes follow the replay's, decisions exactly.  The start is the interactions' own: on
    the replay every hard decision of the 30 ticks holds by 4e-5, every clip by 1e-4, and no contact interval is empty."""
    mp = lshape()
    plant0, prow, tyres = race_setup(mp)
    T_ = 30
    ref = CR.contact_race_ref()(np.asarray(mp.PointAndTangent, float), plant0, HEAT, R.config(**CFG), CR.config(), half_length=SMALL["half_length"],
                                half_width_car=SMALL["half_width"], tyre_params=tyres, plant_params=prow, half_track0=1, laps=3,
                                half_width=mp.halfWidth, slack=mp.slack)
    path, tt, plan = start_contact(mp, plant0, prow, tyres, contact={})
    worst = worst_out = 0.0
    hits = []
    for t in range(T_):
        path.race_tick(1); ref.tick()
        o, io, ko = path.race_read(), path.race_interactions_read(), path.race_contact_read()
        assert np.all(o["phase"] == 0) and np.all(ref.phase == 0), t
        for a_, b_ in ((o["plant"], ref.plant), (o["local"], ref.local), (o["cmd"], ref.cmd)):
            worst = max(worst, float(np.max(np.abs(a_ - b_))))
        assert np.array_equal(o["iters"], ref.iters) and np.array_equal(o["status"], ref.status), t
        for k in R.I32_NAMES:
            assert np.array_equal(io[k], ref.inter[k]), (t, k)
        for k in CR.I32_NAMES:
            assert np.array_equal(ko[k], ref.inter[k]), (t, k)
        for k in R.F64_NAMES:
            worst_out = max(worst_out, float(np.max(np.abs(io[k] - ref.inter[k]))))
        for k in CR.F64_NAMES:
            worst_out = max(worst_out, float(np.max(np.abs(ko[k] - ref.inter[k]))))
        hits.append(int(io["hit"].sum()))
    print("race with the contact model vs replay: %d ticks, worst state / command error %.3g, worst output error %.3g, hits per tick %s, "
          "smallest margins of the replay %.3g / %.3g" % (T_, worst, worst_out, hits, ref.margin, ref.clip_margin))
    assert ref.margin >= 1e-5 and ref.clip_margin >= 1e-5 and ref.empty == 0       # the replay alone, on the CPU
    assert worst <= 2e-6 and worst_out <= 2e-6
    assert min(hits) < hits[0] and hits[-1] > min(hits) and ko["yaw_kick_total"].min() > 0   # a hit ends and one starts; every car was turned
    close(path, tt, plan)


def test_equalities_reruns_and_the_detached_race():
    """friction = 0, yaw_response = 0 attached equals the interactions alone, plant words and planes; a rerun with the model on is bit
    for bit; a race that goes back to the centres form at tick 10 equals, from the same snapshot, one that never had the model."""
    mp = lshape()
    plant0, prow, tyres = race_setup(mp)
    n = 12
    path, tt, plan = start_contact(mp, plant0, prow, tyres)
    plain = run(path, n, extra=("race_interactions_read",))
    close(path, tt, plan)
    path, tt, plan = start_contact(mp, plant0, prow, tyres, contact=dict(friction=0.0, yaw_response=0))
    off = run(path, n, extra=("race_interactions_read",))
    assert path.race_contact_read()["max_partners"].max() >= 1
    close(path, tt, plan)
    races_equal(plain, off)
    for x, y in zip(plain, off):
        assert same(x["race_interactions_read"]["f64"], y["race_interactions_read"]["f64"])
        assert same(x["race_interactions_read"]["i32"], y["race_interactions_read"]["i32"])
    first = None
    for _ in range(2):
        path, tt, plan = start_contact(mp, plant0, prow, tyres, contact={})
        on = run(path, n, extra=("race_interactions_read", "race_contact_read"))
        close(path, tt, plan)
        if first is not None:
            races_equal(first, on)
            for x, y in zip(first, on):
                for name in ("race_interactions_read", "race_contact_read"):
                    assert same(x[name]["f64"], y[name]["f64"]) and same(x[name]["i32"], y[name]["i32"])
        first = on
    assert not same(first[-1]["plant"], plain[-1]["plant"])                     # and the corner form is another race
    # back to the centres form at tick 10 (no draft: the snapshot's live mu words are then the base words a new binding reads)
    nodraft = dict(draft_gain=0.0)
    path, tt, plan = start_contact(mp, plant0, prow, tyres, inter=nodraft, contact={})
    run(path, 10)
    path.race_contact(detach=True)
    with pytest.raises(Exception):
        path.race_contact_read()
    snap = path.race_snapshot()
    a = run(path, 8)
    close(path, tt, plan)
    path, tt, plan = start(mp, plant0, prow, tyres, heats=False)
    path.race_restore(snap)
    path.race_heats(HEAT, turns0=np.full(B, -1), **SMALL)
    path.race_interactions(nodraft)
    b = run(path, 8)
    close(path, tt, plan)
    races_equal(a, b)


def test_attach_orders_give_equal_races():
    """Disturbances, interactions, contact model and walls attached in three orders before the first tick: word-for-word equal races."""
    from lpvmpc import disturbance as D
    mp = lshape()
    plant0, prow, tyres = race_setup(mp)
    rows = D.disturbance_rows(B, patch0=(0.0, float(mp.TrackLength), 0.6))
    got = []
    for order in ("DICW", "WICD", "IDWC"):
        path, tt, plan = start(mp, plant0, prow, tyres)
        for s in order:
            {"D": lambda: path.set_disturbances(rows), "I": lambda: path.race_interactions(CFG), "C": lambda: path.race_contact(),
             "W": lambda: path.race_walls()}[s]()
        got.append(run(path, 6, extra=("race_contact_read", "race_walls_read")))
        close(path, tt, plan)
    for other in got[1:]:
        races_equal(got[0], other)
        for x, y in zip(got[0], other):
            for name in ("race_contact_read", "race_walls_read"):
                assert same(x[name]["f64"], y[name]["f64"]) and same(x[name]["i32"], y[name]["i32"])
    assert got[0][-1]["race_contact_read"]["max_partners"].max() >= 1


def test_refusals_and_lifetime():
    import lpvmpc
    from lpvmpc import _ffi
    mp = lshape()
    plant0, prow, tyres = race_setup(mp)
    e = batch_engine()
    assert e._lib.lpvmpc_race_contact(e._h, None) == -1 and e._lib.lpvmpc_race_contact_read(e._h, None, None) == -1   # no race
    with pytest.raises(lpvmpc.LpvMpcError):
        e.race_contact()
    e.close()
    path, tt, plan = start(mp, plant0, prow, tyres)
    with pytest.raises(lpvmpc.LpvMpcError, match="interactions"):
        path.race_contact()                                                     # no interactions
    with pytest.raises(lpvmpc.LpvMpcError):
        path.race_contact_read()                                                # nothing attached
    path.race_interactions(dict(contact=0))
    with pytest.raises(lpvmpc.LpvMpcError, match="contact = 0"):
        path.race_contact()
    path.race_interactions(CFG)
    path.race_contact()
    path.race_tick(3)
    before = path.race_contact_read()
    assert before["max_partners"].max() >= 1
    for word, v in (("friction", -0.1), ("friction", float("nan")), ("friction", float("inf")), ("yaw_response", 2), ("yaw_response", -1),
                    ("reserved", 1)):
        c = _ffi.default_contact_config()
        setattr(c, word, v)
        assert path._lib.lpvmpc_race_contact(path._h, C_.byref(c)) == -1, word  # LPVMPC_E_ARG, past the Python checks
    after = path.race_contact_read()
    assert same(before["f64"], after["f64"]) and same(before["i32"], after["i32"])   # a refused call leaves the binding as it was
    path.race_contact(dict(friction=0.5))                                      # attaching again: the counters start anew
    assert not path.race_contact_read()["max_partners"].any()
    path.race_tick(1)
    path.race_interactions(CFG)                                                 # re-attaching the interactions drops the contact model
    with pytest.raises(lpvmpc.LpvMpcError):
        path.race_contact_read()
    path.race_contact()
    path.race_interactions(detach=True)                                         # and so does detaching them
    with pytest.raises(lpvmpc.LpvMpcError):
        path.race_contact_read()
    path.race_interactions(CFG)
    path.race_contact()
    path.race_tick(1)
    path.race_heats(HEAT, turns0=np.full(B, -1), **SMALL)                       # and so do the heats
    with pytest.raises(lpvmpc.LpvMpcError):
        path.race_contact_read()
    with pytest.raises(lpvmpc.LpvMpcError):
        path.race_contact()
    path.race_tick(1)
    close(path, tt, plan)
    e = batch_engine()                                                          # the batch form's refusals
    sc, _ = C.case(5, "aligned")
    with pytest.raises(ValueError):
        e.contact_step(sc["heat"], sc["plant"], sc["rows"], 0, contact=dict(friction=-1.0))
    with pytest.raises(lpvmpc.LpvMpcError, match="contact = 0"):
        e.contact_step(sc["heat"], sc["plant"], sc["rows"], 0, cfg=dict(contact=0))
    bad = sc["rows"].copy(); bad[0, 3] = 0.0
    with pytest.raises(lpvmpc.LpvMpcError):
        e.contact_step(sc["heat"], sc["plant"], bad, 0)
    e.close()


def test_the_fleet_interface():
    import lpvmpc
    mp = lshape()
    plant0, prow, tyres = race_setup(mp)
    fleet = lpvmpc.RaceFleet(mp, plant0, laps=3, half_track0=1, plant_params=prow, tyre_params=tyres, kernel_variant=0,
                             heats=dict(heat=HEAT, turns0=np.full(B, -1), **SMALL), interactions=CFG, contact=True)
    fleet.run(3)
    assert fleet.contacts()["max_partners"].max() >= 1 and fleet.contacts()["yaw_kick_total"].max() > 0
    fleet.contact(detach=True)
    with pytest.raises(lpvmpc.LpvMpcError):
        fleet.contacts()
    fleet.contact(dict(friction=0.1))
    fleet.run(1)
    fleet.close()
    with pytest.raises(ValueError):
        lpvmpc.RaceFleet(mp, plant0, laps=3, half_track0=1, plant_params=prow, tyre_params=tyres, heats=dict(heat=HEAT), contact=True)


@pytest.mark.parametrize("kind", ("tbone", "rear_corner"))
def test_a_struck_car_is_spun_only_with_the_contact_model(kind):
    """Two _tyres races from one start: a T-bone ahead of the struck car's centre, and a nose clipping a rear corner.  With the contact
    model the struck car's yaw kick of the first tick is positive (both hits turn it to the left), its psiDot after the tick is not
    zero and is another word than the centres form's race gives; in the batch form on the same start, where no simulator step follows,
    the centres form leaves psiDot the word it was.  (Measured: yaw kick 3.54 / 0.33, psiDot after the tick 3.25 / 0.061 with the
    model, -0.002 / 0.030 without.)"""
    import lpvmpc
    from lpvmpc import interactions as I
    mp = lshape()
    p, _ = I.grid(mp, 7, 0.9, 0.0)
    hl, hw = SMALL["half_length"], SMALL["half_width"]
    plant0 = np.vstack([p[3:], p[3:]])
    x, y, th = plant0[1, 0], plant0[1, 1], plant0[1, 6]                          # the struck car: member 1 of heat 0
    c, s = np.cos(th), np.sin(th)
    if kind == "tbone":
        lx, ly, dth, vx = 0.08, -(hw + hl) + 0.03, 1.45, 1.5                     # from the right, ahead of the centre
    else:
        lx, ly, dth, vx = -(2 * hl) + 0.03, -0.15, 0.0, 1.6                      # from behind, on the right rear corner
    plant0[0] = [x + c * lx - s * ly, y + s * lx + c * ly, vx, 0.0, 0.0, 0.0, th + dth, 0.0]
    prow, tyres = lpvmpc.plant_params(B), lpvmpc.tyre_params(B)
    psi = {}
    for model in (False, True):
        path, tt, plan = start_contact(mp, plant0, prow, tyres, contact={} if model else None)
        path.race_tick(1)
        o, io = path.race_read(), path.race_interactions_read()
        assert io["hit"][:2].tolist() == [1, 1] and not io["hit"][2:].any()
        psi[model] = float(o["plant"][1, 7])
        if model:
            kick = float(path.race_contact_read()["yaw_kick"][1])
        close(path, tt, plan)
    print("%s: yaw kick %.3g, psiDot after the tick %.3g with the model, %.3g without" % (kind, kick, psi[True], psi[False]))
    assert abs(psi[True]) > 0 and psi[True] != psi[False]                       # (the tick's simulator steps follow the kick and damp it)
    assert kick > 0                                                              # hit on the right ahead of the centre, or pushed forward on the right rear corner: turned left
    e = batch_engine()
    heat = np.array([0, 0] + [-1] * (B - 2))
    plain = e.interaction_step(heat, plant0, prow, 0, **SMALL)[0]
    model = e.contact_step(heat, plant0, prow, 0, **SMALL)[0]
    e.close()
    assert same(plain[:, 7], plant0[:, 7]) and not same(plain[:2, :4], plant0[:2, :4])
    assert model[1, 7] != 0.0 and same(model[2:], plant0[2:])
