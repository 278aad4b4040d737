"""GPU: the rules that the four race attachments share -- the heats, the interactions, the contact model and the walls -- asserted once
for all of them: the refusals without a race and with nothing attached, a refused configuration that leaves what is attached as it was,
the detach chain heats -> interactions -> contact model (the walls stand alone), the batch forms' refusals and trivial cases, and one
tick of each batch form against the attached form's first tick, word for word.  What each layer computes is held by its own file
(test_gpu_heats.py, test_gpu_interactions.py, test_gpu_contact.py, test_gpu_walls.py).  The race is the smallest with every case: three
vehicles started with plant parameters, vehicles 0 and 1 in one heat and in contact, vehicle 2 in no heat and aimed at a wall."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_walls import batch_engine, close, same, start

pytestmark = pytest.mark.gpu

B = 3
HEAT = np.array([0, 0, -1], np.int32)
LAYERS = ("heats", "interactions", "contact", "walls")
ATTACH = dict(heats="lpvmpc_race_heats", interactions="lpvmpc_race_interactions", contact="lpvmpc_race_contact", walls="lpvmpc_race_walls")
READ = dict(heats="lpvmpc_race_standings", interactions="lpvmpc_race_interactions_read", contact="lpvmpc_race_contact_read",
            walls="lpvmpc_race_walls_read")


def setup():
    """(map, plant0 [3, 8], plant rows, tyre rows, L): vehicle 0 half a car's length behind vehicle 1 and faster, aimed at the left wall;
    vehicle 2 further on, in no heat, a front corner in the right wall (which stands margin = 0.25 outside the half width 0.3)."""
    import lpvmpc
    from oracle import plant_ref as PR
    mp = lpvmpc.Map("L_shape", 0.2)
    tab = np.asarray(mp.PointAndTangent, float)
    plant0 = np.zeros((B, 8))
    for b, (s, ey, vx, dyaw) in enumerate(((1.2, 0.12, 1.6, 0.4), (1.7, 0.05, 1.0, 0.0), (5.0, -0.25, 1.4, -0.4))):
        x, y, th = PR.get_global_position(tab, s, ey)
        plant0[b] = [x, y, vx, 0.0, 0.0, 0.0, th + dyaw, 0.0]
    return mp, plant0, lpvmpc.sample_plant_params(B, 23), lpvmpc.tyre_params(B), float(tab[-1, 3] + tab[-1, 4])


def attach(path, layers=LAYERS):
    for k in layers:                                                            # (in the order of their dependencies)
        dict(heats=lambda: path.race_heats(HEAT), interactions=path.race_interactions, contact=path.race_contact, walls=path.race_walls)[k]()


def read(path, layer):
    """The layer's planes (f64, i32) as the library returns them."""
    o = dict(heats=path.race_standings, interactions=path.race_interactions_read, contact=path.race_contact_read, walls=path.race_walls_read)[layer]()
    return o["f64"], o["i32"]


def last_error(e):
    return e._lib.lpvmpc_last_error(e._h).decode()


def raw_read(e, layer):
    """The read entry point with NULL destinations: (return code, error text)."""
    args = (None,) * (4 if layer == "heats" else 2)
    return getattr(e._lib, READ[layer])(e._h, *args), last_error(e)


def raw_attach(e, layer, bad=False):
    """The attach entry point past the Python checks, with the defaults or with a configuration it refuses: (return code, error text)."""
    from lpvmpc import _ffi
    nan = float("nan")
    if layer == "heats":
        heat = np.array([0, -2 if bad else 0, -1], np.int32)
        cfg = _ffi.HeatsConfig(0.4, 0.2)
        rc = e._lib.lpvmpc_race_heats(e._h, C.byref(cfg), heat.ctypes.data_as(C.c_void_p), None)
        return rc, last_error(e)
    cfg = dict(interactions=_ffi.default_interaction_config, contact=_ffi.default_contact_config, walls=_ffi.default_wall_config)[layer]()
    if bad:
        setattr(cfg, dict(interactions="draft_gain", contact="friction", walls="margin")[layer], nan)
    return getattr(e._lib, ATTACH[layer])(e._h, C.byref(cfg)), last_error(e)


def not_attached(path, layer):
    from lpvmpc import _ffi
    rc, text = raw_read(path, layer)
    return rc == _ffi.E_ARG and ATTACH[layer] + ")" in text and "attached" in text


@pytest.mark.parametrize("layer", LAYERS)
def test_no_race_on_the_handle(layer):
    from lpvmpc import _ffi
    e = batch_engine()
    for rc, text in (raw_attach(e, layer), raw_read(e, layer)):
        assert rc == _ffi.E_ARG and "call lpvmpc_race_init first" in text, (layer, rc, text)
    e.close()


@pytest.fixture(scope="module")
def bare_race():
    """The race with nothing attached, for the cases that leave it so: (path handle, plant0, plant rows, L)."""
    mp, plant0, prow, tyres, L = setup()
    path, tt, plan = start(mp, plant0, prow, tyres)
    yield path, plant0, prow, L
    close(path, tt, plan)


@pytest.mark.parametrize("layer", LAYERS)
def test_nothing_attached(bare_race, layer):
    assert not_attached(bare_race[0], layer), (layer, raw_read(bare_race[0], layer))


def test_a_refused_configuration_leaves_every_binding_as_it_was():
    """Each layer in turn is attached again with a configuration the library refuses (a non-finite word; for the heats an index below
    -1): the planes of all four read back bit for bit, so the refusal came before the layer's readers were detached, and the race
    ticks on."""
    from lpvmpc import _ffi
    mp, plant0, prow, tyres, _ = setup()
    path, tt, plan = start(mp, plant0, prow, tyres)
    attach(path)
    path.race_tick(1)
    before = {k: read(path, k) for k in LAYERS}
    assert np.isfinite(before["heats"][0][:, :2]).any()                         # (the tick wrote the members' standings)
    for layer in LAYERS:
        rc, text = raw_attach(path, layer, bad=True)
        assert rc == _ffi.E_ARG and ATTACH[layer] in text, (layer, rc, text)
        for k in LAYERS:
            f, i = read(path, k)
            assert same(f, before[k][0]) and same(i, before[k][1]), (layer, k)
    path.race_tick(1)
    assert path.race_read()["ticks"] == 2
    close(path, tt, plan)


def test_the_detach_chain():
    """Detaching the heats detaches the interactions and the contact model, detaching the interactions the contact model; the walls are
    nobody's reader; and with the interactions gone the live mu words are the started rows' again."""
    mp, plant0, prow, tyres, _ = setup()
    path, tt, plan = start(mp, plant0, prow, tyres)
    attach(path)
    path.race_tick(1)
    walls = read(path, "walls")
    path.race_heats(None)
    assert all(not_attached(path, k) for k in ("heats", "interactions", "contact"))
    assert same(read(path, "walls")[0], walls[0]) and same(read(path, "walls")[1], walls[1])
    assert same(path.plant_params_read(), prow)
    attach(path, ("heats", "interactions", "contact"))
    path.race_tick(1)
    walls, standings = read(path, "walls"), read(path, "heats")
    path.race_interactions(detach=True)
    assert not_attached(path, "interactions") and not_attached(path, "contact")
    for k, was in (("walls", walls), ("heats", standings)):
        assert same(read(path, k)[0], was[0]) and same(read(path, k)[1], was[1]), k
    assert same(path.plant_params_read()[:, 6], prow[:, 6])                     # read from the live table once nothing is attached
    path.race_tick(1)
    close(path, tt, plan)


def step(e, layer, plant, prow, L=None, rec=None, phase0=None, t=0, hw=0.3):
    """One tick of the layer's batch form through the Python interface, from a fresh carry: its output planes [(f64, i32), ...]."""
    from lpvmpc import heats as H
    if layer == "heats":
        pose = np.stack([rec["x"][0], rec["y"][0], rec["yaw"][0]], axis=1)
        out, _ = e.heat_step(HEAT, L, pose, rec["track_s"][0], rec["inside"][0], rec["phase"][0], t, carry=H.new_carry(B, phase0=phase0))
        return [(out["f64"], out["i32"])]
    if layer == "interactions":
        return [tuple(e.interaction_step(HEAT, plant, prow, t)[2][k] for k in ("f64", "i32"))]
    if layer == "contact":
        res = e.contact_step(HEAT, plant, prow, t)
        return [(res[2]["f64"], res[2]["i32"]), (res[4]["f64"], res[4]["i32"])]
    return [tuple(e.wall_step(plant, prow, t, half_width=hw)[1][k] for k in ("f64", "i32"))]


@pytest.mark.parametrize("layer", LAYERS)
def test_batch_form_on_the_race_s_own_handle(bare_race, layer):
    import lpvmpc
    path, plant0, prow, L = bare_race
    rec = dict(x=plant0[None, :, 0], y=plant0[None, :, 1], yaw=plant0[None, :, 6], track_s=np.zeros((1, B)), inside=np.ones((1, B), np.int32),
               phase=np.zeros((1, B), np.int32))
    with pytest.raises(lpvmpc.LpvMpcError, match="use another handle") as err:
        step(path, layer, plant0, prow, L=L, rec=rec)
    assert err.value.code == lpvmpc._ffi.E_ARG


def raw_step(e, layer, n, null=None):
    """The layer's batch entry point on arrays for 3 vehicles filled with a sentinel, for n vehicles, argument ``null`` (an index
    into the pointer arguments) NULL: (return code, True if no array changed)."""
    from lpvmpc import _ffi
    mp, plant0, prow, _, L = setup()
    f = lambda *shape: np.full(shape, -7.25)
    i = lambda *shape: np.full(shape, -7, np.int32)
    hc, ic, kc, wc = _ffi.HeatsConfig(0.4, 0.2), _ffi.default_interaction_config(), _ffi.default_contact_config(), _ffi.default_wall_config()
    planes = lambda M: [f(getattr(_ffi, M + "_CARRY_F64"), B), i(getattr(_ffi, M + "_CARRY_I32"), B), f(getattr(_ffi, M + "_F64"), B),
                        i(getattr(_ffi, M + "_I32"), B)]
    if layer == "heats":
        arrays = [HEAT.copy(), f(B), f(B, 3), f(B), i(B), i(B)] + planes("HEAT")
        call = lambda p: e._lib.lpvmpc_heat_step_batch(e._h, n, 1, p[0], p[1], C.byref(hc), 0, *p[2:])
    elif layer == "interactions":
        ci = planes("INTER")
        arrays = [HEAT.copy(), f(B, 8), prow.copy(), ci[0], ci[1], f(B), ci[2], ci[3]]
        call = lambda p: e._lib.lpvmpc_interaction_step_batch(e._h, n, 1, p[0], C.byref(hc), C.byref(ic), 0, p[1], p[2], None, *p[3:])
    elif layer == "contact":
        ci, ck = planes("INTER"), planes("CONTACT")
        arrays = [HEAT.copy(), f(B, 8), prow.copy(), ci[0], ci[1], ck[0], ck[1], f(B), ci[2], ci[3], ck[2], ck[3]]
        call = lambda p: e._lib.lpvmpc_contact_step_batch(e._h, n, 1, p[0], C.byref(hc), C.byref(ic), C.byref(kc), 0, p[1], p[2], None, *p[3:])
    else:
        arrays = [f(B, 8), prow.copy()] + planes("WALL")
        call = lambda p: e._lib.lpvmpc_wall_step_batch(e._h, n, C.byref(wc), 0.3, 0, p[0], p[1], None, *p[2:])
    was = [a.copy() for a in arrays]
    ptrs = [a.ctypes.data_as(C.c_void_p) for a in arrays]
    if null is not None:
        ptrs[null] = None
    rc = call(ptrs)
    return rc, all(same(a, b) for a, b in zip(arrays, was))


@pytest.mark.parametrize("layer", LAYERS)
def test_batch_form_trivial_cases(layer):
    """B = 0 is LPVMPC_OK and writes nothing; a NULL where an array is required is LPVMPC_E_ARG and writes nothing either."""
    from lpvmpc import _ffi
    e = batch_engine()
    assert raw_step(e, layer, 0) == (0, True)
    for null in (1, -1, -3):                                                    # three of the required pointers, inputs and outputs
        assert raw_step(e, layer, B, null=null) == (_ffi.E_ARG, True), (layer, null, last_error(e))
    e.close()


def test_batch_form_against_attached_form():
    """One tick of each batch form from a fresh carry on the plant state the race holds before its first tick equals, word for word,
    the planes the attached form reads after that tick.  The heats run behind the plant's step and locate the vehicles themselves, so
    their batch form takes the pose, s, inside and phase that the race's recorder wrote on that tick (the same words: the recorder
    locates the same plant rows with the same function), and the phases before the tick as the carry's."""
    mp, plant0, prow, tyres, L = setup()
    e = batch_engine(mp)
    for layers in (("heats", "interactions", "walls"), ("heats", "interactions", "contact")):   # (the contact model's tick replaces the interactions')
        path, tt, plan = start(mp, plant0, prow, tyres)
        path.race_record(1, 1)
        attach(path, layers)
        first = path.race_read()
        assert same(first["plant"], plant0)
        path.race_tick(1)
        rec = path.race_record_read(last=1)
        assert rec["tick"][0] == 0
        for layer in layers:
            if layer == "interactions" and "contact" in layers:
                continue                                                        # (compared below, as the contact form wrote them)
            got = step(e, layer, plant0, prow, L=L, rec=rec, phase0=first["phase"], hw=mp.halfWidth)
            want = [read(path, layer)] if layer != "contact" else [read(path, "interactions"), read(path, "contact")]
            for (gf, gi), (wf, wi) in zip(got, want):
                assert same(gf, wf) and same(gi, wi), (layer, gf, wf, gi, wi)
            if layer == "heats":
                assert np.isfinite(wf[0, :2]).all() and np.isnan(wf[:, 2]).all() and wi[0, 2] == -1   # members placed, vehicle 2 in no heat
            if layer == "walls":
                assert wi[0, 2] == 1 and wf[0, 2] > 0                           # vehicle 2 is in the wall: the planes are not the blank ones
        close(path, tt, plan)
    e.close()
