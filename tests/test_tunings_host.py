"""CPU: the per-vehicle tunings' host side (include/lpvmpc.h, "Per-vehicle tunings") -- the row helpers of tuning.py, the two
host-only entry points against the rows lpvmpc_create writes into the device configuration, the assembled QP of a row against
the oracle's, and the conditions the GPU tests of tests/test_gpu_tunings.py stand on: with the rows of tests/_tunings.py the
oracle answers every instance of every batch, and every non-nominal row moves its answer."""
import numpy as np
import pytest

from oracle import lpv_ref as L, osqp_ref as O
from tests import _tunings as TU


def _eng(kind, **kw):
    from lpvmpc import workloads as W
    if kind == "controller":
        Q, R, dR = W.CTRL_TUNINGS["race"]
        w = dict(kind=kind, N=20, dt=1 / 30.0, Q=Q, R=R, dR=dR, L_cf=None, track=None, x0=np.zeros((1, 6)), u_old=np.zeros((1, 2)))
    else:
        w = dict(kind=kind, N=30, dt=0.05, Q=W.PLAN_Q, R=W.PLAN_R, dR=W.PLAN_dR, L_cf=W.PLAN_L, track=None, x0=np.zeros((1, 5)), u_old=np.zeros((1, 2)))
    return TU.HostEngine(w, **kw)


# ---- tuning.py ------------------------------------------------------------------------------------------------------------------
def test_rows_shapes_and_overrides():
    from lpvmpc import tuning, workloads as W
    c, p = _eng("controller"), _eng("planner")
    r = tuning.tuning_rows(5, c)
    assert r.shape == (5, 64) and r.dtype == np.float64 and r.flags.c_contiguous
    Q, R, dR = W.CTRL_TUNINGS["race"]
    assert np.array_equal(r[3, :36], Q.reshape(-1)) and np.array_equal(r[3, 36:40], R.reshape(-1)) and np.array_equal(r[3, 40:42], dR)
    assert np.array_equal(r[0, 48:53], [0.01, 5.0, 0.249, 4.0, 1.0]) and not r[:, 42:48].any() and not r[:, 53:].any()
    dm = np.linspace(0.15, 0.249, 5)
    Qb = np.stack([Q * (1 + 0.1 * b) for b in range(5)])
    r = tuning.tuning_rows(5, c, delta_max=dm, a_max=2.0, Q=Qb, dR=[1.0, 2.0])
    assert np.array_equal(r[:, 50], dm) and np.all(r[:, 51] == 2.0) and np.array_equal(r[:, :36], Qb.reshape(5, 36)) and np.all(r[:, 40:42] == [1.0, 2.0])
    r = tuning.tuning_rows(3, p)
    assert np.array_equal(r[1, :25], W.PLAN_Q.reshape(-1)) and not r[:, 25:36].any() and np.array_equal(r[1, 42:47], W.PLAN_L) and r[1, 47] == 0
    assert np.array_equal(r[2, 48:62], [0.9, -1, -2, r[2, 51], -0.8, 5.0, 1, 2, r[2, 56], 0.8, -0.249, -0.7, 0.249, 2.0])
    r = tuning.tuning_rows(3, p, xmax=[4.0, 1, 2, 0.3, 0.5], umin=np.array([[-0.1, -0.5]] * 3), L_cf=np.arange(5.0))
    assert np.all(r[:, 53] == 4.0) and np.all(r[:, 57] == 0.5) and np.all(r[:, 58:60] == [-0.1, -0.5]) and np.array_equal(r[0, 42:47], np.arange(5.0))
    d = tuning.split_row("planner", r[0])
    assert d["Q"].shape == (5, 5) and np.array_equal(d["xmax"], [4.0, 1, 2, 0.3, 0.5])
    # a handle with other limits: its own row carries them
    r = tuning.tuning_rows(1, _eng("controller", ctrl_delta_max=0.2, params=dict(max_vel=3.0)))
    assert r[0, 49] == 3.0 and r[0, 50] == 0.2


def test_rows_errors():
    from lpvmpc import tuning
    c, p = _eng("controller"), _eng("planner")
    with pytest.raises(TypeError, match="unknown tuning field.*L_cf"):
        tuning.tuning_rows(2, c, L_cf=np.zeros(5))
    with pytest.raises(TypeError, match="unknown tuning field.*delta_max"):
        tuning.tuning_rows(2, p, delta_max=0.2)
    with pytest.raises(ValueError, match="Q must have shape"):
        tuning.tuning_rows(2, c, Q=np.eye(5))
    with pytest.raises(ValueError, match="a_max must have shape"):
        tuning.tuning_rows(2, c, a_max=np.ones(3))
    with pytest.raises(ValueError, match="B must be >= 1"):
        tuning.tuning_rows(0, c)
    r = tuning.tuning_rows(4, c)
    for word, val, msg in ((7, np.nan, "instance 2: a non-finite word of Q"), (37, np.inf, "non-finite word of R"), (50, np.nan, "a NaN limit"),
                           (48, 6.0, "vx_min > max_vel"), (50, -0.1, "delta_max < 0"), (51, -2.0, "a_max < -a_min_abs")):
        bad = r.copy(); bad[2, word] = val
        with pytest.raises(ValueError, match=msg):
            tuning.check_tuning_rows(bad, 4, "controller")
    ok = r.copy(); ok[1, 51] = np.inf; ok[1, 45] = np.nan; ok[1, 60] = np.nan        # an infinite limit; ignored words
    tuning.check_tuning_rows(ok, 4, "controller")
    r = tuning.tuning_rows(4, p)
    for word, val, msg in ((44, np.nan, "non-finite word of L_cf"), (49, 2.0, "xmin > xmax"), (58, 0.3, "umin > umax"), (57, np.nan, "a NaN limit")):
        bad = r.copy(); bad[3, word] = val
        with pytest.raises(ValueError, match="instance 3: .*" + msg):
            tuning.check_tuning_rows(bad, 4, "planner")
    ok = r.copy(); ok[0, 51] = 1.0; ok[0, 56] = -1.0; ok[0, 30] = np.nan               # the ey slots and the words behind Q are ignored
    tuning.check_tuning_rows(ok, 4, "planner")
    with pytest.raises(ValueError, match=r"expected \(5, 64\)"):
        tuning.check_tuning_rows(r, 5, "planner")
    with pytest.raises(ValueError, match="spread of Q"):
        tuning.sample_tunings(4, 1, dict(Q=1.5), c)
    with pytest.raises(TypeError, match="unknown tuning field"):
        tuning.sample_tunings(4, 1, dict(xmin=0.1), c)


def test_sampling_is_seeded_by_global_vehicle_index():
    from lpvmpc import tuning
    for eng, spread in ((_eng("controller"), dict(Q=0.3, dR=0.2, delta_max=0.3)), (_eng("planner"), dict(L_cf=0.3, R=0.1, umax=0.2)), (_eng("controller"), None)):
        whole = tuning.sample_tunings(40, 7, spread, eng)
        assert np.array_equal(tuning.sample_tunings(15, 7, spread, eng, offset=25), whole[25:])
        assert np.array_equal(tuning.sample_tunings(25, 7, spread, eng), whole[:25])
        assert not np.array_equal(tuning.sample_tunings(40, 8, spread, eng), whole)
        own = tuning.tuning_rows(1, eng)[0]
        ratio = whole[:, own != 0] / own[own != 0]
        named = tuning.DEFAULT_SPREAD if spread is None else spread
        assert ratio.min() >= 1 - max(named.values()) - 1e-12 and ratio.max() <= 1 + max(named.values()) + 1e-12
        assert np.array_equal(whole[:, own == 0], np.zeros((40, int((own == 0).sum()))))      # off-diagonal entries stay zero
        f = tuning.fields(eng.kind)
        touched = np.zeros(64, bool)
        for k in named:
            if k in f:
                o, shp = f[k]
                touched[o:o + int(np.prod(shp, dtype=int))] = True
        assert np.array_equal(whole[:, ~touched], np.tile(own[~touched], (40, 1)))
        assert np.unique(whole, axis=0).shape[0] == 40


# ---- the two host-only entry points -----------------------------------------------------------------------------------------------
def _devcfg_block(cfg):
    """The words Q R dR Lcf box_lo[8] box_hi[8] of the device configuration, restated from lpvmpc_create."""
    out = np.zeros(64)
    out[:36] = cfg.Q[:]; out[36:40] = cfg.R[:]; out[40:42] = cfg.dR[:]; out[42:48] = cfg.L_cf[:]
    lo, hi = out[48:56], out[56:64]
    if cfg.kind == 0:
        lo[:6] = -np.inf
        hi[:6] = [-cfg.ctrl_vx_min, cfg.max_vel, cfg.ctrl_delta_max, cfg.ctrl_delta_max, cfg.ctrl_a_max, cfg.ctrl_a_min_abs]
    else:
        lo[:5] = cfg.plan_xmin[:]; hi[:5] = cfg.plan_xmax[:]
        lo[0], hi[0] = cfg.min_vel, cfg.max_vel
        lo[5:7] = cfg.plan_umin[:]; hi[5:7] = cfg.plan_umax[:]
    return out


@pytest.mark.parametrize("kind,kw", [("controller", {}), ("controller", dict(ctrl_vx_min=1.0, ctrl_delta_max=0.2, ctrl_a_max=0.7, ctrl_a_min_abs=0.6, params=dict(max_vel=3.5))),
                                     ("planner", {}), ("planner", dict(plan_xmin=[0.9, -0.05, -1.2, -0.2, -0.3], plan_xmax=[5.0, 0.04, 1.0, 0.2, 0.25],
                                                                       plan_umin=[-0.2, -0.5], plan_umax=[0.18, 1.5], params=dict(min_vel=0.5, max_vel=4.0)))])
def test_device_row_of_a_configuration_is_its_device_block(kind, kw):
    from lpvmpc import _ffi, tuning
    assert _ffi.KIND_CONTROLLER == 0
    eng = _eng(kind, **kw)
    row = tuning.config_row(eng.cfg)
    dev = tuning.device_row(kind, row)
    want = _devcfg_block(eng.cfg)
    assert dev.tobytes() == want.tobytes(), np.nonzero(dev != want)[0]
    # a row's ignored words reach the device row's weights as they are and its limits not at all
    r2 = row.copy(); r2[62] = 7.0; r2[47] = 3.0
    d2 = tuning.device_row(kind, r2)
    assert d2[47] == 3.0 and np.array_equal(d2[48:], dev[48:])
    assert tuning.engine_kwargs(kind, row)["Q"].shape == ((6, 6) if kind == "controller" else (5, 5))


def test_plain_engine_arguments_rebuild_the_row():
    """tuning.engine_kwargs(row) -- the constructor arguments of the plain handle of a row -- give back the row (the words the
    kind reads), so the GPU tests' plain handles solve with the rows they are compared under."""
    from lpvmpc import tuning
    for name in TU.NAMES:
        kind, w = TU.batch(name)
        for row in TU.rows4(name):
            kw = tuning.engine_kwargs(kind, row)
            back = tuning.config_row(TU.config_of(w, **kw))
            used = np.ones(64, bool)
            used[[51, 56]] = kind != "planner"
            assert np.array_equal(back[used], row[used]), (name, np.nonzero(back != row)[0])


# ---- the assembled QP of a row ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ctrl8", "ctrl20d3", "plan20"])
def test_qp_matrices_with_a_rows_words_is_the_oracles_qp(name):
    from lpvmpc import qp_matrices, tuning
    kind, w = TU.batch(name)
    N = int(w["N"])
    for r, row in enumerate(TU.rows4(name)):
        d = tuning.split_row(kind, row)
        g, params, limits = TU.group_case(w, kind, np.arange(3) * 5 + r, row)
        p = dict(L.DEFAULT_PARAMS, **params)
        for j in range(3):
            qp = O.instance_qp(g, kind, j, params, limits)
            if kind == "controller":
                _, A, Bm = L.ctrl_lpv_prediction(p, g["dt"], N, g["track"], g["x0"][j], g["u_prev"][j], g["vel_ref"][j], g["curv_s"][j], g["cf_new"], g["lap"])
                uo = np.asarray(g["u_old"][j]).reshape(-1)
                m = qp_matrices.controller_qp(d["Q"], d["R"], d["dR"], N, A, Bm, np.zeros((N, 6, 1)), g["x0"][j], uo[:2], g["vel_ref"][j], d["max_vel"],
                                              steer_hist=tuple(uo[2:]), bounds={k: d[k] for k in ("vx_min", "delta_max", "a_max", "a_min_abs")})
            else:
                _, A, Bm = L.plan_lpv_prediction(p, g["dt"], N, g["track"], g["x0"][j], g["curv_s"][j], g["u_prev"][j])
                mey = float(g["max_ey"][j])
                xlo, xhi = d["xmin"].copy(), d["xmax"].copy()
                xlo[3], xhi[3] = -mey, mey
                m = qp_matrices.planner_qp(d["Q"], d["R"], d["dR"], d["L_cf"], N, A, Bm, np.zeros((N, 5, 1)), g["x0"][j], g["u_old"][j], mey, xlo[0], xhi[0],
                                           xbox=(xlo, xhi), ubox=(d["umin"], d["umax"]))
            dense = lambda a: np.asarray(a.todense() if hasattr(a, "todense") else a, float)
            for k, want in (("P", qp.P), ("q", qp.q), ("A", qp.A), ("l", qp.l), ("u", qp.u)):
                got, want = dense(m[k]), dense(want)
                assert got.shape == want.shape, (name, r, j, k)
                both = np.isfinite(got) & np.isfinite(want)
                assert np.array_equal(np.isfinite(got) | (np.abs(got) >= 1e20), np.isfinite(want) | (np.abs(want) >= 1e20))
                e = float(np.max(np.abs(np.clip(got, -1e20, 1e20) - np.clip(want, -1e20, 1e20))[both], initial=0.0))
                assert e <= 1e-12 * max(1.0, float(np.max(np.abs(np.clip(want, -1e20, 1e20))))), (name, r, j, k, e)


# ---- the conditions the GPU tests stand on ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TU.NAMES)
def test_the_oracle_answers_every_instance_and_every_row_moves_it(name):
    """No instance of a batch under its interleaved rows is without an answer (status -10); each non-nominal row moves the
    oracle's uPred by at least 1e-2 on some instance that has a solution under both rows, or changes its statuses."""
    kind, w = TU.batch(name)
    B = w["x0"].shape[0]
    mixed, nominal = TU.oracle(name), TU.oracle(name, "nominal")
    assert not np.any(mixed["status"] == -10) and not np.any(nominal["status"] == -10), (name, np.nonzero(mixed["status"] == -10)[0])
    rows = TU.interleaved(B, TU.rows4(name))
    seen = 0
    for g, (row, idx) in enumerate(TU.groups(rows)):
        if g == 0:
            assert np.array_equal(mixed["uPred"][idx], nominal["uPred"][idx], equal_nan=True) and np.array_equal(mixed["iters"][idx], nominal["iters"][idx])
            continue
        seen += 1
        ok = np.isfinite(mixed["uPred"][idx]).all(axis=(1, 2)) & np.isfinite(nominal["uPred"][idx]).all(axis=(1, 2))
        d = float(np.max(np.abs(mixed["uPred"][idx][ok] - nominal["uPred"][idx][ok]), initial=0.0))
        n_it = int(np.sum(mixed["iters"][idx] != nominal["iters"][idx]))
        print("%s row %d: max |du| against the nominal row %.3e, %d of %d iteration counts differ, statuses %s" %
              (name, g, d, n_it, len(idx), dict(zip(*map(list, np.unique(mixed["status"][idx], return_counts=True))))))
        assert d >= 1e-2, (name, g, d)
    assert seen == (3 if kind == "controller" else 2)          # (the planner's rows 1 and 2 are one row)


# ---- the tuned host replay -------------------------------------------------------------------------------------------------------
def test_tuned_race_ref_with_nominal_weights_is_race_ref():
    import lpvmpc
    from lpvmpc import workloads as W
    from tests._race_ref import RaceRef
    from tests._tuned_race_ref import TunedRaceRef
    mp = lpvmpc.Map("L_shape", 0.2)
    B = 3
    rng = np.random.default_rng(9200)
    plant0 = np.zeros((B, 8)); plant0[:, 1] = rng.normal(0, 0.03, B); plant0[:, 2] = rng.uniform(0.8, 1.2, B); plant0[:, 6] = rng.normal(0, 0.03, B)
    kw = dict(laps=1, half_width=mp.halfWidth, slack=mp.slack)
    a = RaceRef(mp.PointAndTangent, plant0, **kw)
    b = TunedRaceRef(mp.PointAndTangent, plant0, path_weights=[W.CTRL_TUNINGS["path"]] * B, tt_weights=[W.CTRL_TUNINGS["race"]] * B,
                     plan_weights=[(W.PLAN_Q, W.PLAN_R, W.PLAN_dR, W.PLAN_L)] * B, **kw)
    for t in range(14):
        a.tick(); b.tick()
        for k in ("plant", "cmd", "local", "iters", "status", "phase", "lap"):
            assert np.array_equal(getattr(a, k), getattr(b, k)), (t, k)
