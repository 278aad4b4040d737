"""CPU: per-vehicle model parameters (include/lpvmpc.h, "Per-vehicle model parameters").  The C ABI declares and exports the two
new calls; the Python helpers build, broadcast, sample and check rows; the oracle alone answers every instance of the batches of
tests/test_gpu_model_params.py with the rows of tests/_model_params.py and tells a rotation of the rows apart; the per-vehicle
kernels live in a translation unit of their own and the per-handle kernels' unit does not name them."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import _model_params as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "autonomous-racing-lpv-mpp-mpc_amd", "csrc")
NEW = ("lpvmpc_set_model_params", "lpvmpc_model_params_read")
NOM = [0.125, 0.125, 1.98, 0.03, 60.0, 60.0, 0.05]


def test_new_calls_are_declared_and_exported():
    """The check of tests/test_cabi.py::test_every_declared_symbol_is_exported, for the two new names: declared in lpvmpc.h and
    exported by the built library."""
    from lpvmpc import _ffi
    h = open(os.path.join(ROOT, "include", "lpvmpc.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    lib = _ffi.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, h), name
        assert name in _ffi.EXPORTS, name
        assert hasattr(lib, name), "liblpvmpc.so does not export %s" % name
    assert re.search(r"#define\s+LPVMPC_MODEL_WORDS\s+7\b", h) and _ffi.MODEL_WORDS == 7
    assert re.search(r"#define\s+LPVMPC_VERSION\s+200\b", h)
    # argument checks that need no device: a NULL handle is refused
    assert lib.lpvmpc_set_model_params(None, 0, None) == _ffi.E_ARG
    assert lib.lpvmpc_model_params_read(None, C.byref(C.c_int32(0)), None) == _ffi.E_ARG


def test_helpers_build_the_engines_rows_and_broadcast():
    import lpvmpc
    r = lpvmpc.model_params(3)
    assert r.shape == (3, 7) and np.array_equal(r, np.tile(NOM, (3, 1)))

    class _Eng(object):                                  # an engine's config: all seven words are read (the model is the engine's)
        class cfg(object):
            lf, lr, m, Iz, Cf, Cr, mu = 0.14, 0.11, 2.3, 0.04, 65.0, 52.0, 0.07
    r = lpvmpc.model_params(2, _Eng(), Cr=[50.0, 70.0], m=2.0)
    assert np.array_equal(r, [[0.14, 0.11, 2.0, 0.04, 65.0, 50.0, 0.07], [0.14, 0.11, 2.0, 0.04, 65.0, 70.0, 0.07]])
    with pytest.raises(ValueError):
        lpvmpc.model_params(3, m=[1.0, 2.0])
    with pytest.raises(TypeError):
        lpvmpc.model_params(3, Cq=1.0)
    with pytest.raises(ValueError):
        lpvmpc.model_params(0)


def test_samples_are_seeded_sliceable_and_within_spread():
    import lpvmpc
    a = lpvmpc.sample_model_params(64, 11)
    assert np.array_equal(a, lpvmpc.sample_model_params(64, 11)) and not np.array_equal(a, lpvmpc.sample_model_params(64, 12))
    assert np.array_equal(a[40:], lpvmpc.sample_model_params(24, 11, offset=40))
    f = a / lpvmpc.model_params(64)
    assert np.array_equal(f[:, :2], np.ones((64, 2)))                                  # lf, lr not in the default spread
    for i, s in ((2, 0.15), (3, 0.15), (4, 0.30), (5, 0.30), (6, 0.50)):
        assert np.all(np.abs(f[:, i] - 1) <= s + 1e-12) and np.std(f[:, i]) > s / 4, i
    assert not np.array_equal(a, lpvmpc.sample_plant_params(64, 11))                   # a model error is independent of the plant's draw
    b = lpvmpc.sample_model_params(8, 11, spread=M.SPREAD)
    assert np.all(np.abs(b[:, :2] / 0.125 - 1) <= 0.10 + 1e-12) and np.all(b[:, 0] != 0.125)
    with pytest.raises(ValueError):
        lpvmpc.sample_model_params(8, 1, spread=dict(m=1.5))
    with pytest.raises(TypeError):
        lpvmpc.sample_model_params(8, 1, spread=dict(mass=0.1))


def test_bad_rows_are_refused_before_the_library_naming_vehicle_and_field():
    from lpvmpc import model
    good = model.model_params(4)
    for a in (good[:3], good[:, :6], good.reshape(-1), np.zeros((4, 7, 1))):
        with pytest.raises(ValueError):
            model.check_model_params(a, 4)
    for (b, i, v) in ((0, 0, np.nan), (1, 3, np.inf), (2, 2, 0.0), (3, 1, -0.1), (0, 4, -1.0), (1, 6, -1e-9), (2, 5, -3.0)):
        x = good.copy(); x[b, i] = v
        with pytest.raises(ValueError) as e:
            model.check_model_params(x, 4)
        assert "model_params" in str(e.value) and "vehicle %d" % b in str(e.value) and M.WORDS[i] in str(e.value), str(e.value)
    x = good.copy(); x[:, 4:] = 0.0
    assert np.array_equal(model.check_model_params(x, 4), x)                          # Cf = Cr = mu = 0 are allowed
    with pytest.raises(ValueError):
        model.check_model_params(np.array([["a"] * 7] * 4), 4)


def test_rows_are_the_four_of_the_issue():
    r = M.rows4()
    from tests.test_gpu_settings import vehicle
    veh = vehicle()
    assert r.shape == (4, 7) and np.array_equal(r[0], NOM) and np.array_equal(r[1], [veh[k] for k in M.WORDS])
    f = r[2:] / r[0]
    for i, k in enumerate(M.WORDS):
        assert np.all(np.abs(f[:, i] - 1) <= M.SPREAD[k] + 1e-12) and np.all(f[:, i] != 1.0), k
    t = M.interleaved(10)
    assert all(np.array_equal(t[b], r[b % 4]) for b in range(10))
    assert [len(i) for _, i in M.groups(t)] == [3, 3, 2, 2]


def test_the_oracle_answers_every_instance_and_tells_a_rotation_apart():
    """What lets tests/test_gpu_model_params.py see every instance and catch an indexing error.  check_batch leaves out the
    instances the oracle does not answer (tick_batch_qp status -10: a roll-out that leaves the track table).  Per (batch, row): at
    most the share that the asymmetric car leaves unanswered on that batch as a handle's vehicle, and never more than 2 %.  With
    the rows rotated by one vehicle the oracle's uPred differs by more than 1e-3 on every batch."""
    from oracle import osqp_ref as O
    from tests.test_gpu_settings import vehicle
    for name, (kind, w) in M.batches().items():
        B = w["x0"].shape[0]
        rows = M.interleaved(B)
        a = M.oracle_rows(w, kind, rows)
        asym = float(np.mean(O.tick_batch_qp(w, kind, params=vehicle(), nthreads=M.NTHREADS)["status"] == -10))
        shares = [float(np.mean(a["status"][idx] == -10)) for _, idx in M.groups(rows)]
        b = M.oracle_rows(w, kind, M.interleaved(B, shift=1))
        ok = np.isfinite(a["uPred"]).all(axis=(1, 2)) & np.isfinite(b["uPred"]).all(axis=(1, 2))
        d = float(np.max(np.abs(a["uPred"][ok] - b["uPred"][ok])))
        print("%s: unanswered per row %s (asymmetric car as the handle's vehicle: %.3f), statuses %s; rows rotated: max |du| %.3e on %d instances"
              % (name, shares, asym, dict(zip(*np.unique(a["status"], return_counts=True))), d, int(ok.sum())))
        assert all(s <= min(asym, 0.02) for s in shares), (name, shares, asym)
        assert ok.sum() >= B // 2 and d > 1e-3, (name, d)


def _source(fname):
    s = open(os.path.join(CSRC, fname)).read()
    return re.sub(r"//.*", "", re.sub(r"/\*.*?\*/", "", s, flags=re.S))


def test_per_vehicle_kernels_have_their_own_translation_unit():
    """The per-handle kernels' object must compile to the code it has alone: lpv_eval.hip defines no per-vehicle kernel and launches
    them through veh_lpv_eval.hip's launchers only; the new unit defines the five per-vehicle forms, is built with contraction off
    like lpv_eval.o and passes the resource gate."""
    old, new = _source("lpv_eval.hip"), _source("veh_lpv_eval.hip")
    kern = lambda s: set(re.findall(r"__global__[^;{]*?\b(\w+_kernel)\s*\(", s))
    assert kern(old) == {"ctrl_lpv_kernel", "ctrl_lpv_pre_kernel", "ctrl_lpv_roll_kernel", "ctrl_abc_kernel", "plan_lpv_kernel", "plan_abc_kernel"}
    five = {"ctrl_lpv_veh_kernel", "ctrl_lpv_pre_veh_kernel", "ctrl_abc_veh_kernel", "plan_lpv_veh_kernel", "plan_abc_veh_kernel"}
    assert kern(new) == five
    assert "VehModel" not in old and "load_model" not in old
    mk = open(os.path.join(CSRC, "Makefile")).read()
    rule = re.search(r"^veh_lpv_eval\.o:.*\n\t(.*)$", mk, flags=re.M).group(1)
    assert "-ffp-contract=off" in rule and "$(RESCHK)" in rule and all(k in rule for k in five)
    # both objects are linked into the library and into the stamps build, which take the one list, and the host object has a rule
    objs = re.search(r"^OBJS\s*:=((?:.*\\\n)*.*)$", mk, flags=re.M).group(1).replace("\\\n", " ").split()
    assert "veh_lpv_eval.o" in objs and "model_params_api.o" in objs
    assert re.search(r"^\$\(OUT\): \$\(OBJS\)\n\t.* -o \$@ \$\(OBJS\)$", mk, flags=re.M)
    assert "STAMPOBJS := $(OBJS:admm_solve.o=admm_solve_stamps.o)" in mk and re.search(r"^\t.* -o \$@ \$\(STAMPOBJS\)$", mk, flags=re.M)
    assert "HOSTOBJS := $(filter %_api.o fleet_launch.o,$(OBJS))" in mk and re.search(r"^\$\(HOSTOBJS\): %\.o: %\.hip\b", mk, flags=re.M)
