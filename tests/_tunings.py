"""Shared by tests/test_tunings_host.py and tests/test_gpu_tunings.py: the tuning rows, the batches and the per-row oracle of the
per-vehicle tunings (include/lpvmpc.h, "Per-vehicle tunings").

BATCHES: the ctrl8, ctrl13 (run-time horizon), ctrl20, ctrl20d3 (DPP kernel, pinned-steering rows), plan20, plan30 and plan40
workloads of tests/test_gpu_settings.py, 67-71 instances each: the smallest shapes that reach every kernel family.

rows4(name): four rows interleaved over a batch (instance b gets row b mod 4) --
  0  the handle's own row (lpvmpc_tuning_from_config of the configuration the workload's engine is created from);
  1  controller: the other reference tuning (CTRL_TUNINGS["path"]; the workloads run "race") with the handle's limits;
     planner: the handle's weights with the boxes PLAN_BOXES of tests/test_gpu_settings.py;
  2  the handle's weights with CTRL_LIMITS / PLAN_BOXES of tests/test_gpu_settings.py (test_limits: the oracle answers these limits
     on these batches);
  3  a sampled row: the diagonals of Q and R, dR and L_cf each x U[0.7, 1.3]; controller delta_max x U[0.6, 1], a_max x U[0.2, 1],
     a_min_abs x U[0.5, 1]; planner epsi box, max_vel and the input boxes x U[0.55, 1].  Seeded by SEED and the batch's position.
The oracle takes weights from the workload dict, max_vel / min_vel from ``params`` and the limits from ``limits=``: the per-row
oracle is tick_batch_qp per row group (oracle_rows), as tests/_model_params.py does for model rows."""
import numpy as np

from oracle import osqp_ref as O

NAMES = ("ctrl8", "ctrl13", "ctrl20", "ctrl20d3", "plan20", "plan30", "plan40")
SEED = 9100
NTHREADS = 16
W = 64

_W, _ROWS, _ORC = {}, {}, {}


def batch(name):
    """(kind, workload dict) of one of NAMES, built once."""
    if name not in _W:
        from tests.test_gpu_settings import WORKLOADS
        kind, make = WORKLOADS[name]
        _W[name] = (kind, make())
    return _W[name]


def delay_of(w):
    return int(np.asarray(w["u_old"]).reshape(w["x0"].shape[0], -1).shape[1] - 2) if w["kind"] == "controller" else 0


def config_of(w, **kw):
    """The lpvmpc_config of the engine a workload runs on (host only); kw: other constructor arguments."""
    from lpvmpc.api import build_config
    args = dict(Q=w["Q"], R=w["R"], dR=w["dR"], L_cf=w["L_cf"], track=w["track"], steering_delay=delay_of(w))
    args.update(kw)
    return build_config(w["kind"], w["N"], w["dt"], **args)


class HostEngine(object):
    """What tuning.tuning_rows needs of an engine -- kind and cfg -- without a handle."""

    def __init__(self, w, **kw):
        self.cfg = config_of(w, **kw)
        self.kind = self.cfg.kind


def rows4(name):
    """[4, 64]: the four rows of a batch (module docstring)."""
    if name in _ROWS:
        return _ROWS[name]
    from lpvmpc import tuning
    from lpvmpc.workloads import CTRL_TUNINGS
    from tests.test_gpu_settings import CTRL_LIMITS, PLAN_BOXES
    kind, w = batch(name)
    eng = HostEngine(w)
    own = tuning.tuning_rows(1, eng)[0]
    rng = np.random.default_rng([SEED, NAMES.index(name)])
    f = tuning.fields(kind)
    s = own.copy()
    for k in ("Q", "R"):
        o, shp = f[k]
        n = shp[0]
        s[[o + j * (n + 1) for j in range(n)]] *= rng.uniform(0.7, 1.3, n)
    s[f["dR"][0]:f["dR"][0] + 2] *= rng.uniform(0.7, 1.3, 2)
    if kind == "controller":
        Qp, Rp, dRp = CTRL_TUNINGS["path"]
        r1 = tuning.tuning_rows(1, eng, Q=Qp, R=Rp, dR=dRp)[0]
        r2 = tuning.tuning_rows(1, eng, **CTRL_LIMITS)[0]
        s[f["delta_max"][0]] *= rng.uniform(0.6, 1.0)
        s[f["a_max"][0]] *= rng.uniform(0.2, 1.0)
        s[f["a_min_abs"][0]] *= rng.uniform(0.5, 1.0)
    else:
        r1 = tuning.tuning_rows(1, eng, **PLAN_BOXES)[0]
        r2 = r1.copy()
        s[f["L_cf"][0]:f["L_cf"][0] + 5] *= rng.uniform(0.7, 1.3, 5)
        s[f["xmin"][0] + 4] *= rng.uniform(0.55, 1.0)
        s[f["xmax"][0] + 4] *= rng.uniform(0.55, 1.0)
        s[f["xmax"][0]] *= rng.uniform(0.55, 1.0)
        s[f["umin"][0]:f["umin"][0] + 2] *= rng.uniform(0.55, 1.0, 2)
        s[f["umax"][0]:f["umax"][0] + 2] *= rng.uniform(0.55, 1.0, 2)
    _ROWS[name] = tuning.check_tuning_rows(np.stack([own, r1, r2, s]), 4, kind)
    return _ROWS[name]


def interleaved(B, rows, shift=0):
    """[B, 64]: instance b gets row (b + shift) mod len(rows)."""
    return np.ascontiguousarray(rows[(np.arange(B) + shift) % len(rows)])


def sub_batch(w, idx):
    B = w["x0"].shape[0]
    return {k: (v[idx] if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == B and k != "track" else v) for k, v in w.items()}


def oracle_args(kind, row):
    """A row as the oracle takes it: (weights to put in the workload dict, params, limits)."""
    from lpvmpc import tuning
    d = tuning.split_row(kind, row)
    wt = dict(Q=d["Q"], R=d["R"], dR=d["dR"])
    if kind == "controller":
        return dict(wt, L_cf=None), dict(max_vel=d["max_vel"]), {k: d[k] for k in ("vx_min", "delta_max", "a_max", "a_min_abs")}
    return (dict(wt, L_cf=d["L_cf"]), dict(min_vel=float(d["xmin"][0]), max_vel=float(d["xmax"][0])),
            dict(xmin=d["xmin"], xmax=d["xmax"], umin=d["umin"], umax=d["umax"]))


def groups(rows):
    """[(row, indices)] of the distinct rows of a [B, 64] table, in order of first appearance."""
    out, seen = [], {}
    for b, r in enumerate(map(bytes, np.ascontiguousarray(rows))):
        if r not in seen:
            seen[r] = len(out)
            out.append((np.array(rows[b]), []))
        out[seen[r]][1].append(b)
    return [(r, np.array(i)) for r, i in out]


def group_case(w, kind, idx, row):
    """(workload, params, limits) of the sub-batch idx as a handle created with ``row`` sees it."""
    wt, params, limits = oracle_args(kind, row)
    return dict(sub_batch(w, idx), **wt), params, limits


def oracle_rows(w, kind, rows):
    """tick_batch_qp with each instance's own row: run per row group and reassembled."""
    B = w["x0"].shape[0]
    out = {}
    for row, idx in groups(rows):
        g, params, limits = group_case(w, kind, idx, row)
        r = O.tick_batch_qp(g, kind, params=params, limits=limits, nthreads=NTHREADS)
        for k, v in r.items():
            if k not in out:
                out[k] = np.full((B,) + v.shape[1:], np.nan if v.dtype.kind == "f" else 0, v.dtype)
            out[k][idx] = v
    return out


def oracle(name, which="interleaved"):
    """The oracle of a batch with its interleaved rows, or with row 0 on every instance ("nominal"); computed once."""
    if (name, which) not in _ORC:
        kind, w = batch(name)
        B = w["x0"].shape[0]
        rows = interleaved(B, rows4(name)) if which == "interleaved" else interleaved(B, rows4(name)[:1])
        _ORC[(name, which)] = oracle_rows(w, kind, rows)
    return _ORC[(name, which)]


def check_interleaved(name, out):
    """check_batch of a device result of batch ``name`` under its interleaved rows against oracle(name), group by group."""
    from tests import _tolerance as T
    kind, w = batch(name)
    B = w["x0"].shape[0]
    ref = oracle(name)
    total = {}
    for row, idx in groups(interleaved(B, rows4(name))):
        g, params, limits = group_case(w, kind, idx, row)
        sub = lambda d: {k: v[idx] for k, v in d.items() if isinstance(v, np.ndarray) and v.shape[:1] == (B,)}
        c = T.check_batch(g, kind, sub(out), sub(ref), params=params, limits=limits)
        for k, v in c.items():
            total[k] = total.get(k, 0) + v
    return total


def plain_engine(w, row, **settings):
    """The plain handle of a row: BatchedSolver created with the row's weights and limits."""
    import lpvmpc
    from lpvmpc import tuning
    kw = tuning.engine_kwargs(w["kind"], row)
    d = delay_of(w)
    if d:
        kw["steering_delay"] = d
    kw.update(settings)
    return lpvmpc.BatchedSolver(w["kind"], w["N"], w["dt"], track=w["track"], **kw)


def solve(eng, w):
    return eng.solve(w["x0"], w["u_prev"], w["vel_ref"], w["curv_s"], w["u_old"], w["max_ey"], w["cf_new"], w["lap"])
