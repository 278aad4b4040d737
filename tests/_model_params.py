"""Shared by tests/test_model_params_host.py and tests/test_gpu_model_params.py: the model rows, the batches and the oracle of
the per-vehicle model parameters (include/lpvmpc.h, "Per-vehicle model parameters").

ROWS: four rows interleaved over a batch (vehicle b gets row b mod 4) -- the nominal words of a handle; the asymmetric car of
tests/golden/params.npz; two rows sampled around the nominal one with lf, lr +-10 %, m, Iz +-15 %, Cf, Cr +-30 %, mu x [0.5, 1.5]
(model.sample_model_params, seeds SEEDS).  The seeds were picked with the oracle alone, on the CPU, so that it answers every
instance of BATCHES with these rows (tests/test_model_params_host.py asserts it): of seeds 1 .. 12, seeds 3, 11 and 12 leave no
roll-out outside the track table; the first two are taken.

BATCHES: the ctrl8, ctrl20, plan30 and plan40 workloads of tests/test_gpu_settings.py (lap 1: curvature given), and the two
controller workloads again on lap 0 (curvature from the map at the rolled-out s, every third instance wrapping at the lap end), at
vx >= 1.2: below 1.04 the forward-Euler yaw mode is unstable and a lap-0 roll-out runs s below 0 (tests/test_gpu_horizons.py
ctrl_workload), which the nominal car does on one instance of the N = 20 batch at vx >= 0.8.  The planner has no lap argument."""
import numpy as np

from oracle import lpv_ref as L, osqp_ref as O

WORDS = ("lf", "lr", "m", "Iz", "Cf", "Cr", "mu")
SPREAD = dict(lf=0.10, lr=0.10, m=0.15, Iz=0.15, Cf=0.30, Cr=0.30, mu=0.50)
SEEDS = (3, 11)
NTHREADS = 16


def rows4():
    from lpvmpc import model
    from tests.test_gpu_settings import vehicle
    veh = vehicle()
    nominal = model.model_params(1)[0]
    assert np.array_equal(nominal, [L.DEFAULT_PARAMS[k] for k in WORDS])
    return np.stack([nominal, [veh[k] for k in WORDS]] + [model.sample_model_params(1, s, SPREAD)[0] for s in SEEDS])


def interleaved(B, rows=None, shift=0):
    """[B, 7]: vehicle b gets row (b + shift) mod 4."""
    rows = rows4() if rows is None else rows
    return np.ascontiguousarray(rows[(np.arange(B) + shift) % len(rows)])


def batches():
    from tests.test_gpu_horizons import ctrl_workload
    from tests.test_gpu_settings import WORKLOADS
    out = {k: (WORKLOADS[k][0], WORKLOADS[k][1]()) for k in ("ctrl8", "ctrl20", "plan30", "plan40")}
    out["ctrl8_lap0"] = ("controller", ctrl_workload(71, 8, seed=8111, lap=0, vmin=1.2))
    out["ctrl20_lap0"] = ("controller", ctrl_workload(71, 20, seed=8114, lap=0, vmin=1.2))
    return out


def params_of(row):
    return {k: float(v) for k, v in zip(WORDS, row)}


def sub_batch(w, idx):
    """The instances idx of a workload dict."""
    B = w["x0"].shape[0]
    return {k: (v[idx] if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == B and k != "track" else v) for k, v in w.items()}


def group_workload(w, kind, idx, row):
    """The sub-batch idx as a handle created with ``row`` sees it: the controller roll-out of a bound handle takes the row's Cf for
    both axles, which on a per-handle path is the call's cf_new."""
    g = sub_batch(w, idx)
    return dict(g, cf_new=float(row[4])) if kind == "controller" else g


def groups(model_rows):
    """[(row, indices)] of the distinct rows of a [B, 7] table, in order of first appearance."""
    out, seen = [], {}
    for b, r in enumerate(map(tuple, model_rows)):
        if r not in seen:
            seen[r] = len(out)
            out.append((np.array(r), []))
        out[seen[r]][1].append(b)
    return [(r, np.array(i)) for r, i in out]


def oracle_rows(w, kind, model_rows):
    """tick_batch_qp with each vehicle's own row: run per row group (params = the row, cf_new = its Cf) and reassembled."""
    B = w["x0"].shape[0]
    out = {}
    for row, idx in groups(model_rows):
        r = O.tick_batch_qp(group_workload(w, kind, idx, row), kind, params=params_of(row), nthreads=NTHREADS)
        for k, v in r.items():
            if k not in out:
                out[k] = np.full((B,) + v.shape[1:], np.nan if v.dtype.kind == "f" else 0, v.dtype)
            out[k][idx] = v
    return out
