#!/usr/bin/env python3
"""Generate tests/golden/estimator_vehicles/design.npz: scipy's per-vertex Kalman gains (lpvmpc.observer_vertex_gains, one
solve_continuous_are per vertex) for 40 vehicle rows -- the nominal row and 39 drawn uniformly within +-30 % of it -- on the two
limit tables of ../estimator/estimator.npz, with the default weights (set 1) and, for the first 8 rows, with a non-diagonal Qo
and Ro (set 2).  The device design (csrc/observer_design.hip) and its numpy restatement are measured against these.

Keys (float64): rows [40, 7], lim_ls / lim_hs [6, 2], L_ls / L_hs [40, 6, 5, 16], Qo2 [6, 6], Ro2 [5, 5],
L2_ls / L2_hs [8, 6, 5, 16].

Usage:  python tests/golden/estimator_vehicles/make_design_golden.py [out.npz]   (needs scipy; no GPU)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, ROOT)

N_ROWS, N_ROWS2, SPREAD, SEED = 40, 8, 0.30, 20261018


def build():
    from lpvmpc.observer import OBS_PARAMS, observer_vertex_gains
    est = np.load(os.path.join(os.path.dirname(HERE), "estimator", "estimator.npz"))
    lim_ls, lim_hs = est["lim_ls"], est["lim_hs"]
    nominal = np.array([OBS_PARAMS[k] for k in ("lf", "lr", "m", "I", "Cf", "Cr", "mu")])
    rng = np.random.default_rng(SEED)
    rows = nominal * (1.0 + rng.uniform(-SPREAD, SPREAD, size=(N_ROWS, 7)))
    rows[0] = nominal
    # symmetric positive definite, every off-diagonal word non-zero
    g = rng.uniform(-1.0, 1.0, size=(6, 6))
    Qo2 = np.eye(6) + 0.1 * (g @ g.T)
    g = rng.uniform(-1.0, 1.0, size=(5, 5))
    Ro2 = np.diag([0.1, 0.1, 0.01, 0.01, 0.01]) + 0.002 * (g @ g.T)
    out = dict(rows=rows, lim_ls=lim_ls, lim_hs=lim_hs, Qo2=Qo2, Ro2=Ro2)
    out["L_ls"] = np.array([observer_vertex_gains(lim_ls, params=r) for r in rows])
    out["L_hs"] = np.array([observer_vertex_gains(lim_hs, params=r) for r in rows])
    out["L2_ls"] = np.array([observer_vertex_gains(lim_ls, Qo2, Ro2, params=r) for r in rows[:N_ROWS2]])
    out["L2_hs"] = np.array([observer_vertex_gains(lim_hs, Qo2, Ro2, params=r) for r in rows[:N_ROWS2]])
    return out


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "design.npz")
    data = build()
    np.savez(path, **data)
    print("wrote %s:" % path, ", ".join("%s%s" % (k, list(v.shape)) for k, v in sorted(data.items())))


if __name__ == "__main__":
    main()
